// gemm_segments_kernels.hip -- libxsmm_hip_gemm_batch_reduce_segments and its ext / offsets siblings: batch-reduce products with a reduce count of their own per C block, one launch.
//
// Segment s sums the products a_list[r] * b_list[r], seg_ptr[s] <= r < seg_ptr[s + 1], into c_list[s] [ref: src/generator_gemm_reference_impl.c:490-498: the
// count and the two pointer lists are read per call].  A work item is (segment, C tile): item = segment * tiles + tile.  Every wave owns one item at a time and
// the waves grid-stride over the items in ascending order, as the grouped kernels do, so the segments a caller lists first start first.  The shape, the leading
// dimensions, beta, the layout bits and the tile edge are the same for every item and travel by value in the kernel arguments (a GemmGroupDesc whose operand
// and stride slots are unused): no table, nothing uploaded.  Per item a wave reads seg_ptr[s], seg_ptr[s + 1] and c_list[s], then walks the two lists; the
// item index is wave-uniform, so all of these are scalar loads, and the pointer pair of product r + 1 is requested before product r's MFMAs are issued
// (ListChain::fetch in gemm_group_tile.hpp).  A whole segment is ONE accumulator chain over (product, k) on one wave -- the reference's order; a long segment
// is never split.  A segment of count 0 stores beta * C (beta = 0: +0; beta = 1: C's own bits).  No LDS, no barrier, no scratch; C leaves through vector stores.
// Block pointers are only known to be element-aligned: 16- / 8-byte loads of B columns and 4-byte loads of VNNI A pairs are chosen per product by a
// wave-uniform test of the pointer, the element-wise loads remain for every other product.
//
// The four entries differ in two things only, and each is a policy of the one item loop (segments_items):
//   where a segment's blocks lie       ListSource: c_list[s] and a ListChain over a_list / b_list.  OffsetSource (libxsmm_hip_gemm_batch_reduce_segments_offsets):
//                                      OFFSET batch-reduce [ref: src/generator_gemm_reference_impl.c:509-513, :186-188], g.c + c_offs[s] and an OffsetChain -- the three
//                                      bases travel by value in the GemmGroupDesc's operand slots, the lists hold signed byte offsets, read with the scalar loads that
//                                      read the pointer lists, one 64-bit add per product.
//   where its epilogue pointers lie    none (NoEpilogue: every use of it in the tiles sits behind `if constexpr`), or the FusedEpilogue of the two ext entries
//                                      [ref: src/generator_gemm_reference_impl.c:294-372] -- column bias, ReLU (+ bitmask), sigmoid -- whose bias and mask blocks are
//                                      d_list[s] / mask_list[s] (GemmSegEpilogue) or d + d_offs[s] / mask + mask_offs[s] (GemmSegOffsEpilogue); without a bias list the one
//                                      `d` is shared.  The entries are wave-uniform and read like C's; the operators are wave-uniform runtime bits of the by-value
//                                      block next to the GemmGroupDesc.  A segment of count 0 stores the activation of its start value (the bias, bias + C) and its
//                                      mask.  The mask bytes leave through vector stores (acc_relu_mask: a whole byte when its 8 rows are valid, read-merge-write for
//                                      the byte that holds row m - 1).
// With offsets A and / or B may be transposed -- the backward passes of a block-sparse layer, dX = W^T dY and dW = dY X^T -- through the transposed load forms of
// the tiles.  The two transposes are template parameters of the kernels, four instances per class: as wave-uniform runtime bits that select the tile instance
// inside ONE kernel they cost 196 / 224 / 88 registers (f32 / bf16 / f64: a wave per SIMD less for f32, two less for f64), although no single form needs more
// than the ADDRESS kernels' 160 / 196 / 72 -- the register allocator does not keep the four bodies apart (DESIGN.md section 9.2 has the numbers).
// The two *_sliced entries (further down) let the CALLER cut a chain: pass 1 is the same item loop over (slice, tile) with the partials
// of a workspace as destinations, pass 2 adds a block's partials in ascending slice order.  The entries above never split a segment.
// The two ext *_sliced entries are the same two passes with the FusedEpilogue's operators applied to the blocks' sums in pass 2
// (gemm_segments_slice_reduce_fused_kernel); pass 1 is launched exactly as for the plain handles.
// 8-bit floats (classes 3 BF8 and 4 HF8): BF8 x BF8 -> f32 / BF8 and HF8 x HF8 -> f32 / HF8 through tile_fp8 (gemm_group_tile.hpp) in the
// plain ADDRESS, OFFSET and sliced kernels -- A VNNI-4, NN only, so the offsets kernels have the <0,0> instance alone; never fused.  Pass 2 stores an 8-bit C
// through the instances <3> / <4> of gemm_segments_slice_reduce_kernel.
// IEEE halves (class 5): F16 x F16 -> f32 / f16 through tile_bf16 with the f16 instructions (gemm_group_tile.hpp, H16) in EVERY kernel
// family bf16 has -- ADDRESS, OFFSET, fused, sliced.  The offsets kernels exist as <0,0> (NN) and <0,1> (NT) only: libxsmm_dispatch_brgemm returns no f16
// handle with TRANS_A, because the reference's F16 loop has no transposed A [ref: src/generator_gemm_reference_impl.c:2049], so TN / TT cannot be asked for.  The arithmetic is the reference's F16 loop, not bf16's: the chain runs from +0 and the
// start value (C, the bias, bias + C), rounded to a half, is added behind it.  So a segment of count 0 under beta = 1 stores f16(C) widened -- for an f32 C NOT
// C's own bits, unlike every other class -- and one slice per block is the unsliced call bit for bit for every beta and with a bias.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "internal.hpp"
#include "gemm_device.hpp"
#include "bf16_cvt.hpp"
#include "gemm_group_tile.hpp"

namespace xamd {

using namespace group_tile;

// A SOURCE says where the blocks of segment s lie: c(g, s) is its C block -- one scalar load -- and chain(g, r0, r1) the chain over its products (constructing
// a chain loads nothing).  ListSource reads three pointer lists, OffsetSource adds signed byte offsets to the three bases in g.a / g.b / g.c.
struct ListSource {
  const void* const* a_list; const void* const* b_list; void* const* c_list;
  __device__ __forceinline__ gptr c(const GemmGroupDesc&, unsigned long long s) const { return (gptr)list_entry((const void*)c_list, s); }
  __device__ __forceinline__ ListChain chain(const GemmGroupDesc& g, unsigned long long r0, unsigned long long r1) const {
    return ListChain{(const void*)(a_list + r0), (const void*)(b_list + r0), r1 - r0, g.a_vec4, g.b_vec16, g.b_vec8};
  }
};
// a_wide: bit 0 / 1: the rows of a transposed A are multiples of 16 / 8 bytes apart (OffsetChain::va16 / va8).  Wide is how the kernel holds it: `int` for a
// parameter of its own, `const int&` for a field of the by-value epilogue block, read where the chain is built.
template <typename Wide> struct OffsetSource {
  const long long* a_offs; const long long* b_offs; const long long* c_offs; Wide a_wide;
  __device__ __forceinline__ gptr c(const GemmGroupDesc& g, unsigned long long s) const { return (gptr)g.c + (long long)uniform_u64(((GM const unsigned long long*)c_offs)[s]); }
  __device__ __forceinline__ OffsetChain chain(const GemmGroupDesc& g, unsigned long long r0, unsigned long long r1) const {
    return OffsetChain{(gcptr)g.a, (gcptr)g.b, (const void*)(a_offs + r0), (const void*)(b_offs + r0), r1 - r0, g.a_vec4, g.b_vec16, g.b_vec8, a_wide & 1, (a_wide >> 1) & 1};
  }
};

// A SEGMENT EPILOGUE says where the FusedEpilogue pointers of segment s come from: nowhere (the plain kernels: NoEpilogue), d_list[s] / mask_list[s], or
// d + d_offs[s] / mask + mask_offs[s]; without a bias list the one `d` is shared by every segment.  The entries are wave-uniform and read like C's.
struct NoSegEpilogue {
  __device__ __forceinline__ NoEpilogue at(unsigned long long) const { return NoEpilogue(); }
};
struct ListSegEpilogue {
  const GemmSegEpilogue& ep;
  __device__ __forceinline__ FusedEpilogue at(unsigned long long s) const {
    FusedEpilogue e{(gcptr)ep.d, nullptr, ep.colbias, ep.act, ep.mask_ld};
    if (ep.colbias && ep.d_list) e.d = list_entry((const void*)ep.d_list, s);
    if (ep.act == 2) e.mask = (GM unsigned char*)list_entry((const void*)ep.mask_list, s);
    return e;
  }
};
struct OffsetSegEpilogue {
  const GemmSegOffsEpilogue& ep;
  __device__ __forceinline__ FusedEpilogue at(unsigned long long s) const {
    FusedEpilogue e{(gcptr)ep.d, nullptr, ep.colbias, ep.act, ep.mask_ld};
    if (ep.colbias && ep.d_offs) e.d += (long long)uniform_u64(((GM const unsigned long long*)ep.d_offs)[s]);
    if (ep.act == 2) e.mask = (GM unsigned char*)ep.mask + (long long)uniform_u64(((GM const unsigned long long*)ep.mask_offs)[s]);
    return e;
  }
};

// CLS: 0 f32, 1 bf16, 2 f64 (16 x 16 tiles only, no epilogue), 3 BF8, 4 HF8 (NN only, no epilogue; C f32 or the operands' type), 5 f16 (everything bf16
// takes; C f32 or f16).  The tile edge is a wave-uniform runtime value, the class and the transposes pick the instance.
template <int CLS, bool TA, bool TB, typename Chain, typename Epi>
__device__ __forceinline__ void segment_tile(const GemmGroupDesc& g, const Chain& ch, gptr c, int tm, int tn, unsigned int lane, const Epi& e) {
  if constexpr (CLS == 2) tile_f64<Chain, TA, TB>(g, ch, c, tm * 16, tn * 16, lane);
  else if constexpr (CLS == 5) {                   // IEEE halves: the bf16 tile with the f16 instructions and the f16 start rule
    if (g.tile == 32) tile_bf16<32, true, Chain, Epi, TA, TB, true>(g, ch, c, tm * 32, tn * 32, lane, e);
    else tile_bf16<16, true, Chain, Epi, TA, TB, true>(g, ch, c, tm * 16, tn * 16, lane, e);
  }
  else if constexpr (CLS >= 3) {
    static_assert(!TA && !TB && !Epi::fused, "8-bit float segments: NN, without operators");
    if (g.tile == 32) tile_fp8<32, true, CLS == 4, Chain>(g, ch, c, tm * 32, tn * 32, lane);
    else tile_fp8<16, true, CLS == 4, Chain>(g, ch, c, tm * 16, tn * 16, lane);
  }
  else if (g.tile == 32) {
    if constexpr (CLS == 1) tile_bf16<32, true, Chain, Epi, TA, TB>(g, ch, c, tm * 32, tn * 32, lane, e);
    else tile_f32<32, true, Chain, Epi, TA, TB>(g, ch, c, tm * 32, tn * 32, lane, e);
  } else {
    if constexpr (CLS == 1) tile_bf16<16, true, Chain, Epi, TA, TB>(g, ch, c, tm * 16, tn * 16, lane, e);
    else tile_f32<16, true, Chain, Epi, TA, TB>(g, ch, c, tm * 16, tn * 16, lane, e);
  }
}

// The item loop of every kernel but the two pass-2 families.  Per item, in this order: seg_ptr[s], seg_ptr[s + 1], C's address, the epilogue's entries, then the chain.
template <int CLS, bool TA, bool TB, typename Source, typename SegEpilogue>
__device__ __forceinline__ void segments_items(const GemmGroupDesc& g, const unsigned long long* seg_ptr, Source src, SegEpilogue sep, unsigned long long total) {
  const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned int lane = threadIdx.x & 63u;
  const unsigned long long step = (unsigned long long)gridDim.x * 4u;
  const unsigned int tiles = (unsigned int)(g.tiles_m * g.tiles_n);
  for (unsigned long long item = (unsigned long long)blockIdx.x * 4u + wave; item < total; item += step) {
    unsigned long long s = item; unsigned int t = 0;
    if (tiles != 1) { s = item / tiles; t = (unsigned int)(item - s * tiles); }
    const unsigned int tn = t / (unsigned int)g.tiles_m, tm = t - tn * (unsigned int)g.tiles_m;
    const unsigned long long r0 = uniform_u64(((GM const unsigned long long*)seg_ptr)[s]), r1 = uniform_u64(((GM const unsigned long long*)seg_ptr)[s + 1]);
    gptr c = src.c(g, s);
    const auto e = sep.at(s);
    const auto ch = src.chain(g, r0, r1);
    segment_tile<CLS, TA, TB>(g, ch, c, (int)tm, (int)tn, lane, e);
  }
}

#define XAMD_SEG_KERNEL(NAME, CLS) \
  __global__ __launch_bounds__(256) void NAME(GemmGroupDesc g, const unsigned long long* __restrict__ seg_ptr, const void* const* __restrict__ a_list, \
    const void* const* __restrict__ b_list, void* const* __restrict__ c_list, unsigned long long total) { \
    segments_items<CLS, false, false>(g, seg_ptr, ListSource{a_list, b_list, c_list}, NoSegEpilogue{}, total); }
XAMD_SEG_KERNEL(gemm_segments_f32_kernel, 0)
XAMD_SEG_KERNEL(gemm_segments_bf16_kernel, 1)
XAMD_SEG_KERNEL(gemm_segments_f64_kernel, 2)
XAMD_SEG_KERNEL(gemm_segments_bf8_kernel, 3)
XAMD_SEG_KERNEL(gemm_segments_hf8_kernel, 4)
XAMD_SEG_KERNEL(gemm_segments_f16_kernel, 5)
#undef XAMD_SEG_KERNEL

#define XAMD_SEG_FUSED_KERNEL(NAME, CLS) \
  __global__ __launch_bounds__(256) void NAME(GemmGroupDesc g, GemmSegEpilogue e, const unsigned long long* __restrict__ seg_ptr, \
    const void* const* __restrict__ a_list, const void* const* __restrict__ b_list, void* const* __restrict__ c_list, unsigned long long total) { \
    segments_items<CLS, false, false>(g, seg_ptr, ListSource{a_list, b_list, c_list}, ListSegEpilogue{e}, total); }
XAMD_SEG_FUSED_KERNEL(gemm_segments_f32_fused_kernel, 0)
XAMD_SEG_FUSED_KERNEL(gemm_segments_bf16_fused_kernel, 1)
XAMD_SEG_FUSED_KERNEL(gemm_segments_f16_fused_kernel, 5)
#undef XAMD_SEG_FUSED_KERNEL

#define XAMD_OFFS_KERNEL(NAME, CLS) \
  template <bool TA, bool TB> __global__ __launch_bounds__(256) void NAME(GemmGroupDesc g, int a_wide, const unsigned long long* __restrict__ seg_ptr, \
    const long long* __restrict__ a_offs, const long long* __restrict__ b_offs, const long long* __restrict__ c_offs, unsigned long long total) { \
    segments_items<CLS, TA, TB>(g, seg_ptr, OffsetSource<int>{a_offs, b_offs, c_offs, a_wide}, NoSegEpilogue{}, total); }
XAMD_OFFS_KERNEL(gemm_segments_offs_f32_kernel, 0)
XAMD_OFFS_KERNEL(gemm_segments_offs_bf16_kernel, 1)
XAMD_OFFS_KERNEL(gemm_segments_offs_f64_kernel, 2)
XAMD_OFFS_KERNEL(gemm_segments_offs_bf8_kernel, 3)          // 8-bit floats: only the NN instance <0,0> exists
XAMD_OFFS_KERNEL(gemm_segments_offs_hf8_kernel, 4)
XAMD_OFFS_KERNEL(gemm_segments_offs_f16_kernel, 5)
#undef XAMD_OFFS_KERNEL

#define XAMD_OFFS_FUSED_KERNEL(NAME, CLS) \
  template <bool TA, bool TB> __global__ __launch_bounds__(256) void NAME(GemmGroupDesc g, GemmSegOffsEpilogue e, const unsigned long long* __restrict__ seg_ptr, \
    const long long* __restrict__ a_offs, const long long* __restrict__ b_offs, const long long* __restrict__ c_offs, unsigned long long total) { \
    segments_items<CLS, TA, TB>(g, seg_ptr, OffsetSource<const int&>{a_offs, b_offs, c_offs, e.a_wide}, OffsetSegEpilogue{e}, total); }
XAMD_OFFS_FUSED_KERNEL(gemm_segments_offs_f32_fused_kernel, 0)
XAMD_OFFS_FUSED_KERNEL(gemm_segments_offs_bf16_fused_kernel, 1)
XAMD_OFFS_FUSED_KERNEL(gemm_segments_offs_f16_fused_kernel, 5)
#undef XAMD_OFFS_FUSED_KERNEL

// ---- sliced segments (libxsmm_hip_gemm_batch_reduce_segments_sliced, ..._offsets_sliced): a chain cut into slices that separate waves walk ------------------
// Pass 1 is the item loop above with one more policy: the item is (slice, tile), and a slice's destination is not a caller's block but its partial in the
// workspace, g.c + slice * g.sc -- computed, no list is read for it.  The GemmGroupDesc of pass 1 has beta = 0, an accumulator-typed C (f32 for the f32 and
// bf16 classes, f64) and ldc = m: the partial is the dense m x n block, each 16-byte aligned (g.sc is m * n accumulators rounded up to 16 bytes).  The chain
// is the base source's, so a slice is the (product, k) chain of a segment started at +0, bit for bit; an empty slice stores +0.
template <typename Base> struct SlicedSource {
  Base base;
  __device__ __forceinline__ gptr c(const GemmGroupDesc& g, unsigned long long s) const { return (gptr)g.c + (long long)s * g.sc; }
  __device__ __forceinline__ auto chain(const GemmGroupDesc& g, unsigned long long r0, unsigned long long r1) const { return base.chain(g, r0, r1); }
};

#define XAMD_SEG_SLICED_KERNEL(NAME, CLS) \
  __global__ __launch_bounds__(256) void NAME(GemmGroupDesc g, const unsigned long long* __restrict__ seg_ptr, const void* const* __restrict__ a_list, \
    const void* const* __restrict__ b_list, unsigned long long total) { \
    segments_items<CLS, false, false>(g, seg_ptr, SlicedSource<ListSource>{ListSource{a_list, b_list, nullptr}}, NoSegEpilogue{}, total); }
XAMD_SEG_SLICED_KERNEL(gemm_segments_sliced_f32_kernel, 0)
XAMD_SEG_SLICED_KERNEL(gemm_segments_sliced_bf16_kernel, 1)
XAMD_SEG_SLICED_KERNEL(gemm_segments_sliced_f64_kernel, 2)
XAMD_SEG_SLICED_KERNEL(gemm_segments_sliced_bf8_kernel, 3)
XAMD_SEG_SLICED_KERNEL(gemm_segments_sliced_hf8_kernel, 4)
XAMD_SEG_SLICED_KERNEL(gemm_segments_sliced_f16_kernel, 5)
#undef XAMD_SEG_SLICED_KERNEL

#define XAMD_OFFS_SLICED_KERNEL(NAME, CLS) \
  template <bool TA, bool TB> __global__ __launch_bounds__(256) void NAME(GemmGroupDesc g, int a_wide, const unsigned long long* __restrict__ seg_ptr, \
    const long long* __restrict__ a_offs, const long long* __restrict__ b_offs, unsigned long long total) { \
    segments_items<CLS, TA, TB>(g, seg_ptr, SlicedSource<OffsetSource<int>>{OffsetSource<int>{a_offs, b_offs, nullptr, a_wide}}, NoSegEpilogue{}, total); }
XAMD_OFFS_SLICED_KERNEL(gemm_segments_offs_sliced_f32_kernel, 0)
XAMD_OFFS_SLICED_KERNEL(gemm_segments_offs_sliced_bf16_kernel, 1)
XAMD_OFFS_SLICED_KERNEL(gemm_segments_offs_sliced_f64_kernel, 2)
XAMD_OFFS_SLICED_KERNEL(gemm_segments_offs_sliced_bf8_kernel, 3)   // <0,0> only
XAMD_OFFS_SLICED_KERNEL(gemm_segments_offs_sliced_hf8_kernel, 4)
#undef XAMD_OFFS_SLICED_KERNEL
// f16, written out: its NT instance came out at 132 registers (3 waves per SIMD) where the bf16 sibling has 128 (4); it is held to the sibling's occupancy
// (NN: no request).  No scratch results (profiles/r06_kernel_resources.txt).
template <bool TA, bool TB> __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TB ? 4 : 1)))
void gemm_segments_offs_sliced_f16_kernel(GemmGroupDesc g, int a_wide, const unsigned long long* __restrict__ seg_ptr,
    const long long* __restrict__ a_offs, const long long* __restrict__ b_offs, unsigned long long total) {
  segments_items<5, TA, TB>(g, seg_ptr, SlicedSource<OffsetSource<int>>{OffsetSource<int>{a_offs, b_offs, nullptr, a_wide}}, NoSegEpilogue{}, total);
}

// Pass 2: acc = C (beta = 1) or +0, then acc += P_j for the block's slices j in ASCENDING order -- one IEEE add each in the accumulator type (the kernels run
// with denormals kept), no atomics, no arrival order -- then one store with C's ldc and type.  CLS: 0 f32 partials -> f32 C, 1 f32 partials -> bf16 C
// (bf16_cvt.hpp: one rounding), 2 f64, 3 / 4 f32 partials -> BF8 / HF8 C (widened on the way in; out through f32x2_to_fp8_ref, the two-step rounding the
// unsliced kernels store with: a lane's four bytes are one dword store under `wide`).  Bandwidth-bound: a work item is (block, run of 64 x V elements of the dense partial), V = 16 bytes of accumulators, so
// lane l owns the elements (64 run + l) V .. + V - 1 of EVERY slice of the block and a wave's load of one slice is 1 KiB contiguous.  Four slices' loads are in
// flight before the first add; a block's last one to three slices go one by one.  A lane's last load may reach past m * n into the partial's padding (inside
// the workspace by construction of g.sc; never added into anything stored).  blk_ptr[b], blk_ptr[b + 1] and C's entry are wave-uniform scalar loads like the
// item heads of pass 1, and the waves grid-stride in the same way.  C is read only under beta = 1 and written for i < m, j < n only: with m a multiple of V and
// columns and block V-element aligned (`wide_ld`, then the pointer) a lane's V elements are one load / store of C, else element by element.  A block without
// slices: beta = 0 stores +0, beta = 1 is skipped.  No LDS, no scratch, vector stores only.
// The f16 class follows the reference's F16 loop instead: acc = +0, acc += P_j in ascending order, THEN acc += f16(C) widened (beta = 1),
// then one store -- CLS 5: f16 C (cvt_pk_f16, the unsliced kernels' conversion), CLS 6: f32 C, rounded to a half on the way in.  The start comes last in the
// unsliced kernels too, so one slice per block is the unsliced call bit for bit for both betas.  beta = 0 with an f32 C has no start and runs instance <0>.  A
// block without slices under beta = 1 is skipped like every class's: an f32 C is NOT rounded there.
// an element of C as the accumulator it starts
template <int CLS, typename X> __device__ __forceinline__ auto slice_c_widen(X x) {
  if constexpr (CLS == 1) return bf16_bits_to_f32(x);
  else if constexpr (CLS == 3) return bf8_to_f32(x);
  else if constexpr (CLS == 4) return hf8_to_f32(x);
  else if constexpr (CLS == 5) return (float)__builtin_bit_cast(_Float16, x);
  else if constexpr (CLS == 6) return (float)(_Float16)x;                        // the f16 class with an f32 C: the start value is rounded to a half on the way in
  else return x;
}
template <int CLS>
__global__ __launch_bounds__(256) void gemm_segments_slice_reduce_kernel(GemmSliceReduce q, unsigned long long total) {
  typedef typename std::conditional<CLS == 2, double, float>::type acc_t;
  typedef typename std::conditional<CLS == 2, double, typename std::conditional<CLS == 1 || CLS == 5, unsigned short, typename std::conditional<CLS == 3 || CLS == 4, unsigned char, float>::type>::type>::type c_t;
  constexpr bool H16 = CLS >= 5;                                                 // the f16 class: the start value is added BEHIND the partials
  constexpr int V = 16 / (int)sizeof(acc_t);
  typedef acc_t vec_t __attribute__((ext_vector_type(V)));
  typedef c_t cvec_t __attribute__((ext_vector_type(V)));
  const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned int lane = threadIdx.x & 63u;
  const unsigned long long step = (unsigned long long)gridDim.x * 4u;
  const unsigned int mn = (unsigned int)q.m * (unsigned int)q.n;
  for (unsigned long long item = (unsigned long long)blockIdx.x * 4u + wave; item < total; item += step) {
    unsigned long long b = item; unsigned int run = 0;
    if (q.runs != 1) { b = item / q.runs; run = (unsigned int)(item - b * q.runs); }
    const unsigned long long s0 = uniform_u64(((GM const unsigned long long*)q.blk_ptr)[b]), s1 = uniform_u64(((GM const unsigned long long*)q.blk_ptr)[b + 1]);
    if (s0 == s1 && q.beta1) continue;
    gptr c = q.c_base ? (gptr)q.c_base + (long long)uniform_u64(((GM const unsigned long long*)q.c_list)[b]) : (gptr)list_entry(q.c_list, b);
    const unsigned int e0 = (run * 64u + lane) * (unsigned int)V;
    const bool live = e0 < mn;
    const unsigned int el = live ? e0 : 0u;                                      // lanes past the block re-read its first elements and store nothing
    const unsigned int j0 = el / (unsigned int)q.m, i0 = el - j0 * (unsigned int)q.m;
    const bool wide = q.wide_ld && ((unsigned int)(size_t)c & (unsigned int)(V * sizeof(c_t) - 1)) == 0;
    GM c_t* cw = (GM c_t*)c + ((long long)j0 * q.ldc + i0);                      // wide: the lane's V elements of one column
    vec_t acc;
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = (acc_t)0;
    if (q.beta1) {
      if (wide) {
        const cvec_t x = *(GM const cvec_t*)cw;
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = slice_c_widen<CLS>(x[v]);
      } else {
        unsigned int i = i0, j = j0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          if (live && e0 + v < mn) acc[v] = slice_c_widen<CLS>(((GM const c_t*)c)[(long long)j * q.ldc + i]);
          if (++i == (unsigned int)q.m) { i = 0; ++j; }
        }
      }
    }
    [[maybe_unused]] vec_t start;
    if constexpr (H16) {                                                       // the sum runs from +0; C (as a half, widened) joins it last
      start = acc;
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = (acc_t)0;
    }
    gcptr p = (gcptr)q.ws + (long long)s0 * q.pstride + (long long)el * (long long)sizeof(acc_t);
    unsigned long long s = s0;
    for (; s + 4 <= s1; s += 4) {
      const vec_t x0 = *(GM const vec_t*)p, x1 = *(GM const vec_t*)(p + q.pstride), x2 = *(GM const vec_t*)(p + 2 * q.pstride), x3 = *(GM const vec_t*)(p + 3 * q.pstride);
      p += 4 * q.pstride;
      acc += x0; acc += x1; acc += x2; acc += x3;
    }
    for (; s < s1; ++s) { acc += *(GM const vec_t*)p; p += q.pstride; }
    if constexpr (H16) { if (q.beta1) acc += start; }
    if (!live) continue;
    if constexpr (CLS == 5) {
      const unsigned int pk[2] = {cvt_pk_f16((float)acc[0], (float)acc[1]), cvt_pk_f16((float)acc[2], (float)acc[3])};
      if (wide) { u32x2 w = {pk[0], pk[1]}; *(GM u32x2*)cw = w; }
      else {
        unsigned int i = i0, j = j0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          if (e0 + v < mn) ((GM unsigned short*)c)[(long long)j * q.ldc + i] = (unsigned short)((v & 1) ? (pk[v / 2] >> 16) : (pk[v / 2] & 0xffffu));
          if (++i == (unsigned int)q.m) { i = 0; ++j; }
        }
      }
    } else if constexpr (CLS == 3 || CLS == 4) {
      const unsigned int w = f32x2_to_fp8_ref((float)acc[0], (float)acc[1], CLS == 4) | (f32x2_to_fp8_ref((float)acc[2], (float)acc[3], CLS == 4) << 16);
      if (wide) *(GM unsigned int*)cw = w;
      else {
        unsigned int i = i0, j = j0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          if (e0 + v < mn) ((GM unsigned char*)c)[(long long)j * q.ldc + i] = (unsigned char)((w >> (8 * v)) & 0xffu);
          if (++i == (unsigned int)q.m) { i = 0; ++j; }
        }
      }
    } else if constexpr (CLS == 1) {
      float x[V]; unsigned int pk[V / 2];
#pragma unroll
      for (int v = 0; v < V; ++v) x[v] = acc[v];
      bf16_pk_exact_n<V / 2>(x, pk);
      if (wide) { u32x2 w = {pk[0], pk[1]}; *(GM u32x2*)cw = w; }
      else {
        unsigned int i = i0, j = j0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          if (e0 + v < mn) ((GM unsigned short*)c)[(long long)j * q.ldc + i] = (unsigned short)((v & 1) ? (pk[v / 2] >> 16) : (pk[v / 2] & 0xffffu));
          if (++i == (unsigned int)q.m) { i = 0; ++j; }
        }
      }
    } else if (wide) *(GM vec_t*)cw = acc;
    else {
      unsigned int i = i0, j = j0;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (e0 + v < mn) ((GM acc_t*)c)[(long long)j * q.ldc + i] = acc[v];
        if (++i == (unsigned int)q.m) { i = 0; ++j; }
      }
    }
  }
}

// ---- pass 2 with the ext ABI's epilogue (libxsmm_hip_gemm_ext_batch_reduce_segments_sliced, ..._offsets_sliced) ------------------------------------------
// acc = start value of the unsliced ext entries (bias, bias + C in one f32 add, C or +0: acc_start in gemm_group_tile.hpp), then acc += P_j in ascending slice
// order as above, then the mask bit !(acc <= 0), then act_fixed<1> / act_fixed<3>, then the store of pass 2.  A block without slices is NOT skipped: it stores
// the activation of its start value and the mask taken from it, for every beta -- what the unsliced ext entry stores for a segment of count 0.  CLS: 0 f32 C,
// 1 bf16 C (the bias has C's type); the f16 class: 5 f16 C, 6 f32 C -- the start value is rounded to a half and added BEHIND the partials (slice_start_take),
// the order of the unsliced f16 kernels, so a block without slices is their segment of count 0 and one slice per block is their call.  The bias and mask entries of block b are wave-uniform scalar loads like C's entry.  No LDS, no scratch, vector stores only.
// Who writes a mask byte.  A byte holds 8 rows of ONE column; every byte is written by exactly one lane with one store, and no byte is ever read-merge-written by
// two lanes.  Two ways of handing out the work, chosen by a wave-uniform test of the kernel arguments:
//   runs   (no bitmask, or m % 8 == 0)  the work items of the plain kernel: lane l owns 4 consecutive elements of the dense partial, 16-byte loads.  With a
//          bitmask m % 8 == 0, so a column starts at a multiple of 8 dense elements, a byte is the 8 elements of the lane pair (2 l, 2 l + 1) -- never cut by the
//          end of a run (256 elements) -- and all its rows are valid: the odd lane's four predicate bits reach the even lane through one DPP quad permute, the
//          even lane stores the whole byte.  Nothing is read.  The bias: a lane's rows are 4 consecutive entries of the m-vector when m % 4 == 0 -- one vector
//          load when the bias pointer allows (wave-uniform), else element by element.
//   bytes  (bitmask and m % 8 != 0)     an element run's end can fall inside a byte, so the runs are not used: the unit of work is a MASK BYTE -- (column j,
//          rows 8 q .. min(8 q + 8, m) - 1), n * ceil(m / 8) units per block -- and lane l of item (block, run) owns the units run * 64 + l, + runs * 64, ...
//          A unit's elements are consecutive in the dense partial but not 16-byte aligned: element loads, four slices in flight as above.  The lane owns all bits
//          of its byte: a whole-byte store when 8 rows are valid, read-merge-write of the column's last byte by that one lane -- no other lane or wave touches it.
template <int CLS> __device__ __forceinline__ float slice_c_load(const GM void* p, long long i) {
  if constexpr (CLS == 1) return bf16_bits_to_f32(((GM const unsigned short*)p)[i]);
  else if constexpr (CLS == 5) return (float)((GM const _Float16*)p)[i];
  else return ((GM const float*)p)[i];
}
// an element of a vector load of C or the bias
template <int CLS, typename X> __device__ __forceinline__ float slice_c_wide(X x) {
  if constexpr (CLS == 1) return bf16_bits_to_f32(x);
  else if constexpr (CLS == 5) return (float)__builtin_bit_cast(_Float16, x);
  else return x;
}
// The f16 class (CLS 5: f16 C and bias, 6: f32 C and bias) takes the start value LAST: what the loads above the partials built -- C, the bias, bias + C in one
// f32 add -- is rounded to a half, widened and set aside, the sum runs from +0, and slice_start_add joins the two in one f32 add (nothing without a start).
template <int CLS> __device__ __forceinline__ float slice_start_take(float& acc) {
  if constexpr (CLS >= 5) { const float s = (float)(_Float16)acc; acc = 0.0f; return s; }
  else return 0.0f;
}

template <int CLS>
__device__ __forceinline__ void slice_reduce_fused_run(const GemmSliceReduce& q, const GemmSliceEpilogue& e, gptr c, gcptr d, GM unsigned char* mask, gcptr ws0,
  unsigned long long ns, unsigned int run, unsigned int lane) {
  typedef typename std::conditional<CLS == 1 || CLS == 5, unsigned short, float>::type c_t;
  constexpr int V = 4;
  typedef c_t cvec_t __attribute__((ext_vector_type(V)));
  const unsigned int m = (unsigned int)q.m, mn = m * (unsigned int)q.n;
  const unsigned int e0 = (run * 64u + lane) * (unsigned int)V;
  const bool live = e0 < mn;
  const unsigned int el = live ? e0 : 0u;                                        // lanes past the block re-read its first elements and store nothing
  const unsigned int j0 = el / m, i0 = el - j0 * m;
  const bool wide = q.wide_ld && ((unsigned int)(size_t)c & (unsigned int)(V * sizeof(c_t) - 1)) == 0;
  GM c_t* cw = (GM c_t*)c + ((long long)j0 * q.ldc + i0);
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  if (q.beta1) {
    if (wide) {
      const cvec_t x = *(GM const cvec_t*)cw;
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = slice_c_wide<CLS>(x[v]);
    } else {
      unsigned int i = i0, j = j0;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (live && e0 + v < mn) acc[v] = slice_c_load<CLS>(c, (long long)j * q.ldc + i);
        if (++i == m) { i = 0; ++j; }
      }
    }
  }
  if (e.colbias) {                                                               // bias, or bias + C in one f32 add
    f32x4 bv;
    if ((m & 3u) == 0 && ((unsigned int)(size_t)d & (unsigned int)(V * sizeof(c_t) - 1)) == 0) {
      const cvec_t x = *(GM const cvec_t*)((GM const c_t*)d + i0);
#pragma unroll
      for (int v = 0; v < V; ++v) bv[v] = slice_c_wide<CLS>(x[v]);
    } else {
      unsigned int i = i0;
#pragma unroll
      for (int v = 0; v < V; ++v) { bv[v] = slice_c_load<CLS>(d, i); if (++i == m) i = 0; }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = q.beta1 ? bv[v] + acc[v] : bv[v];
  }
  [[maybe_unused]] f32x4 start;
  if constexpr (CLS >= 5) {
#pragma unroll
    for (int v = 0; v < V; ++v) { float x = acc[v]; start[v] = slice_start_take<CLS>(x); acc[v] = x; }
  }
  gcptr p = ws0 + (long long)el * 4;
  unsigned long long s = 0;
  for (; s + 4 <= ns; s += 4) {
    const f32x4 x0 = *(GM const f32x4*)p, x1 = *(GM const f32x4*)(p + q.pstride), x2 = *(GM const f32x4*)(p + 2 * q.pstride), x3 = *(GM const f32x4*)(p + 3 * q.pstride);
    p += 4 * q.pstride;
    acc += x0; acc += x1; acc += x2; acc += x3;
  }
  for (; s < ns; ++s) { acc += *(GM const f32x4*)p; p += q.pstride; }
  if constexpr (CLS >= 5) { if (q.beta1 || e.colbias) acc += start; }
  if (e.act == 2) {                                                           // m % 8 == 0: the lane pair's byte, all 8 rows valid (every lane is active here)
    unsigned int nib = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) nib |= (acc[v] <= 0.0f ? 0u : 1u) << v;
    const unsigned int hi = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)nib, 0xB1, 0xf, 0xf, false);   // quad_perm [1, 0, 3, 2]: the pair's other lane
    if (live && (lane & 1u) == 0) mask[(long long)(i0 >> 3) + (long long)j0 * (e.mask_ld >> 3)] = (unsigned char)(nib | (hi << 4));
  }
  if (e.act == 3) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = act_fixed<3>(acc[v]);
  } else if (e.act != 0) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = act_fixed<1>(acc[v]);
  }
  if (!live) return;
  if constexpr (CLS == 5) {
    const unsigned int pk[2] = {cvt_pk_f16(acc[0], acc[1]), cvt_pk_f16(acc[2], acc[3])};
    if (wide) { u32x2 w = {pk[0], pk[1]}; *(GM u32x2*)cw = w; }
    else {
      unsigned int i = i0, j = j0;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (e0 + v < mn) ((GM unsigned short*)c)[(long long)j * q.ldc + i] = (unsigned short)((v & 1) ? (pk[v / 2] >> 16) : (pk[v / 2] & 0xffffu));
        if (++i == m) { i = 0; ++j; }
      }
    }
  } else if constexpr (CLS == 1) {
    float x[V]; unsigned int pk[V / 2];
#pragma unroll
    for (int v = 0; v < V; ++v) x[v] = acc[v];
    bf16_pk_exact_n<V / 2>(x, pk);
    if (wide) { u32x2 w = {pk[0], pk[1]}; *(GM u32x2*)cw = w; }
    else {
      unsigned int i = i0, j = j0;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (e0 + v < mn) ((GM unsigned short*)c)[(long long)j * q.ldc + i] = (unsigned short)((v & 1) ? (pk[v / 2] >> 16) : (pk[v / 2] & 0xffffu));
        if (++i == m) { i = 0; ++j; }
      }
    }
  } else if (wide) *(GM f32x4*)cw = acc;
  else {
    unsigned int i = i0, j = j0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (e0 + v < mn) ((GM float*)c)[(long long)j * q.ldc + i] = acc[v];
      if (++i == m) { i = 0; ++j; }
    }
  }
}

template <int CLS>
__device__ __forceinline__ void slice_reduce_fused_bytes(const GemmSliceReduce& q, const GemmSliceEpilogue& e, gptr c, gcptr d, GM unsigned char* mask, gcptr ws0,
  unsigned long long ns, unsigned int run, unsigned int lane) {
  typedef typename std::conditional<CLS == 1 || CLS == 5, unsigned short, float>::type c_t;
  const unsigned int m = (unsigned int)q.m, mq = (m + 7u) >> 3, units = mq * (unsigned int)q.n;
  for (unsigned int u0 = run * 64u; u0 < units; u0 += q.runs * 64u) {
    const bool live = u0 + lane < units;
    const unsigned int u = live ? u0 + lane : 0u;                                // lanes past the block re-read its first unit and store nothing
    const unsigned int j = u / mq, qi = u - j * mq, i0 = qi * 8u;
    const unsigned int nv = min(8u, m - i0);                                     // valid rows of the byte
    GM c_t* cc = (GM c_t*)c + ((long long)j * q.ldc + i0);
    float acc[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) acc[v] = 0.0f;
    if (q.beta1) {
#pragma unroll
      for (int v = 0; v < 8; ++v) if ((unsigned int)v < nv) acc[v] = slice_c_load<CLS>(cc, v);
    }
    if (e.colbias) {
#pragma unroll
      for (int v = 0; v < 8; ++v) if ((unsigned int)v < nv) { const float bv = slice_c_load<CLS>(d, i0 + v); acc[v] = q.beta1 ? bv + acc[v] : bv; }
    }
    [[maybe_unused]] float start[8];
    if constexpr (CLS >= 5) {
#pragma unroll
      for (int v = 0; v < 8; ++v) start[v] = slice_start_take<CLS>(acc[v]);
    }
    gcptr p = ws0 + ((long long)j * m + i0) * 4;
    unsigned long long s = 0;
    for (; s + 4 <= ns; s += 4) {
      float x[4][8];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int v = 0; v < 8; ++v) x[t][v] = (unsigned int)v < nv ? ((GM const float*)(p + t * q.pstride))[v] : 0.0f;
      }
      p += 4 * q.pstride;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int v = 0; v < 8; ++v) acc[v] += x[t][v];
      }
    }
    for (; s < ns; ++s) {
      float x[8];
#pragma unroll
      for (int v = 0; v < 8; ++v) x[v] = (unsigned int)v < nv ? ((GM const float*)p)[v] : 0.0f;
      p += q.pstride;
#pragma unroll
      for (int v = 0; v < 8; ++v) acc[v] += x[v];
    }
    if constexpr (CLS >= 5) {
      if (q.beta1 || e.colbias) {
#pragma unroll
        for (int v = 0; v < 8; ++v) acc[v] += start[v];
      }
    }
    unsigned int bits = 0;
#pragma unroll
    for (int v = 0; v < 8; ++v) bits |= ((unsigned int)v < nv && !(acc[v] <= 0.0f) ? 1u : 0u) << v;
    if (live) {                                                                  // this lane alone owns the byte
      GM unsigned char* byte = mask + qi + (long long)j * (e.mask_ld >> 3);
      const unsigned int vm = (1u << nv) - 1u;
      *byte = nv == 8u ? (unsigned char)bits : (unsigned char)((*byte & ~vm) | bits);
    }
#pragma unroll
    for (int v = 0; v < 8; ++v) acc[v] = act_fixed<1>(acc[v]);
    if constexpr (CLS == 5) {
      const unsigned int pk[4] = {cvt_pk_f16(acc[0], acc[1]), cvt_pk_f16(acc[2], acc[3]), cvt_pk_f16(acc[4], acc[5]), cvt_pk_f16(acc[6], acc[7])};
#pragma unroll
      for (int v = 0; v < 8; ++v) if (live && (unsigned int)v < nv) ((GM unsigned short*)cc)[v] = (unsigned short)((v & 1) ? (pk[v / 2] >> 16) : (pk[v / 2] & 0xffffu));
    } else if constexpr (CLS == 1) {
      unsigned int pk[4];
      bf16_pk_exact_n<4>(acc, pk);
#pragma unroll
      for (int v = 0; v < 8; ++v) if (live && (unsigned int)v < nv) ((GM unsigned short*)cc)[v] = (unsigned short)((v & 1) ? (pk[v / 2] >> 16) : (pk[v / 2] & 0xffffu));
    } else {
#pragma unroll
      for (int v = 0; v < 8; ++v) if (live && (unsigned int)v < nv) ((GM float*)cc)[v] = acc[v];
    }
  }
}

template <int CLS>
__global__ __launch_bounds__(256) void gemm_segments_slice_reduce_fused_kernel(GemmSliceReduce q, GemmSliceEpilogue e, unsigned long long total) {
  const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned int lane = threadIdx.x & 63u;
  const unsigned long long step = (unsigned long long)gridDim.x * 4u;
  const bool bytes = e.act == 2 && (q.m & 7) != 0;
  for (unsigned long long item = (unsigned long long)blockIdx.x * 4u + wave; item < total; item += step) {
    unsigned long long b = item; unsigned int run = 0;
    if (q.runs != 1) { b = item / q.runs; run = (unsigned int)(item - b * q.runs); }
    const unsigned long long s0 = uniform_u64(((GM const unsigned long long*)q.blk_ptr)[b]), s1 = uniform_u64(((GM const unsigned long long*)q.blk_ptr)[b + 1]);
    gptr c = q.c_base ? (gptr)q.c_base + (long long)uniform_u64(((GM const unsigned long long*)q.c_list)[b]) : (gptr)list_entry(q.c_list, b);
    gcptr d = (gcptr)e.d;
    if (e.colbias && e.d_list) d = e.offs ? d + (long long)uniform_u64(((GM const unsigned long long*)e.d_list)[b]) : list_entry(e.d_list, b);
    GM unsigned char* mask = nullptr;
    if (e.act == 2) mask = e.offs ? (GM unsigned char*)e.mask + (long long)uniform_u64(((GM const unsigned long long*)e.mask_list)[b]) : (GM unsigned char*)list_entry(e.mask_list, b);
    gcptr ws0 = (gcptr)q.ws + (long long)s0 * q.pstride;
    if (bytes) slice_reduce_fused_bytes<CLS>(q, e, c, d, mask, ws0, s1 - s0, run, lane);
    else slice_reduce_fused_run<CLS>(q, e, c, d, mask, ws0, s1 - s0, run, lane);
  }
}

// the four instances of an offsets kernel, indexed by forms & 3 (bit 0 TRANS_A, bit 1 TRANS_B)
#define XAMD_FORMS(NAME) {NAME "<0,0>", NAME "<1,0>", NAME "<0,1>", NAME "<1,1>"}
// f16: the NN and NT instances are all there is (launch_gemm_segments returns an error for the other two forms)
#define XAMD_FORMS_NT(NAME) {NAME "<0,0>", nullptr, NAME "<0,1>", nullptr}
// rows: the classes 0 .. 5 (f32, bf16, f64, BF8, HF8, f16), then (unsliced) the three fused classes f32, bf16, f16; the 8-bit float offsets kernels have the NN instance only
static const char* const kSlicedNames[6] = {"gemm_segments_sliced_f32_kernel", "gemm_segments_sliced_bf16_kernel", "gemm_segments_sliced_f64_kernel",
  "gemm_segments_sliced_bf8_kernel", "gemm_segments_sliced_hf8_kernel", "gemm_segments_sliced_f16_kernel"};
static const char* const kOffsSlicedNames[6][4] = {XAMD_FORMS("gemm_segments_offs_sliced_f32_kernel"), XAMD_FORMS("gemm_segments_offs_sliced_bf16_kernel"),
  XAMD_FORMS("gemm_segments_offs_sliced_f64_kernel"), XAMD_FORMS("gemm_segments_offs_sliced_bf8_kernel"), XAMD_FORMS("gemm_segments_offs_sliced_hf8_kernel"),
  XAMD_FORMS_NT("gemm_segments_offs_sliced_f16_kernel")};
static const char* const kListNames[9] = {"gemm_segments_f32_kernel", "gemm_segments_bf16_kernel", "gemm_segments_f64_kernel", "gemm_segments_bf8_kernel",
  "gemm_segments_hf8_kernel", "gemm_segments_f16_kernel", "gemm_segments_f32_fused_kernel", "gemm_segments_bf16_fused_kernel", "gemm_segments_f16_fused_kernel"};
static const char* const kOffsNames[9][4] = {XAMD_FORMS("gemm_segments_offs_f32_kernel"), XAMD_FORMS("gemm_segments_offs_bf16_kernel"), XAMD_FORMS("gemm_segments_offs_f64_kernel"),
  XAMD_FORMS("gemm_segments_offs_bf8_kernel"), XAMD_FORMS("gemm_segments_offs_hf8_kernel"), XAMD_FORMS_NT("gemm_segments_offs_f16_kernel"),
  XAMD_FORMS("gemm_segments_offs_f32_fused_kernel"), XAMD_FORMS("gemm_segments_offs_bf16_fused_kernel"), XAMD_FORMS_NT("gemm_segments_offs_f16_fused_kernel")};
#undef XAMD_FORMS
#undef XAMD_FORMS_NT

template <bool TA, bool TB>
static void launch_offs_form(const SegmentsLaunch& l, unsigned int grid, hipStream_t st) {
  const long long* a_offs = (const long long*)l.a_list; const long long* b_offs = (const long long*)l.b_list; const long long* c_offs = (const long long*)l.c_list;
  if (l.fused) {
    const GemmSegOffsEpilogue& e = *(const GemmSegOffsEpilogue*)l.epilogue;
    if constexpr (!TA) {                                   // f16: no handle has TRANS_A (dispatch refuses it: the reference's F16 loop has no transposed A), so NN and NT only
      if (l.cls == 5) { hipLaunchKernelGGL((gemm_segments_offs_f16_fused_kernel<false, TB>), dim3(grid), dim3(256), 0, st, l.g, e, l.seg_ptr, a_offs, b_offs, c_offs, l.items); return; }
    }
    if (l.cls == 1) hipLaunchKernelGGL((gemm_segments_offs_bf16_fused_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, l.g, e, l.seg_ptr, a_offs, b_offs, c_offs, l.items);
    else hipLaunchKernelGGL((gemm_segments_offs_f32_fused_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, l.g, e, l.seg_ptr, a_offs, b_offs, c_offs, l.items);
    return;
  }
  const int a_wide = (l.forms >> 2) & 3;
  if constexpr (!TA && !TB) {                              // 8-bit floats: the host refuses the transposed forms
    if (l.cls == 3) { hipLaunchKernelGGL((gemm_segments_offs_bf8_kernel<false, false>), dim3(grid), dim3(256), 0, st, l.g, a_wide, l.seg_ptr, a_offs, b_offs, c_offs, l.items); return; }
    if (l.cls == 4) { hipLaunchKernelGGL((gemm_segments_offs_hf8_kernel<false, false>), dim3(grid), dim3(256), 0, st, l.g, a_wide, l.seg_ptr, a_offs, b_offs, c_offs, l.items); return; }
  }
  if constexpr (!TA) {
    if (l.cls == 5) { hipLaunchKernelGGL((gemm_segments_offs_f16_kernel<false, TB>), dim3(grid), dim3(256), 0, st, l.g, a_wide, l.seg_ptr, a_offs, b_offs, c_offs, l.items); return; }
  }
  if (l.cls == 2) hipLaunchKernelGGL((gemm_segments_offs_f64_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, l.g, a_wide, l.seg_ptr, a_offs, b_offs, c_offs, l.items);
  else if (l.cls == 1) hipLaunchKernelGGL((gemm_segments_offs_bf16_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, l.g, a_wide, l.seg_ptr, a_offs, b_offs, c_offs, l.items);
  else hipLaunchKernelGGL((gemm_segments_offs_f32_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, l.g, a_wide, l.seg_ptr, a_offs, b_offs, c_offs, l.items);
}

static void launch_list(const SegmentsLaunch& l, unsigned int grid, hipStream_t st) {
  const void* const* a_list = (const void* const*)l.a_list; const void* const* b_list = (const void* const*)l.b_list; void* const* c_list = (void* const*)l.c_list;
  if (l.fused) {
    const GemmSegEpilogue& e = *(const GemmSegEpilogue*)l.epilogue;
    if (l.cls == 5) hipLaunchKernelGGL(gemm_segments_f16_fused_kernel, dim3(grid), dim3(256), 0, st, l.g, e, l.seg_ptr, a_list, b_list, c_list, l.items);
    else if (l.cls == 1) hipLaunchKernelGGL(gemm_segments_bf16_fused_kernel, dim3(grid), dim3(256), 0, st, l.g, e, l.seg_ptr, a_list, b_list, c_list, l.items);
    else hipLaunchKernelGGL(gemm_segments_f32_fused_kernel, dim3(grid), dim3(256), 0, st, l.g, e, l.seg_ptr, a_list, b_list, c_list, l.items);
  } else if (l.cls == 5) hipLaunchKernelGGL(gemm_segments_f16_kernel, dim3(grid), dim3(256), 0, st, l.g, l.seg_ptr, a_list, b_list, c_list, l.items);
  else if (l.cls == 4) hipLaunchKernelGGL(gemm_segments_hf8_kernel, dim3(grid), dim3(256), 0, st, l.g, l.seg_ptr, a_list, b_list, c_list, l.items);
  else if (l.cls == 3) hipLaunchKernelGGL(gemm_segments_bf8_kernel, dim3(grid), dim3(256), 0, st, l.g, l.seg_ptr, a_list, b_list, c_list, l.items);
  else if (l.cls == 2) hipLaunchKernelGGL(gemm_segments_f64_kernel, dim3(grid), dim3(256), 0, st, l.g, l.seg_ptr, a_list, b_list, c_list, l.items);
  else if (l.cls == 1) hipLaunchKernelGGL(gemm_segments_bf16_kernel, dim3(grid), dim3(256), 0, st, l.g, l.seg_ptr, a_list, b_list, c_list, l.items);
  else hipLaunchKernelGGL(gemm_segments_f32_kernel, dim3(grid), dim3(256), 0, st, l.g, l.seg_ptr, a_list, b_list, c_list, l.items);
}

template <bool TA, bool TB>
static void launch_offs_sliced_form(const SegmentsLaunch& l, const GemmGroupDesc& g, unsigned int grid, hipStream_t st) {
  const long long* a_offs = (const long long*)l.a_list; const long long* b_offs = (const long long*)l.b_list;
  const int a_wide = (l.forms >> 2) & 3;
  if constexpr (!TA && !TB) {
    if (l.cls == 3) { hipLaunchKernelGGL((gemm_segments_offs_sliced_bf8_kernel<false, false>), dim3(grid), dim3(256), 0, st, g, a_wide, l.seg_ptr, a_offs, b_offs, l.items); return; }
    if (l.cls == 4) { hipLaunchKernelGGL((gemm_segments_offs_sliced_hf8_kernel<false, false>), dim3(grid), dim3(256), 0, st, g, a_wide, l.seg_ptr, a_offs, b_offs, l.items); return; }
  }
  if constexpr (!TA) {
    if (l.cls == 5) { hipLaunchKernelGGL((gemm_segments_offs_sliced_f16_kernel<false, TB>), dim3(grid), dim3(256), 0, st, g, a_wide, l.seg_ptr, a_offs, b_offs, l.items); return; }
  }
  if (l.cls == 2) hipLaunchKernelGGL((gemm_segments_offs_sliced_f64_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, g, a_wide, l.seg_ptr, a_offs, b_offs, l.items);
  else if (l.cls == 1) hipLaunchKernelGGL((gemm_segments_offs_sliced_bf16_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, g, a_wide, l.seg_ptr, a_offs, b_offs, l.items);
  else hipLaunchKernelGGL((gemm_segments_offs_sliced_f32_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, g, a_wide, l.seg_ptr, a_offs, b_offs, l.items);
}

// The two launches of a sliced call, in order on one stream: the slices' partials into the workspace (skipped without slices), then the blocks' sums.
static int launch_sliced(const SegmentsLaunch& l, hipStream_t st, const char** kname) {
  *kname = l.offsets ? kOffsSlicedNames[l.cls][l.forms & 3] : kSlicedNames[l.cls];
  const int V = l.cls == 2 ? 2 : 4;                        // accumulators in 16 bytes
  if (l.items != 0) {
    GemmGroupDesc g = l.g;                                 // pass 1 writes partials: beta = 0, accumulator-typed, dense, `pstride` bytes apart in the workspace
    g.beta1 = 0; g.c_kind = 0; g.ldc = g.m; g.c = (char*)l.workspace; g.sc = l.pstride;
    const unsigned int grid = group_grid(l.items);
    if (!l.offsets) {
      const void* const* a_list = (const void* const*)l.a_list; const void* const* b_list = (const void* const*)l.b_list;
      if (l.cls == 5) hipLaunchKernelGGL(gemm_segments_sliced_f16_kernel, dim3(grid), dim3(256), 0, st, g, l.seg_ptr, a_list, b_list, l.items);
      else if (l.cls == 4) hipLaunchKernelGGL(gemm_segments_sliced_hf8_kernel, dim3(grid), dim3(256), 0, st, g, l.seg_ptr, a_list, b_list, l.items);
      else if (l.cls == 3) hipLaunchKernelGGL(gemm_segments_sliced_bf8_kernel, dim3(grid), dim3(256), 0, st, g, l.seg_ptr, a_list, b_list, l.items);
      else if (l.cls == 2) hipLaunchKernelGGL(gemm_segments_sliced_f64_kernel, dim3(grid), dim3(256), 0, st, g, l.seg_ptr, a_list, b_list, l.items);
      else if (l.cls == 1) hipLaunchKernelGGL(gemm_segments_sliced_bf16_kernel, dim3(grid), dim3(256), 0, st, g, l.seg_ptr, a_list, b_list, l.items);
      else hipLaunchKernelGGL(gemm_segments_sliced_f32_kernel, dim3(grid), dim3(256), 0, st, g, l.seg_ptr, a_list, b_list, l.items);
    } else switch (l.forms & 3) {
      case 0: launch_offs_sliced_form<false, false>(l, g, grid, st); break;
      case 1: launch_offs_sliced_form<true, false>(l, g, grid, st); break;
      case 2: launch_offs_sliced_form<false, true>(l, g, grid, st); break;
      default: launch_offs_sliced_form<true, true>(l, g, grid, st); break;
    }
    const int err = (int)hipGetLastError();
    if (err != 0) return err;
  }
  GemmSliceReduce q;
  q.blk_ptr = l.blk_ptr; q.c_list = l.c_list; q.c_base = l.offsets ? l.g.c : nullptr; q.ws = (const char*)l.workspace; q.pstride = l.pstride;
  q.m = l.g.m; q.n = l.g.n; q.ldc = l.g.ldc; q.beta1 = l.g.beta1;
  const unsigned long long mn = (unsigned long long)l.g.m * (unsigned long long)l.g.n;
  q.runs = slice_reduce_runs(mn, l.cls);
  q.wide_ld = (l.g.m % V == 0 && l.g.ldc % V == 0) ? 1 : 0;      // a lane's V elements as one load / store of C: inside one column, V-element aligned
  const unsigned long long total = l.nblocks * q.runs;
  const unsigned int grid = group_grid(total);
  if (l.fused) {                                         // the ext entries: the block-level epilogue lists travel next to q
    GemmSliceEpilogue e = {};
    if (l.offsets) {
      const GemmSegOffsEpilogue& o = *(const GemmSegOffsEpilogue*)l.epilogue;
      e.d_list = o.d_offs; e.d = o.d; e.mask_list = o.mask_offs; e.mask = o.mask; e.colbias = o.colbias; e.act = o.act; e.mask_ld = o.mask_ld; e.offs = 1;
    } else {
      const GemmSegEpilogue& o = *(const GemmSegEpilogue*)l.epilogue;
      e.d_list = o.d_list; e.d = o.d; e.mask_list = o.mask_list; e.colbias = o.colbias; e.act = o.act; e.mask_ld = o.mask_ld;
    }
    if (l.cls == 5 && l.g.c_kind == 4) hipLaunchKernelGGL(gemm_segments_slice_reduce_fused_kernel<5>, dim3(grid), dim3(256), 0, st, q, e, total);
    else if (l.cls == 5) hipLaunchKernelGGL(gemm_segments_slice_reduce_fused_kernel<6>, dim3(grid), dim3(256), 0, st, q, e, total);
    else if (l.g.c_kind == 1) hipLaunchKernelGGL(gemm_segments_slice_reduce_fused_kernel<1>, dim3(grid), dim3(256), 0, st, q, e, total);
    else hipLaunchKernelGGL(gemm_segments_slice_reduce_fused_kernel<0>, dim3(grid), dim3(256), 0, st, q, e, total);
    return (int)hipGetLastError();
  }
  // the f16 class adds its start value last (instances <5> f16 C, <6> f32 C under beta = 1); an f32 C under beta = 0 has none: instance <0>
  if (l.cls == 5 && l.g.c_kind == 4) hipLaunchKernelGGL(gemm_segments_slice_reduce_kernel<5>, dim3(grid), dim3(256), 0, st, q, total);
  else if (l.cls == 5 && l.g.beta1) hipLaunchKernelGGL(gemm_segments_slice_reduce_kernel<6>, dim3(grid), dim3(256), 0, st, q, total);
  else if (l.cls == 2) hipLaunchKernelGGL(gemm_segments_slice_reduce_kernel<2>, dim3(grid), dim3(256), 0, st, q, total);
  else if (l.g.c_kind == 1) hipLaunchKernelGGL(gemm_segments_slice_reduce_kernel<1>, dim3(grid), dim3(256), 0, st, q, total);
  else if (l.g.c_kind == 2) hipLaunchKernelGGL(gemm_segments_slice_reduce_kernel<3>, dim3(grid), dim3(256), 0, st, q, total);
  else if (l.g.c_kind == 3) hipLaunchKernelGGL(gemm_segments_slice_reduce_kernel<4>, dim3(grid), dim3(256), 0, st, q, total);
  else hipLaunchKernelGGL(gemm_segments_slice_reduce_kernel<0>, dim3(grid), dim3(256), 0, st, q, total);
  return (int)hipGetLastError();
}

int launch_gemm_segments(const SegmentsLaunch& l, void* stream, const char** kname) {
  // f16 kernels exist as NN and NT only (no handle has TRANS_A; segments_handle refuses one): an error here, never another class's kernel
  if (l.cls == 5 && (l.forms & 1)) { *kname = ""; return (int)hipErrorInvalidValue; }
  if (l.sliced) return launch_sliced(l, (hipStream_t)stream, kname);
  const int row = l.fused ? (l.cls == 5 ? 8 : (l.cls == 1 ? 7 : 6)) : l.cls;
  *kname = l.offsets ? kOffsNames[row][l.forms & 3] : kListNames[row];
  if (l.items == 0) return 0;
  const unsigned int grid = group_grid(l.items);
  hipStream_t st = (hipStream_t)stream;
  if (!l.offsets) launch_list(l, grid, st);
  else switch (l.forms & 3) {
    case 0: launch_offs_form<false, false>(l, grid, st); break;
    case 1: launch_offs_form<true, false>(l, grid, st); break;
    case 2: launch_offs_form<false, true>(l, grid, st); break;
    default: launch_offs_form<true, true>(l, grid, st); break;
  }
  return (int)hipGetLastError();
}

}  // namespace xamd
