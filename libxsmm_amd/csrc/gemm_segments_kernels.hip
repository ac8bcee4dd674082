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
#include <hip/hip_runtime.h>
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

// CLS: 0 f32, 1 bf16, 2 f64 (16 x 16 tiles only, no epilogue).  The tile edge is a wave-uniform runtime value, the class and the transposes pick the instance.
template <int CLS, bool TA, bool TB, typename Chain, typename Epi>
__device__ __forceinline__ void segment_tile(const GemmGroupDesc& g, const Chain& ch, gptr c, int tm, int tn, unsigned int lane, const Epi& e) {
  if constexpr (CLS == 2) tile_f64<Chain, TA, TB>(g, ch, c, tm * 16, tn * 16, lane);
  else if (g.tile == 32) {
    if constexpr (CLS == 1) tile_bf16<32, true, Chain, Epi, TA, TB>(g, ch, c, tm * 32, tn * 32, lane, e);
    else tile_f32<32, true, Chain, Epi, TA, TB>(g, ch, c, tm * 32, tn * 32, lane, e);
  } else {
    if constexpr (CLS == 1) tile_bf16<16, true, Chain, Epi, TA, TB>(g, ch, c, tm * 16, tn * 16, lane, e);
    else tile_f32<16, true, Chain, Epi, TA, TB>(g, ch, c, tm * 16, tn * 16, lane, e);
  }
}

// The item loop of all 25 kernels.  Per item, in this order: seg_ptr[s], seg_ptr[s + 1], C's address, the epilogue's entries, then the chain.
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
#undef XAMD_SEG_KERNEL

#define XAMD_SEG_FUSED_KERNEL(NAME, CLS) \
  __global__ __launch_bounds__(256) void NAME(GemmGroupDesc g, GemmSegEpilogue e, const unsigned long long* __restrict__ seg_ptr, \
    const void* const* __restrict__ a_list, const void* const* __restrict__ b_list, void* const* __restrict__ c_list, unsigned long long total) { \
    segments_items<CLS, false, false>(g, seg_ptr, ListSource{a_list, b_list, c_list}, ListSegEpilogue{e}, total); }
XAMD_SEG_FUSED_KERNEL(gemm_segments_f32_fused_kernel, 0)
XAMD_SEG_FUSED_KERNEL(gemm_segments_bf16_fused_kernel, 1)
#undef XAMD_SEG_FUSED_KERNEL

#define XAMD_OFFS_KERNEL(NAME, CLS) \
  template <bool TA, bool TB> __global__ __launch_bounds__(256) void NAME(GemmGroupDesc g, int a_wide, const unsigned long long* __restrict__ seg_ptr, \
    const long long* __restrict__ a_offs, const long long* __restrict__ b_offs, const long long* __restrict__ c_offs, unsigned long long total) { \
    segments_items<CLS, TA, TB>(g, seg_ptr, OffsetSource<int>{a_offs, b_offs, c_offs, a_wide}, NoSegEpilogue{}, total); }
XAMD_OFFS_KERNEL(gemm_segments_offs_f32_kernel, 0)
XAMD_OFFS_KERNEL(gemm_segments_offs_bf16_kernel, 1)
XAMD_OFFS_KERNEL(gemm_segments_offs_f64_kernel, 2)
#undef XAMD_OFFS_KERNEL

#define XAMD_OFFS_FUSED_KERNEL(NAME, CLS) \
  template <bool TA, bool TB> __global__ __launch_bounds__(256) void NAME(GemmGroupDesc g, GemmSegOffsEpilogue e, const unsigned long long* __restrict__ seg_ptr, \
    const long long* __restrict__ a_offs, const long long* __restrict__ b_offs, const long long* __restrict__ c_offs, unsigned long long total) { \
    segments_items<CLS, TA, TB>(g, seg_ptr, OffsetSource<const int&>{a_offs, b_offs, c_offs, e.a_wide}, OffsetSegEpilogue{e}, total); }
XAMD_OFFS_FUSED_KERNEL(gemm_segments_offs_f32_fused_kernel, 0)
XAMD_OFFS_FUSED_KERNEL(gemm_segments_offs_bf16_fused_kernel, 1)
#undef XAMD_OFFS_FUSED_KERNEL

// the four instances of an offsets kernel, indexed by forms & 3 (bit 0 TRANS_A, bit 1 TRANS_B)
#define XAMD_FORMS(NAME) {NAME "<0,0>", NAME "<1,0>", NAME "<0,1>", NAME "<1,1>"}
static const char* const kListNames[5] = {"gemm_segments_f32_kernel", "gemm_segments_bf16_kernel", "gemm_segments_f64_kernel", "gemm_segments_f32_fused_kernel",
  "gemm_segments_bf16_fused_kernel"};
static const char* const kOffsNames[5][4] = {XAMD_FORMS("gemm_segments_offs_f32_kernel"), XAMD_FORMS("gemm_segments_offs_bf16_kernel"), XAMD_FORMS("gemm_segments_offs_f64_kernel"),
  XAMD_FORMS("gemm_segments_offs_f32_fused_kernel"), XAMD_FORMS("gemm_segments_offs_bf16_fused_kernel")};
#undef XAMD_FORMS

template <bool TA, bool TB>
static void launch_offs_form(const SegmentsLaunch& l, unsigned int grid, hipStream_t st) {
  const long long* a_offs = (const long long*)l.a_list; const long long* b_offs = (const long long*)l.b_list; const long long* c_offs = (const long long*)l.c_list;
  if (l.fused) {
    const GemmSegOffsEpilogue& e = *(const GemmSegOffsEpilogue*)l.epilogue;
    if (l.cls == 1) hipLaunchKernelGGL((gemm_segments_offs_bf16_fused_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, l.g, e, l.seg_ptr, a_offs, b_offs, c_offs, l.items);
    else hipLaunchKernelGGL((gemm_segments_offs_f32_fused_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, l.g, e, l.seg_ptr, a_offs, b_offs, c_offs, l.items);
    return;
  }
  const int a_wide = (l.forms >> 2) & 3;
  if (l.cls == 2) hipLaunchKernelGGL((gemm_segments_offs_f64_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, l.g, a_wide, l.seg_ptr, a_offs, b_offs, c_offs, l.items);
  else if (l.cls == 1) hipLaunchKernelGGL((gemm_segments_offs_bf16_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, l.g, a_wide, l.seg_ptr, a_offs, b_offs, c_offs, l.items);
  else hipLaunchKernelGGL((gemm_segments_offs_f32_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, l.g, a_wide, l.seg_ptr, a_offs, b_offs, c_offs, l.items);
}

static void launch_list(const SegmentsLaunch& l, unsigned int grid, hipStream_t st) {
  const void* const* a_list = (const void* const*)l.a_list; const void* const* b_list = (const void* const*)l.b_list; void* const* c_list = (void* const*)l.c_list;
  if (l.fused) {
    const GemmSegEpilogue& e = *(const GemmSegEpilogue*)l.epilogue;
    if (l.cls == 1) hipLaunchKernelGGL(gemm_segments_bf16_fused_kernel, dim3(grid), dim3(256), 0, st, l.g, e, l.seg_ptr, a_list, b_list, c_list, l.items);
    else hipLaunchKernelGGL(gemm_segments_f32_fused_kernel, dim3(grid), dim3(256), 0, st, l.g, e, l.seg_ptr, a_list, b_list, c_list, l.items);
  } else if (l.cls == 2) hipLaunchKernelGGL(gemm_segments_f64_kernel, dim3(grid), dim3(256), 0, st, l.g, l.seg_ptr, a_list, b_list, c_list, l.items);
  else if (l.cls == 1) hipLaunchKernelGGL(gemm_segments_bf16_kernel, dim3(grid), dim3(256), 0, st, l.g, l.seg_ptr, a_list, b_list, c_list, l.items);
  else hipLaunchKernelGGL(gemm_segments_f32_kernel, dim3(grid), dim3(256), 0, st, l.g, l.seg_ptr, a_list, b_list, c_list, l.items);
}

int launch_gemm_segments(const SegmentsLaunch& l, void* stream, const char** kname) {
  const int row = l.fused ? (l.cls == 1 ? 4 : 3) : l.cls;
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
