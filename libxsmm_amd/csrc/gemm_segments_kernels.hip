// gemm_segments_kernels.hip -- libxsmm_hip_gemm_batch_reduce_segments: ADDRESS batch-reduce products with a reduce count of their own per C block, one launch.
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
// libxsmm_hip_gemm_ext_batch_reduce_segments runs the same items through gemm_segments_f32_fused_kernel / _bf16_fused_kernel: the tiles take a FusedEpilogue
// (gemm_group_tile.hpp) whose bias and mask pointers are d_list[s] and mask_list[s], read like c_list[s]; the operators are wave-uniform runtime bits of a small
// by-value block (GemmSegEpilogue) next to the GemmGroupDesc.  A segment of count 0 stores the activation of its start value (the bias, bias + C) and its mask.
// The plain kernels above are instantiated with the default epilogue and are instruction for instruction what they were without it.
//
// libxsmm_hip_gemm_batch_reduce_segments_offsets runs the same items through gemm_segments_offs_f32_kernel / _bf16_kernel / _f64_kernel: OFFSET batch-reduce
// [ref: src/generator_gemm_reference_impl.c:509-513, :186-188].  The three bases travel by value in the GemmGroupDesc's operand slots; a_offs / b_offs / c_offs
// hold signed byte offsets, read with the scalar loads that read the pointer lists above (OffsetChain), one 64-bit add per product.  A and / or B may be
// transposed -- the backward passes of a block-sparse layer, dX = W^T dY and dW = dY X^T -- through the transposed load forms of the tiles.  The two transposes
// are template parameters of the kernels, four instances per class: as wave-uniform runtime bits that select the tile instance inside ONE kernel they cost
// 196 / 224 / 88 registers (f32 / bf16 / f64: a wave per SIMD less for f32, two less for f64), although no single form needs more than the ADDRESS kernels'
// 160 / 196 / 72 -- the register allocator does not keep the four bodies apart (DESIGN.md section 9.2 has the numbers).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "internal.hpp"
#include "gemm_device.hpp"
#include "bf16_cvt.hpp"
#include "gemm_group_tile.hpp"

namespace xamd {

using namespace group_tile;

// CLS: 0 f32, 1 bf16, 2 f64.  FUSED: the ext ABI's epilogue per segment (libxsmm_hip_gemm_ext_batch_reduce_segments); d_list[s] and mask_list[s] are wave-uniform
// like c_list[s] and are read the same way.
template <int CLS, bool FUSED = false>
__device__ __forceinline__ void segments_body(const GemmGroupDesc& g, const unsigned long long* seg_ptr, const void* const* a_list, const void* const* b_list,
  void* const* c_list, unsigned long long total, const GemmSegEpilogue* ep = nullptr) {
  const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned int lane = threadIdx.x & 63u;
  const unsigned long long step = (unsigned long long)gridDim.x * 4u;
  const unsigned int tiles = (unsigned int)(g.tiles_m * g.tiles_n);
  for (unsigned long long item = (unsigned long long)blockIdx.x * 4u + wave; item < total; item += step) {
    unsigned long long s = item; unsigned int t = 0;
    if (tiles != 1) { s = item / tiles; t = (unsigned int)(item - s * tiles); }
    const unsigned int tn = t / (unsigned int)g.tiles_m, tm = t - tn * (unsigned int)g.tiles_m;
    const unsigned long long r0 = uniform_u64(((GM const unsigned long long*)seg_ptr)[s]), r1 = uniform_u64(((GM const unsigned long long*)seg_ptr)[s + 1]);
    gptr c = (gptr)list_entry((const void*)c_list, s);
    const ListChain ch{(const void*)(a_list + r0), (const void*)(b_list + r0), r1 - r0, g.a_vec4, g.b_vec16, g.b_vec8};
    if constexpr (FUSED) {
      FusedEpilogue e{(gcptr)ep->d, nullptr, ep->colbias, ep->act, ep->mask_ld};
      if (ep->colbias && ep->d_list) e.d = list_entry((const void*)ep->d_list, s);
      if (ep->act == 2) e.mask = (GM unsigned char*)list_entry((const void*)ep->mask_list, s);
      if (g.tile == 32) {
        if constexpr (CLS == 1) tile_bf16<32, true>(g, ch, c, (int)tm * 32, (int)tn * 32, lane, e); else tile_f32<32, true>(g, ch, c, (int)tm * 32, (int)tn * 32, lane, e);
      } else {
        if constexpr (CLS == 1) tile_bf16<16, true>(g, ch, c, (int)tm * 16, (int)tn * 16, lane, e); else tile_f32<16, true>(g, ch, c, (int)tm * 16, (int)tn * 16, lane, e);
      }
    } else if constexpr (CLS == 2) tile_f64(g, ch, c, (int)tm * 16, (int)tn * 16, lane);
    else if (g.tile == 32) {
      if constexpr (CLS == 1) tile_bf16<32, true>(g, ch, c, (int)tm * 32, (int)tn * 32, lane); else tile_f32<32, true>(g, ch, c, (int)tm * 32, (int)tn * 32, lane);
    } else {
      if constexpr (CLS == 1) tile_bf16<16, true>(g, ch, c, (int)tm * 16, (int)tn * 16, lane); else tile_f32<16, true>(g, ch, c, (int)tm * 16, (int)tn * 16, lane);
    }
  }
}

__global__ __launch_bounds__(256) void gemm_segments_f32_kernel(GemmGroupDesc g, const unsigned long long* __restrict__ seg_ptr, const void* const* __restrict__ a_list,
  const void* const* __restrict__ b_list, void* const* __restrict__ c_list, unsigned long long total) { segments_body<0>(g, seg_ptr, a_list, b_list, c_list, total); }
__global__ __launch_bounds__(256) void gemm_segments_bf16_kernel(GemmGroupDesc g, const unsigned long long* __restrict__ seg_ptr, const void* const* __restrict__ a_list,
  const void* const* __restrict__ b_list, void* const* __restrict__ c_list, unsigned long long total) { segments_body<1>(g, seg_ptr, a_list, b_list, c_list, total); }
__global__ __launch_bounds__(256) void gemm_segments_f64_kernel(GemmGroupDesc g, const unsigned long long* __restrict__ seg_ptr, const void* const* __restrict__ a_list,
  const void* const* __restrict__ b_list, void* const* __restrict__ c_list, unsigned long long total) { segments_body<2>(g, seg_ptr, a_list, b_list, c_list, total); }

__global__ __launch_bounds__(256) void gemm_segments_f32_fused_kernel(GemmGroupDesc g, GemmSegEpilogue e, const unsigned long long* __restrict__ seg_ptr,
  const void* const* __restrict__ a_list, const void* const* __restrict__ b_list, void* const* __restrict__ c_list, unsigned long long total) {
  segments_body<0, true>(g, seg_ptr, a_list, b_list, c_list, total, &e);
}
__global__ __launch_bounds__(256) void gemm_segments_bf16_fused_kernel(GemmGroupDesc g, GemmSegEpilogue e, const unsigned long long* __restrict__ seg_ptr,
  const void* const* __restrict__ a_list, const void* const* __restrict__ b_list, void* const* __restrict__ c_list, unsigned long long total) {
  segments_body<1, true>(g, seg_ptr, a_list, b_list, c_list, total, &e);
}

// a_wide: bit 0 / 1: the rows of a transposed A are multiples of 16 / 8 bytes apart (OffsetChain::va16 / va8)
template <int CLS, bool TA, bool TB>
__device__ __forceinline__ void segments_offs_tile(const GemmGroupDesc& g, const OffsetChain& ch, gptr c, int tm, int tn, unsigned int lane) {
  if constexpr (CLS == 2) tile_f64<OffsetChain, TA, TB>(g, ch, c, tm * 16, tn * 16, lane);
  else if (g.tile == 32) {
    if constexpr (CLS == 1) tile_bf16<32, true, OffsetChain, NoEpilogue, TA, TB>(g, ch, c, tm * 32, tn * 32, lane);
    else tile_f32<32, true, OffsetChain, NoEpilogue, TA, TB>(g, ch, c, tm * 32, tn * 32, lane);
  } else {
    if constexpr (CLS == 1) tile_bf16<16, true, OffsetChain, NoEpilogue, TA, TB>(g, ch, c, tm * 16, tn * 16, lane);
    else tile_f32<16, true, OffsetChain, NoEpilogue, TA, TB>(g, ch, c, tm * 16, tn * 16, lane);
  }
}
template <int CLS, bool TA, bool TB>
__device__ __forceinline__ void segments_offs_body(const GemmGroupDesc& g, int a_wide, const unsigned long long* seg_ptr, const long long* a_offs, const long long* b_offs,
  const long long* c_offs, unsigned long long total) {
  const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned int lane = threadIdx.x & 63u;
  const unsigned long long step = (unsigned long long)gridDim.x * 4u;
  const unsigned int tiles = (unsigned int)(g.tiles_m * g.tiles_n);
  for (unsigned long long item = (unsigned long long)blockIdx.x * 4u + wave; item < total; item += step) {
    unsigned long long s = item; unsigned int t = 0;
    if (tiles != 1) { s = item / tiles; t = (unsigned int)(item - s * tiles); }
    const unsigned int tn = t / (unsigned int)g.tiles_m, tm = t - tn * (unsigned int)g.tiles_m;
    const unsigned long long r0 = uniform_u64(((GM const unsigned long long*)seg_ptr)[s]), r1 = uniform_u64(((GM const unsigned long long*)seg_ptr)[s + 1]);
    gptr c = (gptr)g.c + (long long)uniform_u64(((GM const unsigned long long*)c_offs)[s]);
    const OffsetChain ch{(gcptr)g.a, (gcptr)g.b, (const void*)(a_offs + r0), (const void*)(b_offs + r0), r1 - r0, g.a_vec4, g.b_vec16, g.b_vec8, a_wide & 1, (a_wide >> 1) & 1};
    segments_offs_tile<CLS, TA, TB>(g, ch, c, (int)tm, (int)tn, lane);
  }
}

#define XAMD_OFFS_KERNEL(NAME, CLS) \
  template <bool TA, bool TB> __global__ __launch_bounds__(256) void NAME(GemmGroupDesc g, int a_wide, const unsigned long long* __restrict__ seg_ptr, \
    const long long* __restrict__ a_offs, const long long* __restrict__ b_offs, const long long* __restrict__ c_offs, unsigned long long total) { \
    segments_offs_body<CLS, TA, TB>(g, a_wide, seg_ptr, a_offs, b_offs, c_offs, total); }
XAMD_OFFS_KERNEL(gemm_segments_offs_f32_kernel, 0)
XAMD_OFFS_KERNEL(gemm_segments_offs_bf16_kernel, 1)
XAMD_OFFS_KERNEL(gemm_segments_offs_f64_kernel, 2)
#undef XAMD_OFFS_KERNEL

const char* gemm_segments_kernel_name(int cls) { return cls == 2 ? "gemm_segments_f64_kernel" : (cls == 1 ? "gemm_segments_bf16_kernel" : "gemm_segments_f32_kernel"); }

int launch_gemm_segments(const GemmGroupDesc& g, int cls, unsigned long long items, const unsigned long long* seg_ptr, const void* const* a_list,
  const void* const* b_list, void* const* c_list, void* stream) {
  if (items == 0) return 0;
  // one wave per item up to 32 768 workgroups (16 rounds of the chip's resident waves); beyond that the waves grid-stride
  const unsigned int grid = (unsigned int)std::min<unsigned long long>((items + 3) / 4, 32768ull);
  hipStream_t st = (hipStream_t)stream;
  if (cls == 2) hipLaunchKernelGGL(gemm_segments_f64_kernel, dim3(grid), dim3(256), 0, st, g, seg_ptr, a_list, b_list, c_list, items);
  else if (cls == 1) hipLaunchKernelGGL(gemm_segments_bf16_kernel, dim3(grid), dim3(256), 0, st, g, seg_ptr, a_list, b_list, c_list, items);
  else hipLaunchKernelGGL(gemm_segments_f32_kernel, dim3(grid), dim3(256), 0, st, g, seg_ptr, a_list, b_list, c_list, items);
  return (int)hipGetLastError();
}

const char* gemm_segments_fused_kernel_name(int cls) { return cls == 1 ? "gemm_segments_bf16_fused_kernel" : "gemm_segments_f32_fused_kernel"; }

int launch_gemm_segments_fused(const GemmGroupDesc& g, const GemmSegEpilogue& e, int cls, unsigned long long items, const unsigned long long* seg_ptr,
  const void* const* a_list, const void* const* b_list, void* const* c_list, void* stream) {
  if (items == 0) return 0;
  const unsigned int grid = (unsigned int)std::min<unsigned long long>((items + 3) / 4, 32768ull);     // the plain launch's rule
  hipStream_t st = (hipStream_t)stream;
  if (cls == 1) hipLaunchKernelGGL(gemm_segments_bf16_fused_kernel, dim3(grid), dim3(256), 0, st, g, e, seg_ptr, a_list, b_list, c_list, items);
  else hipLaunchKernelGGL(gemm_segments_f32_fused_kernel, dim3(grid), dim3(256), 0, st, g, e, seg_ptr, a_list, b_list, c_list, items);
  return (int)hipGetLastError();
}

// forms: bit 0 TRANS_A, bit 1 TRANS_B (the kernel instance); bits 2 / 3: a_wide
const char* gemm_segments_offs_kernel_name(int cls, int forms) {
  static const char* const names[3][4] = {
    {"gemm_segments_offs_f32_kernel<0,0>", "gemm_segments_offs_f32_kernel<1,0>", "gemm_segments_offs_f32_kernel<0,1>", "gemm_segments_offs_f32_kernel<1,1>"},
    {"gemm_segments_offs_bf16_kernel<0,0>", "gemm_segments_offs_bf16_kernel<1,0>", "gemm_segments_offs_bf16_kernel<0,1>", "gemm_segments_offs_bf16_kernel<1,1>"},
    {"gemm_segments_offs_f64_kernel<0,0>", "gemm_segments_offs_f64_kernel<1,0>", "gemm_segments_offs_f64_kernel<0,1>", "gemm_segments_offs_f64_kernel<1,1>"}};
  return names[cls][forms & 3];
}

template <bool TA, bool TB>
static void launch_offs_form(const GemmGroupDesc& g, int a_wide, int cls, unsigned int grid, hipStream_t st, unsigned long long items, const unsigned long long* seg_ptr,
  const long long* a_offs, const long long* b_offs, const long long* c_offs) {
  if (cls == 2) hipLaunchKernelGGL((gemm_segments_offs_f64_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, g, a_wide, seg_ptr, a_offs, b_offs, c_offs, items);
  else if (cls == 1) hipLaunchKernelGGL((gemm_segments_offs_bf16_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, g, a_wide, seg_ptr, a_offs, b_offs, c_offs, items);
  else hipLaunchKernelGGL((gemm_segments_offs_f32_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, g, a_wide, seg_ptr, a_offs, b_offs, c_offs, items);
}

int launch_gemm_segments_offs(const GemmGroupDesc& g, int forms, int cls, unsigned long long items, const unsigned long long* seg_ptr, const long long* a_offs,
  const long long* b_offs, const long long* c_offs, void* stream) {
  if (items == 0) return 0;
  const unsigned int grid = (unsigned int)std::min<unsigned long long>((items + 3) / 4, 32768ull);     // the plain launch's rule
  hipStream_t st = (hipStream_t)stream;
  const int a_wide = (forms >> 2) & 3;
  switch (forms & 3) {
    case 0: launch_offs_form<false, false>(g, a_wide, cls, grid, st, items, seg_ptr, a_offs, b_offs, c_offs); break;
    case 1: launch_offs_form<true, false>(g, a_wide, cls, grid, st, items, seg_ptr, a_offs, b_offs, c_offs); break;
    case 2: launch_offs_form<false, true>(g, a_wide, cls, grid, st, items, seg_ptr, a_offs, b_offs, c_offs); break;
    default: launch_offs_form<true, true>(g, a_wide, cls, grid, st, items, seg_ptr, a_offs, b_offs, c_offs); break;
  }
  return (int)hipGetLastError();
}

}  // namespace xamd
