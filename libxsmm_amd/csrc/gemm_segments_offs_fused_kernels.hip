// gemm_segments_offs_fused_kernels.hip -- libxsmm_hip_gemm_ext_batch_reduce_segments_offsets: OFFSET batch-reduce segments (gemm_segments_kernels.hip) through an
// ext handle, the column bias, the ReLU (+ bitmask) or the sigmoid applied per segment inside the one launch [ref: src/generator_gemm_reference_impl.c:294-372,
// :509-513, :186-188].
//
// The work items, their order and the chain are those of gemm_segments_offs_*_kernel: item = segment * tiles + tile, one wave per item, grid-stride, an
// OffsetChain over a_offs / b_offs from the two bases in the GemmGroupDesc, the transposes as template parameters (four instances per class; DESIGN.md section
// 9.2 has what runtime bits cost).  The tiles take the FusedEpilogue of the ADDRESS fused kernels unchanged -- it holds two POINTERS, and where they come from is
// this unit's business: the bias block of segment s is d + d_offs[s] (d_offs == NULL: d itself, shared), its mask block mask + mask_offs[s].  The two offsets are
// wave-uniform like c_offs[s] and are read with the same scalar 64-bit loads, issued next to it; the two bases and the operator bits travel by value in a
// GemmSegOffsEpilogue next to the GemmGroupDesc.  No LDS, no barrier, no scratch; C and the mask bytes leave through vector stores (acc_relu_mask: a whole byte
// when its 8 rows are valid, read-merge-write for the byte that holds row m - 1).  This unit is a translation unit of its own: the eight instances would double
// the compile of gemm_segments_kernels.hip, and the kernels there stay byte for byte what they were.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "internal.hpp"
#include "gemm_device.hpp"
#include "bf16_cvt.hpp"
#include "gemm_group_tile.hpp"

namespace xamd {

using namespace group_tile;

// CLS: 0 f32, 1 bf16
template <int CLS, bool TA, bool TB>
__device__ __forceinline__ void segments_offs_fused_body(const GemmGroupDesc& g, const GemmSegOffsEpilogue& ep, const unsigned long long* seg_ptr, const long long* a_offs,
  const long long* b_offs, const long long* c_offs, unsigned long long total) {
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
    FusedEpilogue e{(gcptr)ep.d, nullptr, ep.colbias, ep.act, ep.mask_ld};
    if (ep.colbias && ep.d_offs) e.d += (long long)uniform_u64(((GM const unsigned long long*)ep.d_offs)[s]);
    if (ep.act == 2) e.mask = (GM unsigned char*)ep.mask + (long long)uniform_u64(((GM const unsigned long long*)ep.mask_offs)[s]);
    const OffsetChain ch{(gcptr)g.a, (gcptr)g.b, (const void*)(a_offs + r0), (const void*)(b_offs + r0), r1 - r0, g.a_vec4, g.b_vec16, g.b_vec8, ep.a_wide & 1, (ep.a_wide >> 1) & 1};
    if (g.tile == 32) {
      if constexpr (CLS == 1) tile_bf16<32, true, OffsetChain, FusedEpilogue, TA, TB>(g, ch, c, (int)tm * 32, (int)tn * 32, lane, e);
      else tile_f32<32, true, OffsetChain, FusedEpilogue, TA, TB>(g, ch, c, (int)tm * 32, (int)tn * 32, lane, e);
    } else {
      if constexpr (CLS == 1) tile_bf16<16, true, OffsetChain, FusedEpilogue, TA, TB>(g, ch, c, (int)tm * 16, (int)tn * 16, lane, e);
      else tile_f32<16, true, OffsetChain, FusedEpilogue, TA, TB>(g, ch, c, (int)tm * 16, (int)tn * 16, lane, e);
    }
  }
}

#define XAMD_OFFS_FUSED_KERNEL(NAME, CLS) \
  template <bool TA, bool TB> __global__ __launch_bounds__(256) void NAME(GemmGroupDesc g, GemmSegOffsEpilogue e, const unsigned long long* __restrict__ seg_ptr, \
    const long long* __restrict__ a_offs, const long long* __restrict__ b_offs, const long long* __restrict__ c_offs, unsigned long long total) { \
    segments_offs_fused_body<CLS, TA, TB>(g, e, seg_ptr, a_offs, b_offs, c_offs, total); }
XAMD_OFFS_FUSED_KERNEL(gemm_segments_offs_f32_fused_kernel, 0)
XAMD_OFFS_FUSED_KERNEL(gemm_segments_offs_bf16_fused_kernel, 1)
#undef XAMD_OFFS_FUSED_KERNEL

// forms: bit 0 TRANS_A, bit 1 TRANS_B (the kernel instance)
const char* gemm_segments_offs_fused_kernel_name(int cls, int forms) {
  static const char* const names[2][4] = {
    {"gemm_segments_offs_f32_fused_kernel<0,0>", "gemm_segments_offs_f32_fused_kernel<1,0>", "gemm_segments_offs_f32_fused_kernel<0,1>", "gemm_segments_offs_f32_fused_kernel<1,1>"},
    {"gemm_segments_offs_bf16_fused_kernel<0,0>", "gemm_segments_offs_bf16_fused_kernel<1,0>", "gemm_segments_offs_bf16_fused_kernel<0,1>", "gemm_segments_offs_bf16_fused_kernel<1,1>"}};
  return names[cls == 1 ? 1 : 0][forms & 3];
}

template <bool TA, bool TB>
static void launch_offs_fused_form(const GemmGroupDesc& g, const GemmSegOffsEpilogue& e, int cls, unsigned int grid, hipStream_t st, unsigned long long items,
  const unsigned long long* seg_ptr, const long long* a_offs, const long long* b_offs, const long long* c_offs) {
  if (cls == 1) hipLaunchKernelGGL((gemm_segments_offs_bf16_fused_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, g, e, seg_ptr, a_offs, b_offs, c_offs, items);
  else hipLaunchKernelGGL((gemm_segments_offs_f32_fused_kernel<TA, TB>), dim3(grid), dim3(256), 0, st, g, e, seg_ptr, a_offs, b_offs, c_offs, items);
}

int launch_gemm_segments_offs_fused(const GemmGroupDesc& g, const GemmSegOffsEpilogue& e, int forms, int cls, unsigned long long items, const unsigned long long* seg_ptr,
  const long long* a_offs, const long long* b_offs, const long long* c_offs, void* stream) {
  if (items == 0) return 0;
  const unsigned int grid = (unsigned int)std::min<unsigned long long>((items + 3) / 4, 32768ull);     // the plain launch's rule
  hipStream_t st = (hipStream_t)stream;
  switch (forms & 3) {
    case 0: launch_offs_fused_form<false, false>(g, e, cls, grid, st, items, seg_ptr, a_offs, b_offs, c_offs); break;
    case 1: launch_offs_fused_form<true, false>(g, e, cls, grid, st, items, seg_ptr, a_offs, b_offs, c_offs); break;
    case 2: launch_offs_fused_form<false, true>(g, e, cls, grid, st, items, seg_ptr, a_offs, b_offs, c_offs); break;
    default: launch_offs_fused_form<true, true>(g, e, cls, grid, st, items, seg_ptr, a_offs, b_offs, c_offs); break;
  }
  return (int)hipGetLastError();
}

}  // namespace xamd
