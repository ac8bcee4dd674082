// gemm_grouped_kernels.hip -- libxsmm_hip_gemm_batch_grouped, libxsmm_hip_gemm_ext_batch_grouped and the group plans: strided batches of SEVERAL (BR)GEMM
// shapes in one launch, plain or with the ext ABI's epilogue in the store.  Eight kernels (f32 / bf16 x plain / fused x pointer table / table in the
// arguments) behind one launcher (launch_gemm_grouped, gemm_grouped.hpp).
//
// The host (runtime.cpp) builds one GemmGroupDesc per eligible group -- operands of element 0, element and batch-reduce strides, the shape, the C tile edge
// chosen for it and the exclusive prefix of its work items -- and hands the table over in the kernel arguments, uploaded for the call, or resident (a plan).  A work item is (group, element, C tile); every wave owns one item at a
// time and grid-strides over the rest.  The wave finds its group by a binary search over the prefix column of the table: the item index is wave-uniform, so
// the table is read with scalar loads.  Operands go straight from memory to registers; a wave's tile is private (no LDS, no barrier).
//
// The tile bodies (operands swapped into the MFMA, k in natural order so that f32 is the k-ordered fmaf chain bit for bit, clamped loads, -0 / +0 padding of
// ragged k) are gemm_group_tile.hpp, shared with the segment kernels; here a tile walks a STRIDE batch-reduce chain (one block for plain GEMM handles).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <type_traits>
#include "internal.hpp"
#include "gemm_device.hpp"
#include "bf16_cvt.hpp"
#include "gemm_group_tile.hpp"
#include "gemm_grouped.hpp"

namespace xamd {

using namespace group_tile;

// EpiTable: the parallel table of the fused launches (GemmGroupEpi, gemm_grouped.hpp: libxsmm_hip_gemm_ext_batch_grouped, the group plans); NoEpiTable: the
// plain kernels, whose instances are what they were before the parameter existed (every use of the table sits behind `if constexpr`).
struct NoEpiTable {};
template <typename T> struct is_no_epi { static constexpr bool value = false; };
template <> struct is_no_epi<NoEpiTable> { static constexpr bool value = true; };

template <bool BF16, typename Table, typename EpiTable = NoEpiTable>
__device__ __forceinline__ void grouped_body(const Table& groups, int ngroups, unsigned long long total, const EpiTable& epis = EpiTable()) {
  const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned int lane = threadIdx.x & 63u;
  const unsigned long long step = (unsigned long long)gridDim.x * 4u;
  for (unsigned long long item = (unsigned long long)blockIdx.x * 4u + wave; item < total; item += step) {
    int lo = 0, hi = ngroups - 1;                // the last group whose first item is <= item (wave-uniform: scalar loads)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (groups[mid].first <= item) lo = mid; else hi = mid - 1;
    }
    const GemmGroupDesc g = groups[lo];
    const unsigned int local = (unsigned int)(item - g.first);        // the host keeps every group below 2^32 items
    const unsigned int tiles = (unsigned int)(g.tiles_m * g.tiles_n);
    const unsigned int e = local / tiles, t = local - e * tiles;
    const unsigned int tm = t % (unsigned int)g.tiles_m, tn = t / (unsigned int)g.tiles_m;
    gcptr a = (gcptr)g.a + (long long)e * g.sa;
    gcptr b = (gcptr)g.b + (long long)e * g.sb;
    gptr c = (gptr)g.c + (long long)e * g.sc;
    const StrideChain ch = stride_chain(g, a, b);
    // one tile call for both forms: the plain kernels pass NoEpilogue (their instances are what they were), the fused ones the element's epilogue
    const auto run_tile = [&](const auto& ep) {
      typedef typename std::remove_cv<typename std::remove_reference<decltype(ep)>::type>::type Epi;
      if (g.tile == 32) {
        if constexpr (BF16) tile_bf16<32, false, StrideChain, Epi>(g, ch, c, (int)tm * 32, (int)tn * 32, lane, ep); else tile_f32<32, false, StrideChain, Epi>(g, ch, c, (int)tm * 32, (int)tn * 32, lane, ep);
      } else {
        if constexpr (BF16) tile_bf16<16, false, StrideChain, Epi>(g, ch, c, (int)tm * 16, (int)tn * 16, lane, ep); else tile_f32<16, false, StrideChain, Epi>(g, ch, c, (int)tm * 16, (int)tn * 16, lane, ep);
      }
    };
    if constexpr (is_no_epi<EpiTable>::value) run_tile(NoEpilogue());
    else {
      // bias and mask block of element e of the group -- the group and the element are the wave's, so every member is wave-uniform
      const GemmGroupEpi ge = epis[lo];
      FusedEpilogue ep;
      ep.d = (gcptr)ge.d + (long long)e * ge.sd;
      ep.mask = (GM unsigned char*)ge.mask + (long long)e * ge.smask;
      ep.colbias = ge.colbias; ep.act = ge.act; ep.mask_ld = ge.mask_ld;
      run_tile(ep);
    }
  }
}

// The table travels in the kernel arguments when it fits (kGroupedInline groups, 3.4 KiB of the 4 KiB argument segment): it arrives with the dispatch packet,
// where an upload is one more command on the stream that the kernel waits for (measured: 7 us of a 14 us call of one 13^3 x 4096 group).  Longer tables
// are uploaded (stage_host) and read through a pointer.  Either way the wave-uniform reads are scalar loads.
struct GroupedInline { GemmGroupDesc g[kGroupedInline]; };
__global__ __launch_bounds__(256) void gemm_grouped_f32_kernel(const GemmGroupDesc* __restrict__ groups, int ngroups, unsigned long long total) { grouped_body<false>(groups, ngroups, total); }
__global__ __launch_bounds__(256) void gemm_grouped_bf16_kernel(const GemmGroupDesc* __restrict__ groups, int ngroups, unsigned long long total) { grouped_body<true>(groups, ngroups, total); }
__global__ __launch_bounds__(256) void gemm_grouped_f32_inline_kernel(GroupedInline tab, int ngroups, unsigned long long total) { grouped_body<false>(tab.g, ngroups, total); }
__global__ __launch_bounds__(256) void gemm_grouped_bf16_inline_kernel(GroupedInline tab, int ngroups, unsigned long long total) { grouped_body<true>(tab.g, ngroups, total); }

// The fused forms: the same body with FusedEpilogue tiles; the epilogue entries ride next to the group entries, in the arguments (kGroupedFusedInline groups)
// or behind a second pointer.
struct GroupedFusedInline { GemmGroupDesc g[kGroupedFusedInline]; GemmGroupEpi e[kGroupedFusedInline]; };
static_assert(sizeof(GroupedFusedInline) + 16 + 256 <= 4096, "the inline fused table, ngroups, total and the hidden arguments must fit the 4 KiB kernel argument segment");
__global__ __launch_bounds__(256) void gemm_grouped_f32_fused_kernel(const GemmGroupDesc* __restrict__ groups, const GemmGroupEpi* __restrict__ epis, int ngroups, unsigned long long total) {
  grouped_body<false>(groups, ngroups, total, epis);
}
__global__ __launch_bounds__(256) void gemm_grouped_bf16_fused_kernel(const GemmGroupDesc* __restrict__ groups, const GemmGroupEpi* __restrict__ epis, int ngroups, unsigned long long total) {
  grouped_body<true>(groups, ngroups, total, epis);
}
__global__ __launch_bounds__(256) void gemm_grouped_f32_fused_inline_kernel(GroupedFusedInline tab, int ngroups, unsigned long long total) { grouped_body<false>(tab.g, ngroups, total, tab.e); }
__global__ __launch_bounds__(256) void gemm_grouped_bf16_fused_inline_kernel(GroupedFusedInline tab, int ngroups, unsigned long long total) { grouped_body<true>(tab.g, ngroups, total, tab.e); }

// The one launcher: the instance of bf16 x fused x inline, picked once.  The name reported is the pointer-table kernel's for the inline form too.
int launch_gemm_grouped(const GroupedLaunch& l, void* stream, const char** kname) {
  static const char* const kNames[4] = {"gemm_grouped_f32_kernel", "gemm_grouped_bf16_kernel", "gemm_grouped_f32_fused_kernel", "gemm_grouped_bf16_fused_kernel"};
  const bool fused = l.epi != nullptr;
  *kname = kNames[(fused ? 2 : 0) + (l.bf16 ? 1 : 0)];
  if (l.ngroups <= 0 || l.items == 0) return 0;
  if (l.host && l.ngroups > (fused ? kGroupedFusedInline : kGroupedInline)) return (int)hipErrorInvalidValue;
  const dim3 grid(group_grid(l.items)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (!l.host) {
    if (fused) {
      if (l.bf16) hipLaunchKernelGGL(gemm_grouped_bf16_fused_kernel, grid, block, 0, st, l.table, l.epi, l.ngroups, l.items);
      else hipLaunchKernelGGL(gemm_grouped_f32_fused_kernel, grid, block, 0, st, l.table, l.epi, l.ngroups, l.items);
    } else if (l.bf16) hipLaunchKernelGGL(gemm_grouped_bf16_kernel, grid, block, 0, st, l.table, l.ngroups, l.items);
    else hipLaunchKernelGGL(gemm_grouped_f32_kernel, grid, block, 0, st, l.table, l.ngroups, l.items);
  } else if (fused) {
    GroupedFusedInline tab;
    std::memset(&tab, 0, sizeof(tab));
    std::memcpy(tab.g, l.table, (size_t)l.ngroups * sizeof(GemmGroupDesc));
    std::memcpy(tab.e, l.epi, (size_t)l.ngroups * sizeof(GemmGroupEpi));
    if (l.bf16) hipLaunchKernelGGL(gemm_grouped_bf16_fused_inline_kernel, grid, block, 0, st, tab, l.ngroups, l.items);
    else hipLaunchKernelGGL(gemm_grouped_f32_fused_inline_kernel, grid, block, 0, st, tab, l.ngroups, l.items);
  } else {
    GroupedInline tab;
    std::memset(&tab, 0, sizeof(tab));
    std::memcpy(tab.g, l.table, (size_t)l.ngroups * sizeof(GemmGroupDesc));
    if (l.bf16) hipLaunchKernelGGL(gemm_grouped_bf16_inline_kernel, grid, block, 0, st, tab, l.ngroups, l.items);
    else hipLaunchKernelGGL(gemm_grouped_f32_inline_kernel, grid, block, 0, st, tab, l.ngroups, l.items);
  }
  return (int)hipGetLastError();
}

}  // namespace xamd
