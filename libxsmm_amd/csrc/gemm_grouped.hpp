// gemm_grouped.hpp -- what runtime.cpp and gemm_grouped_kernels.hip share for the grouped launches (libxsmm_hip_gemm_batch_grouped,
// libxsmm_hip_gemm_ext_batch_grouped and the group plans).  The table entry (GemmGroupDesc, internal.hpp: the segment kernels read one as well) keeps its 144
// bytes; the epilogue of a fused group is a parallel entry with the same index.
#pragma once
#include "internal.hpp"

namespace xamd {

// The ext ABI's epilogue of one group [ref: src/generator_gemm_reference_impl.c:294-372]: element e of the group reads its m-vector bias (C's type) at
// d + e * sd and writes its ReLU bitmask block at mask + e * smask.
struct GemmGroupEpi {
  const char* d; char* mask;                        // `d.primary` / `c.secondary` of the group's element 0
  long long sd, smask;                              // element byte strides (0: shared)
  int colbias, act, mask_ld;                        // act: 0 none, 1 ReLU, 2 ReLU + bitmask, 3 sigmoid; mask_ld = ldc rounded up to 16
  int pad_;
};
static_assert(sizeof(GemmGroupEpi) == 48, "the fused grouped kernels' epilogue entry");
// Host tables of up to this many groups travel in the kernel arguments: 24 x 144 bytes plain, and fused 18 x (144 + 48) bytes, the same 3456 bytes.
// (gemm_grouped_kernels.hip asserts that the argument block stays within the 4 KiB segment)
constexpr int kGroupedInline = 24;
constexpr int kGroupedFusedInline = 18;

// One launch of a class: `table` holds the groups ordered by `first`, `epi` the parallel epilogue entries of a fused class (NULL: a plain class).
struct GroupedLaunch {
  const GemmGroupDesc* table; const GemmGroupEpi* epi;
  int ngroups;
  unsigned long long items;                         // work items of the whole table
  int bf16;
  bool host;                                        // the tables are host copies for the kernel arguments (at most the inline limit of groups); else device copies
};
// *kname: the pointer-table kernel of bf16 x fused, whichever form carries the table
int launch_gemm_grouped(const GroupedLaunch& l, void* stream, const char** kname);

}  // namespace xamd
