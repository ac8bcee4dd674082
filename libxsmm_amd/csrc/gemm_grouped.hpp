// gemm_grouped.hpp -- what runtime.cpp and gemm_grouped_kernels.hip share for the FUSED grouped launches (libxsmm_hip_gemm_ext_batch_grouped and the group
// plans).  The plain table entry (GemmGroupDesc, internal.hpp) keeps its 144 bytes; the epilogue of a fused group is a parallel entry with the same index.
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
// Fused tables of up to this many groups travel in the kernel arguments: 18 x (144 + 48) bytes are the 3456 bytes of the plain form's 24 x 144.
// (gemm_grouped_kernels.hip asserts that the argument block stays within the 4 KiB segment)
constexpr int kGroupedFusedInline = 18;

// table / epi: device copies (groups ordered by `first`)
int launch_gemm_grouped_fused(const GemmGroupDesc* table, const GemmGroupEpi* epi, int ngroups, unsigned long long items, int bf16, void* stream);
// host tables, copied into the kernel arguments
int launch_gemm_grouped_fused_inline(const GemmGroupDesc* host_table, const GemmGroupEpi* host_epi, int ngroups, unsigned long long items, int bf16, void* stream);
const char* gemm_grouped_fused_kernel_name(int bf16);

}  // namespace xamd
