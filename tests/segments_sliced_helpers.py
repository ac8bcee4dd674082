"""The semantics of libxsmm_hip_gemm_batch_reduce_segments_sliced / ..._offsets_sliced (include/libxsmm_hip.h) restated on the CPU, for the tests of both.

Per C block: every slice is ONE accumulator chain over (product, k) in list order, started at +0, in the accumulator type -- the oracle's chain that the
unsliced segments tests use (for f32 the k-ordered fmaf chain), run with beta = 0 into a dense m x n block of the accumulator type; the block's partials are
then added in ascending slice order, one numpy add of the accumulator type each (IEEE, denormals kept), onto C widened to the accumulator type (beta = 1) or
onto +0 (beta = 0); the sum is stored with one rounding for a bf16 C.  A block without slices stores +0 under beta = 0 and stays untouched under beta = 1."""
import ctypes as C

import numpy as np

from helpers import GemmCase, bf16_to_f32
from libxsmm_amd.capi import DT, GEMM_FLAG
from oracle import pyoracle

# per block [0, 1, 2, 3, 9] slices; products per slice from {0, 1, 2, 7, 19} with an empty slice first (block 2), in the middle (blocks 3, 4) and last (block 4)
SLICES_PER_BLOCK = [0, 1, 2, 3, 9]
PRODUCTS_PER_SLICE = [7, 0, 19, 2, 0, 1, 19, 1, 0, 7, 2, 2, 1, 7, 0]


def csr(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.uint64))]).astype(np.uint64)


def acc_type(case):
    return DT.F64 if case.a_type == DT.F64 else DT.F32


def partial_case(case):
    """The problem one slice is: the handle's operands and layouts, beta = 0, C of the accumulator type and dense (ldc = m)."""
    return GemmCase(case.m, case.n, case.k, a_type=case.a_type, c_type=acc_type(case), lda=case.lda, ldb=case.ldb, ldc=case.m,
                    flags=case.flags & ~GEMM_FLAG.BETA_0, beta=0, br_type=case.br_type, br_count=1, batch=1)


def f32_to_bf16(x):
    """The library's f32 -> bf16 [ref: src/libxsmm_math.c:684-704]: denormals become signed zeros first, NaNs are quieted, everything else rounds to nearest even."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = np.where((u & 0x7f800000) == 0, u & 0x80000000, u)
    nan = ((u & 0x7f800000) == 0x7f800000) & ((u & 0x007fffff) != 0)
    rounded = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u | 0x00400000) >> 16, rounded).astype(np.uint16)


def slice_partial(pcase, param, count, fma):
    """P of one slice: `param` names the slice's first list entries (and, OFFSET, the bases); c.primary and op.tertiary are set here."""
    acc = np.float64 if pcase.c_type == DT.F64 else np.float32
    P = np.full(pcase.m * pcase.n, 7.0, dtype=acc)                               # beta = 0: overwritten, also by a slice of no products (+0)
    cnt = C.c_ulonglong(int(count))
    param.c.primary, param.op.tertiary = P.ctypes.data, C.addressof(cnt)
    pyoracle.oracle().gemm(param, pcase.oracle_desc(), fma=fma and pcase.a_type == DT.F32)
    return P.reshape(pcase.n, pcase.m)


def sliced_reference(case, beta, blk_ptr, seg_ptr, param_of_slice, c_blocks, fma=True):
    """`c_blocks`: one 1-D array of C's type (at least ldc * n elements) per block, the original C; returns the blocks after the call.  `param_of_slice(j)` is a
    fresh GemmParam whose a / b slots name the lists of slice j as a single call of the handle reads them."""
    pcase = partial_case(case)
    acc = np.float64 if pcase.c_type == DT.F64 else np.float32
    out = []
    for b, c0 in enumerate(c_blocks):
        blk = c0.copy()
        j0, j1 = int(blk_ptr[b]), int(blk_ptr[b + 1])
        out.append(blk)
        if j0 == j1 and beta:
            continue
        view = blk[:case.ldc * case.n].reshape(case.n, case.ldc)[:, :case.m]
        if not beta:
            s = np.zeros((case.n, case.m), dtype=acc)
        else:
            s = bf16_to_f32(view).reshape(case.n, case.m).copy() if case.c_type == DT.BF16 else view.astype(acc)
        for j in range(j0, j1):
            P = slice_partial(pcase, param_of_slice(j), int(seg_ptr[j + 1]) - int(seg_ptr[j]), fma)
            s = s + P                                                               # one add of the accumulator type per element and slice, ascending
            assert s.dtype == acc
        view[:] = f32_to_bf16(s).reshape(case.n, case.m) if case.c_type == DT.BF16 else s
    return out
