"""The semantics of libxsmm_hip_gemm_ext_batch_reduce_segments_sliced / ..._offsets_sliced (include/libxsmm_hip.h) restated on the CPU, on top of
tests/segments_sliced_helpers.py.

Per C block: the start value of the unsliced ext entries in numpy.float32 -- bias[i]; bias[i] + C(i,j) as one add of the widened values; C(i,j); or +0 -- then
acc = acc + P_j for the block's slices in ascending order, one numpy.float32 add each (IEEE, denormals kept), P_j being slice_partial's chain from +0 (for f32
the k-ordered fmaf chain); mask bit i % 8 of byte i / 8 + j * (mask_ld / 8) is !(acc <= 0), packed little-endian into a copy of the caller's mask block for
i < m, j < n only; ReLU is np.where(x <= 0, +0, x), sigmoid the oracle's SIGMOID TPP on the f32 pre-activation; a bf16 C is rounded once with f32_to_bf16.  A
block without slices stores the activation of its start value and its mask, for every beta."""
import ctypes as C

import numpy as np

from helpers import bf16_to_f32
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, UNARY
from oracle import pyoracle
from segments_sliced_helpers import f32_to_bf16, partial_case, slice_partial


def widen(x, c_type):
    """Values of C's type as float32."""
    return bf16_to_f32(np.ascontiguousarray(x)).reshape(x.shape).astype(np.float32) if c_type == DT.BF16 else np.asarray(x, dtype=np.float32)


def start_value(case, beta, c_view, bias):
    """[n][m] float32: `c_view` is the block's valid part as stored, `bias` the m-vector of C's type or None."""
    c0 = widen(c_view, case.c_type)
    if bias is None:
        return c0.copy() if beta else np.zeros((case.n, case.m), dtype=np.float32)
    b = widen(bias[:case.m], case.c_type)[None, :]
    return (b + c0) if beta else np.broadcast_to(b, (case.n, case.m)).copy()


def oracle_sigmoid(x):
    """The oracle's SIGMOID TPP, f32 -> f32, on a 2-D array."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, m = x.shape
    out = np.zeros_like(x)
    p = capi.UnaryParam()
    p.in_.primary, p.out.primary = x.ctypes.data, out.ctypes.data
    d = pyoracle.MeltwDesc(m, n, m, m, 0, 0, DT.F32, DT.UNSUPPORTED, DT.UNSUPPORTED, DT.F32, DT.F32, 0, UNARY.SIGMOID, 1)
    pyoracle.oracle().meltw(p, d)
    return out


def mask_of(case, mask_block, acc):
    """A copy of the caller's mask block with the bits of i < m, j < n set to !(acc <= 0)."""
    out = mask_block.copy()
    rows = out[:case.mask_bytes].reshape(case.n, case.mask_ld // 8)
    bits = np.unpackbits(rows, axis=1, bitorder="little")
    bits[:, :case.m] = ~(acc <= 0)
    rows[...] = np.packbits(bits, axis=1, bitorder="little")
    return out


def activation(act, acc):
    if act in (1, 2):
        return np.where(acc <= 0, np.float32(0.0), acc)
    if act == 3:
        return oracle_sigmoid(acc)
    return acc


def sliced_fused_reference(case, beta, colbias, act, blk_ptr, seg_ptr, param_of_slice, c_blocks, bias_of_block, mask_blocks, fma=True, partial=None):
    """`c_blocks` / `mask_blocks`: one 1-D array per block, the original C (C's type) and mask bytes; `bias_of_block(b)`: the m-vector of C's type; returns
    (C blocks, mask blocks) after the call.  `param_of_slice(j)` as in sliced_reference.  `partial(j, count)`, when given, replaces slice_partial (the test of
    the definition against the reference passes the reference's own kernel)."""
    pcase = partial_case(case)
    outc, outm = [], []
    for b, c0 in enumerate(c_blocks):
        blk = c0.copy()
        view = blk[:case.ldc * case.n].reshape(case.n, case.ldc)[:, :case.m]
        acc = start_value(case, beta, view, bias_of_block(b) if colbias else None)
        for j in range(int(blk_ptr[b]), int(blk_ptr[b + 1])):
            count = int(seg_ptr[j + 1]) - int(seg_ptr[j])
            P = partial(j, count) if partial is not None else slice_partial(pcase, param_of_slice(j), count, fma)
            acc = acc + P                                                           # one float32 add per element and slice, ascending
            assert acc.dtype == np.float32
        outm.append(mask_of(case, mask_blocks[b], acc) if act == 2 else mask_blocks[b].copy())
        y = activation(act, acc)
        view[:] = f32_to_bf16(y).reshape(case.n, case.m) if case.c_type == DT.BF16 else y
        outc.append(blk)
    return outc, outm
