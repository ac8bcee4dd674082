"""What tests/test_gemm_grouped_fused_cpu.py and tests/test_gemm_grouped_fused_gpu.py share: the case lists of the grouped tests with the epilogues of the ext
grouped call on them, the expected bytes of an f32 group (the k-ordered fmaf chain started at the bias, FusedSegments.fma_chain's composition for a strided
batch), and the mask bits that the float64 bound decides."""
import copy

import numpy as np

import gemm_ld_helpers as ld
import helpers
from helpers import GemmCase
from libxsmm_amd.capi import DT, GEMM_FLAG
from test_gemm_grouped_gpu import BF16_CASES, F32_CASES

# (colbias, act): bias + ReLU + bitmask, bias only, ReLU only, bias + sigmoid -- rotated over the f32 list
EPILOGUES = [(True, 2), (True, 0), (False, 1), (True, 3)]
SHARED_BIAS = 4                               # index into F32_CASES of the group whose bias is shared by its elements (stride_d = 0): padded ld, bias + ReLU + bitmask


def share_bias(case):
    """Every element reads element 0's bias: the host copy repeats it, so the oracle (which steps the bias) computes the same."""
    case.D = np.tile(case.D[:case.m], case.batch)
    return case


def f32_cases():
    out = []
    for i, kw in enumerate(F32_CASES):
        colbias, act = EPILOGUES[i % len(EPILOGUES)]
        case = GemmCase(colbias=colbias, act=act, **kw)
        if i == SHARED_BIAS:
            assert colbias
            share_bias(case)
        out.append(case)
    return out


def bf16_cases(exact=False):
    """BF16_CASES with bias + ReLU + bitmask; exact: small-integer operands, bias included (any summation order gives the same bits)."""
    out = []
    for i, kw in enumerate(BF16_CASES):
        case = GemmCase(colbias=True, act=2, **kw)
        if exact:
            rng = np.random.default_rng(300 + i)
            ints = lambda n: rng.integers(-1, 2, n).astype(np.float32)
            conv = lambda x, dt: helpers.f32_to_bf16_trunc(x) if dt == DT.BF16 else x
            case.A, case.B = conv(ints(case.A.size), DT.BF16), conv(ints(case.B.size), DT.BF16)
            case.C0, case.D = conv(ints(case.C0.size), case.c_type), conv(ints(case.D.size), case.c_type)
        out.append(case)
    return out


def mask_prefill(case, seed):
    return np.random.default_rng(seed).integers(0, 256, case.batch * case.mask_bytes).astype(np.uint8)


def fma_chain(case, C0, M0):
    """f32: the expected C and mask bytes from the unchanged oracle -- bias (+ C0, one f32 add) written into a copy of C, the (block, k)-ordered fmaf chain with
    beta = 1 on the non-ext descriptor on top of it, the mask bits !(x <= 0) set into a copy of the prefilled masks, then ReLU as np.where(x <= 0, +0, x).
    (Sigmoid groups: the chain BEFORE the activation -- their C is compared with the ext oracle under a tolerance.)"""
    assert case.a_type == DT.F32 and case.c_type == DT.F32
    beta = not (case.flags & GEMM_FLAG.BETA_0)
    plain = copy.copy(case)
    plain.ext, plain.colbias, plain.act = False, False, 0
    plain.flags = case.flags & ~GEMM_FLAG.BETA_0
    plain.C0 = C0.copy()
    v = case.valid_region(plain.C0)
    assert np.shares_memory(v, plain.C0)
    start = v.copy() if beta else np.zeros_like(v)
    if case.colbias:
        bias = case.D.reshape(case.batch, 1, case.m)
        start = (bias + start) if beta else np.broadcast_to(bias, v.shape)
    v[...] = start
    ref, _ = plain.run_oracle(fma=True)
    v = case.valid_region(ref)
    assert np.shares_memory(v, ref)
    msk = None
    if case.act == 2:
        msk = M0.copy()
        rows = msk.reshape(case.batch, case.n, case.mask_ld // 8)
        bits = np.unpackbits(rows, axis=2, bitorder="little")
        bits[:, :, :case.m] = ~(v <= 0)
        rows[...] = np.packbits(bits, axis=2, bitorder="little")
    if case.act in (1, 2):
        v[...] = np.where(v <= 0, np.float32(0.0), v)
    return ref, msk


def decided_mask_bits(case):
    """(decided, positive) as [batch][n][m]: where the float64 restatement of the pre-activation sum lies outside its rounding bound, and its sign there."""
    pre, mag, terms = ld._ref64_pre(case)
    _, bound_pre = ld.bound64(case, pre, mag, terms)
    return np.abs(pre) > bound_pre, pre > 0
