"""The dense parity checks of tests/gemm_ld_helpers.py checked on the reference's restatement alone (no GPU): the masks are right, the per-element bound
holds for the oracle's own serial f32 / f64 loop, the checks reject localized errors, and the old whole-batch bar did not.

Worst err / bound of the oracle's output over CASES, per type (recorded from this test; every one must stay <= 1):
    f32 0.141   f64 0.216   bf16 -> bf16 0.988   bf16 -> f32 0.014   f16 -> f16 0.771   f16 -> f32 0.057   E5M2 -> f32 0.026   E4M3 -> f32 0.072   8-bit integers exact
(a 16-bit C comes close to 1: a result just above a power of two is rounded by almost the whole unit round-off u_c |ref| the bound grants)."""
import copy

import numpy as np
import pytest

from gemm_ld_helpers import assert_dense, logical_c, poison, ref64, _a_index, _b_index, _c_index, _gap_of, _operands
from helpers import GemmCase, TOL_BF16, as_float, normf_rel
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG as F

MXMX = F.VNNI_A | F.VNNI_B | F.TRANS_B
# one case per layout logical_masks knows, lda / ldb / ldc all padded
CASES = {
    "f32_flat": dict(m=17, n=9, k=31, lda=20, ldb=33, ldc=19, beta=1, batch=3),
    "f32_trans_a": dict(m=13, n=7, k=5, lda=8, ldb=6, ldc=15, flags=F.TRANS_A, batch=2, br_type=capi.BR_STRIDE, br_count=3),
    "f32_trans_b": dict(m=13, n=7, k=5, lda=14, ldb=9, ldc=16, flags=F.TRANS_B, beta=1, batch=2, br_type=capi.BR_OFFSET, br_count=3),
    "f32_bias_relu_mask": dict(m=20, n=12, k=16, lda=24, ldb=17, ldc=21, colbias=True, act=2, beta=1, batch=3),
    "f64_trans_ab": dict(m=10, n=12, k=14, lda=15, ldb=13, ldc=11, a_type=DT.F64, flags=F.TRANS_A | F.TRANS_B, batch=2, br_type=capi.BR_ADDRESS, br_count=2),
    "f64_flat": dict(m=23, n=17, k=9, lda=24, ldb=11, ldc=25, a_type=DT.F64, beta=1, batch=3),
    "bf16_vnni_a": dict(m=40, n=40, k=40, lda=44, ldb=42, ldc=41, a_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A, batch=37),
    "bf16_vnni_a_f32": dict(m=33, n=17, k=18, lda=36, ldb=20, ldc=40, a_type=DT.BF16, c_type=DT.F32, flags=F.VNNI_A, beta=1, batch=3, br_type=capi.BR_ADDRESS, br_count=2),
    "bf16_flat": dict(m=12, n=10, k=9, lda=13, ldb=11, ldc=14, a_type=DT.BF16, c_type=DT.BF16, beta=1, batch=2),
    "bf16_trans_a": dict(m=12, n=10, k=8, lda=9, ldb=12, ldc=13, a_type=DT.BF16, c_type=DT.BF16, flags=F.TRANS_A, batch=2),
    "bf16_vnni_b": dict(m=12, n=10, k=8, lda=14, ldb=12, ldc=13, a_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A | F.TRANS_B | F.VNNI_B, batch=2, colbias=True, act=1),
    "bf16_vnni_c": dict(m=16, n=5, k=8, lda=18, ldb=10, ldc=20, a_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A | F.VNNI_C, batch=3),
    "f16_vnni_a": dict(m=17, n=7, k=16, lda=20, ldb=24, ldc=24, a_type=DT.F16, c_type=DT.F16, flags=F.VNNI_A, beta=1, colbias=True, act=2, batch=3),
    "f16_f32_beta1": dict(m=33, n=17, k=18, lda=34, ldb=19, ldc=35, a_type=DT.F16, c_type=DT.F32, flags=F.VNNI_A, beta=1, batch=3, br_type=capi.BR_STRIDE, br_count=2),
    "f16_vnni_c": dict(m=17, n=7, k=16, lda=20, ldb=24, ldc=24, a_type=DT.F16, c_type=DT.F16, flags=F.VNNI_A | F.VNNI_C, batch=3),
    "bf8_vnni4_f32": dict(m=23, n=37, k=20, lda=25, ldb=21, ldc=29, a_type=DT.BF8, c_type=DT.F32, flags=F.VNNI_A, beta=1, batch=3),
    "hf8_flat_f32": dict(m=12, n=10, k=7, lda=13, ldb=9, ldc=14, a_type=DT.HF8, c_type=DT.F32, batch=2, colbias=True, act=1),
    "hf8_vnni_c": dict(m=17, n=7, k=16, lda=20, ldb=24, ldc=24, a_type=DT.HF8, c_type=DT.HF8, flags=F.VNNI_C, batch=3),
    "bf8_c8": dict(m=17, n=9, k=12, lda=18, ldb=13, ldc=20, a_type=DT.BF8, c_type=DT.BF8, flags=F.VNNI_A, beta=1, batch=2),
    "i8u8_vnni4": dict(m=23, n=37, k=20, lda=25, ldb=21, ldc=29, a_type=DT.I8, b_type=DT.U8, c_type=DT.I32, flags=F.VNNI_A, beta=1, batch=3),
    "u8i8_flat": dict(m=12, n=10, k=7, lda=13, ldb=9, ldc=14, a_type=DT.U8, b_type=DT.I8, c_type=DT.I32, batch=2),
    "u8i8_f32_scaled": dict(m=64, n=32, k=160, lda=72, ldb=176, ldc=80, a_type=DT.U8, b_type=DT.I8, c_type=DT.F32, scf=0.25, beta=1, batch=2),
    "bf32_flat": dict(m=17, n=9, k=31, lda=20, ldb=33, ldc=19, a_type=DT.BF32, beta=1, batch=2, colbias=True, act=2),
    "mxfp4_bf16": dict(m=33, n=5, k=64, lda=34, ldb=66, ldc=35, a_type=DT.MXFP4X2, b_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A, batch=2, br_type=capi.BR_STRIDE, br_count=2),
    "mxfp4_f32": dict(m=17, n=9, k=64, lda=20, ldb=65, ldc=24, a_type=DT.MXFP4X2, b_type=DT.F32, c_type=DT.F32, flags=F.VNNI_A, beta=1, batch=2),
    "mxmx_fp4": dict(m=17, n=9, k=64, lda=20, ldb=12, ldc=24, a_type=DT.MXFP4X2, b_type=DT.MXFP4X2, c_type=DT.F32, flags=MXMX, beta=1, batch=2),
    "mxmx_bf8": dict(m=32, n=96, k=64, lda=40, ldb=100, ldc=36, a_type=DT.MXBF8, b_type=DT.MXBF8, c_type=DT.F32, flags=MXMX, batch=2),
    "mxmx_hf8": dict(m=33, n=5, k=32, lda=34, ldb=7, ldc=37, a_type=DT.MXHF8, b_type=DT.MXHF8, c_type=DT.F32, flags=MXMX, batch=2),
}
REF64 = [n for n, kw in CASES.items() if ref64(GemmCase(seed=1, **dict(kw, batch=1))) is not None]
PLAIN64 = [n for n in REF64 if not CASES[n].get("act") and not CASES[n].get("flags", 0) & F.VNNI_C]     # mutations 1 / 2 need results that are not clamped to 0


def _case(name, seed=2024):
    return GemmCase(seed=seed, **CASES[name])


def _encode(x, dt, like):
    """float64 / int64 values -> C's storage type (one round-to-nearest-even)."""
    if dt == DT.BF16:
        u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
        return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    if dt == DT.F16:
        return np.asarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)
    return np.asarray(x).astype(like.dtype)


HALF = {DT.F32: 0.5, DT.F64: 0.5, DT.BF16: 0x3f00, DT.F16: 0x3800, DT.BF8: 0x38, DT.HF8: 0x30, DT.I8: 3, DT.U8: 3}     # 0.5 in each type (integers: 3)


def _poisoned(name):
    """The case with its gaps poisoned and B(k - 1, n - 1) of every block non-zero, so that mutation 2 never drops a zero."""
    case = _case(name)
    poison(case)
    case.B.reshape(-1, case.b_elems)[:, _b_index(case)[-1, -1]] = HALF[case.b_type]
    return case


def _rejected(case, got, ref):
    with pytest.raises(AssertionError):
        assert_dense(case, got, ref)
    return True


@pytest.mark.parametrize("name", list(CASES))
def test_masks_are_the_elements_the_reference_reads(name):
    """The oracle's result on the poisoned case equals its result on the unpoisoned one bit for bit inside m x n (no gap is read: a NaN here is a wrong mask),
    and outside m x n it leaves the sentinel (VNNI_C: the zeros of its re-layout, pad columns included)."""
    clean = _case(name)
    dirty = _case(name)
    mk = poison(dirty)
    for buf in ("A", "B", "C0"):
        gaps = ~mk[buf]
        assert gaps.any(), f"{name}: {buf} has no gap -- the case does not pad it"
        assert np.array_equal(getattr(clean, buf)[mk[buf]], getattr(dirty, buf)[mk[buf]])
    r0, m0 = clean.run_oracle()
    r1, m1 = dirty.run_oracle()
    assert np.array_equal(logical_c(clean, r0).view(np.uint8), logical_c(dirty, r1).view(np.uint8))
    if m0 is not None:
        assert np.array_equal(clean.valid_mask_bits(m0), dirty.valid_mask_bits(m1))
    out = r1[~mk["C0"]]
    want = np.zeros_like(out) if clean.flags & F.VNNI_C else np.full_like(out, _gap_of(dirty.c_type, out))
    assert np.array_equal(out.view(np.uint8), want.view(np.uint8))
    if dirty.c_type not in (DT.I32,):
        assert np.all(np.isfinite(as_float(logical_c(dirty, r1), dirty.c_type)))
    assert_dense(dirty, r1, r1, got_mask=m1)             # every case: the oracle passes its own check


def test_the_bound_holds_for_the_reference_itself():
    """assert_dense accepts the oracle's own output with no element outside the bound, for every ref64 type; the worst ratios are in the module docstring."""
    worst = {}
    for name in REF64:
        case = _case(name)
        poison(case)
        ref, rmask = case.run_oracle()
        stats = {}
        assert_dense(case, ref, ref, got_mask=rmask, stats=stats)
        key = (case.a_type, case.c_type)
        worst[key] = max(worst.get(key, 0.0), stats["ratio"])
    print({f"{a}->{c}": round(v, 3) for (a, c), v in worst.items()})
    assert {k[0] for k in worst} >= {DT.F32, DT.F64, DT.BF16, DT.F16, DT.BF8, DT.HF8, DT.I8}
    assert max(worst.values()) <= 1.0


def _last_k_term(case):
    """float64 [m] products A(i, k-1) B(k-1, n-1) of the LAST batch-reduce block the last problem consumes."""
    conv = (lambda x, dt: x.astype(np.int64)) if case.c_type == DT.I32 else as_float
    A, B, _ = _operands(case, conv)
    return A[-1, -1, :, -1] * B[-1, -1, -1, -1]


def _mutate_last_element(case, ref):
    got = ref.copy()
    got.reshape(case.batch, -1)[-1, _c_index(case)[-1, -1]] = 0
    return got


def _mutate_drop_last_k(case, ref):
    got = ref.copy()
    col = _c_index(case)[-1]
    last = got.reshape(case.batch, -1)[-1]
    cur = last[col].astype(np.int64) if case.c_type == DT.I32 else as_float(last[col], case.c_type)
    last[col] = _encode(cur - _last_k_term(case), case.c_type, got)
    return got


@pytest.mark.parametrize("name", PLAIN64)
def test_localized_errors_in_the_result_are_rejected(name):
    """mutations 1 and 2: the last element of the last problem zeroed; the last k term missing from the last column of the last problem."""
    case = _poisoned(name)
    ref, _ = case.run_oracle()
    assert_dense(case, ref, ref)
    assert logical_c(case, ref)[-1, -1, -1] != 0 and np.any(_last_k_term(case) != 0)
    assert _rejected(case, _mutate_last_element(case, ref), ref)
    assert _rejected(case, _mutate_drop_last_k(case, ref), ref)


@pytest.mark.parametrize("name", list(CASES))
def test_a_write_into_the_gap_of_c_is_rejected(name):
    """mutation 3: one element outside m x n changed by one bit (every case, the ones on the oracle's bar included)."""
    case = _case(name)
    mk = poison(case)
    ref, _ = case.run_oracle()
    got = ref.copy()
    gap = np.flatnonzero(~mk["C0"])[-1]
    got.view(np.uint8)[gap * got.itemsize] ^= 1
    assert _rejected(case, got, ref)


@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("name", REF64)
def test_a_gap_element_used_for_its_logical_neighbour_is_rejected(name, operand):
    """mutation 4: the output a kernel produces that reads the gap element next to the last logical row (A) / column or k (B) instead of that element."""
    case = _case(name)
    mk = poison(case)
    ref, _ = case.run_oracle()
    wrong = copy.copy(case)
    buf = getattr(case, operand).copy()
    idx = (_a_index(case)[-1, 0] if operand == "A" else _b_index(case)[0, -1])         # A(m-1, 0) / B(0, n-1) of the first block of the first problem
    gap = np.flatnonzero(~mk[operand])[0]
    buf[idx] = buf[gap]
    setattr(wrong, operand, buf)
    got, _ = wrong.run_oracle()
    assert not np.array_equal(got, ref)
    assert _rejected(case, got, ref)


def test_the_old_whole_batch_bar_accepts_localized_errors():
    """Why this exists: for the bf16 40^3, batch 37 case of test_ragged_16bit_shapes_on_the_masked_matrix_core_kernel, mutations 1 and 2 pass the whole-batch
    normf_rel < TOL_BF16 that was the only check of the 16-bit kernels -- and assert_dense rejects both."""
    case = GemmCase(m=40, n=40, k=40, a_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A, batch=37, seed=77)
    ref, _ = case.run_oracle()
    for mutate in (_mutate_last_element, _mutate_drop_last_k):
        got = mutate(case, ref)
        assert not np.array_equal(got, ref)
        old = normf_rel(case.valid_region(ref), case.valid_region(got), DT.BF16)
        print(mutate.__name__, old)
        assert 0 < old < TOL_BF16
        assert _rejected(case, got, ref)


def test_every_dense_kernel_name_in_the_sources_has_a_padded_row_or_a_reason():
    """Every quoted gemm_*_kernel name string of the dense sources is either reached by a row of tests/test_gemm_ld_gpu.py: DENSE (asserted there by name on the GPU) or
    listed in its UNREACHABLE with the reason: a kernel name added to the dispatcher fails here until it has one or the other."""
    import glob
    import os
    import re
    from test_gemm_ld_gpu import DENSE, UNREACHABLE
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libxsmm_amd", "csrc")
    files = [os.path.join(csrc, "gemm_kernels.hip")] + [p for pat in ("gemm_wgp*", "gemm_w64*", "gemm_small*", "gemm_sharedb*", "gemm_f64*", "gemm_bitmask*", "gemm_lean*")
                                                        for p in glob.glob(os.path.join(csrc, pat))]
    names = set()
    for path in files:
        names |= set(re.findall(r'"(gemm_[a-z0-9_]+_kernel(?:_lean)?(?:<[0-9,]+>)?)"', open(path).read()))
    assert len(names) > 60, sorted(names)
    rows = {k for k, _ in DENSE}
    assert not (names - rows - set(UNREACHABLE)), sorted(names - rows - set(UNREACHABLE))
    assert not (rows & set(UNREACHABLE)), sorted(rows & set(UNREACHABLE))
    assert not (rows - names), sorted(rows - names)          # a row names a kernel that exists
    assert all(len(why) > 20 for why in UNREACHABLE.values())
