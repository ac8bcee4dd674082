"""The BCSC parity checks of tests/bcsc_parity_helpers.py checked on the reference's loop alone (no GPU): the bound holds for the oracle's own serial float32
accumulation on every row of tests/test_bcsc_parity_gpu.py: BCSC (M-blocks capped at 8), the integer restatement equals it exactly, assert_bcsc rejects planted
errors, and every BCSC kernel name of the source has a row or a reason.

Worst err / bound of the oracle over the rows, per type (recorded from test_the_bound_holds_for_the_reference_on_every_row; every one must stay <= 1):
    bf16 -> bf16 0.993   bf16 -> f32 0.170   f32 0.253   8-bit integers exact
(a bf16 C comes close to 1: a result just above a power of two is rounded by almost the whole unit round-off u_c |ref| the bound grants)."""
import os
import re

import numpy as np
import pytest

from bcsc_parity_helpers import BcscCase, assert_bcsc, bound_of, pristine_margins, ref64, wide
from helpers import as_float, f32_to_bf16_trunc
from libxsmm_amd.capi import DT
from test_bcsc_parity_gpu import BCSC, UNREACHABLE, _id

MB_CAP = 8


def _case(kw):
    return BcscCase(**dict(kw, mb=min(kw.get("mb", 3), MB_CAP)))


def _rejected(case, got, margins=None):
    with pytest.raises(AssertionError):
        assert_bcsc(case, got, margins if margins is not None else pristine_margins(case))
    return True


def test_wide_values_are_what_the_helper_promises():
    rng = np.random.default_rng(3)
    for dt, bits in ((DT.BF16, 7), (DT.F32, 23)):
        v = wide(rng, 1 << 16, dt)
        x = as_float(v, dt)
        nz = x[x != 0]
        assert np.all(np.isfinite(x)) and abs(np.mean(x == 0) - 0.125) < 0.01 and abs(np.mean(nz < 0) - 0.5) < 0.02
        e = np.floor(np.log2(np.abs(nz))).astype(int)
        assert e.min() == -8 and e.max() == 8 and np.bincount(e + 8).min() > 0.8 * nz.size / 17
        raw = v.astype(np.uint32) if dt == DT.BF16 else v.view(np.uint32)
        sig = raw[x != 0] & ((1 << bits) - 1)
        assert all(0.45 < np.mean((sig >> b) & 1) < 0.55 for b in range(bits))                  # every bit of the significand is used
        assert not np.any(v.view(np.uint16 if dt == DT.BF16 else np.uint32)[x == 0])            # the zeros are +0


def test_the_bound_holds_for_the_reference_on_every_row():
    """Float rows: the oracle's serial float32 loop passes assert_bcsc with ratio <= 1; integer rows: it equals the int64 restatement."""
    worst = {}
    for kernel, kw in BCSC:
        case = _case(kw)
        stats = {}
        assert_bcsc(case, case.run_oracle(), pristine_margins(case), stats)
        key = (case.a_type, case.c_type)
        worst[key] = max(worst.get(key, 0.0), stats["ratio"])
        assert stats["ratio"] <= 1.0, _id((kernel, kw))
    print({f"{a}->{c}": round(v, 3) for (a, c), v in worst.items()})
    assert set(worst) == {(DT.BF16, DT.BF16), (DT.BF16, DT.F32), (DT.F32, DT.F32), (DT.U8, DT.I32), (DT.I8, DT.I32)}
    assert worst[(DT.U8, DT.I32)] == 0 and worst[(DT.I8, DT.I32)] == 0


def test_the_rows_carry_the_pattern_edges():
    """Per matrix-core kernel: a block column with every k-block, one with none, one stored in descending order; first and last k-block in use; per family a pattern
    without any block; never a duplicate row index in a column (BcscCase asserts that)."""
    seen, nnz0 = {}, set()
    for kernel, kw in BCSC:
        case = _case(kw)
        nkb = case.K // case.bk
        s = seen.setdefault((kernel, "i8" if case.ints else case.a_type), set())
        s |= {"full"} if any(len(c) == nkb for c in case.cols) and case.nnzb else set()
        s |= {"empty"} if any(len(c) == 0 for c in case.cols) and case.nnzb else set()
        s |= {"descending"} if any(len(c) > 1 and c == sorted(c, reverse=True) for c in case.cols) else set()
        s |= {"first"} if any(0 in c for c in case.cols) else set()
        s |= {"last"} if any(nkb - 1 in c for c in case.cols) else set()
        if case.nnzb == 0:
            nnz0.add("i8" if case.ints else case.a_type)
    for (kernel, fam), s in seen.items():
        if "mfma" in kernel:
            assert s == {"full", "empty", "descending", "first", "last"}, (kernel, fam, s)
    assert nnz0 == {DT.BF16, DT.F32, "i8"}


# ---- planted errors --------------------------------------------------------------------------------------------------------------------------------------------------
# beta = 1 and beta = 0, every C type; each with an empty column, a column of several blocks and several M-blocks
PLANT = {
    "bf16_bf16_beta1": dict(a_type=DT.BF16, M=48, N=64, K=128, mb=4, beta=1),
    "bf16_f32_beta0": dict(a_type=DT.BF16, c_type=DT.F32, M=32, N=96, K=128, bn=32, mb=3),
    "f32_beta1": dict(a_type=DT.F32, M=32, N=64, K=64, bk=16, mb=3, beta=1),
    "u8_beta0": dict(a_type=DT.U8, M=32, N=64, K=128, mb=3),
    "i8_beta1": dict(a_type=DT.I8, M=32, N=64, K=128, mb=3, beta=1),
}


def _plant(name):
    case = BcscCase(seed=99, **PLANT[name])
    ref = case.run_oracle()
    assert_bcsc(case, ref, pristine_margins(case))
    return case, ref


def _full_column(case):
    """(block column, its first element column n) of a column with at least two blocks."""
    nb = next(i for i, c in enumerate(case.cols) if len(c) >= 2)
    return nb, nb * case.bn


@pytest.mark.parametrize("name", [n for n in PLANT if PLANT[n].get("c_type", PLANT[n]["a_type"]) == DT.F32])
def test_an_element_moved_by_twice_its_bound_is_rejected(name):
    """(f32 C: the moved value is stored without a second rounding that could take part of the move back)"""
    case, ref = _plant(name)
    ref3, bound = ref64(case)[0], bound_of(case)
    got = ref.copy().reshape(ref3.shape)
    at = (case.mb - 1, case.N - 1, case.M - 1)
    got[at] = np.float32(ref3[at] + 2.0 * bound[at])
    assert _rejected(case, got.reshape(-1))
    got[at] = ref.reshape(ref3.shape)[at]
    assert_bcsc(case, got.reshape(-1), pristine_margins(case))


@pytest.mark.parametrize("name", list(PLANT))
def test_an_m_block_with_its_neighbours_result_is_rejected(name):
    case, ref = _plant(name)
    got = ref.copy().reshape(case.mb, -1)
    got[1] = got[0]
    assert _rejected(case, got.reshape(-1))


@pytest.mark.parametrize("name", list(PLANT))
def test_a_k_block_left_out_of_one_column_in_one_m_block_is_rejected(name):
    case, ref = _plant(name)
    nb, _ = _full_column(case)
    drop = int(case.colptr[nb + 1]) - 1                                          # the column's last stored block
    colptr = case.colptr.copy(); colptr[nb + 1:] -= 1
    rowidx = np.delete(case.rowidx, drop)
    bvals = np.delete(case.bvals.reshape(-1, case.bn * case.bk), drop, axis=0).reshape(-1)
    last = slice(case.mb - 1, case.mb)
    got = ref.copy().reshape(case.mb, -1)
    got[-1] = case.run_oracle(colptr=colptr, rowidx=rowidx, bvals=bvals, blocks=last)
    assert not np.array_equal(got.reshape(-1), ref)
    assert _rejected(case, got.reshape(-1))


@pytest.mark.parametrize("name", list(PLANT))
def test_two_exchanged_blocks_of_one_column_are_rejected(name):
    case, ref = _plant(name)
    nb, _ = _full_column(case)
    b0 = int(case.colptr[nb])
    bvals = case.bvals.copy().reshape(-1, case.bn * case.bk)
    bvals[[b0, b0 + 1]] = bvals[[b0 + 1, b0]]
    got = case.run_oracle(bvals=bvals.reshape(-1))
    assert not np.array_equal(got, ref)
    assert _rejected(case, got)


def test_bf16_results_truncated_instead_of_rounded_are_rejected():
    case, ref = _plant("bf16_bf16_beta1")
    sums = case.run_oracle(c_type=DT.F32, C0=as_float(case.C0, DT.BF16).astype(np.float32))        # the same float32 sums, not yet rounded
    got = f32_to_bf16_trunc(sums)
    assert 0 < np.mean(got != ref) < 0.6
    assert _rejected(case, got)


@pytest.mark.parametrize("which", ["A", "B", "C"])
@pytest.mark.parametrize("side", [0, 1])
def test_one_changed_margin_byte_is_rejected(which, side):
    case, ref = _plant("bf16_bf16_beta1")
    margins = pristine_margins(case)
    margins[which][side][-1 if side == 0 else 0] ^= 1                            # the byte next to the array
    assert _rejected(case, ref, margins)


@pytest.mark.parametrize("name", list(PLANT))
def test_a_result_in_an_empty_column_that_is_not_exactly_its_start_value_is_rejected(name):
    """One unit in the last place (integers: 1) off 0 / the start value: for f32 C, and for a zero, that is inside the bound, so only the exact check can see it."""
    case, ref = _plant(name)
    n = next(i for i, c in enumerate(case.cols) if len(c) == 0) * case.bn
    got = ref.copy().reshape(case.mb, case.N, case.M)
    at = (1, n, 1)
    if case.c_type == DT.I32:
        got[at] += 1
    elif case.c_type == DT.BF16:
        got[at] = got[at] + 1 if case.beta else 0x0001
    else:
        got[at] = np.nextafter(got[at], np.float32(np.inf)) if case.beta else np.float32(2.0 ** -127)
    if case.c_type == DT.F32 or (case.c_type == DT.BF16 and not case.beta):      # inside the bound, which alone would accept it (one bf16 step off a start value is not)
        moved = abs(float(as_float(got, case.c_type)[at]) - float(ref64(case)[0][at]))
        assert np.isfinite(moved) and moved <= bound_of(case)[at]
    assert _rejected(case, got.reshape(-1))


def test_every_bcsc_kernel_name_in_the_source_has_a_row_or_a_reason():
    """Every quoted bcsc_*_kernel name string of csrc/bcsc_plan.hpp is the expected name of a row of BCSC (asserted there by name on the GPU) or is listed in
    UNREACHABLE with the reason: a kernel name added to plan_bcsc fails here until it has one or the other."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libxsmm_amd", "csrc", "bcsc_plan.hpp")
    names = set(re.findall(r'"(bcsc_[a-z0-9_]+_kernel)"', open(path).read()))
    assert len(names) >= 11, sorted(names)
    rows = {k for k, _ in BCSC}
    assert not (names - rows - set(UNREACHABLE)), sorted(names - rows - set(UNREACHABLE))
    assert not (rows & set(UNREACHABLE)), sorted(rows & set(UNREACHABLE))
    assert not (rows - names), sorted(rows - names)                              # a row names a kernel that exists
    assert all(len(why) > 20 for why in UNREACHABLE.values())
