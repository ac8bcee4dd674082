"""The yardstick of tests/test_meltw_reduce_gpu.py, proven without a GPU (tests/meltw_reduce_helpers.py).

  * the oracle (oracle/oracle_meltw.c: reduce) passes the per-output sum bound and equals exact()'s MAX / MIN / ABSMAX bit for bit, for every type, direction,
    input and output type, with and without REDUCE_INIT_ACC, at every shape of the GPU file, on wide and infinite data -- no case excluded;
  * where oracle/_ref is built, the oracle equals the reference itself bit for bit on those cases at the two smallest shapes of each direction, and on column
    MAX / ABSMAX over data with NaN (the operand order of the reference's MAX decides there);
  * six localized errors, injected into the oracle's results, are rejected by the checks.  What the former bar of tests/test_meltw_gpu.py (rand_values data:
    multiples of 0.1 in [-0.4, 0.5], padding of the same kind, ldo = m, no start values; normf_rel < 1e-5 over the result vector for sums, array_equal for
    MAX / MIN / ABSMAX) says to the same errors on its own data:
        1  MAX / MIN over rows started at -FLT_MAX / FLT_MAX                      accepted (its data hold no infinity)
        2  the last 4-row vector of one column left out of a sum                  rejected
        3  one padding row folded into a MAX                                      accepted (0.5 is in every column already)
        4  the x^2 results written at out + m where they belong at out + ldo      accepted (ldo = m in every case it runs)
        5  the start value added twice                                            rejected -- had it ever set REDUCE_INIT_ACC for f32 / bf16
        6  one chunk of a two-pass partial dropped for one row group              rejected
    What the bound does NOT see: it is a worst-case bound over every summation order, and the oracle's serial sums use only a small part of it (the ratio test
    below asks for no more than 1e-4 of it).  An error smaller than (k + 1) 2^-24 sum |x| passes: error 2 is injected into the column where the dropped four rows
    carry most of sum |x|; the same vector dropped from a column where it is of ordinary magnitude among k = 64 terms of mixed scale, or made of dust, can stay
    inside the bound.  The poisoned padding, the bit-exact serial paths and the cancelling lines (two large opposite values in dust) are what catch such errors.
  * expected_reduce_kernel against a hand-written table at the boundaries of launch_meltw's conditions."""
import numpy as np
import pytest

import meltw_reduce_helpers as rh
from meltw_ew_helpers import FLT_MAX, bits_of, same_bits
from meltw_reduce_helpers import ADD_T, ALL_T, CASES, CMP_T, ROWS_TAGS, ReduceCase, case_id
from libxsmm_amd.capi import DT, UNARY, UNARY_FLAG

R, Cc = UNARY_FLAG.REDUCE_ROWS, UNARY_FLAG.REDUCE_COLS


def _variants(c):
    """(in_dt, out_dt, init) of one shape: F32 results throughout, BF16 and F16 results on the first shape of each path."""
    outs = (DT.F32, DT.BF16, DT.F16) if rh.first_of_path(c) else (DT.F32,)
    return [(i, o, init) for i in (DT.F32, DT.BF16) for o in outs for init in (False, True)]


@pytest.mark.parametrize("typ", ALL_T, ids=lambda t: f"t{t}")
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_oracle_is_inside_the_bound_and_equals_the_exact_extremum(c, typ):
    tag, m, n, ldi, off, batch = c
    for in_dt, out_dt, init in _variants(c):
        for data in ("wide", "infinite"):
            case = ReduceCase(typ, m, n, ldi, tag in ROWS_TAGS, in_dt, out_dt, init=init, batch=batch, off=off, data=data, seed=m + n)
            case.check(case.run_oracle(), what=f"oracle {case_id(c)} t{typ} in{in_dt} out{out_dt} init{int(init)} {data}")


def test_bound_leaves_the_oracle_no_more_room_than_its_derivation():
    """the oracle's serial f32 sums use a fair share of the bound on cancelling data -- the bound is not a loose one that anything would pass."""
    stats = {}
    for typ in ADD_T:
        case = ReduceCase(typ, 4100, 3, 4104, True, DT.F32, DT.F32, data="wide", seed=1)
        case.check(case.run_oracle(), stats=stats)
    assert 1e-4 < stats["ratio"] <= 1.0, stats


def _smallest(rows):
    own = [c for c in CASES if (c[0] in ROWS_TAGS) == rows]
    return sorted(own, key=lambda c: c[1] * c[2])[:2]


@pytest.mark.parametrize("typ", ALL_T, ids=lambda t: f"t{t}")
@pytest.mark.parametrize("rows", [True, False], ids=["rows", "cols"])
def test_oracle_equals_the_reference(reference, rows, typ):
    for c in _smallest(rows):
        tag, m, n, ldi, off, batch = c
        for in_dt, out_dt, init in [(i, o, k) for i in (DT.F32, DT.BF16) for o in (DT.F32, DT.BF16, DT.F16) for k in (False, True)]:
            for data in ("wide", "infinite"):
                case = ReduceCase(typ, m, n, ldi, rows, in_dt, out_dt, init=init, batch=batch, off=off, data=data, seed=3 + m)
                mine, theirs = case.run_oracle(), case.run_reference(reference)
                ok = same_bits(theirs[case.out_mask], mine[case.out_mask], out_dt)
                assert ok.all(), (case_id(c), typ, in_dt, out_dt, init, data, int(np.flatnonzero(~ok)[0]))


@pytest.mark.parametrize("typ", [UNARY.REDUCE_X_OP_MAX, UNARY.REDUCE_X_OP_ABSMAX], ids=["max", "absmax"])
def test_oracle_equals_the_reference_on_a_column_maximum_that_reads_nan(reference, typ):
    """MAX(x, acc) = x < acc ? acc : x takes a NaN x and drops a NaN acc at the next column: the result is the maximum of what follows the row's last NaN."""
    m, n, ldi = 33, 33, 40
    rng = np.random.default_rng(9)
    x = rh.wide(rng, n, m, DT.F32, False)
    x[rng.random((n, m)) < 0.1] = np.nan
    x[n - 1, 5] = np.nan                                   # a NaN in the last column stays
    case = ReduceCase(typ, m, n, ldi, False, data=x[None])
    mine, theirs = case.run_oracle(), case.run_reference(reference)
    assert np.isnan(mine[5]) and np.isfinite(mine[case.out_mask]).sum() > m // 2
    assert same_bits(theirs[case.out_mask], mine[case.out_mask], DT.F32).all()


# ---- the injected errors ----------------------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _rejected(case, got):
    try:
        case.check(got)
    except AssertionError:
        return True
    return False


def _old_bar(case, good, bad):
    """the former bar on the case's results (f32)."""
    return rh.old_bar_accepts(case.typ, good[case.out_mask], bad[case.out_mask])


def _mutate(name, case, out):
    """the oracle's output allocation `out` of `case` with error `name` injected (f32 results, one matrix)."""
    got = out.copy()
    X = case.logical(0)                                    # [n][m]
    m, n = case.m, case.n
    if name == "rows_start_flt_max":
        got[:n] = np.maximum(got[:n], -FLT_MAX) if case.typ == UNARY.REDUCE_X_OP_MAX else np.minimum(got[:n], FLT_MAX)
    elif name == "tail_vector_dropped":                    # the column where those four rows carry most of the sum: a dropped vector of dust is invisible to any bound
        tails = X[:, m - 4:].sum(axis=1)
        j = int(np.argmax(np.abs(tails) / np.abs(X).sum(axis=1)))
        got[j] = _f32(got[j] - _f32(tails[j]))
    elif name == "padding_row_in_max":
        j = n // 2
        pad = rh.load64(case.in_buf[case.front + j * case.ldi + m: case.front + j * case.ldi + m + 1], case.in_dt)[0]
        got[j] = max(got[j], np.float32(pad))
    elif name == "x2_at_out_plus_m":
        good2 = out[case.x2_at: case.x2_at + m].copy()
        got[:] = case.out_buf
        got[:m], got[m: 2 * m] = out[:m], good2
    elif name == "init_twice":
        got[case.out_mask] = _f32(got[case.out_mask] + case.out_buf[case.out_mask])
    elif name == "chunk_dropped":                          # chunk 7 of 32 (66 columns) missing from the row group of rows 8 .. 11
        got[8:12] = _f32(got[8:12] - _f32(X[7 * 66: 8 * 66, 8:12].sum(axis=0)))
    else:
        raise ValueError(name)
    return got


MUTANTS = {
    # name: (type, m, n, ldi, rows, init, data of the new check, whether the former bar accepts it, the former bar's own case: (m, n, ldi, ldo))
    "rows_start_flt_max": (UNARY.REDUCE_X_OP_MAX, 64, 20, 64, True, False, "infinite", True, (75, 33, 80, None)),
    "tail_vector_dropped": (UNARY.REDUCE_X_OP_ADD, 64, 20, 64, True, False, "wide", False, (64, 20, 64, None)),
    "padding_row_in_max": (UNARY.REDUCE_X_OP_MAX, 75, 33, 80, True, False, "wide", True, (75, 33, 80, None)),
    "x2_at_out_plus_m": (UNARY.REDUCE_X_X2_OP_ADD, 64, 20, 64, False, False, "wide", True, (64, 20, 64, 64)),
    "init_twice": (UNARY.REDUCE_X_OP_ADD, 33, 33, 40, False, True, "wide", False, (33, 33, 40, None)),
    "chunk_dropped": (UNARY.REDUCE_X_OP_ADD, 64, 2100, 64, False, False, "wide", False, (64, 2100, 64, None)),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_checks_reject_the_injected_error(name):
    typ, m, n, ldi, rows, init, data, old_accepts, old_shape = MUTANTS[name]
    case = ReduceCase(typ, m, n, ldi, rows, init=init, data=data, seed=17)
    good = case.run_oracle()
    case.check(good)
    bad = _mutate(name, case, good)
    assert not np.array_equal(bits_of(good), bits_of(bad)), "the mutation changed nothing"
    assert _rejected(case, bad)
    if name == "rows_start_flt_max":                       # ... and the mirrored MIN over +inf
        mn = ReduceCase(UNARY.REDUCE_X_OP_MIN, m, n, ldi, rows, data=data, seed=17)
        assert _rejected(mn, _mutate(name, mn, mn.run_oracle()))
    # the former bar, on the data and the layout of the tests that apply it
    om, on, oldi, oldo = old_shape
    old = ReduceCase(typ, om, on, oldi, rows, init=init, data="tame", seed=17, ldo=oldo)
    if init:                                               # tame start values too
        from helpers import rand_values
        old.out_buf[old.out_mask] = rand_values(np.random.default_rng(18), int(old.out_mask.sum()), DT.F32)
    good = old.run_oracle()
    assert _old_bar(old, good, _mutate(name, old, good)) == old_accepts


# ---- which kernel -----------------------------------------------------------------------------------------------------------------------------------------
KERNEL_TABLE = [
    # typ-independent: (flags, m, n, ldi, in_dt, base offset, batch, stride bytes) -> (name, tag)
    ((R, 4, 63, 4, DT.F32, 0, 1, 0), ("reduce_vec_kernel", "vec-rows")),
    ((R, 4, 64, 4, DT.F32, 0, 1, 0), ("reduce_vec_kernel", "vec-rows-cpg4")),
    ((R, 12, 64, 12, DT.BF16, 0, 1, 0), ("reduce_vec_kernel", "vec-rows-cpg4")),
    ((R, 256, 64, 256, DT.F32, 0, 1, 0), ("reduce_vec_kernel", "vec-rows-cpg4")),
    ((R, 256, 63, 256, DT.F32, 0, 1, 0), ("reduce_vec_kernel", "vec-rows")),
    ((R, 260, 64, 260, DT.F32, 0, 1, 0), ("reduce_vec_kernel", "vec-rows")),            # m / 4 = 65 > G = 64
    ((R, 260, 256, 260, DT.F32, 0, 1, 0), ("reduce_vec_kernel", "vec-rows")),
    ((Cc, 4, 255, 4, DT.F32, 0, 1, 0), ("reduce_vec_kernel", "vec-cols-1slice")),
    ((Cc, 4, 256, 4, DT.F32, 0, 1, 0), ("reduce_vec_kernel", "vec-cols-16slice")),
    ((Cc, 12, 256, 12, DT.BF16, 0, 3, 12 * 256 * 2), ("reduce_vec_kernel", "vec-cols-16slice")),
    ((Cc, 260, 255, 260, DT.F32, 0, 1, 0), ("reduce_vec_kernel", "vec-cols-1slice")),
    ((Cc, 256, 63, 256, DT.F32, 0, 1, 0), ("reduce_vec_kernel", "vec-cols-1slice")),
    ((Cc, 256, 64, 256, DT.F32, 0, 1, 0), ("reduce_vec_kernel", "vec-cols-1slice")),     # n / 64 = 1 chunk, and no workspace below n = 2048 anyway
    ((Cc, 8, 2047, 8, DT.F32, 0, 1, 0), ("reduce_vec_kernel", "vec-cols-16slice")),
    ((Cc, 8, 2048, 8, DT.F32, 0, 1, 0), ("reduce_vec_kernel+combine", "two-pass")),
    ((Cc, 8, 2048, 8, DT.F32, 0, 2, 8 * 2048 * 4), ("reduce_vec_kernel", "vec-cols-16slice")),
    ((R, 8, 2048, 8, DT.F32, 0, 1, 0), ("reduce_vec_kernel", "vec-rows-cpg4")),
    ((R, 64, 6, 64, DT.F32, 1, 1, 0), ("reduce_kernel", "general-rows")),              # the base one element off
    ((Cc, 64, 6, 64, DT.F32, 1, 1, 0), ("reduce_kernel", "general-cols")),
    ((R, 64, 6, 64, DT.F32, 2, 1, 0), ("reduce_kernel", "general-rows")),              # 8 bytes: not enough for f32 ...
    ((R, 64, 6, 64, DT.BF16, 4, 1, 0), ("reduce_vec_kernel", "vec-rows")),              # ... enough for bf16
    ((R, 64, 6, 64, DT.BF16, 1, 1, 0), ("reduce_kernel", "general-rows")),
    ((R, 64, 6, 66, DT.F32, 0, 1, 0), ("reduce_kernel", "general-rows")),              # ldi % 4 != 0
    ((Cc, 64, 6, 66, DT.BF16, 0, 1, 0), ("reduce_kernel", "general-cols")),
    ((R, 63, 6, 64, DT.F32, 0, 1, 0), ("reduce_kernel", "general-rows")),
    ((R, 64, 64, 64, DT.F16, 0, 1, 0), ("reduce_kernel", "general-rows")),             # only f32 and bf16 have a vector form
    ((Cc, 64, 256, 64, DT.F16, 0, 1, 0), ("reduce_kernel", "general-cols")),
    ((Cc, 64, 6, 64, DT.F32, 0, 3, 64 * 6 * 4 + 4), ("reduce_kernel", "general-cols")),  # a batch stride that is no multiple of 16 bytes
    ((Cc, 64, 6, 64, DT.BF16, 0, 3, 64 * 6 * 2 + 8), ("reduce_vec_kernel", "vec-cols-1slice")),
]


@pytest.mark.parametrize("args,want", KERNEL_TABLE, ids=[f"{i}-{w[1]}" for i, (_, w) in enumerate(KERNEL_TABLE)])
def test_expected_reduce_kernel_against_the_table(args, want):
    for typ in ALL_T:
        assert rh.expected_reduce_kernel(typ, *args) == want


def test_every_path_has_a_case_and_every_case_its_path():
    assert {c[0] for c in CASES} == set(rh.TAGS)
    for c in CASES:
        tag, m, n, ldi, off, batch = c
        for in_dt in (DT.F32, DT.BF16):
            case = ReduceCase(UNARY.REDUCE_X_OP_ADD, m, n, ldi, tag in ROWS_TAGS, in_dt, batch=batch, off=off, seed=0)
            assert case.expected()[1] == tag, (c, in_dt, case.expected())
            assert case.in_buf.nbytes < 1.3e6


@pytest.mark.parametrize("data", ["wide", "infinite"])
@pytest.mark.parametrize("typ,listed", [(t, True) for t in rh.LISTED_T] + [(t, False) for t in CMP_T], ids=lambda v: str(int(v)))
def test_oracle_meets_the_hand_made_rows_of_the_listed_column_cases(typ, listed, data):
    for in_dt in (DT.F32, DT.BF16):
        for idx8 in (False, True):
            for record in ((False, True) if listed and typ != UNARY.REDUCE_COLS_IDX_OP_ADD else (not listed,)):
                case = rh.ListedCase(typ, in_dt, idx8, record, data, listed=listed, seed=41)
                ref, ref_arg = case.run_oracle()
                case.check(ref, ref_arg, ref, ref_arg)


@pytest.mark.parametrize("typ", CMP_T, ids=lambda t: f"t{t}")
def test_column_extremum_of_a_zero_tie_oracle_exact_and_reference(reference, typ):
    x = rh.zero_ties(np.random.default_rng(3), 33, 33)
    case = ReduceCase(typ, 33, 33, 40, False, data=x[None])
    mine = case.run_oracle()
    case.check(mine)
    want = {UNARY.REDUCE_X_OP_MAX: (0, 1, True, False), UNARY.REDUCE_X_OP_MIN: (3, 4, False, True), UNARY.REDUCE_X_OP_ABSMAX: (2, 2, True, True)}[typ]
    assert mine[want[0]] == 0.0 and mine[want[1]] == 0.0 and bool(np.signbit(mine[want[0]])) == want[2] and bool(np.signbit(mine[want[1]])) == want[3]
    assert np.array_equal(bits_of(case.run_reference(reference)[case.out_mask]), bits_of(mine[case.out_mask]))


@pytest.mark.parametrize("in_dt", [DT.F16, DT.BF8, DT.HF8], ids=["f16", "bf8", "hf8"])
@pytest.mark.parametrize("rows", [True, False], ids=["rows", "cols"])
def test_oracle_passes_the_checks_on_16_and_8_bit_inputs(reference, rows, in_dt):
    for typ in ALL_T:
        case = ReduceCase(typ, 40, 24, 48, rows, in_dt, DT.F32, seed=5)
        mine = case.run_oracle()
        case.check(mine, what=f"t{typ}")
        assert same_bits(case.run_reference(reference)[case.out_mask], mine[case.out_mask], DT.F32).all()
        if typ in CMP_T:                                   # one padding row folded in shows, also where the poison is the type's largest finite value
            assert _rejected(case, _mutate("padding_row_in_max", case, mine)) or typ == UNARY.REDUCE_X_OP_MIN
