"""The f32 / bf16 reduction TPPs on the GPU, per output, over the whole input range (tests/meltw_reduce_helpers.py; the yardstick is proven in
tests/test_meltw_reduce_cpu.py): reduce_kernel, the forms of reduce_vec_kernel, reduce_combine_kernel and reduce_cols_listed_kernel, each named by the case that
runs it; REDUCE_INIT_ACC; BF16 / F16 results; strided batches; listed columns with a recorded argop; MAX nodes inside equations.

Every case: the kernel name launch_meltw reports against expected_reduce_kernel; sums inside (k + 1) 2^-24 S + k FLT_MIN + r per output (bit for bit against the
oracle where the kernel adds in the reference's order), non-finite sums of the right class; MAX / MIN / ABSMAX equal to the reference's fold (bit for bit over columns);
nothing written outside the results; every element around the m x n block poisoned (+inf / -inf / NaN), so a read of it shows."""
import numpy as np
import pytest

import meltw_reduce_helpers as rh
from meltw_ew_helpers import FLT_MAX, bits_of, decode
from meltw_reduce_helpers import ADD_T, ALL_T, CASES, CMP_T, LISTED_T, ROWS_TAGS, ReduceCase, case_id
from libxsmm_amd import capi
from libxsmm_amd.capi import BINARY, BINARY_FLAG, DT, UNARY, UNARY_FLAG

pytestmark = pytest.mark.gpu


def _run(case, tag=None, what=""):
    got, name = case.run_gpu()
    want_name, want_tag = case.expected()
    assert name == want_name, (what, name, want_name)
    if tag is not None:
        assert want_tag == tag, (what, want_tag)
    case.check(got, what=what, oracle_out=case.run_oracle() if rh.serial_order(want_tag) else None)
    return got


@pytest.mark.parametrize("in_dt", [DT.F32, DT.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("typ", ALL_T, ids=lambda t: f"t{t}")
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_reduction_paths(c, typ, in_dt):
    tag, m, n, ldi, off, batch = c
    outs = (DT.F32, DT.BF16, DT.F16) if rh.first_of_path(c) else (DT.F32,)
    for out_dt in outs:
        for data in ("wide", "infinite"):
            case = ReduceCase(typ, m, n, ldi, tag in ROWS_TAGS, in_dt, out_dt, batch=batch, off=off, data=data, seed=m + n)
            _run(case, tag, what=f"{case_id(c)} t{typ} in{in_dt} out{out_dt} {data}")


@pytest.mark.parametrize("in_dt", [DT.F16, DT.BF8, DT.HF8], ids=["f16", "bf8", "hf8"])
@pytest.mark.parametrize("rows", [True, False], ids=["rows", "cols"])
def test_reductions_of_16_and_8_bit_floats(rows, in_dt):
    """the general kernel converts element by element: the per-output bound for the sums, MAX / MIN / ABSMAX against the reference's fold (E4M3 has no infinity: its
    padding holds +-448 and its data stay below)."""
    for typ in ALL_T:
        _run(ReduceCase(typ, 40, 24, 48, rows, in_dt, DT.F32, seed=5), "general-rows" if rows else "general-cols", what=f"t{typ}")


INIT_CASES = [("general-rows", 130, 9, 131, 0, 1), ("general-cols", 33, 33, 40, 0, 1), ("vec-rows-cpg4", 12, 70, 12, 0, 1), ("vec-rows", 1028, 3, 1028, 0, 1),
              ("vec-cols-1slice", 68, 21, 72, 0, 1), ("vec-cols-16slice", 68, 257, 68, 0, 2), ("two-pass", 64, 2100, 64, 0, 1)]


@pytest.mark.parametrize("in_dt,out_dt", [(DT.F32, DT.F32), (DT.BF16, DT.BF16)], ids=["f32", "bf16"])
@pytest.mark.parametrize("typ", ALL_T, ids=lambda t: f"t{t}")
@pytest.mark.parametrize("c", INIT_CASES, ids=case_id)
def test_reduce_init_acc(c, typ, in_dt, out_dt):
    """the start value is one more term of a sum (read in the output's type); MAX / MIN / ABSMAX ignore the flag, as the reference does."""
    tag, m, n, ldi, off, batch = c
    assert c in CASES
    case = ReduceCase(typ, m, n, ldi, tag in ROWS_TAGS, in_dt, out_dt, init=True, batch=batch, off=off, data="wide", seed=23)
    got = _run(case, tag)
    if typ in CMP_T:                                       # ... and so does the oracle: the same results as without the flag
        assert np.array_equal(decode(case.run_oracle()[case.out_mask], out_dt), decode(got[case.out_mask], out_dt))


def test_two_pass_sums_of_x_and_x2_at_a_padded_ldo():
    """the x^2 results of the second pass sit at out + ldo."""
    for in_dt in (DT.F32, DT.BF16):
        case = ReduceCase(UNARY.REDUCE_X_X2_OP_ADD, 64, 2100, 64, False, in_dt, ldo=68, seed=29)
        assert case.x2_at == 68
        _run(case, "two-pass")


@pytest.mark.parametrize("in_dt", [DT.F32, DT.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [True, False], ids=["rows", "cols"])
@pytest.mark.parametrize("odd", [False, True], ids=["stride16", "odd_stride"])
def test_strided_batch(odd, rows, in_dt):
    """batch 3: a stride that keeps every matrix aligned runs the vector kernel, one that does not the general kernel."""
    for typ in (UNARY.REDUCE_X_X2_OP_ADD, UNARY.REDUCE_X_OP_MIN, UNARY.REDUCE_X_OP_ABSMAX):
        case = ReduceCase(typ, 64, 20, 64, rows, in_dt, batch=3, odd_stride=odd, data="infinite", seed=31)
        assert case.expected()[0] == ("reduce_kernel" if odd else "reduce_vec_kernel")
        _run(case)


@pytest.mark.parametrize("typ", CMP_T, ids=lambda t: f"t{t}")
@pytest.mark.parametrize("c", [("general-cols", 33, 33, 40, 0, 1), ("vec-cols-1slice", 68, 21, 72, 0, 1)], ids=case_id)
def test_column_extremum_keeps_the_references_zero_of_a_tie(c, typ):
    """the forms that walk the columns in order: MAX(x, acc) keeps the later of +0 / -0, MIN(x, acc) the earlier, ABS(-0) is -0 -- bit for bit."""
    tag, m, n, ldi, off, batch = c
    x = rh.zero_ties(np.random.default_rng(3), n, m)
    _run(ReduceCase(typ, m, n, ldi, False, data=x[None]), tag)


@pytest.mark.parametrize("in_dt", [DT.F32, DT.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("typ", CMP_T, ids=lambda t: f"t{t}")
@pytest.mark.parametrize("c", [("vec-cols-16slice", 68, 257, 68, 0, 2), ("two-pass", 8, 2048, 8, 0, 1), ("two-pass", 64, 2100, 64, 0, 1)], ids=case_id)
def test_column_extremum_zero_tie_across_slices_and_chunks(c, typ, in_dt):
    """rows 0 .. 2 hold nothing but zeros, the odd one in the last column or in the middle: slices and chunks are contiguous column ranges folded in column order, so
    the zero that stays is the reference's.  (64, 2100, 64): 14 of the 16 slices of a chunk own columns -- the idle ones must not fold their +0 into an ABSMAX of -0."""
    tag, m, n, ldi, off, batch = c
    assert c in CASES
    rng = np.random.default_rng(7)
    x = np.stack([rh.wide(rng, n, m, DT.F32, False) for _ in range(batch)])
    x[:, :, 0], x[:, n - 1, 0] = 0.0, -0.0
    x[:, :, 1], x[:, n - 1, 1] = -0.0, 0.0
    x[:, :, 2], x[:, n // 2 + 1, 2] = 0.0, -0.0
    case = ReduceCase(typ, m, n, ldi, False, in_dt, batch=batch, data=x if in_dt == DT.F32 else rh.encode(x, DT.BF16))
    ext = case.exact(0)["ext"]
    assert np.all(ext[:3] == 0.0) and len(set(np.signbit(ext[:3]).tolist())) == 2      # both zeros among the expected results
    _run(case, tag)


# ---- listed columns and the recorded argop ----------------------------------------------------------------------------------------------------------------
def _listed(typ, in_dt, idx8, record, data, listed=True, seed=0):
    case = rh.ListedCase(typ, in_dt, idx8, record, data, listed=listed, seed=seed)
    got, got_arg, name = case.run_gpu()
    assert name == "reduce_cols_listed_kernel"
    case.check(got, got_arg, *case.run_oracle())


@pytest.mark.parametrize("data", ["wide", "infinite"])
@pytest.mark.parametrize("record", [False, True], ids=["plain", "argop"])
@pytest.mark.parametrize("idx8", [False, True], ids=["idx4", "idx8"])
@pytest.mark.parametrize("in_dt", [DT.F32, DT.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("typ", LISTED_T, ids=["add", "max", "min"])
def test_listed_columns(typ, in_dt, idx8, record, data):
    _listed(typ, in_dt, idx8, record and typ != UNARY.REDUCE_COLS_IDX_OP_ADD, data, seed=41)


@pytest.mark.parametrize("data", ["wide", "infinite"])
@pytest.mark.parametrize("idx8", [False, True], ids=["idx4", "idx8"])
@pytest.mark.parametrize("in_dt", [DT.F32, DT.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("typ", CMP_T, ids=["max", "min", "absmax"])
def test_column_extremum_with_recorded_argop(typ, in_dt, idx8, data):
    _listed(typ, in_dt, idx8, True, data, listed=False, seed=43)


# ---- MAX / MIN nodes inside equations ---------------------------------------------------------------------------------------------------------------------
M, N, LD = 40, 24, 48
A0 = ("arg", 0)
_R, _C = UNARY_FLAG.REDUCE_ROWS, UNARY_FLAG.REDUCE_COLS
VECRED = __import__("os").environ.get("LIBXSMM_HIP_MEQN_VECRED") != "0"      # =0 keeps trees with vector-valued reductions a chain of TPPs


def _eqn(op):
    """name: (tree, argument shape, output shape, matrix, whether the generated kernel takes it) for op = MAX (infinity: -inf) or MIN (+inf)."""
    mat, scalar = (M, N, LD, DT.F32), (1, 1, 1, DT.F32)
    return {
        "rows_of_cols": (("u", op, _R, ("u", op, _C, A0)), mat, scalar, "holes", True),
        "cols_of_rows": (("u", op, _C, ("u", op, _R, A0)), mat, (N, 1, N, DT.F32), "holes", False),          # not one number, not a column vector of the operand: the chain
        "x_minus_col": (("b", BINARY.SUB, BINARY_FLAG.BCAST_COL_IN_1, A0, ("u", op, _C, A0)), mat, (M, N, M, DT.F32), "holes", VECRED),
        # nothing but the infinity: a nesting with a REDUCE_COLS node stops at -FLT_MAX / FLT_MAX, REDUCE_ROWS nodes alone reach the infinity
        "rows_of_cols_all_inf": (("u", op, _R, ("u", op, _C, A0)), mat, scalar, "all", True),
        "rows_of_rows_all_inf": (("u", op, _R, ("u", op, _R, A0)), mat, scalar, "all", True),
        "rows_of_a_vector_all_inf": (("u", op, _R, A0), (M, 1, M, DT.F32), scalar, "all", True),
    }


EQN = {(o, k): v for o, op in (("max", UNARY.REDUCE_X_OP_MAX), ("min", UNARY.REDUCE_X_OP_MIN)) for k, v in _eqn(op).items()}


@pytest.mark.parametrize("jit", [0, 2], ids=["tpp_chain", "fused_jit"])
@pytest.mark.parametrize("key", sorted(EQN), ids=lambda k: f"{k[0]}-{k[1]}")
def test_extremum_nodes_in_equations(key, jit):
    """a matrix with one column and one row of -inf (MIN: +inf), or nothing else: the step chain and the generated kernel against the composition of oracle TPPs, bit
    for bit; the kernel that ran is asserted, so the generated folds (one number, one number per row) are the ones compared."""
    import test_meqn as tm
    api = capi.load()
    tree, shape, out_shape, kind, fused = EQN[key]
    inf = np.float32(-np.inf if key[0] == "max" else np.inf)
    m, n, ld, _ = shape
    rng = np.random.default_rng(53)
    x = np.full(ld * n, np.float32(7.0))                   # the padding rows: a finite value no result may show
    blk = rh.wide(rng, n, m, DT.F32, False)
    if kind == "holes":
        blk[3, :] = inf
        blk[:, 5] = inf
    else:
        blk[:] = inf
    x.reshape(n, ld)[:, :m] = blk
    want = tm.evaluate(tree, {0: shape}, {0: x}, out_shape)
    api.hip_set_jit(jit)
    h = api.dispatch_meqn(tm.build(api, tree, {0: shape}), capi.MeqnArgShape(*out_shape))
    api.hip_set_jit(1)
    assert h
    kname = api.hip_kernel_name(h, 0).decode()
    assert kname.startswith("meqn_jit") == (jit == 2 and fused), kname
    dx = rh._upload(x)
    dy = rh._upload(np.full(out_shape[2] * out_shape[1], np.float32(-7.0)))
    tm._call(api, h, [dx.data_ptr()], dy.data_ptr())
    api.hip_sync(); api.check()
    got = dy.cpu().numpy()
    assert np.array_equal(bits_of(tm._valid(got, out_shape)), bits_of(tm._valid(want, out_shape))), (tm._valid(got, out_shape).ravel()[:6], tm._valid(want, out_shape).ravel()[:6])
    if key[1] == "rows_of_cols_all_inf":
        assert got[0] == (-FLT_MAX if key[0] == "max" else FLT_MAX)
    elif kind == "all":
        assert got[0] == inf
    elif key[1] == "x_minus_col":                          # row 5 is the infinity, its column extremum the start value: inf - (-/+FLT_MAX) stays the infinity, no NaN
        assert np.all(tm._valid(got, out_shape)[:, 5] == inf) and not np.isnan(got).any()
