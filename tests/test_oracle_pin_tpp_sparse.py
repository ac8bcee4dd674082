"""Pins the TPP and sparse parts of the CPU restatement against the REAL reference
(oracle/_ref/libxsmm_ref.so; skipped when it is not available):
  * oracle_meltw_{unary,binary,ternary}  ==  libxsmm_reference_elementwise     (bit for bit)
  * oracle_packed_spgemm_*, oracle_fsspmdm  ~  the reference's own JIT kernels   (its drivers' bounds)
"""
import ctypes as C

import numpy as np
import pytest

from helpers import normf_rel, rand_values
from libxsmm_amd import capi
from libxsmm_amd.capi import BINARY, BINARY_FLAG, DT, GEMM_FLAG, TERNARY, TERNARY_FLAG, UNARY, UNARY_FLAG
from oracle import pyoracle
from sparse_helpers import csr_to_csc, make_bcsc, pack_vnni2, pack_vnni4, random_csr

OP_UNARY, OP_BINARY, OP_TERNARY = 1, 2, 3
NP = {DT.F32: np.float32, DT.F64: np.float64}


def both_unary(reference, typ, m, n, ldi, ldo, in_dt, out_dt, flags=0, aux_in=None, aux_out_bytes=0, op_primary=None,
               in_elems=None, out_elems=None, out_secondary_val=None, seed=0, inp=None, in_tertiary_val=None):
    orc = pyoracle.oracle()
    rng = np.random.default_rng(seed)
    X = inp if inp is not None else rand_values(rng, in_elems or ldi * n, in_dt)
    Y0 = rand_values(rng, out_elems or ldo * n, out_dt)
    comp = DT.F64 if in_dt == DT.F64 else DT.F32
    outs, auxs = [], []
    for who in ("oracle", "reference"):
        y = Y0.copy()
        aux = np.zeros(aux_out_bytes, dtype=np.uint8) if aux_out_bytes else None
        p = capi.UnaryParam()
        p.in_.primary, p.out.primary = X.ctypes.data, y.ctypes.data
        keep = []
        if aux_in is not None:
            p.in_.secondary = aux_in.ctypes.data
        if aux is not None:
            p.out.secondary = aux.ctypes.data
        if out_secondary_val is not None:
            v = (C.c_ulonglong * len(out_secondary_val))(*out_secondary_val) if isinstance(out_secondary_val, (tuple, list)) else C.c_ulonglong(out_secondary_val); keep.append(v); p.out.secondary = C.addressof(v)
        if op_primary is not None:
            p.op.primary = C.addressof(op_primary)
        if in_tertiary_val is not None:
            tv = C.c_ulonglong(in_tertiary_val); keep.append(tv); p.in_.tertiary = C.addressof(tv)
        if who == "oracle":
            orc.meltw(p, pyoracle.MeltwDesc(m, n, ldi, ldo, 0, 0, in_dt, DT.UNSUPPORTED, DT.UNSUPPORTED, comp, out_dt, flags, typ, OP_UNARY))
        else:
            reference.lib.xref_reference_meltw_unary(C.byref(p), typ, capi.UnaryShape(m, n, ldi, ldo, in_dt, out_dt, comp), flags)
        outs.append(y); auxs.append(aux)
    return outs, auxs


UNARY_OPS = [UNARY.IDENTITY, UNARY.XOR, UNARY.X2, UNARY.NEGATE, UNARY.INC, UNARY.RELU, UNARY.SQRT, UNARY.RECIPROCAL, UNARY.TANH, UNARY.SIGMOID,
             UNARY.GELU, UNARY.EXP, UNARY.RECIPROCAL_SQRT, UNARY.TANH_INV, UNARY.SIGMOID_INV, UNARY.GELU_INV]


@pytest.mark.parametrize("typ", UNARY_OPS)
@pytest.mark.parametrize("in_dt,out_dt", [(DT.F32, DT.F32), (DT.BF16, DT.BF16), (DT.F32, DT.BF16), (DT.BF16, DT.F32)])
def test_unary_math_bit_identical(reference, typ, in_dt, out_dt):
    rng = np.random.default_rng(5)
    inp = None
    if typ in (UNARY.SQRT, UNARY.RECIPROCAL_SQRT, UNARY.RECIPROCAL):
        v = (rng.random(40 * 7) + 0.25).astype(np.float32)
        inp = v if in_dt == DT.F32 else (v.view(np.uint32) >> 16).astype(np.uint16)
    (a, b), _ = both_unary(reference, typ, 33, 7, 40, 35, in_dt, out_dt, inp=inp)
    assert np.array_equal(a, b)


LOWP_PAIRS = [(DT.F16, DT.F16), (DT.BF8, DT.BF8), (DT.HF8, DT.HF8), (DT.F32, DT.F16), (DT.F16, DT.F32), (DT.F32, DT.BF8), (DT.F32, DT.HF8), (DT.BF16, DT.HF8), (DT.BF8, DT.BF16)]


@pytest.mark.parametrize("typ", [UNARY.IDENTITY, UNARY.X2, UNARY.NEGATE, UNARY.INC, UNARY.RELU, UNARY.SIGMOID, UNARY.EXP, UNARY.RECIPROCAL])
@pytest.mark.parametrize("in_dt,out_dt", LOWP_PAIRS, ids=lambda x: str(int(x)))
def test_unary_16_and_8_bit_floats_bit_identical(reference, typ, in_dt, out_dt):
    """F16 / BF8 / HF8 in and out [ref: mateltwise ref :262-324]: the restated conversions round exactly like the reference's."""
    inp = None
    if typ == UNARY.RECIPROCAL:
        v = (np.random.default_rng(6).random(40 * 7) + 0.25).astype(np.float32)
        inp = {DT.F32: v, DT.F16: v.astype(np.float16).view(np.uint16), DT.BF16: (v.view(np.uint32) >> 16).astype(np.uint16)}.get(in_dt)
    (a, b), _ = both_unary(reference, typ, 33, 7, 40, 35, in_dt, out_dt, inp=inp)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("out_dt", [DT.F16, DT.BF8, DT.HF8])
def test_narrowing_on_rounding_boundaries_bit_identical(reference, out_dt):
    """IDENTITY f32 -> narrow type over every half value, its neighbours and ties, overflow / underflow thresholds, NaN and infinities."""
    halves = np.arange(0, 1 << 16, 3, dtype=np.uint16).view(np.float16).astype(np.float32)
    halves = halves[np.isfinite(halves)]
    ulp = np.abs(halves) * np.float32(2.0 ** -11)
    with np.errstate(all="ignore"):
        vals = np.concatenate([halves, halves + ulp, halves - ulp, halves + ulp / 2, halves * np.float32(1.0625), halves * np.float32(0.96875),
                               np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 65504.0, 65519.9, 65520.0, 6e-8, 2.98e-8, 2.9802322e-8, 1e-45, 448.0, 464.0, 465.0, 0.001953125, 0.0009765625, 57344.0, 61440.0, 61439.9], dtype=np.float32)]).astype(np.float32)
    n = 64
    m = (vals.size + n - 1) // n
    inp = np.zeros(m * n, dtype=np.float32); inp[:vals.size] = vals
    (a, b), _ = both_unary(reference, UNARY.IDENTITY, m, n, m, m, DT.F32, out_dt, inp=inp)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("flag", [UNARY_FLAG.BCAST_ROW, UNARY_FLAG.BCAST_COL, UNARY_FLAG.BCAST_SCALAR])
def test_unary_broadcast_bit_identical(reference, flag):
    (a, b), _ = both_unary(reference, UNARY.IDENTITY, 37, 11, 40, 37, DT.F32, DT.BF16, flags=flag)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("dt", [DT.F32, DT.BF16])
def test_relu_family_bit_identical(reference, dt):
    m, n, ld = 70, 9, 72
    mask_bytes = (((ld + 15) // 16) * 16 // 8) * n
    (a, b), (ma, mb) = both_unary(reference, UNARY.RELU, m, n, ld, ld, dt, dt, flags=UNARY_FLAG.BITMASK_2BYTEMULT, aux_out_bytes=mask_bytes)
    assert np.array_equal(a, b)
    bits = lambda x: np.unpackbits(x.reshape(n, -1), axis=1, bitorder="little")[:, :m]
    assert np.array_equal(bits(ma), bits(mb))
    (a, b), _ = both_unary(reference, UNARY.RELU_INV, m, n, ld, ld, dt, dt, flags=UNARY_FLAG.BITMASK_2BYTEMULT, aux_in=ma)
    assert np.array_equal(a, b)
    alpha = C.c_float(0.3)
    for typ in (UNARY.LEAKY_RELU, UNARY.ELU):
        (a, b), _ = both_unary(reference, typ, m, n, ld, ld, dt, dt, op_primary=alpha)
        assert np.array_equal(a, b)


TRANSFORMS = [
    (UNARY.TRANSFORM_NORM_TO_NORMT, DT.F32, 37, 19, 40, 19), (UNARY.TRANSFORM_NORM_TO_NORMT, DT.BF16, 64, 64, 64, 64),
    (UNARY.TRANSFORM_NORM_TO_NORMT, DT.F64, 5, 70, 8, 71), (UNARY.TRANSFORM_NORM_TO_NORMT, DT.I8, 33, 34, 33, 34),
    (UNARY.TRANSFORM_NORM_TO_VNNI2, DT.BF16, 32, 16, 32, 32), (UNARY.TRANSFORM_NORM_TO_VNNI2, DT.BF16, 13, 8, 16, 14),
    (UNARY.TRANSFORM_NORM_TO_VNNI4, DT.BF16, 16, 8, 16, 16), (UNARY.TRANSFORM_NORM_TO_VNNI4, DT.I8, 20, 12, 24, 20),
    (UNARY.TRANSFORM_VNNI2_TO_VNNI2T, DT.BF16, 16, 8, 8, 16), (UNARY.TRANSFORM_NORM_TO_VNNI2T, DT.BF16, 16, 6, 16, 6),
    (UNARY.TRANSFORM_VNNI4_TO_VNNI4T, DT.I8, 16, 8, 8, 16), (UNARY.TRANSFORM_NORM_TO_VNNI4T, DT.BF16, 16, 6, 16, 6),
    (UNARY.TRANSFORM_VNNI4_TO_NORM, DT.I8, 12, 8, 12, 12), (UNARY.TRANSFORM_VNNI4_TO_VNNI2, DT.I8, 12, 8, 12, 12),
    (UNARY.TRANSFORM_PADN_MOD2, DT.BF16, 9, 5, 10, 12), (UNARY.TRANSFORM_PADM_MOD2, DT.BF16, 9, 6, 10, 12),
    (UNARY.TRANSFORM_PADNM_MOD4, DT.I8, 9, 6, 10, 12),
]


@pytest.mark.parametrize("typ,dt,m,n,ldi,ldo", TRANSFORMS)
def test_transforms_bit_identical(reference, typ, dt, m, n, ldi, ldo):
    elems = 4 * max(ldi, ldo) * (max(m, n) + 8)
    (a, b), _ = both_unary(reference, typ, m, n, ldi, ldo, dt, dt, in_elems=elems, out_elems=elems)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("dt", [DT.F32, DT.BF16, DT.I8])
@pytest.mark.parametrize("mode", [UNARY_FLAG.GS_COLS, UNARY_FLAG.GS_ROWS, UNARY_FLAG.GS_OFFS])
@pytest.mark.parametrize("idx8", [0, 1])
def test_gather_bit_identical(reference, dt, mode, idx8):
    m, n, big = 24, 10, 40
    rng = np.random.default_rng(9)
    idt = np.uint64 if idx8 else np.uint32
    flags = mode | (UNARY_FLAG.IDX_SIZE_8BYTES if idx8 else UNARY_FLAG.IDX_SIZE_4BYTES)
    cnt = {UNARY_FLAG.GS_COLS: n, UNARY_FLAG.GS_ROWS: m}.get(mode, m * n)
    idx = rng.choice(big if mode != UNARY_FLAG.GS_OFFS else big * big, size=cnt, replace=False).astype(idt)
    (a, b), _ = both_unary(reference, UNARY.GATHER, m, n, big, m, dt, dt, flags=flags, aux_in=idx, in_elems=big * big, out_elems=m * n)
    assert np.array_equal(a, b)


# ---- the rest of the data-movement family (tests/meltw_move_helpers.py): the whole poisoned output allocation, oracle against reference -------------------------
# The twelve transform types the table above does not hold, at the minimal shapes of tests/test_meltw_move_gpu.py and a payload type the reference's
# libxsmm_elementwise_transform_kernel has a branch for [ref: mateltwise ref :966-1062].
MORE_TRANSFORMS = [
    (UNARY.TRANSFORM_NORM_TO_VNNI8, DT.BF16), (UNARY.TRANSFORM_NORM_TO_VNNI8, DT.I8), (UNARY.TRANSFORM_NORM_TO_VNNI2_PAD, DT.BF16), (UNARY.TRANSFORM_NORM_TO_VNNI4_PAD, DT.I8),
    (UNARY.TRANSFORM_NORM_TO_VNNI4_PAD, DT.F16), (UNARY.TRANSFORM_NORM_TO_VNNI8_PAD, DT.BF16), (UNARY.TRANSFORM_VNNI8_TO_VNNI8T, DT.BF16), (UNARY.TRANSFORM_VNNI8_TO_VNNI8T, DT.I8),
    (UNARY.TRANSFORM_NORM_TO_VNNI8T, DT.BF16), (UNARY.TRANSFORM_VNNI2T_TO_NORM, DT.BF16), (UNARY.TRANSFORM_VNNI4T_TO_NORM, DT.BF16), (UNARY.TRANSFORM_VNNI8T_TO_NORM, DT.BF16),
    (UNARY.TRANSFORM_PADM_MOD4, DT.I8), (UNARY.TRANSFORM_PADN_MOD4, DT.I8), (UNARY.TRANSFORM_PADNM_MOD2, DT.BF16),
]
# what the reference cannot run, and why it is not in a table
NOT_PINNED = {
    "GATHER / SCATTER of 8-byte payloads": "libxsmm_elementwise_gather_scatter_kernel has branches for 32-, 16- and 8-bit payloads only [ref: mateltwise ref :1451-1453, "
                                           ":1489-1790]: with F64 / I64 it returns without moving anything (held by test_reference_moves_no_8_byte_payload below); the "
                                           "8-byte instantiations are held against move_numpy's restatement of the same loops in tests/test_meltw_move_cpu.py",
    "transforms at 4- and 8-byte payloads (the transpose apart)": "libxsmm_elementwise_transform_kernel dispatches on 16- and 8-bit types only [ref: :966-1062]",
    "NORM_TO_VNNIv with n % v != 0": "the reference copies the rows n .. Nn - 1 from behind the input matrix [ref: :547-553]; the oracle keeps the zero fill of the same "
                                     "function: the pinned shapes have n % v == 0",
}


def _pin_whole_allocation(reference, case):
    a, b = case.run_oracle(), case.run_reference(reference)
    assert np.array_equal(a, b), f"{case.id()}: {np.count_nonzero(a != b)} bytes differ; first at {int(np.flatnonzero(a != b)[0])}"
    assert not np.array_equal(a, case.out0)


@pytest.mark.parametrize("typ,dt", MORE_TRANSFORMS, ids=lambda x: str(int(x)))
def test_more_transforms_bit_identical(reference, typ, dt):
    from meltw_move_helpers import MoveCase
    from test_meltw_move_gpu import transform_shapes
    _pin_whole_allocation(reference, MoveCase(typ, dt, *transform_shapes(typ)[0], off_out=capi.DT_SIZE[dt]))


@pytest.mark.parametrize("dt", [DT.F32, DT.BF16, DT.I8])
@pytest.mark.parametrize("mode", [UNARY_FLAG.GS_COLS, UNARY_FLAG.GS_ROWS, UNARY_FLAG.GS_OFFS])
@pytest.mark.parametrize("idx8", [0, 1])
def test_scatter_bit_identical(reference, dt, mode, idx8):
    """unique indices; the destination is pre-filled: what no index names keeps its bytes on both sides."""
    from meltw_move_helpers import MoveCase
    case = MoveCase(UNARY.SCATTER, dt, 37, 9, 39, 41, flags=mode | (UNARY_FLAG.IDX_SIZE_8BYTES if idx8 else UNARY_FLAG.IDX_SIZE_4BYTES), off_out=8)
    assert np.unique(case.idx).size == case.idx.size
    _pin_whole_allocation(reference, case)


@pytest.mark.parametrize("mode", [UNARY_FLAG.GS_COLS, UNARY_FLAG.GS_ROWS, UNARY_FLAG.GS_OFFS])
@pytest.mark.parametrize("dt", [DT.F16, DT.F32])
def test_gather_with_repeated_indices_bit_identical(reference, mode, dt):
    """an embedding look-up names rows more than once (the F16 rows are the 16-bit branch through another type)"""
    from meltw_move_helpers import MoveCase
    case = MoveCase(UNARY.GATHER, dt, 37, 9, 41, 39, flags=mode | UNARY_FLAG.IDX_SIZE_4BYTES, off_out=8)
    assert np.unique(case.idx).size < case.idx.size
    _pin_whole_allocation(reference, case)
    _pin_whole_allocation(reference, MoveCase(UNARY.GATHER, dt, 37, 9, 41, 39, flags=mode | UNARY_FLAG.IDX_SIZE_8BYTES, idx="equal" if mode != UNARY_FLAG.GS_OFFS else "reversed"))


def test_reference_moves_no_8_byte_payload(reference):
    """NOT_PINNED's first entry: the reference leaves the output of an F64 gather as it was."""
    from meltw_move_helpers import MoveCase
    case = MoveCase(UNARY.GATHER, DT.F64, 37, 9, 41, 39, flags=UNARY_FLAG.GS_ROWS | UNARY_FLAG.IDX_SIZE_4BYTES)
    assert np.array_equal(case.run_reference(reference), case.out0)
    assert all(len(why) > 60 for why in NOT_PINNED.values())


@pytest.mark.parametrize("typ", [UNARY.REDUCE_X_OP_ADD, UNARY.REDUCE_X2_OP_ADD, UNARY.REDUCE_X_X2_OP_ADD, UNARY.REDUCE_X_OP_MAX, UNARY.REDUCE_X_OP_MIN, UNARY.REDUCE_X_OP_ABSMAX])
@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("in_dt", [DT.F32, DT.BF16])
def test_reductions_bit_identical(reference, typ, rows, in_dt):
    m, n, ldi = 75, 33, 80
    res = n if rows else m
    flags = UNARY_FLAG.REDUCE_ROWS if rows else UNARY_FLAG.REDUCE_COLS
    (a, b), _ = both_unary(reference, typ, m, n, ldi, res, in_dt, DT.F32, flags=flags, out_elems=2 * res)
    used = 2 * res if typ == UNARY.REDUCE_X_X2_OP_ADD else res
    assert np.array_equal(a[:used], b[:used])


@pytest.mark.parametrize("dt", [DT.F32, DT.BF16])
@pytest.mark.parametrize("m,n,ld", [(70, 9, 72), (16, 4, 16), (5, 3, 8)])
@pytest.mark.parametrize("bitm", [0, 1])
def test_dropout_bit_identical(reference, dt, m, n, ld, bitm):
    """DROPOUT draws from 16 xoshiro128+ streams, `w` rows per draw with w = the reference CPU's 32-bit vector length: the oracle is told
    that width (its default, and the device library's, is 16 = AVX-512).  Output, mask and the advanced generator state must match;
    DROPOUT_INV replays the mask."""
    orc = pyoracle.oracle()
    ref_w = int(reference.lib.xref_vlen32())
    assert 1 <= ref_w <= 16
    orc.lib.oracle_set_rng_width(ref_w)
    try:
        rng = np.random.default_rng(8)
        X, Y0 = rand_values(rng, ld * n, dt), rand_values(rng, ld * n, dt)
        state0 = rng.integers(1, 2 ** 32, size=64, dtype=np.uint64).astype(np.uint32)
        prob = C.c_float(0.3)
        flags = UNARY_FLAG.BITMASK_2BYTEMULT if bitm else 0
        mask_bytes = (((ld + 15) // 16) * 16 // 8) * n
        res = []
        for who in ("oracle", "reference"):
            y, st, mask = Y0.copy(), state0.copy(), np.zeros(mask_bytes, dtype=np.uint8)
            p = capi.UnaryParam()
            p.in_.primary, p.out.primary, p.out.secondary, p.op.primary, p.op.secondary = X.ctypes.data, y.ctypes.data, mask.ctypes.data, C.addressof(prob), st.ctypes.data
            if who == "oracle":
                orc.meltw(p, pyoracle.MeltwDesc(m, n, ld, ld, 0, 0, dt, DT.UNSUPPORTED, DT.UNSUPPORTED, DT.F32, dt, flags, UNARY.DROPOUT, OP_UNARY))
            else:
                reference.lib.xref_reference_meltw_unary(C.byref(p), UNARY.DROPOUT, capi.UnaryShape(m, n, ld, ld, dt, dt, DT.F32), flags)
            res.append((y, st, mask))
        (ya, sa, ma), (yb, sb, mb) = res
        valid = lambda y: y.reshape(n, ld)[:, :m]
        assert np.array_equal(valid(ya), valid(yb)) and np.array_equal(sa, sb)
        kept = (valid(ya).view(np.uint16 if dt == DT.BF16 else np.uint32) != 0).mean()
        assert m * n < 100 or 0.5 < kept < 0.9                       # p = 0.3: about 70 % survive
        if bitm:
            bits = lambda x: np.unpackbits(x.reshape(n, -1), axis=1, bitorder="little")[:, :m]
            assert np.array_equal(bits(ma), bits(mb))
            (a, b), _ = both_unary(reference, UNARY.DROPOUT_INV, m, n, ld, ld, dt, dt, flags=flags, aux_in=ma, op_primary=prob)
            assert np.array_equal(a.reshape(n, ld)[:, :m], b.reshape(n, ld)[:, :m])
    finally:
        orc.lib.oracle_set_rng_width(16)


def _wide_f32(rng, count):
    """values over many binades, with specials: what a rounding to E5M2 has to be tried on"""
    v = (rng.standard_normal(count) * 2.0 ** rng.integers(-18, 15, count)).astype(np.float32)
    v[:8] = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 65504.0, 1e-7, -3e-6], dtype=np.float32)
    return v


@pytest.mark.parametrize("what", ["unary_identity", "unary_x2", "binary_add", "ternary_muladd"])
@pytest.mark.parametrize("m,n,ld", [(70, 9, 72), (5, 3, 8), (16, 16, 16)])
def test_stochastic_rounding_bit_identical(reference, what, m, n, ld):
    """*_STOCHASTIC_ROUND to BF8: one xoshiro128++ draw per element, stream = element number % 16, from the state behind op.secondary
    [ref: src/libxsmm_lpflt_quant.c:303-365].  Bytes and the advanced state must match the reference."""
    orc = pyoracle.oracle()
    rng = np.random.default_rng(4)
    X0, X1, X2 = _wide_f32(rng, ld * n), _wide_f32(rng, ld * n), _wide_f32(rng, ld * n)
    state0 = rng.integers(1, 2 ** 32, size=64, dtype=np.uint64).astype(np.uint32)
    res = []
    for who in ("oracle", "reference"):
        y, st = np.zeros(ld * n, dtype=np.uint8), state0.copy()
        if what.startswith("unary"):
            typ = UNARY.IDENTITY if what == "unary_identity" else UNARY.X2
            p = capi.UnaryParam(); p.in_.primary, p.out.primary, p.op.secondary = X0.ctypes.data, y.ctypes.data, st.ctypes.data
            if who == "oracle":
                orc.meltw(p, pyoracle.MeltwDesc(m, n, ld, ld, 0, 0, DT.F32, DT.UNSUPPORTED, DT.UNSUPPORTED, DT.F32, DT.BF8, UNARY_FLAG.STOCHASTIC_ROUND, typ, OP_UNARY))
            else:
                reference.lib.xref_reference_meltw_unary(C.byref(p), typ, capi.UnaryShape(m, n, ld, ld, DT.F32, DT.BF8, DT.F32), UNARY_FLAG.STOCHASTIC_ROUND)
        elif what == "binary_add":
            p = capi.BinaryParam(); p.in0.primary, p.in1.primary, p.out.primary, p.op.secondary = X0.ctypes.data, X1.ctypes.data, y.ctypes.data, st.ctypes.data
            if who == "oracle":
                orc.meltw(p, pyoracle.MeltwDesc(m, n, ld, ld, ld, 0, DT.F32, DT.F32, DT.UNSUPPORTED, DT.F32, DT.BF8, BINARY_FLAG.STOCHASTIC_ROUND, BINARY.ADD, OP_BINARY))
            else:
                reference.lib.xref_reference_meltw_binary(C.byref(p), BINARY.ADD, capi.BinaryShape(m, n, ld, ld, ld, DT.F32, DT.F32, DT.BF8, DT.F32), BINARY_FLAG.STOCHASTIC_ROUND)
        else:
            p = capi.TernaryParam(); p.in0.primary, p.in1.primary, p.in2.primary, p.out.primary, p.op.secondary = X0.ctypes.data, X1.ctypes.data, X2.ctypes.data, y.ctypes.data, st.ctypes.data
            if who == "oracle":
                orc.meltw(p, pyoracle.MeltwDesc(m, n, ld, ld, ld, ld, DT.F32, DT.F32, DT.F32, DT.F32, DT.BF8, TERNARY_FLAG.STOCHASTIC_ROUND, TERNARY.MULADD, OP_TERNARY))
            else:
                reference.lib.xref_reference_meltw_ternary(C.byref(p), TERNARY.MULADD, capi.TernaryShape(m, n, ld, ld, ld, ld, DT.F32, DT.F32, DT.F32, DT.BF8, DT.F32), TERNARY_FLAG.STOCHASTIC_ROUND)
        res.append((y.reshape(n, ld)[:, :m].copy(), st))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert not np.array_equal(res[0][1], state0)


@pytest.mark.parametrize("typ", [UNARY.REDUCE_COLS_IDX_OP_ADD, UNARY.REDUCE_COLS_IDX_OP_MAX, UNARY.REDUCE_COLS_IDX_OP_MIN])
@pytest.mark.parametrize("in_dt", [DT.F32, DT.BF16])
@pytest.mark.parametrize("idx8", [0, 1])
@pytest.mark.parametrize("record", [0, 1])
def test_reduce_over_listed_columns_bit_identical(reference, typ, in_dt, idx8, record):
    """out[i] = op over the listed columns (an embedding bag); MAX / MIN optionally record the winning column [ref: mateltwise ref :1346-1430]."""
    if record and typ == UNARY.REDUCE_COLS_IDX_OP_ADD:
        pytest.skip("nothing to record for a sum")
    m, big, ldi, ncols = 45, 60, 48, 17
    rng = np.random.default_rng(21)
    idt = np.uint64 if idx8 else np.uint32
    idx = rng.integers(0, big, size=ncols).astype(idt)                      # repeats allowed
    flags = UNARY_FLAG.REDUCE_COLS | (0 if idx8 else UNARY_FLAG.IDX_SIZE_4BYTES) | (UNARY_FLAG.REDUCE_RECORD_ARGOP if record else 0)
    (a, b), (xa, xb) = both_unary(reference, typ, m, big, ldi, m, in_dt, DT.F32, flags=flags, aux_in=idx, in_elems=ldi * big, out_elems=m,
                                  in_tertiary_val=ncols, aux_out_bytes=m * (8 if idx8 else 4) if record else 0)
    assert np.array_equal(a, b)
    if record:
        assert np.array_equal(xa, xb)


@pytest.mark.parametrize("typ", [UNARY.REDUCE_X_OP_MAX, UNARY.REDUCE_X_OP_MIN, UNARY.REDUCE_X_OP_ABSMAX])
@pytest.mark.parametrize("idx8", [0, 1])
def test_column_reduction_records_the_extremum_bit_identical(reference, typ, idx8):
    m, n, ldi = 45, 33, 48
    flags = UNARY_FLAG.REDUCE_COLS | UNARY_FLAG.REDUCE_RECORD_ARGOP | (0 if idx8 else UNARY_FLAG.IDX_SIZE_4BYTES)
    (a, b), (xa, xb) = both_unary(reference, typ, m, n, ldi, m, DT.F32, DT.F32, flags=flags, out_elems=m, aux_out_bytes=m * (8 if idx8 else 4))
    assert np.array_equal(a, b) and np.array_equal(xa, xb)


@pytest.mark.parametrize("typ", [BINARY.ADD, BINARY.MUL, BINARY.SUB, BINARY.DIV, BINARY.MULADD, BINARY.MAX, BINARY.MIN, BINARY.CMP_OP_GT, BINARY.CMP_OP_LE, BINARY.CMP_OP_EQ])
@pytest.mark.parametrize("dts", [(DT.F32, DT.F32, DT.F32), (DT.BF16, DT.BF16, DT.BF16), (DT.BF16, DT.F32, DT.F32)])
@pytest.mark.parametrize("flags", [0, BINARY_FLAG.BCAST_COL_IN_0, BINARY_FLAG.BCAST_ROW_IN_1 | BINARY_FLAG.BCAST_SCALAR_IN_0])
def test_binary_bit_identical(reference, typ, dts, flags):
    orc = pyoracle.oracle()
    m, n, ld = 45, 13, 48
    rng = np.random.default_rng(3)
    X0, X1 = rand_values(rng, ld * n, dts[0]), rand_values(rng, ld * n, dts[1])
    cmp_ = typ >= BINARY.CMP_OP_GT
    Y0 = np.zeros((((ld + 15) // 16) * 16 // 8) * n, dtype=np.uint8) if cmp_ else rand_values(rng, ld * n, dts[2])
    outs = []
    for who in ("oracle", "reference"):
        y = Y0.copy()
        p = capi.BinaryParam(); p.in0.primary, p.in1.primary, p.out.primary = X0.ctypes.data, X1.ctypes.data, y.ctypes.data
        if who == "oracle":
            orc.meltw(p, pyoracle.MeltwDesc(m, n, ld, ld, ld, 0, dts[0], dts[1], DT.UNSUPPORTED, DT.F32, dts[2], flags, typ, OP_BINARY))
        else:
            reference.lib.xref_reference_meltw_binary(C.byref(p), typ, capi.BinaryShape(m, n, ld, ld, ld, dts[0], dts[1], dts[2], DT.F32), flags)
        outs.append(y)
    if cmp_:
        bits = lambda x: np.unpackbits(x.reshape(n, -1), axis=1, bitorder="little")[:, :m]
        assert np.array_equal(bits(outs[0]), bits(outs[1]))
    else:
        assert outs[0].tobytes() == outs[1].tobytes()     # raw bytes: 0/0 -> NaN must match too


@pytest.mark.parametrize("dts", [(DT.F32, DT.F32, DT.F32), (DT.BF16, DT.BF16, DT.F32), (DT.BF16, DT.F32, DT.BF16)])
@pytest.mark.parametrize("m,n,ld", [(45, 13, 48), (64, 4, 64), (1, 1, 1), (7, 300, 9)])
def test_dot_product_to_scalar_bit_identical(reference, dts, m, n, ld):
    """BINARY_MUL_AND_REDUCE_TO_SCALAR_OP_ADD [ref: generator_mateltwise_reference_impl.c:2523-2542]: the serial f32 sum in the reference's order"""
    orc = pyoracle.oracle()
    rng = np.random.default_rng(31)
    X0, X1 = rand_values(rng, ld * n, dts[0]), rand_values(rng, ld * n, dts[1])
    typ = BINARY.MUL_AND_REDUCE_TO_SCALAR_OP_ADD
    outs = []
    for who in ("oracle", "reference"):
        y = rand_values(np.random.default_rng(5), 4, dts[2])
        p = capi.BinaryParam(); p.in0.primary, p.in1.primary, p.out.primary = X0.ctypes.data, X1.ctypes.data, y.ctypes.data
        if who == "oracle":
            orc.meltw(p, pyoracle.MeltwDesc(m, n, ld, 1, ld, 0, dts[0], dts[1], DT.UNSUPPORTED, DT.F32, dts[2], 0, typ, OP_BINARY))
        else:
            reference.lib.xref_reference_meltw_binary(C.byref(p), typ, capi.BinaryShape(m, n, ld, ld, 1, dts[0], dts[1], dts[2], DT.F32), 0)
        outs.append(y)
    assert outs[0][:1].tobytes() == outs[1][:1].tobytes()


@pytest.mark.parametrize("in_dt,out_dt", [(DT.F32, DT.F32), (DT.BF16, DT.BF16), (DT.BF16, DT.F32), (DT.F16, DT.F32), (DT.F32, DT.BF8), (DT.F64, DT.F64)])
@pytest.mark.parametrize("m,n,ld", [(45, 13, 48), (64, 64, 64), (1, 1, 1), (7, 300, 9)])
def test_reduce_to_scalar_bit_identical(reference, in_dt, out_dt, m, n, ld):
    """UNARY_REDUCE_TO_SCALAR_OP_ADD [ref: generator_mateltwise_reference_impl.c:2097-2116]: one serial sum over the block, f32 (f64 when all three types are)"""
    outs, _ = both_unary(reference, UNARY.REDUCE_TO_SCALAR_OP_ADD, m, n, ld, 1, in_dt, out_dt, out_elems=4, seed=41)
    assert outs[0].tobytes() == outs[1].tobytes()


@pytest.mark.parametrize("in_dt,out_dt", [(DT.F32, DT.F32), (DT.BF16, DT.BF16), (DT.BF16, DT.F32), (DT.F32, DT.F16)])
@pytest.mark.parametrize("bc,bn,C_,N_", [(16, 4, 64, 32), (8, 8, 8, 8), (32, 2, 96, 10), (5, 3, 20, 9)])
def test_reduce_ncnc_format_bit_identical(reference, in_dt, out_dt, bc, bn, C_, N_):
    """UNARY_REDUCE_X_OP_ADD_NCNC_FORMAT [ref: :2118-2141]: blocked [N / bn][C / bc][bn][bc] input (m = bc, n = bn, ldi = C, ldo = N), one sum per channel"""
    outs, _ = both_unary(reference, UNARY.REDUCE_X_OP_ADD_NCNC_FORMAT, bc, bn, C_, N_, in_dt, out_dt, in_elems=C_ * N_, out_elems=C_ + 3, seed=42)
    assert outs[0].tobytes() == outs[1].tobytes()


@pytest.mark.parametrize("typ", [UNARY.DECOMP_FP32_TO_BF16X2, UNARY.DECOMP_FP32_TO_BF16X3])
@pytest.mark.parametrize("m,n,ldi,ldo", [(32, 8, 32, 32), (17, 5, 20, 24), (9, 2, 9, 12)])
def test_decomp_f32_to_bf16_pieces_bit_identical(reference, typ, m, n, ldi, ldo):
    """DECOMP_FP32_TO_BF16X2 / X3 [ref: :2437-2470]: truncated leading piece(s), RNE of the remainder; wide-exponent data, denormals and specials included"""
    rng = np.random.default_rng(43)
    X = _wide_f32(rng, ldi * n)
    piece = ldo * n * 2
    outs, _ = both_unary(reference, typ, m, n, ldi, ldo, DT.F32, DT.BF16, inp=X, out_elems=3 * ldo * n, out_secondary_val=(piece, 2 * piece), seed=44)
    assert outs[0].tobytes() == outs[1].tobytes()


@pytest.mark.parametrize("typ", [TERNARY.SELECT, TERNARY.MULADD, TERNARY.NMULADD])
@pytest.mark.parametrize("dt", [DT.F32, DT.BF16])
def test_ternary_bit_identical(reference, typ, dt):
    orc = pyoracle.oracle()
    m, n, ld = 40, 9, 48
    rng = np.random.default_rng(6)
    X0, X1 = rand_values(rng, ld * n, dt), rand_values(rng, ld * n, dt)
    X2 = rng.integers(0, 256, size=(((ld + 15) // 16) * 16 // 8) * n, dtype=np.uint8) if typ == TERNARY.SELECT else rand_values(rng, ld * n, dt)
    Y0 = rand_values(rng, ld * n, dt)
    outs = []
    for who in ("oracle", "reference"):
        y = Y0.copy()
        p = capi.TernaryParam(); p.in0.primary, p.in1.primary, p.in2.primary, p.out.primary = X0.ctypes.data, X1.ctypes.data, X2.ctypes.data, y.ctypes.data
        if who == "oracle":
            orc.meltw(p, pyoracle.MeltwDesc(m, n, ld, ld, ld, ld, dt, dt, dt, DT.F32, dt, 0, typ, OP_TERNARY))
        else:
            reference.lib.xref_reference_meltw_ternary(C.byref(p), typ, capi.TernaryShape(m, n, ld, ld, ld, ld, dt, dt, dt, dt, DT.F32), 0)
        outs.append(y)
    assert np.array_equal(outs[0], outs[1])


# ---- sparse: restated gold loops vs the reference's own JIT kernels -------------------------------------
@pytest.mark.parametrize("dt", [DT.F32, DT.F64])
@pytest.mark.parametrize("M,N,K,P,density,beta0", [(35, 16, 35, 16, 0.09, 0), (9, 10, 9, 8, 0.4, 0), (20, 3, 50, 16, 0.1, 0)])
def test_packed_csr_asparse_vs_reference_jit(reference, dt, M, N, K, P, density, beta0):
    orc = pyoracle.oracle()
    rng = np.random.default_rng(42)
    rowptr, colidx = random_csr(rng, M, K, density)
    vals = rand_values(rng, len(colidx), dt) + NP[dt](0.05)
    B, C0 = rand_values(rng, K * N * P, dt), rand_values(rng, M * N * P, dt)
    ref_c, jit_c = C0.copy(), C0.copy()
    orc.lib.oracle_packed_spgemm_csr_asparse(dt, M, N, K, P, rowptr.ctypes.data, colidx.ctypes.data, vals.ctypes.data, B.ctypes.data, N, ref_c.ctypes.data, N, beta0)
    h = reference.create_packed_spgemm_csr(capi.gemm_shape(M, N, K, 0, N, N, dt, dt, dt, dt), GEMM_FLAG.BETA_0 if beta0 else 0, 0, P,
                                           rowptr.ctypes.data, colidx.ctypes.data, vals.ctypes.data)
    if not h:
        pytest.skip("reference JIT refused")
    p = capi.GemmParam(); p.a.primary, p.b.primary, p.c.primary = vals.ctypes.data, B.ctypes.data, jit_c.ctypes.data
    capi.Api.call(h, p)
    assert normf_rel(ref_c, jit_c, dt) <= (1e-5 if dt == DT.F32 else 1e-12)
    reference.release_kernel(h)


@pytest.mark.parametrize("dt", [DT.F32, DT.F64])
def test_packed_csc_bsparse_vs_reference_jit(reference, dt):
    orc = pyoracle.oracle()
    M, N, K, P = 9, 20, 35, 16
    rng = np.random.default_rng(7)
    rowptr, colidx = random_csr(rng, K, N, 0.2)
    vals = rand_values(rng, len(colidx), dt) + NP[dt](0.05)
    colptr, rowidx, cvals = csr_to_csc(rowptr, colidx, vals, K, N)
    A, C0 = rand_values(rng, M * K * P, dt), rand_values(rng, M * N * P, dt)
    ref_c, ref2_c, jit_c = C0.copy(), C0.copy(), C0.copy()
    orc.lib.oracle_packed_spgemm_csc_bsparse(dt, M, N, K, P, colptr.ctypes.data, rowidx.ctypes.data, cvals.ctypes.data, A.ctypes.data, K, ref_c.ctypes.data, N, 0)
    orc.lib.oracle_packed_spgemm_csr_bsparse(dt, M, N, K, P, rowptr.ctypes.data, colidx.ctypes.data, vals.ctypes.data, A.ctypes.data, K, ref2_c.ctypes.data, N, 0)
    assert np.array_equal(ref_c, ref2_c)          # the CSR and CSC restatements agree bit for bit
    h = reference.create_packed_spgemm_csc(capi.gemm_shape(M, N, K, K, 0, N, dt, dt, dt, dt), 0, 0, P, colptr.ctypes.data, rowidx.ctypes.data, cvals.ctypes.data)
    if not h:
        pytest.skip("reference JIT refused")
    p = capi.GemmParam(); p.a.primary, p.b.primary, p.c.primary = A.ctypes.data, cvals.ctypes.data, jit_c.ctypes.data
    capi.Api.call(h, p)
    assert normf_rel(ref_c, jit_c, dt) <= (1e-5 if dt == DT.F32 else 1e-12)
    reference.release_kernel(h)


@pytest.mark.parametrize("dt", [DT.F32, DT.F64])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_fsspmdm_vs_reference(reference, dt, beta):
    orc = pyoracle.oracle()
    M, N, K = 35, 96, 35
    rng = np.random.default_rng(3)
    rowptr, colidx = random_csr(rng, M, K, 0.15)
    vals = rand_values(rng, len(colidx), dt) + NP[dt](0.05)
    a_dense = np.zeros((M, K), dtype=NP[dt])
    for i in range(M):
        a_dense[i, colidx[rowptr[i]:rowptr[i + 1]]] = vals[rowptr[i]:rowptr[i + 1]]
    B, C0 = rand_values(rng, K * N, dt), rand_values(rng, M * N, dt)
    ref_c, lib_c = C0.copy(), C0.copy()
    alpha = NP[dt](1.5)
    sv = (alpha * vals).astype(NP[dt])
    orc.lib.oracle_fsspmdm(dt, M, N, K, rowptr.ctypes.data, colidx.ctypes.data, sv.ctypes.data, B.ctypes.data, N, ref_c.ctypes.data, N, int(beta == 0.0))
    ct = C.c_double if dt == DT.F64 else C.c_float
    cal, cbe = ct(float(alpha)), ct(beta)
    h = reference.fsspmdm_create(dt, M, N, K, K, N, N, C.addressof(cal), C.addressof(cbe), a_dense.ctypes.data, 0, None)
    assert h
    reference.fsspmdm_execute(h, B.ctypes.data, lib_c.ctypes.data)
    assert normf_rel(ref_c, lib_c, dt) <= (1e-5 if dt == DT.F32 else 1e-12)
    reference.fsspmdm_destroy(h)


@pytest.mark.parametrize("a_type,c_type,vnni,bk,bn", [(DT.F32, DT.F32, 0, 8, 8), (DT.BF16, DT.BF16, 1, 32, 32), (DT.BF16, DT.F32, 1, 32, 16)])
@pytest.mark.parametrize("beta0", [0, 1])
def test_bcsc_vs_reference_jit(reference, a_type, c_type, vnni, bk, bn, beta0):
    orc = pyoracle.oracle()
    M, N, K, mb = 64, 64, 256, 4
    rng = np.random.default_rng(11)
    colptr, rowidx, bvals = make_bcsc(rng, K, N, bk, bn, 0.25, a_type)
    A = rand_values(rng, mb * K * M, a_type)
    A_run = pack_vnni2(A, mb, K, M) if vnni else A
    C0 = rand_values(rng, mb * N * M, c_type)
    ref_c, jit_c = C0.copy(), C0.copy()
    orc.lib.oracle_packed_spgemm_bcsc(a_type, c_type, M, N, K, mb, bk, bn, vnni, A_run.ctypes.data, bvals.ctypes.data, colptr.ctypes.data, rowidx.ctypes.data, ref_c.ctypes.data, beta0)
    flags = (GEMM_FLAG.BETA_0 if beta0 else 0) | (GEMM_FLAG.VNNI_A if vnni else 0)
    h = reference.create_packed_spgemm_bcsc(capi.gemm_shape(mb, 0, K, K, 0, N, a_type, a_type, c_type, DT.F32), flags, 0, capi.SpgemmConfig(M, bk, bn))
    if not h:
        pytest.skip("reference JIT refused this BCSC configuration on this host")
    nblk = C.c_ulonglong(N // bn)
    p = capi.GemmParam()
    p.a.primary, p.b.primary, p.b.secondary, p.b.tertiary, p.b.quaternary, p.c.primary = \
        A_run.ctypes.data, bvals.ctypes.data, colptr.ctypes.data, rowidx.ctypes.data, C.addressof(nblk), jit_c.ctypes.data
    capi.Api.call(h, p)
    assert normf_rel(ref_c, jit_c, c_type) <= (5e-3 if c_type == DT.BF16 else 1e-4)
    reference.release_kernel(h)


@pytest.mark.parametrize("a_type", [DT.U8, DT.I8])
@pytest.mark.parametrize("bk,bn,beta0", [(32, 16, 0), (32, 32, 1), (8, 8, 0), (16, 4, 1)])
def test_bcsc_int8_vs_reference_jit(reference, a_type, bk, bn, beta0):
    """8-bit integer BCSC (unsigned x signed -> int32, VNNI-4 A): the restatement is EQUAL to the reference's JIT kernel."""
    orc = pyoracle.oracle()
    M, N, K, mb = 64, 64, 256, 3
    rng = np.random.default_rng(13)
    b_type = DT.I8 if a_type == DT.U8 else DT.U8
    colptr, rowidx, bvals = make_bcsc(rng, K, N, bk, bn, 0.25, b_type)
    A = rng.integers(0, 256, mb * K * M).astype(np.uint8) if a_type == DT.U8 else rng.integers(-128, 128, mb * K * M).astype(np.int8)
    bvals = rng.integers(-128, 128, bvals.size).astype(np.int8) if b_type == DT.I8 else rng.integers(0, 256, bvals.size).astype(np.uint8)
    A_run = pack_vnni4(A, mb, K, M)
    C0 = rng.integers(-1000, 1000, mb * N * M).astype(np.int32)
    ref_c, jit_c = C0.copy(), C0.copy()
    orc.lib.oracle_packed_spgemm_bcsc(a_type, DT.I32, M, N, K, mb, bk, bn, 1, A_run.ctypes.data, bvals.ctypes.data, colptr.ctypes.data, rowidx.ctypes.data, ref_c.ctypes.data, beta0)
    flags = (GEMM_FLAG.BETA_0 if beta0 else 0) | GEMM_FLAG.VNNI_A
    h = reference.create_packed_spgemm_bcsc(capi.gemm_shape(mb, 0, K, K, 0, N, a_type, b_type, DT.I32, DT.I32), flags, 0, capi.SpgemmConfig(M, bk, bn))
    if not h:
        pytest.skip("reference JIT refused this BCSC configuration on this host")
    nblk = C.c_ulonglong(N // bn)
    p = capi.GemmParam()
    p.a.primary, p.b.primary, p.b.secondary, p.b.tertiary, p.b.quaternary, p.c.primary = \
        A_run.ctypes.data, bvals.ctypes.data, colptr.ctypes.data, rowidx.ctypes.data, C.addressof(nblk), jit_c.ctypes.data
    capi.Api.call(h, p)
    assert np.array_equal(ref_c, jit_c)
    reference.release_kernel(h)


@pytest.mark.parametrize("M,N,K,P,density,beta0", [(9, 9, 9, 16, 0.3, 0), (35, 35, 4, 32, 0.1, 0), (20, 9, 7, 64, 0.5, 0)])
def test_packed_csc_csparse_vs_reference_jit(reference, M, N, K, P, density, beta0):
    """The C-sparse variant of the packed CSC kernel (ldc == 0) has no gold loop in the reference: the restatement is pinned against the
    reference's JIT kernel itself (summation order differs: 1e-5 of the norm).  Pinned for beta = 1 only: with LIBXSMM_GEMM_FLAG_BETA_0 the
    reference's AVX-512 kernel returns values that are NOT sum_k sum_p A*B for columns with more than two stored entries (observed here on
    9x9 / 24 entries: off by O(1), while the same call with beta = 1 agrees to 3e-7) -- for beta = 0 the restatement is checked against plain
    algebra instead (test_packed_csc_csparse_beta0_is_the_plain_sum)."""
    orc = pyoracle.oracle()
    rng = np.random.default_rng(17)
    rowptr, colidx = random_csr(rng, N, M, density)                       # CSR of C^T == CSC of C: pointer over n, indices = rows m
    nnz = int(rowptr[-1])
    A = rand_values(rng, K * M * P, DT.F32); B = rand_values(rng, K * N * P, DT.F32)
    C0 = rand_values(rng, max(1, nnz), DT.F32)
    ref_c, jit_c = C0.copy(), C0.copy()
    orc.lib.oracle_packed_spgemm_csc_csparse(N, K, P, rowptr.ctypes.data, colidx.ctypes.data, A.ctypes.data, M, B.ctypes.data, N, ref_c.ctypes.data, beta0)
    h = reference.create_packed_spgemm_csc(capi.gemm_shape(M, N, K, M, N, 0, DT.F32, DT.F32, DT.F32, DT.F32), GEMM_FLAG.BETA_0 if beta0 else 0, 0, P,
                                           rowptr.ctypes.data, colidx.ctypes.data, C0.ctypes.data)
    if not h:
        pytest.skip("reference JIT refused the C-sparse configuration on this host")
    p = capi.GemmParam()
    p.a.primary, p.b.primary, p.c.primary = A.ctypes.data, B.ctypes.data, jit_c.ctypes.data
    capi.Api.call(h, p)
    assert normf_rel(ref_c, jit_c, DT.F32) <= 1e-5
    reference.release_kernel(h)


def test_packed_csc_csparse_beta0_is_the_plain_sum():
    orc = pyoracle.oracle()
    rng = np.random.default_rng(18)
    M, N, K, P = 9, 9, 9, 16
    rowptr, colidx = random_csr(rng, N, M, 0.3)
    nnz = int(rowptr[-1])
    A = rand_values(rng, K * M * P, DT.F32); B = rand_values(rng, K * N * P, DT.F32)
    got = rand_values(rng, nnz, DT.F32)
    orc.lib.oracle_packed_spgemm_csc_csparse(N, K, P, rowptr.ctypes.data, colidx.ctypes.data, A.ctypes.data, M, B.ctypes.data, N, got.ctypes.data, 1)
    A3, B3 = A.reshape(K, M, P).astype(np.float64), B.reshape(K, N, P).astype(np.float64)
    want = np.array([(A3[:, colidx[z], :] * B3[:, n, :]).sum() for n in range(N) for z in range(rowptr[n], rowptr[n + 1])])
    assert np.allclose(got, want, rtol=1e-6, atol=1e-6)


# ---- dense packed GEMMs: restatement vs the reference's JIT kernels -------------------------------------------------
PACKED_GEMM = [(9, 9, 9, 16, 0), (4, 7, 5, 8, 1), (20, 9, 20, 16, 1), (35, 9, 35, 8, 0)]


@pytest.mark.parametrize("dt", [DT.F32, DT.F64])
@pytest.mark.parametrize("kind", ["packed", "ac_rm", "bc_rm"])
@pytest.mark.parametrize("M,N,K,P,beta0", PACKED_GEMM)
def test_packed_gemm_vs_reference_jit(reference, kind, dt, M, N, K, P, beta0):
    npdt = np.float32 if dt == DT.F32 else np.float64
    rng = np.random.default_rng(17)
    orc = pyoracle.oracle()
    flags = GEMM_FLAG.BETA_0 if beta0 else 0
    if kind == "packed":      # column-major, all packed: A [K][lda=M], B [N][ldb=K], C [N][ldc=M]
        A, B, C0 = (rng.random(K * M * P) - 0.5).astype(npdt), (rng.random(N * K * P) - 0.5).astype(npdt), (rng.random(N * M * P) - 0.5).astype(npdt)
        shape, fn, ofn = capi.gemm_shape(M, N, K, M, K, M, dt, dt, dt, dt), reference.create_packed_gemm, orc.lib.oracle_packed_gemm
        lda, ldb, ldc = M, K, M
    elif kind == "ac_rm":     # A [M][lda=K][P], B [K][ldb=N], C [M][ldc=N][P]
        A, B, C0 = (rng.random(M * K * P) - 0.5).astype(npdt), (rng.random(K * N) - 0.5).astype(npdt), (rng.random(M * N * P) - 0.5).astype(npdt)
        shape, fn, ofn = capi.gemm_shape(M, N, K, K, N, N, dt, dt, dt, dt), reference.create_packed_gemm_ac_rm, orc.lib.oracle_packed_gemm_ac_rm
        lda, ldb, ldc = K, N, N
    else:                     # A [M][lda=K], B [K][ldb=N][P], C [M][ldc=N][P]
        A, B, C0 = (rng.random(M * K) - 0.5).astype(npdt), (rng.random(K * N * P) - 0.5).astype(npdt), (rng.random(M * N * P) - 0.5).astype(npdt)
        shape, fn, ofn = capi.gemm_shape(M, N, K, K, N, N, dt, dt, dt, dt), reference.create_packed_gemm_bc_rm, orc.lib.oracle_packed_gemm_bc_rm
        lda, ldb, ldc = K, N, N
    mine = C0.copy()
    ofn(dt, M, N, K, P, A.ctypes.data, lda, B.ctypes.data, ldb, mine.ctypes.data, ldc, beta0)
    h = fn(shape, flags, 0, P)
    if not h:
        pytest.skip("the reference JIT declines this packed GEMM on this host")
    theirs = C0.copy()
    p = capi.GemmParam()
    p.a.primary, p.b.primary, p.c.primary = A.ctypes.data, B.ctypes.data, theirs.ctypes.data
    capi.Api.call(h, p)
    assert normf_rel(theirs, mine, dt) <= (1e-5 if dt == DT.F32 else 1e-12)


# ---- QUANT / DEQUANT TPPs ----------------------------------------------------------------------------
QUANT_CASES = [(DT.I8, UNARY_FLAG.SIGN_SAT_QUANT), (DT.I8, 0), (DT.I16, UNARY_FLAG.SIGN_SAT_QUANT), (DT.I32, 0), (DT.I8, UNARY_FLAG.NO_SCF_QUANT | UNARY_FLAG.SIGN_SAT_QUANT)]


@pytest.mark.parametrize("out_dt,flags", QUANT_CASES)
def test_quant_bit_identical(reference, out_dt, flags):
    rng = np.random.default_rng(9)
    x = ((rng.random(40 * 9) - 0.5) * 40.0).astype(np.float32)          # |x * 7.5| reaches 150: saturation is exercised
    x[:8] = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.6, -127.4]            # ties go to even
    scf = np.array([7.5], dtype=np.float32)
    if flags & UNARY_FLAG.NO_SCF_QUANT or not (flags & UNARY_FLAG.SIGN_SAT_QUANT):
        x = np.clip(x, -15.0, 15.0)                                      # the wrapping forms are only defined inside the target range
        x[:6] = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5]
    (a, b), _ = both_unary(reference, UNARY.QUANT, 33, 9, 40, 36, DT.F32, out_dt, flags=flags, aux_in=scf, inp=x)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("in_dt", [DT.I8, DT.I16, DT.I32])
@pytest.mark.parametrize("flags", [0, UNARY_FLAG.NO_SCF_QUANT])
def test_dequant_bit_identical(reference, in_dt, flags):
    scf = np.array([0.125], dtype=np.float32)
    (a, b), _ = both_unary(reference, UNARY.DEQUANT, 33, 9, 40, 36, in_dt, DT.F32, flags=flags, aux_in=scf)
    assert np.array_equal(a, b)
