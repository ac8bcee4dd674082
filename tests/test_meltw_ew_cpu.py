"""The element-wise parity checks of tests/meltw_ew_helpers.py proved on the reference's restatement alone (no GPU): the masks are the elements the oracle
reads, the per-element bound holds for the oracle's own libm with the recorded ratios, the checks reject five localized errors (three of which the bars of
tests/test_meltw_gpu.py accepted), the oracle equals the reference itself on the wide tables (when oracle/_ref is built), every kernel name launch_meltw can
report is asserted somewhere or excused, and expected_kernel says what the conditions of launch_meltw say.

Oracle's worst (|oracle - t| - FLT_MIN)+ / (2^-24 S_op), f32 in and out, over all_bf16() fed as f32 and f32_wide (printed by test_the_bound_holds_for_the_oracle...):
    TANH 2.407   SIGMOID 1.450   EXP 1.000   GELU 1.865   GELU_INV 1.998   TANH_INV 1.894   SIGMOID_INV 1.033   ELU 1.829
(the values meltw_ew_helpers.ORACLE_RATIO holds; the device's K_op is four times each)."""
import os
import re

import numpy as np
import pytest

import meltw_ew_helpers as H
from meltw_ew_helpers import COL, NONE, OP_BINARY, OP_TERNARY, OP_UNARY, ROW, SCALAR, EwCase
from helpers import normf_rel, rand_values
from libxsmm_amd.capi import BINARY, DT, TERNARY, UNARY
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- masks ----------------------------------------------------------------------------------------------------------------------------------------------
def test_masks_of_every_broadcast_kind_by_hand():
    m, n, ld = 3, 4, 5
    assert np.flatnonzero(H.layout(NONE, m, n, ld)).tolist() == [0, 1, 2, 5, 6, 7, 10, 11, 12, 15, 16, 17]
    assert np.flatnonzero(H.layout(ROW, m, n, ld)).tolist() == [0, 5, 10, 15]           # one value per column j, at j * ld
    assert np.flatnonzero(H.layout(COL, m, n, ld)).tolist() == [0, 1, 2]                 # the first m elements
    assert np.flatnonzero(H.layout(SCALAR, m, n, ld)).tolist() == [0]
    assert [H.extent(k, m, n, ld) for k in H.KINDS] == [18, 16, 3, 1]
    assert H.layout(ROW, m, n, ld, 20).size == 20 and H.layout(ROW, m, n, ld, 20).sum() == 4


@pytest.mark.parametrize("dt", [DT.F32, DT.BF16])
def test_masks_are_the_elements_the_oracle_reads(dt):
    """For all 16 operand-kind pairs of SUB at a padded ld: the oracle's result over poisoned operands holds no NaN, equals in0 - in1 of the LOGICAL values, and
    leaves the sentinel outside m x n.  A mask that misses an element the oracle reads shows as NaN; an element put at the wrong place as a wrong difference."""
    m, n, batch = 37, 9, 2
    rng = np.random.default_rng(3)
    vals = [H.encode(rng.integers(-8, 9, batch * n * m).astype(np.float32), dt).reshape(batch, n, m) for _ in range(2)]
    for k0 in H.KINDS:
        for k1 in H.KINDS:
            case = EwCase(OP_BINARY, BINARY.SUB, (dt, dt), dt, m, n, vals, (41, 43, 45), kinds=(k0, k1), batch=batch)
            for opd in case.ins:
                assert np.isnan(H.decode(opd.buf[~opd.mask], dt)).all() and (~opd.mask).sum() >= 5 * batch
            out = case.run_oracle()
            a, b = case.x64(0), case.x64(1)
            pick = {NONE: lambda v: v, ROW: lambda v: np.broadcast_to(v[:, :, :1], v.shape), COL: lambda v: np.broadcast_to(v[:, :1, :], v.shape),
                    SCALAR: lambda v: np.broadcast_to(v[:, :1, :1], v.shape)}
            assert np.array_equal(a, pick[k0](H.decode(vals[0], dt))) and np.array_equal(b, pick[k1](H.decode(vals[1], dt)))
            assert np.array_equal(H.decode(case.out.logical(out), dt), a - b), (k0, k1)
            assert np.array_equal(H.decode(out[~case.out.mask], dt), np.full((~case.out.mask).sum(), -7.0))
            case.check_exact(out, out)


# ---- the bound ------------------------------------------------------------------------------------------------------------------------------------------
def _approx_inputs():
    return np.concatenate([H.bf16_to_f32(H.all_bf16()), H.f32_wide(np.random.default_rng(11), 64 * 256)])


def _oracle_unary(typ, x, out_dt, in_dt=DT.F32):
    m = 256
    v = x.reshape(-1, m)
    case = EwCase(OP_UNARY, typ, (in_dt,), out_dt, m, v.shape[0], [v], (m + 8, m + 16), alpha=H.ALPHA if typ in (UNARY.LEAKY_RELU, UNARY.ELU) else None)
    return case, case.run_oracle()


def test_the_bound_holds_for_the_oracle_with_the_recorded_ratios():
    """K_op comes from here: the oracle's own worst ratio per operation (f32 out), which must not exceed the recorded ORACLE_RATIO and must come within 15 % of
    it (a recorded value far above the measurement would hand the device slack nobody measured).  Every class (NaN, +-inf) agrees; into bf16 the oracle stays
    inside the device's K_op as well."""
    x = _approx_inputs()
    measured = {}
    for typ in H.APPROX_UNARY:
        case, out = _oracle_unary(typ, x, DT.F32)
        ratio, class_ok = H.approx_ratio(typ, case.x64(0), H.decode(case.out.logical(out), DT.F32), DT.F32)
        assert class_ok.all(), int(typ)
        measured[typ] = H.oracle_ratio(typ, case.x64(0), H.decode(case.out.logical(out), DT.F32))
        case.check_approx(out, out, k=H.ORACLE_RATIO[typ])
        case16, out16 = _oracle_unary(typ, x, DT.BF16)
        case16.check_approx(out16, out16)
    print("oracle ratios:", {int(k): round(v, 3) for k, v in measured.items()})
    for typ, r in measured.items():
        assert r <= H.ORACLE_RATIO[typ] + 0.005, (int(typ), r)
        assert r >= 0.85 * H.ORACLE_RATIO[typ], (int(typ), r)
        assert H.K_OP[typ] == 4.0 * H.ORACLE_RATIO[typ]


def test_exact_unary_ops_are_exact_in_float64_terms():
    """SQRT, RECIPROCAL and RECIPROCAL_SQRT of the oracle are correctly rounded operations (1 / sqrt: two of them): the f32 result is within one / two roundings of
    the float64 value -- why the device is held to the oracle's bits for them and not to a libm bound."""
    x = _approx_inputs()
    x = x[np.isfinite(x) & (x > 2.0 ** -60) & (x < 2.0 ** 60)]
    x = x[: x.size // 256 * 256]
    for typ, f, roundings in ((UNARY.SQRT, np.sqrt, 1), (UNARY.RECIPROCAL, lambda v: 1 / v, 1), (UNARY.RECIPROCAL_SQRT, lambda v: 1 / np.sqrt(v), 2)):
        case, out = _oracle_unary(typ, x, DT.F32)
        t = f(case.x64(0))
        assert np.all(np.abs(H.decode(case.out.logical(out), DT.F32) - t) <= roundings * 2.0 ** -24 * np.abs(t) * (1 + 2.0 ** -20))


# ---- mutations ------------------------------------------------------------------------------------------------------------------------------------------
def _rejected(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)
    return True


def test_mutation_1_a_truncating_bf16_store_is_rejected_and_the_old_bar_took_it():
    x = H.f32_wide(np.random.default_rng(11), 64 * 256)
    x = np.where(np.isfinite(x) & (np.abs(x) < 1e15), x, np.float32(1.5)).astype(np.float32)
    case, ref = _oracle_unary(UNARY.X2, x, DT.BF16)
    with np.errstate(over="ignore"):
        y = (x * x).astype(np.float32)
    y = np.where(np.abs(y) < H.FLT_MIN, np.float32(0) * y, y)                   # the reference flushes denormals before it rounds
    got = ref.copy()
    got[case.out.mask] = (y.view(np.uint32) >> 16).astype(np.uint16)
    assert 0.2 < np.mean(got != ref) < 0.6                                     # about half of all roundings go up
    old = normf_rel(case.out.logical(ref), case.out.logical(got), DT.BF16)
    print("truncating store, old bar:", old)
    assert 0 < old < 7e-3
    assert _rejected(case.check_exact, ref, got)
    case.check_exact(ref, ref)


def test_mutation_2_max_as_fmaxf_is_rejected_and_driver_values_never_showed_it():
    a, b = H.pair_grid(DT.F32)
    case = EwCase(OP_BINARY, BINARY.MAX, (DT.F32, DT.F32), DT.F32, 256, 256, [a, b], (264, 272, 280))
    ref = case.run_oracle()
    got = ref.copy()
    got[case.out.mask] = np.fmax(a, b).ravel()
    assert _rejected(case.check_exact, ref, got)
    nan_one = np.isnan(a) ^ np.isnan(b)
    assert np.isnan(case.out.logical(ref)[0][nan_one]).sum() > 0 and not np.isnan(np.fmax(a, b)[nan_one]).any()      # (a > b) ? a : b hands b on, fmaxf the number
    rng = np.random.default_rng(5)
    da, db = rand_values(rng, 45 * 13, DT.F32).reshape(13, 45), rand_values(rng, 45 * 13, DT.F32).reshape(13, 45)
    drv = EwCase(OP_BINARY, BINARY.MAX, (DT.F32, DT.F32), DT.F32, 45, 13, [da, db], (48, 45, 50))
    dref = drv.run_oracle()
    assert np.array_equal(drv.out.logical(dref)[0], np.fmax(da, db))             # the old test's array_equal on these values accepts fmaxf


def test_mutation_3_row_and_column_broadcast_swapped_are_rejected():
    """in0 is a ROW operand at a padded ld: a kernel that reads it as a column vector (element i), or with ld = m (element j * m), reads poison or the wrong value."""
    m, n = 37, 9
    rng = np.random.default_rng(6)
    vals = [H.encode(rng.standard_normal(2 * n * m), DT.F32).reshape(2, n, m) for _ in range(2)]
    case = EwCase(OP_BINARY, BINARY.SUB, (DT.F32, DT.F32), DT.F32, m, n, vals, (41, 43, 45), kinds=(ROW, NONE), batch=2)
    ref = case.run_oracle()
    swapped = EwCase(OP_BINARY, BINARY.SUB, (DT.F32, DT.F32), DT.F32, m, n, vals, (41, 43, 45), kinds=(ROW, NONE), batch=2)
    swapped.flags = H.bcast_flags(OP_BINARY, (COL, NONE))
    assert _rejected(case.check_exact, ref, swapped.run_oracle())
    wrong_ld = EwCase(OP_BINARY, BINARY.SUB, (DT.F32, DT.F32), DT.F32, m, n, vals, (41, 43, 45), kinds=(ROW, NONE), batch=2)
    wrong_ld.lds = (m, 43, 45)
    got = wrong_ld.run_oracle()
    assert np.isnan(case.out.logical(got)).any()
    assert _rejected(case.check_exact, ref, got)


def test_mutation_4_one_tanh_element_64_ulps_off_is_rejected_and_the_old_bar_took_it():
    x = H.f32_wide(np.random.default_rng(11), 64 * 256)
    case, ref = _oracle_unary(UNARY.TANH, x, DT.F32)
    case.check_approx(ref, ref)
    with np.errstate(invalid="ignore"):
        k = int(np.flatnonzero(case.out.mask)[np.nanargmin(np.abs(x - 0.7))])
    got = ref.copy()
    got.view(np.uint32)[k] += 64
    fin = np.isfinite(x)
    old = normf_rel(case.out.logical(ref).ravel()[fin], case.out.logical(got).ravel()[fin], DT.F32)
    print("64 ulps, old bar:", old)
    assert 0 < old < 7e-4
    assert _rejected(case.check_approx, ref, got)
    for ulps in (16, 10):                                                       # K_op = 8.92 in units of 2^-24 |t|: 16 and 10 ulps (2^-23 |t| each at most) are out as well
        g2 = ref.copy(); g2.view(np.uint32)[k] += ulps
        assert _rejected(case.check_approx, ref, g2)


@pytest.mark.parametrize("approx", [False, True])
def test_mutation_5_one_byte_at_row_m_of_a_padded_output_is_rejected(approx):
    x = H.f32_wide(np.random.default_rng(11), 64 * 256)
    case, ref = _oracle_unary(UNARY.TANH if approx else UNARY.X2, x, DT.BF16)
    got = ref.copy()
    row_m = case.out.off + 256                                                  # element (m, 0): the first padding row of column 0
    assert not case.out.mask[row_m] and case.out.mask[row_m - 1]
    got.view(np.uint8)[row_m * 2] ^= 1
    assert _rejected(case.check_approx if approx else case.check_exact, ref, got)


def test_same_bits_takes_nan_for_nan_and_nothing_else():
    r = np.array([0x7fc00000, 0xffc00000, 0x7fc00000, 0x7f800001, 0x3f800000, 0x00000000], dtype=np.uint32).view(np.float32)
    g = np.array([0xffc00000, 0x7fc12345, 0x7f800001, 0x7f800001, 0x3f800001, 0x80000000], dtype=np.uint32).view(np.float32)
    assert H.same_bits(r, g, DT.F32).tolist() == [True, True, False, True, False, False]
    rb, gb = np.array([0x7fc0, 0x7f81], dtype=np.uint16), np.array([0xffc1, 0x7fc1], dtype=np.uint16)
    assert H.same_bits(rb, gb, DT.BF16).tolist() == [True, False]


# ---- oracle against the reference -----------------------------------------------------------------------------------------------------------------------
needs_reference = pytest.mark.skipif(not pyoracle.have_reference(), reason="oracle/_ref/libxsmm_ref.so not built")


def _against_reference(case, pure=False):
    out, ref = case.run_oracle(), case.run_reference()
    case.check_exact(ref, out, pure=pure, what="oracle against the reference")


@needs_reference
@pytest.mark.parametrize("typ", H.EXACT_UNARY + H.APPROX_UNARY, ids=lambda t: str(int(t)))
def test_oracle_equals_the_reference_unary(typ):
    """Same libm on both sides: same bits, the transcendental ones included."""
    from test_meltw_ew_gpu import UNARY_COMBOS, unary_case
    for table, in_dt, out_dt in UNARY_COMBOS:
        _against_reference(unary_case(typ, table, in_dt, out_dt, "general"))
    v = H.f32_on_bf16_boundaries().reshape(-1, 512)
    if typ in (UNARY.IDENTITY, UNARY.X2):
        _against_reference(EwCase(OP_UNARY, typ, (DT.F32,), DT.BF16, 512, v.shape[0], [v], (520, 528)))


@needs_reference
@pytest.mark.parametrize("dts_name", ["f32", "bf16", "bf16_f32_f32", "bf16_f32_bf16", "f64"])
def test_oracle_equals_the_reference_binary(dts_name):
    from test_meltw_ew_gpu import ARITH, BINARY_DTS, _pairs, binary_case
    for typ in ARITH:
        _against_reference(binary_case(typ, dts_name, "general"))
    if dts_name in ("f32", "bf16"):
        d0, d1, _ = BINARY_DTS[dts_name]
        for typ in (BINARY.CMP_OP_GT, BINARY.CMP_OP_GE, BINARY.CMP_OP_LT, BINARY.CMP_OP_LE, BINARY.CMP_OP_EQ, BINARY.CMP_OP_NE):
            _against_reference(EwCase(OP_BINARY, typ, (d0, d1), d0, 256, 256, [_pairs(d0)[0], _pairs(d1)[1]], (259, 261, 270), out_bits=True))


@needs_reference
@pytest.mark.parametrize("dt", [DT.F32, DT.BF16])
def test_oracle_equals_the_reference_ternary(dt):
    from test_meltw_ew_gpu import _triples, bcast_case, kind_tuples
    vals = list(_triples(dt))
    for typ in (TERNARY.MULADD, TERNARY.NMULADD):
        _against_reference(EwCase(OP_TERNARY, typ, (dt,) * 3, dt, 40, 1600, vals, (48, 56, 64, 72)))
    bits = np.random.default_rng(13).integers(0, 256, 4 * 1600 * 16, dtype=np.uint8)
    _against_reference(EwCase(OP_TERNARY, TERNARY.SELECT, (dt, dt), dt, 40, 1600, vals[:2], (43, 45, 50, 47), select_bits=bits), pure=True)
    for kinds in kind_tuples(3):
        _against_reference(bcast_case(OP_TERNARY, TERNARY.NMULADD, (dt,) * 4, "general", kinds))


# ---- which kernel ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_name_launch_meltw_can_report_is_asserted_or_excused():
    """Every `*name = "..."` literal of csrc/meltw_kernels.hip is a key of test_meltw_ew_gpu.NAMES; a value names this suite's GPU file (whose rows assert the five
    element-wise kernels), `file::test` of another GPU test file that holds the quoted name next to a hip_kernel_name assertion, or starts with `reason:`."""
    from test_meltw_ew_gpu import GENERAL, HERE, NAMES, PATH_KERNEL, REFUSED
    assert all(len(why) > 20 for why in REFUSED.values())            # a combination dispatch refuses stays in the table with its reason
    src = open(os.path.join(ROOT, "libxsmm_amd", "csrc", "meltw_kernels.hip")).read()
    names = set(re.findall(r'\*name = (?:[^;"]*\? )?"([^"]+)"(?: : "([^"]+)")?', src))
    names = {n for pair in names for n in pair if n}
    assert len(names) >= 30 and "meltw_unary_vec4_kernel" in names and "reduce_cols_listed_f64_kernel" in names, sorted(names)
    assert names == set(NAMES), (sorted(names - set(NAMES)), sorted(set(NAMES) - names))
    here = {k for k, v in NAMES.items() if v == HERE}
    assert here == set(PATH_KERNEL.values()) | set(GENERAL.values())
    for name, where in NAMES.items():
        if where == HERE:
            continue
        if where.startswith("reason:"):
            assert len(where) > 40
            continue
        path, _, test = where.partition("::")
        text = open(os.path.join(ROOT, path)).read()
        assert test and re.search(r"^def " + test + r"\(", text, re.M), where
        assert f'"{name}"' in text and "hip_kernel_name" in text, f"{where} does not assert {name}"


def test_expected_kernel_against_hand_written_cases():
    F, B = DT.F32, DT.BF16
    ek = H.expected_kernel
    U, Bi, T = OP_UNARY, OP_BINARY, OP_TERNARY
    # all f32: four per thread
    assert ek(U, UNARY.TANH, (F,), F, 64, 7, (64,), 68, (NONE,), (0,), 0, (0,), 0) == "meltw_ew8_kernel"
    assert ek(U, UNARY.TANH, (F,), F, 12, 7, (12,), 20, (NONE,), (0,), 0, (0,), 0) == "meltw_ew8_kernel"
    assert ek(U, UNARY.TANH, (F,), F, 64, 7, (66,), 68, (NONE,), (0,), 0, (0,), 0) == "meltw_unary_kernel"           # ldi % 4
    assert ek(U, UNARY.TANH, (F,), F, 64, 7, (64,), 68, (NONE,), (8,), 8, (0,), 0) == "meltw_unary_kernel"           # 8 bytes off: f32 wants 16 in both vector kernels
    # bf16: eight per thread, else four, else one
    assert ek(U, UNARY.RELU, (B,), B, 64, 7, (64,), 72, (NONE,), (0,), 0, (0,), 0) == "meltw_ew8_kernel"
    assert ek(U, UNARY.RELU, (B,), B, 64, 7, (64,), 72, (NONE,), (0,), 0, (0,), 0, bitmask=True) == "meltw_unary_kernel"
    assert ek(U, UNARY.RELU, (B,), B, 12, 7, (12,), 20, (NONE,), (0,), 0, (0,), 0) == "meltw_unary_vec4_kernel"      # m % 8
    assert ek(U, UNARY.RELU, (B,), B, 64, 7, (64,), 72, (NONE,), (8,), 8, (0,), 0) == "meltw_unary_vec4_kernel"      # 8 bytes off
    assert ek(U, UNARY.RELU, (B,), B, 64, 7, (64,), 72, (NONE,), (0,), 0, (136,), 144) == "meltw_unary_vec4_kernel"  # batch stride 8 mod 16
    assert ek(U, UNARY.RELU, (B,), B, 64, 7, (64,), 72, (NONE,), (2,), 2, (0,), 0) == "meltw_unary_kernel"           # one element off
    assert ek(U, UNARY.RELU, (B,), B, 64, 7, (64,), 72, (NONE,), (0,), 0, (130,), 130) == "meltw_unary_kernel"
    assert ek(U, UNARY.RELU, (B,), F, 12, 7, (12,), 20, (NONE,), (0,), 0, (0,), 0) == "meltw_unary_kernel"           # mixed types: eight or one
    assert ek(U, UNARY.RELU, (B,), B, 33, 7, (40,), 35, (NONE,), (0,), 0, (0,), 0) == "meltw_unary_kernel"
    assert ek(U, UNARY.X2, (B,), B, 40, 9, (41,), 48, (ROW,), (2,), 0, (6,), 0) == "meltw_ew8_kernel"                # a ROW operand: any ld, any alignment
    assert ek(U, UNARY.X2, (B,), B, 40, 9, (41,), 48, (COL,), (2,), 0, (0,), 0) == "meltw_unary_kernel"              # a COL operand is loaded 16 bytes at a time
    assert ek(U, UNARY.X2, (B,), B, 40, 9, (48,), 48, (ROW,), (0,), 0, (0,), 0) != "meltw_unary_vec4_kernel"
    assert ek(U, UNARY.X2, (DT.F16,), F, 64, 9, (64,), 64, (NONE,), (0,), 0, (0,), 0) == "meltw_unary_kernel"
    assert ek(U, UNARY.X2, (DT.F64,), DT.F64, 64, 9, (64,), 64, (NONE,), (0,), 0, (0,), 0) == "meltw_unary_kernel"
    # binary / ternary
    assert ek(Bi, BINARY.SUB, (B, F), F, 40, 9, (48, 56), 64, (NONE, NONE), (0, 0), 0, (0, 0), 0) == "meltw_ew8_kernel"
    assert ek(Bi, BINARY.SUB, (B, F), F, 44, 9, (48, 56), 64, (NONE, NONE), (0, 0), 0, (0, 0), 0) == "meltw_binary_kernel"    # mixed: m % 8
    assert ek(Bi, BINARY.SUB, (F, F), F, 44, 9, (48, 56), 64, (NONE, NONE), (0, 0), 0, (0, 0), 0) == "meltw_ew8_kernel"
    assert ek(Bi, BINARY.SUB, (F, F), F, 44, 9, (48, 56), 64, (NONE, NONE), (0, 4), 0, (0, 0), 0) == "meltw_binary_kernel"
    assert ek(Bi, BINARY.SUB, (F, F), F, 44, 9, (48, 57), 64, (NONE, SCALAR), (0, 4), 0, (0, 4), 0) == "meltw_ew8_kernel"
    assert ek(Bi, BINARY.CMP_OP_GT, (F, F), F, 64, 9, (64, 64), 64, (NONE, NONE), (0, 0), 0, (0, 0), 0) == "meltw_binary_kernel"
    assert ek(Bi, BINARY.ADD, (DT.F64, DT.F64), DT.F64, 64, 9, (64, 64), 64, (NONE, NONE), (0, 0), 0, (0, 0), 0) == "meltw_binary_kernel"
    assert ek(T, TERNARY.NMULADD, (B, B, B), B, 40, 9, (48, 56, 64), 72, (NONE, COL, ROW), (0, 0, 2), 0, (0, 0, 0), 0) == "meltw_ew8_kernel"
    assert ek(T, TERNARY.NMULADD, (B, B, B), B, 37, 9, (41, 49, 57), 46, (NONE, COL, ROW), (0, 0, 0), 0, (0, 0, 0), 0) == "meltw_ternary_kernel"
    assert ek(T, TERNARY.SELECT, (F, F, F), F, 40, 9, (48, 48, 48), 48, (NONE,) * 3, (0, 0, 0), 0, (0, 0, 0), 0) == "meltw_ternary_kernel"


def test_every_gpu_row_expects_the_kernel_its_path_names():
    """The rows of tests/test_meltw_ew_gpu.py, built here without a GPU: expected() of each case is the kernel its path was written for."""
    import test_meltw_ew_gpu as G
    for typ, table, in_dt, out_dt, path in G.unary_rows():
        assert G.unary_case(typ, table, in_dt, out_dt, path).expected() == G.PATH_KERNEL.get(path, "meltw_unary_kernel"), (int(typ), table, path)
    for typ in G.ARITH:
        for name in G.BINARY_DTS:
            for path in ("stream", "general"):
                want = "meltw_ew8_kernel" if (path == "stream" and name != "f64") else "meltw_binary_kernel"
                assert G.binary_case(typ, name, path).expected() == want
    seen = set()
    for op, typ, name, path in G.bcast_rows():
        for kinds in G.kind_tuples(op):
            case = G.bcast_case(op, typ, G.BC_DTS[op][name], path, kinds)
            assert case.expected() == ("meltw_ew8_kernel" if path == "stream" else G.GENERAL[op]), (op, name, path, kinds)
            seen.add(case.expected())
    for path in G.SMALL_PATHS:
        for dt in (DT.F32, DT.BF16):
            for op, typ in ((OP_UNARY, UNARY.RELU), (OP_BINARY, BINARY.MULADD), (OP_TERNARY, TERNARY.NMULADD)):
                want = "meltw_unary_vec4_kernel" if (path == "off_8_bytes" and op == OP_UNARY and dt == DT.BF16) else G.GENERAL[op]
                assert G.small_case(op, typ, dt, path).expected() == want, (path, int(dt), op)
    assert seen == {"meltw_ew8_kernel"} | set(G.GENERAL.values())
