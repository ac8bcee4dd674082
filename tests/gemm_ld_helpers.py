"""Dense GEMM / BRGEMM parity at PADDED leading dimensions: what tests/sparse_helpers.py does for the packed and sparse kernels, for a constructed GemmCase.

  logical_masks(case)  boolean masks over case.A / B / C0 / D / S / SB: the elements the operation may read (C: the m x n result), for every layout GemmCase
                       builds -- flat, TRANS_A / TRANS_B, VNNI_A [k/vf][lda][vf], VNNI_B, VNNI_C, the MXFP4 / MX x MX element and scale layouts, all nbr
                       blocks of all batch elements.  The index formulas are the oracle's (oracle/oracle_gemm.c: a_index / b_index, contract_*).
  poison(case)         in place: input gaps get the type's quiet NaN (integers and E2M1 pairs, which have none, their largest-magnitude code: those kernels are
                       compared bit for bit), C's gaps a finite sentinel the data cannot produce (-7 in the type, C_GAP_INT for integers).
  ref64(case)          (ref, mag, terms): float64 restatement of sum over the batch-reduce blocks of A * B (+ C0 with beta = 1) (+ column bias), ReLU, on the
                       logical sub-arrays decoded with helpers.as_float; shape [batch][n][m].
  assert_dense(...)    no non-finite result; every byte outside m x n equals the oracle's buffer; a per-element bound where ref64 applies, else the oracle
                       bars of the suite per batch element.

ref64 covers f32, f64, bf16, f16, E5M2 / E4M3 operands with f32 C, and 8-bit integer operands with i32 C (exact).  NOT covered -- these stay on the oracle, per
problem: the MX types, BF32 (the operands are rounded to bf16 first), low-bit weights, 8-bit weights x bf16, 8-bit integers with a scaled f32 C, the sigmoid, and
C of an 8-bit float type (held to its code-distance bar).

One rounding rule of the operation is part of ref64 because it is the operation's definition, not the kernel's error: IEEE-half GEMMs add the start value
(C0, bias) AFTER the sum and round it to a half on the way in [oracle_gemm.c: contract_f16, contract_fused_lowp]."""
import numpy as np

from helpers import TOL_BF16, TOL_F32, TOL_F64, as_float, normf_rel
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG as F

from sparse_helpers import C_GAP             # the same sentinel as the packed / sparse suite: -7 in C's type

C_GAP_INT = -70007          # |sum| of 8-bit integer cases stays far below
FP8 = (DT.BF8, DT.HF8)
INT8 = (DT.I8, DT.U8)
# quiet NaN per type; for types without one the largest-magnitude code
NAN_CODE = {DT.BF16: 0x7fc0, DT.F16: 0x7e00, DT.BF8: 0x7e, DT.HF8: 0x7f, DT.MXBF8: 0x7e, DT.MXHF8: 0x7f, DT.MXFP4X2: 0xff, DT.I8: -128, DT.U8: 255}
E8M0_NAN = 0xff
# -7 = -1.75 * 2^2 in each C type
GAP_CODE = {DT.BF16: 0xc0e0, DT.F16: 0xc700, DT.BF8: 0xc7, DT.HF8: 0xce}


def _vf_a(case):
    """k-pack factor of A's VNNI layout as the oracle reads it (1: flat)."""
    va = bool(case.flags & F.VNNI_A)
    a, b = case.a_type, case.b_type
    if a in (DT.BF16, DT.F16):
        return 2 if va else 1
    if a in FP8:
        return (2 if b == DT.BF16 else 4) if va else 1
    if a in INT8 and b in INT8:
        return 4 if (va or case.c_type == DT.F32) else 1
    return 1


def _a_index(case):
    """flat element (byte for the MX types) index of A(i, s) inside one block: int array [m][k'] (k' = the k positions stored per element)."""
    m, k, lda = case.m, case.k, case.lda
    i = np.arange(m)[:, None]
    if case.mx:                                        # [k/2][lda] bytes, two k per byte
        return (np.arange(k // 2)[None, :] * lda + i)
    if case.mxmx:                                      # [k/8][lda][4] (E2M1 pairs) / [k/4][lda][4] bytes
        g = np.arange(k // (2 if case.a_type == DT.MXFP4X2 else 1))[None, :]
        return (g // 4) * (lda * 4) + i * 4 + g % 4
    s = np.arange(k)[None, :]
    if case.flags & F.TRANS_A:
        return i * lda + s
    kb = _vf_a(case)
    return (s // kb) * (lda * kb) + i * kb + s % kb


def _b_index(case):
    """flat index of B(s, j) inside one block: [k'][n]."""
    n, k, ldb = case.n, case.k, case.ldb
    j = np.arange(n)[None, :]
    if case.mxmx:
        g = np.arange(k // (2 if case.a_type == DT.MXFP4X2 else 1))[:, None]
        return (g // 4) * (ldb * 4) + j * 4 + g % 4
    s = np.arange(k)[:, None]
    tb, vb = bool(case.flags & F.TRANS_B), bool(case.flags & F.VNNI_B)
    if tb and vb:
        kb = _vf_a(case)
        return j * kb + (s // kb) * (ldb * kb) + s % kb
    if tb:
        return s * ldb + j
    return j * ldb + s


def _c_index(case):
    """flat index of C(i, j) inside one batch element: [n][m]."""
    i, j = np.arange(case.m)[None, :], np.arange(case.n)[:, None]
    if case.flags & F.VNNI_C:
        vf = 4 if capi.DT_SIZE[case.c_type] == 1 else 2
        return (j // vf) * (case.ldc * vf) + i * vf + j % vf
    return j * case.ldc + i


def _scale_index(rows, ld, k):
    return np.arange(k // 32)[:, None] * ld + np.arange(rows)[None, :]


def _block_mask(idx, elems, nblocks):
    one = np.zeros(elems, dtype=bool)
    one[idx.ravel()] = True
    return np.tile(one, nblocks)


def block_masks(case):
    """The masks of ONE block of A, of B and of one C (callers that keep their blocks in pools of their own: the segments tests)."""
    return (_block_mask(_a_index(case), case.a_elems, 1), _block_mask(_b_index(case), case.b_elems, 1), _block_mask(_c_index(case), case.c_elems, 1))


def gap_values(case):
    """(A gap value, B gap value, C sentinel) as poison writes them."""
    return _nan_of(case.a_type, case.A), _nan_of(case.b_type, case.B), _gap_of(case.c_type, case.C0)


def logical_masks(case):
    """{"A", "B", "C0", "D", "S", "SB"} -> boolean mask of the buffer's shape (None where the case has no such buffer)."""
    nb_b = (1 if case.B.size == case.nbr * case.b_elems else case.batch) * case.nbr
    out = {"A": _block_mask(_a_index(case), case.a_elems, case.batch * case.nbr), "B": _block_mask(_b_index(case), case.b_elems, nb_b),
           "C0": _block_mask(_c_index(case), case.c_elems, case.batch), "D": None if case.D is None else np.ones(case.D.size, dtype=bool), "S": None, "SB": None}
    if case.mx or case.mxmx:
        out["S"] = _block_mask(_scale_index(case.m, case.lda, case.k), case.s_elems, case.batch * case.nbr)
    if case.mxmx:
        out["SB"] = _block_mask(_scale_index(case.n, case.ldb, case.k), case.sb_elems, case.SB.size // case.sb_elems)
    for name, mk in out.items():
        assert mk is None or mk.shape == getattr(case, name).shape, name
    return out


def _nan_of(dt, arr):
    if dt in (DT.F32, DT.F64, DT.BF32):
        return np.nan
    return np.array(NAN_CODE[dt]).astype(arr.dtype)


def _gap_of(dt, arr):
    if dt in (DT.F32, DT.F64):
        return C_GAP
    if dt in GAP_CODE:
        return np.array(GAP_CODE[dt]).astype(arr.dtype)
    return C_GAP_INT        # i32


def poison(case):
    """Overwrite every gap of the case's buffers in place; returns the masks."""
    mk = logical_masks(case)
    case.A[~mk["A"]] = _nan_of(case.a_type, case.A)
    case.B[~mk["B"]] = _nan_of(case.b_type, case.B)
    case.C0[~mk["C0"]] = _gap_of(case.c_type, case.C0)
    if case.D is not None:
        case.D[~mk["D"]] = _gap_of(case.c_type, case.D)
    if mk["S"] is not None:
        case.S[~mk["S"]] = E8M0_NAN
    if mk["SB"] is not None:
        case.SB[~mk["SB"]] = E8M0_NAN
    return mk


def logical_c(case, Cbuf):
    """[batch][n][m] view-copy of the result inside a C buffer (VNNI_C included)."""
    return np.ascontiguousarray(Cbuf.reshape(case.batch, case.c_elems)[:, _c_index(case)])


def _ref64_applies(case):
    a, b, c = case.a_type, case.b_type, case.c_type
    if case.act == 3 or case.mx or case.mxmx or a != b:
        return False
    if a in (DT.F32, DT.F64):
        return c == a
    if a in (DT.BF16, DT.F16):
        return c in (a, DT.F32)
    if a in FP8:
        return c == DT.F32
    return False


def _exact_applies(case):
    return case.a_type in INT8 and case.b_type in INT8 and case.c_type == DT.I32


def _operands(case, conv):
    """A [batch][nbr][m][k], B [batch or 1][nbr][k][n] (block r of B is the one the batch-reduce mode pairs with block r of A), C0 [batch][n][m]."""
    A = conv(case.A, case.a_type).reshape(case.batch, case.nbr, case.a_elems)[:, :, _a_index(case)]
    B = conv(case.B, case.b_type).reshape(-1, case.nbr, case.b_elems)[:, :, _b_index(case)]
    if case.br_type == capi.BR_OFFSET:
        A, B = A[:, (case.offs_a // case.br_stride_a)], B[:, (case.offs_b // case.br_stride_b)]
    elif case.br_type == capi.BR_ADDRESS:
        B = B[:, ::-1]
    return A, B, conv(case.C0, case.c_type).reshape(case.batch, case.c_elems)[:, _c_index(case)]


def _contract(A, B):
    """sum over the blocks r of A_r B_r as [batch][n][m] (a B shared by the batch broadcasts)."""
    return np.matmul(B.transpose(0, 1, 3, 2), A.transpose(0, 1, 3, 2)).sum(axis=1)


def _ref64_pre(case):
    """(pre-activation, mag, terms) in float64, [batch][n][m]."""
    A, B, C0 = _operands(case, as_float)
    pre, mag = _contract(A, B), _contract(np.abs(A), np.abs(B))
    terms = case.nbr * case.k
    start = None
    if not case.flags & F.BETA_0:
        start, terms = C0, terms + 1
    if case.colbias:
        bias = as_float(case.D, case.c_type).reshape(case.batch, 1, case.m)
        start, terms = (bias if start is None else bias + start), terms + 1
    if start is not None:
        if case.a_type == DT.F16:                       # the operation rounds the start value to a half before it adds it
            start = np.broadcast_to(start, pre.shape).astype(np.float32).astype(np.float16).astype(np.float64)
        pre, mag = pre + start, mag + np.abs(start)
    return pre, mag, terms


def ref64(case):
    """(ref, mag, terms), or None where the restatement does not apply (module docstring)."""
    if _exact_applies(case):
        A, B, C0 = _operands(case, lambda x, dt: x.astype(np.int64))
        ref = _contract(A, B)
        return (ref if case.flags & F.BETA_0 else ref + C0), None, 0
    if not _ref64_applies(case):
        return None
    pre, mag, terms = _ref64_pre(case)
    return (np.maximum(pre, 0.0) if case.act in (1, 2) else pre), mag, terms


def _u(dt):
    return {DT.F64: 2.0 ** -53, DT.F32: 2.0 ** -24, DT.BF16: 2.0 ** -8, DT.F16: 2.0 ** -11}[dt]


def _tiny(dt):
    return {DT.F64: 2.0 ** -1022, DT.F32: 2.0 ** -126, DT.BF16: 2.0 ** -126, DT.F16: 2.0 ** -14}[dt]


def bound64(case, ref, mag, terms):
    """|got - ref| <= e + u_c (|ref| + e) + tiny, e = (terms + 2) u mag: assert_componentwise's bound plus one rounding to C's type."""
    acc = DT.F64 if case.a_type == DT.F64 else DT.F32
    e = (terms + 2) * _u(acc) * mag
    u_c = _u(case.c_type) if case.c_type in (DT.BF16, DT.F16) else 0.0
    return e + u_c * (np.abs(ref) + e) + _tiny(case.c_type), e + _tiny(acc)


def oracle_tol(case):
    return {DT.BF16: TOL_BF16, DT.F64: TOL_F64, DT.F16: 1e-3}.get(case.c_type, TOL_F32)


def _fp8_key(x):
    x = x.astype(np.int32)
    return np.where(x & 0x80, -(x & 0x7f), x & 0x7f)                                 # sign-magnitude -> monotonic


def assert_outside_equals_oracle(case, got, ref_oracle):
    """Every byte of got outside the m x n result equals the oracle's buffer (run from the same C0): the caller's padding came back, VNNI_C pad columns hold
    what the reference writes there."""
    out = ~logical_masks(case)["C0"]
    g, r = got.reshape(-1)[out], ref_oracle.reshape(-1)[out]
    assert np.array_equal(g.view(np.uint8), r.view(np.uint8)), f"{np.count_nonzero(g != r)} elements of C outside m x n differ from the reference's buffer"


def assert_dense(case, got, ref_oracle, got_mask=None, stats=None):
    """got / ref_oracle: the C buffers of run_gpu and run_oracle on the SAME case; got_mask: the ReLU bit mask run_gpu returned (act = 2).
    stats: optional dict, receives "ratio" = the worst err / bound (per-element part) or "normf" = the worst per-problem normf_rel."""
    g_raw = logical_c(case, got)
    g = g_raw.astype(np.int64) if case.c_type == DT.I32 else as_float(g_raw, case.c_type)
    assert np.all(np.isfinite(g)), f"{np.count_nonzero(~np.isfinite(g))} non-finite results (a gap was read?)"
    assert_outside_equals_oracle(case, got, ref_oracle)
    r64 = ref64(case)
    if r64 is not None and r64[1] is None:              # integers: exact
        assert np.array_equal(g, r64[0]), f"{np.count_nonzero(g != r64[0])} integer results differ"
        if stats is not None:
            stats["ratio"] = 0.0
    elif r64 is not None:
        ref, mag, terms = r64
        bound, _ = bound64(case, ref, mag, terms)
        err = np.abs(g - ref)
        if stats is not None:
            stats["ratio"] = float(np.max(err / bound))
        bad = err > bound
        assert not bad.any(), (f"{np.count_nonzero(bad)} elements outside the per-element bound; worst err / bound {float(np.max(err / bound)):.3f} at "
                               f"(batch, j, i) = {tuple(int(x) for x in np.unravel_index(np.argmax(err / bound), err.shape))}")
    else:
        r_raw = logical_c(case, ref_oracle)
        if case.c_type in FP8:
            gk, rk = _fp8_key(g_raw.view(np.uint8)), _fp8_key(r_raw.view(np.uint8))
            assert np.max(np.abs(gk - rk)) <= 1 and np.mean(gk != rk) < 0.03, (int(np.max(np.abs(gk - rk))), float(np.mean(gk != rk)))
        else:
            worst = max(normf_rel(r_raw[b], g_raw[b], case.c_type) for b in range(case.batch))
            if stats is not None:
                stats["normf"] = worst
            assert worst < oracle_tol(case), f"worst problem: normf_rel={worst}"
    if got_mask is not None:
        gb = case.valid_mask_bits(got_mask)
        if _ref64_applies(case):
            pre, mag, terms = _ref64_pre(case)
            _, bound_pre = bound64(case, pre, mag, terms)
            decided = np.abs(pre) > bound_pre
        else:                                           # no restatement: the oracle's pre-activation at the suite's fixed thresholds
            act, case.act = case.act, 0
            try:
                pre = as_float(logical_c(case, case.run_oracle()[0]), case.c_type)
            finally:
                case.act = act
            decided = np.abs(pre) > (1e-5 if case.c_type in (DT.F32, DT.F64) else 1e-2)
        assert decided.mean() > 0.5
        assert np.array_equal(gb[decided], (pre > 0)[decided].astype(gb.dtype)), f"{np.count_nonzero(gb[decided] != (pre > 0)[decided])} decided ReLU mask bits differ"
