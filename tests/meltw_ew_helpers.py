"""Element-wise TPP parity (libxsmm_dispatch_meltw_unary / binary / ternary) over the WHOLE input range, at padded leading dimensions, with poisoned
input gaps, per element -- what tests/gemm_ld_helpers.py does for the dense GEMMs.

  tables        all_bf16 / all_f16 / all_fp8: every bit pattern; f32_on_bf16_boundaries: every upper half crossed with the lower halves around the RNE tie;
                f32_wide: normal * 2^[-20, 8], a sweep of [-12, 12], the overflow / underflow points of expf, +-0, denormals, inf, NaN; f32_on_narrow_boundaries:
                every value of F16 / E5M2 / E4M3, every midpoint between two neighbours and its two f32 neighbours; pair_grid / triple_grid: about 256 (40)
                interesting values of a type crossed with themselves.
  layout        the elements an operand of broadcast kind none / row / col / scalar owns (the oracle's elem_index: row reads j * ld, col the first m, scalar
                element 0) and extent, the number of elements the runtime stages for a host-resident operand of that kind.
  EwCase        one TPP call: operands built at their extent plus a tail, every element outside the mask holds the type's NaN (inputs) or -7 (output); runs the
                oracle and the device on the same bytes; knows the kernel the dispatcher must pick (expected_kernel restates ew8_ok and the vec4 condition of
                csrc/meltw_kernels.hip: launch_meltw).
  same_bits     equal bit patterns, or NaN on both sides with the same quiet bit: a NaN that arithmetic PRODUCES is the negative default NaN on x86 and the
                positive one on CDNA, and a NaN that passes through an operation keeps its payload on one and not on the other.
  assert_exact  same_bits on every logical element and array_equal on every byte outside (pure moves: array_equal on everything).
  assert_approx the operations that call libm, per element against a float64 restatement t of the SAME formula:
                    |got - t| <= K_op 2^-24 S_op(x) + u_out |t| + FLT_MIN
                S_op is the sum of the magnitudes the f32 formula adds (so a cancelling tail -- GELU at x = -9, 1 - tanh^2 at |x| = 9 -- is held to the absolute
                error of its terms, not to a relative error of a result that is all rounding), u_out the unit round-off of the output type, FLT_MIN lets a libm
                flush a denormal result.  Non-finite t: the class must agree (NaN / inf of the same sign).  A result at the overflow threshold of the OUTPUT
                type (|t| (1 + u_out) + e >= its largest finite value) may be that infinity: RNE of the operation's store.
                K_op = 4 x ORACLE_RATIO[op]: the oracle's own worst |oracle - t| / (2^-24 S_op) over these tables (glibc, measured and held in
                tests/test_meltw_ew_cpu.py); the device's libm is another implementation of the same functions with OpenCL-class accuracy (a few ulp for tanh /
                erf where glibc stays below two).
"""
import ctypes as C
import math

import numpy as np

from gemm_ld_helpers import GAP_CODE, NAN_CODE, _u
from helpers import NP_OF, as_float, bf16_to_f32
from libxsmm_amd import capi
from libxsmm_amd.capi import BINARY, DT, TERNARY, UNARY, UNARY_FLAG
from oracle import pyoracle

OP_UNARY, OP_BINARY, OP_TERNARY = 1, 2, 3
NONE, ROW, COL, SCALAR = 0, 1, 2, 3
KINDS = (NONE, ROW, COL, SCALAR)
FLT_MIN, FLT_MAX = 2.0 ** -126, float(np.finfo(np.float32).max)
FP8 = (DT.BF8, DT.HF8)

EXACT_UNARY = [UNARY.IDENTITY, UNARY.XOR, UNARY.X2, UNARY.NEGATE, UNARY.INC, UNARY.RELU, UNARY.SQRT, UNARY.RECIPROCAL, UNARY.RECIPROCAL_SQRT, UNARY.LEAKY_RELU]
APPROX_UNARY = [UNARY.TANH, UNARY.SIGMOID, UNARY.GELU, UNARY.EXP, UNARY.TANH_INV, UNARY.SIGMOID_INV, UNARY.GELU_INV, UNARY.ELU]
ALPHA = 0.3            # LEAKY_RELU / ELU

# the oracle's worst (|oracle - t| - FLT_MIN)+ / (2^-24 S_op), f32 results, over all_bf16() fed as f32 TOGETHER WITH f32_wide (glibc on x86-64; measured and held by
# tests/test_meltw_ew_cpu.py).  Over all_bf16() alone: TANH 2.23, SIGMOID 1.29, EXP 1.00, GELU 1.84, GELU_INV 2.00, TANH_INV 1.44, SIGMOID_INV 0.85, ELU 1.82 -- the
# 24-bit mantissas of f32_wide land closer to the rounding ties of tanhf than 8-bit ones do.
ORACLE_RATIO = {UNARY.TANH: 2.41, UNARY.SIGMOID: 1.45, UNARY.EXP: 1.00, UNARY.GELU: 1.87, UNARY.GELU_INV: 2.00, UNARY.TANH_INV: 1.90, UNARY.SIGMOID_INV: 1.04,
                UNARY.ELU: 1.83}
K_OP = {op: 4.0 * r for op, r in ORACLE_RATIO.items()}


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------------------
def all_bf16():
    return np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)


def all_f16():
    return np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)


def all_fp8(dt):
    assert dt in FP8
    return np.arange(256, dtype=np.uint16).astype(np.uint8)


def f32_on_bf16_boundaries():
    """Every upper half x the lower halves around the tie: 0x7f7f8000 (rounds to inf), every NaN shape, denormals (flushed first by the reference)."""
    up = np.arange(1 << 16, dtype=np.uint32) << 16
    lo = np.array([0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff], dtype=np.uint32)
    return (up[None, :] | lo[:, None]).reshape(-1).view(np.float32)


_F32_SPECIALS = [0.0, 1e-45, FLT_MIN, 20.0, 87.3, 88.72, 88.73, 103.9, 104.1, FLT_MAX, np.inf]


def f32_wide(rng, count):
    """count f32 values: the specials first (both signs, NaN, a signalling NaN), a linear sweep of [-12, 12], the rest normal * 2^[-20, 8]."""
    sp = np.array(_F32_SPECIALS, dtype=np.float64)
    head = np.concatenate([sp, -sp, [np.nan]]).astype(np.float32)
    head = np.concatenate([head, np.array([0x7f800001, 0xffc00000], dtype=np.uint32).view(np.float32)])
    sweep = np.linspace(-12.0, 12.0, max((count - head.size) // 2, 2)).astype(np.float32)
    rest = count - head.size - sweep.size
    assert rest > 0
    rnd = (rng.standard_normal(rest) * 2.0 ** rng.integers(-20, 9, rest)).astype(np.float32)
    return np.concatenate([head, sweep, rnd])


def f64_wide(rng, count):
    sp = np.array([0.0, 5e-324, 2.2250738585072014e-308, 1e-310, 1.0, 0.25, 3.0, 1e300, 1.7976931348623157e308, np.inf])
    head = np.concatenate([sp, -sp, [np.nan]])
    return np.concatenate([head, rng.standard_normal(count - head.size) * 2.0 ** rng.integers(-40, 41, count - head.size)])


def encode(x, dt):
    """float values -> the storage type by ONE round-to-nearest-even (bf16 without the reference's denormal flush: table construction only)."""
    if dt == DT.F64:
        return np.asarray(x, dtype=np.float64)
    x32 = np.asarray(x, dtype=np.float32)
    if dt == DT.F32:
        return x32
    if dt == DT.BF16:
        u = x32.view(np.uint32).astype(np.uint64)
        r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
        return np.where(np.isnan(x32), np.uint16(0x7fc0), r).astype(np.uint16)
    if dt == DT.F16:
        with np.errstate(over="ignore"):
            return x32.astype(np.float16).view(np.uint16)
    raise ValueError(dt)


def decode(x, dt):
    with np.errstate(invalid="ignore"):                 # a signalling NaN widened to float64
        return np.asarray(x, dtype=np.float64) if dt in (DT.F32, DT.F64) else as_float(x, dt)


def f32_on_narrow_boundaries(dt):
    """f32 inputs of a narrowing store to F16 / E5M2 / E4M3: every finite value of the type, every midpoint between two neighbours (an exact tie in f32), the f32
    neighbours of each midpoint, and what lies past the largest value; +-0, inf, NaN, f32 denormals."""
    codes = all_f16() if dt == DT.F16 else all_fp8(dt)
    v = decode(codes, dt)
    v = np.unique(v[np.isfinite(v)])
    mid = ((v[:-1] + v[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (v[:-1] + v[1:]) / 2)
    top = np.float32(v[-1])
    past = np.array([top * np.float32(1.0 + 2.0 ** -12), top * np.float32(1.03), top * np.float32(1.0625), top * np.float32(1.07), top * 2, top * 4], dtype=np.float32)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-39, FLT_MIN, FLT_MAX, -FLT_MAX], dtype=np.float32)
    with np.errstate(over="ignore"):
        return np.concatenate([v.astype(np.float32), mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)), past, -past, sp]).astype(np.float32)


def interesting(dt, count, seed=7):
    """count values of the type: zeros, denormals, the smallest and largest normal, the expf thresholds, inf, NaN (quiet, signalling, negative), then random ones."""
    rng = np.random.default_rng(seed)
    if dt == DT.F64:
        sp = np.array([0.0, 5e-324, 2.2250738585072014e-308, 1.0, 3.0, 1e200, 1.7976931348623157e308, np.inf])
        head = np.concatenate([sp, -sp, [np.nan, -np.nan]])
        head = np.concatenate([head, np.array([0x7ff0000000000001], dtype=np.uint64).view(np.float64)])
        if count < 30:
            head = head[[0, 8, 1, 2, 3, 11, 6, 14, 7, 15, 16, 18]]
        rest = rng.standard_normal(count - head.size) * 2.0 ** rng.integers(-30, 31, count - head.size)
        return np.concatenate([head, rest])
    sp = np.array([0.0, 1e-45, FLT_MIN, 1.0, 3.0, 20.0, 88.72, 1e19, 2e19, FLT_MAX, np.inf], dtype=np.float64)
    head = np.concatenate([sp, -sp]).astype(np.float32)
    if dt == DT.F32:
        head = np.concatenate([head, np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7fa55555, 0x00400000, 0x807fffff], dtype=np.uint32).view(np.float32)])
        if count < 64:
            head = head[[0, 11, 1, 2, 3, 14, 8, 9, 20, 10, 21, 22, 24, 26]]
        rest = (rng.standard_normal(count - head.size) * 2.0 ** rng.integers(-20, 9, count - head.size)).astype(np.float32)
        return np.concatenate([head, rest])
    assert dt == DT.BF16
    head = encode(head, DT.BF16)         # FLT_MAX -> inf, 1e-45 -> 0: replaced by the type's own edge codes below
    head = np.concatenate([head, np.array([0x0001, 0x8001, 0x007f, 0x0080, 0x7f7f, 0xff7f, 0x7fc0, 0xffc0, 0x7f81, 0x7fa5], dtype=np.uint16)])
    if count < 64:
        head = head[[0, 11, 2, 3, 14, 8, 19, 10, 21, 22, 24, 26, 28, 30]]
    rest = encode((rng.standard_normal(count - head.size) * 2.0 ** rng.integers(-20, 9, count - head.size)).astype(np.float32), DT.BF16)
    return np.concatenate([head, rest])


def pair_grid(dt, count=256):
    """(in0, in1) as [n = count][m = count] logical matrices: in0(i, j) = v[i], in1(i, j) = v[j]."""
    v = interesting(dt, count)
    return np.ascontiguousarray(np.broadcast_to(v[None, :], (count, count))), np.ascontiguousarray(np.broadcast_to(v[:, None], (count, count)))


def triple_grid(dt, count=40):
    """(in0, in1, in2) as [n = count^2][m = count]: v[i], v[j % count], v[j // count]."""
    v = interesting(dt, count)
    j = np.arange(count * count)
    shape = (count * count, count)
    return (np.ascontiguousarray(np.broadcast_to(v[None, :], shape)), np.ascontiguousarray(np.broadcast_to(v[j % count][:, None], shape)),
            np.ascontiguousarray(np.broadcast_to(v[j // count][:, None], shape)))


# ---- layout and poison ----------------------------------------------------------------------------------------------------------------------------------
def extent(kind, m, n, ld):
    """elements an operand of this kind spans: what run_meltw's extent() stages for host memory (csrc/runtime.cpp)."""
    return {NONE: ld * (n - 1) + m, ROW: ld * (n - 1) + 1, COL: m, SCALAR: 1}[kind]


def layout_index(kind, m, n, ld):
    """[n][m] element index the operation reads for (i, j) [oracle_meltw.c: elem_index]."""
    i, j = np.arange(m)[None, :], np.arange(n)[:, None]
    return {NONE: j * ld + i, ROW: j * ld + 0 * i, COL: i + 0 * j, SCALAR: 0 * i + 0 * j}[kind]


def layout(kind, m, n, ld, elems=None):
    """boolean mask over `elems` elements (default: the extent): the elements an operand of this broadcast kind owns."""
    mask = np.zeros(extent(kind, m, n, ld) if elems is None else elems, dtype=bool)
    mask[layout_index(kind, m, n, ld).ravel()] = True
    return mask


def nan_of(dt):
    return np.nan if dt in (DT.F32, DT.F64) else NAN_CODE[dt]


def gap_of(dt):
    return -7.0 if dt in (DT.F32, DT.F64) else GAP_CODE[dt]


def poison_inputs(buf, mask, dt):
    """in place: NaN everywhere outside the mask (padding rows, tails, the elements in front of an offset pointer)."""
    buf[~mask] = nan_of(dt)
    return buf


# ---- comparisons ----------------------------------------------------------------------------------------------------------------------------------------
_QUIET = {DT.F64: 1 << 51, DT.F32: 1 << 22, DT.BF16: 1 << 6, DT.F16: 1 << 9, DT.BF8: 1 << 1, DT.HF8: 0}
_UINT = {8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}


def bits_of(x):
    x = np.ascontiguousarray(x)
    return x.view(_UINT[x.itemsize])


def same_bits(ref, got, dt):
    """boolean array: equal bit patterns, or NaN on both sides with the reference's quiet bit."""
    rb, gb = bits_of(ref), bits_of(got)
    rn, gn = np.isnan(decode(ref, dt)), np.isnan(decode(got, dt))
    q = rb.dtype.type(_QUIET[dt])
    return (rb == gb) | (rn & gn & ((rb & q) == (gb & q)))


def assert_exact(ref_buf, got_buf, mask, dt, pure=False, what=""):
    """ref_buf / got_buf: the oracle's and the device's whole output allocation; mask: its logical elements."""
    assert ref_buf.shape == got_buf.shape == mask.shape
    out_r, out_g = bits_of(ref_buf)[~mask], bits_of(got_buf)[~mask]
    assert np.array_equal(out_r, out_g), f"{what}: {np.count_nonzero(out_r != out_g)} elements outside the logical output differ from the reference's buffer"
    r, g = ref_buf[mask], got_buf[mask]
    ok = (bits_of(r) == bits_of(g)) if pure else same_bits(r, g, dt)
    if not ok.all():
        k = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(~ok)} of {ok.size} logical elements differ; first at logical element {k}: "
                             f"ref 0x{int(bits_of(r)[k]):x} ({decode(r[k:k + 1], dt)[0]!r}) got 0x{int(bits_of(g)[k]):x} ({decode(g[k:k + 1], dt)[0]!r})")


def u_out(dt):
    """unit round-off of an output type (the 8-bit floats are rounded through a half first [ref: src/libxsmm_math.c], so both round-offs)."""
    return {DT.BF8: 2.0 ** -3 + 2.0 ** -11, DT.HF8: 2.0 ** -4 + 2.0 ** -11}.get(dt) or _u(dt)


def max_of(dt):
    return {DT.F32: FLT_MAX, DT.BF16: float(bf16_to_f32(np.array([0x7f7f], dtype=np.uint16))[0]), DT.F16: 65504.0, DT.BF8: 57344.0, DT.HF8: 448.0}[dt]


_erf = np.vectorize(math.erf, otypes=[np.float64])


def restate64(op, x, alpha=ALPHA):
    """(t, S): float64 value of the reference's f32 formula and the sum of the magnitudes that formula adds."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        if op == UNARY.TANH:
            t = np.tanh(x); return t, np.abs(t)
        if op in (UNARY.SIGMOID, UNARY.SIGMOID_INV):
            th = np.tanh(x / 2); s = (th + 1) / 2; S = (np.abs(th) + 1) / 2
            return (s, S) if op == UNARY.SIGMOID else (s * (1 - s), S)
        if op == UNARY.EXP:
            t = np.exp(x); return t, t
        e = _erf(x / math.sqrt(2.0))
        if op == UNARY.GELU:
            return (e + 1) * 0.5 * x, (np.abs(e) + 1) * 0.5 * np.abs(x)
        if op == UNARY.GELU_INV:
            tail = x / math.sqrt(2 * math.pi) * np.exp(-0.5 * x * x)
            return 0.5 + 0.5 * e + tail, 0.5 + 0.5 * np.abs(e) + np.abs(tail)
        if op == UNARY.TANH_INV:
            th = np.tanh(x); return 1 - th * th, 1 + th * th
        if op == UNARY.ELU:
            ex = np.exp(x)
            return np.where(x <= 0, alpha * (ex - 1), x), np.where(x <= 0, abs(alpha) * (ex + 1), 0.0)
    raise ValueError(op)


def approx_ratio(op, x, got, out_dt, alpha=ALPHA):
    """(ratio, class_ok) per element: (|got - t| - u_out |t| - FLT_MIN)+ / (2^-24 S_op), and whether a non-finite / overflowing t met its class."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(got, dtype=np.float64)
    t, S = restate64(op, x, alpha)
    u, top = u_out(out_dt), max_of(out_dt)
    with np.errstate(all="ignore"):
        cls = ~np.isfinite(t) | (np.abs(t) > FLT_MAX)
        tc = np.where(np.abs(t) > FLT_MAX, np.sign(t) * np.inf, t)
        class_ok = np.where(np.isnan(tc), np.isnan(g), g == tc)
        e = 2.0 ** -24 * S
        may_inf = ~cls & (np.abs(t) * (1 + u) + e >= top) & np.isinf(g) & (np.sign(g) == np.sign(t))
        excess = np.maximum(np.abs(g - t) - u * np.abs(t) - FLT_MIN, 0.0)
        ratio = np.where(excess == 0, 0.0, excess / e)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)            # NaN where t is a number
        ratio = np.where(cls | may_inf, 0.0, ratio)
    return ratio, np.where(cls, class_ok, True)


def oracle_ratio(op, x, got, alpha=ALPHA):
    """worst (|got - t| - FLT_MIN)+ / (2^-24 S_op) over the elements with a finite t: how K_op is measured on the oracle's f32 results (the round-off of the
    output is NOT taken off here: it is part of what the oracle's libm and store do, so K_op carries it once more)."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(got, dtype=np.float64)
    t, S = restate64(op, x, alpha)
    with np.errstate(all="ignore"):
        fin = np.isfinite(t) & (np.abs(t) <= FLT_MAX) & np.isfinite(g)
        excess = np.maximum(np.abs(g - t) - FLT_MIN, 0.0)
        raw = np.where(fin, np.where(excess == 0, 0.0, excess / (2.0 ** -24 * S)), 0.0)
    return float(np.max(raw))


def assert_approx(op, x, got, out_dt, alpha=ALPHA, what="", stats=None, k=None):
    """x: the inputs as float64, got: the device's results decoded to float64, both over the logical elements only.  No element is skipped."""
    ratio, class_ok = approx_ratio(op, x, got, out_dt, alpha)
    ratio, class_ok = ratio.ravel(), class_ok.ravel()
    k = K_OP[op] if k is None else k
    if stats is not None:
        stats["ratio"] = max(stats.get("ratio", 0.0), float(ratio.max()))
    x, got = np.asarray(x, dtype=np.float64).ravel(), np.asarray(got, dtype=np.float64).ravel()
    bad = ~class_ok.ravel()
    if bad.any():
        e = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {bad.sum()} elements of the wrong class; first: element {e}, x = {x[e]!r}, t = {restate64(op, x[e:e + 1], alpha)[0][0]!r}, got {got[e]!r}")
    if ratio.max() > k:
        e = int(np.argmax(ratio))
        raise AssertionError(f"{what}: {np.count_nonzero(ratio > k)} elements outside K = {k}; worst: element {e}, x = {x[e]!r}, t = {restate64(op, x[e:e + 1], alpha)[0][0]!r}, "
                             f"got {got[e]!r}, err / (2^-24 S) = {float(ratio[e]):.2f}")


# ---- which kernel ---------------------------------------------------------------------------------------------------------------------------------------
def ran(handle, batched):
    return capi.load().hip_kernel_name(handle, 1 if batched else 0).decode()


_EW8_UNARY = {UNARY.IDENTITY, UNARY.XOR, UNARY.X2, UNARY.SQRT, UNARY.TANH, UNARY.TANH_INV, UNARY.SIGMOID, UNARY.SIGMOID_INV, UNARY.GELU, UNARY.GELU_INV, UNARY.NEGATE,
              UNARY.INC, UNARY.RECIPROCAL, UNARY.RECIPROCAL_SQRT, UNARY.EXP}
_EW8_UNARY_NOMASK = {UNARY.RELU, UNARY.LEAKY_RELU, UNARY.ELU}
_EW8_BINARY = {BINARY.ADD, BINARY.SUB, BINARY.MUL, BINARY.DIV, BINARY.MULADD, BINARY.MAX, BINARY.MIN}
_VEC4_NOT = {UNARY.REPLICATE_COL_VAR, UNARY.RELU_INV, UNARY.LEAKY_RELU_INV, UNARY.ELU_INV, UNARY.UNZIP, UNARY.DUMP}
_F = (DT.F32, DT.BF16)


def expected_kernel(op, typ, in_dts, out_dt, m, n, in_lds, ldo, kinds, in_ptrs, out_ptr, in_strides, out_stride, bitmask=False):
    """The name launch_meltw reports for a plain element-wise TPP: ew8_ok, then (unary) the vec4 condition, then the general kernel of the operation.
    in_ptrs / out_ptr: addresses (only their residue mod 16 matters); in_strides / out_stride: batch strides in bytes (0 for a single call)."""
    nin = len(in_dts)
    assert nin == op
    g = 4 if out_dt == DT.F32 and all(t == DT.F32 for t in in_dts) else 8
    ok = m % g == 0 and ldo % g == 0 and out_dt in _F and out_ptr % 16 == 0 and out_stride % 16 == 0
    for o in range(nin):
        ok = ok and in_dts[o] in _F
        if kinds[o] == NONE:
            ok = ok and in_lds[o] % g == 0
        if kinds[o] in (NONE, COL):
            ok = ok and in_ptrs[o] % 16 == 0 and in_strides[o] % 16 == 0
    if op == OP_UNARY:
        ok = ok and (typ in _EW8_UNARY or (typ in _EW8_UNARY_NOMASK and not bitmask))
    elif op == OP_BINARY:
        ok = ok and typ in _EW8_BINARY
    else:
        ok = ok and typ in (TERNARY.MULADD, TERNARY.NMULADD)
    if ok:
        return "meltw_ew8_kernel"
    if op == OP_BINARY:
        return "meltw_binary_kernel"
    if op == OP_TERNARY:
        return "meltw_ternary_kernel"
    simple = kinds[0] == NONE and in_dts[0] == out_dt and out_dt in _F and m % 4 == 0 and in_lds[0] % 4 == 0 and ldo % 4 == 0 and not bitmask and typ not in _VEC4_NOT
    esz = 4 if in_dts[0] == DT.F32 else 2
    aligned = all(v % (4 * esz) == 0 for v in (in_ptrs[0], out_ptr, in_strides[0], out_stride))
    return "meltw_unary_vec4_kernel" if simple and aligned else "meltw_unary_kernel"


# ---- one call -------------------------------------------------------------------------------------------------------------------------------------------
def _round_up(x, q):
    return (x + q - 1) // q * q


class Operand:
    """One operand's whole allocation: `off` poisoned elements in front of the pointer, `batch` blocks of `per` elements (the extent plus a tail)."""

    def __init__(self, dt, kind, m, n, ld, batch, off, odd_stride, fill, tail=5, bits=False):
        self.dt, self.kind, self.ld, self.batch, self.off, self.bits = dt, kind, ld, batch, off, bits
        self.size = 1 if bits else capi.DT_SIZE[dt]
        if bits:                                        # a bit matrix: ld rounded up to 16, one bit per element [oracle_meltw.c: bit_put / bit_get]
            self.ld_bits = _round_up(ld, 16)
            ext = (self.ld_bits // 8) * n
            one = np.zeros(ext, dtype=bool)
        else:
            ext = extent(kind, m, n, ld)
            one = None
        per = _round_up((ext + tail) * self.size, 16) // self.size
        if odd_stride:
            per += 1
            assert (per * self.size) % 16 != 0
        self.per = per
        self.idx = None if bits else layout_index(kind, m, n, ld)
        total = off + batch * per
        self.mask = np.zeros(total, dtype=bool)
        if not bits:
            one = layout(kind, m, n, ld, per)
            for b in range(batch):
                self.mask[off + b * per: off + (b + 1) * per] = one
        self.buf = np.full(total, fill, dtype=np.uint8 if bits else NP_OF[dt])
        self.m, self.n = m, n

    @property
    def stride(self):
        return self.per * self.size

    def put(self, values):
        """values: [batch][n][m] logical values in the storage type; a broadcast operand takes what its kind reads (column 0 / row 0 / element 0)."""
        v = np.asarray(values).reshape(self.batch, self.n, self.m)
        for b in range(self.batch):
            blk = self.buf[self.off + b * self.per: self.off + (b + 1) * self.per]
            if self.kind == NONE:
                blk[self.idx] = v[b]
            elif self.kind == ROW:
                blk[self.idx[:, 0]] = v[b, :, 0]
            elif self.kind == COL:
                blk[self.idx[0, :]] = v[b, 0, :]
            else:
                blk[0] = v[b, 0, 0]

    def logical(self, buf=None):
        """[batch][n][m] gather of what the operation reads / wrote."""
        buf = self.buf if buf is None else buf
        return np.stack([buf[self.off + b * self.per: self.off + (b + 1) * self.per][self.idx] for b in range(self.batch)])

    def logical_bits(self, buf):
        out = []
        for b in range(self.batch):
            blk = buf[self.off + b * self.per: self.off + b * self.per + (self.ld_bits // 8) * self.n]
            out.append(np.unpackbits(blk.reshape(self.n, -1), axis=1, bitorder="little")[:, :self.m])
        return np.stack(out)


def bcast_flags(op, kinds):
    f = 0
    for o, k in enumerate(kinds):
        if k == NONE:
            continue
        if op == OP_UNARY:
            f |= {ROW: UNARY_FLAG.BCAST_ROW, COL: UNARY_FLAG.BCAST_COL, SCALAR: UNARY_FLAG.BCAST_SCALAR}[k]
        elif op == OP_BINARY:
            f |= {ROW: 1, COL: 4, SCALAR: 16}[k] << o
        else:
            f |= {ROW: 1, COL: 8, SCALAR: 64}[k] << o
    return f


def _upload(x):
    import torch
    v = {np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}.get(x.dtype.type)
    return torch.from_numpy(np.ascontiguousarray(x.view(v) if v else x)).to("cuda:0")


class EwCase:
    """One element-wise TPP over padded, poisoned operands.

    op, typ            OP_UNARY / OP_BINARY / OP_TERNARY and the operation
    in_dts, out_dt     storage types (SELECT: two inputs, the third operand is its bit mask)
    values             per input the [batch][n][m] logical values in the storage type
    lds                leading dimensions of the inputs, then of the output
    kinds              broadcast kind per input
    off_bytes          every pointer is moved this many bytes into its allocation (0: 256-byte aligned allocations as torch hands them out)
    odd_stride         batch strides that are a multiple of the element size but not of 16 bytes
    prev               [batch][n][m] start values of the output (MULADD reads them); default: the sentinel
    inplace            None, or the input index the output aliases
    out_bits           the result is a bit matrix (CMP_OP_*)"""

    def __init__(self, op, typ, in_dts, out_dt, m, n, values, lds, kinds=None, batch=1, off_bytes=0, odd_stride=False, prev=None, inplace=None, out_bits=False,
                 alpha=None, select_bits=None):
        self.op, self.typ, self.in_dts, self.out_dt, self.m, self.n, self.batch = op, typ, tuple(in_dts), out_dt, m, n, batch
        self.select = op == OP_TERNARY and typ == TERNARY.SELECT
        nin = len(self.in_dts)
        self.kinds = tuple(kinds) if kinds is not None else (NONE,) * nin
        self.lds, self.out_bits, self.inplace, self.alpha = tuple(lds), out_bits, inplace, alpha
        self.flags = bcast_flags(op, self.kinds)
        self.ins = []
        for o in range(nin):
            sz = capi.DT_SIZE[self.in_dts[o]]
            assert off_bytes % sz == 0
            opd = Operand(self.in_dts[o], self.kinds[o], m, n, self.lds[o], batch, off_bytes // sz, odd_stride, nan_of(self.in_dts[o]))
            opd.put(values[o])
            self.ins.append(opd)
        if self.select:
            self.sel = Operand(DT.U8, NONE, m, n, self.lds[2], batch, off_bytes, odd_stride, 0, bits=True)
            self.sel.buf[:] = select_bits[: self.sel.buf.size]
        ldo = self.lds[-1]
        if inplace is not None:
            self.out = self.ins[inplace]
            assert self.kinds[inplace] == NONE and self.in_dts[inplace] == out_dt and self.lds[inplace] == ldo
        elif out_bits:
            self.out = Operand(DT.U8, NONE, m, n, ldo, batch, off_bytes, odd_stride, 0xa5, bits=True)
        else:
            sz = capi.DT_SIZE[out_dt]
            self.out = Operand(out_dt, NONE, m, n, ldo, batch, off_bytes // sz, odd_stride, gap_of(out_dt))
            if prev is not None:
                self.out.put(prev)

    # -- descriptors
    def comp(self):
        return DT.F64 if self.in_dts[0] == DT.F64 else DT.F32

    def oracle_desc(self):
        t = list(self.in_dts) + [DT.UNSUPPORTED] * (3 - len(self.in_dts))
        l = list(self.lds[:-1]) + [0] * (3 - len(self.in_dts))
        if self.select:
            t[2], l[2] = DT.IMPLICIT, self.lds[2]
        return pyoracle.MeltwDesc(self.m, self.n, l[0], self.lds[-1], l[1], l[2], t[0], t[1], t[2], self.comp(), self.out_dt, self.flags, self.typ, self.op)

    def shape(self):
        d, l, m, n = self.in_dts, self.lds, self.m, self.n
        if self.op == OP_UNARY:
            return capi.UnaryShape(m, n, l[0], l[1], d[0], self.out_dt, self.comp())
        if self.op == OP_BINARY:
            return capi.BinaryShape(m, n, l[0], l[1], l[2], d[0], d[1], self.out_dt, self.comp())
        return capi.TernaryShape(m, n, l[0], l[1], l[2], l[3], d[0], d[1], d[0] if self.select else d[2], self.out_dt, self.comp())

    def dispatch(self, api):
        fn = {OP_UNARY: api.dispatch_meltw_unary, OP_BINARY: api.dispatch_meltw_binary, OP_TERNARY: api.dispatch_meltw_ternary}[self.op]
        return fn(self.typ, self.shape(), self.flags)

    def _param(self, in_ptrs, out_ptr, sel_ptr, b, keep):
        p = {OP_UNARY: capi.UnaryParam, OP_BINARY: capi.BinaryParam, OP_TERNARY: capi.TernaryParam}[self.op]()
        names = {OP_UNARY: ("in_",), OP_BINARY: ("in0", "in1"), OP_TERNARY: ("in0", "in1", "in2")}[self.op]
        for o, opd in enumerate(self.ins):
            getattr(p, names[o]).primary = in_ptrs[o] + opd.off * opd.size + b * opd.stride
        if self.select:
            p.in2.primary = sel_ptr + self.sel.off + b * self.sel.stride
        p.out.primary = out_ptr + self.out.off * self.out.size + b * self.out.stride
        if self.alpha is not None:
            a = C.c_float(self.alpha); keep.append(a); p.op.primary = C.addressof(a)
        return p

    def run_oracle(self):
        """The oracle's whole output allocation (the case's own buffers stay as they are, in-place rows included)."""
        orc = pyoracle.oracle()
        ins = [o.buf.copy() for o in self.ins]
        out = ins[self.inplace] if self.inplace is not None else self.out.buf.copy()
        keep = []
        for b in range(self.batch):
            orc.meltw(self._param([x.ctypes.data for x in ins], out.ctypes.data, self.sel.buf.ctypes.data if self.select else 0, b, keep), self.oracle_desc())
        return out

    def run_reference(self):
        ref = pyoracle.reference()
        ins = [o.buf.copy() for o in self.ins]
        out = ins[self.inplace] if self.inplace is not None else self.out.buf.copy()
        keep = []
        fn = {OP_UNARY: ref.lib.xref_reference_meltw_unary, OP_BINARY: ref.lib.xref_reference_meltw_binary, OP_TERNARY: ref.lib.xref_reference_meltw_ternary}[self.op]
        for b in range(self.batch):
            p = self._param([x.ctypes.data for x in ins], out.ctypes.data, self.sel.buf.ctypes.data if self.select else 0, b, keep)
            fn(C.byref(p), self.typ, self.shape(), self.flags)
        return out

    def expected(self, ptrs=None):
        """The kernel name for 256-byte aligned allocations (ptrs: the actual base addresses, when a test knows them)."""
        batched = self.batch > 1
        bases = ptrs if ptrs is not None else [0] * (len(self.ins) + 1)
        in_ptrs = [bases[o] + opd.off * opd.size for o, opd in enumerate(self.ins)]
        out_ptr = bases[-1] + self.out.off * self.out.size
        if self.select:
            return "meltw_ternary_kernel"
        return expected_kernel(self.op, self.typ, self.in_dts, self.out_dt, self.m, self.n, self.lds[:-1], self.lds[-1],
                               self.kinds, in_ptrs, out_ptr, [opd.stride if batched else 0 for opd in self.ins], self.out.stride if batched else 0)

    def run_gpu(self, host=(), hint=None):
        """(whole output allocation, handle, kernel name).  host: input indices handed over as plain host memory (single synchronous calls only)."""
        api = capi.load()
        h = self.dispatch(api)
        assert h, "dispatch returned NULL"
        dev = [None if o in host else _upload(opd.buf) for o, opd in enumerate(self.ins)]
        hostbufs = {o: self.ins[o].buf.copy() for o in host}
        d_out = dev[self.inplace] if self.inplace is not None else _upload(self.out.buf)
        d_sel = _upload(self.sel.buf) if self.select else None
        keep = []
        in_ptrs = [hostbufs[o].ctypes.data if o in host else dev[o].data_ptr() for o in range(len(self.ins))]
        p = self._param(in_ptrs, d_out.data_ptr(), d_sel.data_ptr() if d_sel is not None else 0, 0, keep)
        old = api.hip_get_streaming_hint()
        try:
            if hint is not None:
                api.hip_set_streaming_hint(hint)
            if self.batch == 1:
                capi.Api.call(h, p)
            elif self.op == OP_UNARY:
                api.hip_meltw_unary_batch_strided(h, C.byref(p), self.batch, self.ins[0].stride, self.out.stride, 0)
            elif self.op == OP_BINARY:
                api.hip_meltw_binary_batch_strided(h, C.byref(p), self.batch, self.ins[0].stride, self.ins[1].stride, self.out.stride)
            else:
                api.hip_meltw_ternary_batch_strided(h, C.byref(p), self.batch, self.ins[0].stride, self.ins[1].stride, self.ins[2].stride if not self.select else self.sel.stride,
                                                    self.out.stride)
            api.hip_sync(); api.check()
        finally:
            if hint is not None:
                api.hip_set_streaming_hint(old)
        got = d_out.cpu().numpy().view(self.out.buf.dtype)
        for o, opd in enumerate(self.ins):                     # an input the operation does not alias comes back untouched
            if o != self.inplace and o not in host:
                assert np.array_equal(bits_of(dev[o].cpu().numpy().view(opd.buf.dtype)), bits_of(opd.buf)), f"input {o} was written"
        return got, h, ran(h, self.batch > 1)

    # -- checks
    def x64(self, o=0):
        """[batch][n][m] float64 values operand o contributes to each element."""
        x = decode(self.ins[o].logical(), self.in_dts[o])
        if self.in_dts[o] == DT.BF16:                   # the reference loads a bf16 denormal as a signed zero [ref: src/libxsmm_math.c:587-597]
            x = np.where(np.abs(x) < FLT_MIN, np.copysign(0.0, x), x)
        return x

    def check_exact(self, ref, got, pure=False, what=""):
        if self.out_bits:
            assert np.array_equal(self.out.logical_bits(ref), self.out.logical_bits(got)), f"{what}: logical bits differ"
            assert np.array_equal(ref, got), f"{what}: bytes of the bit matrix outside the logical bits differ"
            return
        assert_exact(ref, got, self.out.mask, self.out_dt, pure=pure, what=what)

    def check_approx(self, ref, got, what="", stats=None, k=None):
        """per-element bound inside, array_equal outside."""
        out_r, out_g = bits_of(ref)[~self.out.mask], bits_of(got)[~self.out.mask]
        assert np.array_equal(out_r, out_g), f"{what}: {np.count_nonzero(out_r != out_g)} elements outside the logical output differ from the reference's buffer"
        assert_approx(self.typ, self.x64(0), decode(self.out.logical(got), self.out_dt), self.out_dt, alpha=self.alpha if self.alpha is not None else ALPHA, what=what,
                      stats=stats, k=k)
