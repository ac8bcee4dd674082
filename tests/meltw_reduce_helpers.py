"""Parity of the f32 / bf16 reduction TPPs (REDUCE_X_OP_ADD / X2_OP_ADD / X_X2_OP_ADD / MAX / MIN / ABSMAX over rows or columns, the listed-column forms) over the
whole input range, at padded leading dimensions, with poisoned gaps, PER OUTPUT -- what tests/meltw_ew_helpers.py does for the element-wise TPPs.

  exact          the reference's loop [ref: src/generator_mateltwise_reference_impl.c:1296-1430] in float64 over the inputs as the oracle loads them (a bf16
                 denormal is a signed zero): per output the sum of x and of x^2 (exact to 2^-53 relative: every term is an f32 value), sum |x| and sum x^2 as the
                 scales of the bound, and MAX / MIN / ABSMAX folded with the reference's own macros: over rows the accumulator starts at the column's first
                 element and is the first operand, over columns it starts at -FLT_MAX / FLT_MAX / 0 and is the second; ABS(a) = 0 <= a ? a : -a.
  data           wide: normal * 2^[-20, 8], both signs, +-0, denormals, outputs made of two large opposite values and dust; infinite: wide plus lines (the elements
                 that fold into one output) that are all -inf, all +inf, hold one of them, both (sums: NaN) or a NaN (sums only).
  poison         everything outside the m x n block -- padding rows, the tail of the allocation, the elements in front of the pointer -- holds +inf for MAX / ABSMAX,
                 -inf for MIN and NaN for the sums (E4M3 has no infinity: +-448, which its data stay below): one read of it changes a result.  Outputs hold -7
                 outside the results.
  checks         sums            |got - exact| <= (k + 1) 2^-24 S + k FLT_MIN + r(exact): k terms (a start value is one more), S = sum |x| (sum x^2 for the squares),
                                 r = the round-off of the output type.  (k - 1) 2^-24 S bounds an f32 sum of k terms in ANY order (to first order; the second-order
                                 term is below 2^-24 S for k < 2^12), one more 2^-24 S the rounding of the squares, the last one the slack for that first-order step.
                                 k FLT_MIN: a flushed denormal per term, as meltw_ew_helpers grants.  A non-finite exact sum: the class must agree.
                 serial sums     same bits as the oracle (the paths that add in the reference's order).
                 extrema         equal in value to exact over rows (either zero of a +-0 tie), the same bits over columns.  Extremum data hold no NaN.
                 untouched       every output element outside the results still holds what it held.
  expected_reduce_kernel  restates the conditions of csrc/meltw_kernels.hip: launch_meltw and of csrc/runtime.cpp (the workspace of the two-pass form).
"""
import ctypes as C

import numpy as np

from helpers import NP_OF
from meltw_ew_helpers import FLT_MAX, FLT_MIN, bits_of, decode, encode, gap_of, max_of, nan_of, same_bits, u_out
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, UNARY, UNARY_FLAG
from oracle import pyoracle

ADD_T = (UNARY.REDUCE_X_OP_ADD, UNARY.REDUCE_X2_OP_ADD, UNARY.REDUCE_X_X2_OP_ADD)
CMP_T = (UNARY.REDUCE_X_OP_MAX, UNARY.REDUCE_X_OP_MIN, UNARY.REDUCE_X_OP_ABSMAX)
ALL_T = ADD_T + CMP_T
LISTED_T = (UNARY.REDUCE_COLS_IDX_OP_ADD, UNARY.REDUCE_COLS_IDX_OP_MAX, UNARY.REDUCE_COLS_IDX_OP_MIN)
FRONT = 8                       # poisoned elements in front of every input pointer (32 / 16 bytes: the pointer stays aligned for the vector kernels)
TAIL = 5                        # ... and behind the last column's padding
_TINY = {DT.F32: 2.0 ** -126, DT.BF16: 2.0 ** -126, DT.F16: 2.0 ** -14, DT.BF8: 2.0 ** -14, DT.HF8: 2.0 ** -6}


def want_x(typ):
    return typ != UNARY.REDUCE_X2_OP_ADD


def want_x2(typ):
    return typ in (UNARY.REDUCE_X2_OP_ADD, UNARY.REDUCE_X_X2_OP_ADD)


def load64(codes, dt):
    """the values the reference's loop sees: decode, and a bf16 denormal as a signed zero [ref: src/libxsmm_math.c:587-597]."""
    x = decode(codes, dt)
    return np.where(np.abs(x) < FLT_MIN, np.copysign(0.0, x), x) if dt == DT.BF16 else x


def _abs(a):                    # LIBXSMM_ABS
    return np.where(0.0 <= a, a, -a)


def fold_extremum(X, typ, rows):
    """X: [n][m] float64 (NaN-free).  The reference's fold with its macros MAX(A, B) = A < B ? B : A, MIN(A, B) = A < B ? A : B."""
    steps = [X[:, i] for i in range(X.shape[1])] if rows else [X[j, :] for j in range(X.shape[0])]
    if rows:
        acc = steps[0].copy()
        for v in steps:
            if typ == UNARY.REDUCE_X_OP_MAX:
                acc = np.where(acc < v, v, acc)
            elif typ == UNARY.REDUCE_X_OP_MIN:
                acc = np.where(acc < v, acc, v)
            else:
                a, b = _abs(acc), _abs(v)
                acc = np.where(a < b, b, a)
        return acc
    acc = np.full(X.shape[1], -FLT_MAX if typ == UNARY.REDUCE_X_OP_MAX else FLT_MAX if typ == UNARY.REDUCE_X_OP_MIN else 0.0)
    for v in steps:
        if typ == UNARY.REDUCE_X_OP_MIN:
            acc = np.where(v < acc, v, acc)
        else:
            v = _abs(v) if typ == UNARY.REDUCE_X_OP_ABSMAX else v
            acc = np.where(v < acc, acc, v)
    return acc


def exact(X, typ, rows, init=None):
    """X: [n][m] float64 as loaded.  Returns a dict per output: sum, sum2, abs (sum |x|), sq (sum x^2), k (terms), ext (extremum, CMP_T only).
    init = (x start values, x^2 start values) as loaded, or None."""
    ax = 1 if rows else 0
    with np.errstate(invalid="ignore", over="ignore"):
        r = {"sum": X.sum(axis=ax), "sum2": (X * X).sum(axis=ax), "abs": np.abs(X).sum(axis=ax), "sq": (X * X).sum(axis=ax), "k": X.shape[ax]}
        if init is not None:
            r["sum"], r["abs"] = r["sum"] + init[0], r["abs"] + np.abs(init[0])
            r["sum2"], r["sq"] = r["sum2"] + init[1], r["sq"] + np.abs(init[1])
            r["k"] += 1
    if typ in CMP_T:
        r["ext"] = fold_extremum(X, typ, rows)
    return r


def store(v, dt):
    """f32 values -> the output type as the reference's store rounds them (bf16: an f32 denormal goes to a signed zero first)."""
    v = np.asarray(v, dtype=np.float32)
    if dt == DT.BF16:
        v = np.where(np.abs(v) < np.float32(FLT_MIN), np.copysign(np.float32(0), v), v)
    return encode(v, dt)


# ---- data -------------------------------------------------------------------------------------------------------------------------------------------------
def wide(rng, n, m, in_dt, rows):
    """[n][m] f32 values (bf16 input: bf16-representable, some of them bf16 denormal codes)."""
    x = (rng.standard_normal((n, m)) * 2.0 ** rng.integers(-20, 9, (n, m))).astype(np.float32)
    pick = rng.random((n, m))
    x[pick < 0.04] = 0.0
    x[(pick >= 0.04) & (pick < 0.08)] = -0.0
    den = (pick >= 0.08) & (pick < 0.12)
    x[den] = (rng.integers(1, 1 << 23, int(den.sum())).astype(np.uint32) | (rng.integers(0, 2, int(den.sum())).astype(np.uint32) << 31)).view(np.float32)
    lines, inner = (n, m) if rows else (m, n)
    if inner >= 2:                                   # every seventh line: two large opposite values in dust -- a result near zero under a large sum |x|
        for q in range(3 % lines, lines, 7):
            line = x[q, :] if rows else x[:, q]
            line *= np.float32(2.0 ** -18)
            a, b = rng.choice(inner, 2, replace=False)
            line[a], line[b] = np.float32(700.0 + q), np.float32(-(700.0 + q))
    if in_dt == DT.BF16:
        codes = encode(x, DT.BF16)
        den = den & (np.abs(x) < 1.0)                # (not the large pairs)
        codes[den] = (rng.integers(1, 0x80, int(den.sum())) | (rng.integers(0, 2, int(den.sum())) << 15)).astype(np.uint16)
        return codes
    if in_dt == DT.F16:
        return encode(x, DT.F16)
    if in_dt in (DT.BF8, DT.HF8):                    # every finite code of the type
        codes = rng.integers(0, 256, (n, m)).astype(np.uint8)
        bad = ((codes & 0x7c) == 0x7c) if in_dt == DT.BF8 else ((codes & 0x7f) == 0x7f)
        codes[bad] &= 0x83
        if in_dt == DT.HF8:                          # +-448 is the poison of the extremum runs
            codes[(codes & 0x7f) == 0x7e] -= 1
        return codes
    assert in_dt == DT.F32
    return x


def infinite(rng, n, m, in_dt, rows, sums):
    """wide with, as far as the number of lines allows: line 0 all -inf, 1 all +inf, 2 one +inf, 3 one -inf and, for sums, 4 both infinities, 5 a NaN."""
    codes = wide(rng, n, m, in_dt, rows)
    pinf, ninf = encode(np.float32(np.inf), in_dt), encode(np.float32(-np.inf), in_dt)
    lines, inner = (n, m) if rows else (m, n)

    def line(q):
        return codes[q, :] if rows else codes[:, q]
    plan = [("all", ninf), ("all", pinf), ("one", pinf), ("one", ninf)] + ([("both", None), ("nan", None)] if sums else [])
    for q, (kind, v) in enumerate(plan[:lines]):
        q = (q * 5) % lines if lines >= 26 else q       # spread over the lanes / blocks of a large shape
        if kind == "all":
            line(q)[:] = v
        elif kind == "one":
            line(q)[int(rng.integers(0, inner))] = v
        elif kind == "both":
            if inner >= 2:
                a, b = rng.choice(inner, 2, replace=False)
                line(q)[a], line(q)[b] = pinf, ninf
        else:
            line(q)[int(rng.integers(0, inner))] = nan_of(in_dt)
    return codes


def tame(rng, n, m, in_dt):
    """the data of the older tests: multiples of 0.1 in [-0.4, 0.5]."""
    from helpers import rand_values
    return rand_values(rng, n * m, in_dt).reshape(n, m)


def poison_of(typ, dt):
    if typ in ADD_T or typ == UNARY.REDUCE_COLS_IDX_OP_ADD:
        return nan_of(dt)
    neg = typ in (UNARY.REDUCE_X_OP_MIN, UNARY.REDUCE_COLS_IDX_OP_MIN)
    if dt == DT.BF8:                                 # E5M2 infinities
        return np.uint8(0xfc if neg else 0x7c)
    if dt == DT.HF8:                                 # E4M3 has no infinity: the largest finite value, +-448, which wide() keeps out of the block
        return np.uint8(0xfe if neg else 0x7e)
    return encode(np.float32(-np.inf if neg else np.inf), dt)


# ---- which kernel -----------------------------------------------------------------------------------------------------------------------------------------
TAGS = ("general-rows", "general-cols", "vec-rows-cpg4", "vec-rows", "vec-cols-1slice", "vec-cols-16slice", "two-pass")


def expected_reduce_kernel(typ, flags, m, n, ldi, in_dt, base_offset=0, batch=1, stride_bytes=0):
    """(reported name, path tag).  base_offset: elements between a 256-byte aligned allocation and the pointer; stride_bytes: the batch stride of the input."""
    rows = bool(flags & UNARY_FLAG.REDUCE_ROWS)
    al = 8 if in_dt == DT.BF16 else 16
    sz = capi.DT_SIZE[in_dt]
    vec = in_dt in (DT.F32, DT.BF16) and m % 4 == 0 and ldi % 4 == 0 and (base_offset * sz) % al == 0 and stride_bytes % al == 0 and batch < 65536
    if not vec:
        return "reduce_kernel", "general-rows" if rows else "general-cols"
    m4 = m // 4
    G = 1
    while G < 64 and G < m4:
        G <<= 1
    gx = (m4 + 15) // 16
    nchunks = 1
    if not rows and batch == 1 and n >= 2048 and gx < 512:        # n >= 2048: only then does the runtime hand the launcher a workspace for the partial results
        nchunks = min(128, n // 64, 512 // gx)
    if rows and m4 <= G and n >= 64:
        return "reduce_vec_kernel", "vec-rows-cpg4"
    if nchunks > 1:
        return "reduce_vec_kernel+combine", "two-pass"
    if rows:
        return "reduce_vec_kernel", "vec-rows"
    return "reduce_vec_kernel", "vec-cols-16slice" if n >= 256 else "vec-cols-1slice"


def serial_order(tag):
    """the paths whose sums are the reference's chain of additions."""
    return tag in ("general-cols", "vec-cols-1slice")


# ---- one call ---------------------------------------------------------------------------------------------------------------------------------------------
def _round_up(x, q):
    return (x + q - 1) // q * q


def _upload(x):
    import torch
    v = {np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}.get(x.dtype.type)
    return torch.from_numpy(np.ascontiguousarray(x.view(v) if v else x)).to("cuda:0")


class ReduceCase:
    """One reduction TPP over `batch` padded, poisoned matrices.

    off         extra elements between the (aligned) allocation and the pointer, on top of FRONT
    odd_stride  a batch stride that is a multiple of the element size but not of 16 (f32) / 8 (bf16) bytes
    data        'wide' | 'infinite' | 'tame', or an [batch][n][m] array of codes
    ldo         default: the result size + 3 (over rows the API ignores it: the x^2 results follow the n x results)"""

    def __init__(self, typ, m, n, ldi, rows, in_dt=DT.F32, out_dt=DT.F32, init=False, batch=1, off=0, odd_stride=False, data="wide", seed=0, ldo=None):
        self.typ, self.m, self.n, self.ldi, self.rows, self.in_dt, self.out_dt, self.init, self.batch, self.off = typ, m, n, ldi, bool(rows), in_dt, out_dt, init, batch, off
        rng = np.random.default_rng(seed)
        self.res = n if rows else m
        self.ldo = self.res + 3 if ldo is None else ldo
        self.x2_at = (n if rows else self.ldo) if (want_x(typ) and want_x2(typ)) else 0
        self.flags = (UNARY_FLAG.REDUCE_ROWS if rows else UNARY_FLAG.REDUCE_COLS) | (UNARY_FLAG.REDUCE_INIT_ACC if init else 0)
        isz, osz = capi.DT_SIZE[in_dt], capi.DT_SIZE[out_dt]
        self.isz, self.osz = isz, osz
        al = 8 if in_dt == DT.BF16 else 16
        per = _round_up((ldi * n + TAIL) * isz, 16) // isz
        if odd_stride:
            per += 1
            assert (per * isz) % al != 0
        self.per = per
        self.front = FRONT + off
        is_tame = isinstance(data, str) and data == "tame"
        if isinstance(data, str):
            sums = typ in ADD_T
            gen = {"wide": lambda: wide(rng, n, m, in_dt, rows), "infinite": lambda: infinite(rng, n, m, in_dt, rows, sums), "tame": lambda: tame(rng, n, m, in_dt)}[data]
            blocks = np.stack([gen() for _ in range(batch)])
        else:
            blocks = np.asarray(data).reshape(batch, n, m)
        if is_tame:                                  # the older tests' padding: ordinary values of the same distribution
            from helpers import rand_values
            self.in_buf = rand_values(rng, self.front + batch * per, in_dt)
        else:
            self.in_buf = np.full(self.front + batch * per, poison_of(typ, in_dt), dtype=NP_OF[in_dt])
        self.idx = (np.arange(n)[:, None] * ldi + np.arange(m)[None, :])
        # outputs: -7 everywhere, start values (random, of the data's scale) in the results
        oper = _round_up((2 * max(self.ldo, self.res) + TAIL) * osz, 16) // osz
        self.oper = oper
        self.out_buf = np.full(batch * oper, gap_of(out_dt), dtype=NP_OF[out_dt])
        self.out_mask = np.zeros(batch * oper, dtype=bool)
        for b in range(batch):
            if want_x(typ):
                self.out_mask[b * oper: b * oper + self.res] = True
            if want_x2(typ):
                self.out_mask[b * oper + self.x2_at: b * oper + self.x2_at + self.res] = True
        if init:
            k = int(self.out_mask.sum())
            self.out_buf[self.out_mask] = store((rng.standard_normal(k) * 2.0 ** rng.integers(-10, 6, k)).astype(np.float32), out_dt)
        self._put(blocks)
        if isinstance(data, str) and not is_tame:
            self._scale_to_fit()

    def _put(self, blocks):
        for b in range(self.batch):
            self.in_buf[self.front + b * self.per: self.front + (b + 1) * self.per][self.idx] = blocks[b]

    def logical(self, b):
        """[n][m] float64 values of matrix b as the loop loads them."""
        return load64(self.in_buf[self.front + b * self.per: self.front + (b + 1) * self.per][self.idx], self.in_dt)

    def init_values(self, b):
        if not (self.init and self.typ in ADD_T):
            return None
        o = load64(self.out_buf[b * self.oper: (b + 1) * self.oper], self.out_dt)
        zero = np.zeros(self.res)
        return (o[:self.res] if want_x(self.typ) else zero, o[self.x2_at: self.x2_at + self.res] if want_x2(self.typ) else zero)

    def exact(self, b):
        return exact(self.logical(b), self.typ, self.rows, self.init_values(b))

    def _scale_to_fit(self):
        """halve the finite data until sum |x| and sum x^2 (start values included) of every output are below half the largest finite value of the OUTPUT
        type: no intermediate sum can then overflow in any order."""
        if self.typ not in ADD_T:
            return
        half = max_of(self.out_dt) / 2
        for _ in range(200):
            worst = 0.0
            for b in range(self.batch):
                X = self.logical(b)
                X = np.where(np.isfinite(X), X, 0.0)
                ax = 1 if self.rows else 0
                iv = self.init_values(b)
                s1 = np.abs(X).sum(axis=ax) + (np.abs(iv[0]) if iv else 0.0)
                s2 = (X * X).sum(axis=ax) + (np.abs(iv[1]) if iv else 0.0)
                worst = max(worst, float(s1.max()) if want_x(self.typ) else 0.0, float(s2.max()) if want_x2(self.typ) else 0.0)
            if worst < half:
                return
            block = np.zeros(self.in_buf.size, dtype=bool)
            for b in range(self.batch):
                block[self.front + b * self.per: self.front + (b + 1) * self.per][self.idx] = True
            for buf, dt, sel in ((self.in_buf, self.in_dt, block),) + (((self.out_buf, self.out_dt, self.out_mask),) if self.init else ()):
                v = decode(buf, dt)
                sel = sel & np.isfinite(v)
                buf[sel] = encode((v[sel] * 0.5).astype(np.float32), dt)
        raise AssertionError("data do not fit the output type")

    # -- descriptors and runs
    def in_offset_bytes(self):
        return self.front * self.isz

    def expected(self):
        return expected_reduce_kernel(self.typ, self.flags, self.m, self.n, self.ldi, self.in_dt, self.front, self.batch, self.per * self.isz if self.batch > 1 else 0)

    def _param(self, in_ptr, out_ptr, b=0):
        p = capi.UnaryParam()
        p.in_.primary = in_ptr + self.front * self.isz + b * self.per * self.isz
        p.out.primary = out_ptr + b * self.oper * self.osz
        return p

    def shape(self):
        return capi.UnaryShape(self.m, self.n, self.ldi, self.ldo, self.in_dt, self.out_dt, DT.F32)

    def run_oracle(self):
        orc = pyoracle.oracle()
        x, out = self.in_buf.copy(), self.out_buf.copy()
        d = pyoracle.MeltwDesc(self.m, self.n, self.ldi, self.ldo, 0, 0, self.in_dt, DT.UNSUPPORTED, DT.UNSUPPORTED, DT.F32, self.out_dt, self.flags, self.typ, 1)
        for b in range(self.batch):
            orc.meltw(self._param(x.ctypes.data, out.ctypes.data, b), d)
        return out

    def run_reference(self, ref):
        """the reference's loop; it stores ldo elements per result over columns (the gap holds what its malloc held): only the results are meaningful."""
        x, out = self.in_buf.copy(), self.out_buf.copy()
        for b in range(self.batch):
            p = self._param(x.ctypes.data, out.ctypes.data, b)
            ref.lib.xref_reference_meltw_unary(C.byref(p), self.typ, self.shape(), self.flags)
        return out

    def run_gpu(self):
        """(whole output allocation, kernel name)."""
        api = capi.load()
        h = api.dispatch_meltw_unary(self.typ, self.shape(), self.flags)
        assert h, "dispatch returned NULL"
        dx, dy = _upload(self.in_buf), _upload(self.out_buf)
        assert dx.data_ptr() % 256 == 0
        p = self._param(dx.data_ptr(), dy.data_ptr())
        if self.batch == 1:
            capi.Api.call(h, p)
        else:
            api.hip_meltw_unary_batch_strided(h, C.byref(p), self.batch, self.per * self.isz, self.oper * self.osz, 0)
        api.hip_sync(); api.check()
        got = dy.cpu().numpy().view(self.out_buf.dtype)
        assert np.array_equal(bits_of(dx.cpu().numpy().view(self.in_buf.dtype)), bits_of(self.in_buf)), "the input was written"
        return got, api.hip_kernel_name(h, 1 if self.batch > 1 else 0).decode()

    # -- checks
    def results(self, buf, b):
        """(x results, x^2 results) of matrix b as stored codes (None where the type has none)."""
        o = buf[b * self.oper: (b + 1) * self.oper]
        return (o[:self.res] if want_x(self.typ) else None, o[self.x2_at: self.x2_at + self.res] if want_x2(self.typ) else None)

    def check(self, got, what="", oracle_out=None, stats=None):
        """every check of the module docstring on a whole output allocation.  oracle_out: the oracle's allocation, for the serial-order sums."""
        assert got.shape == self.out_buf.shape
        outside = ~self.out_mask
        bad = bits_of(got)[outside] != bits_of(self.out_buf)[outside]
        assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the results were written; first at {int(np.flatnonzero(outside)[np.flatnonzero(bad)[0]])}"
        for b in range(self.batch):
            ex = self.exact(b)
            gx, gx2 = self.results(got, b)
            if self.typ in CMP_T:
                check_extremum(gx, ex["ext"], self.out_dt, bitwise=not self.rows, what=f"{what} matrix {b}")
                continue
            if gx is not None:
                check_sum(gx, ex["sum"], ex["abs"], ex["k"], self.out_dt, what=f"{what} matrix {b} x", stats=stats)
            if gx2 is not None:
                check_sum(gx2, ex["sum2"], ex["sq"], ex["k"], self.out_dt, what=f"{what} matrix {b} x^2", stats=stats)
        if oracle_out is not None and self.typ in ADD_T:
            ok = same_bits(oracle_out[self.out_mask], got[self.out_mask], self.out_dt)
            assert ok.all(), f"{what}: {int((~ok).sum())} serially added sums differ from the oracle's bits; first at result {int(np.flatnonzero(~ok)[0])}"


def sum_bound(ex, S, k, out_dt):
    u = 0.0 if out_dt == DT.F32 else u_out(out_dt)
    return (k + 1) * 2.0 ** -24 * S + k * FLT_MIN + u * np.maximum(np.abs(ex), _TINY[out_dt])


def check_sum(got_codes, ex, S, k, out_dt, what="", stats=None):
    g = decode(got_codes, out_dt)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(ex)
        cls = np.where(np.isnan(ex), np.isnan(g), g == ex)
        err = np.abs(g - np.where(fin, ex, 0.0))
        bound = sum_bound(np.where(fin, ex, 0.0), np.where(fin, S, 0.0), k, out_dt)
        ok = np.where(fin, err <= bound, cls)
    if stats is not None and fin.any():
        stats["ratio"] = max(stats.get("ratio", 0.0), float(np.max(np.where(fin, err / bound, 0.0))))
    if not ok.all():
        q = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} results outside the bound; first: result {q}, exact {ex[q]!r}, got {g[q]!r}, "
                             f"bound {bound[q]!r} (S = {S[q]!r}, k = {k})")


def check_extremum(got_codes, ext, out_dt, bitwise, what=""):
    want = store(ext, out_dt)
    if bitwise:
        ok = bits_of(want) == bits_of(np.ascontiguousarray(got_codes))
    else:
        ok = decode(want, out_dt) == decode(got_codes, out_dt)
    if not ok.all():
        q = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} extrema differ; first: result {q}, exact {decode(want[q:q + 1], out_dt)[0]!r} "
                             f"(0x{int(bits_of(want)[q]):x}), got {decode(got_codes[q:q + 1], out_dt)[0]!r} (0x{int(bits_of(np.ascontiguousarray(got_codes))[q]):x})")


def old_bar_accepts(typ, ref_results, got_results):
    """the bar of tests/test_meltw_gpu.py: array_equal for MAX / MIN / ABSMAX, normf_rel < 1e-5 over the whole result vector for the sums (f32 results)."""
    from helpers import normf_rel
    if typ in CMP_T:
        return bool(np.array_equal(ref_results, got_results))
    with np.errstate(all="ignore"):
        return bool(normf_rel(ref_results, got_results, DT.F32) < 1e-5)


# ---- the shapes -------------------------------------------------------------------------------------------------------------------------------------------
# (path tag, m, n, ldi, extra base offset in elements, batch): the smallest shapes that reach each path of launch_meltw and each loop inside it.  The direction follows
# from the tag.  The column reduction of ONE matrix takes the two-pass form from n = 2048 on (below that the runtime allocates no workspace for the partial results), so
# (8, 130, 8) and (64, 1219, 64) run the one-slice and the sixteen-slice form.
CASES = [
    ("general-rows", 1, 5, 1, 0, 1), ("general-rows", 63, 5, 70, 0, 1),
    ("general-rows", 130, 9, 131, 0, 1),            # two lane trips plus a ragged one, n no multiple of the 4 waves
    ("general-rows", 64, 6, 64, 1, 1),              # the base one element off: forced off the vector path
    ("general-cols", 257, 1, 259, 0, 1), ("general-cols", 33, 33, 40, 0, 1),
    ("vec-rows-cpg4", 4, 64, 4, 0, 1), ("vec-rows-cpg4", 8, 67, 8, 0, 1),
    ("vec-rows-cpg4", 12, 70, 12, 0, 1),            # m / 4 = 3 < G = 4: one idle lane per group
    ("vec-rows-cpg4", 256, 65, 260, 0, 1),
    ("vec-rows", 12, 7, 16, 0, 1),                  # n < 64
    ("vec-rows", 260, 3, 260, 0, 1),                # the tail loop only
    ("vec-rows", 1028, 3, 1028, 0, 1),              # the 4-vector loop plus tail
    ("vec-rows", 4100, 3, 4104, 0, 1),              # the 16-vector loop, then tail
    ("vec-cols-1slice", 4, 1, 4, 0, 1),
    ("vec-cols-1slice", 68, 21, 72, 0, 1),          # two blocks, a ragged row group, 16 + 4 + 1 columns
    ("vec-cols-1slice", 64, 255, 64, 0, 3),
    ("vec-cols-1slice", 8, 130, 8, 0, 1),
    ("vec-cols-16slice", 8, 256, 8, 0, 2), ("vec-cols-16slice", 68, 257, 68, 0, 2), ("vec-cols-16slice", 16, 600, 20, 0, 2),
    ("vec-cols-16slice", 64, 1219, 64, 0, 1),
    ("two-pass", 8, 2048, 8, 0, 1),                 # the smallest n: 32 chunks of 64 columns, four per slice
    ("two-pass", 64, 2100, 64, 0, 1),               # 32 chunks of 66 columns, the last one ragged (54); the combine's 16-loop, then its tail
]
ROWS_TAGS = ("general-rows", "vec-rows-cpg4", "vec-rows")


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}ld{c[3]}" + (f"off{c[4]}" if c[4] else "") + (f"b{c[5]}" if c[5] > 1 else "")


def first_of_path(c):
    return c == next(k for k in CASES if k[0] == c[0])


# ---- listed columns and the recorded argop ----------------------------------------------------------------------------------------------------------------
SENTINEL = 77


class ListedCase:
    """REDUCE_COLS_IDX_OP_ADD / MAX / MIN over a list with repeats (listed = False: REDUCE_X_OP_MAX / MIN / ABSMAX over all columns with REDUCE_RECORD_ARGOP), m = 45 rows
    of a 30-column table at ldi = 48.  Unlisted columns, padding rows and what surrounds the table hold the poison; results and recorded columns have three sentinel
    elements behind them.  Rows 0 .. 2 are made by hand (MAX / MIN / ABSMAX): row 0 reads NaN in every listed column, row 1 -inf (MIN: +inf) in every listed column,
    row 2 its extremum twice, in columns 4 and 9 (the list ends 4, 9, 4)."""

    def __init__(self, typ, in_dt, idx8, record, data, listed=True, m=45, ldi=48, width=30, seed=0):
        self.typ, self.in_dt, self.idx8, self.record, self.listed, self.m, self.ldi, self.width = typ, in_dt, idx8, record, listed, m, ldi, width
        rng = np.random.default_rng(seed)
        self.is_min = typ in (UNARY.REDUCE_COLS_IDX_OP_MIN, UNARY.REDUCE_X_OP_MIN)
        self.is_add = typ == UNARY.REDUCE_COLS_IDX_OP_ADD
        cols = np.concatenate([rng.integers(0, width, 14), [4, 9, 4]]) if listed else np.arange(width)
        codes = wide(rng, width, m, in_dt, False) if data == "wide" else infinite(rng, width, m, in_dt, False, self.is_add)
        used = np.unique(cols)
        if not self.is_add:
            codes[:, 0][used] = nan_of(in_dt)
            codes[:, 1][used] = encode(np.float32(np.inf if self.is_min else -np.inf), in_dt)
            codes[:, 2][used] = encode(np.float32(1.0), in_dt)
            codes[:, 2][[4, 9]] = encode(np.float32(-900.0 if self.is_min else 900.0), in_dt)
        self.buf = np.full(FRONT + ldi * width + TAIL, poison_of(typ, in_dt), dtype=NP_OF[in_dt])
        self.buf[FRONT: FRONT + ldi * width].reshape(width, ldi)[used, :m] = codes[used]
        self.out0 = np.full(m + 3, -7.0, dtype=np.float32)
        self.itype = np.uint64 if idx8 else np.uint32
        self.idx, self.arg0 = cols.astype(self.itype), np.full(m + 3, SENTINEL, dtype=self.itype)
        self.flags = UNARY_FLAG.REDUCE_COLS | (0 if idx8 else UNARY_FLAG.IDX_SIZE_4BYTES) | (UNARY_FLAG.REDUCE_RECORD_ARGOP if record else 0)
        self.cnt = C.c_ulonglong(len(cols))

    def _param(self, x, o, i, a):
        p = capi.UnaryParam()
        p.in_.primary, p.out.primary = x + FRONT * capi.DT_SIZE[self.in_dt], o
        if self.listed:
            p.in_.secondary, p.in_.tertiary = i, C.addressof(self.cnt)
        if self.record:
            p.out.secondary = a
        return p

    def run_oracle(self):
        x, ref, ref_arg = self.buf.copy(), self.out0.copy(), self.arg0.copy()
        d = pyoracle.MeltwDesc(self.m, self.width, self.ldi, self.m, 0, 0, self.in_dt, DT.UNSUPPORTED, DT.UNSUPPORTED, DT.F32, DT.F32, self.flags, self.typ, 1)
        pyoracle.oracle().meltw(self._param(x.ctypes.data, ref.ctypes.data, self.idx.ctypes.data, ref_arg.ctypes.data), d)
        return ref, ref_arg

    def run_gpu(self):
        api = capi.load()
        h = api.dispatch_meltw_unary(self.typ, capi.UnaryShape(self.m, self.width, self.ldi, self.m, self.in_dt, DT.F32, DT.F32), self.flags)
        assert h, "dispatch returned NULL"
        dx, dy, di, da = _upload(self.buf), _upload(self.out0), _upload(self.idx), _upload(self.arg0)
        capi.Api.call(h, self._param(dx.data_ptr(), dy.data_ptr(), di.data_ptr(), da.data_ptr()))
        api.hip_sync(); api.check()
        return dy.cpu().numpy(), da.cpu().numpy().view(self.itype), api.hip_kernel_name(h, 0).decode()

    def check(self, got, got_arg, ref, ref_arg):
        """got against the oracle (the reference's serial loop: bit for bit, the sentinels behind the results included) and against what rows 0 .. 2 must give."""
        m, typ = self.m, self.typ
        ok = same_bits(ref, got, DT.F32)
        assert ok.all(), np.flatnonzero(~ok)[:4]
        assert np.array_equal(got[m:], self.out0[m:])
        if self.record:
            assert np.array_equal(ref_arg, got_arg)
        else:
            assert np.array_equal(got_arg, self.arg0)
        if self.is_add:
            return
        absmax = typ == UNARY.REDUCE_X_OP_ABSMAX
        start = FLT_MAX if self.is_min else 0.0 if absmax else -FLT_MAX
        if self.record or self.is_min:
            assert got[0] == start                                  # x >= acc, x <= acc and MIN(x, acc) = x < acc ? x : acc never take a NaN
        else:
            assert np.isnan(got[0])                                 # MAX(x, acc) = x < acc ? acc : x does
        assert got[1] == (np.inf if absmax else start)              # nor does the infinity beyond the start value (ABSMAX: |-inf|)
        assert got[2] == (-900.0 if self.is_min else 900.0)
        if self.record:
            assert got_arg[0] == SENTINEL and (absmax or got_arg[1] == SENTINEL)
            assert got_arg[2] == (4 if self.listed else 9)          # the later equal extremum
            assert np.all(got_arg[m:] == SENTINEL)


def zero_ties(rng, n, m):
    """[n][m] f32 for the column direction: rows 0 .. 4 have a zero as their extremum, twice, with both signs (columns 3 and 7): MAX(x, acc) keeps the LAST of two equal
    values, MIN(x, acc) the FIRST, and ABS(-0) = -0."""
    assert n >= 8 and m >= 5
    x = wide(rng, n, m, DT.F32, False)
    x[:, 0:2] = -1.0                                  # MAX: the later zero
    x[3, 0], x[7, 0], x[3, 1], x[7, 1] = 0.0, -0.0, -0.0, 0.0
    x[:, 2] = 0.0                                     # ABSMAX: nothing but zeros, the last one negative
    x[n - 1, 2] = -0.0
    x[:, 3:5] = 1.0                                   # MIN: the earlier zero
    x[3, 3], x[7, 3], x[3, 4], x[7, 4] = 0.0, -0.0, -0.0, 0.0
    return x
