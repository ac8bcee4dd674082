"""Matrix-equation parity (libxsmm_dispatch_meqn) PER ELEMENT over the whole input range, at padded leading dimensions with poisoned padding, through both
evaluation paths (the generated kernel and the chain of TPP launches) -- what tests/meltw_ew_helpers.py and tests/meltw_reduce_helpers.py do for the TPPs.

  EqCase     one tree in tests/test_meqn.py's notation, its argument shapes and output shape.  Every argument is built at its leading dimension plus a tail,
             everything outside its m x n block holds the type's NaN; the output holds -7 everywhere.  `expect` names the kernel a handle dispatched with
             LIBXSMM_HIP_JIT=2 must report (meqn_jit_e / meqn_jit_r / meqn_tpp_chain); with LIBXSMM_HIP_JIT=0 it is always meqn_tpp_chain.
  ref64      a float64 walk of the tree: (t, e) per element, t the value of the f32 formula in float64 and e a running absolute error bound.
                 leaf       t = the argument as the reference loads it (a bf16 denormal is a signed zero), e = 0
                 every node e = [the largest |f(corner) - t| over the corners of the operands' intervals [t_i - e_i, t_i + e_i]]  +  2^-24 |t|  +  FLT_MIN
                            (one f32 rounding, one flushed denormal); selections (IDENTITY, NEGATE, RELU, MAX, MIN) round nothing and add nothing
                 libm       TANH / SIGMOID / EXP add K_OP[op] 2^-24 S_op (meltw_ew_helpers.restate64); RECIPROCAL_SQRT is two correctly rounded operations
                 sums       REDUCE_X_OP_ADD / X2_OP_ADD, the dot product, MATMUL: sum of the propagated e_i  +  (k + 1) 2^-24 sum |t_i|  +  k FLT_MIN, k terms
                            (meltw_reduce_helpers: any order of k additions).  A REDUCE_COLS / REDUCE_ROWS pair is two such sums (N terms, then M): the
                            generated kernel's order -- ceil(units / 256) serial units of 8 per thread, then an 8-level tree in LDS -- is no deeper.
                 extrema    the largest e_i of the line; a REDUCE_COLS extremum starts at -+FLT_MAX [ref: mateltwise ref :1378,:1405]
                 a pole or an overflow threshold inside an interval makes e infinite: either side of it is a correct f32 result.  Such elements stay in
                 the check (a NaN still fails) and are what empty_share counts.
             The store of the result is NOT part of t: the check grants it as u_out (|t| + e), so that t stays the point both paths round FROM.
  check      |got - t| <= e + u_out (|t| + e) + FLT_MIN on EVERY element; a non-finite t: the class must agree (NaN, or the infinity of that sign); a result at
             the overflow threshold of the output type may be that infinity (the rule of meltw_ew_helpers.assert_approx).
  empty_share  the share of the finite, normal (|t| >= FLT_MIN) results whose running bound e exceeds 2^-12 |t| + FLT_MIN (f32 output) or 2^-6 |t| (bf16
               output): at most MAX_EMPTY on every row.  GUARD_DOMAIN restricts the inputs the share is taken over for the rows that name one (the CHECK always
               covers the whole table).
  rules      chain against the oracle composition: same_bits unless the tree holds libm, a sum or a MATMUL (then ref64);
             generated kernel against the chain: same_bits for element-wise trees (libm included: the same device libm, contraction off) and for trees whose
             reductions are per row over the columns (serial, the reference's order) or extrema; ref64 where a SUM folds to ONE number (a tree in LDS).
"""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np

import test_meqn as tm
from gemm_ld_helpers import GAP_CODE, NAN_CODE
from libxsmm_amd import capi
from libxsmm_amd.capi import BINARY, DT, TERNARY, UNARY, UNARY_FLAG
from meltw_ew_helpers import FLT_MAX, FLT_MIN, K_OP, bits_of, decode, layout_index, max_of, restate64, same_bits, u_out, NONE
from meltw_reduce_helpers import load64

U = 2.0 ** -24
TAIL = 5
MAX_EMPTY = 0.10
LIBM = (UNARY.TANH, UNARY.SIGMOID, UNARY.EXP)
SELECT = (UNARY.IDENTITY, UNARY.NEGATE, UNARY.RELU, UNARY.DUMP)
SUMS = (UNARY.REDUCE_X_OP_ADD, UNARY.REDUCE_X2_OP_ADD)
NPDT = tm.NPDT


def _nan(dt):
    return np.nan if dt == DT.F32 else NAN_CODE[dt]


def _gap(dt):
    return -7.0 if dt == DT.F32 else GAP_CODE[dt]


# ---- the tree ---------------------------------------------------------------------------------------------------------------------------------------------
def shape_of(t, arg_shapes):
    """(m, n) of a node's result [ref: src/libxsmm_matrixeqn.c:869-936]."""
    if t[0] == "arg":
        return arg_shapes[t[1]][0], arg_shapes[t[1]][1]
    kids = [shape_of(c, arg_shapes) for c in t[3:]]
    if t[0] == "mm":
        return kids[0][0], kids[1][1]
    if t[0] == "u" and t[1] in tm.REDUCES:
        return (kids[0][1], 1) if t[2] & UNARY_FLAG.REDUCE_ROWS else (kids[0][0], 1)
    if t[0] == "b" and t[1] == BINARY.MUL_AND_REDUCE_TO_SCALAR_OP_ADD:
        return 1, 1
    return max(k[0] for k in kids), max(k[1] for k in kids)


def nodes(t):
    yield t
    if t[0] != "arg":
        for c in t[3:]:
            yield from nodes(c)


def traits(tree, arg_shapes):
    """what decides the comparison rule: libm, sum (any sum reduction, dot product), mm, fold (a SUM whose result is ONE number: added as a tree in LDS)."""
    r = dict(libm=False, sum=False, mm=False, fold=False)
    for t in nodes(tree):
        if t[0] == "mm":
            r["mm"] = True
        elif t[0] == "u" and t[1] in LIBM:
            r["libm"] = True
        elif t[0] == "u" and t[1] in tm.REDUCES:
            r["sum"] |= t[1] in SUMS
            r["fold"] |= t[1] in SUMS and shape_of(t, arg_shapes) == (1, 1)
        elif t[0] == "b" and t[1] == BINARY.MUL_AND_REDUCE_TO_SCALAR_OP_ADD:
            r["sum"] = r["fold"] = True
    return r


def chain_rule(tree, arg_shapes):
    """chain (or the reference's own evaluator) against the oracle composition."""
    tr = traits(tree, arg_shapes)
    return "ref64" if tr["libm"] or tr["sum"] or tr["mm"] else "same_bits"


def fused_rule(tree, arg_shapes):
    """generated kernel against the chain, from the same bytes.  (An extremum folded to one number is the same number in any order: same_bits.  The tables of
    such rows hold no NaN -- the documented contract -- and their extremum is no zero, so the +-0 tie of meltw_reduce_helpers cannot arise.)"""
    return "ref64" if traits(tree, arg_shapes)["fold"] else "same_bits"


def leaf_order(tree):
    """input positions in the order the code generator meets them: the kernel-argument order of a generated kernel."""
    order = []
    for t in nodes(tree):
        if t[0] == "arg" and t[1] not in order:
            order.append(t[1])
    return order


# ---- ref64 ------------------------------------------------------------------------------------------------------------------------------------------------
def _corners(f, ts, es):
    """t = f(ts) and the largest |f - t| over the corners of the operands' intervals (NaN at a corner: no bound)."""
    with np.errstate(all="ignore"):
        t = f(*ts)
        worst = np.zeros(np.shape(t))
        for signs in itertools.product((-1.0, 1.0), repeat=len(ts)):
            d = np.abs(f(*[np.where(e > 0, x + s * e, x) for x, e, s in zip(ts, es, signs)]) - t)
            worst = np.maximum(worst, np.where(np.isnan(d), np.inf, d))
    return t, worst


def _settle(t, e):
    """what an f32 result can be: beyond FLT_MAX the infinity, at the threshold either (no bound); a non-finite t carries no bound (its class is checked)."""
    with np.errstate(all="ignore"):
        a = np.abs(t)
        over = np.isfinite(t) & (a - e > FLT_MAX * (1 + U))
        edge = np.isfinite(t) & ~over & ((a + e) * (1 + U) >= FLT_MAX)
        t = np.where(over, np.sign(t) * np.inf, t)
        e = np.where(edge, np.inf, e)
        return t, np.where(np.isfinite(t), e, 0.0)


_UN = {UNARY.IDENTITY: lambda x: x, UNARY.DUMP: lambda x: x, UNARY.NEGATE: lambda x: -x, UNARY.RELU: lambda x: np.where(x <= 0, 0.0, x), UNARY.X2: lambda x: x * x,
       UNARY.INC: lambda x: x + 1.0, UNARY.SQRT: np.sqrt, UNARY.RECIPROCAL: lambda x: 1.0 / x, UNARY.RECIPROCAL_SQRT: lambda x: 1.0 / np.sqrt(x),
       UNARY.TANH: np.tanh, UNARY.SIGMOID: lambda x: (np.tanh(x / 2) + 1) / 2, UNARY.EXP: np.exp}
_BIN = {BINARY.ADD: lambda x, y: x + y, BINARY.SUB: lambda x, y: x - y, BINARY.MUL: lambda x, y: x * y, BINARY.DIV: lambda x, y: x / y,
        BINARY.MAX: lambda x, y: np.where(x > y, x, y), BINARY.MIN: lambda x, y: np.where(x > y, y, x)}


def _pole(t, e):
    return (e > 0) & (np.abs(t) <= e)


def ref64(tree, arg_shapes, arrays):
    """(t, e) as [n][m] float64 arrays of the head's extent."""
    def rounded(t, prop, extra=0.0, roundings=1):
        with np.errstate(all="ignore"):
            return _settle(t, prop + extra + roundings * (U * np.abs(t) + FLT_MIN))

    def total(t, e, k, axis):
        """a sum of k terms along an axis: ((k + 1) 2^-24 sum |t_i| + k FLT_MIN) on top of the terms' own bounds."""
        with np.errstate(all="ignore"):
            s = t.sum(axis=axis, keepdims=True)
            b = e.sum(axis=axis, keepdims=True) + (k + 1) * U * np.abs(t).sum(axis=axis, keepdims=True) + k * FLT_MIN
        return _settle(s, np.where(np.isnan(b), np.inf, b))

    def ev(t):
        if t[0] == "arg":
            m, n, ld, dt = arg_shapes[t[1]]
            x = load64(np.asarray(arrays[t[1]])[layout_index(NONE, m, n, ld)], dt)
            return x, np.zeros(x.shape)
        kids = [ev(c) for c in t[3:]]
        ts, es = [k[0] for k in kids], [k[1] for k in kids]
        if t[0] == "mm":                                         # [n][k] x [k][m] in [col][row] storage: out(j, i) = sum_s A(s, i) B(j, s)
            (a, ea), (b, eb) = kids
            k = a.shape[0]
            if t[1] == BINARY.MATMUL_A_VNNI:                     # A(i, s) of an argument in VNNI-2 layout: [k / 2][ld][2]
                m, n, ld, dt = arg_shapes[t[3][1]]
                s, i = np.arange(n)[:, None], np.arange(m)[None, :]
                a = load64(np.asarray(arrays[t[3][1]])[(s // 2) * ld * 2 + i * 2 + s % 2], dt)
            with np.errstate(all="ignore"):
                terms = b[:, :, None] * a[None, :, :]
                te = np.abs(b)[:, :, None] * ea[None, :, :] + eb[:, :, None] * np.abs(a)[None, :, :] + eb[:, :, None] * ea[None, :, :]
            s, e = total(terms, te, k, 1)
            return s[:, 0, :], e[:, 0, :]
        if t[0] == "u" and t[1] in tm.REDUCES:
            x, e = kids[0]
            over_rows = bool(t[2] & UNARY_FLAG.REDUCE_ROWS)
            axis = 1 if over_rows else 0
            if t[1] in SUMS:
                if t[1] == UNARY.REDUCE_X2_OP_ADD:
                    x, e = rounded(*_corners(_UN[UNARY.X2], [x], [e]), roundings=0)
                s, b = total(x, e, x.shape[axis], axis)
            else:
                big = t[1] == UNARY.REDUCE_X_OP_MAX
                s = (x.max if big else x.min)(axis=axis, keepdims=True)
                if not over_rows:
                    s = np.maximum(s, -FLT_MAX) if big else np.minimum(s, FLT_MAX)
                b = e.max(axis=axis, keepdims=True)
            return s.reshape(1, -1), b.reshape(1, -1)               # a vector result is m x 1 whichever way it was reduced
        if t[0] == "b" and t[1] == BINARY.MUL_AND_REDUCE_TO_SCALAR_OP_ADD:
            p, e = rounded(*_corners(_BIN[BINARY.MUL], ts, es), roundings=0)
            s, b = total(p.reshape(1, -1), e.reshape(1, -1), p.size, 1)
            return s, b
        if t[0] == "u":
            op = t[1]
            v, prop = _corners(_UN[op], ts, es)
            if op in (UNARY.RECIPROCAL, UNARY.RECIPROCAL_SQRT):
                prop = np.where(_pole(ts[0], es[0]), np.inf, prop)
            if op in SELECT:
                return _settle(v, prop)
            if op in LIBM:
                with np.errstate(all="ignore"):
                    extra = K_OP[op] * U * restate64(op, ts[0])[1]
                return rounded(v, prop, np.where(np.isfinite(extra), extra, 0.0))
            return rounded(v, prop, roundings=2 if op == UNARY.RECIPROCAL_SQRT else 1)
        if t[0] == "b":
            v, prop = _corners(_BIN[t[1]], ts, es)
            if t[1] == BINARY.DIV:
                prop = np.where(_pole(ts[1], es[1]), np.inf, prop)
            return _settle(v, prop) if t[1] in (BINARY.MAX, BINARY.MIN) else rounded(v, prop)
        assert t[1] in (TERNARY.MULADD, TERNARY.NMULADD), t[1]
        # MULADD: in2 + in0 * in1; NMULADD: in1 - in0 * in2 -- the product is rounded on its own (contraction off)
        a, b, c = (0, 1, 2) if t[1] == TERNARY.MULADD else (0, 2, 1)
        p, pe = rounded(*_corners(_BIN[BINARY.MUL], [ts[a], ts[b]], [es[a], es[b]]))
        return rounded(*_corners(_BIN[BINARY.ADD if t[1] == TERNARY.MULADD else BINARY.SUB], [ts[c], p], [es[c], pe]))

    t, e = ev(tree)
    m, n = shape_of(tree, arg_shapes)
    return np.broadcast_to(t, (n, m)).copy(), np.broadcast_to(e, (n, m)).copy()


def bound_of(t, e, out_dt):
    with np.errstate(all="ignore"):
        return e + u_out(out_dt) * (np.abs(t) + e) + FLT_MIN


def ref64_ratio(got, t, e, out_dt):
    """(err / bound per element, ok per element).  got: the results decoded to float64."""
    g = np.asarray(got, dtype=np.float64)
    u, top = u_out(out_dt), max_of(out_dt)
    with np.errstate(all="ignore"):
        bound = bound_of(t, e, out_dt)
        err = np.abs(g - t)
        fin = np.isfinite(t)
        may_inf = fin & ((np.abs(t) + e) * (1 + u) >= top) & np.isinf(g) & (np.sign(g) == np.sign(t))
        ok_fin = (err <= bound) | may_inf
        ok_cls = np.where(np.isnan(t), np.isnan(g), g == t)
        ratio = np.where(fin & np.isfinite(bound) & ~may_inf & ~np.isnan(g), err / bound, 0.0)
    return ratio, np.where(fin, ok_fin, ok_cls)


def assert_ref64(got, t, e, out_dt, what="", stats=None):
    ratio, ok = ref64_ratio(got, t, e, out_dt)
    if stats is not None:
        stats["ratio"] = max(stats.get("ratio", 0.0), float(ratio.max()))
    if not ok.all():
        k = np.unravel_index(int(np.flatnonzero(~ok.ravel())[0]), ok.shape)
        raise AssertionError(f"{what}: {np.count_nonzero(~ok)} of {ok.size} elements outside the ref64 bound; first at (col, row) {k}: t = {t[k]!r}, e = {e[k]!r}, "
                             f"got {np.asarray(got)[k]!r}, err / bound = {float(ratio[k]):.3f}")


def empty_share(t, e, out_dt, where=None):
    """share of the finite results whose running bound says (almost) nothing.  Counted over the results that are normal f32 numbers: the bf16 cap has no
    FLT_MIN term, so an exact zero or an underflowed result (whose bound IS a few FLT_MIN, and says a lot) would count as empty whatever the bound."""
    with np.errstate(all="ignore"):
        fin = np.isfinite(t) & (np.abs(t) >= FLT_MIN)
    if where is not None:
        fin = fin & where
    with np.errstate(all="ignore"):
        cap = 2.0 ** -12 * np.abs(t) + FLT_MIN if out_dt == DT.F32 else 2.0 ** -6 * np.abs(t)
    return float(np.count_nonzero(fin & (e > cap))) / max(1, int(np.count_nonzero(fin)))


def assert_same_bits(ref, got, dt, what=""):
    ok = same_bits(ref, got, dt)
    if not ok.all():
        k = np.unravel_index(int(np.flatnonzero(~ok.ravel())[0]), ok.shape)
        raise AssertionError(f"{what}: {np.count_nonzero(~ok)} of {ok.size} elements differ; first at (col, row) {k}: "
                             f"ref 0x{int(bits_of(ref)[k]):x} ({decode(ref[k], dt)!r}) got 0x{int(bits_of(got)[k]):x} ({decode(got[k], dt)!r})")


# ---- one equation -----------------------------------------------------------------------------------------------------------------------------------------
class EqCase:
    """tree, arg_shapes [(m, n, ld, dt)], out_shape (m, n, ld, dt); expect: the kernel of a LIBXSMM_HIP_JIT=2 handle; comp: the op type of every node."""

    def __init__(self, tree, arg_shapes, out_shape, expect, comp=DT.F32):
        self.tree, self.shapes, self.out_shape, self.expect, self.comp = tree, list(arg_shapes), tuple(out_shape), expect, comp
        assert expect in ("meqn_jit_e", "meqn_jit_r", "meqn_tpp_chain")
        self.m, self.n = shape_of(tree, self.shapes)                   # the head's own extent (a reducing head: 1 x 1 whatever the caller declares)
        self.ldo, self.odt = out_shape[2], out_shape[3]
        self.out_idx = layout_index(NONE, self.m, self.n, self.ldo)
        self.out_elems = self.ldo * (self.n - 1) + self.m + TAIL

    # -- buffers
    def arg_elems(self, k):
        m, n, ld, _ = self.shapes[k]
        return ld * n + TAIL                                           # (the oracle composition takes ld * n elements per argument)

    def pack(self, values):
        """values[k]: [n][m] logical values of argument k in its storage type -> the poisoned buffers."""
        bufs = []
        for k, (m, n, ld, dt) in enumerate(self.shapes):
            b = np.full(self.arg_elems(k), _nan(dt), dtype=NPDT[dt])
            b[layout_index(NONE, m, n, ld)] = np.asarray(values[k]).reshape(n, m)
            bufs.append(b)
        return bufs

    def new_out(self):
        return np.full(self.out_elems, _gap(self.odt), dtype=NPDT[self.odt])

    def logical(self, out):
        return np.asarray(out)[self.out_idx]

    def out64(self, out):
        return decode(self.logical(out), self.odt)

    # -- executors
    def oracle(self, bufs):
        """the oracle composition's logical result [n][m] (its own zero-initialised output: the padding is the device's business)."""
        out = tm.evaluate(self.tree, self.shapes, [b.copy() for b in bufs], (self.m, self.n, self.ldo, self.odt), comp=self.comp)
        return np.asarray(out)[self.out_idx]

    def ref64(self, bufs):
        return ref64(self.tree, self.shapes, bufs)

    def dispatch(self, api, jit):
        before = api.hip_get_jit()
        api.hip_set_jit(jit)
        try:
            h = api.dispatch_meqn(tm.build(api, self.tree, self.shapes, comp=self.comp), capi.MeqnArgShape(*self.out_shape))
        finally:
            api.hip_set_jit(before)
        assert h, "dispatch returned NULL"
        name = api.hip_kernel_name(h, 0).decode()
        want = self.expect if jit == 2 else "meqn_tpp_chain"
        assert name.startswith(want) and (want != "meqn_tpp_chain" or name == want), f"jit={jit}: kernel {name}, expected {want}"
        return h

    # -- checks
    def check_untouched(self, out, what=""):
        """every byte outside the head's m x n block still holds the sentinel."""
        mask = np.ones(self.out_elems, dtype=bool)
        mask[self.out_idx.ravel()] = False
        bad = bits_of(np.asarray(out))[mask] != bits_of(self.new_out())[mask]
        assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the {self.m} x {self.n} result were written (first: element {int(np.flatnonzero(mask)[np.flatnonzero(bad)[0]])})"

    def check(self, out, rule, ref_logical, bufs=None, te=None, what="", stats=None):
        """out: a whole output allocation.  rule 'same_bits': against ref_logical; 'ref64': against (t, e) (computed from bufs when not given)."""
        self.check_untouched(out, what)
        if rule == "same_bits":
            assert_same_bits(ref_logical, self.logical(out), self.odt, what)
        else:
            t, e = te if te is not None else self.ref64(bufs)
            assert_ref64(self.out64(out), t, e, self.odt, what, stats)


def upload(x):
    import torch
    v = {np.uint16: np.int16}.get(x.dtype.type)
    return torch.from_numpy(np.ascontiguousarray(x.view(v) if v else x)).to("cuda:0")


def call(api, h, ptrs, out_ptr):
    tm._call(api, h, ptrs, out_ptr)
    api.hip_sync(); api.check()


def run_gpu(case, api, h, bufs, arg_offset=None, out_offset=0):
    """One call of handle h on fresh device copies of bufs and a fresh poisoned output; returns the whole output allocation.
    arg_offset = (k, elements): argument k is uploaded that many elements into a larger allocation (its pointer moves, its bytes do not)."""
    dev = []
    ptrs = []
    for k, b in enumerate(bufs):
        shift = arg_offset[1] if arg_offset and arg_offset[0] == k else 0
        d = upload(np.concatenate([np.full(shift, _nan(case.shapes[k][3]), dtype=b.dtype), b]) if shift else b)
        dev.append(d); ptrs.append(d.data_ptr() + shift * b.itemsize)
    o0 = case.new_out()
    out = upload(np.concatenate([np.full(out_offset, _gap(case.odt), dtype=o0.dtype), o0]) if out_offset else o0)
    call(api, h, ptrs, out.data_ptr() + out_offset * o0.itemsize)
    got = out.cpu().numpy().view(o0.dtype)
    if out_offset:
        assert np.array_equal(bits_of(got[:out_offset]), bits_of(np.full(out_offset, _gap(case.odt), dtype=o0.dtype))), "the elements in front of the output were written"
    for k, (d, b) in enumerate(zip(dev, bufs)):
        back = d.cpu().numpy().view(b.dtype)
        assert np.array_equal(bits_of(back[back.size - b.size:]), bits_of(b)), f"argument {k} was written"
    return got[out_offset:]


# ---- the generated kernels on the host (the emulation of tests/test_jit_emulated_cpu.py) ----------------------------------------------------------------------
def emulate(tmp_path, case):
    """Generates the kernel of `case` in a dry-run child, builds the same text for the host and returns (kernel name, launch(bufs, out))."""
    import test_jit_emulated_cpu as emu
    args = {"root": emu.ROOT, "tests": os.path.join(emu.ROOT, "tests"), "case": emu._plain((case.tree, case.shapes, case.out_shape))}
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1", LIBXSMM_HIP_JIT="2", LIBXSMM_HIP_JIT_DUMP=str(tmp_path))
    env.pop("LIBXSMM_VERBOSE", None); env.pop("LIBXSMM_HIP_MEQN_VECRED", None)
    r = subprocess.run([sys.executable, "-c", emu.VECRED_CHILD % args], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    kernel = [ln for ln in r.stdout.splitlines() if ln.startswith("KERNEL ")][-1][7:]
    assert kernel.startswith(case.expect), kernel
    src = open(tmp_path / (kernel + ".hip")).read()
    sig = re.search(r"void " + kernel + r"\(([^)]*)\)", src).group(1)
    params = [p.strip().split()[-1] for p in sig.split(",")]
    order = leaf_order(case.tree)
    assert params == [f"in{i}" for i in range(len(order))] + ["out"], params
    host = re.sub(r"#define GM .*", "#define GM", src)
    phased = kernel.startswith("meqn_jit_r")
    if phased:
        text = emu.PHASED_PRELUDE + host + emu.PHASED_DRIVER.replace("KERNEL", kernel).replace("ARGS", ", ".join(f"l->a[{i}]" for i in range(len(params))))
    else:
        total = int(re.search(r"if \(t >= (\d+)LL\) return;", src).group(1))
        text = emu.MEQN_PRELUDE + host + 'extern "C" int emulate_launch(void** a) {\n  for (long long t = 0; t < %d; ++t) { blockIdx.x = (unsigned int)(t / 256); threadIdx.x = (unsigned int)(t %% 256);\n    %s(%s); }\n  return 0;\n}\n' % (
            (total + 255) // 256 * 256, kernel, ", ".join(f"a[{i}]" for i in range(len(params))))
    cpp = tmp_path / "emulated.cpp"
    cpp.write_text(text)
    so = str(tmp_path / "emulated.so")
    c = subprocess.run([emu.CLANG, "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off", "-mfma", "-shared", "-fPIC", "-pthread", str(cpp), "-o", so], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-3000:]
    lib = C.CDLL(so)
    lib.emulate_launch.argtypes = [C.c_void_p]

    def launch(bufs):
        out = case.new_out()
        held = [b.copy() for b in bufs]
        ptrs = (C.c_void_p * len(params))(*[held[k].ctypes.data for k in order], out.ctypes.data)
        assert lib.emulate_launch(ptrs) == 0
        for k, (a, b) in enumerate(zip(held, bufs)):
            assert np.array_equal(bits_of(a), bits_of(b)), f"argument {k} was written"
        return out
    return kernel, launch


# ---- trees --------------------------------------------------------------------------------------------------------------------------------------------------
A = tm.A
RC, RR = UNARY_FLAG.REDUCE_COLS, UNARY_FLAG.REDUCE_ROWS
BF = capi.BINARY_FLAG
TF = capi.TERNARY_FLAG


def to_one(op, x):
    """a REDUCE_COLS / REDUCE_ROWS pair: ONE number."""
    return ("u", op, RR, ("u", op, RC, x))


def t_recip_mul():
    """RECIPROCAL(a0) * a1: a bf16 denormal in a0 is a zero, its reciprocal an infinity."""
    return ("b", BINARY.MUL, 0, ("u", UNARY.RECIPROCAL, 0, A(0)), A(1))


def t_unary(op):
    return ("u", op, 0, A(0))


def t_binary(op):
    return ("b", op, 0, A(0), A(1))


def t_bcasts():
    """(a0 * row(a1) + col(a2)) * scalar(a3)"""
    return ("b", BINARY.MUL, BF.BCAST_SCALAR_IN_1, ("t", TERNARY.MULADD, TF.BCAST_ROW_IN_1 | TF.BCAST_COL_IN_2, A(0), A(1), A(2)), A(3))


def t_minus_max():
    """x - max x: the scalar MAX phase alone (every operation exact or correctly rounded)."""
    return ("b", BINARY.SUB, BF.BCAST_SCALAR_IN_1, A(0), to_one(UNARY.REDUCE_X_OP_MAX, A(0)))


def t_col_softmax():
    """exp(x - colmax) / colsum, max and sum per row over the columns: two vector phases.  (The quotient is a DIV node: a RECIPROCAL of the vector of sums is
    arithmetic on a vector, which the code generator leaves to the chain.)"""
    ex = ("u", UNARY.EXP, 0, ("b", BINARY.SUB, BF.BCAST_COL_IN_1, A(0), ("u", UNARY.REDUCE_X_OP_MAX, RC, A(0))))
    return ("b", BINARY.DIV, BF.BCAST_COL_IN_1, ex, ("u", UNARY.REDUCE_X_OP_ADD, RC, ex))


def t_col_softmax_reciprocal():
    """exp(x - colmax) * (1 / colsum): the RECIPROCAL of the vector of sums is arithmetic on a vector -- no phase of the generated kernel, so the chain runs."""
    ex = ("u", UNARY.EXP, 0, ("b", BINARY.SUB, BF.BCAST_COL_IN_1, A(0), ("u", UNARY.REDUCE_X_OP_MAX, RC, A(0))))
    return ("b", BINARY.MUL, BF.BCAST_COL_IN_1, ex, ("u", UNARY.RECIPROCAL, 0, ("u", UNARY.REDUCE_X_OP_ADD, RC, ex)))


def t_sum_head():
    return to_one(UNARY.REDUCE_X_OP_ADD, A(0))


def reshaped(name, m, n, ld=None):
    """an entry of test_meqn.CASES whose full-size operands all share one shape, at another m x n (1 x 1 and vector operands keep their kind)."""
    tree, shapes, out = tm.CASES[name]
    M0, N0 = max(s[0] for s in shapes), max(s[1] for s in shapes)
    fit = lambda s: ((m if s[0] == M0 else s[0]), (n if s[1] == N0 else s[1]), ((ld or m) if s[0] == M0 else s[2]), s[3])   # noqa: E731
    return tree, [fit(s) for s in shapes], (fit(out) if (out[0], out[1]) != (1, 1) else out)


# ---- tables (the generators of meltw_ew_helpers / meltw_reduce_helpers, cut and scaled to an operand) -------------------------------------------------------------
def _as(dt, f32):
    from meltw_ew_helpers import encode
    return f32.astype(np.float32) if dt == DT.F32 else encode(f32, DT.BF16)


def table(kind, dt, m, n, seed):
    """[n][m] values of type dt.
    wide      meltw_reduce_helpers.wide: normal * 2^[-20, 8], +-0, denormals (bf16: denormal codes), cancelling pairs.  No NaN, no inf.
    mild      wide * 2^-6 (exact): what a softmax can take without every exponential underflowing
    small     wide * 2^-9: what sigmoid's (tanh + 1) / 2 can take without cancelling
    nonzero   mild with the zeros and denormals replaced by 1: a factor whose zeros would make every eighth result an exact zero, where any bound is "large"
    positive  |wide| with the denormals and zeros replaced by 1: the operands of a sum that ends in ONE number, whose bound (relative to sum |t_i|) says
              nothing about a sum that cancels
    all       bf16: every bit pattern (m * n = 65536, shuffled); f32: meltw_ew_helpers.f32_wide (specials, the sweep of [-12, 12], normal * 2^[-20, 8])
    pairs     meltw_ew_helpers.pair_grid (m = n values of the type crossed with themselves: NaN, infinities, +-0, denormals)
    edges     f32: f32_on_bf16_boundaries, a seeded sample of m * n; bf16: interesting()
    """
    from meltw_ew_helpers import all_bf16, f32_on_bf16_boundaries, f32_wide, interesting, pair_grid
    from meltw_reduce_helpers import wide
    rng = np.random.default_rng(seed)
    if kind in ("wide", "mild", "small", "nonzero", "positive"):
        x = wide(rng, n, m, dt, rows=False)
        if kind == "wide":
            return x
        f = decode(x, dt).astype(np.float32)
        if kind in ("mild", "small"):
            return _as(dt, f * np.float32(2.0 ** (-6 if kind == "mild" else -9)))
        if kind == "nonzero":
            return _as(dt, np.where(np.abs(f) < FLT_MIN, np.float32(1.0), f * np.float32(2.0 ** -6)))
        f = np.abs(f)
        return _as(dt, np.where(f < FLT_MIN, np.float32(1.0), f))
    if kind == "all":
        if dt == DT.BF16:
            assert m * n == 1 << 16
            return rng.permutation(all_bf16()).reshape(n, m)
        return rng.permutation(f32_wide(rng, m * n)).reshape(n, m)
    if kind == "pairs":                      # meltw_ew_helpers.pair_grid: argument seed % 2 of the pair
        assert m == n
        return pair_grid(dt, m)[seed % 2]
    assert kind == "edges"
    if dt == DT.F32:
        return rng.choice(f32_on_bf16_boundaries(), m * n, replace=False).reshape(n, m)
    return rng.permutation(interesting(DT.BF16, m * n)).reshape(n, m)


def values(case, kind, seed):
    """one table per argument (kind: one name, or one per argument)."""
    kinds = [kind] * len(case.shapes) if isinstance(kind, str) else list(kind)
    return [table(kinds[k], dt, m, n, seed * 101 + k) for k, (m, n, ld, dt) in enumerate(case.shapes)]


# ---- the rows -----------------------------------------------------------------------------------------------------------------------------------------------
B16, F32 = DT.BF16, DT.F32
# test_meqn.CASES at their own shapes: (the kernel of a LIBXSMM_HIP_JIT=2 handle, table)
_CASES = {"simple": ("meqn_jit_e", "wide"), "bias_relu_bf16": ("meqn_jit_e", "wide"), "reduce_bcast": ("meqn_jit_r", "wide"), "ternary_muladd": ("meqn_jit_e", "wide"),
          "tanh_sigmoid_chain": ("meqn_jit_e", ("small", "nonzero")), "layernorm_affine": ("meqn_jit_e", "wide"), "matmul_mul": ("meqn_tpp_chain", "mild"),
          "matmul_vnni_bf16": ("meqn_tpp_chain", "mild"), "dot_to_scalar": ("meqn_jit_r", "positive"), "mul_dot_to_scalar": ("meqn_jit_r", "positive"),
          "softmax_fwd": ("meqn_jit_r", "mild"), "softmax_bwd": ("meqn_jit_r", ("positive", "mild")), "sum_of_squares": ("meqn_jit_r", "wide"),
          "matmul_sum_to_scalar": ("meqn_tpp_chain", "positive"), "mixed_precision": ("meqn_jit_e", "wide")}


def _full(m, n, dt, ld=None):
    return (m, n, ld or m, dt)


def rows():
    """name -> (EqCase, table).  Shapes: the smallest at which each rule of csrc/meqn.cpp: generate_fused flips (8-row units, 256 threads, units > 256 * 64,
    M * N <= 2^14, M <= 2048, ld % 8); nothing above 2^17 elements."""
    r = {}
    for name, (expect, tab) in _CASES.items():
        tree, shapes, out = tm.CASES[name]
        r["case_" + name] = (EqCase(tree, shapes, out, expect), tab)
    # element-wise form: one unit; three columns; 264 units (a second block with idle threads)
    for m, n in ((8, 1), (24, 3), (64, 33)):
        r[f"recip_mul_{m}x{n}"] = (EqCase(t_recip_mul(), [_full(m, n, B16, m + 8), _full(m, n, F32)], _full(m, n, F32, m + 16), "meqn_jit_e"), "wide")
        r[f"bias_relu_bf16_{m}x{n}"] = (EqCase(*reshaped("bias_relu_bf16", m, n), "meqn_jit_e"), "wide")
    # MAX / MIN / DIV nodes over the pair grids: NaN, infinities, +-0 ties
    for op, nm in ((BINARY.MAX, "max"), (BINARY.MIN, "min"), (BINARY.DIV, "div")):
        for dt, dn in ((B16, "bf16"), (F32, "f32")):
            r[f"{nm}_pairs_{dn}"] = (EqCase(t_binary(op), [_full(256, 256, dt)] * 2, _full(256, 256, dt, 264), "meqn_jit_e"), "pairs")
    # libm and the correctly rounded functions over every bf16 code / the wide f32 table
    for op, nm in ((UNARY.SQRT, "sqrt"), (UNARY.RECIPROCAL_SQRT, "rsqrt"), (UNARY.EXP, "exp"), (UNARY.TANH, "tanh"), (UNARY.SIGMOID, "sigmoid")):
        r[f"{nm}_all_bf16"] = (EqCase(t_unary(op), [_full(64, 1024, B16)], _full(64, 1024, B16), "meqn_jit_e"), "all")
        r[f"{nm}_all_f32"] = (EqCase(t_unary(op), [_full(64, 1024, F32)], _full(64, 1024, F32), "meqn_jit_e"), "all")
    r["store_edges_bf16_out"] = (EqCase(t_unary(UNARY.IDENTITY), [_full(64, 1024, F32)], _full(64, 1024, B16), "meqn_jit_e"), "edges")
    # row, column and scalar broadcasts
    for dt, dn in ((B16, "bf16"), (F32, "f32")):
        r[f"bcasts_{dn}"] = (EqCase(t_bcasts(), [_full(24, 3, dt, 32), (1, 3, 5, dt), (24, 1, 24, dt), (1, 1, 1, dt)], _full(24, 3, dt, 40), "meqn_jit_e"), "wide")
    # a 1 x 1 head, bf16 and f32
    r["sum_head_bf16"] = (EqCase(t_sum_head(), [_full(64, 12, B16, 72)], (1, 1, 1, B16), "meqn_jit_r"), "positive")
    r["sum_head_f32"] = (EqCase(t_sum_head(), [_full(8, 3, F32)], (1, 1, 1, F32), "meqn_jit_r"), "positive")
    # scalar-reduction phases: 253 idle threads in the fold; threads that own two units; the last fused shape; the first chained one
    for m, n, expect in ((8, 3, "meqn_jit_r"), (64, 40, "meqn_jit_r"), (8, 16384, "meqn_jit_r"), (8, 16385, "meqn_tpp_chain")):
        r[f"softmax_fwd_{m}x{n}"] = (EqCase(*reshaped("softmax_fwd", m, n), expect), "mild")
        r[f"minus_max_{m}x{n}"] = (EqCase(t_minus_max(), [_full(m, n, F32, m + 8)], _full(m, n, F32), expect), "wide")
    # vector-reduction phases: M at its cap with M * N = 2^14; M beyond it; M * N > 2^14 (per-row trees: the chain, folds to one number stay phased)
    for m, n, expect in ((64, 12, "meqn_jit_r"), (2048, 8, "meqn_jit_r"), (2056, 4, "meqn_tpp_chain"), (8, 2049, "meqn_tpp_chain")):
        r[f"col_softmax_{m}x{n}"] = (EqCase(t_col_softmax(), [_full(m, n, B16)], _full(m, n, B16), expect), "mild")
        r[f"reduce_bcast_{m}x{n}"] = (EqCase(*reshaped("reduce_bcast", m, n, m + 8), expect), "wide")
    r["col_softmax_reciprocal_64x12"] = (EqCase(t_col_softmax_reciprocal(), [_full(64, 12, B16)], _full(64, 12, B16), "meqn_tpp_chain"), "mild")
    r["softmax_fwd_8x2049"] = (EqCase(*reshaped("softmax_fwd", 8, 2049), "meqn_jit_r"), "mild")
    # what the code generator declines: M no multiple of 8, an argument / the output at a leading dimension that is none, an op type that is not f32
    s = tm.CASES["simple"][0]
    r["chain_m20"] = (EqCase(s, [_full(20, 3, F32, 24)] * 4, _full(20, 3, F32, 24), "meqn_tpp_chain"), "wide")
    r["chain_arg_ld44"] = (EqCase(s, [_full(40, 3, F32, 48), _full(40, 3, F32, 44), _full(40, 3, F32, 48), _full(40, 3, F32, 48)], _full(40, 3, F32, 48), "meqn_tpp_chain"), "wide")
    r["chain_out_ld44"] = (EqCase(s, [_full(40, 3, F32, 48)] * 4, _full(40, 3, F32, 44), "meqn_tpp_chain"), "wide")
    r["chain_bf16_op"] = (EqCase(t_binary(BINARY.ADD), [_full(40, 3, B16, 48)] * 2, _full(40, 3, B16, 48), "meqn_tpp_chain", comp=B16), "wide")
    return r


# Rows whose guard is taken over a stated part of their table (the check itself covers all of it).  sigmoid is (tanh(x / 2) + 1) / 2: below x = -6 the sum cancels
# to less than K_OP 2^-12 of its terms, so the f32 formula -- the reference's -- has no relative accuracy there and neither has any bound on it.
GUARD_DOMAIN = {"sigmoid_all_f32": ("x >= -6", lambda x: x >= -6.0)}


def guard_share(name, case, bufs, t, e):
    """empty_share of a row, over its GUARD_DOMAIN (a condition on argument 0, element-wise trees only) where it names one."""
    where = None
    if name in GUARD_DOMAIN:
        m, n, ld, dt = case.shapes[0]
        where = GUARD_DOMAIN[name][1](load64(np.asarray(bufs[0])[layout_index(NONE, m, n, ld)], dt))
    return empty_share(t, e, case.odt, where)
