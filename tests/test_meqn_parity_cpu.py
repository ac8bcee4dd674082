"""Matrix-equation parity without a GPU (tests/meqn_parity_helpers.py): the float64 bound against the oracle composition and the reference's own evaluator, the
generated kernels executed on the host over the full-range tables, and what the new check rejects that the older one accepted."""
import numpy as np
import pytest

import meqn_parity_helpers as mp
from helpers import normf_rel
from libxsmm_amd.capi import BINARY, DT, UNARY
from meltw_ew_helpers import decode

ROWS = mp.rows()


def _data(case, tab, seed):
    return case.pack(mp.values(case, tab, seed))


@pytest.mark.parametrize("name", sorted(ROWS))
def test_oracle_composition_lies_inside_the_ref64_bound(name):
    """Every row of the GPU table, both data sets: the oracle composition is inside the bound on every element, and the bound says something on at least 90 %
    of the finite, normal results (meqn_parity_helpers.empty_share; sigmoid_all_f32 takes the share over x >= -6, see GUARD_DOMAIN)."""
    case, tab = ROWS[name]
    for seed in (1, 2):
        bufs = _data(case, tab, seed)
        t, e = case.ref64(bufs)
        got = decode(case.oracle(bufs), case.odt)
        ratio, ok = mp.ref64_ratio(got, t, e, case.odt)
        share = mp.guard_share(name, case, bufs, t, e)
        print(f"{name} seed {seed}: worst err / bound {ratio.max():.3f}, empty share {share:.3f}")
        mp.assert_ref64(got, t, e, case.odt, what=name)
        assert share <= mp.MAX_EMPTY, (name, share)


REF_ROWS = [n for n in sorted(ROWS) if not mp.traits(ROWS[n][0].tree, ROWS[n][0].shapes)["mm"] and ROWS[n][0].comp == DT.F32]
REF_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import meqn_parity_helpers as mp
import test_meqn as tm
from libxsmm_amd import capi
from oracle import pyoracle
ref = pyoracle.reference()
ref.lib.xref_set_target_arch(b"generic")
rows = mp.rows()
for name in %(names)r:
    case, tab = rows[name]
    h = ref.dispatch_meqn(tm.build(ref, case.tree, case.shapes), capi.MeqnArgShape(*case.out_shape))
    if not h:
        print(json.dumps({"row": name, "result": "declined"}), flush=True)
        continue
    bufs = case.pack(mp.values(case, tab, 1))
    held = [b.copy() for b in bufs]
    theirs = case.new_out()
    tm._call(ref, h, [a.ctypes.data for a in held], theirs.ctypes.data)
    try:
        case.check(theirs, "ref64" if mp.traits(case.tree, case.shapes)["libm"] else "same_bits", case.oracle(bufs), bufs=bufs, what=name)
        print(json.dumps({"row": name, "result": "ok"}), flush=True)
    except AssertionError as e:
        print(json.dumps({"row": name, "result": str(e)[:600]}), flush=True)
"""


@pytest.fixture(scope="module")
def reference_results(reference):
    """One child process for all rows: the reference's target is process-wide state.  With the target `generic` its JIT declines every equation and
    libxsmm_dispatch_meqn hands out the reference's own evaluator (src/generator_matequation_reference_impl.c) -- the code the oracle composition restates.
    (On the host's own target the handle is the CPU JIT: polynomial tanh / exp, Newton reciprocals, fused multiply-adds, its own order of sums, no denormal
    flush -- an implementation of its own, which tests/test_meqn.py holds to a matrix norm.)"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", REF_CHILD % {"root": root, "tests": os.path.join(root, "tests"), "names": REF_ROWS}], capture_output=True, text=True, timeout=900)
    out = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("{"):
            d = json.loads(ln)
            out[d["row"]] = d["result"]
    assert r.returncode == 0 and len(out) == len(REF_ROWS), r.stdout[-2000:] + r.stderr[-2000:]
    return out


@pytest.mark.parametrize("name", REF_ROWS)
def test_oracle_composition_matches_the_reference_evaluator_over_the_full_range(reference_results, name):
    """The oracle composition against the reference's own libxsmm_dispatch_meqn on the same full-range bytes, poisoned padding included: the same bits for
    trees without libm, the ref64 bound otherwise.  (MATMUL nodes are left out: the reference's evaluator prints `Invalid OP` for them and exits.)"""
    if reference_results[name] == "declined":
        pytest.skip("the reference declines this equation on this host")
    assert reference_results[name] == "ok", reference_results[name]


# the generated kernels on the host: form x types, the full-range tables
EMULATED = ["recip_mul_24x3", "bias_relu_bf16_24x3", "bcasts_bf16", "bcasts_f32", "case_mixed_precision", "case_tanh_sigmoid_chain", "case_layernorm_affine",     # _e
            "softmax_fwd_8x3", "softmax_fwd_64x40", "minus_max_64x40", "sum_head_bf16", "case_softmax_bwd", "case_dot_to_scalar",                                # _r, scalar phases
            "col_softmax_64x12", "reduce_bcast_64x12", "case_reduce_bcast"]                                                                                      # _r, vector phases


@pytest.mark.parametrize("name", EMULATED)
def test_generated_kernel_on_the_host_matches_per_element(tmp_path, name):
    """The text hiprtc compiles, built for the host (tests/test_jit_emulated_cpu.py), fed the full-range tables with poisoned padding.  The oracle composition
    stands in for the chain (it is the chain's bits wherever the rule is same_bits; host libm on both sides).  Before the generated loads flushed bf16
    denormals, recip_mul_24x3 failed here: RECIPROCAL of the codes 0x0040 / 0x007f / 0x8040 gave 1.70e38 / 8.57e37 / -1.70e38 where the chain gives +-inf."""
    case, tab = ROWS[name]
    kernel, launch = mp.emulate(tmp_path, case)
    stats = {}
    for seed in (1, 2):
        vals = mp.values(case, tab, seed)
        if name == "recip_mul_24x3":
            vals[0][0, :3] = [0x0040, 0x007f, 0x8040]
        bufs = case.pack(vals)
        out = launch(bufs)
        case.check(out, mp.fused_rule(case.tree, case.shapes), case.oracle(bufs), bufs=bufs, what=f"{name} ({kernel}) seed {seed}", stats=stats)
    print(f"{name} ({kernel}): rule {mp.fused_rule(case.tree, case.shapes)}, worst err / bound {stats.get('ratio', 0.0):.3f}")


def _f32(codes):
    return (np.asarray(codes).astype(np.uint32) << 16).view(np.float32)


def _tanh(x):
    return np.tanh(x.astype(np.float64)).astype(np.float32)


def _out_of(case, bufs):
    out = case.new_out()
    out[case.out_idx] = case.oracle(bufs)
    return out


def _accepts(check):
    try:
        check()
    except AssertionError:
        return False
    return True


def test_the_new_check_rejects_what_the_old_bar_accepted():
    """Seven errors injected into an otherwise correct result; per injection (new check accepts, old bar accepts).  The new check (padding untouched, same_bits
    against the chain, ref64 against the float64 walk) rejects all seven.  The old bar -- normf_rel(_valid) < BY_NORM for a tree with libm or a sum,
    array_equal(_valid) otherwise -- ACCEPTS 3 of the 7: the element 4 ulp off, the one element of the last column, the write into the padding.  (It rejects
    the unflushed denormal only because it cannot take a result that holds an infinity at all: NaN < bound is false for the correct result too.)"""
    tree = ("b", BINARY.ADD, mp.BF.BCAST_ROW_IN_1, ("b", BINARY.MUL, 0, mp.t_recip_mul(), ("u", UNARY.TANH, 0, mp.A(2))), mp.A(3))   # RECIPROCAL(a0) * a1 * tanh(a2) + row(a3)
    m, n = 24, 3
    case = mp.EqCase(tree, [(m, n, 32, DT.BF16), (m, n, m, DT.F32), (m, n, m, DT.F32), (1, n, 5, DT.F32)], (m, n, 40, DT.F32), "meqn_jit_e")
    kinds = ["wide", "mild", "mild", "mild"]
    smax = mp.EqCase(mp.t_minus_max(), [(8, 3, 16, DT.F32)], (8, 3, 8, DT.F32), "meqn_jit_r")           # x - max x: the tree with a scalar MAX phase

    def correct(c, vals):
        bufs = c.pack(vals)
        out = c.new_out()
        out[c.out_idx] = c.oracle(bufs)
        return bufs, out, c.ref64(bufs)

    def verdict(c, good, te, out, libm):
        new = _accepts(lambda: (c.check(out, "same_bits", c.logical(good)), c.check(out, "ref64", None, te=te)))
        with np.errstate(all="ignore"):
            old = bool(normf_rel(c.logical(good), c.logical(out), DT.F32) < 1e-6) if libm else bool(np.array_equal(c.logical(out), c.logical(good)))
        return new, old

    vals = mp.values(case, kinds, 5)
    with_denormals = [v.copy() for v in vals]
    with_denormals[0][1, :3] = [0x0040, 0x007f, 0x8040]
    vals[0] = np.where((vals[0] & 0x7f80) == 0, np.uint16(0x3f80), vals[0])          # five injections on data whose results are all finite, as the old bar needs them
    bufs, good, te = correct(case, vals)
    assert np.isfinite(case.logical(good)).all() and verdict(case, good, te, good, True) == (True, True)
    seen = {}
    x = good.copy(); k = case.out_idx[n - 1, m - 3]; x[k] = (x[k:k + 1].view(np.uint32) + 4).view(np.float32)[0]
    seen["4 ulp in the last 8-row unit"] = verdict(case, good, te, x, True)
    x = good.copy(); k = case.out_idx[n - 1, 5]; x[k] = np.float32(x[k] * np.float32(1 + 2.0 ** -12))
    seen["one element of the last column off"] = verdict(case, good, te, x, True)
    x = good.copy(); x[case.out_idx[1, m - 1] + 1] = 1.0
    seen["one padding element written"] = verdict(case, good, te, x, True)
    b2 = [b.copy() for b in bufs]
    b2[3][np.arange(n) * 5] = bufs[3][np.arange(n) * 1]                                # what a read at j * m (m = 1) instead of j * ld finds
    seen["a broadcast row read at j * m"] = verdict(case, good, te, _out_of(case, b2), True)
    seen["the output of the previous call"] = verdict(case, good, te, correct(case, mp.values(case, kinds, 6))[1], True)
    bufs_d, good_d, te_d = correct(case, with_denormals)                               # data with bf16 denormals: the correct result holds infinities
    assert verdict(case, good_d, te_d, good_d, True) == (True, False)
    with np.errstate(all="ignore"):                                                     # no flush: a bare shift
        wrong = (np.float32(1.0) / _f32(with_denormals[0]) * vals[1]).astype(np.float32) * _tanh(vals[2]) + vals[3].reshape(n, 1)
    x = good_d.copy(); den = (with_denormals[0] & 0x7f80) == 0
    x[case.out_idx[den]] = wrong.astype(np.float32)[den]
    seen["a bf16 denormal argument not flushed"] = verdict(case, good_d, te_d, x, True)
    neg = -np.abs(mp.table("positive", DT.F32, 8, 3, 9))                               # all negative: a MAX that starts at 0 stays 0
    sbufs, sgood, ste = correct(smax, [neg])
    x = smax.new_out(); x[smax.out_idx] = neg - np.float32(0.0)
    assert verdict(smax, sgood, ste, sgood, False) == (True, True)
    seen["a scalar MAX started at 0"] = verdict(smax, sgood, ste, x, False)
    print({k: {"new accepts": v[0], "old accepts": v[1]} for k, v in seen.items()})
    assert len(seen) == 7 and not any(new for new, _ in seen.values()), seen
    assert sorted(k for k, (_, old) in seen.items() if old) == sorted(["4 ulp in the last 8-row unit", "one element of the last column off", "one padding element written"])

