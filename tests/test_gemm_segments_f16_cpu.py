"""IEEE-half (f16) handles in the ten segments entries (include/libxsmm_hip.h) without a GPU, in dry-run mode: F16 x F16 -> f32 and -> f16 handles are accepted by
the four plain entries (A flat and VNNI-2), by the OFFSET entries in the forms NN and NT and by the four ext entries with a column bias, ReLU + bitmask, sigmoid
and without operators (-4: accepted, no device, nothing launched); the two workspace queries count 4-byte accumulators; comp type F16, VNNI_C and a transpose
in an ADDRESS entry are refused with -3 and one error line that names the reason, a missing bias or mask list with -2; an f16 group of a grouped batch still
runs on its own and a group plan still refuses it.  No f16 handle has TRANS_A or VNNI_B -- libxsmm_dispatch_brgemm returns none, as the reference does
(tests/test_dispatch_differential_cpu.py) -- so the forms TN / TT and the refusals of VNNI_B and of VNNI_A with TRANS_A cannot be reached for f16."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import ctypes as C
sys.path.insert(0, %(root)r)
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG, UNARY, UNARY_FLAG
api = capi.load()
def err():
    e = api.hip_get_last_error(); api.hip_clear_last_error(); return e
M, N, K = 40, 24, 20
def sh(c, comp=DT.F32, ta=False, tb=False):
    return capi.gemm_shape(M, N, K, K if ta else M, N if tb else K, M, DT.F16, DT.F16, c, comp)
off, adr = capi.br_config(capi.BR_OFFSET, 0, 0, 0), capi.br_config(capi.BR_ADDRESS, 0, 0, 0)
V, B0, TA, TB, VC = GEMM_FLAG.VNNI_A, GEMM_FLAG.BETA_0, GEMM_FLAG.TRANS_A, GEMM_FLAG.TRANS_B, GEMM_FLAG.VNNI_C
CT = dict(f32=DT.F32, f16=DT.F16)
FORMS = dict(nn=V, nt=TB | B0)
OPS = dict(bias=lambda c: (capi.no_argops(), capi.postops_colbias(M, c)),
           relumask=lambda c: (capi.argops_cp(M, UNARY.RELU, UNARY_FLAG.BITMASK_2BYTEMULT), capi.no_postops()),
           sigmoid=lambda c: (capi.argops_cp(M, UNARY.SIGMOID), capi.postops_colbias(M, c)),
           none=lambda c: (capi.no_argops(), capi.no_postops()))
H = {}
for tag, c in CT.items():
    H["a_vnni_" + tag] = api.dispatch_brgemm(sh(c), V | B0, 0, adr)
    H["a_flat_" + tag] = api.dispatch_brgemm(sh(c), 0, 0, adr)
    for form, fl in FORMS.items():
        H["o_%%s_%%s" %% (form, tag)] = api.dispatch_brgemm(sh(c, ta=bool(fl & TA), tb=bool(fl & TB)), fl, 0, off)
    for op, mk in OPS.items():
        H["e_%%s_%%s" %% (op, tag)] = api.dispatch_brgemm_ext(sh(c), V, 0, adr, *mk(c))
        H["oe_%%s_%%s" %% (op, tag)] = api.dispatch_brgemm_ext(sh(c, tb=True), TB | B0, 0, off, *mk(c))
H.update(
    comp=api.dispatch_brgemm(sh(DT.F16, comp=DT.F16), B0, 0, adr),
    o_comp=api.dispatch_brgemm(sh(DT.F32, comp=DT.F16), 0, 0, off),
    e_comp=api.dispatch_brgemm_ext(sh(DT.F16, comp=DT.F16), 0, 0, adr, *OPS["bias"](DT.F16)),
    vnni_c=api.dispatch_brgemm(sh(DT.F16), V | VC | B0, 0, adr),
    o_vnni_c=api.dispatch_brgemm(sh(DT.F16), VC | B0, 0, off),
    a_tb=api.dispatch_brgemm(sh(DT.F16, tb=True), TB, 0, adr),
    a_tb32=api.dispatch_brgemm(sh(DT.F32, tb=True), V | TB | B0, 0, adr),
    plain=api.dispatch_gemm(sh(DT.F16), B0, 0),
    f32=api.dispatch_gemm(capi.gemm_shape(32, 32, 32, 32, 32, 32, DT.F32, DT.F32, DT.F32, DT.F32), B0, 0),
)
print("handles", ",".join(k for k, v in H.items() if not v) or "all")
# what keeps TN / TT out of reach: dispatch gives no f16 handle with TRANS_A
print("ta_handles", sum(1 for c in CT.values() for fl in (TA, TA | TB, TA | B0) if api.dispatch_brgemm(sh(c, ta=True, tb=bool(fl & TB)), fl, 0, off)))
# never dereferenced on the host: validation reads none of the arrays, none of the bases and not the workspace
BLK, SEG, LA, LB, LC, WS, A, B, CC, DL, LD, LM, MK = (i << 20 for i in range(1, 14))
NS = 5
def call(tag, fn, *args):
    sys.stderr.write("MARK %%s begin\n" %% tag); sys.stderr.flush()
    fn(*args)
    sys.stderr.write("MARK %%s end\n" %% tag); sys.stderr.flush()
    print(tag, err())
def param(offsets, ext=False, bias=True):
    p = capi.GemmExtParam() if ext else capi.GemmParam()
    if offsets:
        p.a.primary, p.b.primary, p.c.primary = A, B, CC
    if ext and offsets:
        p.c.secondary = MK
        if bias:
            p.d.primary = DL
    return p
def plain(tag, h, offsets):
    fn = api.hip_gemm_batch_reduce_segments_offsets if offsets else api.hip_gemm_batch_reduce_segments
    call(tag, fn, h, C.byref(param(offsets)), NS, SEG, LA, LB, LC)
def sliced(tag, h, offsets):
    need = api.hip_gemm_batch_reduce_segments_sliced_workspace(h, NS)
    api.hip_clear_last_error()
    fn = api.hip_gemm_batch_reduce_segments_offsets_sliced if offsets else api.hip_gemm_batch_reduce_segments_sliced
    call(tag, fn, h, C.byref(param(offsets)), 3, BLK, NS, SEG, LA, LB, LC, WS, need or 1 << 19)
def ext(tag, h, offsets, ld=LD, lm=LM, bias=True):
    fn = api.hip_gemm_ext_batch_reduce_segments_offsets if offsets else api.hip_gemm_ext_batch_reduce_segments
    call(tag, fn, h, C.byref(param(offsets, True, bias)), NS, SEG, LA, LB, LC, ld, lm)
def ext_sliced(tag, h, offsets, ld=LD, lm=LM):
    need = api.hip_gemm_ext_batch_reduce_segments_sliced_workspace(h, NS) or 1 << 19        # (a refused handle: 0 -- the call gets room enough)
    api.hip_clear_last_error()
    fn = api.hip_gemm_ext_batch_reduce_segments_offsets_sliced if offsets else api.hip_gemm_ext_batch_reduce_segments_sliced
    call(tag, fn, h, C.byref(param(offsets, True)), 3, BLK, NS, SEG, LA, LB, LC, ld, lm, WS, need)
for tag in CT:
    plain("ok_address_vnni_" + tag, H["a_vnni_" + tag], False)
    plain("ok_address_flat_" + tag, H["a_flat_" + tag], False)
    sliced("ok_sliced_vnni_" + tag, H["a_vnni_" + tag], False)
    sliced("ok_sliced_flat_" + tag, H["a_flat_" + tag], False)
    for form in FORMS:
        plain("ok_offset_%%s_%%s" %% (form, tag), H["o_%%s_%%s" %% (form, tag)], True)
        sliced("ok_offset_sliced_%%s_%%s" %% (form, tag), H["o_%%s_%%s" %% (form, tag)], True)
    for op in OPS:
        ext("ok_ext_%%s_%%s" %% (op, tag), H["e_%%s_%%s" %% (op, tag)], False)
        ext("ok_ext_offset_%%s_%%s" %% (op, tag), H["oe_%%s_%%s" %% (op, tag)], True)
        ext_sliced("ok_ext_sliced_%%s_%%s" %% (op, tag), H["e_%%s_%%s" %% (op, tag)], False)
        ext_sliced("ok_ext_offset_sliced_%%s_%%s" %% (op, tag), H["oe_%%s_%%s" %% (op, tag)], True)
    q = [api.hip_gemm_batch_reduce_segments_sliced_workspace(H[p + tag], n) for p in ("a_vnni_", "a_flat_", "o_nt_") for n in (0, 1, 5, 1000)]
    q += [api.hip_gemm_ext_batch_reduce_segments_sliced_workspace(H[p + tag], n) for p in ("e_bias_", "oe_relumask_", "e_none_") for n in (0, 1, 5, 1000)]
    print("query_" + tag, ",".join(str(x) for x in q), err())
plain("comp", H["comp"], False)
plain("o_comp", H["o_comp"], True)
sliced("s_comp", H["comp"], False)
ext("e_comp", H["e_comp"], False)
plain("vnni_c", H["vnni_c"], False)
plain("o_vnni_c", H["o_vnni_c"], True)
sliced("s_vnni_c", H["vnni_c"], False)
plain("a_tb", H["a_tb"], False)
plain("a_tb32", H["a_tb32"], False)
sliced("s_tb", H["a_tb"], False)
print("query_comp", api.hip_gemm_batch_reduce_segments_sliced_workspace(H["comp"], 5), err())
ext("no_bias", H["e_bias_f16"], False, ld=None)                 # neither d_list nor param->d.primary
ext("o_no_bias", H["oe_bias_f32"], True, bias=False)            # the base d_offs is added to
ext("no_mask", H["e_relumask_f32"], False, lm=None)
ext("o_no_mask", H["oe_relumask_f16"], True, lm=None)
ext_sliced("s_no_mask", H["e_relumask_f16"], False, lm=None)
# grouped batches: an f16 group runs as its own strided launch (accepted: -4), a plan does not take it
def grp(h):
    g = capi.GemmGroup()
    g.kernel = h; g.count = 4; g.stride_a, g.stride_b, g.stride_c = 1 << 16, 1 << 16, 1 << 16
    g.param.a.primary, g.param.b.primary, g.param.c.primary = 1 << 20, 2 << 20, 3 << 20
    return g
arr = (capi.GemmGroup * 2)(grp(H["f32"]), grp(H["plain"]))
call("grouped", api.hip_gemm_batch_grouped, arr, 2)
sys.stderr.write("MARK plan begin\n"); sys.stderr.flush()
p = api.hip_gemm_group_plan_create(arr, 2)
sys.stderr.write("MARK plan end\n"); sys.stderr.flush()
print("plan", "%%s/%%d" %% ("null" if not p else "plan", err()))
print("launches", api.hip_launch_count(0))
"""

CT = ("f32", "f16")
FORMS = ("nn", "nt")
OPS = ("bias", "relumask", "sigmoid", "none")
PLAIN = ["ok_%s_%s_%s" % (e, a, c) for e in ("address", "sliced") for a in ("vnni", "flat") for c in CT]
OFFSET = ["ok_%s_%s_%s" % (e, f, c) for e in ("offset", "offset_sliced") for f in FORMS for c in CT]
EXT = ["ok_%s_%s_%s" % (e, o, c) for e in ("ext", "ext_offset", "ext_sliced", "ext_offset_sliced") for o in OPS for c in CT]
COMP = "comp type F16 is not taken (the running sum is rounded to a half after every product"
REFUSED = {"comp": COMP, "o_comp": COMP, "s_comp": COMP, "e_comp": COMP,
           "vnni_c": "VNNI layouts of B and C are not taken", "o_vnni_c": "VNNI layouts of B and C are not taken", "s_vnni_c": "VNNI layouts of B and C are not taken",
           "a_tb": "transposed operands are not taken (NN only)", "a_tb32": "transposed operands are not taken (NN only)", "s_tb": "transposed operands are not taken (NN only)"}
MISSING = {"no_bias": "d_list and param->d.primary are both NULL", "o_no_bias": "param->d.primary", "no_mask": "mask_list is NULL", "o_no_mask": "mask_offs is NULL",
           "s_no_mask": "mask_list is NULL"}
M, N = 40, 24


@pytest.fixture(scope="module")
def child():
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1")
    env.pop("LIBXSMM_VERBOSE", None)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _codes(child):
    return dict(ln.split() for ln in child.stdout.splitlines() if len(ln.split()) == 2 and not ln.startswith("query_"))


def _errors(child, tag):
    err = child.stderr.split(f"MARK {tag} begin\n")[1].split(f"MARK {tag} end\n")[0]
    return err, [ln for ln in err.splitlines() if "ERROR" in ln]


def test_every_handle_is_dispatched(child):
    got = _codes(child)
    assert got["handles"] == "all" and got["ta_handles"] == "0", child.stdout


@pytest.mark.parametrize("tags", [PLAIN, OFFSET, EXT], ids=["plain-vnni-and-flat", "offset-nn-nt", "ext-bias-relumask-sigmoid-none"])
def test_f16_handles_are_accepted(child, tags):
    """F16 -> f32 and F16 -> f16 end with -4: accepted, then no device, and only that is printed.  (Without the feature: -3, "operand types".)"""
    got = _codes(child)
    for tag in tags:
        assert got[tag] == "-4", (tag, child.stdout + child.stderr)
        err, lines = _errors(child, tag)
        assert len(lines) == 1 and "no HIP device" in lines[0], (tag, err)
    assert got["launches"] == "0"


def test_refusals_are_minus_three_with_one_error_that_names_the_reason(child):
    got = _codes(child)
    for tag, words in REFUSED.items():
        assert got[tag] == "-3", (tag, child.stdout)
        err, lines = _errors(child, tag)
        assert len(lines) == 1 and words in lines[0] and "no HIP device" not in err, (tag, err)
    assert "which only the dense generic kernel does" in _errors(child, "comp")[1][0]


def test_a_missing_bias_or_mask_list_is_minus_two(child):
    got = _codes(child)
    for tag, words in MISSING.items():
        assert got[tag] == "-2", (tag, child.stdout)
        err, lines = _errors(child, tag)
        assert len(lines) == 1 and words in lines[0] and "no HIP device" not in err, (tag, err)


def test_the_workspace_queries_count_four_byte_accumulators(child):
    out = dict(ln.split(None, 1) for ln in child.stdout.splitlines() if ln.startswith("query_"))
    for c in CT:
        sizes, code = out["query_" + c].split()
        assert code == "0"
        sizes = [int(x) for x in sizes.split(",")]
        assert len(sizes) == 24
        for ns, got in zip((0, 1, 5, 1000) * 6, sizes):
            assert got % 16 == 0 and ns * M * N * 4 <= got <= ns * (M * N * 4 + 15) and (got == 0) == (ns == 0), (c, ns, got)
    assert out["query_comp"].split() == ["0", "-3"]


def test_an_f16_group_still_runs_on_its_own_and_a_plan_still_refuses_it(child):
    got = _codes(child)
    assert got["grouped"] == "-4" and got["plan"] == "null/-3", child.stdout
    err, lines = _errors(child, "grouped")
    assert len(lines) == 1 and "no HIP device" in lines[0], err
    err, lines = _errors(child, "plan")
    assert len(lines) == 1 and "cannot enter the grouped kernels" in lines[0], err
