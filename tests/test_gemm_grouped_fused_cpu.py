"""libxsmm_hip_gemm_ext_batch_grouped and the group plans without a GPU: the C layout of libxsmm_hip_gemm_ext_group against its ctypes mirror, every refusal of
the entry and of the plan functions in dry-run mode (every group is validated before anything is launched or built, so the documented codes come before the
missing device is noticed), and the mask condition of the GPU file met by the oracle alone on the inputs that file uses."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import grouped_fused_helpers as gf
from libxsmm_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("kernel", "param", "count", "stride_a", "stride_b", "stride_c", "stride_d", "stride_mask")

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include <libxsmm.h>
int main(void) {
  printf("size %zu\n", sizeof(libxsmm_hip_gemm_ext_group));
BODY
  return 0;
}
"""


def test_ext_group_struct_layout_matches_the_ctypes_mirror(tmp_path):
    body = "\n".join(f'  printf("{f} %zu %zu\\n", offsetof(libxsmm_hip_gemm_ext_group, {f}), sizeof(((libxsmm_hip_gemm_ext_group*)0)->{f}));' for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C.replace("BODY", body))
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.strip()}
    want = {"size": (C.sizeof(capi.GemmExtGroup),)}
    for f in FIELDS:
        want[f] = (getattr(capi.GemmExtGroup, f).offset, getattr(capi.GemmExtGroup, f).size)
    assert got == want


VALIDATION_CHILD = r"""
import sys
import ctypes as C
sys.path.insert(0, %(root)r)
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG, UNARY, UNARY_FLAG
api = capi.load()
def err():
    e = api.hip_get_last_error(); api.hip_clear_last_error(); return e
sh = lambda m, t=DT.F32, c=DT.F32: capi.gemm_shape(m, m, m, m, m, m, t, t, c, DT.F32)
nobr = capi.br_config()
stride = capi.br_config(capi.BR_STRIDE, 24 * 24 * 4, 24 * 24 * 4, 0)
relu = api.dispatch_brgemm_ext(sh(32), GEMM_FLAG.BETA_0, 0, nobr, capi.argops_cp(32, UNARY.RELU), capi.no_postops())
bias = api.dispatch_brgemm_ext(sh(16), 0, 0, nobr, capi.no_argops(), capi.postops_colbias(16, DT.F32))
bitm = api.dispatch_brgemm_ext(sh(16, DT.BF16, DT.BF16), GEMM_FLAG.VNNI_A, 0, nobr, capi.argops_cp(16, UNARY.RELU, UNARY_FLAG.BITMASK_2BYTEMULT), capi.postops_colbias(16, DT.BF16))
noop = api.dispatch_brgemm_ext(sh(20), 0, 0, nobr, capi.no_argops(), capi.no_postops())
brx = api.dispatch_brgemm_ext(sh(24), 0, 0, stride, capi.argops_cp(24, UNARY.SIGMOID), capi.no_postops())
f64x = api.dispatch_brgemm_ext(capi.gemm_shape(8, 8, 8, 8, 8, 8, DT.F64, DT.F64, DT.F64, DT.F64), 0, 0, nobr, capi.no_argops(), capi.no_postops())
tax = api.dispatch_brgemm_ext(sh(20), GEMM_FLAG.TRANS_A, 0, nobr, capi.argops_cp(20, UNARY.RELU), capi.no_postops())
plain = api.dispatch_gemm(sh(32), GEMM_FLAG.BETA_0, 0)
plain2 = api.dispatch_gemm(sh(16, DT.BF16, DT.BF16), GEMM_FLAG.VNNI_A, 0)
plain3 = api.dispatch_gemm(sh(16), 0, 0)
pta = api.dispatch_gemm(sh(20), GEMM_FLAG.TRANS_A, 0)
pbr = api.dispatch_brgemm(sh(24), 0, 0, stride)
tpp = api.dispatch_meltw_unary(UNARY.IDENTITY, capi.UnaryShape(16, 16, 16, 16, DT.F32, DT.F32, DT.F32), 0)
assert relu and bias and bitm and noop and brx and f64x and tax and plain and plain2 and plain3 and pta and pbr and tpp
cnt = C.c_ulonglong(3)
def grp(h, count=4, brc=True, d=True, mask=True, cls=capi.GemmExtGroup):
    g = cls()
    g.kernel = h; g.count = count; g.stride_a, g.stride_b, g.stride_c = 1 << 16, 1 << 16, 1 << 16
    g.param.a.primary, g.param.b.primary, g.param.c.primary = 1 << 20, 2 << 20, 3 << 20
    if cls is capi.GemmExtGroup:
        g.stride_d, g.stride_mask = 64, 1 << 10
        if d:
            g.param.d.primary = 4 << 20
        if mask:
            g.param.c.secondary = 5 << 20
    if brc:
        g.param.op.tertiary = C.addressof(cnt)
    return g
pg = lambda h, **kw: grp(h, cls=capi.GemmGroup, **kw)
def run(*gs, n=None):
    arr = (capi.GemmExtGroup * max(len(gs), 1))(*gs)
    api.hip_gemm_ext_batch_grouped(arr, len(gs) if n is None else n)
    return err()
def plan(*gs, cls=capi.GemmExtGroup):
    arr = (cls * max(len(gs), 1))(*gs)
    p = (api.hip_gemm_ext_group_plan_create if cls is capi.GemmExtGroup else api.hip_gemm_group_plan_create)(arr, len(gs))
    return "%%s/%%d" %% ("null" if not p else "plan", err())
api.hip_gemm_ext_batch_grouped(None, 3); print("null_list", err())
api.hip_gemm_ext_batch_grouped(None, 0); print("null_empty", err())
print("ngroups0", run(grp(relu), n=0))
print("all_count0", run(grp(relu, 0), grp(brx, 0), grp(bitm, 0)))
print("br_no_count", run(grp(relu), grp(brx, brc=False)))
print("bias_no_d", run(grp(relu), grp(bias, d=False)))
print("bitmask_no_mask", run(grp(relu), grp(bitm, mask=False)))
print("unknown", run(grp(relu), grp(12345)))
print("plain", run(grp(relu), grp(plain)))
print("tpp", run(grp(relu), grp(tpp)))
sys.stderr.write("MARK plain_msg begin\n"); sys.stderr.flush()
run(grp(plain))
sys.stderr.write("MARK plain_msg end\n"); sys.stderr.flush()
sys.stderr.write("MARK late_refusal begin\n"); sys.stderr.flush()
print("late_refusal", run(grp(relu), grp(bias), grp(bitm), grp(noop), grp(brx), grp(f64x), grp(tax), grp(plain)))
sys.stderr.write("MARK late_refusal end\n"); sys.stderr.flush()
print("valid", run(grp(relu), grp(bias), grp(bitm), grp(noop), grp(brx), grp(f64x), grp(tax)))
print("valid_one", run(grp(relu)))
# plans: the entry's codes, then the refusal of groups that cannot enter the grouped kernels, then the missing device
api.hip_gemm_ext_group_plan_create(None, 2); print("plan_null_list", err())
api.hip_gemm_group_plan_create(None, 2); print("plain_plan_null_list", err())
print("plan_br_no_count", plan(grp(relu), grp(brx, brc=False)))
print("plan_bias_no_d", plan(grp(relu), grp(bias, d=False)))
print("plan_unknown", plan(grp(relu), grp(12345)))
print("plan_plain_handle", plan(grp(relu), grp(plain)))
print("plain_plan_ext_handle", plan(pg(plain), pg(relu), cls=capi.GemmGroup))
print("plain_plan_tpp", plan(pg(plain), pg(tpp), cls=capi.GemmGroup))
print("plain_plan_br_no_count", plan(pg(plain), pg(pbr, brc=False), cls=capi.GemmGroup))
sys.stderr.write("MARK plan_trans begin\n"); sys.stderr.flush()
print("plan_trans_a", plan(grp(relu), grp(bias), grp(tax)))
sys.stderr.write("MARK plan_trans end\n"); sys.stderr.flush()
print("plain_plan_trans_a", plan(pg(plain), pg(plain3), pg(pta), cls=capi.GemmGroup))
print("plan_f64", plan(grp(relu), grp(f64x)))
print("plan_valid", plan(grp(relu), grp(bias), grp(bitm), grp(noop), grp(brx)))
print("plain_plan_valid", plan(pg(plain), pg(plain2), pg(plain3), pg(pbr), cls=capi.GemmGroup))
api.hip_gemm_group_plan_launch(None); print("launch_null", err())
print("launches_null", api.hip_gemm_group_plan_launches(None), err())
api.hip_gemm_group_plan_destroy(None); print("destroy_null", err())
print("launches", api.hip_launch_count(0))
"""


def test_ext_grouped_entry_and_plan_refusals_set_the_documented_error_codes(tmp_path):
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1")
    env.pop("LIBXSMM_VERBOSE", None)
    r = subprocess.run([sys.executable, "-c", VALIDATION_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(ln.split(None, 1) for ln in r.stdout.splitlines() if len(ln.split()) >= 2)
    assert got == {"null_list": "-2",                                    # groups == NULL with ngroups > 0
                   "null_empty": "0", "ngroups0": "0", "all_count0": "0",     # nothing to do
                   "br_no_count": "-2", "bias_no_d": "-2", "bitmask_no_mask": "-2",
                   "unknown": "-3", "plain": "-3", "tpp": "-3",
                   "late_refusal": "-3",                                 # the last group is refused ...
                   "valid": "-4", "valid_one": "-4",                     # accepted (fallback groups included); then: no device
                   "plan_null_list": "-2", "plain_plan_null_list": "-2",
                   "plan_br_no_count": "null/-2", "plan_bias_no_d": "null/-2", "plan_unknown": "null/-3", "plan_plain_handle": "null/-3",
                   "plain_plan_ext_handle": "null/-3", "plain_plan_tpp": "null/-3", "plain_plan_br_no_count": "null/-2",
                   "plan_trans_a": "null/-3", "plain_plan_trans_a": "null/-3", "plan_f64": "null/-3",      # accepted by the call, refused by a plan
                   "plan_valid": "null/-4", "plain_plan_valid": "null/-4",                                  # validated; then: no device
                   "launch_null": "-2", "launches_null": "0 -2", "destroy_null": "0",
                   "launches": "0"}, r.stdout + r.stderr
    # a plain handle is pointed to the plain entry
    msg = r.stderr.split("MARK plain_msg begin\n")[1].split("MARK plain_msg end\n")[0]
    assert "libxsmm_hip_gemm_batch_grouped" in msg, msg
    # ... and nothing before the late refusal was attempted: every error is printed (set_error), and the only one of that call is the refusal -- a call that
    # launched group by group would have met the missing device first
    late = r.stderr.split("MARK late_refusal begin\n")[1].split("MARK late_refusal end\n")[0]
    lines = [ln for ln in late.splitlines() if "ERROR" in ln]
    assert len(lines) == 1 and "group 7" in lines[0] and "not an ext kernel" in lines[0] and "no HIP device" not in late, late
    # the plan's refusal names the group
    trans = r.stderr.split("MARK plan_trans begin\n")[1].split("MARK plan_trans end\n")[0]
    lines = [ln for ln in trans.splitlines() if "ERROR" in ln]
    assert len(lines) == 1 and "group 2" in lines[0] and "plan" in lines[0], trans


def test_the_oracle_alone_meets_the_mask_condition_on_the_random_bf16_inputs():
    """The GPU file compares mask bits only where the float64 bound decides them and allows at most half of them to be undecided: the oracle itself, on
    the same random inputs, meets both halves of that condition."""
    for case in gf.bf16_cases():
        _, mask = case.run_oracle()
        decided, positive = gf.decided_mask_bits(case)
        assert decided.mean() >= 0.5, (case.m, case.n, case.k, float(decided.mean()))
        bits = case.valid_mask_bits(mask)
        assert np.array_equal(bits[decided], positive[decided].astype(bits.dtype)), (case.m, case.n, case.k)
