"""libxsmm_hip_gemm_batch_grouped without a GPU: the C layout of libxsmm_hip_gemm_group against its ctypes mirror, and the refusals of the entry point in
dry-run mode -- every group is validated before anything is launched, so the documented codes come before the missing device is noticed."""
import ctypes as C
import os
import subprocess
import sys

from libxsmm_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("kernel", "param", "count", "stride_a", "stride_b", "stride_c")

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include <libxsmm.h>
int main(void) {
  printf("size %zu\n", sizeof(libxsmm_hip_gemm_group));
BODY
  return 0;
}
"""


def test_group_struct_layout_matches_the_ctypes_mirror(tmp_path):
    body = "\n".join(f'  printf("{f} %zu %zu\\n", offsetof(libxsmm_hip_gemm_group, {f}), sizeof(((libxsmm_hip_gemm_group*)0)->{f}));' for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C.replace("BODY", body))
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.strip()}
    want = {"size": (C.sizeof(capi.GemmGroup),)}
    for f in FIELDS:
        want[f] = (getattr(capi.GemmGroup, f).offset, getattr(capi.GemmGroup, f).size)
    assert got == want


VALIDATION_CHILD = r"""
import sys
import ctypes as C
sys.path.insert(0, %(root)r)
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG, UNARY
api = capi.load()
def err():
    e = api.hip_get_last_error(); api.hip_clear_last_error(); return e
sh = lambda m, t=DT.F32, c=DT.F32: capi.gemm_shape(m, m, m, m, m, m, t, t, c, DT.F32)
f32 = api.dispatch_gemm(sh(32), GEMM_FLAG.BETA_0, 0)
bf16 = api.dispatch_gemm(sh(16, DT.BF16, DT.BF16), GEMM_FLAG.VNNI_A, 0)
f64 = api.dispatch_gemm(capi.gemm_shape(8, 8, 8, 8, 8, 8, DT.F64, DT.F64, DT.F64, DT.F64), 0, 0)
br = api.dispatch_brgemm(sh(24), 0, 0, capi.br_config(capi.BR_STRIDE, 24 * 24 * 4, 24 * 24 * 4, 0))
ext = api.dispatch_brgemm_ext(sh(32), 0, 0, capi.br_config(), capi.argops_cp(32, UNARY.RELU), capi.no_postops())
tpp = api.dispatch_meltw_unary(UNARY.IDENTITY, capi.UnaryShape(16, 16, 16, 16, DT.F32, DT.F32, DT.F32), 0)
assert f32 and bf16 and f64 and br and ext and tpp
cnt = C.c_ulonglong(3)
def grp(h, count=4, brc=True):
    g = capi.GemmGroup()
    g.kernel = h; g.count = count; g.stride_a, g.stride_b, g.stride_c = 1 << 16, 1 << 16, 1 << 16
    g.param.a.primary, g.param.b.primary, g.param.c.primary = 1 << 20, 2 << 20, 3 << 20
    if brc:
        g.param.op.tertiary = C.addressof(cnt)
    return g
def run(*gs, n=None):
    arr = (capi.GemmGroup * max(len(gs), 1))(*gs)
    api.hip_gemm_batch_grouped(arr, len(gs) if n is None else n)
    return err()
api.hip_gemm_batch_grouped(None, 3); print("null_list", err())
api.hip_gemm_batch_grouped(None, 0); print("null_empty", err())
print("ngroups0", run(grp(f32), n=0))
print("all_count0", run(grp(f32, 0), grp(br, 0), grp(bf16, 0)))
print("br_no_count", run(grp(f32), grp(br, brc=False)))
print("unknown", run(grp(f32), grp(12345)))
print("tpp", run(grp(f32), grp(tpp)))
print("ext", run(grp(f32), grp(ext)))
sys.stderr.write("MARK late_refusal begin\n"); sys.stderr.flush()
print("late_refusal", run(grp(f32), grp(bf16), grp(br), grp(f64), grp(ext)))
sys.stderr.write("MARK late_refusal end\n"); sys.stderr.flush()
# the order of the checks: the first offending group decides, whatever follows it
def msg():
    m = api.hip_get_last_error_string().decode(); return m.replace("\n", " ")
api.hip_gemm_batch_grouped((capi.GemmGroup * 3)(grp(f32), grp(12345), grp(br, brc=False)), 3); print("MSG order_unknown_first", msg()); print("order_unknown_first", err())
api.hip_gemm_batch_grouped((capi.GemmGroup * 3)(grp(f32), grp(br, brc=False), grp(12345)), 3); print("MSG order_br_first", msg()); print("order_br_first", err())
# an ext handle: the entry names the ext strided entry, the plain plan the ext form of its own call
api.hip_gemm_batch_grouped((capi.GemmGroup * 2)(grp(f32), grp(ext)), 2); print("MSG entry_ext", msg()); err()
p = api.hip_gemm_group_plan_create((capi.GemmGroup * 2)(grp(f32), grp(ext)), 2); print("MSG plan_ext", msg()); print("plan_ext", "%%s/%%d" %% ("null" if not p else "plan", err()))
print("valid", run(grp(f32), grp(bf16), grp(br), grp(f64)))
print("valid_one", run(grp(f32)))
print("launches", api.hip_launch_count(0))
"""


def test_grouped_entry_refusals_set_the_documented_error_codes(tmp_path):
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1")
    env.pop("LIBXSMM_VERBOSE", None)
    r = subprocess.run([sys.executable, "-c", VALIDATION_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(ln.split() for ln in r.stdout.splitlines() if len(ln.split()) == 2)
    assert got == {"null_list": "-2",            # groups == NULL with ngroups > 0
                   "null_empty": "0", "ngroups0": "0", "all_count0": "0",     # nothing to do
                   "br_no_count": "-2",          # a BRGEMM handle without op.tertiary
                   "unknown": "-3", "tpp": "-3", "ext": "-3",
                   "late_refusal": "-3",         # the last group is refused ...
                   "order_unknown_first": "-3", "order_br_first": "-2", "plan_ext": "null/-3",
                   "valid": "-4", "valid_one": "-4",       # accepted; then: no device
                   "launches": "0"}, r.stdout + r.stderr
    # ... and nothing before it was attempted: every error is printed (set_error), and the only one of that call is the refusal -- a call that launched group
    # by group would have met the missing device first
    err = r.stderr.split("MARK late_refusal begin\n")[1].split("MARK late_refusal end\n")[0]
    lines = [ln for ln in err.splitlines() if "ERROR" in ln]
    assert len(lines) == 1 and "ext handles" in lines[0] and "no HIP device" not in err, err

    # the first offending group is the one named, with its own code: unknown handle before a missing count, and the other way round
    msgs = {ln.split()[1]: ln.split(None, 2)[2] for ln in r.stdout.splitlines() if ln.startswith("MSG ") and len(ln.split()) > 2}
    assert "group 1" in msgs["order_unknown_first"] and "unknown kernel handle" in msgs["order_unknown_first"], msgs
    assert "group 1" in msgs["order_br_first"] and "op.tertiary" in msgs["order_br_first"], msgs
    # the two wordings of the ext-handle refusal, each with its own pointer
    assert "ext handles are not taken" in msgs["entry_ext"] and "libxsmm_hip_gemm_ext_batch_strided" in msgs["entry_ext"], msgs
    assert "ext handles are not taken" in msgs["plan_ext"] and "use the ext form of this call" in msgs["plan_ext"], msgs
