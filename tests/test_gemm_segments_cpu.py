"""libxsmm_hip_gemm_batch_reduce_segments without a GPU: the symbol is exported and mirrored, and in dry-run mode every documented refusal sets its code
before the missing device is noticed -- validation comes first, an accepted call ends with -4 and nothing launched."""
import os
import subprocess
import sys

from libxsmm_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_mirrored(api):
    assert "libxsmm_hip_gemm_batch_reduce_segments" in capi.declared_symbols()
    assert hasattr(api.lib, "libxsmm_hip_gemm_batch_reduce_segments")
    assert len(api.hip_gemm_batch_reduce_segments.argtypes) == 7 and api.hip_gemm_batch_reduce_segments.restype is None


VALIDATION_CHILD = r"""
import sys
import ctypes as C
sys.path.insert(0, %(root)r)
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG, UNARY
api = capi.load()
def err():
    e = api.hip_get_last_error(); api.hip_clear_last_error(); return e
sh = lambda m, t=DT.F32, c=DT.F32, comp=DT.F32: capi.gemm_shape(m, m, m, m, m, m, t, t, c, comp)
adr = capi.br_config(capi.BR_ADDRESS, 0, 0, 0)
f32 = api.dispatch_brgemm(sh(32), GEMM_FLAG.BETA_0, 0, adr)
f64 = api.dispatch_brgemm(sh(23, DT.F64, DT.F64, DT.F64), 0, 0, adr)
bf16 = api.dispatch_brgemm(sh(64, DT.BF16, DT.BF16), GEMM_FLAG.VNNI_A | GEMM_FLAG.BETA_0, 0, adr)
bf16f = api.dispatch_brgemm(sh(16, DT.BF16, DT.F32), 0, 0, adr)
plain = api.dispatch_gemm(sh(32), GEMM_FLAG.BETA_0, 0)
stride = api.dispatch_brgemm(sh(24), 0, 0, capi.br_config(capi.BR_STRIDE, 24 * 24 * 4, 24 * 24 * 4, 0))
trans = api.dispatch_brgemm(sh(20), GEMM_FLAG.TRANS_A, 0, adr)
i8 = api.dispatch_brgemm(sh(32, DT.I8, DT.I32, DT.I32), GEMM_FLAG.VNNI_A, 0, adr)
ext = api.dispatch_brgemm_ext(sh(32), 0, 0, adr, capi.argops_cp(32, UNARY.RELU), capi.no_postops())
tpp = api.dispatch_meltw_unary(UNARY.IDENTITY, capi.UnaryShape(16, 16, 16, 16, DT.F32, DT.F32, DT.F32), 0)
assert f32 and f64 and bf16 and bf16f and plain and stride and trans and i8 and ext and tpp
# never dereferenced on the host: validation reads none of the four arrays
SEG, LA, LB, LC = 1 << 20, 2 << 20, 3 << 20, 4 << 20
p = capi.GemmParam()
def run(h, n=5, param=True, seg=SEG, la=LA, lb=LB, lc=LC, tag=None):
    if tag:
        sys.stderr.write("MARK %%s begin\n" %% tag); sys.stderr.flush()
    api.hip_gemm_batch_reduce_segments(h, C.byref(p) if param else None, n, seg, la, lb, lc)
    if tag:
        sys.stderr.write("MARK %%s end\n" %% tag); sys.stderr.flush()
    return err()
print("null_param", run(f32, param=False))
print("null_seg", run(f32, seg=None))
print("null_a", run(f32, la=None))
print("null_b", run(f32, lb=None))
print("null_c", run(f32, lc=None))
print("empty", run(f32, n=0))
print("empty_null", run(f32, n=0, param=False, seg=None, la=None, lb=None, lc=None))
print("unknown", run(12345, tag="unknown"))
print("tpp", run(tpp, tag="tpp"))
print("ext", run(ext, tag="ext"))
print("plain", run(plain, tag="plain"))
print("stride", run(stride, tag="stride"))
print("trans", run(trans, tag="trans"))
print("i8", run(i8, tag="i8"))
print("f32", run(f32))
print("f64", run(f64))
print("bf16", run(bf16))
print("bf16f", run(bf16f))
print("launches", api.hip_launch_count(0))
"""

REFUSED = {"unknown": "unknown kernel handle", "tpp": "not a BRGEMM", "ext": "ext handles", "plain": "not an ADDRESS batch-reduce",
           "stride": "not an ADDRESS batch-reduce", "trans": "transposed", "i8": "operand types"}


def test_segments_entry_refusals_set_the_documented_error_codes():
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1")
    env.pop("LIBXSMM_VERBOSE", None)
    r = subprocess.run([sys.executable, "-c", VALIDATION_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(ln.split() for ln in r.stdout.splitlines() if len(ln.split()) == 2)
    want = {"null_param": "-2", "null_seg": "-2", "null_a": "-2", "null_b": "-2", "null_c": "-2",      # a NULL array while nsegments > 0
            "empty": "0", "empty_null": "0",                                                          # nsegments == 0: nothing to do, no error
            "f32": "-4", "f64": "-4", "bf16": "-4", "bf16f": "-4",                                    # accepted; then: no device
            "launches": "0"}
    want.update({tag: "-3" for tag in REFUSED})
    assert got == want, r.stdout + r.stderr
    # a refused call prints exactly one error, the one that names the reason, and never reaches the device check
    for tag, words in REFUSED.items():
        err = r.stderr.split(f"MARK {tag} begin\n")[1].split(f"MARK {tag} end\n")[0]
        lines = [ln for ln in err.splitlines() if "ERROR" in ln]
        assert len(lines) == 1 and words in lines[0] and "no HIP device" not in err, (tag, err)
