"""libxsmm_hip_gemm_ext_batch_reduce_segments without a GPU: the symbol is exported and mirrored; in dry-run mode every documented refusal sets its code before
the missing device is noticed (an accepted call ends with -4 and nothing launched); the plain entry still refuses ext handles; and the CPU restatement of a
fused ADDRESS call equals the reference's C kernel bit for bit at counts 0, 1 and 3 -- which fixes what a segment of count 0 stores when the handle has a bias."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import GemmCase
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_mirrored(api):
    assert "libxsmm_hip_gemm_ext_batch_reduce_segments" in capi.declared_symbols()
    assert hasattr(api.lib, "libxsmm_hip_gemm_ext_batch_reduce_segments")
    assert len(api.hip_gemm_ext_batch_reduce_segments.argtypes) == 9 and api.hip_gemm_ext_batch_reduce_segments.restype is None


VALIDATION_CHILD = r"""
import sys
import ctypes as C
sys.path.insert(0, %(root)r)
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG, UNARY, UNARY_FLAG
api = capi.load()
def err():
    e = api.hip_get_last_error(); api.hip_clear_last_error(); return e
sh = lambda m, t=DT.F32, c=DT.F32, comp=DT.F32: capi.gemm_shape(m, m, m, m, m, m, t, t, c, comp)
adr = capi.br_config(capi.BR_ADDRESS, 0, 0, 0)
relu, none = lambda m, fl=0: capi.argops_cp(m, UNARY.RELU, fl), capi.no_argops()
ext = api.dispatch_brgemm_ext
f32_bias_relu = ext(sh(32), GEMM_FLAG.BETA_0, 0, adr, relu(32), capi.postops_colbias(32, DT.F32))
f32_mask = ext(sh(20), 0, 0, adr, relu(20, UNARY_FLAG.BITMASK_2BYTEMULT), capi.no_postops())
bf16_sigmoid = ext(sh(64, DT.BF16, DT.BF16), GEMM_FLAG.VNNI_A | GEMM_FLAG.BETA_0, 0, adr, capi.argops_cp(64, UNARY.SIGMOID), capi.no_postops())
bf16f_bias = ext(sh(16, DT.BF16, DT.F32), 0, 0, adr, none, capi.postops_colbias(16, DT.F32))
f32_free = ext(sh(32), GEMM_FLAG.BETA_0, 0, adr, none, capi.no_postops())
f64_free = ext(sh(23, DT.F64, DT.F64, DT.F64), 0, 0, adr, none, capi.no_postops())
plain = api.dispatch_brgemm(sh(32), GEMM_FLAG.BETA_0, 0, adr)
tpp = api.dispatch_meltw_unary(UNARY.IDENTITY, capi.UnaryShape(16, 16, 16, 16, DT.F32, DT.F32, DT.F32), 0)
stride = ext(sh(24), 0, 0, capi.br_config(capi.BR_STRIDE, 24 * 24 * 4, 24 * 24 * 4, 0), relu(24), capi.no_postops())
trans = ext(sh(20), GEMM_FLAG.TRANS_A, 0, adr, relu(20), capi.no_postops())
i8 = ext(sh(32, DT.I8, DT.I32, DT.I32), GEMM_FLAG.VNNI_A, 0, adr, none, capi.no_postops())
handles = dict(f32_bias_relu=f32_bias_relu, f32_mask=f32_mask, bf16_sigmoid=bf16_sigmoid, bf16f_bias=bf16f_bias, f32_free=f32_free, f64_free=f64_free,
               plain=plain, tpp=tpp, stride=stride, trans=trans, i8=i8)
assert all(handles.values()), handles
# never dereferenced on the host: validation reads none of the arrays
SEG, LA, LB, LC, LD, LM, D = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20, 7 << 20
def run(h, n=5, param=True, seg=SEG, la=LA, lb=LB, lc=LC, ld=LD, lm=LM, d=None, tag=None):
    p = capi.GemmExtParam()
    p.d.primary = d
    if tag:
        sys.stderr.write("MARK %%s begin\n" %% tag); sys.stderr.flush()
    api.hip_gemm_ext_batch_reduce_segments(h, C.byref(p) if param else None, n, seg, la, lb, lc, ld, lm)
    if tag:
        sys.stderr.write("MARK %%s end\n" %% tag); sys.stderr.flush()
    return err()
print("null_param", run(f32_bias_relu, param=False))
print("null_seg", run(f32_bias_relu, seg=None))
print("null_a", run(f32_bias_relu, la=None))
print("null_b", run(f32_bias_relu, lb=None))
print("null_c", run(f32_bias_relu, lc=None))
print("empty", run(f32_bias_relu, n=0))
print("empty_null", run(f32_bias_relu, n=0, param=False, seg=None, la=None, lb=None, lc=None, ld=None, lm=None))
print("unknown", run(12345, tag="unknown"))
print("plain", run(plain, tag="plain"))
print("tpp", run(tpp, tag="tpp"))
print("stride", run(stride, tag="stride"))
print("trans", run(trans, tag="trans"))
print("i8", run(i8, tag="i8"))
print("no_d", run(f32_bias_relu, ld=None, tag="no_d"))
print("no_mask", run(f32_mask, lm=None, tag="no_mask"))
print("f32_bias_relu", run(f32_bias_relu, lm=None))
print("f32_shared_d", run(f32_bias_relu, ld=None, lm=None, d=D))
print("f32_mask", run(f32_mask, ld=None))
print("bf16_sigmoid", run(bf16_sigmoid, ld=None, lm=None))
print("bf16f_bias", run(bf16f_bias, lm=None))
print("f32_free", run(f32_free, ld=None, lm=None))
print("f64_free", run(f64_free, ld=None, lm=None))
# the plain entry keeps refusing ext handles
sys.stderr.write("MARK plain_entry begin\n"); sys.stderr.flush()
api.hip_gemm_batch_reduce_segments(f32_bias_relu, C.byref(capi.GemmParam()), 5, SEG, LA, LB, LC)
sys.stderr.write("MARK plain_entry end\n"); sys.stderr.flush()
print("plain_entry", err())
print("launches", api.hip_launch_count(0))
"""

REFUSED = {"unknown": "unknown kernel handle", "plain": "not an ext kernel", "tpp": "not a BRGEMM", "stride": "not an ADDRESS batch-reduce", "trans": "transposed",
           "i8": "operand types", "plain_entry": "ext handles"}
MISSING = {"no_d": "d_list and param->d.primary are both NULL", "no_mask": "mask_list is NULL"}
ACCEPTED = ("f32_bias_relu", "f32_shared_d", "f32_mask", "bf16_sigmoid", "bf16f_bias", "f32_free", "f64_free")


def test_ext_segments_entry_refusals_set_the_documented_error_codes():
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1")
    env.pop("LIBXSMM_VERBOSE", None)
    r = subprocess.run([sys.executable, "-c", VALIDATION_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(ln.split() for ln in r.stdout.splitlines() if len(ln.split()) == 2)
    want = {"null_param": "-2", "null_seg": "-2", "null_a": "-2", "null_b": "-2", "null_c": "-2",      # a NULL array while nsegments > 0
            "empty": "0", "empty_null": "0",                                                          # nsegments == 0: nothing to do, no error
            "launches": "0"}
    want.update({tag: "-4" for tag in ACCEPTED})                                                      # accepted; then: no device
    want.update({tag: "-3" for tag in REFUSED})
    want.update({tag: "-2" for tag in MISSING})
    assert got == want, r.stdout + r.stderr
    # a refused call prints exactly one error, the one that names the reason, and never reaches the device check
    for tag, words in {**REFUSED, **MISSING}.items():
        err = r.stderr.split(f"MARK {tag} begin\n")[1].split(f"MARK {tag} end\n")[0]
        lines = [ln for ln in err.splitlines() if "ERROR" in ln]
        assert len(lines) == 1 and words in lines[0] and "no HIP device" not in err, (tag, err)


ADDRESS_CASES = [dict(m=20, n=12, k=16, colbias=True, act=2, beta=1),
                 dict(m=32, n=24, k=16, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, colbias=True, act=1)]


@pytest.mark.parametrize("kw", ADDRESS_CASES, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
@pytest.mark.parametrize("count", [0, 1, 3])
def test_restatement_of_fused_address_calls_is_bit_identical_to_reference_c_kernel(kw, count, reference):
    """A fused ADDRESS batch-reduce call whose count is passed as 0, 1 or 3 (three blocks are there): the oracle the GPU tests compare with is the reference's C
    kernel bit for bit, C and the whole mask buffer.  Count 0 with a bias: the start value goes through the activation and is stored, the mask comes from it."""
    case = GemmCase(seed=777, br_type=capi.BR_ADDRESS, br_count=3, **kw)
    case.br_count = count                                   # make_param passes it in op.tertiary; the operands keep three blocks
    c_or, m_or = case.run_oracle()
    c_rf, m_rf = case.run_reference(jit=False)
    assert c_or.tobytes() == c_rf.tobytes()
    if m_or is not None:
        assert m_or.tobytes() == m_rf.tobytes() and m_or.any()
    if count == 0:                                          # what a segment of count 0 means with a bias: activation(bias (+ C)), one rounding to C's type
        from helpers import as_float
        v = as_float(case.valid_region(c_or), case.c_type)
        bias = as_float(case.D, case.c_type)[None, None, :]
        start = bias + (as_float(case.valid_region(case.C0), case.c_type) if kw.get("beta") else 0.0)
        want = np.broadcast_to(np.maximum(start, 0.0), v.shape).astype(np.float32)
        assert np.array_equal(v, as_float(_to_c(want, case.c_type), case.c_type))


def _to_c(x, dt):
    """f32 -> C's type as the reference rounds it (bf16: round to nearest even; the values here are normal numbers)."""
    if dt != DT.BF16:
        return x
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
