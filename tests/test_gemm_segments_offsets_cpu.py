"""libxsmm_hip_gemm_batch_reduce_segments_offsets without a GPU: the symbol is exported and mirrored; in dry-run mode every documented refusal sets its code
before the missing device is noticed (an accepted call -- NN, TN, NT, TT -- ends with -4 and nothing launched) while the two ADDRESS entries keep refusing
transposes; and the CPU restatement of an OFFSET batch-reduce call with transposed operands equals the reference's C kernel bit for bit at counts 0, 1 and 3."""
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
    assert "libxsmm_hip_gemm_batch_reduce_segments_offsets" in capi.declared_symbols()
    assert hasattr(api.lib, "libxsmm_hip_gemm_batch_reduce_segments_offsets")
    assert len(api.hip_gemm_batch_reduce_segments_offsets.argtypes) == 7 and api.hip_gemm_batch_reduce_segments_offsets.restype is None


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
off, adr = capi.br_config(capi.BR_OFFSET, 0, 0, 0), capi.br_config(capi.BR_ADDRESS, 0, 0, 0)
TA, TB = GEMM_FLAG.TRANS_A, GEMM_FLAG.TRANS_B
f32_nn = api.dispatch_brgemm(sh(32), GEMM_FLAG.BETA_0, 0, off)
f32_tn = api.dispatch_brgemm(sh(32), TA, 0, off)
f32_nt = api.dispatch_brgemm(sh(20), TB | GEMM_FLAG.BETA_0, 0, off)
f32_tt = api.dispatch_brgemm(sh(13), TA | TB, 0, off)
f64_tn = api.dispatch_brgemm(sh(23, DT.F64, DT.F64, DT.F64), TA, 0, off)
bf16_ta = api.dispatch_brgemm(sh(64, DT.BF16, DT.BF16), TA | GEMM_FLAG.BETA_0, 0, off)
bf16_vnni_tb = api.dispatch_brgemm(sh(16, DT.BF16, DT.F32), GEMM_FLAG.VNNI_A | TB, 0, off)
plain = api.dispatch_gemm(sh(32), GEMM_FLAG.BETA_0, 0)
stride = api.dispatch_brgemm(sh(24), 0, 0, capi.br_config(capi.BR_STRIDE, 24 * 24 * 4, 24 * 24 * 4, 0))
address = api.dispatch_brgemm(sh(32), GEMM_FLAG.BETA_0, 0, adr)
address_ta = api.dispatch_brgemm(sh(20), TA, 0, adr)
i8 = api.dispatch_brgemm(sh(32, DT.I8, DT.I32, DT.I32), GEMM_FLAG.VNNI_A, 0, off)
vnni_b = api.dispatch_brgemm(sh(32, DT.BF16, DT.BF16), GEMM_FLAG.VNNI_B | TB, 0, off)
ext = api.dispatch_brgemm_ext(sh(32), 0, 0, off, capi.argops_cp(32, UNARY.RELU), capi.no_postops())
ext_ta = api.dispatch_brgemm_ext(sh(20), TA, 0, adr, capi.argops_cp(20, UNARY.RELU), capi.no_postops())
tpp = api.dispatch_meltw_unary(UNARY.IDENTITY, capi.UnaryShape(16, 16, 16, 16, DT.F32, DT.F32, DT.F32), 0)
handles = dict(f32_nn=f32_nn, f32_tn=f32_tn, f32_nt=f32_nt, f32_tt=f32_tt, f64_tn=f64_tn, bf16_ta=bf16_ta, bf16_vnni_tb=bf16_vnni_tb, plain=plain, stride=stride,
               address=address, address_ta=address_ta, i8=i8, vnni_b=vnni_b, ext=ext, ext_ta=ext_ta, tpp=tpp)
assert all(handles.values()), handles
# never dereferenced on the host: validation reads none of the four arrays and none of the three bases
SEG, OA, OB, OC, A, B, CC = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20, 7 << 20
def run(h, n=5, param=True, seg=SEG, oa=OA, ob=OB, oc=OC, a=A, b=B, c=CC, tag=None):
    p = capi.GemmParam()
    p.a.primary, p.b.primary, p.c.primary = a, b, c
    if tag:
        sys.stderr.write("MARK %%s begin\n" %% tag); sys.stderr.flush()
    api.hip_gemm_batch_reduce_segments_offsets(h, C.byref(p) if param else None, n, seg, oa, ob, oc)
    if tag:
        sys.stderr.write("MARK %%s end\n" %% tag); sys.stderr.flush()
    return err()
print("null_param", run(f32_nn, param=False))
print("null_seg", run(f32_nn, seg=None))
print("null_a_offs", run(f32_nn, oa=None))
print("null_b_offs", run(f32_nn, ob=None))
print("null_c_offs", run(f32_nn, oc=None))
print("null_a_base", run(f32_nn, a=None))
print("null_b_base", run(f32_nn, b=None))
print("null_c_base", run(f32_nn, c=None))
print("empty", run(f32_nn, n=0))
print("empty_null", run(f32_nn, n=0, param=False, seg=None, oa=None, ob=None, oc=None))
print("unknown", run(12345, tag="unknown"))
print("tpp", run(tpp, tag="tpp"))
print("ext", run(ext, tag="ext"))
print("plain", run(plain, tag="plain"))
print("stride", run(stride, tag="stride"))
print("address", run(address, tag="address"))
print("i8", run(i8, tag="i8"))
print("vnni_b", run(vnni_b, tag="vnni_b"))
for name in ("f32_nn", "f32_tn", "f32_nt", "f32_tt", "f64_tn", "bf16_ta", "bf16_vnni_tb"):
    print(name, run(handles[name]))
# the two ADDRESS entries keep refusing transposed operands
q = capi.GemmParam()
sys.stderr.write("MARK address_entry begin\n"); sys.stderr.flush()
api.hip_gemm_batch_reduce_segments(address_ta, C.byref(q), 5, SEG, OA, OB, OC)
sys.stderr.write("MARK address_entry end\n"); sys.stderr.flush()
print("address_entry", err())
e = capi.GemmExtParam()
sys.stderr.write("MARK ext_entry begin\n"); sys.stderr.flush()
api.hip_gemm_ext_batch_reduce_segments(ext_ta, C.byref(e), 5, SEG, OA, OB, OC, None, None)
sys.stderr.write("MARK ext_entry end\n"); sys.stderr.flush()
print("ext_entry", err())
print("launches", api.hip_launch_count(0))
"""

REFUSED = {"unknown": "unknown kernel handle", "tpp": "not a BRGEMM", "ext": "ext handles", "plain": "not an OFFSET batch-reduce",
           "stride": "not an OFFSET batch-reduce", "address": "not an OFFSET batch-reduce", "i8": "operand types", "vnni_b": "VNNI layouts of B and C",
           "address_entry": "transposed operands are not taken (NN only)", "ext_entry": "transposed operands are not taken (NN only)"}
NULLS = ("null_param", "null_seg", "null_a_offs", "null_b_offs", "null_c_offs", "null_a_base", "null_b_base", "null_c_base")
ACCEPTED = ("f32_nn", "f32_tn", "f32_nt", "f32_tt", "f64_tn", "bf16_ta", "bf16_vnni_tb")


def test_offsets_entry_refusals_set_the_documented_error_codes():
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1")
    env.pop("LIBXSMM_VERBOSE", None)
    r = subprocess.run([sys.executable, "-c", VALIDATION_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(ln.split() for ln in r.stdout.splitlines() if len(ln.split()) == 2)
    want = {"empty": "0", "empty_null": "0", "launches": "0"}                                          # nsegments == 0: nothing to do, no error
    want.update({tag: "-2" for tag in NULLS})                                                          # a NULL array or base while nsegments > 0
    want.update({tag: "-4" for tag in ACCEPTED})                                                       # accepted; then: no device
    want.update({tag: "-3" for tag in REFUSED})
    assert got == want, r.stdout + r.stderr
    # a refused call prints exactly one error, the one that names the reason, and never reaches the device check
    for tag, words in REFUSED.items():
        err = r.stderr.split(f"MARK {tag} begin\n")[1].split(f"MARK {tag} end\n")[0]
        lines = [ln for ln in err.splitlines() if "ERROR" in ln]
        assert len(lines) == 1 and words in lines[0] and "no HIP device" not in err, (tag, err)


FORMS = {"NN": 0, "TN": GEMM_FLAG.TRANS_A, "NT": GEMM_FLAG.TRANS_B, "TT": GEMM_FLAG.TRANS_A | GEMM_FLAG.TRANS_B}
M, N, K = 13, 17, 29


def padded(flags):
    """Padded leading dimensions of the 13 x 17 x 29 problem under `flags`: lda >= k with TRANS_A (else >= m), ldb >= n with TRANS_B (else >= k)."""
    return dict(lda=(K if flags & GEMM_FLAG.TRANS_A else M) + 3, ldb=(N if flags & GEMM_FLAG.TRANS_B else K) + 2, ldc=M + 5)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("types", [(DT.F32, DT.F32), (DT.F64, DT.F64), (DT.BF16, DT.BF16)], ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("count", [0, 1, 3])
def test_restatement_of_transposed_offset_calls_is_bit_identical_to_reference_c_kernel(form, types, count, reference):
    """An OFFSET batch-reduce call whose count is passed as 0, 1 or 3 (three blocks are there), NN / TN / NT / TT: the oracle the GPU tests compare with -- plain
    and as the k-ordered fmaf chain -- indexes the transposed operands as the reference's C kernel does, bit for bit over the whole C buffer."""
    flags = FORMS[form]
    for beta in (0, 1):
        case = GemmCase(M, N, K, a_type=types[0], c_type=types[1], flags=flags, beta=beta, br_type=capi.BR_OFFSET, br_count=3, seed=888 + beta, **padded(flags))
        case.br_count = count                               # make_param passes it in op.tertiary; the operands keep three blocks
        c_rf = case.C0.copy()
        p, keep = case.make_param(case.A, case.B, c_rf, offs=(case.offs_a, case.offs_b))
        rc = reference.lib.xref_reference_gemm(C.byref(p), case.shape(), case.flags, 0, case.brcfg())
        if rc != 0:
            pytest.skip(f"the reference's dispatcher refuses {form} {types} on this host (descriptor_init_brgemm returned NULL)")
        c_or, _ = case.run_oracle()
        assert c_or.tobytes() == c_rf.tobytes(), f"{form} beta={beta} count={count}"
        if types[0] == DT.F32:
            # the fmaf chain the f32 kernels are held to rounds once per step where the reference's kernel rounds the product and the sum, so it is compared
            # on small integers, where both are exact: what is checked is its indexing of the transposed operands and of the offset lists
            ex = GemmCase(M, N, K, flags=flags, beta=beta, br_type=capi.BR_OFFSET, br_count=3, seed=890, **padded(flags))
            rng = np.random.default_rng(5)
            ex.A[:] = rng.integers(-2, 3, ex.A.size); ex.B[:] = rng.integers(-2, 3, ex.B.size); ex.C0[:] = rng.integers(-2, 3, ex.C0.size)
            ex.br_count = count
            x_rf = ex.C0.copy()
            p, keep = ex.make_param(ex.A, ex.B, x_rf, offs=(ex.offs_a, ex.offs_b))
            assert reference.lib.xref_reference_gemm(C.byref(p), ex.shape(), ex.flags, 0, ex.brcfg()) == 0
            assert ex.run_oracle(fma=True)[0].tobytes() == x_rf.tobytes(), f"fma chain, {form} beta={beta} count={count}"
