"""libxsmm_hip_gemm_ext_batch_reduce_segments_offsets without a GPU: the symbol is exported and mirrored; in dry-run mode every documented refusal sets its code
before the missing device is noticed (an accepted call -- NN, TN, NT, TT, with and without operators -- ends with -4 and nothing launched) while the three older
entries answer the same handles as their own tests pin; and the CPU restatement of a fused OFFSET batch-reduce call with transposed operands -- the ext oracle,
and the composition the GPU tests hold the f32 kernels to -- equals the reference's C kernel bit for bit, C and mask, at counts 0, 1 and 3."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import GemmCase
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_mirrored(api):
    assert "libxsmm_hip_gemm_ext_batch_reduce_segments_offsets" in capi.declared_symbols()
    assert hasattr(api.lib, "libxsmm_hip_gemm_ext_batch_reduce_segments_offsets")
    assert len(api.hip_gemm_ext_batch_reduce_segments_offsets.argtypes) == 9 and api.hip_gemm_ext_batch_reduce_segments_offsets.restype is None


VALIDATION_CHILD = r"""
import sys
import ctypes as C
sys.path.insert(0, %(root)r)
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG, UNARY, UNARY_FLAG, BINARY, BINARY_FLAG
api = capi.load()
def err():
    e = api.hip_get_last_error(); api.hip_clear_last_error(); return e
sh = lambda m, t=DT.F32, c=DT.F32, comp=DT.F32: capi.gemm_shape(m, m, m, m, m, m, t, t, c, comp)
off, adr = capi.br_config(capi.BR_OFFSET, 0, 0, 0), capi.br_config(capi.BR_ADDRESS, 0, 0, 0)
TA, TB = GEMM_FLAG.TRANS_A, GEMM_FLAG.TRANS_B
relu, none = lambda m, fl=0: capi.argops_cp(m, UNARY.RELU, fl), capi.no_argops()
ext = api.dispatch_brgemm_ext
f32_bias_relu = ext(sh(32), GEMM_FLAG.BETA_0, 0, off, relu(32), capi.postops_colbias(32, DT.F32))
f32_tn_mask = ext(sh(20), TA, 0, off, relu(20, UNARY_FLAG.BITMASK_2BYTEMULT), capi.no_postops())
f32_tt_bias_mask = ext(sh(13), TA | TB, 0, off, relu(13, UNARY_FLAG.BITMASK_2BYTEMULT), capi.postops_colbias(13, DT.F32))
bf16_nt_sigmoid = ext(sh(64, DT.BF16, DT.BF16), GEMM_FLAG.VNNI_A | TB | GEMM_FLAG.BETA_0, 0, off, capi.argops_cp(64, UNARY.SIGMOID), capi.no_postops())
bf16f_ta_bias = ext(sh(16, DT.BF16, DT.F32), TA, 0, off, none, capi.postops_colbias(16, DT.F32))
f32_free = ext(sh(32), GEMM_FLAG.BETA_0 | TB, 0, off, none, capi.no_postops())
f64_free = ext(sh(23, DT.F64, DT.F64, DT.F64), TA, 0, off, none, capi.no_postops())
# f64 with operators, a VNNI-2 A under TRANS_A and operators outside the list have no handle: the dispatcher refuses them before any entry could
assert not ext(sh(23, DT.F64, DT.F64, DT.F64), 0, 0, off, relu(23), capi.no_postops())
assert not ext(sh(32, DT.BF16, DT.BF16), GEMM_FLAG.VNNI_A | TA, 0, off, relu(32), capi.no_postops())
assert not ext(sh(32), 0, 0, off, none, capi.ExtBinaryPostops(32, DT.F32, BINARY.ADD, BINARY_FLAG.BCAST_ROW_IN_0))
plain = api.dispatch_brgemm(sh(32), GEMM_FLAG.BETA_0, 0, off)
tpp = api.dispatch_meltw_unary(UNARY.IDENTITY, capi.UnaryShape(16, 16, 16, 16, DT.F32, DT.F32, DT.F32), 0)
stride = ext(sh(24), 0, 0, capi.br_config(capi.BR_STRIDE, 24 * 24 * 4, 24 * 24 * 4, 0), relu(24), capi.no_postops())
address = ext(sh(32), GEMM_FLAG.BETA_0, 0, adr, relu(32), capi.postops_colbias(32, DT.F32))
address_ta = ext(sh(20), TA, 0, adr, relu(20), capi.no_postops())
i8 = ext(sh(32, DT.I8, DT.I32, DT.I32), GEMM_FLAG.VNNI_A, 0, off, none, capi.no_postops())
vnni_b = ext(sh(32, DT.BF16, DT.BF16), GEMM_FLAG.VNNI_B | TB, 0, off, relu(32), capi.no_postops())
handles = dict(f32_bias_relu=f32_bias_relu, f32_tn_mask=f32_tn_mask, f32_tt_bias_mask=f32_tt_bias_mask, bf16_nt_sigmoid=bf16_nt_sigmoid, bf16f_ta_bias=bf16f_ta_bias,
               f32_free=f32_free, f64_free=f64_free, plain=plain, tpp=tpp, stride=stride, address=address, address_ta=address_ta, i8=i8, vnni_b=vnni_b)
assert all(handles.values()), handles
# never dereferenced on the host: validation reads none of the six arrays and none of the five bases
SEG, OA, OB, OC, OD, OM, A, B, CC, D, M = (i << 20 for i in range(1, 12))
def run(h, n=5, param=True, seg=SEG, oa=OA, ob=OB, oc=OC, od=OD, om=OM, a=A, b=B, c=CC, d=D, m=M, tag=None):
    p = capi.GemmExtParam()
    p.a.primary, p.b.primary, p.c.primary, p.d.primary, p.c.secondary = a, b, c, d, m
    if tag:
        sys.stderr.write("MARK %%s begin\n" %% tag); sys.stderr.flush()
    api.hip_gemm_ext_batch_reduce_segments_offsets(h, C.byref(p) if param else None, n, seg, oa, ob, oc, od, om)
    if tag:
        sys.stderr.write("MARK %%s end\n" %% tag); sys.stderr.flush()
    return err()
print("null_param", run(f32_bias_relu, param=False, tag="null_param"))
print("null_seg", run(f32_bias_relu, seg=None, tag="null_seg"))
print("null_a_offs", run(f32_bias_relu, oa=None, tag="null_a_offs"))
print("null_b_offs", run(f32_bias_relu, ob=None, tag="null_b_offs"))
print("null_c_offs", run(f32_bias_relu, oc=None, tag="null_c_offs"))
print("null_a_base", run(f32_bias_relu, a=None, tag="null_a_base"))
print("null_b_base", run(f32_bias_relu, b=None, tag="null_b_base"))
print("null_c_base", run(f32_bias_relu, c=None, tag="null_c_base"))
print("null_d_base", run(f32_bias_relu, d=None, tag="null_d_base"))
print("null_d_base_shared", run(f32_bias_relu, d=None, od=None, tag="null_d_base_shared"))
print("null_mask_offs", run(f32_tn_mask, om=None, tag="null_mask_offs"))
print("null_mask_base", run(f32_tt_bias_mask, m=None, tag="null_mask_base"))
print("empty", run(f32_bias_relu, n=0))
print("empty_null", run(f32_bias_relu, n=0, param=False, seg=None, oa=None, ob=None, oc=None, od=None, om=None))
print("unknown", run(12345, tag="unknown"))
print("plain", run(plain, tag="plain"))
print("tpp", run(tpp, tag="tpp"))
print("stride", run(stride, tag="stride"))
print("address", run(address, tag="address"))
print("i8", run(i8, tag="i8"))
print("vnni_b", run(vnni_b, tag="vnni_b"))
# accepted: the mask arguments are ignored without the bitmask flag, the bias arguments without a bias
print("f32_bias_relu", run(f32_bias_relu, om=None, m=None))
print("f32_shared_d", run(f32_bias_relu, od=None, om=None, m=None))
print("f32_tn_mask", run(f32_tn_mask, od=None, d=None))
print("f32_tt_bias_mask", run(f32_tt_bias_mask))
print("bf16_nt_sigmoid", run(bf16_nt_sigmoid, od=None, om=None, d=None, m=None))
print("bf16f_ta_bias", run(bf16f_ta_bias, om=None, m=None))
print("f32_free", run(f32_free, od=None, om=None, d=None, m=None))
print("f64_free", run(f64_free, od=None, om=None, d=None, m=None))
# the three older entries, called with the same handles, answer as their own tests pin
def older(tag, call):
    sys.stderr.write("MARK %%s begin\n" %% tag); sys.stderr.flush()
    call()
    sys.stderr.write("MARK %%s end\n" %% tag); sys.stderr.flush()
    print(tag, err())
q = capi.GemmParam(); q.a.primary, q.b.primary, q.c.primary = A, B, CC
e = capi.GemmExtParam()
older("offsets_entry", lambda: api.hip_gemm_batch_reduce_segments_offsets(f32_bias_relu, C.byref(q), 5, SEG, OA, OB, OC))
older("offsets_entry_free", lambda: api.hip_gemm_batch_reduce_segments_offsets(f32_free, C.byref(q), 5, SEG, OA, OB, OC))
older("plain_entry", lambda: api.hip_gemm_batch_reduce_segments(f32_bias_relu, C.byref(q), 5, SEG, OA, OB, OC))
older("ext_entry", lambda: api.hip_gemm_ext_batch_reduce_segments(f32_bias_relu, C.byref(e), 5, SEG, OA, OB, OC, OD, None))
older("ext_entry_ta", lambda: api.hip_gemm_ext_batch_reduce_segments(address_ta, C.byref(e), 5, SEG, OA, OB, OC, None, None))
older("ext_entry_address", lambda: api.hip_gemm_ext_batch_reduce_segments(address, C.byref(e), 5, SEG, OA, OB, OC, OD, None))
older("offsets_entry_plain", lambda: api.hip_gemm_batch_reduce_segments_offsets(plain, C.byref(q), 5, SEG, OA, OB, OC))
print("launches", api.hip_launch_count(0))
"""

REFUSED = {"unknown": "unknown kernel handle", "plain": "not an ext kernel", "tpp": "not a BRGEMM", "stride": "not an OFFSET batch-reduce",
           "address": "not an OFFSET batch-reduce", "i8": "operand types", "vnni_b": "VNNI layouts of B and C",
           "offsets_entry": "ext handles", "offsets_entry_free": "ext handles", "plain_entry": "ext handles", "ext_entry": "not an ADDRESS batch-reduce",
           "ext_entry_ta": "transposed operands are not taken (NN only)"}
NULLS = {"null_param": "param is NULL", "null_seg": "seg_ptr is NULL", "null_a_offs": "a_offs is NULL", "null_b_offs": "b_offs is NULL", "null_c_offs": "c_offs is NULL",
         "null_a_base": "param->a.primary", "null_b_base": "param->b.primary", "null_c_base": "param->c.primary", "null_d_base": "param->d.primary",
         "null_d_base_shared": "param->d.primary", "null_mask_offs": "mask_offs is NULL", "null_mask_base": "param->c.secondary"}
ACCEPTED = ("f32_bias_relu", "f32_shared_d", "f32_tn_mask", "f32_tt_bias_mask", "bf16_nt_sigmoid", "bf16f_ta_bias", "f32_free", "f64_free",
            "ext_entry_address", "offsets_entry_plain")


def test_fused_offsets_entry_refusals_set_the_documented_error_codes():
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1")
    env.pop("LIBXSMM_VERBOSE", None)
    r = subprocess.run([sys.executable, "-c", VALIDATION_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(ln.split() for ln in r.stdout.splitlines() if len(ln.split()) == 2)
    want = {"empty": "0", "empty_null": "0", "launches": "0"}                                          # nsegments == 0: nothing to do, no error
    want.update({tag: "-2" for tag in NULLS})                                                          # a NULL required array or base while nsegments > 0
    want.update({tag: "-4" for tag in ACCEPTED})                                                       # accepted; then: no device
    want.update({tag: "-3" for tag in REFUSED})
    assert got == want, r.stdout + r.stderr
    # a refused call prints exactly one error, the one that names the reason, and never reaches the device check
    for tag, words in {**REFUSED, **NULLS}.items():
        err = r.stderr.split(f"MARK {tag} begin\n")[1].split(f"MARK {tag} end\n")[0]
        lines = [ln for ln in err.splitlines() if "ERROR" in ln]
        assert len(lines) == 1 and words in lines[0] and "no HIP device" not in err, (tag, err)


FORMS = {"NN": 0, "TN": GEMM_FLAG.TRANS_A, "NT": GEMM_FLAG.TRANS_B, "TT": GEMM_FLAG.TRANS_A | GEMM_FLAG.TRANS_B}
TYPES = {"f32": (DT.F32, DT.F32), "bf16": (DT.BF16, DT.BF16), "bf16f": (DT.BF16, DT.F32)}
M, N, K = 13, 17, 29


def padded(flags):
    """Padded leading dimensions of the 13 x 17 x 29 problem under `flags`: lda >= k with TRANS_A (else >= m), ldb >= n with TRANS_B (else >= k)."""
    return dict(lda=(K if flags & GEMM_FLAG.TRANS_A else M) + 3, ldb=(N if flags & GEMM_FLAG.TRANS_B else K) + 2, ldc=M + 5)


def _fused_case(flags, types, beta, count, seed, ints=False):
    """An OFFSET ext case with bias + ReLU + bitmask over three blocks whose count is passed as `count`, and a mask buffer prefilled with random bytes."""
    case = GemmCase(M, N, K, a_type=types[0], c_type=types[1], flags=flags, beta=beta, br_type=capi.BR_OFFSET, br_count=3, colbias=True, act=2, seed=seed, **padded(flags))
    rng = np.random.default_rng(seed + 1)
    if ints:
        case.A[:] = rng.integers(-2, 3, case.A.size); case.B[:] = rng.integers(-2, 3, case.B.size)
        case.C0[:] = rng.integers(-2, 3, case.C0.size); case.D[:] = rng.integers(-2, 3, case.D.size)
    case.br_count = count                                   # make_param passes it in op.tertiary; the operands keep three blocks
    return case, rng.integers(0, 256, case.mask_bytes).astype(np.uint8)


def _reference(reference, case, mask0):
    c, m = case.C0.copy(), mask0.copy()
    p, keep = case.make_param(case.A, case.B, c, case.D, m, offs=(case.offs_a, case.offs_b))
    rc = reference.lib.xref_reference_gemm_ext(C.byref(p), case.shape(), case.flags, 0, case.brcfg(), case.argops(), case.postops())
    return rc, c, m


def _chain_composition(case, mask0):
    """FusedSegments.fma_chain's composition for one call: bias (+ C0, one f32 add) written into a copy of C, the k-ordered fmaf chain with beta = 1 through the
    NON-ext descriptor on top of it, the mask bits !(x <= 0) merged into the prefilled mask, then ReLU as np.where(x <= 0, +0, x)."""
    plain = GemmCase(M, N, K, flags=case.flags & ~GEMM_FLAG.BETA_0, beta=1, br_type=capi.BR_OFFSET, br_count=3, lda=case.lda, ldb=case.ldb, ldc=case.ldc)
    plain.br_count = case.br_count
    c, m = case.C0.copy(), mask0.copy()
    v = c[:case.ldc * N].reshape(N, case.ldc)[:, :M]
    beta = 0 if case.flags & GEMM_FLAG.BETA_0 else 1
    v[...] = (case.D[None, :] + v) if beta else np.broadcast_to(case.D[None, :], v.shape)
    p, keep = plain.make_param(case.A, case.B, c, offs=(case.offs_a, case.offs_b))
    pyoracle.oracle().gemm(p, plain.oracle_desc(), fma=True)
    rows = m.reshape(N, case.mask_ld // 8)
    bits = np.unpackbits(rows, axis=1, bitorder="little")
    bits[:, :M] = ~(v <= 0)
    rows[...] = np.packbits(bits, axis=1, bitorder="little")
    v[...] = np.where(v <= 0, np.float32(0.0), v)
    return c, m


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("types", list(TYPES))
@pytest.mark.parametrize("count", [0, 1, 3])
def test_restatement_of_fused_offset_calls_is_bit_identical_to_reference_c_kernel(form, types, count, reference):
    """A fused OFFSET batch-reduce call (bias + ReLU + bitmask) whose count is passed as 0, 1 or 3, NN / TN / NT / TT: the ext oracle the GPU tests compare with is
    the reference's C kernel bit for bit over the whole C and mask buffers; for f32 so is, on small integers, the composition that states the fmaf chain."""
    flags = FORMS[form]
    for beta in (0, 1):
        case, mask0 = _fused_case(flags, TYPES[types], beta, count, 900 + beta)
        rc, c_rf, m_rf = _reference(reference, case, mask0)
        if rc != 0:
            assert form != "NN", "the reference's dispatcher must take the NN descriptor"
            pytest.skip(f"the reference's dispatcher refuses {form} {types} on this host (descriptor_init_brgemm_ext returned NULL)")
        c_or, m_or = case.C0.copy(), mask0.copy()
        p, keep = case.make_param(case.A, case.B, c_or, case.D, m_or, offs=(case.offs_a, case.offs_b))
        pyoracle.oracle().gemm(p, case.oracle_desc())
        assert c_or.tobytes() == c_rf.tobytes(), f"C: {form} {types} beta={beta} count={count}"
        assert m_or.tobytes() == m_rf.tobytes(), f"mask: {form} {types} beta={beta} count={count}"
        assert not np.array_equal(m_rf, mask0)
        if types == "f32":
            # the fmaf chain rounds once per step where the reference's kernel rounds the product and the sum: compared on small integers, where both are exact --
            # what is checked is the composition's start value, its indexing of the transposed operands and offset lists, its mask and its ReLU
            ex, xmask0 = _fused_case(flags, TYPES[types], beta, count, 910 + beta, ints=True)
            rc, x_rf, xm_rf = _reference(reference, ex, xmask0)
            assert rc == 0
            x_ch, xm_ch = _chain_composition(ex, xmask0)
            assert x_ch.tobytes() == x_rf.tobytes(), f"fma chain composition, C: {form} beta={beta} count={count}"
            assert xm_ch.tobytes() == xm_rf.tobytes(), f"fma chain composition, mask: {form} beta={beta} count={count}"
