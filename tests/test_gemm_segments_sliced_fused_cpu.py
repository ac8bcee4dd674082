"""The sliced ext segments entries (include/libxsmm_hip.h) without a GPU: the three symbols are exported and mirrored; in dry-run mode every documented refusal
sets its code -- one error line that names the reason -- before the missing device is noticed, accepted calls end with -4 and nothing launched, and the
workspace query keeps its bounds for ext handles; the CPU statement of the semantics (tests/segments_sliced_fused_helpers.py) equals, bit for bit, the
reference's own kernel called once per slice with beta = 0 followed by the start value, the adds in slice order, the mask and ReLU in numpy; and its blocks
without slices equal the ext oracle called with a count of 0."""
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
from segments_sliced_fused_helpers import sliced_fused_reference
from segments_sliced_helpers import csr, partial_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("libxsmm_hip_gemm_ext_batch_reduce_segments_sliced_workspace", "libxsmm_hip_gemm_ext_batch_reduce_segments_sliced",
         "libxsmm_hip_gemm_ext_batch_reduce_segments_offsets_sliced")


def test_symbols_are_declared_exported_and_mirrored(api):
    for name in NAMES:
        assert name in capi.declared_symbols() and hasattr(api.lib, name), name
    assert len(api.hip_gemm_ext_batch_reduce_segments_sliced_workspace.argtypes) == 2 and api.hip_gemm_ext_batch_reduce_segments_sliced_workspace.restype is C.c_size_t
    for fn in (api.hip_gemm_ext_batch_reduce_segments_sliced, api.hip_gemm_ext_batch_reduce_segments_offsets_sliced):
        assert len(fn.argtypes) == 13 and fn.restype is None


VALIDATION_CHILD = r"""
import sys
import ctypes as C
sys.path.insert(0, %(root)r)
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG, UNARY, UNARY_FLAG
api = capi.load()
def err():
    e = api.hip_get_last_error(); api.hip_clear_last_error(); return e
def sh(m, n=None, k=None, t=DT.F32, c=DT.F32, comp=DT.F32):
    n, k = n or m, k or m
    return capi.gemm_shape(m, n, k, m, k, m, t, t, c, comp)
off, adr = capi.br_config(capi.BR_OFFSET, 0, 0, 0), capi.br_config(capi.BR_ADDRESS, 0, 0, 0)
TA, TB, B0 = GEMM_FLAG.TRANS_A, GEMM_FLAG.TRANS_B, GEMM_FLAG.BETA_0
relu, none = lambda m, fl=0: capi.argops_cp(m, UNARY.RELU, fl), capi.no_argops()
MASK = UNARY_FLAG.BITMASK_2BYTEMULT
ext = api.dispatch_brgemm_ext
f64 = dict(t=DT.F64, c=DT.F64, comp=DT.F64)
H = dict(
    bias_relu=ext(sh(32), B0, 0, adr, relu(32), capi.postops_colbias(32, DT.F32)),
    mask=ext(sh(40, 24, 9), 0, 0, adr, relu(40, MASK), capi.no_postops()),
    bias_mask=ext(sh(13, 17, 29), B0, 0, adr, relu(13, MASK), capi.postops_colbias(13, DT.F32)),
    bf16_sigmoid=ext(sh(64, t=DT.BF16, c=DT.BF16), GEMM_FLAG.VNNI_A | B0, 0, adr, capi.argops_cp(64, UNARY.SIGMOID), capi.no_postops()),
    bf16f_bias=ext(sh(24, t=DT.BF16, c=DT.F32), 0, 0, adr, none, capi.postops_colbias(24, DT.F32)),
    free=ext(sh(32), B0, 0, adr, none, capi.no_postops()),
    f64_free=ext(sh(23, 19, 13, **f64), 0, 0, adr, none, capi.no_postops()),
    o_bias_relu=ext(sh(32), B0, 0, off, relu(32), capi.postops_colbias(32, DT.F32)),
    o_tn_mask=ext(sh(20), TA, 0, off, relu(20, MASK), capi.no_postops()),
    o_tt_bias_mask=ext(sh(13), TA | TB, 0, off, relu(13, MASK), capi.postops_colbias(13, DT.F32)),
    o_bf16_nt_sigmoid=ext(sh(64, t=DT.BF16, c=DT.BF16), GEMM_FLAG.VNNI_A | TB | B0, 0, off, capi.argops_cp(64, UNARY.SIGMOID), capi.no_postops()),
    o_bf16f_ta_bias=ext(sh(16, t=DT.BF16, c=DT.F32), TA, 0, off, none, capi.postops_colbias(16, DT.F32)),
    o_free=ext(sh(32), B0 | TB, 0, off, none, capi.no_postops()),
    o_f64_free=ext(sh(23, **f64), TA, 0, off, none, capi.no_postops()),
    plain=api.dispatch_brgemm(sh(32), B0, 0, adr),
    o_plain=api.dispatch_brgemm(sh(32), B0, 0, off),
    tpp=api.dispatch_meltw_unary(UNARY.IDENTITY, capi.UnaryShape(16, 16, 16, 16, DT.F32, DT.F32, DT.F32), 0),
    stride=ext(sh(24), 0, 0, capi.br_config(capi.BR_STRIDE, 24 * 24 * 4, 24 * 24 * 4, 0), relu(24), capi.no_postops()),
    adr_ta=ext(sh(20), TA, 0, adr, relu(20), capi.no_postops()),
    i8=ext(sh(32, t=DT.I8, c=DT.I32, comp=DT.I32), GEMM_FLAG.VNNI_A, 0, adr, none, capi.no_postops()),
    o_vnni_b=ext(sh(32, t=DT.BF16, c=DT.BF16), GEMM_FLAG.VNNI_B | TB, 0, off, relu(32), capi.no_postops()),
)
assert all(H.values()), H
# an f64 handle with ReLU has no handle at all: the dispatcher refuses it in the siblings' words before any entry could; the entries see NULL
f64_relu = ext(sh(23, **f64), 0, 0, adr, relu(23), capi.no_postops())
print("f64_relu_dispatch", 1 if f64_relu else 0)
err()
# never dereferenced on the host: validation reads none of the arrays, none of the bases and not the workspace
BLK, SEG, LA, LB, LC, LD, LM, WS, A, B, CC, D, M = (i << 20 for i in range(1, 14))
NS = 5
def run(tag, h, offsets=False, nb=3, ns=NS, param=True, blk=BLK, seg=SEG, la=LA, lb=LB, lc=LC, ld=LD, lm=LM, ws=WS, wsb=None, a=A, b=B, c=CC, d=None, m=None):
    need = api.hip_gemm_ext_batch_reduce_segments_sliced_workspace(h, ns)
    api.hip_clear_last_error()
    p = capi.GemmExtParam()
    if offsets:
        p.a.primary, p.b.primary, p.c.primary = a, b, c
    p.d.primary, p.c.secondary = d, m
    sys.stderr.write("MARK %%s begin\n" %% tag); sys.stderr.flush()
    fn = api.hip_gemm_ext_batch_reduce_segments_offsets_sliced if offsets else api.hip_gemm_ext_batch_reduce_segments_sliced
    fn(h, C.byref(p) if param else None, nb, blk, ns, seg, la, lb, lc, ld, lm, ws, need if wsb is None else need + wsb)
    sys.stderr.write("MARK %%s end\n" %% tag); sys.stderr.flush()
    print(tag, err())
br = H["bias_relu"]
run("null_param", br, param=False)
run("null_blk", br, blk=None)
run("null_c_list", br, lc=None)
run("null_seg", br, seg=None)
run("null_a_list", br, la=None)
run("null_b_list", br, lb=None)
run("null_ws", br, ws=None)
run("short_ws", br, wsb=-1)
run("no_bias", br, ld=None)                                                     # neither d_list nor param->d.primary
run("no_mask_list", H["mask"], lm=None)
run("no_mask_list_bias", H["bias_mask"], lm=None)
run("o_null_c_offs", H["o_bias_relu"], offsets=True, lc=None, d=D)
run("o_null_a_offs", H["o_bias_relu"], offsets=True, la=None, d=D)
run("o_null_a_base", H["o_bias_relu"], offsets=True, a=None, d=D)
run("o_null_c_base", H["o_bias_relu"], offsets=True, c=None, d=D)
run("o_short_ws", H["o_tn_mask"], offsets=True, wsb=-1, m=M)
run("o_no_bias_base", H["o_bias_relu"], offsets=True)                           # d_offs without param->d.primary
run("o_no_bias_base_shared", H["o_bias_relu"], offsets=True, ld=None)
run("o_no_mask_offs", H["o_tn_mask"], offsets=True, lm=None, m=M)
run("o_no_mask_base", H["o_tt_bias_mask"], offsets=True, d=D)
run("misaligned_ws", br, ws=WS + 8)
run("o_misaligned_ws", H["o_tn_mask"], offsets=True, ws=WS + 4, m=M)
run("unknown", 12345)
run("f64_relu", f64_relu)
for tag in ("plain", "tpp", "stride", "adr_ta", "i8"):
    run(tag, H[tag])
run("offset_handle", H["o_bias_relu"])
for tag in ("o_plain", "o_vnni_b"):
    run(tag, H[tag], offsets=True)
run("o_address_handle", br, offsets=True, d=D)
run("o_tpp", H["tpp"], offsets=True)
run("empty", br, nb=0, ns=0)
run("empty_null", br, nb=0, ns=0, param=False, blk=None, seg=None, la=None, lb=None, lc=None, ld=None, lm=None, ws=None)
# accepted: blocks without slices need neither the slices' arrays nor a workspace; the mask arguments are ignored without the bitmask flag, the bias arguments
# without a bias; d_list = NULL with param->d.primary is the shared bias
run("ok_no_slices", br, ns=0, seg=None, la=None, lb=None, ws=None, lm=None)
run("ok_bias_relu", br, lm=None)
run("ok_shared_bias", br, ld=None, lm=None, d=D)
run("ok_mask", H["mask"], ld=None)
run("ok_bias_mask", H["bias_mask"])
run("ok_bf16_sigmoid", H["bf16_sigmoid"], ld=None, lm=None)
run("ok_bf16f_bias", H["bf16f_bias"], lm=None)
run("ok_free", H["free"], ld=None, lm=None)
run("ok_f64_free", H["f64_free"], ld=None, lm=None)
run("ok_o_bias_relu", H["o_bias_relu"], offsets=True, lm=None, d=D)
run("ok_o_shared_bias", H["o_bias_relu"], offsets=True, ld=None, lm=None, d=D)
run("ok_o_tn_mask", H["o_tn_mask"], offsets=True, ld=None, m=M)
run("ok_o_tt_bias_mask", H["o_tt_bias_mask"], offsets=True, d=D, m=M)
run("ok_o_bf16_nt_sigmoid", H["o_bf16_nt_sigmoid"], offsets=True, ld=None, lm=None)
run("ok_o_bf16f_ta_bias", H["o_bf16f_ta_bias"], offsets=True, lm=None, d=D)
run("ok_o_free", H["o_free"], offsets=True, ld=None, lm=None)
run("ok_o_f64_free", H["o_f64_free"], offsets=True, ld=None, lm=None)
print("launches", api.hip_launch_count(0))
for tag in ("bias_relu", "f64_free", "bf16_sigmoid", "mask", "o_tn_mask"):
    print("query_" + tag, ",".join(str(api.hip_gemm_ext_batch_reduce_segments_sliced_workspace(H[tag], n)) for n in (0, 1, 5, 1000)))
print("query_clean", err())
for tag in ("plain", "tpp", "i8"):
    print("query_" + tag, api.hip_gemm_ext_batch_reduce_segments_sliced_workspace(H[tag], 5), err())
print("query_f64_relu", api.hip_gemm_ext_batch_reduce_segments_sliced_workspace(f64_relu, 5), err())
# the plain query keeps refusing ext handles
print("query_plain_entry", api.hip_gemm_batch_reduce_segments_sliced_workspace(br, 5), err())
"""

MINUS2 = {"null_param": "param is NULL but nblocks", "null_blk": "blk_ptr is NULL but nblocks", "null_c_list": "c_list is NULL but nblocks",
          "null_seg": "seg_ptr is NULL but nslices", "null_a_list": "a_list is NULL but nslices", "null_b_list": "b_list is NULL but nslices",
          "null_ws": "workspace is NULL but nslices", "short_ws": "workspace_bytes", "no_bias": "d_list and param->d.primary are both NULL",
          "no_mask_list": "mask_list is NULL", "no_mask_list_bias": "mask_list is NULL", "o_null_c_offs": "c_offs is NULL but nblocks",
          "o_null_a_offs": "a_offs is NULL but nslices", "o_null_a_base": "param->a.primary", "o_null_c_base": "param->c.primary", "o_short_ws": "workspace_bytes",
          "o_no_bias_base": "param->d.primary", "o_no_bias_base_shared": "param->d.primary", "o_no_mask_offs": "mask_offs is NULL", "o_no_mask_base": "param->c.secondary"}
MINUS3 = {"misaligned_ws": "not 16-byte aligned", "o_misaligned_ws": "not 16-byte aligned", "unknown": "unknown kernel handle", "f64_relu": "unknown kernel handle",
          "plain": "not an ext kernel", "tpp": "not a BRGEMM", "stride": "not an ADDRESS batch-reduce", "adr_ta": "transposed operands are not taken (NN only)",
          "i8": "operand types", "offset_handle": "not an ADDRESS batch-reduce", "o_plain": "not an ext kernel", "o_vnni_b": "VNNI layouts of B and C",
          "o_address_handle": "not an OFFSET batch-reduce", "o_tpp": "not a BRGEMM"}
ACCEPTED = ["ok_" + t for t in ("no_slices", "bias_relu", "shared_bias", "mask", "bias_mask", "bf16_sigmoid", "bf16f_bias", "free", "f64_free", "o_bias_relu",
                                "o_shared_bias", "o_tn_mask", "o_tt_bias_mask", "o_bf16_nt_sigmoid", "o_bf16f_ta_bias", "o_free", "o_f64_free")]
# (m, n, tile edge, bytes of an accumulator) of the handles whose workspace is queried
QUERIED = {"bias_relu": (32, 32, 32, 4), "f64_free": (23, 19, 16, 8), "bf16_sigmoid": (64, 64, 32, 4), "mask": (40, 24, 32, 4), "o_tn_mask": (20, 20, 32, 4)}


@pytest.fixture(scope="module")
def child():
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1")
    env.pop("LIBXSMM_VERBOSE", None)
    r = subprocess.run([sys.executable, "-c", VALIDATION_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_sliced_ext_entries_refusals_set_the_documented_error_codes(child):
    got = dict(ln.split() for ln in child.stdout.splitlines() if len(ln.split()) == 2 and not ln.startswith("query_"))
    want = {"empty": "0", "empty_null": "0", "launches": "0", "f64_relu_dispatch": "0"}               # nblocks == 0: nothing to do, no error
    want.update({tag: "-2" for tag in MINUS2})
    want.update({tag: "-3" for tag in MINUS3})
    want.update({tag: "-4" for tag in ACCEPTED})                                                       # accepted; then: no device
    assert got == want, child.stdout + child.stderr
    # a refused call prints exactly one error, the one that names the reason, and never reaches the device check
    for tag, words in list(MINUS2.items()) + list(MINUS3.items()):
        err = child.stderr.split(f"MARK {tag} begin\n")[1].split(f"MARK {tag} end\n")[0]
        lines = [ln for ln in err.splitlines() if "ERROR" in ln]
        assert len(lines) == 1 and words in lines[0] and "no HIP device" not in err, (tag, err)


def test_workspace_query_keeps_its_bounds_for_ext_handles(child):
    out = dict(ln.split(None, 1) for ln in child.stdout.splitlines() if ln.startswith("query_"))
    assert out["query_clean"] == "0"
    for tag, (m, n, t, asz) in QUERIED.items():
        sizes = [int(x) for x in out["query_" + tag].split(",")]
        for ns, got in zip((0, 1, 5, 1000), sizes):
            lo, hi = ns * m * n * asz, ns * (-(-m // t) * t) * (-(-n // t) * t) * asz
            assert got % 16 == 0 and lo <= got <= hi and (got == 0) == (ns == 0), (tag, ns, got, lo, hi)
    for tag in ("plain", "tpp", "i8", "f64_relu", "plain_entry"):                 # an ineligible handle: 0 and the handle's refusal
        assert out["query_" + tag].split() == ["0", "-3"], (tag, out["query_" + tag])


FORMS = {"NN": 0, "NT": GEMM_FLAG.TRANS_B}
M, N, K = 13, 17, 29
BLOCKS, PRODUCTS = [0, 1, 3], [3, 0, 1, 3]                                        # blocks of 0, 1 and 3 slices; slices of 0, 1 and 3 products


class _Host:
    """Host operands of one small sliced ext call: pools, lists, C, bias and prefilled mask blocks."""

    def __init__(self, mode, form, beta, gen, seed):
        flags = FORMS[form]
        br = capi.BR_ADDRESS if mode == "address" else capi.BR_OFFSET
        lda, ldb, ldc = M + 3, (N if flags & GEMM_FLAG.TRANS_B else K) + 2, M + 5
        self.mode = mode
        self.blk_ptr, self.seg_ptr = csr(BLOCKS), csr(PRODUCTS)
        total, npool = int(self.seg_ptr[-1]), 4
        self.case = case = GemmCase(M, N, K, lda=lda, ldb=ldb, ldc=ldc, flags=flags, beta=beta, br_type=br, br_count=1, seed=seed)
        rng = np.random.default_rng(seed)
        self.A, self.B = gen(rng, npool * case.a_elems), gen(rng, npool * case.b_elems)
        self.c0 = [gen(rng, case.c_elems) for _ in BLOCKS]
        self.bias = [gen(rng, M) for _ in BLOCKS]
        self.m0 = [rng.integers(0, 256, case.mask_bytes).astype(np.uint8) for _ in BLOCKS]
        ai, bi = rng.integers(0, npool, total), rng.integers(0, npool, total)
        self.oa, self.ob = (ai * case.a_elems * 4).astype(np.int64), (bi * case.b_elems * 4).astype(np.int64)
        self.la, self.lb = (self.oa + self.A.ctypes.data).view(np.uint64), (self.ob + self.B.ctypes.data).view(np.uint64)

    def param_of_slice(self, j):
        p = capi.GemmParam()
        r = int(self.seg_ptr[j]) * 8
        if self.mode == "address":
            p.a.primary, p.b.primary = self.la.ctypes.data + r, self.lb.ctypes.data + r
        else:
            p.a.primary, p.b.primary, p.a.secondary, p.b.secondary = self.A.ctypes.data, self.B.ctypes.data, self.oa.ctypes.data + r, self.ob.ctypes.data + r
        return p


def _ints(rng, n):
    return rng.integers(-2, 3, n).astype(np.float32)


def _tenths(rng, n):
    return ((np.floor(rng.random(n) * 10.0) - 4.0) / 10.0).astype(np.float32)


@pytest.mark.parametrize("mode,form", [("address", "NN"), ("offset", "NT")])
@pytest.mark.parametrize("exact", [True, False], ids=["fma-chain-on-integers", "plain-on-random"])
def test_definition_equals_the_reference_called_once_per_slice(mode, form, exact, reference):
    """f32 NN ADDRESS and NT OFFSET, bias + ReLU + bitmask and bias alone, beta 0 and 1.  The helper's result against the reference's C kernel called once per
    slice with beta = 0 into an m x n f32 block, followed here by the start value, the float32 adds in slice order, the mask and ReLU.  The fmaf chain rounds
    once per step where the reference's kernel rounds the product and the sum, so it is compared on small integers, where both are exact; on random values the
    helper runs the oracle's plain chain, which is the reference's bit for bit."""
    for beta in (0, 1):
        h = _Host(mode, form, beta, _ints if exact else _tenths, 40 + beta)
        case, pcase = h.case, partial_case(h.case)
        for colbias, act in ((True, 2), (True, 0), (False, 2), (False, 1)):
            gotc, gotm = sliced_fused_reference(case, beta, colbias, act, h.blk_ptr, h.seg_ptr, h.param_of_slice, h.c0, lambda b: h.bias[b], h.m0, fma=exact)
            for b, c in enumerate(h.c0):
                want = c.copy()
                view = want.reshape(N, case.ldc)[:, :M]
                acc = view.copy() if beta else np.zeros((N, M), dtype=np.float32)
                if colbias:
                    acc = (h.bias[b][None, :] + acc) if beta else np.repeat(h.bias[b][None, :], N, axis=0)
                for j in range(int(h.blk_ptr[b]), int(h.blk_ptr[b + 1])):
                    P = np.full(M * N, 5.0, dtype=np.float32)
                    cnt = C.c_ulonglong(int(h.seg_ptr[j + 1] - h.seg_ptr[j]))
                    p = h.param_of_slice(j)
                    p.c.primary, p.op.tertiary = P.ctypes.data, C.addressof(cnt)
                    rc = reference.lib.xref_reference_gemm(C.byref(p), pcase.shape(), pcase.flags, 0, pcase.brcfg())
                    assert rc == 0, f"the reference's dispatcher refuses {mode} {form}"
                    acc = acc + P.reshape(N, M)
                wantm = h.m0[b].copy()
                if act == 2:
                    rows = wantm.reshape(N, case.mask_ld // 8)
                    for j in range(N):
                        for i in range(M):
                            bit = 0 if acc[j, i] <= 0 else 1
                            rows[j, i // 8] = (int(rows[j, i // 8]) & ~(1 << (i % 8))) | (bit << (i % 8))
                if act:
                    acc = np.where(acc <= 0, np.float32(0.0), acc)
                view[:] = acc
                what = f"{mode} {form} beta={beta} colbias={colbias} act={act} block {b}"
                assert want.tobytes() == gotc[b].tobytes(), what
                assert wantm.tobytes() == gotm[b].tobytes(), what + ": mask"


@pytest.mark.parametrize("c_type", [DT.F32, DT.BF16], ids=["f32", "bf16"])
def test_blocks_without_slices_equal_the_ext_oracle_called_with_a_count_of_zero(c_type):
    """Every beta / bias / activation, sigmoid among them: C and mask of the helper's blocks without slices are bitwise what the ext oracle stores for count 0."""
    from helpers import rand_values
    a_type = DT.F32 if c_type == DT.F32 else DT.BF16
    orc = pyoracle.oracle()
    rng = np.random.default_rng(77)
    for beta in (0, 1):
        for colbias, act in ((False, 0), (True, 0), (True, 1), (False, 2), (True, 2), (False, 3), (True, 3)):
            case = GemmCase(M, N, K, a_type=a_type, c_type=c_type, ldc=M + 5, beta=beta, colbias=colbias, act=act, br_type=capi.BR_ADDRESS, br_count=1, seed=5)
            c0, bias = rand_values(rng, case.c_elems, c_type), rand_values(rng, M, c_type)
            m0 = rng.integers(0, 256, case.mask_bytes).astype(np.uint8)
            gotc, gotm = sliced_fused_reference(case, beta, colbias, act, csr([0]), csr([]), None, [c0], lambda b: bias, [m0])
            want, wantm = c0.copy(), m0.copy()
            p = capi.GemmExtParam() if case.ext else capi.GemmParam()
            cnt = C.c_ulonglong(0)
            empty = np.zeros(1, dtype=np.uint64)
            p.a.primary = p.b.primary = empty.ctypes.data
            p.c.primary, p.op.tertiary = want.ctypes.data, C.addressof(cnt)
            if colbias:
                p.d.primary = bias.ctypes.data
            if act == 2:
                p.c.secondary = wantm.ctypes.data
            orc.gemm(p, case.oracle_desc())
            what = f"beta={beta} colbias={colbias} act={act}"
            assert want.tobytes() == gotc[0].tobytes(), what
            assert wantm.tobytes() == gotm[0].tobytes(), what + ": mask"
