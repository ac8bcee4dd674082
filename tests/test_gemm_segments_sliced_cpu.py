"""The sliced segments entries (include/libxsmm_hip.h) without a GPU: the three symbols are exported and mirrored; in dry-run mode every documented refusal sets
its code -- one error line that names the reason -- before the missing device is noticed, accepted calls end with -4 and nothing launched, and the workspace
query keeps its bounds; and the CPU statement of the semantics (tests/segments_sliced_helpers.py) equals, bit for bit, the reference's own kernel called once
per slice with beta = 0 and added up in slice order."""
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
from segments_sliced_helpers import csr, f32_to_bf16, partial_case, sliced_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_mirrored(api):
    for name in ("libxsmm_hip_gemm_batch_reduce_segments_sliced_workspace", "libxsmm_hip_gemm_batch_reduce_segments_sliced",
                 "libxsmm_hip_gemm_batch_reduce_segments_offsets_sliced"):
        assert name in capi.declared_symbols() and hasattr(api.lib, name), name
    assert len(api.hip_gemm_batch_reduce_segments_sliced_workspace.argtypes) == 2 and api.hip_gemm_batch_reduce_segments_sliced_workspace.restype is C.c_size_t
    for fn in (api.hip_gemm_batch_reduce_segments_sliced, api.hip_gemm_batch_reduce_segments_offsets_sliced):
        assert len(fn.argtypes) == 11 and fn.restype is None


VALIDATION_CHILD = r"""
import sys
import ctypes as C
sys.path.insert(0, %(root)r)
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG, UNARY
api = capi.load()
def err():
    e = api.hip_get_last_error(); api.hip_clear_last_error(); return e
def sh(m, n=None, k=None, t=DT.F32, c=DT.F32, comp=DT.F32):
    n, k = n or m, k or m
    return capi.gemm_shape(m, n, k, m, k, m, t, t, c, comp)
off, adr = capi.br_config(capi.BR_OFFSET, 0, 0, 0), capi.br_config(capi.BR_ADDRESS, 0, 0, 0)
TA, TB = GEMM_FLAG.TRANS_A, GEMM_FLAG.TRANS_B
H = dict(
    f32=api.dispatch_brgemm(sh(32), GEMM_FLAG.BETA_0, 0, adr),
    f64=api.dispatch_brgemm(sh(23, 19, 13, DT.F64, DT.F64, DT.F64), 0, 0, adr),
    bf16=api.dispatch_brgemm(sh(64, t=DT.BF16, c=DT.BF16), GEMM_FLAG.VNNI_A | GEMM_FLAG.BETA_0, 0, adr),
    bf16_f32=api.dispatch_brgemm(sh(24, t=DT.BF16, c=DT.F32), 0, 0, adr),
    f32_ragged=api.dispatch_brgemm(sh(40, 24, 9), 0, 0, adr),
    o_nn=api.dispatch_brgemm(sh(32), GEMM_FLAG.BETA_0, 0, off),
    o_tn=api.dispatch_brgemm(sh(32), TA, 0, off),
    o_nt=api.dispatch_brgemm(sh(20), TB | GEMM_FLAG.BETA_0, 0, off),
    o_tt=api.dispatch_brgemm(sh(13), TA | TB, 0, off),
    o_f64_tn=api.dispatch_brgemm(sh(23, t=DT.F64, c=DT.F64, comp=DT.F64), TA, 0, off),
    o_bf16_ta=api.dispatch_brgemm(sh(64, t=DT.BF16, c=DT.BF16), TA | GEMM_FLAG.BETA_0, 0, off),
    plain=api.dispatch_gemm(sh(32), GEMM_FLAG.BETA_0, 0),
    stride=api.dispatch_brgemm(sh(24), 0, 0, capi.br_config(capi.BR_STRIDE, 24 * 24 * 4, 24 * 24 * 4, 0)),
    adr_ta=api.dispatch_brgemm(sh(20), TA, 0, adr),
    i8=api.dispatch_brgemm(sh(32, t=DT.I8, c=DT.I32, comp=DT.I32), GEMM_FLAG.VNNI_A, 0, adr),
    o_vnni_b=api.dispatch_brgemm(sh(32, t=DT.BF16, c=DT.BF16), GEMM_FLAG.VNNI_B | TB, 0, off),
    ext=api.dispatch_brgemm_ext(sh(32), 0, 0, adr, capi.argops_cp(32, UNARY.RELU), capi.no_postops()),
    o_ext=api.dispatch_brgemm_ext(sh(32), 0, 0, off, capi.argops_cp(32, UNARY.RELU), capi.no_postops()),
    tpp=api.dispatch_meltw_unary(UNARY.IDENTITY, capi.UnaryShape(16, 16, 16, 16, DT.F32, DT.F32, DT.F32), 0),
)
assert all(H.values()), H
# never dereferenced on the host: validation reads none of the arrays, none of the bases and not the workspace
BLK, SEG, LA, LB, LC, WS, A, B, CC = (i << 20 for i in range(1, 10))
NS = 5
def run(tag, h, offsets=False, nb=3, ns=NS, param=True, blk=BLK, seg=SEG, la=LA, lb=LB, lc=LC, ws=WS, wsb=None, a=A, b=B, c=CC, mark=True):
    need = api.hip_gemm_batch_reduce_segments_sliced_workspace(h, ns)
    api.hip_clear_last_error()
    p = capi.GemmParam()
    if offsets:
        p.a.primary, p.b.primary, p.c.primary = a, b, c
    sys.stderr.write("MARK %%s begin\n" %% tag); sys.stderr.flush()
    fn = api.hip_gemm_batch_reduce_segments_offsets_sliced if offsets else api.hip_gemm_batch_reduce_segments_sliced
    fn(h, C.byref(p) if param else None, nb, blk, ns, seg, la, lb, lc, ws, need if wsb is None else need + wsb)
    sys.stderr.write("MARK %%s end\n" %% tag); sys.stderr.flush()
    print(tag, err())
f32 = H["f32"]
run("null_param", f32, param=False)
run("null_blk", f32, blk=None)
run("null_c_list", f32, lc=None)
run("null_seg", f32, seg=None)
run("null_a_list", f32, la=None)
run("null_b_list", f32, lb=None)
run("null_ws", f32, ws=None)
run("short_ws", f32, wsb=-1)
run("o_null_c_offs", H["o_nn"], offsets=True, lc=None)
run("o_null_a_offs", H["o_nn"], offsets=True, la=None)
run("o_null_a_base", H["o_nn"], offsets=True, a=None)
run("o_null_b_base", H["o_nn"], offsets=True, b=None)
run("o_null_c_base", H["o_nn"], offsets=True, c=None)
run("o_short_ws", H["o_tn"], offsets=True, wsb=-1)
run("misaligned_ws", f32, ws=WS + 8)
run("o_misaligned_ws", H["o_nt"], offsets=True, ws=WS + 4)
run("unknown", 12345)
for tag in ("tpp", "ext", "plain", "stride", "adr_ta", "i8"):
    run(tag, H[tag])
run("offset_handle", H["o_nn"])
for tag in ("o_ext", "o_vnni_b"):
    run(tag, H[tag], offsets=True)
run("o_address_handle", f32, offsets=True)
run("o_tpp", H["tpp"], offsets=True)
run("empty", f32, nb=0, ns=0)
run("empty_null", f32, nb=0, ns=0, param=False, blk=None, seg=None, la=None, lb=None, lc=None, ws=None)
run("no_slices", f32, ns=0, seg=None, la=None, lb=None, ws=None)               # blocks without slices need neither the slices' arrays nor a workspace
for tag in ("f32", "f64", "bf16", "bf16_f32", "f32_ragged"):
    run("ok_" + tag, H[tag])
for tag in ("o_nn", "o_tn", "o_nt", "o_tt", "o_f64_tn", "o_bf16_ta"):
    run("ok_" + tag, H[tag], offsets=True)
print("launches", api.hip_launch_count(0))
for tag in ("f32", "f64", "bf16", "f32_ragged", "o_tn"):
    print("query_" + tag, ",".join(str(api.hip_gemm_batch_reduce_segments_sliced_workspace(H[tag], n)) for n in (0, 1, 5, 1000)))
print("query_clean", err())
for tag in ("ext", "plain", "tpp", "i8"):
    print("query_" + tag, api.hip_gemm_batch_reduce_segments_sliced_workspace(H[tag], 5), err())
"""

MINUS2 = {"null_param": "param is NULL but nblocks", "null_blk": "blk_ptr is NULL but nblocks", "null_c_list": "c_list is NULL but nblocks",
          "null_seg": "seg_ptr is NULL but nslices", "null_a_list": "a_list is NULL but nslices", "null_b_list": "b_list is NULL but nslices",
          "null_ws": "workspace is NULL but nslices", "short_ws": "workspace_bytes", "o_null_c_offs": "c_offs is NULL but nblocks",
          "o_null_a_offs": "a_offs is NULL but nslices", "o_null_a_base": "param->a.primary", "o_null_b_base": "param->b.primary", "o_null_c_base": "param->c.primary",
          "o_short_ws": "workspace_bytes"}
MINUS3 = {"misaligned_ws": "not 16-byte aligned", "o_misaligned_ws": "not 16-byte aligned", "unknown": "unknown kernel handle", "tpp": "not a BRGEMM",
          "ext": "ext handles", "plain": "not an ADDRESS batch-reduce", "stride": "not an ADDRESS batch-reduce", "adr_ta": "transposed operands are not taken (NN only)",
          "i8": "operand types", "offset_handle": "not an ADDRESS batch-reduce", "o_ext": "ext handles",
          "o_vnni_b": "VNNI layouts of B and C", "o_address_handle": "not an OFFSET batch-reduce", "o_tpp": "not a BRGEMM"}
ACCEPTED = ["no_slices"] + ["ok_" + t for t in ("f32", "f64", "bf16", "bf16_f32", "f32_ragged", "o_nn", "o_tn", "o_nt", "o_tt", "o_f64_tn", "o_bf16_ta")]
# (m, n, tile edge, bytes of an accumulator) of the handles whose workspace is queried
QUERIED = {"f32": (32, 32, 32, 4), "f64": (23, 19, 16, 8), "bf16": (64, 64, 32, 4), "f32_ragged": (40, 24, 32, 4), "o_tn": (32, 32, 32, 4)}


@pytest.fixture(scope="module")
def child():
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1")
    env.pop("LIBXSMM_VERBOSE", None)
    r = subprocess.run([sys.executable, "-c", VALIDATION_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_sliced_entries_refusals_set_the_documented_error_codes(child):
    got = dict(ln.split() for ln in child.stdout.splitlines() if len(ln.split()) == 2 and not ln.startswith("query_"))
    want = {"empty": "0", "empty_null": "0", "launches": "0"}                                          # nblocks == 0: nothing to do, no error
    want.update({tag: "-2" for tag in MINUS2})
    want.update({tag: "-3" for tag in MINUS3})
    want.update({tag: "-4" for tag in ACCEPTED})                                                       # accepted; then: no device
    assert got == want, child.stdout + child.stderr
    # a refused call prints exactly one error, the one that names the reason, and never reaches the device check (a short or misaligned workspace among them)
    for tag, words in list(MINUS2.items()) + list(MINUS3.items()):
        err = child.stderr.split(f"MARK {tag} begin\n")[1].split(f"MARK {tag} end\n")[0]
        lines = [ln for ln in err.splitlines() if "ERROR" in ln]
        assert len(lines) == 1 and words in lines[0] and "no HIP device" not in err, (tag, err)


def test_workspace_query_keeps_its_bounds(child):
    out = dict(ln.split(None, 1) for ln in child.stdout.splitlines() if ln.startswith("query_"))
    assert out["query_clean"] == "0"
    for tag, (m, n, t, asz) in QUERIED.items():
        sizes = [int(x) for x in out["query_" + tag].split(",")]
        for ns, got in zip((0, 1, 5, 1000), sizes):
            lo, hi = ns * m * n * asz, ns * (-(-m // t) * t) * (-(-n // t) * t) * asz
            assert got % 16 == 0 and lo <= got <= hi and (got == 0) == (ns == 0), (tag, ns, got, lo, hi)
    for tag in ("ext", "plain", "tpp", "i8"):                                     # an ineligible handle: 0 and the handle's refusal
        assert out["query_" + tag].split() == ["0", "-3"], (tag, out["query_" + tag])


def test_helper_bf16_conversion_is_the_oracles():
    orc = pyoracle.oracle()
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(2000).astype(np.float32), rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        np.array([0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf, 3.3895314e38, 1.0039062, 1.0117188], dtype=np.float32)])
    x = x[~np.isnan(x)]
    want = np.array([orc.lib.oracle_f32_to_bf16_rne(float(v)) for v in x], dtype=np.uint16)
    assert np.array_equal(f32_to_bf16(x), want)


FORMS = {"NN": 0, "NT": GEMM_FLAG.TRANS_B}
M, N, K = 13, 17, 29
BLOCKS, PRODUCTS = [0, 1, 3], [3, 0, 1, 3]                                        # blocks of 0, 1 and 3 slices; slices of 0, 1 and 3 products


@pytest.mark.parametrize("mode,form", [("address", "NN"), ("offset", "NN"), ("offset", "NT")])
@pytest.mark.parametrize("exact", [True, False], ids=["fma-chain-on-integers", "plain-on-random"])
def test_definition_equals_the_reference_called_once_per_slice(mode, form, exact, reference):
    """f32 NN and NT.  The helper's result -- per-slice chains from +0, numpy.float32 adds in slice order, then beta -- against the reference's C kernel called once
    per slice with beta = 0 into an m x n f32 block and the same adds.  The fmaf chain rounds once per step where the reference's kernel rounds the product and the
    sum, so it is compared on small integers, where both are exact; on random values the helper runs the oracle's plain chain, which is the reference's bit for bit."""
    flags = FORMS[form]
    br = capi.BR_ADDRESS if mode == "address" else capi.BR_OFFSET
    lda, ldb, ldc = M + 3, (N if flags & GEMM_FLAG.TRANS_B else K) + 2, M + 5
    blk_ptr, seg_ptr = csr(BLOCKS), csr(PRODUCTS)
    total, npool = int(seg_ptr[-1]), 4
    for beta in (0, 1):
        case = GemmCase(M, N, K, lda=lda, ldb=ldb, ldc=ldc, flags=flags, beta=beta, br_type=br, br_count=1, seed=40 + beta)
        rng = np.random.default_rng(7 + beta)
        gen = (lambda n: rng.integers(-2, 3, n).astype(np.float32)) if exact else (lambda n: ((np.floor(rng.random(n) * 10.0) - 4.0) / 10.0).astype(np.float32))
        A, B = gen(npool * case.a_elems), gen(npool * case.b_elems)
        c0 = [gen(case.c_elems) for _ in BLOCKS]
        ai, bi = rng.integers(0, npool, total), rng.integers(0, npool, total)
        oa, ob = (ai * case.a_elems * 4).astype(np.int64), (bi * case.b_elems * 4).astype(np.int64)
        la, lb = (oa + A.ctypes.data).view(np.uint64), (ob + B.ctypes.data).view(np.uint64)

        def param_of_slice(j):
            p = capi.GemmParam()
            r = int(seg_ptr[j]) * 8
            if mode == "address":
                p.a.primary, p.b.primary = la.ctypes.data + r, lb.ctypes.data + r
            else:
                p.a.primary, p.b.primary, p.a.secondary, p.b.secondary = A.ctypes.data, B.ctypes.data, oa.ctypes.data + r, ob.ctypes.data + r
            return p

        got = sliced_reference(case, beta, blk_ptr, seg_ptr, param_of_slice, c0, fma=exact)
        pcase = partial_case(case)
        for b, c in enumerate(c0):
            want = c.copy()
            j0, j1 = int(blk_ptr[b]), int(blk_ptr[b + 1])
            if j1 > j0 or not beta:
                view = want.reshape(N, ldc)[:, :M]
                acc = view.copy() if beta else np.zeros((N, M), dtype=np.float32)
                for j in range(j0, j1):
                    P = np.full(M * N, 5.0, dtype=np.float32)
                    cnt = C.c_ulonglong(int(seg_ptr[j + 1] - seg_ptr[j]))
                    p = param_of_slice(j)
                    p.c.primary, p.op.tertiary = P.ctypes.data, C.addressof(cnt)
                    rc = reference.lib.xref_reference_gemm(C.byref(p), pcase.shape(), pcase.flags, 0, pcase.brcfg())
                    assert rc == 0, f"the reference's dispatcher refuses {mode} {form}"
                    acc = acc + P.reshape(N, M)
                view[:] = acc
            assert want.tobytes() == got[b].tobytes(), f"{mode} {form} beta={beta} block {b}"
