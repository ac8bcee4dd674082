"""libxsmm_hip_gemm_batch_reduce_segments_offsets (include/libxsmm_hip.h): segments through OFFSET batch-reduce handles -- three bases and signed byte offsets
instead of absolute block pointers -- with A and / or B transposed, the backward passes of a block-sparse layer.  f32 segments are bitwise the oracle's (product,
k)-ordered fmaf chain in all four forms, f64 and bf16 segments lie within the dense kernels' tolerances and are bitwise on exact data; NN equals the ADDRESS entry
bit for bit; one set of offset lists serves two copies of the operands; the call equals its loop of single OFFSET calls; one call is one launch; the launch modes
keep the results; the grid-stride holds at scale; a layer's Y, dX and dW are one call each.  The last test re-runs the parity and scale tests with every operand
flush against unmapped memory (run this file with -x)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import helpers
from helpers import GemmCase, NP_OF, TOL_BF16, TOL_F64, normf_rel
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG
from oracle import pyoracle
from test_gemm_segments_gpu import COUNTS, Pool, _down, _ints, _same, _up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

TA, TB = GEMM_FLAG.TRANS_A, GEMM_FLAG.TRANS_B
FORMS = {"NN": 0, "TN": TA, "NT": TB, "TT": TA | TB}


def _offs(ptrs, base):
    """Signed byte offsets of absolute addresses from `base`."""
    return ptrs.view(np.int64) - np.int64(base)


class OffsetSegments:
    """One offsets call: pools of A and B blocks, one C block per segment and the CSR-style offset lists -- on the host for the oracle and on the device.  The base
    of every operand is its pool's main array; the pool's LAST block is an allocation of its own, so its offset is large and may be negative.  `shared_only`
    keeps every listed block inside the main arrays: the offset lists then do not depend on where the pools lie."""

    def __init__(self, api, m, n, k, form="NN", counts=COUNTS, a_type=DT.F32, c_type=None, flags=0, beta=0, pads=(0, 0, 0), seed=0, exact=False, npool=9,
                 shared_only=False):
        self.api = api
        flags |= FORMS[form]
        lda, ldb, ldc = (k if flags & TA else m) + pads[0], (n if flags & TB else k) + pads[1], m + pads[2]      # lda >= k under TRANS_A, ldb >= n under TRANS_B
        self.case = case = GemmCase(m, n, k, a_type=a_type, c_type=c_type, lda=lda, ldb=ldb, ldc=ldc, flags=flags, beta=beta,
                                    br_type=capi.BR_OFFSET, br_count=1, batch=1, seed=seed)
        rng = np.random.default_rng(1000 + seed)
        gen = _ints if exact else helpers.rand_values
        self.counts = np.asarray(counts, dtype=np.uint64)
        self.nseg = len(self.counts)
        self.seg_ptr = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.uint64)
        total = int(self.seg_ptr[-1])
        ncb = self.nseg + (1 if shared_only else 0)                               # (shared_only: the C pool's own last block is not a segment's)
        self.A = Pool(gen(rng, Pool.size(npool, case.a_elems), a_type), npool, case.a_elems)
        self.B = Pool(gen(rng, Pool.size(npool, case.b_elems), case.b_type), npool, case.b_elems)
        self.C0 = Pool(gen(rng, Pool.size(ncb, case.c_elems), case.c_type), ncb, case.c_elems)
        seg_of = np.repeat(np.arange(self.nseg), self.counts.astype(np.int64))
        r_of = np.arange(total) - self.seg_ptr[seg_of].astype(np.int64)
        used = npool - 1 if shared_only else npool
        self.ai = (seg_of * 3 + r_of) % used                                      # A blocks are shared across segments ...
        self.bi = np.where(seg_of % 2 == 0, seg_of % used, (seg_of + r_of) % used)     # ... and even segments use ONE B for all their products
        self.dA, self.dB = self.A.upload(), self.B.upload()
        self.oa = _offs(self.A.dev_ptrs(self.dA, self.ai), self.dA[0].data_ptr())
        self.ob = _offs(self.B.dev_ptrs(self.dB, self.bi), self.dB[0].data_ptr())
        self.d_seg, self.d_oa, self.d_ob = _up(self.seg_ptr), _up(self.oa), _up(self.ob)
        self.handle = case.dispatch(api)
        assert self.handle

    def new_c(self):
        """A fresh device copy of the C blocks and their offsets from its main array."""
        dC = self.C0.upload()
        oc = _offs(self.C0.dev_ptrs(dC, range(self.nseg)), dC[0].data_ptr())
        return dC, _up(oc), oc

    def run(self, cset, dA=None, dB=None):
        p = capi.GemmParam()
        p.a.primary, p.b.primary, p.c.primary = (dA or self.dA)[0].data_ptr(), (dB or self.dB)[0].data_ptr(), cset[0][0].data_ptr()
        self.api.hip_gemm_batch_reduce_segments_offsets(self.handle, C.byref(p), self.nseg, self.d_seg.data_ptr(), self.d_oa.data_ptr(), self.d_ob.data_ptr(),
                                                        cset[1].data_ptr())

    def run_checked(self):
        cset = self.new_c()
        self.run(cset)
        self.api.hip_sync(); self.api.check()
        return self.C0.download(cset[0])

    def run_loop(self):
        """The loop the call replaces: one blocking single OFFSET call of the same handle per segment."""
        dC, _, oc = self.new_c()
        for s in range(self.nseg):
            p = capi.GemmParam()
            cnt = C.c_ulonglong(int(self.counts[s]))
            p.a.primary, p.b.primary = self.dA[0].data_ptr(), self.dB[0].data_ptr()
            p.a.secondary = self.d_oa.data_ptr() + int(self.seg_ptr[s]) * 8
            p.b.secondary = self.d_ob.data_ptr() + int(self.seg_ptr[s]) * 8
            p.c.primary = dC[0].data_ptr() + int(oc[s]); p.op.tertiary = C.addressof(cnt)
            capi.Api.call(self.handle, p)
        self.api.hip_sync(); self.api.check()
        return self.C0.download(dC)

    def run_address(self):
        """The same blocks through the ADDRESS entry: pointer lists = base + offset (NN only)."""
        c = self.case
        adr = GemmCase(c.m, c.n, c.k, a_type=c.a_type, c_type=c.c_type, lda=c.lda, ldb=c.ldb, ldc=c.ldc, flags=c.flags & ~GEMM_FLAG.BETA_0,
                       beta=0 if c.flags & GEMM_FLAG.BETA_0 else 1, br_type=capi.BR_ADDRESS, br_count=1, batch=1).dispatch(self.api)
        assert adr
        dC, _, oc = self.new_c()
        la = _up((self.oa + np.int64(self.dA[0].data_ptr())).view(np.uint64))
        lb = _up((self.ob + np.int64(self.dB[0].data_ptr())).view(np.uint64))
        lc = _up((oc + np.int64(dC[0].data_ptr())).view(np.uint64))
        p = capi.GemmParam()
        self.api.hip_gemm_batch_reduce_segments(adr, C.byref(p), self.nseg, self.d_seg.data_ptr(), la.data_ptr(), lb.data_ptr(), lc.data_ptr())
        self.api.hip_sync(); self.api.check()
        return self.C0.download(dC)

    def oracle(self, fma=False):
        orc, d = pyoracle.oracle(), self.case.oracle_desc()
        ref = self.C0.copy()
        oa = _offs(self.A.host_ptrs(self.ai), self.A.host[0].ctypes.data)
        ob = _offs(self.B.host_ptrs(self.bi), self.B.host[0].ctypes.data)
        oc = _offs(ref.host_ptrs(range(self.nseg)), ref.host[0].ctypes.data)
        for s in range(self.nseg):
            p = capi.GemmParam()
            cnt = C.c_ulonglong(int(self.counts[s]))                            # the oracle accepts a count of 0
            p.a.primary, p.b.primary = self.A.host[0].ctypes.data, self.B.host[0].ctypes.data
            p.a.secondary = oa.ctypes.data + int(self.seg_ptr[s]) * 8
            p.b.secondary = ob.ctypes.data + int(self.seg_ptr[s]) * 8
            p.c.primary = ref.host[0].ctypes.data + int(oc[s]); p.op.tertiary = C.addressof(cnt)
            orc.gemm(p, d, fma=fma)
        return ref.host

    def valid(self, arrays, s):
        c = self.case
        return self.C0.block(arrays, s)[:c.ldc * c.n].reshape(c.n, c.ldc)[:, :c.m]

    def assert_padding_untouched(self, got, what):
        c = self.case
        for s in range(self.nseg):
            g = self.C0.block(got, s)[:c.ldc * c.n].reshape(c.n, c.ldc)[:, c.m:]
            assert np.array_equal(g, self.C0.block(self.C0.host, s)[:c.ldc * c.n].reshape(c.n, c.ldc)[:, c.m:]), f"{what}: segment {s} wrote beyond m x n"
        for a, b in zip(got, self.C0.host):                                       # the elements between the blocks
            if len(a) > c.c_elems:
                assert np.array_equal(a[c.c_elems::c.c_elems + 1], b[c.c_elems::c.c_elems + 1]), what


F32_SHAPES = [dict(m=32, n=32, k=32), dict(m=16, n=16, k=16), dict(m=13, n=17, k=29), dict(m=13, n=13, k=13), dict(m=40, n=40, k=40), dict(m=9, n=5, k=3),
              dict(m=20, n=24, k=18, pads=(3, 3, 9))]          # (NN: lda, ldb, ldc = 23, 21, 29; the transposed forms keep the same padding past k / n)


@pytest.mark.parametrize("form", list(FORMS))
def test_f32_offset_segments_are_bitwise_the_fma_chain(form):
    api = capi.load()
    for i, kw in enumerate(F32_SHAPES):
        for beta in (0, 1):
            sg = OffsetSegments(api, form=form, beta=beta, seed=10 * i + beta, **kw)
            got, ref = sg.run_checked(), sg.oracle(fma=True)
            # whole arrays: the m x n blocks are the (product, k)-ordered fmaf chain bit for bit, and the padding of C beyond m x n is unchanged
            assert _same(got, ref), f"{form} {kw} beta={beta}: differs from the (product, k)-ordered fmaf chain (or wrote outside m x n)"
            for s in np.flatnonzero(sg.counts == 0):                              # empty segments: +0 under beta = 0, untouched under beta = 1
                v = sg.valid(got, s)
                want = sg.valid(sg.C0.host, s) if beta else np.zeros_like(v)
                assert np.array_equal(v.view(np.uint32), want.view(np.uint32)), f"{form} {kw} beta={beta}: empty segment {s}"


F64_SHAPES = [dict(m=16, n=16, k=16), dict(m=23, n=23, k=23), dict(m=8, n=40, k=5), dict(m=20, n=24, k=18, pads=(3, 3, 9))]


@pytest.mark.parametrize("form", list(FORMS))
def test_f64_offset_segments_match_the_oracle(form):
    api = capi.load()
    for i, kw in enumerate(F64_SHAPES):
        for beta in (0, 1):
            sg = OffsetSegments(api, form=form, a_type=DT.F64, beta=beta, seed=100 + 10 * i + beta, **kw)
            got, ref = sg.run_checked(), sg.oracle()
            for s in range(sg.nseg):
                err = normf_rel(sg.valid(ref, s), sg.valid(got, s), DT.F64)
                assert err < TOL_F64, f"{form} {kw} beta={beta} segment {s} (count {sg.counts[s]}): normf_rel = {err}"
            sg.assert_padding_untouched(got, f"{form} {kw} beta={beta}")
            ex = OffsetSegments(api, form=form, a_type=DT.F64, beta=beta, seed=150 + 10 * i + beta, exact=True, **kw)
            assert _same(ex.run_checked(), ex.oracle()), f"{form} {kw} beta={beta}: exact data differs from the oracle"


# (A layout, form): flat A x flat B, VNNI A x flat B, TRANS_A x flat B, flat A x TRANS_B, VNNI A x TRANS_B, TRANS_A x TRANS_B
BF16_FORMS = {"flat-N": (0, "NN"), "vnni-N": (GEMM_FLAG.VNNI_A, "NN"), "T-N": (0, "TN"), "flat-T": (0, "NT"), "vnni-T": (GEMM_FLAG.VNNI_A, "NT"), "T-T": (0, "TT")}
BF16_SHAPES = [dict(m=32, n=32, k=32), dict(m=16, n=16, k=16, beta=1), dict(m=13, n=17, k=29), dict(m=64, n=64, k=64), dict(m=24, n=40, k=34, pads=(3, 3, 6), beta=1)]


@pytest.mark.parametrize("name", list(BF16_FORMS))
def test_bf16_offset_segments_match_the_oracle(name):
    api = capi.load()
    flags, form = BF16_FORMS[name]
    for i, kw in enumerate(BF16_SHAPES):
        if flags & GEMM_FLAG.VNNI_A and kw["k"] % 2:
            continue                                                              # VNNI-2 pairs k: no handle exists for an odd k
        for c_type in (DT.BF16, DT.F32):
            sg = OffsetSegments(api, form=form, a_type=DT.BF16, c_type=c_type, flags=flags, seed=200 + i, **kw)
            got, ref = sg.run_checked(), sg.oracle()
            for s in range(sg.nseg):                                              # (count-0 segments with bf16 C included)
                err = normf_rel(sg.valid(ref, s), sg.valid(got, s), sg.case.c_type)
                assert err < TOL_BF16, f"{name} {kw} -> {c_type} segment {s} (count {sg.counts[s]}): normf_rel = {err}"
            sg.assert_padding_untouched(got, f"{name} {kw} -> {c_type}")
            ex = OffsetSegments(api, form=form, a_type=DT.BF16, c_type=c_type, flags=flags, seed=250 + i, exact=True, **kw)
            got = ex.run_checked()
            assert _same(got, ex.oracle()), f"{name} {kw} -> {c_type}: exact data differs from the oracle"
            ex.assert_padding_untouched(got, f"{name} {kw} -> {c_type} (exact)")


NN_CASES = [dict(m=32, n=32, k=32), dict(m=13, n=17, k=29, beta=1), dict(m=20, n=24, k=18, pads=(3, 3, 9)), dict(m=23, n=23, k=23, a_type=DT.F64, beta=1),
            dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A), dict(m=24, n=40, k=34, a_type=DT.BF16, c_type=DT.F32, pads=(3, 3, 6), beta=1)]


def test_nn_equals_the_address_entry_bit_for_bit():
    api = capi.load()
    for i, kw in enumerate(NN_CASES):
        sg = OffsetSegments(api, seed=280 + i, **kw)                              # random data: the same blocks, the same chain, the same bits
        assert _same(sg.run_checked(), sg.run_address()), f"{kw}: differs from libxsmm_hip_gemm_batch_reduce_segments on base + offset"


def test_one_set_of_offset_lists_serves_two_copies_of_the_operands():
    api = capi.load()
    for i, kw in enumerate((dict(m=32, n=32, k=32, form="TN"), dict(m=13, n=17, k=29, form="NT", beta=1), dict(m=24, n=40, k=34, a_type=DT.BF16, form="TT"))):
        sg = OffsetSegments(api, seed=290 + i, shared_only=True, **kw)
        first = sg.new_c()
        dA2, dB2, dC2 = sg.A.upload(), sg.B.upload(), sg.C0.upload()              # second copies while the first are alive: other addresses
        assert dA2[0].data_ptr() != sg.dA[0].data_ptr() and dB2[0].data_ptr() != sg.dB[0].data_ptr() and dC2[0].data_ptr() != first[0][0].data_ptr()
        sg.run(first)
        sg.run((dC2, first[1]), dA=dA2, dB=dB2)                                   # the SAME four device lists, three other bases
        api.hip_sync(); api.check()
        got1, got2 = sg.C0.download(first[0]), sg.C0.download(dC2)
        assert _same(got1, got2), f"{kw}: the result depends on where the operands lie"
        if sg.case.a_type == DT.F32:
            assert _same(got1, sg.oracle(fma=True)), kw
        for dev, host in ((sg.d_seg, sg.seg_ptr), (sg.d_oa, sg.oa), (sg.d_ob, sg.ob), (first[1], first[2])):
            assert np.array_equal(_down(dev, host), host), "an offset list changed"


LOOP_CASES = [dict(m=32, n=32, k=32), dict(m=13, n=17, k=29, beta=1, form="TN"), dict(m=20, n=24, k=18, pads=(3, 3, 9), form="NT"),
              dict(m=23, n=23, k=23, a_type=DT.F64, form="TN"), dict(m=16, n=16, k=16, a_type=DT.F64, beta=1, form="NT"),
              dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, form="NT"),
              dict(m=24, n=40, k=34, a_type=DT.BF16, c_type=DT.F32, beta=1, form="TN"), dict(m=13, n=13, k=13, form="TT", beta=1)]


def test_the_call_equals_its_loop_of_single_offset_calls():
    api = capi.load()
    for i, kw in enumerate(LOOP_CASES):
        sg = OffsetSegments(api, seed=300 + i, exact=True, **kw)                  # (the single OFFSET call takes a count of 0: the empty segments take part)
        assert _same(sg.run_checked(), sg.run_loop()), f"{kw}: differs from the loop of single OFFSET calls through the same handle"


def test_one_launch_per_call_through_the_new_kernels():
    api = capi.load()
    for kw, name in ((dict(m=32, n=32, k=32, form="TN"), b"gemm_segments_offs_f32_kernel<1,0>"), (dict(m=23, n=23, k=23, a_type=DT.F64, form="NT"), b"gemm_segments_offs_f64_kernel<0,1>"),
                     (dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A), b"gemm_segments_offs_bf16_kernel<0,0>")):
        sg = OffsetSegments(api, seed=400, **kw)
        cset = sg.new_c()
        api.hip_launch_count(1)
        sg.run(cset)
        assert api.hip_launch_count(1) == 1
        api.hip_sync(); api.check()
        assert api.hip_kernel_name(sg.handle, 1) == name


def _scale(api, nseg, edge, form, beta, seed):
    """`nseg` f32 segments of edge^3 with skewed counts (1 %: 64, a few empty, the rest 2) on exact data, every segment against a numpy integer sum."""
    rng = np.random.default_rng(seed)
    npool, e2 = 16, edge * edge
    counts = np.where(rng.random(nseg) < 0.01, 64, 2).astype(np.uint64)
    counts[::997] = 0
    seg_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    total = int(seg_ptr[-1])
    ai, bi = rng.integers(0, npool, total), rng.integers(0, npool, total)
    A, B = _ints(rng, npool * e2, DT.F32), _ints(rng, npool * e2, DT.F32)
    C0 = _ints(rng, nseg * e2, DT.F32)
    dA, dB, dC = _up(A), _up(B), _up(C0.copy())
    lists = [_up(seg_ptr), _up((ai * e2 * 4).astype(np.int64)), _up((bi * e2 * 4).astype(np.int64)), _up(np.arange(nseg, dtype=np.int64) * (e2 * 4))]
    h = GemmCase(edge, edge, edge, flags=FORMS[form], beta=beta, br_type=capi.BR_OFFSET, br_count=1, batch=1).dispatch(api)
    assert h
    p = capi.GemmParam()
    p.a.primary, p.b.primary, p.c.primary = dA.data_ptr(), dB.data_ptr(), dC.data_ptr()
    api.hip_launch_count(1)
    api.hip_gemm_batch_reduce_segments_offsets(h, C.byref(p), nseg, *[x.data_ptr() for x in lists])
    assert api.hip_launch_count(1) == 1
    api.hip_sync(); api.check()
    got = _down(dC, C0).reshape(nseg, e2)
    # blocks in memory order: flat A is [k][i], TRANS_A [i][k]; flat B is [j][k], TRANS_B [k][j]; C is [j][i]
    Am, Bm = A.reshape(npool, edge, edge).astype(np.int32), B.reshape(npool, edge, edge).astype(np.int32)
    sub = ("bkj" if FORMS[form] & TB else "bjk") + "," + ("aik" if FORMS[form] & TA else "aki") + "->abji"
    pair = np.einsum(sub, Bm, Am).reshape(npool * npool, e2)
    csum = np.zeros((total + 1, e2), dtype=np.int32)
    np.cumsum(pair[ai * npool + bi], axis=0, out=csum[1:])
    ref = csum[seg_ptr[1:].astype(np.int64)] - csum[seg_ptr[:-1].astype(np.int64)]
    if beta:
        ref = ref + C0.reshape(nseg, e2).astype(np.int32)
    bad = np.flatnonzero((got.astype(np.float64) != ref).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {nseg} segments differ from the numpy sum, first: segment {bad[0]} (count {counts[bad[0]]})"
    assert not np.signbit(got[counts == 0]).any() or beta                     # empty segments under beta = 0 are +0


def test_scale_transposed_f32_segments():
    api = capi.load()
    _scale(api, 60000, 16, "TN", 0, 500)
    _scale(api, 140000, 8, "NT", 1, 501)              # more items than one wave each: the waves grid-stride


def test_modes_stream_pipeline_and_coalescing_keep_the_results():
    import torch
    from test_gemm_grouped_gpu import Group
    api = capi.load()
    segs = [OffsetSegments(api, seed=600 + i, **kw) for i, kw in enumerate((dict(m=32, n=32, k=32, form="TN"), dict(m=23, n=23, k=23, a_type=DT.F64, beta=1, form="NT"),
                                                                             dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, form="TT")))]
    strided = Group(api, GemmCase(m=32, n=32, k=32, batch=40, seed=612))
    want = [sg.run_checked() for sg in segs]                                  # blocking
    want_strided = strided.run_own(api)
    # stream-ordered on a torch stream
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    csets = [sg.new_c() for sg in segs]
    for sg, cs in zip(segs, csets):
        sg.run(cs)
    api.hip_sync(); api.check()
    for sg, cs, w in zip(segs, csets, want):
        assert _same(sg.C0.download(cs[0]), w), "stream-ordered"
    # inside a pipeline section, next to a strided call
    csets = [sg.new_c() for sg in segs]
    assert api.hip_pipeline_begin(4) == 0
    segs[0].run(csets[0])
    segs[1].run(csets[1])
    api.hip_gemm_batch_strided(strided.handle, C.byref(strided.param), strided.case.batch, strided.sa, strided.sb, strided.case.bs_c)
    segs[2].run(csets[2])
    assert api.hip_pipeline_end() == 0
    api.hip_sync(); api.check()
    for sg, cs, w in zip(segs, csets, want):
        assert _same(sg.C0.download(cs[0]), w), "pipeline section"
    assert np.array_equal(strided.result().view(np.uint8), want_strided.view(np.uint8))
    # coalescing: a queued single call writes the block that every product of the offsets call reads as (transposed) A; the queue is flushed first
    m = 32
    rng = np.random.default_rng(620)
    X, Y = (torch.from_numpy(_ints(rng, m * m, DT.F32)).to("cuda:0") for _ in range(2))
    Bs = torch.from_numpy(_ints(rng, 3 * m * m, DT.F32)).to("cuda:0")
    T = torch.zeros(m * m, dtype=torch.float32, device="cuda:0")
    out = torch.zeros(2 * m * m, dtype=torch.float32, device="cuda:0")
    plain = GemmCase(m, m, m, seed=621).dispatch(api)
    off = GemmCase(m, m, m, flags=TA, br_type=capi.BR_OFFSET, br_count=1, seed=622).dispatch(api)
    seg_ptr = torch.tensor([0, 1, 3], dtype=torch.int64, device="cuda:0")
    oa = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    ob = torch.tensor([i * m * m * 4 for i in range(3)], dtype=torch.int64, device="cuda:0")
    oc = torch.tensor([0, m * m * 4], dtype=torch.int64, device="cuda:0")
    api.hip_set_async(2)
    p = capi.GemmParam(); p.a.primary, p.b.primary, p.c.primary = X.data_ptr(), Y.data_ptr(), T.data_ptr()
    capi.Api.call(plain, p)                                                   # queued, nothing launched yet
    q = capi.GemmParam(); q.a.primary, q.b.primary, q.c.primary = T.data_ptr(), Bs.data_ptr(), out.data_ptr()
    api.hip_gemm_batch_reduce_segments_offsets(off, C.byref(q), 2, seg_ptr.data_ptr(), oa.data_ptr(), ob.data_ptr(), oc.data_ptr())
    api.hip_sync(); api.check()
    api.hip_set_async(0); api.hip_set_stream(None)
    col = lambda t: t.cpu().numpy().astype(np.float64).reshape(m, m).T        # column-major block -> matrix
    Tm = (col(X) @ col(Y)).T                                                  # TRANS_A: the block is read as its transpose
    Bm = [col(Bs[i * m * m:(i + 1) * m * m]) for i in range(3)]
    got = out.cpu().numpy().astype(np.float64).reshape(2, m, m)
    assert np.array_equal(got[0].T, Tm @ Bm[0]) and np.array_equal(got[1].T, Tm @ Bm[1] + Tm @ Bm[2])


def test_a_captured_call_replays_on_new_operand_values():
    """One call captured on one stream (one linear node); the operand VALUES are overwritten in place -- the bases travel by value, so the replay reads the same
    addresses -- the graph is replayed once and recomputes from them."""
    import torch
    api = capi.load()
    sg = OffsetSegments(api, m=32, n=32, k=32, form="TN", seed=700)
    new = OffsetSegments(api, m=32, n=32, k=32, form="TN", seed=701)          # same pattern and layout, other values
    cset = sg.new_c()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        api.hip_set_stream(side.cuda_stream)
        api.hip_launch_count(1)
        g.capture_begin()
        sg.run(cset)
        g.capture_end()
        assert api.hip_launch_count(0) == 1
    api.check()
    torch.cuda.current_stream().wait_stream(side)
    api.hip_set_stream(None); api.hip_set_async(0)
    for dev, pool in ((sg.dA, new.A), (sg.dB, new.B), (cset[0], new.C0)):
        for d, h in zip(dev, pool.host):
            d.copy_(torch.from_numpy(h))
    torch.cuda.synchronize()
    g.replay(); torch.cuda.synchronize()
    assert _same(sg.C0.download(cset[0]), new.oracle(fma=True))


def _blocks(D, e):
    """Dense matrix -> its e x e blocks, column-major each: [block row][block column][e * e]."""
    R, Cc = D.shape[0] // e, D.shape[1] // e
    return np.ascontiguousarray(D.reshape(R, e, Cc, e).transpose(0, 2, 3, 1)).reshape(R, Cc, e * e)


def _dense(blocks, e):
    R, Cc = blocks.shape[:2]
    return blocks.reshape(R, Cc, e, e).transpose(0, 3, 1, 2).reshape(R * e, Cc * e)


def test_a_block_sparse_layer_forward_and_backward_is_one_call_each():
    """W: 6 x 5 blocks of 16 x 16, about half present, in BSR form (values in block-row order).  Y = W X over W's block rows (NN), dX = W^T dY over W's block
    columns (TRANS_A, the SAME value buffer, lists in block-column order), dW = dY X^T per present block (TRANS_B), on small integers against numpy float64."""
    api = capi.load()
    e, R, Cc, P = 16, 6, 5, 3
    bb = e * e * 4                                                            # bytes of a block
    rng = np.random.default_rng(800)
    present = rng.random((R, Cc)) < 0.5
    present[2, :] = False                                                     # an empty block row: a segment of count 0
    rows, cols = np.nonzero(present)                                          # block-row order
    nnz = len(rows)
    pos = -np.ones((R, Cc), dtype=np.int64); pos[rows, cols] = np.arange(nnz)
    ints = lambda *shape: rng.integers(-1, 2, shape).astype(np.float32)
    Wd = ints(R * e, Cc * e) * np.kron(present, np.ones((e, e), dtype=np.float32))
    Xd, dYd = ints(Cc * e, P * e), ints(R * e, P * e)
    vals = _blocks(Wd, e)[rows, cols]                                         # [nnz][e * e]
    d_vals, d_x, d_dy = _up(vals.copy()), _up(_blocks(Xd, e).copy()), _up(_blocks(dYd, e).copy())
    mk = lambda form: GemmCase(e, e, e, flags=FORMS[form], beta=0, br_type=capi.BR_OFFSET, br_count=1, batch=1).dispatch(api)

    def call(h, counts, oa, ob, nseg, a, b, c):
        seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        lists = [_up(seg), _up(np.asarray(oa, dtype=np.int64)), _up(np.asarray(ob, dtype=np.int64)), _up(np.arange(nseg, dtype=np.int64) * bb)]
        p = capi.GemmParam(); p.a.primary, p.b.primary, p.c.primary = a.data_ptr(), b.data_ptr(), c.data_ptr()
        api.hip_launch_count(1)
        api.hip_gemm_batch_reduce_segments_offsets(h, C.byref(p), nseg, *[x.data_ptr() for x in lists])
        assert api.hip_launch_count(1) == 1
        api.hip_sync(); api.check()

    # forward: segment (r, p) sums W[r, c] X[c, p] over the blocks of block row r
    d_y = _up(np.full((R, P, e * e), 7.0, dtype=np.float32))
    fa = [pos[r, c] * bb for r in range(R) for p in range(P) for c in np.flatnonzero(present[r])]
    fb = [(c * P + p) * bb for r in range(R) for p in range(P) for c in np.flatnonzero(present[r])]
    call(mk("NN"), [present[r].sum() for r in range(R) for p in range(P)], fa, fb, R * P, d_vals, d_x, d_y)
    assert np.array_equal(_dense(_down(d_y, vals).reshape(R, P, e * e), e).astype(np.float64), Wd.astype(np.float64) @ Xd.astype(np.float64))
    # backward, data: segment (c, p) sums W[r, c]^T dY[r, p] over the blocks of block column c -- W's own buffer, block-column-ordered lists
    d_dx = _up(np.full((Cc, P, e * e), 7.0, dtype=np.float32))
    ba = [pos[r, c] * bb for c in range(Cc) for p in range(P) for r in np.flatnonzero(present[:, c])]
    bl = [(r * P + p) * bb for c in range(Cc) for p in range(P) for r in np.flatnonzero(present[:, c])]
    call(mk("TN"), [present[:, c].sum() for c in range(Cc) for p in range(P)], ba, bl, Cc * P, d_vals, d_dy, d_dx)
    assert np.array_equal(_dense(_down(d_dx, vals).reshape(Cc, P, e * e), e).astype(np.float64), Wd.T.astype(np.float64) @ dYd.astype(np.float64))
    # backward, weights: segment z = (r, c) sums dY[r, p] X[c, p]^T over p, into the gradient's BSR value buffer
    d_dw = _up(np.full((nnz, e * e), 7.0, dtype=np.float32))
    wa = [(r * P + p) * bb for r, c in zip(rows, cols) for p in range(P)]
    wb = [(c * P + p) * bb for r, c in zip(rows, cols) for p in range(P)]
    call(mk("NT"), [P] * nnz, wa, wb, nnz, d_dy, d_x, d_dw)
    full = _blocks((dYd.astype(np.float64) @ Xd.T.astype(np.float64)).astype(np.float32), e)
    assert np.array_equal(_down(d_dw, vals).reshape(nnz, e * e), full[rows, cols])


def test_c_example_runs_a_layer_forward_and_backward(tmp_path):
    libdir = os.path.join(ROOT, "libxsmm_amd", "lib")
    exe = str(tmp_path / "segments_backward_driver")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "segments_backward_driver.c"),
           "-L" + libdir, "-lxsmm_amd", "-lm", "-Wl,-rpath," + libdir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "normf_rel" in r.stdout


def test_guarded_rerun_with_operands_flush_against_unmapped_memory():
    """The f32, f64 and scale tests again with every upload flush against unmapped address space (tests/guard.py via tests/conftest.py): the main pools, the last
    A, B and C block (arrays of their own) and the four lists.  These are parity tests on valid inputs: an access outside an operand would fault the subprocess.
    Why none is expected (gemm_group_tile.hpp): every load clamps its row / column to m - 1 / n - 1 and its k to K - 1; the 16- and 8-byte loads of a transposed A
    start at i * lda + kk with kk + 3 (f32) or kk + E - 1 (bf16) below the last whole k block <= K <= lda, so the last row of a TRANS_A block is read up to element
    (m - 1) * lda + K - 1 at most; a TRANS_B operand is read element-wise at k * ldb + min(j, n - 1) with k <= K - 1, so its last k row ends at (K - 1) * ldb +
    n - 1.  The second side only runs once the first has passed."""
    for side in ("end", "front"):
        env = dict(os.environ, LIBXSMM_TEST_GUARD=side)
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
               "-k", "test_f32_offset_segments_are_bitwise or test_f64_offset_segments_match or test_scale_transposed", "-v", "--no-header"]
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
        print(f"guarded run ({side}): {time.time() - t0:.1f} s")
        assert r.returncode == 0, f"guarded run ({side}) ended with {r.returncode} (negative / 134: the GPU faulted on an out-of-bounds access):\n{tail}"
        assert "9 passed" in r.stdout, tail
