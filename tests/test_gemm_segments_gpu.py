"""libxsmm_hip_gemm_batch_reduce_segments (include/libxsmm_hip.h): ADDRESS batch-reduce products with a reduce count of their own per C block, in one launch,
equal the loop of single calls they replace.  f32 segments are bitwise the oracle's (product, k)-ordered fmaf chain, f64 and bf16 segments lie within the dense
kernels' tolerances and are bitwise on exact data; empty segments follow beta; one call is one launch of the new kernel; the grid-stride holds at scale; stream
order, pipeline sections, the coalescing queue and graph capture keep the results.  The last test re-runs the parity and scale tests with every operand flush
against unmapped memory (run this file with -x)."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# every count of {0, 1, 2, 3, 7, 19, 64} in one call; empty segments at the front, in the middle and at the very end of the lists
COUNTS = [0, 3, 64, 1, 0, 2, 7, 19, 1, 0]


def _up(x):
    """Device image of a host array: guarded (flush against unmapped memory) when the guard is on, as GemmCase.run_gpu uploads."""
    if helpers.UPLOAD_HOOK is not None:
        return helpers.UPLOAD_HOOK(x)
    import torch
    x = np.ascontiguousarray(x)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint64): np.int64}.get(x.dtype)
    return torch.from_numpy(x.view(view) if view else x).to("cuda:0")


def _down(buf, like):
    return np.ascontiguousarray(buf.cpu().numpy()).view(like.dtype)


def _ints(rng, count, dt):
    """Small-integer operands (-1 / 0 / 1): every partial sum is exact, so any summation order gives the same bits."""
    v = rng.integers(-1, 2, count).astype(np.float32)
    return helpers.f32_to_bf16_trunc(v) if dt == DT.BF16 else v.astype(NP_OF[dt])


class Pool:
    """`nblocks` blocks of `elems` elements, one element apart (so the blocks take every alignment an element allows); the LAST block is an array of its own:
    under the guard it sits flush against unmapped memory like the end (or front) of the main array."""

    def __init__(self, values, nblocks, elems):
        self.nblocks, self.elems, self.pitch = nblocks, elems, elems + 1
        self.esz = values.dtype.itemsize
        self.host = [np.ascontiguousarray(values[:(nblocks - 1) * self.pitch]) if nblocks > 1 else values[:0].copy(),
                     np.ascontiguousarray(values[(nblocks - 1) * self.pitch:(nblocks - 1) * self.pitch + elems])]

    @staticmethod
    def size(nblocks, elems):
        return nblocks * (elems + 1)

    def copy(self):
        p = Pool.__new__(Pool)
        p.__dict__.update(self.__dict__)
        p.host = [h.copy() for h in self.host]
        return p

    def upload(self):
        return [_up(h) if h.size else None for h in self.host]

    def _addr(self, bases, b):
        return bases[1] if b == self.nblocks - 1 else bases[0] + b * self.pitch * self.esz

    def host_ptrs(self, idx):
        bases = [h.ctypes.data for h in self.host]
        return np.array([self._addr(bases, int(b)) for b in idx], dtype=np.uint64)

    def dev_ptrs(self, dev, idx):
        bases = [d.data_ptr() if d is not None else 0 for d in dev]
        return np.array([self._addr(bases, int(b)) for b in idx], dtype=np.uint64)

    def block(self, arrays, b):
        return arrays[1] if b == self.nblocks - 1 else arrays[0][b * self.pitch:b * self.pitch + self.elems]

    def download(self, dev):
        return [_down(d, h) if d is not None else h.copy() for d, h in zip(dev, self.host)]


class Segments:
    """One segments call: pools of A and B blocks, one C block per segment, the CSR-style lists -- on the host for the oracle and on the device."""

    def __init__(self, api, m, n, k, counts=COUNTS, a_type=DT.F32, c_type=None, flags=0, beta=0, lda=None, ldb=None, ldc=None, seed=0, exact=False, npool=9, prepare=None):
        self.api = api
        self.case = case = GemmCase(m, n, k, a_type=a_type, c_type=c_type, lda=lda, ldb=ldb, ldc=ldc, flags=flags, beta=beta,
                                    br_type=capi.BR_ADDRESS, br_count=1, batch=1, seed=seed)
        rng = np.random.default_rng(1000 + seed)
        gen = _ints if exact else helpers.rand_values
        self.counts = np.asarray(counts, dtype=np.uint64)
        self.nseg = len(self.counts)
        self.seg_ptr = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.uint64)
        total = int(self.seg_ptr[-1])
        self.A = Pool(gen(rng, Pool.size(npool, case.a_elems), a_type), npool, case.a_elems)
        self.B = Pool(gen(rng, Pool.size(npool, case.b_elems), case.b_type), npool, case.b_elems)
        self.C0 = Pool(gen(rng, Pool.size(self.nseg, case.c_elems), case.c_type), self.nseg, case.c_elems)
        seg_of = np.repeat(np.arange(self.nseg), self.counts.astype(np.int64))
        r_of = np.arange(total) - self.seg_ptr[seg_of].astype(np.int64)
        self.ai = (seg_of * 3 + r_of) % npool                                     # A blocks are shared across segments ...
        self.bi = np.where(seg_of % 2 == 0, seg_of % npool, (seg_of + r_of) % npool)   # ... and even segments use ONE B for all their products
        if prepare is not None:              # the host pools before they are uploaded (tests/test_gemm_ld_gpu.py poisons the gaps of every block)
            prepare(self)
        self.dA, self.dB = self.A.upload(), self.B.upload()
        self.d_seg = _up(self.seg_ptr)
        self.d_la, self.d_lb = _up(self.A.dev_ptrs(self.dA, self.ai)), _up(self.B.dev_ptrs(self.dB, self.bi))
        self.handle = case.dispatch(api)
        assert self.handle

    def new_c(self):
        dC = self.C0.upload()
        return dC, _up(self.C0.dev_ptrs(dC, range(self.nseg)))

    def run(self, cset):
        p = capi.GemmParam()
        self.api.hip_gemm_batch_reduce_segments(self.handle, C.byref(p), self.nseg, self.d_seg.data_ptr(), self.d_la.data_ptr(), self.d_lb.data_ptr(), cset[1].data_ptr())

    def run_checked(self):
        cset = self.new_c()
        self.run(cset)
        self.api.hip_sync(); self.api.check()
        return self.C0.download(cset[0])

    def run_loop(self):
        """The loop the call replaces: one blocking call of the same handle per segment."""
        dC = self.C0.upload()
        cp = self.C0.dev_ptrs(dC, range(self.nseg))
        for s in range(self.nseg):
            p = capi.GemmParam()
            cnt = C.c_ulonglong(int(self.counts[s]))
            p.a.primary = self.d_la.data_ptr() + int(self.seg_ptr[s]) * 8
            p.b.primary = self.d_lb.data_ptr() + int(self.seg_ptr[s]) * 8
            p.c.primary = int(cp[s]); p.op.tertiary = C.addressof(cnt)
            capi.Api.call(self.handle, p)
        self.api.hip_sync(); self.api.check()
        return self.C0.download(dC)

    def oracle(self, fma=False):
        orc, d = pyoracle.oracle(), self.case.oracle_desc()
        ref = self.C0.copy()
        la, lb, lc = self.A.host_ptrs(self.ai), self.B.host_ptrs(self.bi), ref.host_ptrs(range(self.nseg))
        for s in range(self.nseg):
            p = capi.GemmParam()
            cnt = C.c_ulonglong(int(self.counts[s]))                            # the oracle accepts a count of 0
            p.a.primary = la.ctypes.data + int(self.seg_ptr[s]) * 8
            p.b.primary = lb.ctypes.data + int(self.seg_ptr[s]) * 8
            p.c.primary = int(lc[s]); p.op.tertiary = C.addressof(cnt)
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


def _same(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


F32_SHAPES = [dict(m=32, n=32, k=32), dict(m=16, n=16, k=16), dict(m=13, n=17, k=29), dict(m=13, n=13, k=13),
              dict(m=20, n=24, k=18, lda=23, ldb=21, ldc=29), dict(m=40, n=40, k=40), dict(m=9, n=5, k=3)]


def test_f32_segments_are_bitwise_the_fma_chain():
    api = capi.load()
    for i, kw in enumerate(F32_SHAPES):
        for beta in (0, 1):
            sg = Segments(api, beta=beta, seed=10 * i + beta, **kw)
            got, ref = sg.run_checked(), sg.oracle(fma=True)
            # whole arrays: the m x n blocks are the (product, k)-ordered fmaf chain bit for bit, and the padding of C beyond m x n is unchanged
            assert _same(got, ref), f"{kw} beta={beta}: differs from the (product, k)-ordered fmaf chain (or wrote outside m x n)"
            for s in np.flatnonzero(sg.counts == 0):                              # empty segments: +0 under beta = 0, untouched under beta = 1
                v = sg.valid(got, s)
                want = sg.valid(sg.C0.host, s) if beta else np.zeros_like(v)
                assert np.array_equal(v.view(np.uint32), want.view(np.uint32)), f"{kw} beta={beta}: empty segment {s}"


F64_SHAPES = [dict(m=16, n=16, k=16), dict(m=23, n=23, k=23), dict(m=32, n=32, k=32), dict(m=8, n=40, k=5), dict(m=20, n=24, k=18, lda=23, ldb=21, ldc=29)]


def test_f64_segments_match_the_oracle():
    api = capi.load()
    for i, kw in enumerate(F64_SHAPES):
        for beta in (0, 1):
            sg = Segments(api, a_type=DT.F64, beta=beta, seed=100 + 10 * i + beta, **kw)
            got, ref = sg.run_checked(), sg.oracle()
            for s in range(sg.nseg):
                err = normf_rel(sg.valid(ref, s), sg.valid(got, s), DT.F64)
                assert err < TOL_F64, f"{kw} beta={beta} segment {s} (count {sg.counts[s]}): normf_rel = {err}"
            sg.assert_padding_untouched(got, f"{kw} beta={beta}")
            ex = Segments(api, a_type=DT.F64, beta=beta, seed=150 + 10 * i + beta, exact=True, **kw)
            assert _same(ex.run_checked(), ex.oracle()), f"{kw} beta={beta}: exact data differs from the oracle"


BF16_CASES = [dict(m=32, n=32, k=32, c_type=DT.F32),                                                  # flat A -> f32
              dict(m=16, n=16, k=16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, beta=1),                 # VNNI A -> bf16, 16-tile
              dict(m=13, n=17, k=29, c_type=DT.BF16),                                                 # ragged, flat A -> bf16
              dict(m=64, n=64, k=64, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A),                         # 2 x 2 tiles
              dict(m=24, n=40, k=34, c_type=DT.F32, flags=GEMM_FLAG.VNNI_A, lda=27, ldb=37, ldc=30, beta=1),   # padded, VNNI A -> f32
              dict(m=13, n=13, k=13, c_type=DT.BF16, beta=1)]                                         # ragged 16-tile, flat A -> bf16


def test_bf16_segments_match_the_oracle():
    api = capi.load()
    for i, kw in enumerate(BF16_CASES):
        sg = Segments(api, a_type=DT.BF16, seed=200 + i, **kw)
        got, ref = sg.run_checked(), sg.oracle()
        for s in range(sg.nseg):                                                  # (count-0 segments with bf16 C included)
            err = normf_rel(sg.valid(ref, s), sg.valid(got, s), sg.case.c_type)
            assert err < TOL_BF16, f"{kw} segment {s} (count {sg.counts[s]}): normf_rel = {err}"
        sg.assert_padding_untouched(got, str(kw))
        ex = Segments(api, a_type=DT.BF16, seed=250 + i, exact=True, **kw)
        assert _same(ex.run_checked(), ex.oracle()), f"{kw}: exact data differs from the oracle"


LOOP_CASES = [dict(m=32, n=32, k=32), dict(m=13, n=17, k=29, beta=1), dict(m=23, n=23, k=23, a_type=DT.F64), dict(m=16, n=16, k=16, a_type=DT.F64, beta=1),
              dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A), dict(m=24, n=40, k=34, a_type=DT.BF16, c_type=DT.F32, beta=1)]


def test_the_call_equals_its_loop_on_the_device():
    api = capi.load()
    for i, kw in enumerate(LOOP_CASES):
        sg = Segments(api, seed=300 + i, exact=True, **kw)
        assert _same(sg.run_checked(), sg.run_loop()), f"{kw}: differs from the loop of single calls through the same handle"


def test_one_launch_per_call_through_the_new_kernel():
    api = capi.load()
    for kw, name in ((dict(m=32, n=32, k=32), b"gemm_segments_f32_kernel"), (dict(m=23, n=23, k=23, a_type=DT.F64), b"gemm_segments_f64_kernel"),
                     (dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A), b"gemm_segments_bf16_kernel")):
        sg = Segments(api, seed=400, **kw)
        cset = sg.new_c()
        api.hip_launch_count(1)
        sg.run(cset)
        assert api.hip_launch_count(1) == 1
        api.hip_sync(); api.check()
        assert api.hip_kernel_name(sg.handle, 1) == name


def _scale(api, nseg, edge, dt, beta, seed):
    """`nseg` segments of edge^3 with skewed counts (1 %: 64, a few empty, the rest 2) on exact data, every segment against a numpy sum."""
    rng = np.random.default_rng(seed)
    npool, e2 = 16, edge * edge
    counts = np.where(rng.random(nseg) < 0.01, 64, 2).astype(np.uint64)
    counts[::997] = 0
    seg_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    total = int(seg_ptr[-1])
    ai, bi = rng.integers(0, npool, total), rng.integers(0, npool, total)
    npdt = NP_OF[dt]
    A, B = _ints(rng, npool * e2, dt), _ints(rng, npool * e2, dt)
    C0 = _ints(rng, nseg * e2, dt)
    dA, dB, dC = _up(A), _up(B), _up(C0.copy())
    esz = A.itemsize
    lists = [_up(seg_ptr), _up((dA.data_ptr() + ai * e2 * esz).astype(np.uint64)), _up((dB.data_ptr() + bi * e2 * esz).astype(np.uint64)),
             _up((dC.data_ptr() + np.arange(nseg, dtype=np.int64) * (e2 * esz)).astype(np.uint64))]
    case = GemmCase(edge, edge, edge, a_type=dt, beta=beta, br_type=capi.BR_ADDRESS, br_count=1, batch=1)
    h = case.dispatch(api)
    assert h
    p = capi.GemmParam()
    api.hip_launch_count(1)
    api.hip_gemm_batch_reduce_segments(h, C.byref(p), nseg, *[x.data_ptr() for x in lists])
    assert api.hip_launch_count(1) == 1
    api.hip_sync(); api.check()
    got = _down(dC, C0).reshape(nseg, e2)
    # column-major blocks: C(i, j) = sum_k A(i, k) B(k, j)  <=>  as row-major arrays C^T = B^T A^T; every pair of pool blocks once, then per-product gathers
    Am, Bm = A.reshape(npool, edge, edge).astype(np.int32), B.reshape(npool, edge, edge).astype(np.int32)
    pair = np.einsum("bjk,aki->abji", Bm, Am).reshape(npool * npool, e2)
    csum = np.zeros((total + 1, e2), dtype=np.int32)
    np.cumsum(pair[ai * npool + bi], axis=0, out=csum[1:])
    ref = csum[seg_ptr[1:].astype(np.int64)] - csum[seg_ptr[:-1].astype(np.int64)]
    if beta:
        ref = ref + C0.reshape(nseg, e2).astype(np.int32)
    bad = np.flatnonzero((got.astype(np.float64) != ref).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {nseg} segments differ from the numpy sum, first: segment {bad[0]} (count {counts[bad[0]]})"
    assert not np.signbit(got[counts == 0]).any() or beta                     # empty segments under beta = 0 are +0


def test_scale_f32_sixty_thousand_segments():
    api = capi.load()
    _scale(api, 60000, 16, DT.F32, 0, 500)
    _scale(api, 140000, 8, DT.F32, 1, 501)            # more items than one wave each: the waves grid-stride


def test_scale_f64_twenty_thousand_segments():
    api = capi.load()
    _scale(api, 20000, 16, DT.F64, 1, 510)


def test_modes_stream_pipeline_and_coalescing_keep_the_results():
    import torch
    from test_gemm_grouped_gpu import Group
    api = capi.load()
    segs = [Segments(api, seed=600 + i, **kw) for i, kw in enumerate((dict(m=32, n=32, k=32), dict(m=23, n=23, k=23, a_type=DT.F64, beta=1),
                                                                       dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A)))]
    mk_groups = lambda: [Group(api, GemmCase(m=13, n=17, k=29, batch=9, seed=610)), Group(api, GemmCase(m=16, n=16, k=16, batch=12, seed=611))]
    groups, blocking_groups = mk_groups(), mk_groups()
    strided = Group(api, GemmCase(m=32, n=32, k=32, batch=40, seed=612))
    want = [sg.run_checked() for sg in segs]                                  # blocking
    arr = (capi.GemmGroup * len(blocking_groups))(*[g.entry() for g in blocking_groups])
    api.hip_gemm_batch_grouped(arr, len(blocking_groups))
    api.hip_sync(); api.check()
    want_groups = [g.result() for g in blocking_groups]
    want_strided = strided.run_own(api)
    # stream-ordered on a torch stream
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    csets = [sg.new_c() for sg in segs]
    for sg, cs in zip(segs, csets):
        sg.run(cs)
    api.hip_sync(); api.check()
    for sg, cs, w in zip(segs, csets, want):
        assert _same(sg.C0.download(cs[0]), w), "stream-ordered"
    # inside a pipeline section, next to a grouped call and a strided call
    csets = [sg.new_c() for sg in segs]
    assert api.hip_pipeline_begin(4) == 0
    segs[0].run(csets[0])
    arr = (capi.GemmGroup * len(groups))(*[g.entry() for g in groups])
    api.hip_gemm_batch_grouped(arr, len(groups))
    segs[1].run(csets[1])
    api.hip_gemm_batch_strided(strided.handle, C.byref(strided.param), strided.case.batch, strided.sa, strided.sb, strided.case.bs_c)
    segs[2].run(csets[2])
    assert api.hip_pipeline_end() == 0
    api.hip_sync(); api.check()
    for sg, cs, w in zip(segs, csets, want):
        assert _same(sg.C0.download(cs[0]), w), "pipeline section"
    for g, w in zip(groups, want_groups):
        assert np.array_equal(g.result().view(np.uint8), w.view(np.uint8))
    assert np.array_equal(strided.result().view(np.uint8), want_strided.view(np.uint8))
    # coalescing: a queued single call writes the block that every product of the segments call reads as A; the queue is flushed first
    m = 32
    rng = np.random.default_rng(620)
    X, Y = (torch.from_numpy(_ints(rng, m * m, DT.F32)).to("cuda:0") for _ in range(2))
    Bs = torch.from_numpy(_ints(rng, 3 * m * m, DT.F32)).to("cuda:0")
    T = torch.zeros(m * m, dtype=torch.float32, device="cuda:0")
    out = torch.zeros(2 * m * m, dtype=torch.float32, device="cuda:0")
    plain = GemmCase(m, m, m, seed=621).dispatch(api)
    adr = GemmCase(m, m, m, br_type=capi.BR_ADDRESS, br_count=1, seed=622).dispatch(api)
    seg_ptr = torch.tensor([0, 1, 3], dtype=torch.int64, device="cuda:0")
    la = torch.tensor([T.data_ptr()] * 3, dtype=torch.int64, device="cuda:0")
    lb = torch.tensor([Bs.data_ptr() + i * m * m * 4 for i in range(3)], dtype=torch.int64, device="cuda:0")
    lc = torch.tensor([out.data_ptr(), out.data_ptr() + m * m * 4], dtype=torch.int64, device="cuda:0")
    api.hip_set_async(2)
    p = capi.GemmParam(); p.a.primary, p.b.primary, p.c.primary = X.data_ptr(), Y.data_ptr(), T.data_ptr()
    capi.Api.call(plain, p)                                                   # queued, nothing launched yet
    q = capi.GemmParam()
    api.hip_gemm_batch_reduce_segments(adr, C.byref(q), 2, seg_ptr.data_ptr(), la.data_ptr(), lb.data_ptr(), lc.data_ptr())
    api.hip_sync(); api.check()
    api.hip_set_async(0); api.hip_set_stream(None)
    col = lambda t: t.cpu().numpy().astype(np.float64).reshape(m, m).T        # column-major block -> matrix
    Tm = col(X) @ col(Y)
    Bm = [col(Bs[i * m * m:(i + 1) * m * m]) for i in range(3)]
    got = out.cpu().numpy().astype(np.float64).reshape(2, m, m)
    assert np.array_equal(got[0].T, Tm @ Bm[0]) and np.array_equal(got[1].T, Tm @ Bm[1] + Tm @ Bm[2])


def test_a_captured_call_replays_on_new_operand_values():
    """One call captured on one stream (one linear node); the operand VALUES are overwritten in place, the graph is replayed once and recomputes from them."""
    import torch
    api = capi.load()
    sg = Segments(api, m=32, n=32, k=32, seed=700)
    new = Segments(api, m=32, n=32, k=32, seed=701)                           # same pattern and layout, other values
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


def test_c_example_multiplies_a_block_sparse_matrix_in_one_call(tmp_path):
    libdir = os.path.join(ROOT, "libxsmm_amd", "lib")
    exe = str(tmp_path / "segments_driver")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "segments_driver.c"),
           "-L" + libdir, "-lxsmm_amd", "-lm", "-Wl,-rpath," + libdir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "normf_rel" in r.stdout


def test_guarded_rerun_with_operands_flush_against_unmapped_memory():
    """The f32, f64 and scale tests again with every upload flush against unmapped address space (tests/guard.py via tests/conftest.py): the main pools, the last
    A, B and C block (arrays of their own) and the four lists.  These are parity tests on valid inputs: an access outside an operand would fault the subprocess.
    The second side only runs once the first has passed."""
    for side in ("end", "front"):
        env = dict(os.environ, LIBXSMM_TEST_GUARD=side)
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
               "-k", "test_f32_segments_are_bitwise or test_f64_segments_match or test_scale_f32 or test_scale_f64", "-v", "--no-header"]
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
        print(f"guarded run ({side}): {time.time() - t0:.1f} s")
        assert r.returncode == 0, f"guarded run ({side}) ended with {r.returncode} (negative / 134: the GPU faulted on an out-of-bounds access):\n{tail}"
        assert "4 passed" in r.stdout, tail
