"""libxsmm_hip_gemm_ext_batch_reduce_segments (include/libxsmm_hip.h): the segments call through an ext handle -- column bias, ReLU (+ bitmask), sigmoid fused
into the one launch -- equals the loop of fused single calls it replaces.  f32 segments are bitwise the oracle's (product, k)-ordered fmaf chain started at the
bias, mask bits included, with every byte outside the m x n blocks and every mask bit beyond them left alone; bf16 segments are bitwise the ext oracle on exact
data and within the dense kernels' tolerances on random data; a shared bias, the launch modes, graph capture and 60 000 / 140 000 segments keep the results.  The
last test re-runs the parity tests with every operand, bias and mask block flush against unmapped memory (run this file with -x)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import helpers
from gemm_ld_helpers import bound64
from helpers import GemmCase, TOL_BF16, TOL_F32, as_float, normf_rel
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG
from oracle import pyoracle
from test_gemm_segments_gpu import COUNTS, Pool, Segments, _down, _ints, _same, _up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

NBIAS = 4      # bias blocks, one element apart (every alignment an element allows); the segments share them


class FusedSegments(Segments):
    """A segments call with an epilogue: the plain call's pools and lists, a pool of bias vectors that the segments share (d_list repeats its entries) and one
    mask block per segment, prefilled with random bytes.  set_epilogue picks the handle; the pools stay."""

    def __init__(self, api, m, n, k, colbias=False, act=0, **kw):
        exact = kw.get("exact", False)
        super().__init__(api, m, n, k, counts=COUNTS, **kw)
        case = self.case
        rng = np.random.default_rng(5000 + kw.get("seed", 0))
        gen = _ints if exact else helpers.rand_values
        self.D = Pool(gen(rng, Pool.size(NBIAS, m), case.c_type), NBIAS, m)
        self.di = (np.arange(self.nseg) * 3) % NBIAS                              # 0, 3, 2, 1, 0, ...: repeated entries, the last block among them
        self.M0 = Pool(rng.integers(0, 256, Pool.size(self.nseg, case.mask_bytes)).astype(np.uint8), self.nseg, case.mask_bytes)
        self.dD = self.D.upload()
        self.d_ld = _up(self.D.dev_ptrs(self.dD, self.di))
        self.kw = dict(m=m, n=n, k=k, a_type=case.a_type, c_type=case.c_type, lda=case.lda, ldb=case.ldb, ldc=case.ldc,
                       flags=case.flags & ~GEMM_FLAG.BETA_0, br_type=capi.BR_ADDRESS, br_count=1)
        self.beta = 0 if case.flags & GEMM_FLAG.BETA_0 else 1
        self.set_epilogue(colbias, act)

    def set_epilogue(self, colbias, act):
        self.colbias, self.act = colbias, act
        self.ext = GemmCase(beta=self.beta, colbias=colbias, act=act, **self.kw)      # (descriptor only: its operands are not used)
        self.ext_handle = self.api.dispatch_brgemm_ext(self.ext.shape(), self.ext.flags, 0, self.ext.brcfg(), self.ext.argops(), self.ext.postops())
        assert self.ext_handle
        return self

    # ---- device ---------------------------------------------------------------------------------------------------------------------------------
    def new_out(self):
        dC, dM = self.C0.upload(), self.M0.upload()
        return dict(C=dC, lc=_up(self.C0.dev_ptrs(dC, range(self.nseg))), M=dM, lm=_up(self.M0.dev_ptrs(dM, range(self.nseg))))

    def run(self, out, shared_d=None):
        """shared_d: a device address -- d_list = NULL and param->d.primary carries the one bias of every segment."""
        p = capi.GemmExtParam()
        ld = self.d_ld.data_ptr() if self.colbias else None
        if shared_d is not None:
            p.d.primary, ld = shared_d, None
        self.api.hip_gemm_ext_batch_reduce_segments(self.ext_handle, C.byref(p), self.nseg, self.d_seg.data_ptr(), self.d_la.data_ptr(), self.d_lb.data_ptr(),
                                                    out["lc"].data_ptr(), ld, out["lm"].data_ptr() if self.act == 2 else None)

    def result(self, out):
        return self.C0.download(out["C"]), self.M0.download(out["M"])

    def run_checked(self, **kw):
        out = self.new_out()
        self.run(out, **kw)
        self.api.hip_sync(); self.api.check()
        return self.result(out)

    def run_loop(self):
        """The loop the call replaces: one blocking fused call per segment, d.primary, c.secondary and the count set per segment."""
        out = self.new_out()
        cp, mp = self.C0.dev_ptrs(out["C"], range(self.nseg)), self.M0.dev_ptrs(out["M"], range(self.nseg))
        dp = self.D.dev_ptrs(self.dD, self.di)
        for s in range(self.nseg):
            p = capi.GemmExtParam()
            cnt = C.c_ulonglong(int(self.counts[s]))
            p.a.primary = self.d_la.data_ptr() + int(self.seg_ptr[s]) * 8
            p.b.primary = self.d_lb.data_ptr() + int(self.seg_ptr[s]) * 8
            p.c.primary = int(cp[s]); p.op.tertiary = C.addressof(cnt)
            if self.colbias:
                p.d.primary = int(dp[s])
            if self.act == 2:
                p.c.secondary = int(mp[s])
            capi.Api.call(self.ext_handle, p)
        self.api.hip_sync(); self.api.check()
        return self.result(out)

    # ---- host ------------------------------------------------------------------------------------------------------------------------------------
    def _host_lists(self, ref):
        return self.A.host_ptrs(self.ai), self.B.host_ptrs(self.bi), ref.host_ptrs(range(self.nseg))

    def oracle_ext(self):
        """(C arrays, mask arrays) of the ext oracle called once per segment -- the reference's fused call [oracle/oracle_gemm.c]."""
        orc, d = pyoracle.oracle(), self.ext.oracle_desc()
        ref, msk = self.C0.copy(), self.M0.copy()
        la, lb, lc = self._host_lists(ref)
        ld, lm = self.D.host_ptrs(self.di), msk.host_ptrs(range(self.nseg))
        for s in range(self.nseg):
            p = capi.GemmExtParam()
            cnt = C.c_ulonglong(int(self.counts[s]))
            p.a.primary = la.ctypes.data + int(self.seg_ptr[s]) * 8
            p.b.primary = lb.ctypes.data + int(self.seg_ptr[s]) * 8
            p.c.primary = int(lc[s]); p.op.tertiary = C.addressof(cnt)
            if self.colbias:
                p.d.primary = int(ld[s])
            if self.act == 2:
                p.c.secondary = int(lm[s])
            orc.gemm(p, d)
        return ref.host, msk.host

    def bias_of(self, s):
        return self.D.block(self.D.host, int(self.di[s]))

    def mask_rows(self, arrays, s):
        c = self.case
        return self.M0.block(arrays, s).reshape(c.n, c.mask_ld // 8)

    def mask_bits(self, arrays, s):
        return np.unpackbits(self.mask_rows(arrays, s), axis=1, bitorder="little")[:, :self.case.m]

    def fma_chain(self):
        """f32: the expected bytes from the unchanged oracle -- bias (+ C0, one f32 add) written into a copy of C, the (product, k)-ordered fmaf chain with beta = 1
        on the non-ext descriptor on top of it, the mask bits !(x <= 0) set into a copy of the prefilled masks, then ReLU as np.where(x <= 0, +0, x)."""
        orc = pyoracle.oracle()
        d = GemmCase(beta=1, **self.kw).oracle_desc()
        ref, msk = self.C0.copy(), self.M0.copy()
        for s in range(self.nseg):
            v = self.valid(ref.host, s)
            start = v.copy() if self.beta else np.zeros_like(v)
            if self.colbias:
                start = (self.bias_of(s)[None, :] + start) if self.beta else np.broadcast_to(self.bias_of(s)[None, :], v.shape)
            v[...] = start
        la, lb, lc = self._host_lists(ref)
        for s in range(self.nseg):
            p = capi.GemmParam()
            cnt = C.c_ulonglong(int(self.counts[s]))
            p.a.primary = la.ctypes.data + int(self.seg_ptr[s]) * 8
            p.b.primary = lb.ctypes.data + int(self.seg_ptr[s]) * 8
            p.c.primary = int(lc[s]); p.op.tertiary = C.addressof(cnt)
            orc.gemm(p, d, fma=True)
        for s in range(self.nseg):
            v = self.valid(ref.host, s)
            if self.act == 2:
                rows = self.mask_rows(msk.host, s)
                bits = np.unpackbits(rows, axis=1, bitorder="little")
                bits[:, :self.case.m] = ~(v <= 0)
                rows[...] = np.packbits(bits, axis=1, bitorder="little")
            if self.act in (1, 2):
                v[...] = np.where(v <= 0, np.float32(0.0), v)
        return ref.host, msk.host

    def pre64(self):
        """Per segment: (pre-activation sum, sum of magnitudes, terms) in float64 as [n][m] -- tests/gemm_ld_helpers.py's restatement for one chain."""
        c = self.case
        ai = lambda blk: as_float(blk, c.a_type)
        out = []
        for s in range(self.nseg):
            pre, mag, terms = np.zeros((c.n, c.m)), np.zeros((c.n, c.m)), int(self.counts[s]) * c.k
            for r in range(int(self.seg_ptr[s]), int(self.seg_ptr[s + 1])):
                a, b = ai(self.A.block(self.A.host, int(self.ai[r]))), ai(self.B.block(self.B.host, int(self.bi[r])))
                if c.flags & GEMM_FLAG.VNNI_A:                                     # [k / 2][lda][2] -> [k][lda]
                    kp = (c.k + 1) // 2
                    a = a[:kp * c.lda * 2].reshape(kp, c.lda, 2).transpose(0, 2, 1).reshape(2 * kp, c.lda)[:c.k]
                else:
                    a = a[:c.k * c.lda].reshape(c.k, c.lda)
                am = a[:, :c.m]                                                    # [k][m]
                bm = b[:c.n * c.ldb].reshape(c.n, c.ldb)[:, :c.k]                  # [n][k]
                pre += bm @ am; mag += np.abs(bm) @ np.abs(am)
            if self.beta:
                c0 = as_float(self.valid(self.C0.host, s), c.c_type)
                pre, mag, terms = pre + c0, mag + np.abs(c0), terms + 1
            if self.colbias:
                bias = as_float(self.bias_of(s), c.c_type)[None, :]
                pre, mag, terms = pre + bias, mag + np.abs(bias), terms + 1
            out.append((pre, mag, terms))
        return out

    def assert_outside_untouched(self, got, gotm, what):
        self.assert_padding_untouched(got, what)
        if self.act != 2:
            assert _same(gotm, self.M0.host), f"{what}: a mask block was written without a bitmask"
            return
        c = self.case
        for s in range(self.nseg):
            g = np.unpackbits(self.mask_rows(gotm, s), axis=1, bitorder="little")[:, c.m:]
            assert np.array_equal(g, np.unpackbits(self.mask_rows(self.M0.host, s), axis=1, bitorder="little")[:, c.m:]), f"{what}: segment {s}: mask bits beyond m changed"
        for a, b in zip(gotm, self.M0.host):                                      # the bytes between the blocks
            if len(a) > c.mask_bytes:
                assert np.array_equal(a[c.mask_bytes::c.mask_bytes + 1], b[c.mask_bytes::c.mask_bytes + 1]), what


F32_SHAPES = [dict(m=32, n=32, k=32), dict(m=16, n=16, k=16), dict(m=13, n=17, k=29), dict(m=13, n=13, k=13),
              dict(m=20, n=24, k=18, lda=23, ldb=21, ldc=29), dict(m=40, n=40, k=40)]
EPILOGUES = [(True, 0), (True, 1), (False, 2), (True, 2)]          # bias only, bias + ReLU, ReLU + bitmask, bias + ReLU + bitmask


def test_f32_fused_segments_are_bitwise_the_fma_chain_mask_included():
    api = capi.load()
    for i, kw in enumerate(F32_SHAPES):
        for beta in (0, 1):
            sg = FusedSegments(api, beta=beta, seed=10 * i + beta, **kw)
            for colbias, act in EPILOGUES:
                what = f"{kw} beta={beta} colbias={colbias} act={act}"
                sg.set_epilogue(colbias, act)
                (got, gotm), (ref, refm) = sg.run_checked(), sg.fma_chain()
                # whole arrays: the m x n blocks and their mask bits are the chain's, every other byte and bit (padding, gaps, bits beyond m) is the caller's
                assert _same(got, ref), f"{what}: C differs from the fmaf chain started at the bias (or bytes outside m x n changed)"
                assert _same(gotm, refm), f"{what}: the mask differs from !(x <= 0) of the chain (or bits outside m x n changed)"
                orc, _ = sg.oracle_ext()
                for s in range(sg.nseg):
                    err = normf_rel(sg.valid(orc, s), sg.valid(ref, s), DT.F32)
                    assert err < TOL_F32, f"{what} segment {s}: the expected value is {err} from the ext oracle"


BF16_CASES = [dict(m=32, n=32, k=32, c_type=DT.F32),                                                  # flat A -> f32
              dict(m=16, n=16, k=16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, beta=1),                 # VNNI A -> bf16, 16-tile
              dict(m=13, n=17, k=29, c_type=DT.BF16),                                                 # ragged, flat A -> bf16
              dict(m=64, n=64, k=64, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A),                         # 2 x 2 tiles
              dict(m=24, n=40, k=34, c_type=DT.F32, flags=GEMM_FLAG.VNNI_A, lda=27, ldb=37, ldc=30, beta=1)]   # padded, VNNI A -> f32


def decided_mask_bits(sg):
    """Per segment of count > 0: (decided, positive) -- the mask bits the float64 restatement decides beyond the accumulation's error bound, and their value."""
    out = {}
    for s, (pre, mag, terms) in enumerate(sg.pre64()):
        if sg.counts[s] > 0:
            _, bound_pre = bound64(sg.case, pre, mag, terms)
            out[s] = (np.abs(pre) > bound_pre, pre > 0)
    return out


def test_bf16_fused_segments_match_the_ext_oracle():
    api = capi.load()
    for i, kw in enumerate(BF16_CASES):
        ex = FusedSegments(api, a_type=DT.BF16, seed=250 + i, exact=True, colbias=True, act=2, **kw)
        (got, gotm), (ref, refm) = ex.run_checked(), ex.oracle_ext()
        assert _same(got, ref) and _same(gotm, refm), f"{kw}: exact data differs from the ext oracle (C {_same(got, ref)}, mask {_same(gotm, refm)})"
        sg = FusedSegments(api, a_type=DT.BF16, seed=200 + i, colbias=True, act=2, **kw)
        (got, gotm), (ref, refm) = sg.run_checked(), sg.oracle_ext()
        tol = TOL_F32 if sg.case.c_type == DT.F32 else TOL_BF16
        for s in range(sg.nseg):
            err = normf_rel(sg.valid(ref, s), sg.valid(got, s), sg.case.c_type)
            assert err < tol, f"{kw} segment {s} (count {sg.counts[s]}): normf_rel = {err}"
        sg.assert_outside_untouched(got, gotm, str(kw))
        dec = decided_mask_bits(sg)
        share = np.mean(np.concatenate([d.ravel() for d, _ in dec.values()]))
        assert share > 0.5, f"{kw}: only {share:.2f} of the mask bits are decided"
        for s in range(sg.nseg):
            bits = sg.mask_bits(gotm, s)
            if s in dec:
                d, pos = dec[s]
                assert np.array_equal(bits[d], pos[d].astype(bits.dtype)), f"{kw} segment {s}: {np.count_nonzero(bits[d] != pos[d])} decided mask bits differ"
            else:                                                                 # count 0: the mask of the start value, exactly
                assert np.array_equal(bits, sg.mask_bits(refm, s)), f"{kw}: empty segment {s}: mask differs from the ext oracle"


def test_sigmoid_segments_match_the_ext_oracle():
    api = capi.load()
    for kw in (dict(m=20, n=12, k=16, beta=1), dict(m=32, n=32, k=32, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A)):
        sg = FusedSegments(api, seed=300, act=3, **kw)
        (got, gotm), (ref, _) = sg.run_checked(), sg.oracle_ext()
        tol = TOL_F32 if sg.case.c_type == DT.F32 else TOL_BF16
        for s in range(sg.nseg):
            err = normf_rel(sg.valid(ref, s), sg.valid(got, s), sg.case.c_type)
            assert err < tol, f"{kw} segment {s} (count {sg.counts[s]}): normf_rel = {err}"
        sg.assert_outside_untouched(got, gotm, str(kw))


def test_a_shared_bias_equals_a_list_of_equal_entries():
    api = capi.load()
    for kw in (dict(m=13, n=17, k=29, beta=1), dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A)):
        sg = FusedSegments(api, seed=350, colbias=True, act=2, **kw)
        one = int(sg.D.dev_ptrs(sg.dD, [1])[0])                                   # an odd element offset
        shared = sg.run_checked(shared_d=one)
        sg.di = np.ones(sg.nseg, dtype=np.int64)
        sg.d_ld = _up(sg.D.dev_ptrs(sg.dD, sg.di))
        listed = sg.run_checked()
        assert _same(shared[0], listed[0]) and _same(shared[1], listed[1]), f"{kw}: d_list = NULL differs from a d_list of equal entries"
        if sg.case.a_type == DT.F32:
            ref = sg.fma_chain()
            assert _same(listed[0], ref[0]) and _same(listed[1], ref[1])


LOOP_CASES = [dict(m=13, n=17, k=29, beta=1, colbias=True, act=2), dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, colbias=True, act=1)]


def test_the_fused_call_equals_its_loop_on_the_device():
    api = capi.load()
    for i, kw in enumerate(LOOP_CASES):
        sg = FusedSegments(api, seed=400 + i, exact=True, **kw)
        one, loop = sg.run_checked(), sg.run_loop()
        assert _same(one[0], loop[0]) and _same(one[1], loop[1]), f"{kw}: differs from the loop of fused single calls through the same handle"


def test_one_launch_per_call_through_the_fused_kernels():
    api = capi.load()
    for kw, name in ((dict(m=32, n=32, k=32, colbias=True, act=2), b"gemm_segments_f32_fused_kernel"),
                     (dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, colbias=True, act=1), b"gemm_segments_bf16_fused_kernel"),
                     (dict(m=23, n=23, k=23, a_type=DT.F64), b"gemm_segments_f64_kernel")):             # an ext handle without operators
        sg = FusedSegments(api, seed=450, **kw)
        out = sg.new_out()
        api.hip_launch_count(1)
        sg.run(out)
        assert api.hip_launch_count(1) == 1
        api.hip_sync(); api.check()
        assert api.hip_kernel_name(sg.ext_handle, 1) == name
        if sg.case.a_type == DT.F64:                                              # ... is the plain product; no mask byte is touched
            cset = sg.new_c()
            Segments.run(sg, cset)
            api.hip_sync(); api.check()
            assert _same(sg.result(out)[0], sg.C0.download(cset[0])) and _same(sg.result(out)[1], sg.M0.host)


MODE_CASES = [dict(m=32, n=32, k=32, colbias=True, act=2), dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, colbias=True, act=1)]


def test_modes_stream_pipeline_and_capture_keep_the_results():
    import torch
    api = capi.load()
    segs = [FusedSegments(api, seed=500 + i, **kw) for i, kw in enumerate(MODE_CASES)]
    want = [sg.run_checked() for sg in segs]                                      # blocking
    same = lambda sg, out, w: all(_same(x, y) for x, y in zip(sg.result(out), w))
    # stream-ordered on a torch stream
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    outs = [sg.new_out() for sg in segs]
    for sg, out in zip(segs, outs):
        sg.run(out)
    api.hip_sync(); api.check()
    assert all(same(sg, out, w) for sg, out, w in zip(segs, outs, want)), "stream-ordered"
    # inside a pipeline section
    outs = [sg.new_out() for sg in segs]
    assert api.hip_pipeline_begin(4) == 0
    for sg, out in zip(segs, outs):
        sg.run(out)
    assert api.hip_pipeline_end() == 0
    api.hip_sync(); api.check()
    assert all(same(sg, out, w) for sg, out, w in zip(segs, outs, want)), "pipeline section"
    api.hip_set_stream(None); api.hip_set_async(0)
    # one call captured on one stream: a single kernel node, no branches; three replays, each from a fresh C and mask
    for sg, w in zip(segs, want):
        out = sg.new_out()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            api.hip_set_stream(side.cuda_stream)
            api.hip_launch_count(1)
            g.capture_begin()
            sg.run(out)
            g.capture_end()
            assert api.hip_launch_count(0) == 1
        api.check()
        torch.cuda.current_stream().wait_stream(side)
        api.hip_set_stream(None); api.hip_set_async(0)
        for _ in range(3):
            for dev, pool in ((out["C"], sg.C0), (out["M"], sg.M0)):
                for d, h in zip(dev, pool.host):
                    if d is not None:
                        d.copy_(torch.from_numpy(h.view(np.int16) if h.dtype == np.uint16 else h))
            torch.cuda.synchronize()
            g.replay(); torch.cuda.synchronize()
            assert same(sg, out, w), "graph replay"


def _scale_fused(api, nseg, edge, beta, seed):
    """`nseg` f32 segments of edge^3 with skewed counts (1 %: 64, a few empty, the rest 2) on exact data, bias + ReLU + bitmask, against a numpy sum: the bias
    indexes C's rows, the mask is the sign of the sum."""
    rng = np.random.default_rng(seed)
    npool, e2, nb = 16, edge * edge, 5
    mask_ld = (edge + 15) // 16 * 16
    mb = mask_ld // 8 * edge
    counts = np.where(rng.random(nseg) < 0.01, 64, 2).astype(np.uint64)
    counts[::997] = 0
    seg_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    total = int(seg_ptr[-1])
    ai, bi, di = rng.integers(0, npool, total), rng.integers(0, npool, total), rng.integers(0, nb, nseg)
    A, B, C0, D = _ints(rng, npool * e2, DT.F32), _ints(rng, npool * e2, DT.F32), _ints(rng, nseg * e2, DT.F32), _ints(rng, nb * edge, DT.F32)
    M0 = rng.integers(0, 256, nseg * mb).astype(np.uint8)
    dA, dB, dC, dD, dM = _up(A), _up(B), _up(C0.copy()), _up(D), _up(M0.copy())
    seq = np.arange(nseg, dtype=np.int64)
    lists = [_up(seg_ptr), _up((dA.data_ptr() + ai * e2 * 4).astype(np.uint64)), _up((dB.data_ptr() + bi * e2 * 4).astype(np.uint64)),
             _up((dC.data_ptr() + seq * (e2 * 4)).astype(np.uint64)), _up((dD.data_ptr() + di * (edge * 4)).astype(np.uint64)), _up((dM.data_ptr() + seq * mb).astype(np.uint64))]
    case = GemmCase(edge, edge, edge, beta=beta, br_type=capi.BR_ADDRESS, br_count=1, colbias=True, act=2)
    h = case.dispatch(api)
    assert h
    p = capi.GemmExtParam()
    api.hip_launch_count(1)
    api.hip_gemm_ext_batch_reduce_segments(h, C.byref(p), nseg, *[x.data_ptr() for x in lists])
    assert api.hip_launch_count(1) == 1
    api.hip_sync(); api.check()
    got, gotm = _down(dC, C0).reshape(nseg, edge, edge), _down(dM, M0).reshape(nseg, edge, mask_ld // 8)
    # column-major blocks: as row-major arrays C^T = B^T A^T; every pair of pool blocks once, then per-product gathers (test_gemm_segments_gpu._scale)
    Am, Bm = A.reshape(npool, edge, edge).astype(np.int32), B.reshape(npool, edge, edge).astype(np.int32)
    pair = np.einsum("bjk,aki->abji", Bm, Am).reshape(npool * npool, e2)
    csum = np.zeros((total + 1, e2), dtype=np.int32)
    np.cumsum(pair[ai * npool + bi], axis=0, out=csum[1:])
    pre = (csum[seg_ptr[1:].astype(np.int64)] - csum[seg_ptr[:-1].astype(np.int64)]).reshape(nseg, edge, edge)
    pre = pre + D.reshape(nb, edge).astype(np.int32)[di][:, None, :]              # C(i, j) += bias[i]: i is the last axis
    if beta:
        pre = pre + C0.reshape(nseg, edge, edge).astype(np.int32)
    bad = np.flatnonzero((got.astype(np.float64) != np.maximum(pre, 0)).any(axis=(1, 2)))
    assert bad.size == 0, f"{bad.size} of {nseg} segments differ from the numpy sum, first: segment {bad[0]} (count {counts[bad[0]]})"
    assert not np.signbit(got).any()                                              # ReLU stores +0
    bits = np.unpackbits(M0.reshape(nseg, edge, mask_ld // 8), axis=2, bitorder="little")
    bits[:, :, :edge] = pre > 0
    badm = np.flatnonzero((gotm != np.packbits(bits, axis=2, bitorder="little")).any(axis=(1, 2)))
    assert badm.size == 0, f"the masks of {badm.size} of {nseg} segments differ (bits of the sum's sign, every other bit as prefilled), first: segment {badm[0]}"


def test_scale_sixty_thousand_fused_segments():
    api = capi.load()
    _scale_fused(api, 60000, 16, 0, 600)
    _scale_fused(api, 140000, 8, 1, 601)              # more items than one wave each: the waves grid-stride


def test_c_example_runs_a_block_row_loop_with_bias_and_relu(tmp_path):
    libdir = os.path.join(ROOT, "libxsmm_amd", "lib")
    exe = str(tmp_path / "segments_fused_driver")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "segments_fused_driver.c"),
           "-L" + libdir, "-lxsmm_amd", "-lm", "-Wl,-rpath," + libdir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "normf_rel" in r.stdout


def test_guarded_rerun_with_operands_flush_against_unmapped_memory():
    """The f32 and bf16 parity tests again with every upload flush against unmapped address space (tests/guard.py via tests/conftest.py): the main pools, the last
    A, B, C, bias and mask block (arrays of their own) and the six lists.  These are parity tests on valid inputs: an access outside an operand -- a bias load
    that is not clamped, a mask byte past its block -- would fault the subprocess.  The second side only runs once the first has passed."""
    for side in ("end", "front"):
        env = dict(os.environ, LIBXSMM_TEST_GUARD=side)
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
               "-k", "test_f32_fused_segments_are_bitwise or test_bf16_fused_segments_match", "-v", "--no-header"]
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
        print(f"guarded run ({side}): {time.time() - t0:.1f} s")
        assert r.returncode == 0, f"guarded run ({side}) ended with {r.returncode} (negative / 134: the GPU faulted on an out-of-bounds access):\n{tail}"
        assert "2 passed" in r.stdout, tail
