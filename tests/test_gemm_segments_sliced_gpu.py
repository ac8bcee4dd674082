"""libxsmm_hip_gemm_batch_reduce_segments_sliced / ..._offsets_sliced (include/libxsmm_hip.h): segments whose chains the caller has cut into slices.  f32 results
are bitwise the CPU statement of the semantics (tests/segments_sliced_helpers.py: per-slice fmaf chains from +0, float32 adds in slice order, then beta) in the
ADDRESS form and in all four OFFSET forms, with padded ldc and gaps that come back untouched; f64 and bf16 are bitwise on small integers and within the dense
kernels' tolerances on random values; one slice per block under beta = 0 is bitwise the unsliced call; two calls give the same bits, on another stream and with
re-uploaded lists; a call is two launches; the workspace is written inside the queried size only; both passes grid-stride; the launch modes and graph capture
keep the results.  The last test re-runs the parity tests with every operand flush against unmapped memory (run this file with -x)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import helpers
from helpers import GemmCase, TOL_BF16, TOL_F64, normf_rel
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG
from segments_sliced_helpers import PRODUCTS_PER_SLICE, SLICES_PER_BLOCK, csr, sliced_reference
from test_gemm_segments_gpu import Pool, _down, _ints, _up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

TA, TB = GEMM_FLAG.TRANS_A, GEMM_FLAG.TRANS_B
FORMS = {"NN": 0, "TN": TA, "NT": TB, "TT": TA | TB}
MID = 4                                        # the OFFSET bases point at block 4 of the A and B pools (block 2 of C): the blocks in front have negative offsets


class Sliced:
    """One sliced call: pools of A and B blocks, one C block per block of the two-level CSR, and the lists -- on the host for the CPU statement and on the device.
    `form` None is the ADDRESS entry, else the OFFSET entry in that transpose form."""

    def __init__(self, api, m, n, k, form=None, slices=SLICES_PER_BLOCK, products=PRODUCTS_PER_SLICE, a_type=DT.F32, c_type=None, flags=0, beta=0, pads=(0, 0, 0),
                 seed=0, exact=False, npool=9):
        self.api, self.form, self.beta = api, form, beta
        flags |= FORMS[form or "NN"]
        lda, ldb, ldc = (k if flags & TA else m) + pads[0], (n if flags & TB else k) + pads[1], m + pads[2]
        self.case = case = GemmCase(m, n, k, a_type=a_type, c_type=c_type, lda=lda, ldb=ldb, ldc=ldc, flags=flags, beta=beta,
                                    br_type=capi.BR_ADDRESS if form is None else capi.BR_OFFSET, br_count=1, batch=1, seed=seed)
        rng = np.random.default_rng(2000 + seed)
        gen = _ints if exact else helpers.rand_values
        self.blk_ptr, self.seg_ptr = csr(slices), csr(products)
        self.nblocks, self.nslices = len(slices), len(products)
        assert int(self.blk_ptr[-1]) == self.nslices and self.nblocks >= 4
        total = int(self.seg_ptr[-1])
        self.A = Pool(gen(rng, Pool.size(npool, case.a_elems), a_type), npool, case.a_elems)
        self.B = Pool(gen(rng, Pool.size(npool, case.b_elems), case.b_type), npool, case.b_elems)
        self.C0 = Pool(gen(rng, Pool.size(self.nblocks, case.c_elems), case.c_type), self.nblocks, case.c_elems)    # (the padding of ldc and the gaps hold values too)
        sl_of = np.repeat(np.arange(self.nslices), np.asarray(products, dtype=np.int64))
        r_of = np.arange(total) - self.seg_ptr[sl_of].astype(np.int64)
        self.ai = (sl_of * 3 + r_of) % npool                                      # A blocks are shared across slices and blocks ...
        self.bi = np.where(sl_of % 2 == 0, sl_of % npool, (sl_of + r_of) % npool)      # ... and even slices use ONE B for all their products
        self.dA, self.dB = self.A.upload(), self.B.upload()
        self.handle = case.dispatch(api)
        assert self.handle
        self.ws_bytes = api.hip_gemm_batch_reduce_segments_sliced_workspace(self.handle, self.nslices)
        api.check()
        self.upload_lists()

    def _mid(self, pool, block):
        return block * pool.pitch * pool.esz

    def upload_lists(self):
        pa, pb = self.A.dev_ptrs(self.dA, self.ai), self.B.dev_ptrs(self.dB, self.bi)
        if self.form is None:
            self.la, self.lb = pa, pb
        else:
            self.a_base, self.b_base = self.dA[0].data_ptr() + self._mid(self.A, MID), self.dB[0].data_ptr() + self._mid(self.B, MID)
            self.la, self.lb = pa.view(np.int64) - np.int64(self.a_base), pb.view(np.int64) - np.int64(self.b_base)
            assert (self.la < 0).any() or (self.lb < 0).any()
        self.d_blk, self.d_seg, self.d_la, self.d_lb = _up(self.blk_ptr), _up(self.seg_ptr), _up(self.la), _up(self.lb)

    def new_c(self):
        dC = self.C0.upload()
        pc = self.C0.dev_ptrs(dC, range(self.nblocks))
        if self.form is None:
            return dC, _up(pc), 0
        c_base = dC[0].data_ptr() + self._mid(self.C0, 2)
        return dC, _up(pc.view(np.int64) - np.int64(c_base)), c_base

    def new_ws(self, extra=0):
        return _up(np.full(self.ws_bytes + extra, 0xA5, dtype=np.uint8))

    def param(self, cset):
        p = capi.GemmParam()
        if self.form is not None:
            p.a.primary, p.b.primary, p.c.primary = self.a_base, self.b_base, cset[2]
        return p

    def run(self, cset, ws=None, ws_bytes=None):
        self.ws = ws if ws is not None else self.new_ws()                      # kept alive until the next call
        fn = self.api.hip_gemm_batch_reduce_segments_sliced if self.form is None else self.api.hip_gemm_batch_reduce_segments_offsets_sliced
        fn(self.handle, C.byref(self.param(cset)), self.nblocks, self.d_blk.data_ptr(), self.nslices, self.d_seg.data_ptr(), self.d_la.data_ptr(), self.d_lb.data_ptr(),
           cset[1].data_ptr(), self.ws.data_ptr(), self.ws_bytes if ws_bytes is None else ws_bytes)

    def run_unsliced(self, cset):
        """The unsliced sibling on the same lists: every slice a segment (one slice per block only)."""
        assert self.nslices == self.nblocks
        fn = self.api.hip_gemm_batch_reduce_segments if self.form is None else self.api.hip_gemm_batch_reduce_segments_offsets
        fn(self.handle, C.byref(self.param(cset)), self.nslices, self.d_seg.data_ptr(), self.d_la.data_ptr(), self.d_lb.data_ptr(), cset[1].data_ptr())

    def run_checked(self):
        cset = self.new_c()
        self.run(cset)
        self.api.hip_sync(); self.api.check()
        return self.C0.download(cset[0])

    def reference(self, fma=True):
        """The CPU statement of the semantics on the host pools, as arrays laid out like a download."""
        ha, hb = self.A.host_ptrs(self.ai), self.B.host_ptrs(self.bi)
        a0, b0 = self.A.host[0].ctypes.data, self.B.host[0].ctypes.data
        oa, ob = ha.view(np.int64) - np.int64(a0), hb.view(np.int64) - np.int64(b0)

        def param_of_slice(j):
            p = capi.GemmParam()
            r = int(self.seg_ptr[j]) * 8
            if self.form is None:
                p.a.primary, p.b.primary = ha.ctypes.data + r, hb.ctypes.data + r
            else:
                p.a.primary, p.b.primary, p.a.secondary, p.b.secondary = a0, b0, oa.ctypes.data + r, ob.ctypes.data + r
            return p

        blocks = sliced_reference(self.case, self.beta, self.blk_ptr, self.seg_ptr, param_of_slice, [self.C0.block(self.C0.host, b) for b in range(self.nblocks)], fma=fma)
        out = self.C0.copy()
        for b, blk in enumerate(blocks):
            self.C0.block(out.host, b)[:] = blk
        return out.host

    def valid(self, arrays, b):
        c = self.case
        return self.C0.block(arrays, b)[:c.ldc * c.n].reshape(c.n, c.ldc)[:, :c.m]

    def assert_padding_untouched(self, got, what):
        c = self.case
        for b in range(self.nblocks):
            g = self.C0.block(got, b)[:c.ldc * c.n].reshape(c.n, c.ldc)[:, c.m:]
            assert np.array_equal(g, self.C0.block(self.C0.host, b)[:c.ldc * c.n].reshape(c.n, c.ldc)[:, c.m:]), f"{what}: block {b} wrote beyond m x n"
        for a, b in zip(got, self.C0.host):                                       # the elements between the blocks
            if len(a) > c.c_elems:
                assert np.array_equal(a[c.c_elems::c.c_elems + 1], b[c.c_elems::c.c_elems + 1]), what


def _same(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# one 32-tile; ragged 16-tiles; several tiles with ragged k -- each with a padded ldc whose gaps hold values that must come back
F32_SHAPES = [dict(m=32, n=32, k=32, pads=(0, 0, 4)), dict(m=23, n=19, k=13, pads=(2, 3, 5)), dict(m=40, n=24, k=9, pads=(0, 0, 7)), dict(m=32, n=32, k=32)]


@pytest.mark.parametrize("form", [None] + list(FORMS), ids=["ADDRESS", "NN", "TN", "NT", "TT"])
def test_f32_sliced_segments_are_bitwise_the_statement(form):
    api = capi.load()
    for i, kw in enumerate(F32_SHAPES):
        for beta in (0, 1):
            sg = Sliced(api, form=form, beta=beta, seed=10 * i + beta, **kw)
            got, ref = sg.run_checked(), sg.reference()
            # whole arrays: the m x n blocks bit for bit, the padding of ldc and the gaps between the blocks unchanged
            assert _same(got, ref), f"{form} {kw} beta={beta}: differs from per-slice fmaf chains added in slice order (or wrote outside m x n)"
            v = sg.valid(got, 0)                                                  # the block without slices: +0 under beta = 0, untouched under beta = 1
            want = sg.valid(sg.C0.host, 0) if beta else np.zeros_like(v)
            assert np.array_equal(v.view(np.uint32), want.view(np.uint32)), f"{form} {kw} beta={beta}: the block without slices"


F64_SHAPES = [dict(m=23, n=19, k=13, pads=(2, 3, 5)), dict(m=16, n=16, k=16), dict(m=8, n=40, k=5, pads=(0, 0, 1))]


@pytest.mark.parametrize("form", [None, "NN", "TN"], ids=["ADDRESS", "NN", "TN"])
def test_f64_sliced_segments(form):
    api = capi.load()
    for i, kw in enumerate(F64_SHAPES):
        for beta in (0, 1):
            ex = Sliced(api, form=form, a_type=DT.F64, beta=beta, seed=100 + 10 * i + beta, exact=True, **kw)
            assert _same(ex.run_checked(), ex.reference()), f"{form} {kw} beta={beta}: exact data differs from the statement"
            sg = Sliced(api, form=form, a_type=DT.F64, beta=beta, seed=150 + 10 * i + beta, **kw)
            got, ref = sg.run_checked(), sg.reference()
            for b in range(sg.nblocks):
                err = normf_rel(sg.valid(ref, b), sg.valid(got, b), DT.F64)
                assert err < TOL_F64, f"{form} {kw} beta={beta} block {b}: normf_rel = {err}"
            sg.assert_padding_untouched(got, f"{form} {kw} beta={beta}")


# (A layout, C type): flat and VNNI-2 A, f32 and bf16 C; the 16-tile, the 32-tile, several tiles, ragged
BF16_CASES = [dict(m=32, n=32, k=32, c_type=DT.F32), dict(m=16, n=16, k=16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, beta=1), dict(m=13, n=17, k=29, c_type=DT.BF16, pads=(0, 0, 3)),
              dict(m=64, n=64, k=64, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A), dict(m=24, n=40, k=34, c_type=DT.F32, flags=GEMM_FLAG.VNNI_A, pads=(3, 3, 6), beta=1),
              dict(m=13, n=13, k=13, c_type=DT.BF16, beta=1), dict(m=24, n=16, k=32, c_type=DT.BF16, beta=1, pads=(0, 0, 8))]


@pytest.mark.parametrize("form", [None, "NN", "TN"], ids=["ADDRESS", "NN", "TN"])
def test_bf16_sliced_segments(form):
    api = capi.load()
    for i, kw in enumerate(BF16_CASES):
        if form == "TN" and kw.get("flags", 0) & GEMM_FLAG.VNNI_A:
            continue                                                              # a transposed A is flat
        ex = Sliced(api, form=form, a_type=DT.BF16, seed=250 + i, exact=True, **kw)
        got = ex.run_checked()
        assert _same(got, ex.reference()), f"{form} {kw}: exact data differs from the statement"
        sg = Sliced(api, form=form, a_type=DT.BF16, seed=200 + i, **kw)
        got, ref = sg.run_checked(), sg.reference()
        for b in range(sg.nblocks):
            err = normf_rel(sg.valid(ref, b), sg.valid(got, b), sg.case.c_type)
            assert err < TOL_BF16, f"{form} {kw} block {b}: normf_rel = {err}"
        sg.assert_padding_untouched(got, f"{form} {kw}")


ONE_SLICE = [dict(m=32, n=32, k=32), dict(m=23, n=19, k=13, pads=(2, 3, 5), form="NT"), dict(m=40, n=24, k=9, form="TN"), dict(m=23, n=23, k=23, a_type=DT.F64),
             dict(m=16, n=16, k=16, a_type=DT.F64, form="TN"), dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A),
             dict(m=24, n=40, k=34, a_type=DT.BF16, c_type=DT.F32, form="NN", pads=(3, 3, 6))]


def test_one_slice_per_block_is_bitwise_the_unsliced_call():
    api = capi.load()
    products = [0, 3, 64, 1, 2, 7, 19]
    for i, kw in enumerate(ONE_SLICE):
        sg = Sliced(api, slices=[1] * len(products), products=products, beta=0, seed=300 + i, **kw)       # random values: the same chain, the same bits
        want = sg.new_c()
        sg.run_unsliced(want)
        api.hip_sync(); api.check()
        assert _same(sg.run_checked(), sg.C0.download(want[0])), f"{kw}: differs from the unsliced entry on the same lists"


def test_two_calls_give_the_same_bits_on_another_stream_and_with_reuploaded_lists():
    import torch
    api = capi.load()
    for i, kw in enumerate((dict(m=40, n=24, k=9, form="NT", beta=1, pads=(0, 0, 7)), dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A),
                            dict(m=23, n=19, k=13, a_type=DT.F64, beta=1))):
        sg = Sliced(api, seed=350 + i, **kw)
        first = sg.run_checked()
        side = torch.cuda.Stream()
        api.hip_set_stream(side.cuda_stream)
        cset = sg.new_c()
        torch.cuda.synchronize()
        sg.run(cset)
        api.hip_sync(); api.check()
        api.hip_set_stream(None); api.hip_set_async(0)
        assert _same(sg.C0.download(cset[0]), first), f"{kw}: another stream"
        old = (sg.d_blk, sg.d_seg, sg.d_la, sg.d_lb)                              # kept alive: the new lists lie elsewhere
        sg.upload_lists()
        assert sg.d_la.data_ptr() != old[2].data_ptr()
        assert _same(sg.run_checked(), first), f"{kw}: re-uploaded lists"


def test_a_call_is_two_launches_through_the_new_kernels():
    api = capi.load()
    for kw, name in ((dict(m=32, n=32, k=32), b"gemm_segments_sliced_f32_kernel"), (dict(m=23, n=19, k=13, a_type=DT.F64), b"gemm_segments_sliced_f64_kernel"),
                     (dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A), b"gemm_segments_sliced_bf16_kernel"),
                     (dict(m=32, n=32, k=32, form="TN"), b"gemm_segments_offs_sliced_f32_kernel<1,0>"), (dict(m=23, n=19, k=13, a_type=DT.F64, form="NT"), b"gemm_segments_offs_sliced_f64_kernel<0,1>"),
                     (dict(m=32, n=32, k=32, a_type=DT.BF16, form="TT"), b"gemm_segments_offs_sliced_bf16_kernel<1,1>")):
        sg = Sliced(api, seed=400, **kw)
        cset = sg.new_c()
        api.hip_launch_count(1)
        sg.run(cset)
        assert api.hip_launch_count(1) == 2
        api.hip_sync(); api.check()
        assert api.hip_kernel_name(sg.handle, 1) == name
    # no slices: the first launch is skipped, the blocks are +0 (beta = 0); no blocks: nothing
    sg = Sliced(api, m=32, n=32, k=32, seed=401)
    cset = sg.new_c()
    zeros = _up(np.zeros(sg.nblocks + 1, dtype=np.uint64))
    api.hip_launch_count(1)
    api.hip_gemm_batch_reduce_segments_sliced(sg.handle, C.byref(capi.GemmParam()), sg.nblocks, zeros.data_ptr(), 0, None, None, None, cset[1].data_ptr(), None, 0)
    assert api.hip_launch_count(1) == 1
    api.hip_sync(); api.check()
    got = sg.C0.download(cset[0])
    for b in range(sg.nblocks):
        assert not sg.valid(got, b).view(np.uint32).any()
    api.hip_gemm_batch_reduce_segments_sliced(sg.handle, C.byref(capi.GemmParam()), 0, None, 0, None, None, None, None, None, 0)
    assert api.hip_launch_count(1) == 0
    api.check()


def test_the_workspace_is_written_inside_the_queried_size_only():
    api = capi.load()
    for i, kw in enumerate((dict(m=23, n=19, k=13), dict(m=23, n=19, k=13, a_type=DT.F64, form="TN"), dict(m=40, n=24, k=9, a_type=DT.BF16, c_type=DT.BF16, form="NN"))):
        sg = Sliced(api, seed=450 + i, **kw)
        ws = sg.new_ws(extra=64)                                                  # 64 bytes more than asked for, a pattern in all of it
        cset = sg.new_c()
        sg.run(cset, ws=ws)
        api.hip_sync(); api.check()
        if sg.case.a_type == DT.F32:
            assert _same(sg.C0.download(cset[0]), sg.reference()), kw
        tail = _down(ws, np.zeros(1, dtype=np.uint8))[sg.ws_bytes:]
        assert tail.size == 64 and (tail == 0xA5).all(), f"{kw}: bytes beyond the queried size were written"
        cset = sg.new_c()                                                         # one byte short: -2, nothing launched, C untouched
        api.hip_launch_count(1)
        sg.run(cset, ws=ws, ws_bytes=sg.ws_bytes - 1)
        assert api.hip_get_last_error() == -2 and api.hip_launch_count(1) == 0
        api.hip_clear_last_error()
        assert _same(sg.C0.download(cset[0]), sg.C0.host)


def _grid_stride(api, nblocks, per_block, beta, seed):
    """`nblocks` blocks of `per_block` slices of ONE 4 x 4 x 4 f32 product each, on small integers, every block against a numpy integer sum."""
    rng = np.random.default_rng(seed)
    npool, e, e2 = 16, 4, 16
    nslices = nblocks * per_block
    blk_ptr = np.arange(nblocks + 1, dtype=np.uint64) * per_block
    seg_ptr = np.arange(nslices + 1, dtype=np.uint64)
    ai, bi = rng.integers(0, npool, nslices), rng.integers(0, npool, nslices)
    A, B, C0 = _ints(rng, npool * e2, DT.F32), _ints(rng, npool * e2, DT.F32), _ints(rng, nblocks * e2, DT.F32)
    dA, dB, dC = _up(A), _up(B), _up(C0.copy())
    lists = [_up(seg_ptr), _up((dA.data_ptr() + ai * e2 * 4).astype(np.uint64)), _up((dB.data_ptr() + bi * e2 * 4).astype(np.uint64)),
             _up((dC.data_ptr() + np.arange(nblocks, dtype=np.int64) * (e2 * 4)).astype(np.uint64))]
    d_blk = _up(blk_ptr)
    h = GemmCase(e, e, e, beta=beta, br_type=capi.BR_ADDRESS, br_count=1, batch=1).dispatch(api)
    assert h
    nbytes = api.hip_gemm_batch_reduce_segments_sliced_workspace(h, nslices)
    ws = _up(np.zeros(nbytes, dtype=np.uint8))
    api.hip_launch_count(1)
    api.hip_gemm_batch_reduce_segments_sliced(h, C.byref(capi.GemmParam()), nblocks, d_blk.data_ptr(), nslices, *[x.data_ptr() for x in lists], ws.data_ptr(), nbytes)
    assert api.hip_launch_count(1) == 2
    api.hip_sync(); api.check()
    got = _down(dC, C0).reshape(nblocks, e2)
    Am, Bm = A.reshape(npool, e, e).astype(np.int32), B.reshape(npool, e, e).astype(np.int32)
    pair = np.einsum("bjk,aki->abji", Bm, Am).reshape(npool * npool, e2)          # column-major blocks: as row-major arrays C^T = B^T A^T
    ref = pair[ai * npool + bi].reshape(nblocks, per_block, e2).sum(axis=1)
    if beta:
        ref = ref + C0.reshape(nblocks, e2).astype(np.int32)
    bad = np.flatnonzero((got.astype(np.float64) != ref).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {nblocks} blocks differ from the numpy sum, first: block {bad[0]}"


def test_both_passes_grid_stride():
    """140 000 slices in 35 000 blocks: more (slice, tile) items than one wave each in pass 1.  A 4 x 4 block is one run of pass 2, so its waves only grid-stride with
    more than 131 072 BLOCKS: the second call has 140 000 blocks of one slice."""
    api = capi.load()
    _grid_stride(api, 35000, 4, 1, 500)
    _grid_stride(api, 140000, 1, 0, 501)


def test_modes_stream_pipeline_and_coalescing_keep_the_results():
    import torch
    from test_gemm_grouped_gpu import Group
    api = capi.load()
    segs = [Sliced(api, seed=600 + i, **kw) for i, kw in enumerate((dict(m=32, n=32, k=32, form="NT", beta=1), dict(m=23, n=19, k=13, a_type=DT.F64, beta=1),
                                                                    dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, form="TN")))]
    strided = Group(api, GemmCase(m=32, n=32, k=32, batch=40, seed=612))
    want = [sg.run_checked() for sg in segs]                                  # blocking
    want_strided = strided.run_own(api)
    workspaces = [sg.new_ws() for sg in segs]                                 # one per call in flight
    # stream-ordered on a torch stream
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    csets = [sg.new_c() for sg in segs]
    for sg, cs, ws in zip(segs, csets, workspaces):
        sg.run(cs, ws=ws)
    api.hip_sync(); api.check()
    for sg, cs, w in zip(segs, csets, want):
        assert _same(sg.C0.download(cs[0]), w), "stream-ordered"
    # inside a pipeline section, next to a strided call: both launches of a call go to one lane
    csets = [sg.new_c() for sg in segs]
    assert api.hip_pipeline_begin(4) == 0
    segs[0].run(csets[0], ws=workspaces[0])
    segs[1].run(csets[1], ws=workspaces[1])
    api.hip_gemm_batch_strided(strided.handle, C.byref(strided.param), strided.case.batch, strided.sa, strided.sb, strided.case.bs_c)
    segs[2].run(csets[2], ws=workspaces[2])
    assert api.hip_pipeline_end() == 0
    api.hip_sync(); api.check()
    for sg, cs, w in zip(segs, csets, want):
        assert _same(sg.C0.download(cs[0]), w), "pipeline section"
    assert np.array_equal(strided.result().view(np.uint8), want_strided.view(np.uint8))
    # coalescing: a queued single call writes the block that every product of the sliced call reads as A; the queue is flushed first
    m = 32
    rng = np.random.default_rng(620)
    X, Y = (torch.from_numpy(_ints(rng, m * m, DT.F32)).to("cuda:0") for _ in range(2))
    Bs = torch.from_numpy(_ints(rng, 3 * m * m, DT.F32)).to("cuda:0")
    T = torch.zeros(m * m, dtype=torch.float32, device="cuda:0")
    out = torch.zeros(2 * m * m, dtype=torch.float32, device="cuda:0")
    plain = GemmCase(m, m, m, seed=621).dispatch(api)
    adr = GemmCase(m, m, m, br_type=capi.BR_ADDRESS, br_count=1, seed=622).dispatch(api)
    blk_ptr = torch.tensor([0, 1, 3], dtype=torch.int64, device="cuda:0")     # block 0: one slice; block 1: two slices of one product
    seg_ptr = torch.tensor([0, 1, 2, 3], dtype=torch.int64, device="cuda:0")
    la = torch.tensor([T.data_ptr()] * 3, dtype=torch.int64, device="cuda:0")
    lb = torch.tensor([Bs.data_ptr() + i * m * m * 4 for i in range(3)], dtype=torch.int64, device="cuda:0")
    lc = torch.tensor([out.data_ptr(), out.data_ptr() + m * m * 4], dtype=torch.int64, device="cuda:0")
    nbytes = api.hip_gemm_batch_reduce_segments_sliced_workspace(adr, 3)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    api.hip_set_async(2)
    p = capi.GemmParam(); p.a.primary, p.b.primary, p.c.primary = X.data_ptr(), Y.data_ptr(), T.data_ptr()
    capi.Api.call(plain, p)                                                   # queued, nothing launched yet
    api.hip_gemm_batch_reduce_segments_sliced(adr, C.byref(capi.GemmParam()), 2, blk_ptr.data_ptr(), 3, seg_ptr.data_ptr(), la.data_ptr(), lb.data_ptr(), lc.data_ptr(),
                                              ws.data_ptr(), nbytes)
    api.hip_sync(); api.check()
    api.hip_set_async(0); api.hip_set_stream(None)
    col = lambda t: t.cpu().numpy().astype(np.float64).reshape(m, m).T        # column-major block -> matrix
    Tm = col(X) @ col(Y)
    Bm = [col(Bs[i * m * m:(i + 1) * m * m]) for i in range(3)]
    got = out.cpu().numpy().astype(np.float64).reshape(2, m, m)
    assert np.array_equal(got[0].T, Tm @ Bm[0]) and np.array_equal(got[1].T, Tm @ Bm[1] + Tm @ Bm[2])


def test_a_captured_call_replays_on_new_operand_values():
    """One call captured on one stream (two kernel nodes in order); A is overwritten in place, the graph is replayed once and compared with a fresh call."""
    import torch
    api = capi.load()
    sg = Sliced(api, m=32, n=32, k=32, form="NT", seed=700)
    new = Sliced(api, m=32, n=32, k=32, form="NT", seed=701)                  # same pattern and layout, other values
    cset, ws = sg.new_c(), sg.new_ws()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        api.hip_set_stream(side.cuda_stream)
        api.hip_launch_count(1)
        g.capture_begin()
        sg.run(cset, ws=ws)
        g.capture_end()
        assert api.hip_launch_count(0) == 2
    api.check()
    torch.cuda.current_stream().wait_stream(side)
    api.hip_set_stream(None); api.hip_set_async(0)
    for d, h in zip(sg.dA, new.A.host):                                       # A in place; B and C keep their values
        d.copy_(torch.from_numpy(h))
    torch.cuda.synchronize()
    g.replay(); torch.cuda.synchronize()
    got = sg.C0.download(cset[0])
    sg.A = new.A
    assert _same(got, sg.run_checked()), "the replay differs from a fresh call on the new A"
    assert _same(got, sg.reference())


def test_c_example_computes_a_block_sparse_weight_gradient_in_one_sliced_call(tmp_path):
    libdir = os.path.join(ROOT, "libxsmm_amd", "lib")
    exe = str(tmp_path / "segments_sliced_driver")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "segments_sliced_driver.c"),
           "-L" + libdir, "-lxsmm_amd", "-lm", "-Wl,-rpath," + libdir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "normf_rel" in r.stdout and "2 launches" in r.stdout


GUARDED = "test_f32_sliced_segments_are_bitwise or test_f64_sliced_segments or test_bf16_sliced_segments or test_both_passes_grid_stride"


def test_guarded_rerun_with_operands_flush_against_unmapped_memory():
    """The parity and grid-stride tests again with every upload flush against unmapped address space (tests/guard.py via tests/conftest.py): the pools, the last A,
    B and C block (arrays of their own), the five lists and the workspace, which is exactly as large as the query says.  These are parity tests on valid inputs: an
    access outside an operand would fault the subprocess.  Why none is expected: pass 1 is the unsliced kernels' item loop, whose loads clamp to the operands, and
    stores a dense m x n partial; in pass 2 a lane's 16-byte load starts at an element below m * n of a partial that is padded to a multiple of 16 bytes, and C is
    read and written at i < m, j < n only.  The second side only runs once the first has passed."""
    for side in ("end", "front"):
        env = dict(os.environ, LIBXSMM_TEST_GUARD=side)
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "-k", GUARDED, "-v", "--no-header"]
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
        print(f"guarded run ({side}): {time.time() - t0:.1f} s")
        assert r.returncode == 0, f"guarded run ({side}) ended with {r.returncode} (negative / 134: the GPU faulted on an out-of-bounds access):\n{tail}"
        assert "12 passed" in r.stdout, tail
