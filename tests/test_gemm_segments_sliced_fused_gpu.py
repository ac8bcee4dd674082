"""libxsmm_hip_gemm_ext_batch_reduce_segments_sliced / ..._offsets_sliced (include/libxsmm_hip.h): sliced segments through an ext handle -- column bias, ReLU
(+ bitmask), sigmoid applied to the blocks' sums in the second launch.  f32 results are bitwise the CPU statement of the semantics
(tests/segments_sliced_fused_helpers.py), whole C and whole mask arrays -- padding, gaps, bits beyond m and the bytes between the blocks included -- in the
ADDRESS form and in all four OFFSET forms, at the shapes where a mask byte straddles an element run of the second pass; bf16 is bitwise on exact data and within
the dense kernels' tolerances on random data, with every mask bit the float64 restatement decides; one slice per block without a bias under beta = 0 is bitwise
the unsliced ext call; blocks without slices are the unsliced call's segments of count 0; an ext handle without operators is the plain sliced call; two calls
give the same bits; a call is two launches; the launch modes, graph capture and a grid-striding second pass keep the results.  The last test re-runs the parity
tests with every operand flush against unmapped memory (run this file with -x)."""
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
from segments_sliced_fused_helpers import sliced_fused_reference
from segments_sliced_helpers import PRODUCTS_PER_SLICE, SLICES_PER_BLOCK
from test_gemm_segments_gpu import Pool, _down, _ints, _same, _up
from test_gemm_segments_sliced_gpu import FORMS, Sliced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

NBIAS = 4      # bias blocks, one element apart (every alignment an element allows); the blocks share them


class SlicedFused(Sliced):
    """A sliced call with an epilogue: the plain sliced call's pools and lists, a pool of bias vectors that the blocks share and one mask block per C block,
    prefilled with random bytes.  set_epilogue picks the ext handle; the pools stay.  In the OFFSET form the bias base is bias block 1 and the mask base mask
    block 2, so the blocks in front have negative offsets."""

    def __init__(self, api, m, n, k, colbias=False, act=0, **kw):
        super().__init__(api, m, n, k, **kw)
        case = self.case
        rng = np.random.default_rng(7000 + kw.get("seed", 0))
        gen = _ints if kw.get("exact", False) else helpers.rand_values
        self.D = Pool(gen(rng, Pool.size(NBIAS, m), case.c_type), NBIAS, m)
        self.di = (np.arange(self.nblocks) * 3) % NBIAS                           # 0, 3, 2, 1, 0: repeated entries, the last block among them
        self.M0 = Pool(rng.integers(0, 256, Pool.size(self.nblocks, case.mask_bytes)).astype(np.uint8), self.nblocks, case.mask_bytes)
        self.dD = self.D.upload()
        self.plain_handle, self.plain_ws_bytes = self.handle, self.ws_bytes
        self.set_epilogue(colbias, act)

    def set_epilogue(self, colbias, act):
        c = self.case
        self.colbias, self.act = colbias, act
        self.ext = GemmCase(c.m, c.n, c.k, a_type=c.a_type, c_type=c.c_type, lda=c.lda, ldb=c.ldb, ldc=c.ldc, flags=c.flags & ~GEMM_FLAG.BETA_0, beta=self.beta,
                            br_type=c.br_type, br_count=1, colbias=colbias, act=act)      # (descriptor only: its operands are not used)
        self.handle = self.api.dispatch_brgemm_ext(self.ext.shape(), self.ext.flags, 0, self.ext.brcfg(), self.ext.argops(), self.ext.postops())
        assert self.handle
        self.ws_bytes = self.api.hip_gemm_ext_batch_reduce_segments_sliced_workspace(self.handle, self.nslices)
        self.api.check()
        assert self.ws_bytes == self.plain_ws_bytes
        return self

    # ---- device ---------------------------------------------------------------------------------------------------------------------------------
    def new_out(self):
        dC, lc, c_base = self.new_c()
        dM = self.M0.upload()
        pd, pm = self.D.dev_ptrs(self.dD, self.di), self.M0.dev_ptrs(dM, range(self.nblocks))
        d_base = m_base = 0
        if self.form is not None:
            d_base, m_base = int(self.D.dev_ptrs(self.dD, [1])[0]), int(self.M0.dev_ptrs(dM, [2])[0])
            pd, pm = pd.view(np.int64) - np.int64(d_base), pm.view(np.int64) - np.int64(m_base)
            assert (pm < 0).any()
        return dict(C=dC, lc=lc, c_base=c_base, M=dM, ld=_up(pd), lm=_up(pm), d_base=d_base, m_base=m_base)

    def ext_param(self, out, shared_d=None):
        p = capi.GemmExtParam()
        if self.form is not None:
            p.a.primary, p.b.primary, p.c.primary, p.d.primary, p.c.secondary = self.a_base, self.b_base, out["c_base"], out["d_base"], out["m_base"]
        if shared_d is not None:
            p.d.primary = shared_d
        return p

    def run(self, out, ws=None, ws_bytes=None, shared_d=None):
        """shared_d: a device address -- d_list / d_offs = NULL and param->d.primary carries the one bias of every block."""
        self.ws = ws if ws is not None else self.new_ws()                      # kept alive until the next call
        fn = self.api.hip_gemm_ext_batch_reduce_segments_sliced if self.form is None else self.api.hip_gemm_ext_batch_reduce_segments_offsets_sliced
        ld = out["ld"].data_ptr() if self.colbias and shared_d is None else None
        fn(self.handle, C.byref(self.ext_param(out, shared_d)), self.nblocks, self.d_blk.data_ptr(), self.nslices, self.d_seg.data_ptr(), self.d_la.data_ptr(),
           self.d_lb.data_ptr(), out["lc"].data_ptr(), ld, out["lm"].data_ptr() if self.act == 2 else None, self.ws.data_ptr(), self.ws_bytes if ws_bytes is None else ws_bytes)

    def run_unsliced(self, out, seg=None):
        """The unsliced ext sibling on the same lists: every slice a segment (one slice per block only).  `seg`: another seg_ptr on the device."""
        assert self.nslices == self.nblocks or seg is not None
        fn = self.api.hip_gemm_ext_batch_reduce_segments if self.form is None else self.api.hip_gemm_ext_batch_reduce_segments_offsets
        fn(self.handle, C.byref(self.ext_param(out)), self.nblocks, (seg if seg is not None else self.d_seg).data_ptr(), self.d_la.data_ptr(), self.d_lb.data_ptr(),
           out["lc"].data_ptr(), out["ld"].data_ptr() if self.colbias else None, out["lm"].data_ptr() if self.act == 2 else None)

    def run_plain(self, out):
        """The plain sliced entry on the matching plain handle."""
        self.ws = self.new_ws()
        fn = self.api.hip_gemm_batch_reduce_segments_sliced if self.form is None else self.api.hip_gemm_batch_reduce_segments_offsets_sliced
        fn(self.plain_handle, C.byref(self.param((out["C"], out["lc"], out["c_base"]))), self.nblocks, self.d_blk.data_ptr(), self.nslices, self.d_seg.data_ptr(),
           self.d_la.data_ptr(), self.d_lb.data_ptr(), out["lc"].data_ptr(), self.ws.data_ptr(), self.plain_ws_bytes)

    def result(self, out):
        return self.C0.download(out["C"]), self.M0.download(out["M"])

    def run_checked(self, **kw):
        out = self.new_out()
        self.run(out, **kw)
        self.api.hip_sync(); self.api.check()
        return self.result(out)

    # ---- host ------------------------------------------------------------------------------------------------------------------------------------
    def bias_of(self, b):
        return self.D.block(self.D.host, int(self.di[b]))

    def reference(self, fma=True):
        """The CPU statement on the host pools: (C arrays, mask arrays) laid out like a download."""
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

        nb = range(self.nblocks)
        cb, mb = sliced_fused_reference(self.case, self.beta, self.colbias, self.act, self.blk_ptr, self.seg_ptr, param_of_slice,
                                        [self.C0.block(self.C0.host, b) for b in nb], self.bias_of, [self.M0.block(self.M0.host, b) for b in nb], fma=fma)
        outc, outm = self.C0.copy(), self.M0.copy()
        for b in nb:
            self.C0.block(outc.host, b)[:] = cb[b]
            self.M0.block(outm.host, b)[:] = mb[b]
        return outc.host, outm.host

    def mask_rows(self, arrays, b):
        c = self.case
        return self.M0.block(arrays, b).reshape(c.n, c.mask_ld // 8)

    def mask_bits(self, arrays, b):
        return np.unpackbits(self.mask_rows(arrays, b), axis=1, bitorder="little")[:, :self.case.m]

    def pre64(self):
        """Per block: (pre-activation sum, sum of magnitudes, terms) in float64 as [n][m] -- tests/gemm_ld_helpers.py's restatement (flat and VNNI-2 A, flat B)."""
        c = self.case
        assert not c.flags & (GEMM_FLAG.TRANS_A | GEMM_FLAG.TRANS_B)
        out = []
        for b in range(self.nblocks):
            r0, r1 = int(self.seg_ptr[int(self.blk_ptr[b])]), int(self.seg_ptr[int(self.blk_ptr[b + 1])])
            nsl = int(self.blk_ptr[b + 1]) - int(self.blk_ptr[b])
            pre, mag, terms = np.zeros((c.n, c.m)), np.zeros((c.n, c.m)), (r1 - r0) * c.k + nsl
            for r in range(r0, r1):
                a, bb = as_float(self.A.block(self.A.host, int(self.ai[r])), c.a_type), as_float(self.B.block(self.B.host, int(self.bi[r])), c.a_type)
                if c.flags & GEMM_FLAG.VNNI_A:                                     # [k / 2][lda][2] -> [k][lda]
                    kp = (c.k + 1) // 2
                    a = a[:kp * c.lda * 2].reshape(kp, c.lda, 2).transpose(0, 2, 1).reshape(2 * kp, c.lda)[:c.k]
                else:
                    a = a[:c.k * c.lda].reshape(c.k, c.lda)
                am, bm = a[:, :c.m], bb[:c.n * c.ldb].reshape(c.n, c.ldb)[:, :c.k]
                pre += bm @ am; mag += np.abs(bm) @ np.abs(am)
            if self.beta:
                c0 = as_float(self.valid(self.C0.host, b), c.c_type)
                pre, mag, terms = pre + c0, mag + np.abs(c0), terms + 1
            if self.colbias:
                bias = as_float(self.bias_of(b), c.c_type)[None, :]
                pre, mag, terms = pre + bias, mag + np.abs(bias), terms + 1
            out.append((pre, mag, terms))
        return out

    def assert_outside_untouched(self, got, gotm, what):
        self.assert_padding_untouched(got, what)
        if self.act != 2:
            assert _same(gotm, self.M0.host), f"{what}: a mask block was written without a bitmask"
            return
        c = self.case
        for b in range(self.nblocks):
            g = np.unpackbits(self.mask_rows(gotm, b), axis=1, bitorder="little")[:, c.m:]
            assert np.array_equal(g, np.unpackbits(self.mask_rows(self.M0.host, b), axis=1, bitorder="little")[:, c.m:]), f"{what}: block {b}: mask bits beyond m changed"
        for a, b in zip(gotm, self.M0.host):                                      # the bytes between the blocks
            if len(a) > c.mask_bytes:
                assert np.array_equal(a[c.mask_bytes::c.mask_bytes + 1], b[c.mask_bytes::c.mask_bytes + 1]), what


def decided_mask_bits(sg):
    """Per block with slices: (decided, positive) -- the mask bits the float64 restatement decides beyond the accumulation's error bound, and their value."""
    out = {}
    for b, (pre, mag, terms) in enumerate(sg.pre64()):
        if sg.blk_ptr[b + 1] > sg.blk_ptr[b]:
            _, bound_pre = bound64(sg.case, pre, mag, terms)
            out[b] = (np.abs(pre) > bound_pre, pre > 0)
    return out


# the wide path with one byte per lane pair; the 16-tile; m % 8 != 0 with three element runs (dense element 256 is row 9 of column 19: a mask byte straddles
# the runs); m < 8 (every column one partial byte, element 256 inside column 51); m % 4 == 0 but % 8 != 0 with padded leading dimensions (element 256 is row 4
# of column 7); two runs with m % 4 == 0; several tiles and seven runs
F32_SHAPES = [dict(m=32, n=32, k=32), dict(m=16, n=16, k=16), dict(m=13, n=41, k=29), dict(m=5, n=60, k=7), dict(m=36, n=20, k=18, pads=(3, 2, 4)),
              dict(m=12, n=30, k=9), dict(m=40, n=40, k=40)]
RAGGED = F32_SHAPES[2:6]
EPILOGUES = [(True, 0), (True, 1), (False, 2), (True, 2)]          # bias only, bias + ReLU, ReLU + bitmask, bias + ReLU + bitmask


@pytest.mark.parametrize("form", [None] + list(FORMS), ids=["ADDRESS", "NN", "TN", "NT", "TT"])
def test_f32_sliced_fused_segments_are_bitwise_the_statement(form):
    api = capi.load()
    for i, kw in enumerate(F32_SHAPES if form in (None, "NN") else RAGGED):
        for beta in (0, 1):
            sg = SlicedFused(api, form=form, beta=beta, seed=10 * i + beta, **kw)
            for colbias, act in EPILOGUES:
                what = f"{form} {kw} beta={beta} colbias={colbias} act={act}"
                sg.set_epilogue(colbias, act)
                (got, gotm), (ref, refm) = sg.run_checked(), sg.reference()
                # whole arrays: the m x n blocks and their mask bits are the statement's, every other byte and bit (padding, gaps, bits beyond m) is the caller's
                assert _same(got, ref), f"{what}: C differs from the statement (or bytes outside m x n changed)"
                assert _same(gotm, refm), f"{what}: the mask differs from !(x <= 0) of the sum (or bits outside m x n changed)"


# (A layout, C type): flat and VNNI-2 A, f32 and bf16 C; the 32-tile, the 16-tile, ragged with bytes that straddle runs, several tiles, padded
BF16_CASES = [dict(m=32, n=32, k=32, c_type=DT.F32), dict(m=16, n=16, k=16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, beta=1), dict(m=13, n=41, k=29, c_type=DT.BF16),
              dict(m=64, n=64, k=64, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A), dict(m=36, n=20, k=18, c_type=DT.F32, flags=GEMM_FLAG.VNNI_A, pads=(3, 2, 4), beta=1),
              dict(m=5, n=60, k=7, c_type=DT.BF16, beta=1)]


@pytest.mark.parametrize("form", [None, "NN"], ids=["ADDRESS", "NN"])
def test_bf16_sliced_fused_segments(form):
    api = capi.load()
    for i, kw in enumerate(BF16_CASES):
        ex = SlicedFused(api, form=form, a_type=DT.BF16, seed=250 + i, exact=True, colbias=True, act=2, **kw)
        (got, gotm), (ref, refm) = ex.run_checked(), ex.reference()
        assert _same(got, ref) and _same(gotm, refm), f"{form} {kw}: exact data differs from the statement (C {_same(got, ref)}, mask {_same(gotm, refm)})"
        sg = SlicedFused(api, form=form, a_type=DT.BF16, seed=200 + i, colbias=True, act=2, **kw)
        (got, gotm), (ref, refm) = sg.run_checked(), sg.reference()
        tol = TOL_F32 if sg.case.c_type == DT.F32 else TOL_BF16
        for b in range(sg.nblocks):
            err = normf_rel(sg.valid(ref, b), sg.valid(got, b), sg.case.c_type)
            print(f"{form} {kw} block {b}: normf_rel = {err}")
            assert err < tol, f"{form} {kw} block {b}: normf_rel = {err}"
        sg.assert_outside_untouched(got, gotm, f"{form} {kw}")
        dec = decided_mask_bits(sg)
        share = np.mean(np.concatenate([d.ravel() for d, _ in dec.values()]))
        print(f"{form} {kw}: decided share {share:.3f}")
        assert share > 0.5, f"{kw}: only {share:.2f} of the mask bits are decided"
        for b in range(sg.nblocks):
            bits = sg.mask_bits(gotm, b)
            if b in dec:
                d, pos = dec[b]
                assert np.array_equal(bits[d], pos[d].astype(bits.dtype)), f"{form} {kw} block {b}: {np.count_nonzero(bits[d] != pos[d])} decided mask bits differ"
            else:                                                                 # no slices: the mask of the start value, exactly
                assert np.array_equal(bits, sg.mask_bits(refm, b)), f"{form} {kw}: block {b} without slices: mask differs from the statement"


SIGMOID_CASES = [dict(m=20, n=12, k=16, beta=1, colbias=True), dict(m=32, n=32, k=32, form="NT"), dict(m=13, n=41, k=29, form="TN", beta=1),
                 dict(m=32, n=32, k=32, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, colbias=True), dict(m=24, n=40, k=34, a_type=DT.BF16, c_type=DT.F32, form="NN", beta=1)]


def test_sigmoid_sliced_segments_match_the_statement():
    api = capi.load()
    for i, kw in enumerate(SIGMOID_CASES):
        sg = SlicedFused(api, seed=300 + i, act=3, **kw)
        (got, gotm), (ref, _) = sg.run_checked(), sg.reference()
        tol = TOL_F32 if sg.case.c_type == DT.F32 else TOL_BF16
        for b in range(sg.nblocks):
            err = normf_rel(sg.valid(ref, b), sg.valid(got, b), sg.case.c_type)
            print(f"{kw} block {b}: normf_rel = {err}")
            assert err < tol, f"{kw} block {b}: normf_rel = {err}"
        sg.assert_outside_untouched(got, gotm, str(kw))


ONE_SLICE = [dict(m=32, n=32, k=32), dict(m=13, n=41, k=29, pads=(2, 3, 5), form="NT"), dict(m=36, n=20, k=18, form="TN"),
             dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A), dict(m=24, n=40, k=34, a_type=DT.BF16, c_type=DT.F32, form="NT", pads=(3, 3, 6))]


def test_one_slice_per_block_without_a_bias_is_bitwise_the_unsliced_ext_call():
    api = capi.load()
    products = [0, 3, 64, 1, 2, 7, 19]
    for i, kw in enumerate(ONE_SLICE):
        sg = SlicedFused(api, slices=[1] * len(products), products=products, beta=0, seed=350 + i, **kw)   # random values: the same chain, the same bits
        for act in (1, 2, 3):
            sg.set_epilogue(False, act)
            want = sg.new_out()
            sg.run_unsliced(want)
            api.hip_sync(); api.check()
            got, (wc, wm) = sg.run_checked(), sg.result(want)
            assert _same(got[0], wc) and _same(got[1], wm), f"{kw} act={act}: differs from the unsliced ext entry on the same lists"


def test_blocks_without_slices_are_the_unsliced_calls_segments_of_count_zero():
    api = capi.load()
    # (the ADDRESS form: the fixture's OFFSET lists want at least one product; the OFFSET forms' block without slices is block 0 of the parity tests)
    for i, kw in enumerate((dict(m=13, n=41, k=29, pads=(0, 0, 3)), dict(m=32, n=32, k=32), dict(m=16, n=16, k=16, a_type=DT.BF16, c_type=DT.BF16),
                            dict(m=5, n=60, k=7, a_type=DT.BF16, c_type=DT.BF16))):
        for beta in (0, 1):
            sg = SlicedFused(api, slices=[0] * 5, products=[], beta=beta, seed=380 + i, **kw)
            zeros = _up(np.zeros(sg.nblocks + 1, dtype=np.uint64))
            sg.d_la = sg.d_lb = zeros                                             # never read: no products; the unsliced entry wants its lists non-NULL
            for colbias, act in ((False, 0), (True, 0), (True, 1), (False, 2), (True, 2), (False, 3), (True, 3)):
                if not colbias and act == 0:
                    continue                                                      # no operators: the plain path, below
                sg.set_epilogue(colbias, act)
                want = sg.new_out()
                sg.run_unsliced(want, seg=zeros)
                api.hip_sync(); api.check()
                out = sg.new_out()
                api.hip_launch_count(1)
                sg.run(out)
                assert api.hip_launch_count(1) == 1                               # no slices: the first launch is skipped
                api.hip_sync(); api.check()
                got, (wc, wm) = sg.result(out), sg.result(want)
                assert _same(got[0], wc) and _same(got[1], wm), f"{kw} beta={beta} colbias={colbias} act={act}: differs from segments of count 0"


def test_an_ext_handle_without_operators_is_the_plain_sliced_call():
    api = capi.load()
    for i, (kw, name) in enumerate(((dict(m=13, n=41, k=29, beta=1, pads=(0, 0, 3)), b"gemm_segments_sliced_f32_kernel"),
                                    (dict(m=23, n=19, k=13, a_type=DT.F64, beta=1), b"gemm_segments_sliced_f64_kernel"),
                                    (dict(m=23, n=19, k=13, a_type=DT.F64, form="TN"), b"gemm_segments_offs_sliced_f64_kernel<1,0>"),
                                    (dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A), b"gemm_segments_sliced_bf16_kernel"),
                                    (dict(m=32, n=32, k=32, form="NT", beta=1), b"gemm_segments_offs_sliced_f32_kernel<0,1>"))):
        sg = SlicedFused(api, seed=400 + i, **kw)
        want = sg.new_out()
        sg.run_plain(want)
        api.hip_sync(); api.check()
        out = sg.new_out()
        api.hip_launch_count(1)
        sg.run(out)
        assert api.hip_launch_count(1) == 2
        api.hip_sync(); api.check()
        assert api.hip_kernel_name(sg.handle, 1) == name
        got, (wc, wm) = sg.result(out), sg.result(want)
        assert _same(got[0], wc), f"{kw}: differs from the plain sliced call"     # beta = 1: the block without slices stays untouched
        assert _same(got[1], sg.M0.host) and _same(wm, sg.M0.host)


def test_a_shared_bias_equals_a_list_of_equal_entries():
    api = capi.load()
    for i, kw in enumerate((dict(m=13, n=41, k=29, beta=1), dict(m=32, n=32, k=32, form="NT"), dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A))):
        sg = SlicedFused(api, seed=420 + i, colbias=True, act=2, **kw)
        one = int(sg.D.dev_ptrs(sg.dD, [1])[0])                                   # an odd element offset
        shared = sg.run_checked(shared_d=one)
        sg.di = np.ones(sg.nblocks, dtype=np.int64)
        listed = sg.run_checked()
        assert _same(shared[0], listed[0]) and _same(shared[1], listed[1]), f"{kw}: a NULL bias list differs from a list of equal entries"
        if sg.case.a_type == DT.F32:
            ref = sg.reference()
            assert _same(listed[0], ref[0]) and _same(listed[1], ref[1])


def test_two_calls_give_the_same_bits_on_another_stream_and_with_reuploaded_lists():
    import torch
    api = capi.load()
    for i, kw in enumerate((dict(m=13, n=41, k=29, form="NT", beta=1, pads=(0, 0, 7)), dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A))):
        sg = SlicedFused(api, seed=440 + i, colbias=True, act=2, **kw)
        first = sg.run_checked()
        side = torch.cuda.Stream()
        api.hip_set_stream(side.cuda_stream)
        out = sg.new_out()
        torch.cuda.synchronize()
        sg.run(out)
        api.hip_sync(); api.check()
        api.hip_set_stream(None); api.hip_set_async(0)
        again = sg.result(out)
        assert _same(again[0], first[0]) and _same(again[1], first[1]), f"{kw}: another stream"
        old = (sg.d_blk, sg.d_seg, sg.d_la, sg.d_lb)                              # kept alive: the new lists lie elsewhere
        sg.upload_lists()
        assert sg.d_la.data_ptr() != old[2].data_ptr()
        again = sg.run_checked()
        assert _same(again[0], first[0]) and _same(again[1], first[1]), f"{kw}: re-uploaded lists"


def test_a_call_is_two_launches_and_the_first_is_the_plain_sliced_kernel():
    api = capi.load()
    for kw, name in ((dict(m=32, n=32, k=32), b"gemm_segments_sliced_f32_kernel"),
                     (dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A), b"gemm_segments_sliced_bf16_kernel"),
                     (dict(m=13, n=41, k=29, form="TN"), b"gemm_segments_offs_sliced_f32_kernel<1,0>"),
                     (dict(m=32, n=32, k=32, a_type=DT.BF16, form="TT"), b"gemm_segments_offs_sliced_bf16_kernel<1,1>")):
        sg = SlicedFused(api, seed=460, colbias=True, act=2, **kw)
        out = sg.new_out()
        api.hip_launch_count(1)
        sg.run(out)
        assert api.hip_launch_count(1) == 2
        api.hip_sync(); api.check()
        assert api.hip_kernel_name(sg.handle, 1) == name
    api.hip_gemm_ext_batch_reduce_segments_sliced(sg.handle, C.byref(capi.GemmExtParam()), 0, None, 0, None, None, None, None, None, None, None, 0)
    assert api.hip_launch_count(1) == 0                                           # no blocks: nothing
    api.check()


def test_the_workspace_is_written_inside_the_queried_size_only():
    api = capi.load()
    for i, kw in enumerate((dict(m=13, n=41, k=29), dict(m=5, n=60, k=7, a_type=DT.BF16, c_type=DT.BF16, form="NN"))):
        sg = SlicedFused(api, seed=480 + i, colbias=True, act=2, **kw)
        ws = sg.new_ws(extra=64)                                                  # 64 bytes more than asked for, a pattern in all of it
        out = sg.new_out()
        sg.run(out, ws=ws)
        api.hip_sync(); api.check()
        if sg.case.a_type == DT.F32:
            got, ref = sg.result(out), sg.reference()
            assert _same(got[0], ref[0]) and _same(got[1], ref[1]), kw
        tail = _down(ws, np.zeros(1, dtype=np.uint8))[sg.ws_bytes:]
        assert tail.size == 64 and (tail == 0xA5).all(), f"{kw}: bytes beyond the queried size were written"
        out = sg.new_out()                                                        # one byte short: -2, nothing launched, C and the masks untouched
        api.hip_launch_count(1)
        sg.run(out, ws=ws, ws_bytes=sg.ws_bytes - 1)
        assert api.hip_get_last_error() == -2 and api.hip_launch_count(1) == 0
        api.hip_clear_last_error()
        got = sg.result(out)
        assert _same(got[0], sg.C0.host) and _same(got[1], sg.M0.host)


def _grid_stride(api, nblocks, m, n, beta, seed):
    """`nblocks` blocks of ONE slice of one m x n x 4 f32 product, on small integers, bias + ReLU + bitmask, every block against a numpy integer sum."""
    rng = np.random.default_rng(seed)
    npool, k, nb = 16, 4, 5
    ea, eb, ec = m * k, k * n, m * n
    mask_ld = (m + 15) // 16 * 16
    mb = mask_ld // 8 * n
    blk_ptr = np.arange(nblocks + 1, dtype=np.uint64)
    ai, bi, di = rng.integers(0, npool, nblocks), rng.integers(0, npool, nblocks), rng.integers(0, nb, nblocks)
    A, B, C0, D = _ints(rng, npool * ea, DT.F32), _ints(rng, npool * eb, DT.F32), _ints(rng, nblocks * ec, DT.F32), _ints(rng, nb * m, DT.F32)
    M0 = rng.integers(0, 256, nblocks * mb).astype(np.uint8)
    dA, dB, dC, dD, dM = _up(A), _up(B), _up(C0.copy()), _up(D), _up(M0.copy())
    seq = np.arange(nblocks, dtype=np.int64)
    lists = [_up((dA.data_ptr() + ai * ea * 4).astype(np.uint64)), _up((dB.data_ptr() + bi * eb * 4).astype(np.uint64)), _up((dC.data_ptr() + seq * (ec * 4)).astype(np.uint64)),
             _up((dD.data_ptr() + di * (m * 4)).astype(np.uint64)), _up((dM.data_ptr() + seq * mb).astype(np.uint64))]
    d_blk = _up(blk_ptr)
    h = GemmCase(m, n, k, beta=beta, br_type=capi.BR_ADDRESS, br_count=1, colbias=True, act=2).dispatch(api)
    assert h
    nbytes = api.hip_gemm_ext_batch_reduce_segments_sliced_workspace(h, nblocks)
    ws = _up(np.zeros(nbytes, dtype=np.uint8))
    api.hip_launch_count(1)
    api.hip_gemm_ext_batch_reduce_segments_sliced(h, C.byref(capi.GemmExtParam()), nblocks, d_blk.data_ptr(), nblocks, d_blk.data_ptr(), *[x.data_ptr() for x in lists],
                                                  ws.data_ptr(), nbytes)
    assert api.hip_launch_count(1) == 2
    api.hip_sync(); api.check()
    got, gotm = _down(dC, C0).reshape(nblocks, n, m), _down(dM, M0).reshape(nblocks, n, mask_ld // 8)
    Am, Bm = A.reshape(npool, k, m).astype(np.int32), B.reshape(npool, n, k).astype(np.int32)      # column-major blocks: as row-major arrays C^T = B^T A^T
    pair = np.einsum("bjk,aki->abji", Bm, Am).reshape(npool * npool, n, m)
    pre = pair[ai * npool + bi] + D.reshape(nb, m).astype(np.int32)[di][:, None, :]
    if beta:
        pre = pre + C0.reshape(nblocks, n, m).astype(np.int32)
    bad = np.flatnonzero((got.astype(np.float64) != np.maximum(pre, 0)).any(axis=(1, 2)))
    assert bad.size == 0, f"{bad.size} of {nblocks} blocks differ from the numpy sum, first: block {bad[0]}"
    assert not np.signbit(got).any()                                              # ReLU stores +0
    bits = np.unpackbits(M0.reshape(nblocks, n, mask_ld // 8), axis=2, bitorder="little")
    bits[:, :, :m] = pre > 0
    badm = np.flatnonzero((gotm != np.packbits(bits, axis=2, bitorder="little")).any(axis=(1, 2)))
    assert badm.size == 0, f"the masks of {badm.size} of {nblocks} blocks differ (bits of the sum's sign, every other bit as prefilled), first: block {badm[0]}"


def test_the_second_pass_grid_strides():
    """A 16 x 16 block is one run of pass 2 (and 12 x 16 one item of mask bytes), so its waves only grid-stride with more than 131 072 blocks."""
    api = capi.load()
    _grid_stride(api, 131073, 16, 16, 1, 500)
    _grid_stride(api, 131073, 12, 16, 0, 501)


def test_modes_stream_pipeline_and_coalescing_keep_the_results():
    import torch
    api = capi.load()
    segs = [SlicedFused(api, seed=600 + i, **kw) for i, kw in enumerate((dict(m=32, n=32, k=32, form="NT", beta=1, colbias=True, act=2), dict(m=13, n=41, k=29, colbias=True, act=2),
                                                                         dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, form="TN", colbias=True, act=1)))]
    want = [sg.run_checked() for sg in segs]                                      # blocking
    same = lambda sg, out, w: all(_same(x, y) for x, y in zip(sg.result(out), w))
    workspaces = [sg.new_ws() for sg in segs]                                     # one per call in flight
    # stream-ordered on a torch stream
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    outs = [sg.new_out() for sg in segs]
    for sg, out, ws in zip(segs, outs, workspaces):
        sg.run(out, ws=ws)
    api.hip_sync(); api.check()
    assert all(same(sg, out, w) for sg, out, w in zip(segs, outs, want)), "stream-ordered"
    # inside a pipeline section: both launches of a call go to one lane
    outs = [sg.new_out() for sg in segs]
    assert api.hip_pipeline_begin(4) == 0
    for sg, out, ws in zip(segs, outs, workspaces):
        sg.run(out, ws=ws)
    assert api.hip_pipeline_end() == 0
    api.hip_sync(); api.check()
    assert all(same(sg, out, w) for sg, out, w in zip(segs, outs, want)), "pipeline section"
    # coalescing: a queued single call writes the block that every product of the sliced call reads as A; the queue is flushed first
    m = 32
    rng = np.random.default_rng(620)
    X, Y = (torch.from_numpy(_ints(rng, m * m, DT.F32)).to("cuda:0") for _ in range(2))
    Bs = torch.from_numpy(_ints(rng, 3 * m * m, DT.F32)).to("cuda:0")
    T = torch.zeros(m * m, dtype=torch.float32, device="cuda:0")
    out = torch.zeros(2 * m * m, dtype=torch.float32, device="cuda:0")
    plain = GemmCase(m, m, m, seed=621).dispatch(api)
    adr = GemmCase(m, m, m, br_type=capi.BR_ADDRESS, br_count=1, act=1, seed=622).dispatch(api)
    blk_ptr = torch.tensor([0, 1, 3], dtype=torch.int64, device="cuda:0")         # block 0: one slice; block 1: two slices of one product
    seg_ptr = torch.tensor([0, 1, 2, 3], dtype=torch.int64, device="cuda:0")
    la = torch.tensor([T.data_ptr()] * 3, dtype=torch.int64, device="cuda:0")
    lb = torch.tensor([Bs.data_ptr() + i * m * m * 4 for i in range(3)], dtype=torch.int64, device="cuda:0")
    lc = torch.tensor([out.data_ptr(), out.data_ptr() + m * m * 4], dtype=torch.int64, device="cuda:0")
    nbytes = api.hip_gemm_ext_batch_reduce_segments_sliced_workspace(adr, 3)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    api.hip_set_async(2)
    p = capi.GemmParam(); p.a.primary, p.b.primary, p.c.primary = X.data_ptr(), Y.data_ptr(), T.data_ptr()
    capi.Api.call(plain, p)                                                       # queued, nothing launched yet
    api.hip_gemm_ext_batch_reduce_segments_sliced(adr, C.byref(capi.GemmExtParam()), 2, blk_ptr.data_ptr(), 3, seg_ptr.data_ptr(), la.data_ptr(), lb.data_ptr(), lc.data_ptr(),
                                                  None, None, ws.data_ptr(), nbytes)
    api.hip_sync(); api.check()
    api.hip_set_async(0); api.hip_set_stream(None)
    col = lambda t: t.cpu().numpy().astype(np.float64).reshape(m, m).T            # column-major block -> matrix
    Tm = col(X) @ col(Y)
    Bm = [col(Bs[i * m * m:(i + 1) * m * m]) for i in range(3)]
    got = out.cpu().numpy().astype(np.float64).reshape(2, m, m)
    assert np.array_equal(got[0].T, np.maximum(Tm @ Bm[0], 0)) and np.array_equal(got[1].T, np.maximum(Tm @ Bm[1] + Tm @ Bm[2], 0))


def test_a_captured_call_replays_on_new_operand_values():
    """One call captured on one stream (two kernel nodes in order); A is overwritten in place, the graph is replayed once and compared with a fresh call."""
    import torch
    api = capi.load()
    sg = SlicedFused(api, m=13, n=41, k=29, form="NT", seed=700, colbias=True, act=2)
    new = SlicedFused(api, m=13, n=41, k=29, form="NT", seed=701, colbias=True, act=2)       # same pattern and layout, other values
    out, ws = sg.new_out(), sg.new_ws()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        api.hip_set_stream(side.cuda_stream)
        api.hip_launch_count(1)
        g.capture_begin()
        sg.run(out, ws=ws)
        g.capture_end()
        assert api.hip_launch_count(0) == 2
    api.check()
    torch.cuda.current_stream().wait_stream(side)
    api.hip_set_stream(None); api.hip_set_async(0)
    for d, h in zip(sg.dA, new.A.host):                                           # A in place; B, C, the bias and the masks keep their values
        d.copy_(torch.from_numpy(h))
    torch.cuda.synchronize()
    g.replay(); torch.cuda.synchronize()
    got = sg.result(out)
    sg.A = new.A
    fresh, ref = sg.run_checked(), sg.reference()
    assert _same(got[0], fresh[0]) and _same(got[1], fresh[1]), "the replay differs from a fresh call on the new A"
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])


def test_c_example_runs_a_convolution_with_bias_relu_and_bitmask_in_one_sliced_call_per_image(tmp_path):
    libdir = os.path.join(ROOT, "libxsmm_amd", "lib")
    exe = str(tmp_path / "segments_sliced_fused_driver")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "segments_sliced_fused_driver.c"),
           "-L" + libdir, "-lxsmm_amd", "-lm", "-Wl,-rpath," + libdir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "normf_rel" in r.stdout and "2 launches" in r.stdout


GUARDED = "test_f32_sliced_fused_segments_are_bitwise or test_bf16_sliced_fused_segments or test_the_second_pass_grid_strides"


def test_guarded_rerun_with_operands_flush_against_unmapped_memory():
    """The bitwise and grid-stride tests again with every upload flush against unmapped address space (tests/guard.py via tests/conftest.py): the pools, the last
    A, B, C, bias and mask block (arrays of their own), the seven lists and the workspace, which is exactly as large as the query says.  These are parity tests on
    valid inputs: an access outside an operand would fault the subprocess.  Why none is expected: pass 1 is the plain sliced kernels'; in pass 2 a lane's 16-byte
    load starts at an element below m * n of a partial that is padded to 16 bytes, a mask-byte unit loads its valid rows only, the bias is read at rows < m (as one
    vector only where m % 4 == 0), and C and the masks are read and written at i < m, j < n only.  The second side only runs once the first has passed."""
    for side in ("end", "front"):
        env = dict(os.environ, LIBXSMM_TEST_GUARD=side)
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "-k", GUARDED, "-v", "--no-header"]
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
        print(f"guarded run ({side}): {time.time() - t0:.1f} s")
        assert r.returncode == 0, f"guarded run ({side}) ended with {r.returncode} (negative / 134: the GPU faulted on an out-of-bounds access):\n{tail}"
        assert "8 passed" in r.stdout, tail
