"""libxsmm_hip_gemm_ext_batch_reduce_segments_offsets (include/libxsmm_hip.h): OFFSET segments through an ext handle -- five bases, signed byte offsets, A and / or
B transposed, column bias, ReLU (+ bitmask) or sigmoid fused into the one launch.  f32 segments are bitwise the oracle's (product, k)-ordered fmaf chain started at
the bias in all four forms, mask bits included, with every byte outside the m x n blocks and every mask bit beyond them left alone; bf16 segments are bitwise the
ext oracle on exact data and within the dense kernels' tolerances on random data; NN equals the ADDRESS fused entry bit for bit and the call equals its loop of
single ext OFFSET calls; a shared bias, the launch modes, capture and 140 000 segments keep the results.  The bases point into the middle of their buffers, so
offsets of both signs occur.  The last test re-runs the parity tests with every operand, bias and mask block flush against unmapped memory (run this file with -x)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import helpers
from helpers import GemmCase, TOL_BF16, TOL_F32, as_float, normf_rel
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG
from oracle import pyoracle
from test_gemm_segments_fused_gpu import EPILOGUES, NBIAS, FusedSegments, decided_mask_bits
from test_gemm_segments_gpu import COUNTS, Pool, _down, _ints, _same, _up
from test_gemm_segments_offsets_gpu import BF16_FORMS, BF16_SHAPES, FORMS, TA, TB, OffsetSegments, _offs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

assert COUNTS == [0, 3, 64, 1, 0, 2, 7, 19, 1, 0]


class FusedOffsetSegments(OffsetSegments):
    """An offsets call with an epilogue: OffsetSegments' pools and lists, FusedSegments' pool of bias vectors that the segments share (d_offs repeats its entries)
    and one mask block per segment, prefilled with random bytes.  Every base is the address of a block in the MIDDLE of its pool's main array: the blocks in
    front of it have negative offsets, and the pool's last block, an allocation of its own, lies wherever the allocator put it."""
    bias_of, mask_rows, mask_bits, assert_outside_untouched = (FusedSegments.bias_of, FusedSegments.mask_rows, FusedSegments.mask_bits,
                                                               FusedSegments.assert_outside_untouched)

    def __init__(self, api, m, n, k, colbias=False, act=0, **kw):
        exact, seed = kw.get("exact", False), kw.get("seed", 0)
        super().__init__(api, m, n, k, **kw)
        case = self.case
        rng = np.random.default_rng(5000 + seed)
        gen = _ints if exact else helpers.rand_values
        self.D = Pool(gen(rng, Pool.size(NBIAS, m), case.c_type), NBIAS, m)
        self.di = (np.arange(self.nseg) * 3) % NBIAS                              # 0, 3, 2, 1, 0, ...: repeated entries, the last block among them
        self.M0 = Pool(rng.integers(0, 256, Pool.size(self.nseg, case.mask_bytes)).astype(np.uint8), self.nseg, case.mask_bytes)
        self.dD = self.D.upload()
        mid = lambda pool, dev: int(pool.dev_ptrs(dev, [(pool.nblocks - 1) // 2])[0])
        self.mid = mid
        self.base_a, self.base_b, self.base_d = mid(self.A, self.dA), mid(self.B, self.dB), mid(self.D, self.dD)
        self.oa, self.ob = _offs(self.A.dev_ptrs(self.dA, self.ai), self.base_a), _offs(self.B.dev_ptrs(self.dB, self.bi), self.base_b)
        self.od = _offs(self.D.dev_ptrs(self.dD, self.di), self.base_d)
        assert (self.oa < 0).any() and (self.oa > 0).any() and (self.ob < 0).any() and (self.od < 0).any()
        self.d_oa, self.d_ob, self.d_od = _up(self.oa), _up(self.ob), _up(self.od)
        self.kw = dict(m=m, n=n, k=k, a_type=case.a_type, c_type=case.c_type, lda=case.lda, ldb=case.ldb, ldc=case.ldc, flags=case.flags & ~GEMM_FLAG.BETA_0)
        self.beta = 0 if case.flags & GEMM_FLAG.BETA_0 else 1
        self.set_epilogue(colbias, act)

    def set_epilogue(self, colbias, act):
        self.colbias, self.act = colbias, act
        self.ext = GemmCase(beta=self.beta, colbias=colbias, act=act, br_type=capi.BR_OFFSET, br_count=1, **self.kw)     # (descriptor only)
        self.ext_handle = self.api.dispatch_brgemm_ext(self.ext.shape(), self.ext.flags, 0, self.ext.brcfg(), self.ext.argops(), self.ext.postops())
        assert self.ext_handle
        return self

    # ---- device ---------------------------------------------------------------------------------------------------------------------------------
    def new_out(self):
        dC, dM = self.C0.upload(), self.M0.upload()
        bc, bm = self.mid(self.C0, dC), self.mid(self.M0, dM)
        oc, om = _offs(self.C0.dev_ptrs(dC, range(self.nseg)), bc), _offs(self.M0.dev_ptrs(dM, range(self.nseg)), bm)
        assert (oc < 0).any() and (om < 0).any()
        return dict(C=dC, M=dM, base_c=bc, base_m=bm, oc=oc, om=om, d_oc=_up(oc), d_om=_up(om))

    def param(self, out, shared_d=None):
        p = capi.GemmExtParam()
        p.a.primary, p.b.primary, p.c.primary = self.base_a, self.base_b, out["base_c"]
        if self.colbias:
            p.d.primary = self.base_d if shared_d is None else shared_d
        if self.act == 2:
            p.c.secondary = out["base_m"]
        return p

    def run(self, out, shared_d=None):
        """shared_d: a device address -- d_offs = NULL and param->d.primary is the one bias of every segment."""
        od = self.d_od.data_ptr() if self.colbias and shared_d is None else None
        self.api.hip_gemm_ext_batch_reduce_segments_offsets(self.ext_handle, C.byref(self.param(out, shared_d)), self.nseg, self.d_seg.data_ptr(), self.d_oa.data_ptr(),
                                                            self.d_ob.data_ptr(), out["d_oc"].data_ptr(), od, out["d_om"].data_ptr() if self.act == 2 else None)

    def result(self, out):
        return self.C0.download(out["C"]), self.M0.download(out["M"])

    def run_checked(self, **kw):
        out = self.new_out()
        self.run(out, **kw)
        self.api.hip_sync(); self.api.check()
        return self.result(out)

    def run_loop(self):
        """The loop the call replaces: one blocking fused OFFSET call per segment.  None when the single-call path does not take the handle."""
        out = self.new_out()
        for s in range(self.nseg):
            p = self.param(out)
            cnt = C.c_ulonglong(int(self.counts[s]))
            p.a.secondary = self.d_oa.data_ptr() + int(self.seg_ptr[s]) * 8
            p.b.secondary = self.d_ob.data_ptr() + int(self.seg_ptr[s]) * 8
            p.c.primary = out["base_c"] + int(out["oc"][s]); p.op.tertiary = C.addressof(cnt)
            if self.colbias:
                p.d.primary = self.base_d + int(self.od[s])
            if self.act == 2:
                p.c.secondary = out["base_m"] + int(out["om"][s])
            capi.Api.call(self.ext_handle, p)
            if s == 0 and self.api.hip_get_last_error() != 0:
                self.api.hip_clear_last_error()
                return None
        self.api.hip_sync(); self.api.check()
        return self.result(out)

    def run_address(self):
        """The same blocks through the ADDRESS fused entry: pointer lists = base + offset (NN only)."""
        adr = GemmCase(beta=self.beta, colbias=self.colbias, act=self.act, br_type=capi.BR_ADDRESS, br_count=1, **self.kw).dispatch(self.api)
        assert adr
        out = self.new_out()
        ptrs = lambda offs, base: _up((offs + np.int64(base)).view(np.uint64))
        lists = [ptrs(self.oa, self.base_a), ptrs(self.ob, self.base_b), ptrs(out["oc"], out["base_c"]), ptrs(self.od, self.base_d), ptrs(out["om"], out["base_m"])]
        p = capi.GemmExtParam()
        self.api.hip_gemm_ext_batch_reduce_segments(adr, C.byref(p), self.nseg, self.d_seg.data_ptr(), lists[0].data_ptr(), lists[1].data_ptr(), lists[2].data_ptr(),
                                                    lists[3].data_ptr() if self.colbias else None, lists[4].data_ptr() if self.act == 2 else None)
        self.api.hip_sync(); self.api.check()
        return self.result(out)

    # ---- host ------------------------------------------------------------------------------------------------------------------------------------
    def _host_calls(self, ref, ext):
        """One host param per segment over the host pools (offsets from the pools' main arrays)."""
        oa = _offs(self.A.host_ptrs(self.ai), self.A.host[0].ctypes.data)
        ob = _offs(self.B.host_ptrs(self.bi), self.B.host[0].ctypes.data)
        lc = ref.host_ptrs(range(self.nseg))
        for s in range(self.nseg):
            p = capi.GemmExtParam() if ext else capi.GemmParam()
            cnt = C.c_ulonglong(int(self.counts[s]))
            p.a.primary, p.b.primary = self.A.host[0].ctypes.data, self.B.host[0].ctypes.data
            p.a.secondary = oa.ctypes.data + int(self.seg_ptr[s]) * 8
            p.b.secondary = ob.ctypes.data + int(self.seg_ptr[s]) * 8
            p.c.primary = int(lc[s]); p.op.tertiary = C.addressof(cnt)
            yield s, p, (oa, ob, cnt)

    def oracle_ext(self):
        """(C arrays, mask arrays) of the ext oracle called once per segment -- the reference's fused OFFSET call [oracle/oracle_gemm.c]."""
        orc, d = pyoracle.oracle(), self.ext.oracle_desc()
        ref, msk = self.C0.copy(), self.M0.copy()
        ld, lm = self.D.host_ptrs(self.di), msk.host_ptrs(range(self.nseg))
        for s, p, keep in self._host_calls(ref, True):
            if self.colbias:
                p.d.primary = int(ld[s])
            if self.act == 2:
                p.c.secondary = int(lm[s])
            orc.gemm(p, d)
        return ref.host, msk.host

    def fma_chain(self):
        """f32: FusedSegments.fma_chain's composition over the offset lists -- bias (+ C0, one f32 add) written into a copy of C, the (product, k)-ordered fmaf
        chain with beta = 1 on the non-ext descriptor on top of it, the mask bits !(x <= 0) set into a copy of the prefilled masks, then ReLU."""
        orc = pyoracle.oracle()
        d = GemmCase(beta=1, br_type=capi.BR_OFFSET, br_count=1, **self.kw).oracle_desc()
        ref, msk = self.C0.copy(), self.M0.copy()
        for s in range(self.nseg):
            v = self.valid(ref.host, s)
            start = v.copy() if self.beta else np.zeros_like(v)
            if self.colbias:
                start = (self.bias_of(s)[None, :] + start) if self.beta else np.broadcast_to(self.bias_of(s)[None, :], v.shape)
            v[...] = start
        for s, p, keep in self._host_calls(ref, False):
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
        """Per segment: (pre-activation sum, sum of magnitudes, terms) in float64 as [n][m] -- FusedSegments.pre64 with the transposed layouts."""
        c = self.case
        ta, tb = bool(c.flags & TA), bool(c.flags & TB)
        out = []
        for s in range(self.nseg):
            pre, mag, terms = np.zeros((c.n, c.m)), np.zeros((c.n, c.m)), int(self.counts[s]) * c.k
            for r in range(int(self.seg_ptr[s]), int(self.seg_ptr[s + 1])):
                a = as_float(self.A.block(self.A.host, int(self.ai[r])), c.a_type)
                b = as_float(self.B.block(self.B.host, int(self.bi[r])), c.a_type)
                if ta:                                                             # [m][lda] -> [k][m]
                    am = a[:c.m * c.lda].reshape(c.m, c.lda)[:, :c.k].T
                elif c.flags & GEMM_FLAG.VNNI_A:                                   # [k / 2][lda][2] -> [k][lda]
                    kp = (c.k + 1) // 2
                    am = a[:kp * c.lda * 2].reshape(kp, c.lda, 2).transpose(0, 2, 1).reshape(2 * kp, c.lda)[:c.k, :c.m]
                else:
                    am = a[:c.k * c.lda].reshape(c.k, c.lda)[:, :c.m]
                bm = b[:c.k * c.ldb].reshape(c.k, c.ldb)[:, :c.n].T if tb else b[:c.n * c.ldb].reshape(c.n, c.ldb)[:, :c.k]     # [n][k]
                pre += bm @ am; mag += np.abs(bm) @ np.abs(am)
            if self.beta:
                c0 = as_float(self.valid(self.C0.host, s), c.c_type)
                pre, mag, terms = pre + c0, mag + np.abs(c0), terms + 1
            if self.colbias:
                bias = as_float(self.bias_of(s), c.c_type)[None, :]
                pre, mag, terms = pre + bias, mag + np.abs(bias), terms + 1
            out.append((pre, mag, terms))
        return out


F32_SHAPES = [dict(m=32, n=32, k=32), dict(m=16, n=16, k=16), dict(m=13, n=17, k=29), dict(m=13, n=13, k=13), dict(m=20, n=24, k=18, pads=(3, 3, 9)), dict(m=40, n=40, k=40)]


@pytest.mark.parametrize("form", list(FORMS))
def test_f32_fused_offset_segments_are_bitwise_the_fma_chain_mask_included(form):
    api = capi.load()
    for i, kw in enumerate(F32_SHAPES):
        for beta in (0, 1):
            sg = FusedOffsetSegments(api, form=form, beta=beta, seed=10 * i + beta, **kw)
            for colbias, act in EPILOGUES:                                        # bias, bias + ReLU, ReLU + bitmask, bias + ReLU + bitmask
                what = f"{form} {kw} beta={beta} colbias={colbias} act={act}"
                sg.set_epilogue(colbias, act)
                (got, gotm), (ref, refm) = sg.run_checked(), sg.fma_chain()
                # whole arrays: the m x n blocks and their mask bits are the chain's, every other byte and bit (padding, gaps, bits beyond m) is the caller's
                assert _same(got, ref), f"{what}: C differs from the fmaf chain started at the bias (or bytes outside m x n changed)"
                assert _same(gotm, refm), f"{what}: the mask differs from !(x <= 0) of the chain (or bits outside m x n changed)"
                orc, _ = sg.oracle_ext()
                for s in range(sg.nseg):
                    err = normf_rel(sg.valid(orc, s), sg.valid(ref, s), DT.F32)
                    assert err < TOL_F32, f"{what} segment {s}: the expected value is {err} from the ext oracle"


@pytest.mark.parametrize("name", list(BF16_FORMS))
def test_bf16_fused_offset_segments_match_the_ext_oracle(name):
    api = capi.load()
    flags, form = BF16_FORMS[name]
    for i, kw in enumerate(BF16_SHAPES):
        if flags & GEMM_FLAG.VNNI_A and kw["k"] % 2:
            continue                                                              # VNNI-2 pairs k: no handle exists for an odd k
        for c_type in (DT.BF16, DT.F32):
            what = f"{name} {kw} -> {c_type}"
            ex = FusedOffsetSegments(api, form=form, a_type=DT.BF16, c_type=c_type, flags=flags, seed=250 + i, exact=True, colbias=True, act=2, **kw)
            (got, gotm), (ref, refm) = ex.run_checked(), ex.oracle_ext()
            assert _same(got, ref) and _same(gotm, refm), f"{what}: exact data differs from the ext oracle (C {_same(got, ref)}, mask {_same(gotm, refm)})"
            sg = FusedOffsetSegments(api, form=form, a_type=DT.BF16, c_type=c_type, flags=flags, seed=200 + i, colbias=True, act=2, **kw)
            (got, gotm), (ref, refm) = sg.run_checked(), sg.oracle_ext()
            tol = TOL_F32 if c_type == DT.F32 else TOL_BF16
            for s in range(sg.nseg):
                err = normf_rel(sg.valid(ref, s), sg.valid(got, s), c_type)
                assert err < tol, f"{what} segment {s} (count {sg.counts[s]}): normf_rel = {err}"
            sg.assert_outside_untouched(got, gotm, what)
            dec = decided_mask_bits(sg)
            share = np.mean(np.concatenate([d.ravel() for d, _ in dec.values()]))
            assert share > 0.5, f"{what}: only {share:.2f} of the mask bits are decided"
            for s in range(sg.nseg):
                bits = sg.mask_bits(gotm, s)
                if s in dec:
                    d, pos = dec[s]
                    assert np.array_equal(bits[d], pos[d].astype(bits.dtype)), f"{what} segment {s}: {np.count_nonzero(bits[d] != pos[d])} decided mask bits differ"
                else:                                                             # count 0: the mask of the start value, exactly
                    assert np.array_equal(bits, sg.mask_bits(refm, s)), f"{what}: empty segment {s}: mask differs from the ext oracle"


SIGMOID_CASES = [dict(m=20, n=12, k=16, beta=1, form="TN"), dict(m=32, n=32, k=32, form="NT"),
                 dict(m=32, n=32, k=32, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A), dict(m=24, n=40, k=34, a_type=DT.BF16, c_type=DT.F32, form="TT", pads=(3, 3, 6), beta=1)]


def test_sigmoid_offset_segments_match_the_ext_oracle():
    api = capi.load()
    for kw in SIGMOID_CASES:
        sg = FusedOffsetSegments(api, seed=300, act=3, **kw)
        (got, gotm), (ref, _) = sg.run_checked(), sg.oracle_ext()
        tol = TOL_F32 if sg.case.c_type == DT.F32 else TOL_BF16
        for s in range(sg.nseg):
            err = normf_rel(sg.valid(ref, s), sg.valid(got, s), sg.case.c_type)
            assert err < tol, f"{kw} segment {s} (count {sg.counts[s]}): normf_rel = {err}"
        sg.assert_outside_untouched(got, gotm, str(kw))


NN_CASES = [dict(m=32, n=32, k=32, colbias=True, act=2), dict(m=13, n=17, k=29, beta=1, colbias=True, act=2), dict(m=20, n=24, k=18, pads=(3, 3, 9), colbias=True, act=1),
            dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, colbias=True, act=2),
            dict(m=24, n=40, k=34, a_type=DT.BF16, c_type=DT.F32, pads=(3, 3, 6), beta=1, colbias=True, act=2), dict(m=32, n=32, k=32, a_type=DT.BF16, c_type=DT.BF16, act=3)]


def test_nn_equals_the_address_fused_entry_bit_for_bit():
    api = capi.load()
    for i, kw in enumerate(NN_CASES):
        sg = FusedOffsetSegments(api, seed=380 + i, **kw)                         # random data: the same blocks, the same chain, the same bits
        one, adr = sg.run_checked(), sg.run_address()
        assert _same(one[0], adr[0]) and _same(one[1], adr[1]), f"{kw}: differs from libxsmm_hip_gemm_ext_batch_reduce_segments on base + offset"


LOOP_CASES = [dict(m=13, n=17, k=29, beta=1, colbias=True, act=2), dict(m=32, n=32, k=32, form="TN", colbias=True, act=2), dict(m=20, n=24, k=18, pads=(3, 3, 9), form="NT", colbias=True, act=1),
              dict(m=13, n=13, k=13, form="TT", beta=1, colbias=True, act=2), dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, colbias=True, act=1),
              dict(m=24, n=40, k=34, a_type=DT.BF16, c_type=DT.F32, beta=1, form="TN", colbias=True, act=2), dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, form="NT", act=2)]


def test_the_fused_call_equals_its_loop_of_single_ext_offset_calls():
    api = capi.load()
    taken = []
    for i, kw in enumerate(LOOP_CASES):
        sg = FusedOffsetSegments(api, seed=400 + i, exact=True, **kw)
        one, loop = sg.run_checked(), sg.run_loop()
        if loop is None:                                                          # a form the single-call path does not take has no loop to compare with
            print(f"single-call path refuses {kw}")
            continue
        taken.append(kw.get("form", "NN"))
        assert _same(one[0], loop[0]) and _same(one[1], loop[1]), f"{kw}: differs from the loop of fused single OFFSET calls through the same handle"
    assert taken.count("NN") == 2, taken


def test_a_shared_bias_equals_offsets_of_equal_entries_and_entries_may_repeat():
    api = capi.load()
    for kw in (dict(m=13, n=17, k=29, beta=1, form="TN"), dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A)):
        sg = FusedOffsetSegments(api, seed=350, colbias=True, act=2, **kw)
        assert len(set(sg.od.tolist())) < sg.nseg                                 # (the default d_offs repeats its entries: the parity tests cover that)
        one = int(sg.D.dev_ptrs(sg.dD, [1])[0])                                   # an odd element offset
        shared = sg.run_checked(shared_d=one)
        sg.di = np.ones(sg.nseg, dtype=np.int64)
        sg.od = _offs(sg.D.dev_ptrs(sg.dD, sg.di), sg.base_d)
        sg.d_od = _up(sg.od)
        listed = sg.run_checked()
        assert _same(shared[0], listed[0]) and _same(shared[1], listed[1]), f"{kw}: d_offs = NULL differs from a d_offs of equal entries"
        if sg.case.a_type == DT.F32:
            ref = sg.fma_chain()
            assert _same(listed[0], ref[0]) and _same(listed[1], ref[1])


def test_f64_runs_the_plain_offsets_kernels_without_operators_and_is_refused_with_them():
    """(f64 with operators is refused where every fused f64 call is: libxsmm_dispatch_brgemm_ext returns no handle, so no entry ever sees one.)"""
    api = capi.load()
    for form, name in (("TN", b"gemm_segments_offs_f64_kernel<1,0>"), ("NT", b"gemm_segments_offs_f64_kernel<0,1>")):
        sg = OffsetSegments(api, m=23, n=23, k=23, form=form, a_type=DT.F64, beta=1, seed=450)
        case = sg.case
        free = api.dispatch_brgemm_ext(case.shape(), case.flags, 0, case.brcfg(), capi.no_argops(), capi.no_postops())
        relu = api.dispatch_brgemm_ext(case.shape(), case.flags, 0, case.brcfg(), capi.argops_cp(case.ldc, capi.UNARY.RELU), capi.no_postops())
        assert free and not relu
        want = sg.run_checked()
        cset = sg.new_c()
        p = capi.GemmExtParam()
        p.a.primary, p.b.primary, p.c.primary = sg.dA[0].data_ptr(), sg.dB[0].data_ptr(), cset[0][0].data_ptr()
        args = (C.byref(p), sg.nseg, sg.d_seg.data_ptr(), sg.d_oa.data_ptr(), sg.d_ob.data_ptr(), cset[1].data_ptr(), None, None)
        api.hip_launch_count(1)
        api.hip_gemm_ext_batch_reduce_segments_offsets(None, *args)             # what such a caller holds: refused, nothing launched, C untouched
        assert api.hip_get_last_error() == -3 and api.hip_launch_count(0) == 0
        api.hip_clear_last_error()
        assert _same(sg.C0.download(cset[0]), sg.C0.host), "a refused call wrote C"
        api.hip_gemm_ext_batch_reduce_segments_offsets(free, *args)
        assert api.hip_launch_count(1) == 1
        api.hip_sync(); api.check()
        assert api.hip_kernel_name(free, 1) == name
        assert _same(sg.C0.download(cset[0]), want), f"{form}: differs from the plain offsets call"


def test_one_launch_per_call_through_the_named_instances():
    api = capi.load()
    for kw, name in ((dict(m=32, n=32, k=32, form="TN", colbias=True, act=2), b"gemm_segments_offs_f32_fused_kernel<1,0>"),
                     (dict(m=13, n=17, k=29, form="TT", act=1), b"gemm_segments_offs_f32_fused_kernel<1,1>"),
                     (dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, colbias=True, act=1), b"gemm_segments_offs_bf16_fused_kernel<0,0>"),
                     (dict(m=32, n=32, k=32, a_type=DT.BF16, c_type=DT.F32, form="NT", act=3), b"gemm_segments_offs_bf16_fused_kernel<0,1>"),
                     (dict(m=32, n=32, k=32, form="NT"), b"gemm_segments_offs_f32_kernel<0,1>")):       # an ext handle without operators
        sg = FusedOffsetSegments(api, seed=460, **kw)
        out = sg.new_out()
        api.hip_launch_count(1)
        sg.run(out)
        assert api.hip_launch_count(1) == 1
        api.hip_sync(); api.check()
        assert api.hip_kernel_name(sg.ext_handle, 1) == name
        if not (sg.colbias or sg.act):                                            # ... is the plain product; no mask byte is touched
            got = sg.result(out)
            assert _same(got[0], OffsetSegments.oracle(sg, fma=True)) and _same(got[1], sg.M0.host)


def _scale_fused(api, nseg, edge, form, beta, seed):
    """`nseg` f32 segments of edge^3 with skewed counts (1 %: 64, a few empty, the rest 1) on exact data, bias + ReLU + bitmask, against a numpy sum; the bases
    lie in the middle of the operands."""
    rng = np.random.default_rng(seed)
    npool, e2, nb = 16, edge * edge, 5
    mask_ld = (edge + 15) // 16 * 16
    mb = mask_ld // 8 * edge
    counts = np.where(rng.random(nseg) < 0.01, 64, 1).astype(np.uint64)
    counts[::997] = 0
    seg_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    total = int(seg_ptr[-1])
    ai, bi, di = rng.integers(0, npool, total), rng.integers(0, npool, total), rng.integers(0, nb, nseg)
    A, B, C0, D = _ints(rng, npool * e2, DT.F32), _ints(rng, npool * e2, DT.F32), _ints(rng, nseg * e2, DT.F32), _ints(rng, nb * edge, DT.F32)
    M0 = rng.integers(0, 256, nseg * mb).astype(np.uint8)
    dA, dB, dC, dD, dM = _up(A), _up(B), _up(C0.copy()), _up(D), _up(M0.copy())
    seq = np.arange(nseg, dtype=np.int64)
    ha, hs, hd = npool // 2, nseg // 2, nb // 2                                   # the block every base points at
    lists = [_up(seg_ptr), _up(((ai - ha) * e2 * 4).astype(np.int64)), _up(((bi - ha) * e2 * 4).astype(np.int64)), _up((seq - hs) * (e2 * 4)),
             _up(((di - hd) * edge * 4).astype(np.int64)), _up((seq - hs) * mb)]
    case = GemmCase(edge, edge, edge, flags=FORMS[form], beta=beta, br_type=capi.BR_OFFSET, br_count=1, colbias=True, act=2)
    h = case.dispatch(api)
    assert h
    p = capi.GemmExtParam()
    p.a.primary, p.b.primary, p.c.primary = dA.data_ptr() + ha * e2 * 4, dB.data_ptr() + ha * e2 * 4, dC.data_ptr() + hs * e2 * 4
    p.d.primary, p.c.secondary = dD.data_ptr() + hd * edge * 4, dM.data_ptr() + hs * mb
    api.hip_launch_count(1)
    api.hip_gemm_ext_batch_reduce_segments_offsets(h, C.byref(p), nseg, *[x.data_ptr() for x in lists])
    assert api.hip_launch_count(1) == 1
    api.hip_sync(); api.check()
    got, gotm = _down(dC, C0).reshape(nseg, edge, edge), _down(dM, M0).reshape(nseg, edge, mask_ld // 8)
    # blocks in memory order: flat A is [k][i], TRANS_A [i][k]; flat B is [j][k], TRANS_B [k][j]; C is [j][i] (test_gemm_segments_offsets_gpu._scale)
    Am, Bm = A.reshape(npool, edge, edge).astype(np.int32), B.reshape(npool, edge, edge).astype(np.int32)
    sub = ("bkj" if FORMS[form] & TB else "bjk") + "," + ("aik" if FORMS[form] & TA else "aki") + "->abji"
    pair = np.einsum(sub, Bm, Am).reshape(npool * npool, e2)
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


def test_scale_fused_offset_segments_past_one_wave_per_item():
    api = capi.load()
    _scale_fused(api, 40000, 16, "TN", 0, 600)        # more than 32 768 work items
    _scale_fused(api, 140000, 8, "NT", 1, 601)        # more items than one wave each (4 x 32 768): the waves grid-stride


MODE_CASES = [dict(m=32, n=32, k=32, form="TN", colbias=True, act=2), dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, form="NT", flags=GEMM_FLAG.VNNI_A, colbias=True, act=1)]


def test_modes_stream_pipeline_and_coalescing_keep_the_results():
    import torch
    api = capi.load()
    segs = [FusedOffsetSegments(api, seed=500 + i, **kw) for i, kw in enumerate(MODE_CASES)]
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
    # coalescing: a queued single call writes the block that every product of the fused offsets call reads as (transposed) A; the queue is flushed first
    m = 32
    rng = np.random.default_rng(620)
    X, Y = (torch.from_numpy(_ints(rng, m * m, DT.F32)).to("cuda:0") for _ in range(2))
    Bs = torch.from_numpy(_ints(rng, 3 * m * m, DT.F32)).to("cuda:0")
    bias = torch.from_numpy(rng.integers(-40, 41, 2 * m).astype(np.float32)).to("cuda:0")
    T = torch.zeros(m * m, dtype=torch.float32, device="cuda:0")
    out = torch.zeros(2 * m * m, dtype=torch.float32, device="cuda:0")
    plain = GemmCase(m, m, m, seed=621).dispatch(api)
    off = GemmCase(m, m, m, flags=TA, br_type=capi.BR_OFFSET, br_count=1, colbias=True, act=1, seed=622).dispatch(api)
    dev = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda:0")
    seg_ptr, oa, ob = dev([0, 1, 3]), dev([0, 0, 0]), dev([i * m * m * 4 for i in range(3)])
    oc, od = dev([m * m * 4, 0]), dev([0, -m * 4])                                # bases: the second half of `out`... and of `bias`
    api.hip_set_async(2)
    p = capi.GemmParam(); p.a.primary, p.b.primary, p.c.primary = X.data_ptr(), Y.data_ptr(), T.data_ptr()
    capi.Api.call(plain, p)                                                       # queued, nothing launched yet
    q = capi.GemmExtParam(); q.a.primary, q.b.primary, q.c.primary, q.d.primary = T.data_ptr(), Bs.data_ptr(), out.data_ptr(), bias.data_ptr() + m * 4
    api.hip_gemm_ext_batch_reduce_segments_offsets(off, C.byref(q), 2, seg_ptr.data_ptr(), oa.data_ptr(), ob.data_ptr(), oc.data_ptr(), od.data_ptr(), None)
    api.hip_sync(); api.check()
    api.hip_set_async(0); api.hip_set_stream(None)
    col = lambda t: t.cpu().numpy().astype(np.float64).reshape(m, m).T            # column-major block -> matrix
    Tm = (col(X) @ col(Y)).T                                                      # TRANS_A: the block is read as its transpose
    Bm = [col(Bs[i * m * m:(i + 1) * m * m]) for i in range(3)]
    bv = bias.cpu().numpy().astype(np.float64).reshape(2, m)
    got = out.cpu().numpy().astype(np.float64).reshape(2, m, m)
    assert np.array_equal(got[1].T, np.maximum(Tm @ Bm[0] + bv[1][:, None], 0)) and np.array_equal(got[0].T, np.maximum(Tm @ Bm[1] + Tm @ Bm[2] + bv[0][:, None], 0))


def test_a_captured_call_replays_on_new_operand_values():
    """One call captured on one stream (one linear node); the operand, bias and mask VALUES are overwritten in place -- the five bases travel by value, so the
    replay reads the same addresses -- the graph is replayed once and recomputes from them."""
    import torch
    api = capi.load()
    kw = dict(m=32, n=32, k=32, form="TN", colbias=True, act=2)
    sg = FusedOffsetSegments(api, seed=700, **kw)
    new = FusedOffsetSegments(api, seed=701, **kw)                                # same pattern and layout, other values
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
    for dev, pool in ((sg.dA, new.A), (sg.dB, new.B), (sg.dD, new.D), (out["C"], new.C0), (out["M"], new.M0)):
        for d, h in zip(dev, pool.host):
            d.copy_(torch.from_numpy(h))
    torch.cuda.synchronize()
    g.replay(); torch.cuda.synchronize()
    got, ref = sg.result(out), new.fma_chain()
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])


def test_guarded_rerun_with_operands_flush_against_unmapped_memory():
    """The f32 and bf16 parity tests again with every upload flush against unmapped address space (tests/guard.py via tests/conftest.py): the main pools, the last
    A, B, C, bias and mask block (arrays of their own) and the six lists.  These are parity tests on valid inputs: an access outside an operand -- a bias load
    that is not clamped, a mask byte past its block, a wide load of a transposed row past k -- would fault the subprocess.  Why none is expected: the loads are
    those of the plain offsets kernels (gemm_group_tile.hpp: rows / columns clamp to m - 1 / n - 1, k to K - 1, wide loads inside whole k blocks), the bias load
    clamps its row to m - 1, and a mask byte is written only by the lane of a valid row i = 8 q < m and column j < n: byte q + j * mask_ld / 8 of a block of
    mask_ld / 8 * n.  The second side only runs once the first has passed."""
    for side in ("end", "front"):
        env = dict(os.environ, LIBXSMM_TEST_GUARD=side)
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
               "-k", "test_f32_fused_offset_segments_are_bitwise or test_bf16_fused_offset_segments_match", "-v", "--no-header"]
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
        print(f"guarded run ({side}): {time.time() - t0:.1f} s")
        assert r.returncode == 0, f"guarded run ({side}) ended with {r.returncode} (negative / 134: the GPU faulted on an out-of-bounds access):\n{tail}"
        assert "10 passed" in r.stdout, tail
