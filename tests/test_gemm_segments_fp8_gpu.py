"""8-bit float (BF8 = E5M2, HF8 = E4M3) segments (include/libxsmm_hip.h): BF8 x BF8 -> f32 / BF8 and HF8 x HF8 -> f32 / HF8 handles, A VNNI-4, through the ADDRESS,
OFFSET and sliced entries.  On exact data (-1 / 0 / +1: every partial sum is exact) the results are bitwise the oracle's and the loop of single calls; on the
reference driver's random data an f32 C lies within the reference's own bound for chains as deep as the dense fp8 tests cover and within the documented
matrix-core bound beyond, an 8-bit C is at most the neighbouring code away in under 5 % of its elements; padding and gaps stay the caller's; every entry is one
launch (sliced: two) of the kernel named in the header; sliced calls repeat their bits; the launch modes and a captured graph keep the results; an ext handle
without operators is the plain call.  The last test re-runs the parity tests with every operand flush against unmapped memory (run this file with -x)."""
import contextlib
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import helpers
from helpers import GemmCase, TOL_F32, normf_rel
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG
from oracle import pyoracle
from segments_sliced_helpers import partial_case, slice_partial
from test_gemm_segments_gpu import COUNTS, Segments, _same, _up
from test_gemm_segments_offsets_gpu import OffsetSegments
from test_gemm_segments_sliced_gpu import Sliced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

V = GEMM_FLAG.VNNI_A
assert COUNTS == [0, 3, 64, 1, 0, 2, 7, 19, 1, 0]
# the smallest shapes that reach every path of the tile: (m, n, k, types, beta, (lda, ldb, ldc) - (m, k, m))
SHAPES = [
    dict(m=32, n=32, k=64, a_type=DT.HF8, c_type=DT.F32),                                   # a whole 32-tile, DEEP where the block is aligned
    dict(m=16, n=16, k=32, a_type=DT.BF8, c_type=DT.F32, beta=1),                           # one 16 x 16 x 32 step
    dict(m=23, n=37, k=20, a_type=DT.HF8, c_type=DT.F32, beta=1, pads=(2, 1, 6)),           # lda 25, ldb 21, ldc 29: ragged m, n; one step + a ragged quad; byte loads
    dict(m=12, n=10, k=8, a_type=DT.BF8, c_type=DT.BF8, beta=1),                            # ragged 16-tile, own-type C
    dict(m=40, n=40, k=40, a_type=DT.BF8, c_type=DT.BF8),                                   # 2 x 2 tiles, ragged
    dict(m=64, n=32, k=160, a_type=DT.HF8, c_type=DT.HF8, pads=(8, 16, 16)),                # lda 72, ldb 176, ldc 80: wide loads at padded leading dimensions
]
IDS = ["32x32x64-hf8-f32", "16x16x32-bf8-f32-beta1", "23x37x20-hf8-f32-beta1-padded", "12x10x8-bf8-bf8-beta1", "40x40x40-bf8-bf8", "64x32x160-hf8-hf8-padded"]
ONE = {DT.BF8: (0xbc, 0x00, 0x3c), DT.HF8: (0xb8, 0x00, 0x38)}                              # the bytes of -1 / 0 / +1
# random data, f32 C: the reference's bound for chains of count * k <= 576 (what test_fp8_gemm_matches_oracle covers with these instructions); deeper chains are
# held to the documented matrix-core bound (test_fp8_mfma_with_wide_exponent_range_data)
DEPTH_REF, TOL_DEEP = 576, 2e-4


def _exact(rng, count, dt):
    """-1 / 0 / +1 in `dt`: for the 8-bit floats their bytes (a cast of -1 to uint8 is 0xff, a NaN code)."""
    if dt in ONE:
        return np.asarray(ONE[dt], dtype=np.uint8)[rng.integers(0, 3, count)]
    assert dt == DT.F32
    return rng.integers(-1, 2, count).astype(np.float32)


@contextlib.contextmanager
def exact_values(on=True):
    """The pools of Segments / OffsetSegments / Sliced are drawn with helpers.rand_values: while this is active they hold -1 / 0 / +1."""
    saved = helpers.rand_values
    if on:
        helpers.rand_values = _exact
    try:
        yield
    finally:
        helpers.rand_values = saved


def make(api, entry, exact, seed, m, n, k, a_type, c_type, beta=0, pads=(0, 0, 0), **kw):
    with exact_values(exact):
        if entry == "address":
            return Segments(api, m, n, k, a_type=a_type, c_type=c_type, flags=V, beta=beta, lda=m + pads[0], ldb=k + pads[1], ldc=m + pads[2], seed=seed, **kw)
        if entry == "offset":
            return OffsetSegments(api, m, n, k, a_type=a_type, c_type=c_type, flags=V, beta=beta, pads=pads, seed=seed, **kw)
        return Sliced(api, m, n, k, form=None if entry == "sliced" else "NN", a_type=a_type, c_type=c_type, flags=V, beta=beta, pads=pads, seed=seed, **kw)


def _key(x):
    """8-bit float codes on one monotonic integer axis (sign-magnitude -> signed)."""
    x = x.astype(np.int32)
    return np.where(x & 0x80, -(x & 0x7f), x & 0x7f)


def check_random(sg, got, ref, nblocks, depth_of, what):
    """f32 C: normf_rel per block against the bound of its depth.  8-bit C: at most the neighbouring code, fewer than 5 % of all elements differ."""
    c = sg.case
    if c.c_type == DT.F32:
        for s in range(nblocks):
            err, depth = normf_rel(sg.valid(ref, s), sg.valid(got, s), DT.F32), depth_of(s)
            print(f"{what} block {s}: depth {depth} normf_rel {err:.3e}")
            assert err < (TOL_F32 if depth <= DEPTH_REF else TOL_DEEP), f"{what} block {s} (depth {depth}): normf_rel = {err}"
    else:
        d = np.concatenate([np.abs(_key(sg.valid(got, s)) - _key(sg.valid(ref, s))).ravel() for s in range(nblocks)])
        print(f"{what}: {np.mean(d != 0):.4f} of {d.size} elements differ, largest distance {d.max()} codes")
        assert d.max() <= 1 and np.mean(d != 0) < 0.05, f"{what}: {np.mean(d != 0)} of the elements differ, largest distance {d.max()} codes"


@pytest.mark.parametrize("entry", ["address", "offset"])
@pytest.mark.parametrize("kw", SHAPES, ids=IDS)
def test_exact_data_is_bitwise_the_oracle_and_the_loop(kw, entry):
    api = capi.load()
    for beta in (0, 1):
        sg = make(api, entry, True, 10 + beta, **dict(kw, beta=beta))
        got, ref = sg.run_checked(), sg.oracle()
        # whole arrays: the m x n blocks bit for bit, the padding of ldc and the gaps between the blocks unchanged
        assert _same(got, ref), f"{entry} {kw} beta={beta}: differs from the oracle (or wrote outside m x n)"
        sg.assert_padding_untouched(got, f"{entry} {kw} beta={beta}")
        assert _same(got, sg.run_loop()), f"{entry} {kw} beta={beta}: differs from the loop of single calls through the same handle"
        for s in np.flatnonzero(sg.counts == 0):                                  # empty segments: +0 under beta = 0, C's own bytes under beta = 1
            v = sg.valid(got, s)
            want = sg.valid(sg.C0.host, s) if beta else np.zeros_like(v)
            assert np.array_equal(v.view(np.uint8), want.view(np.uint8)), f"{entry} {kw} beta={beta}: empty segment {s}"


@pytest.mark.parametrize("entry", ["address", "offset"])
@pytest.mark.parametrize("kw", SHAPES, ids=IDS)
def test_random_data_matches_the_oracle(kw, entry):
    """Measured on an MI355X (largest normf_rel per depth = count * k, f32 C): DESIGN.md section 9.7."""
    api = capi.load()
    sg = make(api, entry, False, 20, **kw)
    got, ref = sg.run_checked(), sg.oracle()
    check_random(sg, got, ref, sg.nseg, lambda s: int(sg.counts[s]) * sg.case.k, f"{entry} {kw}")
    sg.assert_padding_untouched(got, f"{entry} {kw}")


KERNELS = [("address", DT.BF8, b"gemm_segments_bf8_kernel"), ("address", DT.HF8, b"gemm_segments_hf8_kernel"),
           ("offset", DT.BF8, b"gemm_segments_offs_bf8_kernel<0,0>"), ("offset", DT.HF8, b"gemm_segments_offs_hf8_kernel<0,0>"),
           ("sliced", DT.BF8, b"gemm_segments_sliced_bf8_kernel"), ("sliced", DT.HF8, b"gemm_segments_sliced_hf8_kernel"),
           ("offset_sliced", DT.BF8, b"gemm_segments_offs_sliced_bf8_kernel<0,0>"), ("offset_sliced", DT.HF8, b"gemm_segments_offs_sliced_hf8_kernel<0,0>")]


def test_kernel_names_and_launch_counts():
    api = capi.load()
    for entry, t, name in KERNELS:
        for c_type in (DT.F32, t):
            sg = make(api, entry, True, 30, m=40, n=40, k=40, a_type=t, c_type=c_type)
            cset = sg.new_c()
            api.hip_launch_count(1)
            sg.run(cset)
            assert api.hip_launch_count(1) == (2 if "sliced" in entry else 1), (entry, t)
            api.hip_sync(); api.check()
            assert api.hip_kernel_name(sg.handle, 1) == name, (entry, t, api.hip_kernel_name(sg.handle, 1))
    # nslices = 0: only pass 2 runs -- instance <0>, <3> or <4> by C's type -- and stores +0 under beta = 0
    for t, c_type in ((DT.BF8, DT.F32), (DT.BF8, DT.BF8), (DT.HF8, DT.HF8)):
        sg = make(api, "sliced", True, 31, m=40, n=40, k=40, a_type=t, c_type=c_type)
        cset = sg.new_c()
        zeros = _up(np.zeros(sg.nblocks + 1, dtype=np.uint64))
        api.hip_launch_count(1)
        api.hip_gemm_batch_reduce_segments_sliced(sg.handle, C.byref(capi.GemmParam()), sg.nblocks, zeros.data_ptr(), 0, None, None, None, cset[1].data_ptr(), None, 0)
        assert api.hip_launch_count(1) == 1
        api.hip_sync(); api.check()
        got = sg.C0.download(cset[0])
        for b in range(sg.nblocks):
            assert not sg.valid(got, b).view(np.uint8).any()
        sg.assert_padding_untouched(got, "no slices")


def sliced_statement(sg):
    """The CPU statement of a sliced call for these classes (segments_sliced_helpers.py says it for f32 / bf16 / f64): f32 partials from +0 per slice (the oracle's
    chain), added in ascending slice order to widen(C) or +0 in numpy.float32, then ONE store -- through the oracle's f32 -> f16 -> 8 bits for an 8-bit C."""
    c, orc = sg.case, pyoracle.oracle()
    pcase = partial_case(c)
    ha, hb = sg.A.host_ptrs(sg.ai), sg.B.host_ptrs(sg.bi)
    a0, b0 = sg.A.host[0].ctypes.data, sg.B.host[0].ctypes.data
    oa, ob = ha.view(np.int64) - np.int64(a0), hb.view(np.int64) - np.int64(b0)
    cvt = {DT.BF8: orc.lib.oracle_f32_to_bf8_rne, DT.HF8: orc.lib.oracle_f32_to_hf8_rne}.get(c.c_type)
    out = sg.C0.copy()
    for b in range(sg.nblocks):
        j0, j1 = int(sg.blk_ptr[b]), int(sg.blk_ptr[b + 1])
        if j0 == j1 and sg.beta:
            continue
        view = sg.C0.block(out.host, b)[:c.ldc * c.n].reshape(c.n, c.ldc)[:, :c.m]
        if not sg.beta:
            s = np.zeros((c.n, c.m), dtype=np.float32)
        else:
            s = view.astype(np.float32) if cvt is None else helpers.as_float(view, c.c_type).astype(np.float32)
        for j in range(j0, j1):
            p = capi.GemmParam()
            r = int(sg.seg_ptr[j]) * 8
            if sg.form is None:
                p.a.primary, p.b.primary = ha.ctypes.data + r, hb.ctypes.data + r
            else:
                p.a.primary, p.b.primary, p.a.secondary, p.b.secondary = a0, b0, oa.ctypes.data + r, ob.ctypes.data + r
            s = s + slice_partial(pcase, p, int(sg.seg_ptr[j + 1]) - int(sg.seg_ptr[j]), False)
            assert s.dtype == np.float32
        view[:] = s if cvt is None else np.array([cvt(C.c_float(x)) & 0xff for x in s.ravel()], dtype=np.uint8).reshape(c.n, c.m)
    return out.host


# blocks of 0, 1, 2, 3 and 9 slices of 0 .. 19 products (the siblings' pattern); then one chain of 64 products cut into 1, 4 and 16 slices next to an empty block
CUTS = dict(slices=[1, 4, 16, 0], products=[64] + [16] * 4 + [4] * 16)
SLICED_SHAPES = [SHAPES[0], SHAPES[2], SHAPES[3], SHAPES[5]]
SLICED_IDS = [IDS[0], IDS[2], IDS[3], IDS[5]]


@pytest.mark.parametrize("entry", ["sliced", "offset_sliced"])
@pytest.mark.parametrize("kw", SLICED_SHAPES, ids=SLICED_IDS)
def test_sliced_exact_data_is_bitwise_the_statement(kw, entry):
    api = capi.load()
    for beta in (0, 1):
        for cut in (dict(), CUTS):
            sg = make(api, entry, True, 40 + beta, **dict(kw, beta=beta), **cut)
            got = sg.run_checked()
            assert _same(got, sliced_statement(sg)), f"{entry} {kw} beta={beta} {cut}: differs from the statement (or wrote outside m x n)"
            sg.assert_padding_untouched(got, f"{entry} {kw} beta={beta}")
            b = 3 if cut else 0                                                   # the block without slices follows beta
            v = sg.valid(got, b)
            want = sg.valid(sg.C0.host, b) if beta else np.zeros_like(v)
            assert np.array_equal(v.view(np.uint8), want.view(np.uint8)), f"{entry} {kw} beta={beta}: the block without slices"
        if beta == 0:                                                             # the same 64-product chain in 1, 4 and 16 slices: exact sums, one result
            sg = make(api, entry, True, 42, **dict(kw, beta=0), **CUTS)
            sg.ai[:] = np.tile(sg.ai[:64], 3); sg.bi[:] = np.tile(sg.bi[:64], 3)
            sg.upload_lists()
            got = sg.run_checked()
            assert np.array_equal(sg.valid(got, 0), sg.valid(got, 1)) and np.array_equal(sg.valid(got, 0), sg.valid(got, 2)), f"{entry} {kw}: 1, 4 and 16 slices differ"
            assert _same(got, sliced_statement(sg))


@pytest.mark.parametrize("entry", ["sliced", "offset_sliced"])
@pytest.mark.parametrize("kw", SLICED_SHAPES, ids=SLICED_IDS)
def test_sliced_random_data_matches_the_statement_and_repeats_its_bits(kw, entry):
    import torch
    api = capi.load()
    for cut in (dict(), CUTS):
        sg = make(api, entry, False, 50, **kw, **cut)
        got, ref = sg.run_checked(), sliced_statement(sg)
        depth = lambda b: int(sg.seg_ptr[int(sg.blk_ptr[b + 1])] - sg.seg_ptr[int(sg.blk_ptr[b])]) * sg.case.k      # noqa: E731
        check_random(sg, got, ref, sg.nblocks, depth, f"{entry} {kw} {cut}")
        sg.assert_padding_untouched(got, f"{entry} {kw}")
        assert _same(sg.run_checked(), got), f"{entry} {kw}: a second run gives other bits"
        side = torch.cuda.Stream()
        api.hip_set_stream(side.cuda_stream)
        cset = sg.new_c()
        torch.cuda.synchronize()
        sg.run(cset)
        api.hip_sync(); api.check()
        api.hip_set_stream(None); api.hip_set_async(0)
        assert _same(sg.C0.download(cset[0]), got), f"{entry} {kw}: another stream gives other bits"


def test_one_slice_per_block_is_bitwise_the_unsliced_call():
    api = capi.load()
    products = [0, 3, 64, 1, 2, 7, 19]
    for i, kw in enumerate(SHAPES):
        for entry in ("sliced", "offset_sliced"):
            sg = make(api, entry, False, 60 + i, **dict(kw, beta=0), slices=[1] * len(products), products=products)      # random values: the same chain, the same bits
            want = sg.new_c()
            sg.run_unsliced(want)
            api.hip_sync(); api.check()
            assert _same(sg.run_checked(), sg.C0.download(want[0])), f"{entry} {kw}: differs from the unsliced entry on the same lists"


def test_a_short_workspace_is_minus_two_and_an_unaligned_one_minus_three():
    api = capi.load()
    for t, c_type in ((DT.BF8, DT.BF8), (DT.HF8, DT.F32)):
        sg = make(api, "sliced", True, 70, m=23, n=37, k=20, a_type=t, c_type=c_type, pads=(2, 1, 6))
        assert sg.ws_bytes % 16 == 0 and sg.ws_bytes >= sg.nslices * 23 * 37 * 4
        ws = sg.new_ws(extra=64)
        for ws_ptr_shift, ws_bytes, code in ((0, sg.ws_bytes - 1, -2), (4, sg.ws_bytes, -3)):
            cset = sg.new_c()
            api.hip_launch_count(1)
            fn = api.hip_gemm_batch_reduce_segments_sliced
            fn(sg.handle, C.byref(sg.param(cset)), sg.nblocks, sg.d_blk.data_ptr(), sg.nslices, sg.d_seg.data_ptr(), sg.d_la.data_ptr(), sg.d_lb.data_ptr(),
               cset[1].data_ptr(), ws.data_ptr() + ws_ptr_shift, ws_bytes)
            assert api.hip_get_last_error() == code and api.hip_launch_count(1) == 0
            api.hip_clear_last_error()
            assert _same(sg.C0.download(cset[0]), sg.C0.host)
        cset = sg.new_c()                                                         # and the queried size is enough: nothing beyond it is written
        sg.run(cset, ws=ws)
        api.hip_sync(); api.check()
        tail = np.ascontiguousarray(ws.cpu().numpy()).view(np.uint8)[sg.ws_bytes:]
        assert tail.size == 64 and (tail == 0xA5).all()


def test_modes_stream_pipeline_coalescing_and_graph_keep_the_results():
    import torch
    api = capi.load()
    kw = dict(m=40, n=40, k=40, a_type=DT.BF8, c_type=DT.BF8, beta=1)
    segs = [make(api, entry, False, 80 + i, **kw) for i, entry in enumerate(("address", "offset", "sliced"))]
    want = [sg.run_checked() for sg in segs]                                      # blocking
    workspaces = [None, None, segs[2].new_ws()]
    run = lambda sg, cs, ws: sg.run(cs, ws=ws) if ws is not None else sg.run(cs)  # noqa: E731
    # stream-ordered on a torch stream
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    csets = [sg.new_c() for sg in segs]
    for sg, cs, ws in zip(segs, csets, workspaces):
        run(sg, cs, ws)
    api.hip_sync(); api.check()
    for sg, cs, w in zip(segs, csets, want):
        assert _same(sg.C0.download(cs[0]), w), "stream-ordered"
    # inside a pipeline section
    csets = [sg.new_c() for sg in segs]
    assert api.hip_pipeline_begin(4) == 0
    for sg, cs, ws in zip(segs, csets, workspaces):
        run(sg, cs, ws)
    assert api.hip_pipeline_end() == 0
    api.hip_sync(); api.check()
    for sg, cs, w in zip(segs, csets, want):
        assert _same(sg.C0.download(cs[0]), w), "pipeline section"
    # the coalescing queue: a queued single call is flushed ahead of the segments call
    single = GemmCase(32, 32, 32, seed=81)
    h = single.dispatch(api)
    dA, dB, dC, dC1 = _up(single.A), _up(single.B), _up(single.C0.copy()), _up(single.C0.copy())
    p = capi.GemmParam(); p.a.primary, p.b.primary, p.c.primary = dA.data_ptr(), dB.data_ptr(), dC1.data_ptr()
    capi.Api.call(h, p)                                                           # blocking: what the queued call below must give
    api.hip_sync(); api.check()
    api.hip_set_async(2)
    p = capi.GemmParam(); p.a.primary, p.b.primary, p.c.primary = dA.data_ptr(), dB.data_ptr(), dC.data_ptr()
    capi.Api.call(h, p)                                                           # queued
    csets = [sg.new_c() for sg in segs]
    for sg, cs, ws in zip(segs, csets, workspaces):
        run(sg, cs, ws)
    api.hip_sync(); api.check()
    api.hip_set_async(0); api.hip_set_stream(None)
    for sg, cs, w in zip(segs, csets, want):
        assert _same(sg.C0.download(cs[0]), w), "coalescing queue"
    assert np.array_equal(dC.cpu().numpy(), dC1.cpu().numpy())
    # a captured call, replayed after the operands were overwritten in place
    sg, new = make(api, "address", False, 82, **kw), make(api, "address", False, 83, **kw)
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
        for d, hst in zip(dev, pool.host):
            d.copy_(torch.from_numpy(hst))
    torch.cuda.synchronize()
    g.replay(); torch.cuda.synchronize()
    got = sg.C0.download(cset[0])
    sg.A, sg.B, sg.C0 = new.A, new.B, new.C0
    assert _same(got, sg.run_checked()), "the replay differs from a fresh call on the new operands"


def test_an_ext_handle_without_operators_is_bit_for_bit_the_plain_call():
    api = capi.load()
    for kw in (SHAPES[2], SHAPES[4]):
        sg = make(api, "address", False, 90, **kw)
        want = sg.run_checked()
        c = sg.case
        ext = api.dispatch_brgemm_ext(c.shape(), c.flags, 0, c.brcfg(), capi.no_argops(), capi.no_postops())
        assert ext
        cset = sg.new_c()
        api.hip_launch_count(1)
        api.hip_gemm_ext_batch_reduce_segments(ext, C.byref(capi.GemmExtParam()), sg.nseg, sg.d_seg.data_ptr(), sg.d_la.data_ptr(), sg.d_lb.data_ptr(), cset[1].data_ptr(), None, None)
        assert api.hip_launch_count(1) == 1
        api.hip_sync(); api.check()
        assert api.hip_kernel_name(ext, 1) == (b"gemm_segments_hf8_kernel" if c.a_type == DT.HF8 else b"gemm_segments_bf8_kernel")
        assert _same(sg.C0.download(cset[0]), want), f"{kw}: the ext entry differs from the plain one"


def test_c_example_multiplies_a_block_sparse_hf8_layer_in_one_call(tmp_path):
    libdir = os.path.join(ROOT, "libxsmm_amd", "lib")
    exe = str(tmp_path / "segments_fp8_driver")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "segments_fp8_driver.c"),
           "-L" + libdir, "-lxsmm_amd", "-lm", "-Wl,-rpath," + libdir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "normf_rel" in r.stdout and "1 launch" in r.stdout


GUARDED = "test_exact_data_is_bitwise or test_random_data_matches or test_sliced_exact_data"      # (the sliced random-data test runs the same kernels on the same layouts)


def test_guarded_rerun_with_operands_flush_against_unmapped_memory():
    """The exact-data and random-data parity tests again with every upload flush against unmapped address space (tests/guard.py via tests/conftest.py): the pools,
    the last A, B and C block (arrays of their own), the lists and the workspace, which is exactly as large as the query says.  These are parity tests on valid
    inputs: an access outside an operand would fault the subprocess.  Why none is expected (gemm_group_tile.hpp, tile_fp8): a lane's row / column is clamped to
    m - 1 / n - 1; a whole step reads k0 .. k0 + 7 with k0 + 8 <= K, as two dwords of the VNNI-4 image at ((k0 / 4 + e) * lda + i) * 4 (4-byte aligned blocks
    only) and one 8-byte load at j * ldb + k0 (8-byte aligned blocks and ldb only), or byte by byte; the ragged step reads bytes at min(k, K - 1).  So an A block
    is read inside bytes 0 .. ((K / 4 - 1) * lda + m - 1) * 4 + 3, a B block inside 0 .. (n - 1) * ldb + K - 1, both inside the lda * k / ldb * n bytes of a block.
    C is read and written at i < m, j < n only, byte by byte or as f32; pass 2 reads 16 bytes of a partial that is padded to 16 and stores a dword of C only when
    m, ldc and the pointer are multiples of 4.  The second side only runs once the first has passed."""
    for side in ("end", "front"):
        env = dict(os.environ, LIBXSMM_TEST_GUARD=side)
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "-k", GUARDED, "-v", "--no-header"]
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
        print(f"guarded run ({side}): {time.time() - t0:.1f} s")
        assert r.returncode == 0, f"guarded run ({side}) ended with {r.returncode} (negative / 134: the GPU faulted on an out-of-bounds access):\n{tail}"
        assert "32 passed" in r.stdout, tail
