"""IEEE-half (f16) segments (include/libxsmm_hip.h): F16 x F16 -> f32 / f16 handles, A flat or VNNI-2, through the ADDRESS and OFFSET (NN, NT) entries, their ext
siblings with a column bias, ReLU (+ bitmask) and sigmoid, and the sliced forms of all of them.  The arithmetic is the reference's F16 loop, not bf16's: the
chain runs from +0 and the start value (C, the bias, bias + C), rounded to a half, is added behind it.  On exact data (-1 / 0 / +1: every partial sum is exact)
the results are bitwise the oracle's and the loop of single calls; on the reference driver's random data each segment lies within the dense f16 bounds of this
project (tests/test_gemm_gpu.py::_tol); the start rule is checked on an f32 C with 24-bit mantissas; one slice per block is bitwise the unsliced call for every
beta and with a bias; padding, gaps and mask bits outside the blocks stay the caller's; the launch modes and a captured graph keep the bits.  The last test
re-runs the parity tests with every operand flush against unmapped memory (run this file with -x).

No f16 handle has TRANS_A (libxsmm_dispatch_brgemm returns none: the reference's F16 loop has no transposed A), so the OFFSET forms are NN and NT."""
import contextlib
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import helpers
from helpers import TOL_F32, normf_rel
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG
from oracle import pyoracle
from segments_sliced_fused_helpers import activation, mask_of
from segments_sliced_helpers import partial_case, slice_partial
from test_gemm_segments_fused_gpu import FusedSegments
from test_gemm_segments_gpu import COUNTS, Segments, _same, _up
from test_gemm_segments_offsets_fused_gpu import FusedOffsetSegments
from test_gemm_segments_offsets_gpu import OffsetSegments
from test_gemm_segments_sliced_fused_gpu import SlicedFused
from test_gemm_segments_sliced_gpu import Sliced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

V = GEMM_FLAG.VNNI_A
assert COUNTS == [0, 3, 64, 1, 0, 2, 7, 19, 1, 0]
# the smallest shapes that reach every path of the tile: flags, form (OFFSET entries) and (lda, ldb, ldc) - their smallest values
SHAPES = [
    dict(m=13, n=11, k=18),                                    # 16-tile, ragged k, flat A
    dict(m=40, n=24, k=20, flags=V),                           # 32-tile, ragged rows / columns / k, VNNI-2
    dict(m=33, n=17, k=18, pads=(0, 0, 7), beta=1),            # ldc = 40, beta = 1
    dict(m=64, n=64, k=64, flags=V),                           # whole tiles, wide loads, the DEEP round
    dict(m=32, n=32, k=34, form="NT", pads=(3, 3, 6)),         # transposed B, odd leading dimensions
]
IDS = ["13x11x18-flat", "40x24x20-vnni", "33x17x18-ldc40-beta1", "64x64x64-vnni", "32x32x34-nt-padded"]
# Random data: this project's bounds for dense f16 GEMMs (tests/test_gemm_gpu.py::_tol) -- the reference's 1.2e-5 for an f32 C, 1e-3 for an f16 C -- for chains
# of count * k <= 576; deeper chains are held to the segment family's matrix-core bound 2e-4 (tests/test_gemm_segments_fp8_gpu.py), whatever C's type.
DEPTH_REF, TOL_DEEP, TOL_F16 = 576, 2e-4, 1e-3


def _exact(rng, count, dt):
    """-1 / 0 / +1 in `dt`; halves as numpy.float16 viewed as uint16 (a cast of -1 to uint16 would be the bit pattern 0xffff, a NaN)."""
    v = rng.integers(-1, 2, count)
    if dt == DT.F16:
        return v.astype(np.float16).view(np.uint16)
    assert dt == DT.F32
    return v.astype(np.float32)


@contextlib.contextmanager
def exact_values(on=True):
    """The pools of the sibling files' classes are drawn with helpers.rand_values: while this is active they hold -1 / 0 / +1."""
    saved = helpers.rand_values
    if on:
        helpers.rand_values = _exact
    try:
        yield
    finally:
        helpers.rand_values = saved


def make(api, entry, exact, seed, m, n, k, c_type, flags=0, form="NN", beta=0, pads=(0, 0, 0), colbias=False, act=0, **kw):
    """entry: address / offset / sliced / offset_sliced, with the prefix ext_ the ext sibling (colbias, act)."""
    ext, base = entry.startswith("ext_"), entry.replace("ext_", "")
    e = dict(colbias=colbias, act=act) if ext else {}
    lds = dict(lda=m + pads[0], ldb=k + pads[1], ldc=m + pads[2])
    with exact_values(exact):
        if base == "address":
            assert form == "NN"
            return (FusedSegments if ext else Segments)(api, m, n, k, a_type=DT.F16, c_type=c_type, flags=flags, beta=beta, seed=seed, **lds, **e, **kw)
        if base == "offset":
            return (FusedOffsetSegments if ext else OffsetSegments)(api, m, n, k, form=form, a_type=DT.F16, c_type=c_type, flags=flags, beta=beta, pads=pads, seed=seed, **e, **kw)
        assert base in ("sliced", "offset_sliced") and (form == "NN" or base == "offset_sliced")
        return (SlicedFused if ext else Sliced)(api, m, n, k, form=None if base == "sliced" else form, a_type=DT.F16, c_type=c_type, flags=flags, beta=beta, pads=pads,
                                                seed=seed, **e, **kw)


def entries_of(kw):
    """The unsliced entries a shape can go through: a transposed B needs the OFFSET entry."""
    return ("offset",) if kw.get("form", "NN") != "NN" else ("address", "offset")


def tol_of(c_type, depth):
    return TOL_DEEP if depth > DEPTH_REF else (TOL_F16 if c_type == DT.F16 else TOL_F32)


def to_f16_bits(x):
    """f32 -> f16 through the oracle's conversion [ref: src/libxsmm_math.c libxsmm_convert_f32_to_f16], element by element."""
    fn = pyoracle.oracle().lib.oracle_f32_to_f16
    x = np.ascontiguousarray(x, dtype=np.float32)
    return np.array([fn(C.c_float(v)) & 0xffff for v in x.ravel()], dtype=np.uint16).reshape(x.shape)


def widen(x, c_type):
    """Values of C's type as float32."""
    return np.ascontiguousarray(x).view(np.float16).astype(np.float32) if c_type == DT.F16 else np.asarray(x, dtype=np.float32)


def round16(x):
    """f32 -> f16 -> f32: what the start value goes through."""
    return widen(to_f16_bits(x), DT.F16)


def check_segments(sg, got, ref, n, depth_of, what):
    worst = {}
    for s in range(n):
        err, depth = normf_rel(sg.valid(ref, s), sg.valid(got, s), sg.case.c_type), depth_of(s)
        worst[depth] = max(worst.get(depth, 0.0), err)
        assert err < tol_of(sg.case.c_type, depth), f"{what} block {s} (depth {depth}): normf_rel = {err}"
    print(f"{what}: largest normf_rel per depth {worst}")


# ---- unsliced: the four plain and ext entries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_type", [DT.F32, DT.F16], ids=["f32", "f16"])
@pytest.mark.parametrize("kw", SHAPES, ids=IDS)
def test_exact_data_is_bitwise_the_oracle_and_the_loop(kw, c_type):
    api = capi.load()
    for entry in entries_of(kw):
        for beta in (0, 1):
            sg = make(api, entry, True, 10 + beta, c_type=c_type, **dict(kw, beta=beta))
            got, ref = sg.run_checked(), sg.oracle()
            # whole arrays: the m x n blocks bit for bit, the padding of ldc and the gaps between the blocks unchanged
            assert _same(got, ref), f"{entry} {kw} beta={beta}: differs from the oracle (or wrote outside m x n)"
            sg.assert_padding_untouched(got, f"{entry} {kw} beta={beta}")
            assert _same(got, sg.run_loop()), f"{entry} {kw} beta={beta}: differs from the loop of single calls through the same handle"


EPILOGUES = [(True, 0), (False, 2), (True, 2), (True, 3)]          # bias, ReLU + bitmask, bias + ReLU + bitmask, bias + sigmoid


@pytest.mark.parametrize("c_type", [DT.F32, DT.F16], ids=["f32", "f16"])
@pytest.mark.parametrize("kw", SHAPES, ids=IDS)
def test_fused_exact_data_is_bitwise_the_ext_oracle_mask_included(kw, c_type):
    api = capi.load()
    for entry in entries_of(kw):
        for beta in (0, 1):
            sg = make(api, "ext_" + entry, True, 20 + beta, c_type=c_type, **dict(kw, beta=beta))
            for colbias, act in EPILOGUES:
                what = f"ext {entry} {kw} beta={beta} colbias={colbias} act={act}"
                sg.set_epilogue(colbias, act)
                (got, gotm), (ref, refm) = sg.run_checked(), sg.oracle_ext()
                sg.assert_outside_untouched(got, gotm, what)
                if act == 3:                                                      # the sums are exact, the hardware's exp is not the oracle's
                    check_segments(sg, got, ref, sg.nseg, lambda s: 0, what)
                    continue
                assert _same(got, ref), f"{what}: C differs from the ext oracle (or bytes outside m x n changed)"
                assert _same(gotm, refm), f"{what}: the mask differs from the ext oracle (or bits outside m x n changed)"
                if act == 2 and colbias:
                    loop = sg.run_loop()
                    assert loop is None or (_same(got, loop[0]) and _same(gotm, loop[1])), f"{what}: differs from the loop of fused single calls"


@pytest.mark.parametrize("c_type", [DT.F32, DT.F16], ids=["f32", "f16"])
@pytest.mark.parametrize("kw", SHAPES, ids=IDS)
def test_random_data_matches_the_oracle(kw, c_type):
    """Measured on an MI355X (largest normf_rel per depth = count * k): DESIGN.md section 9.8."""
    api = capi.load()
    for entry in entries_of(kw):
        sg = make(api, entry, False, 30, c_type=c_type, **kw)
        got, ref = sg.run_checked(), sg.oracle()
        check_segments(sg, got, ref, sg.nseg, lambda s: int(sg.counts[s]) * sg.case.k, f"{entry} {kw}")
        sg.assert_padding_untouched(got, f"{entry} {kw}")
        fs = make(api, "ext_" + entry, False, 31, c_type=c_type, colbias=True, act=1, **kw)
        (got, gotm), (ref, _) = fs.run_checked(), fs.oracle_ext()
        check_segments(fs, got, ref, fs.nseg, lambda s: int(fs.counts[s]) * fs.case.k, f"ext {entry} {kw} bias + ReLU")
        fs.assert_outside_untouched(got, gotm, f"ext {entry} {kw}")


def _wide_c(sg, seed):
    """C values with 24-bit mantissas, large against the sums (|C| up to 64; a half keeps 11 bits), written into the host pool before it is uploaded."""
    rng = np.random.default_rng(seed)
    for h in sg.C0.host:
        h[:] = rng.uniform(-64.0, 64.0, h.size).astype(np.float32)
    assert any((h.view(np.uint32) & 0x1fff).any() for h in sg.C0.host)


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "bias-plus-c"])
def test_the_start_value_is_rounded_to_a_half_and_added_last(fused):
    api = capi.load()
    kw = dict(m=33, n=17, k=18, pads=(0, 0, 7), beta=1)
    sg = make(api, "ext_address" if fused else "address", False, 40, c_type=DT.F32, colbias=fused, **kw)
    _wide_c(sg, 41)
    # ---- on the CPU first: the check discriminates.  The same chain started at the UNROUNDED start value (bf16's order) is outside the bound for a long segment
    ref = sg.oracle_ext()[0] if fused else sg.oracle()
    zero = make(api, "address", False, 40, c_type=DT.F32, **dict(kw, beta=0))     # same seed: the same A, B and lists; beta = 0: the sums alone
    sums = zero.oracle()
    long_s = int(np.argmax(sg.counts))
    start = sg.valid(sg.C0.host, long_s).astype(np.float32)
    if fused:
        start = sg.bias_of(long_s)[None, :sg.case.m].astype(np.float32) + start
    wrong = start + zero.valid(sums, long_s)
    assert wrong.dtype == np.float32
    err = normf_rel(sg.valid(ref, long_s), wrong, DT.F32)
    print(f"start first, unrounded: normf_rel {err:.3e} from the oracle")
    assert err > TOL_F32, f"the unrounded start value is only {err} from the oracle: the test would not tell the two orders apart"
    # ---- the GPU: a segment of count 0 is f16(start) widened, bit for bit; every segment within its bound
    got = sg.run_checked()
    got = got[0] if fused else got
    for s in np.flatnonzero(sg.counts == 0):
        st = sg.valid(sg.C0.host, s).astype(np.float32)
        if fused:
            st = sg.bias_of(s)[None, :sg.case.m].astype(np.float32) + st
        want = round16(st)
        assert np.array_equal(sg.valid(got, s).view(np.uint32), want.view(np.uint32)), f"empty segment {s}: not f16(start) widened"
        assert np.array_equal(sg.valid(ref, s).view(np.uint32), want.view(np.uint32)), f"empty segment {s}: the oracle disagrees"
        assert not np.array_equal(want.view(np.uint32), st.view(np.uint32))
    check_segments(sg, got, ref, sg.nseg, lambda s: int(sg.counts[s]) * sg.case.k, f"start rule fused={fused}")
    assert normf_rel(wrong, sg.valid(got, long_s), DT.F32) > TOL_F32


# ---- sliced -----------------------------------------------------------------------------------------------------------------------------------------------
def sliced_statement(sg):
    """The CPU statement of pass 2 for the f16 class: acc = +0; acc += P_j in ascending slice order, one numpy.float32 add each (P_j: the oracle's chain of the
    slice from +0); then the start value -- C, the bias, bias + C in one f32 add -- rounded to a half, widened and added in one f32 add; mask !(x <= 0);
    activation; one store, an f16 C through the oracle's f32 -> f16.  A block without slices: plain entries +0 (beta = 0) or untouched (beta = 1); ext entries the
    same statement with no partials.  Returns (C arrays, mask arrays or None)."""
    c = sg.case
    fused = isinstance(sg, SlicedFused)
    colbias, act = (sg.colbias, sg.act) if fused else (False, 0)
    pcase = partial_case(c)
    ha, hb = sg.A.host_ptrs(sg.ai), sg.B.host_ptrs(sg.bi)
    a0, b0 = sg.A.host[0].ctypes.data, sg.B.host[0].ctypes.data
    oa, ob = ha.view(np.int64) - np.int64(a0), hb.view(np.int64) - np.int64(b0)
    outc, outm = sg.C0.copy(), (sg.M0.copy() if fused else None)
    for b in range(sg.nblocks):
        j0, j1 = int(sg.blk_ptr[b]), int(sg.blk_ptr[b + 1])
        view = sg.C0.block(outc.host, b)[:c.ldc * c.n].reshape(c.n, c.ldc)[:, :c.m]
        if not fused and j0 == j1:
            if not sg.beta:
                view[:] = 0
            continue
        acc = np.zeros((c.n, c.m), dtype=np.float32)
        for j in range(j0, j1):
            p = capi.GemmParam()
            r = int(sg.seg_ptr[j]) * 8
            if sg.form is None:
                p.a.primary, p.b.primary = ha.ctypes.data + r, hb.ctypes.data + r
            else:
                p.a.primary, p.b.primary, p.a.secondary, p.b.secondary = a0, b0, oa.ctypes.data + r, ob.ctypes.data + r
            acc = acc + slice_partial(pcase, p, int(sg.seg_ptr[j + 1]) - int(sg.seg_ptr[j]), False)
            assert acc.dtype == np.float32
        if sg.beta or colbias:
            start = widen(view, c.c_type) if sg.beta else np.zeros((c.n, c.m), dtype=np.float32)
            if colbias:
                bias = widen(sg.bias_of(b)[:c.m], c.c_type)[None, :]
                start = (bias + start) if sg.beta else np.broadcast_to(bias, (c.n, c.m))
            acc = acc + round16(start)
            assert acc.dtype == np.float32
        if act == 2:
            sg.M0.block(outm.host, b)[:] = mask_of(c, sg.M0.block(sg.M0.host, b), acc)
        y = activation(act, acc)
        view[:] = to_f16_bits(y) if c.c_type == DT.F16 else y
    return outc.host, (outm.host if fused else None)


def run_sliced(sg):
    out = sg.run_checked()
    return out if isinstance(sg, SlicedFused) else (out, None)


def same_out(a, b):
    return _same(a[0], b[0]) and (a[1] is None or _same(a[1], b[1]))


# blocks of 0, 1, 2, 3 and 9 slices of 0 .. 19 products (the siblings' pattern); then one chain of 64 products cut into 1, 4 and 16 slices next to an empty block
CUTS = dict(slices=[1, 4, 16, 0], products=[64] + [16] * 4 + [4] * 16)
SLICED_CASES = [("sliced", SHAPES[0]), ("offset_sliced", SHAPES[1]), ("sliced", SHAPES[2]), ("offset_sliced", SHAPES[3]), ("offset_sliced", SHAPES[4])]


@pytest.mark.parametrize("c_type", [DT.F32, DT.F16], ids=["f32", "f16"])
@pytest.mark.parametrize("entry,kw", SLICED_CASES, ids=IDS)
def test_sliced_exact_data_is_bitwise_the_statement(entry, kw, c_type):
    api = capi.load()
    for beta in (0, 1):
        for cut in (dict(), CUTS):
            sg = make(api, entry, True, 50 + beta, c_type=c_type, **dict(kw, beta=beta), **cut)
            got = run_sliced(sg)
            assert same_out(got, sliced_statement(sg)), f"{entry} {kw} beta={beta} {cut}: differs from the statement (or wrote outside m x n)"
            sg.assert_padding_untouched(got[0], f"{entry} {kw} beta={beta}")
            b = 3 if cut else 0                                                   # the block without slices: +0 under beta = 0, untouched under beta = 1
            v = sg.valid(got[0], b)
            want = sg.valid(sg.C0.host, b) if beta else np.zeros_like(v)
            assert np.array_equal(v.view(np.uint8), want.view(np.uint8)), f"{entry} {kw} beta={beta}: the block without slices"
        fs = make(api, "ext_" + entry, True, 52 + beta, c_type=c_type, **dict(kw, beta=beta), **CUTS)
        for colbias, act in ((True, 2), (False, 2), (True, 0)):
            fs.set_epilogue(colbias, act)
            got = run_sliced(fs)
            assert same_out(got, sliced_statement(fs)), f"ext {entry} {kw} beta={beta} colbias={colbias} act={act}: differs from the statement"
            fs.assert_outside_untouched(got[0], got[1], f"ext {entry} {kw} beta={beta}")


@pytest.mark.parametrize("c_type", [DT.F32, DT.F16], ids=["f32", "f16"])
@pytest.mark.parametrize("entry,kw", SLICED_CASES, ids=IDS)
def test_sliced_random_data_matches_the_statement_and_repeats_its_bits(entry, kw, c_type):
    """Pass 2 is plain IEEE arithmetic on the partials; the partials are the matrix core's sums, within the bound of their depth of the oracle's, so on random
    data the statement holds within that bound (bit for bit on exact data, above).  Measured: DESIGN.md section 9.8."""
    import torch
    api = capi.load()
    for ext in (False, True):
        sg = make(api, ("ext_" if ext else "") + entry, False, 60, c_type=c_type, colbias=ext, act=2 if ext else 0, **dict(kw, beta=1), **CUTS)
        got, ref = run_sliced(sg), sliced_statement(sg)
        depth = lambda b: int(sg.seg_ptr[int(sg.blk_ptr[b + 1])] - sg.seg_ptr[int(sg.blk_ptr[b])]) * sg.case.k      # noqa: E731
        check_segments(sg, got[0], ref[0], sg.nblocks, depth, f"{entry} {kw} ext={ext}")
        for rep in range(3):                                                      # the same bits on every run ...
            assert same_out(run_sliced(sg), got), f"{entry} {kw} ext={ext}: run {rep + 2} gives other bits"
        side = torch.cuda.Stream()                                                # ... and stream-ordered on another stream
        api.hip_set_stream(side.cuda_stream)
        out = sg.new_out() if ext else sg.new_c()
        torch.cuda.synchronize()
        sg.run(out)
        api.hip_sync(); api.check()
        api.hip_set_stream(None); api.hip_set_async(0)
        again = sg.result(out) if ext else (sg.C0.download(out[0]), None)
        assert same_out(again, got), f"{entry} {kw} ext={ext}: another stream gives other bits"


@pytest.mark.parametrize("c_type", [DT.F32, DT.F16], ids=["f32", "f16"])
def test_one_slice_per_block_is_bitwise_the_unsliced_call_for_every_beta_and_with_a_bias(c_type):
    """The start value comes last in both forms, so -- unlike every other class -- this holds under beta = 1 and with a bias, on random data."""
    api = capi.load()
    products = [0, 3, 64, 1, 2, 7, 19]
    for i, (entry, kw) in enumerate(SLICED_CASES):
        for beta in (0, 1):
            sg = make(api, entry, False, 70 + i, c_type=c_type, **dict(kw, beta=beta), slices=[1] * len(products), products=products)
            want = sg.new_c()
            sg.run_unsliced(want)
            api.hip_sync(); api.check()
            assert _same(sg.run_checked(), sg.C0.download(want[0])), f"{entry} {kw} beta={beta}: differs from the unsliced entry on the same lists"
            fs = make(api, "ext_" + entry, False, 80 + i, c_type=c_type, **dict(kw, beta=beta), slices=[1] * len(products), products=products)
            for colbias, act in ((True, 2), (False, 1), (True, 0)):
                fs.set_epilogue(colbias, act)
                want = fs.new_out()
                fs.run_unsliced(want)
                api.hip_sync(); api.check()
                assert same_out(fs.run_checked(), fs.result(want)), f"ext {entry} {kw} beta={beta} colbias={colbias} act={act}: differs from the unsliced ext entry"


def test_an_ext_block_without_slices_is_the_unsliced_segment_of_count_zero():
    api = capi.load()
    for c_type in (DT.F32, DT.F16):
        for beta in (0, 1):
            fs = make(api, "ext_sliced", False, 90, c_type=c_type, colbias=True, act=2, **dict(SHAPES[2], beta=beta), slices=[0, 1, 0, 2], products=[3, 0, 5])
            if c_type == DT.F32:
                _wide_c(fs, 91)
            got = fs.run_checked()
            seg = _up(np.zeros(fs.nblocks + 1, dtype=np.uint64))                  # the unsliced call with every count 0
            want = fs.new_out()
            fs.run_unsliced(want, seg=seg)
            api.hip_sync(); api.check()
            want = fs.result(want)
            for b in (0, 2):
                assert np.array_equal(fs.valid(got[0], b), fs.valid(want[0], b)) and np.array_equal(fs.mask_rows(got[1], b), fs.mask_rows(want[1], b)), (c_type, beta, b)
            st = sliced_statement(fs)                                             # (random data: only the blocks without partials are compared bit for bit)
            for b in (0, 2):
                assert np.array_equal(fs.valid(got[0], b).view(np.uint8), fs.valid(st[0], b).view(np.uint8)), f"block {b} without slices differs from the statement"


def _grid_stride(api, nblocks, m, n, c_type, beta, fused, seed):
    """`nblocks` blocks of ONE slice of one m x n x 4 f16 product on -1 / 0 / +1 (every value exact in a half), through the plain sliced entry or, `fused`, the ext
    one with bias + ReLU + bitmask; every block against a numpy integer sum; run twice: the same bits."""
    rng = np.random.default_rng(seed)
    npool, k, nb = 16, 4, 5
    ea, eb, ec, csz = m * k, k * n, m * n, capi.DT_SIZE[c_type]
    mask_ld = (m + 15) // 16 * 16
    mb = mask_ld // 8 * n
    blk_ptr = np.arange(nblocks + 1, dtype=np.uint64)
    ai, bi, di = rng.integers(0, npool, nblocks), rng.integers(0, npool, nblocks), rng.integers(0, nb, nblocks)
    A, B, C0, D = _exact(rng, npool * ea, DT.F16), _exact(rng, npool * eb, DT.F16), _exact(rng, nblocks * ec, c_type), _exact(rng, nb * m, c_type)
    M0 = rng.integers(0, 256, nblocks * mb).astype(np.uint8)
    dA, dB, dD = _up(A), _up(B), _up(D)
    seq = np.arange(nblocks, dtype=np.int64)
    d_blk = _up(blk_ptr)
    h = helpers.GemmCase(m, n, k, a_type=DT.F16, c_type=c_type, beta=beta, br_type=capi.BR_ADDRESS, br_count=1, colbias=fused, act=2 if fused else 0).dispatch(api)
    assert h
    query = api.hip_gemm_ext_batch_reduce_segments_sliced_workspace if fused else api.hip_gemm_batch_reduce_segments_sliced_workspace
    nbytes = query(h, nblocks)
    runs = []
    for _ in range(2):
        dC, dM = _up(C0.copy()), _up(M0.copy())
        lists = [_up((dA.data_ptr() + ai * ea * 2).astype(np.uint64)), _up((dB.data_ptr() + bi * eb * 2).astype(np.uint64)), _up((dC.data_ptr() + seq * (ec * csz)).astype(np.uint64))]
        ws = _up(np.zeros(nbytes, dtype=np.uint8))
        api.hip_launch_count(1)
        if fused:
            lists += [_up((dD.data_ptr() + di * (m * csz)).astype(np.uint64)), _up((dM.data_ptr() + seq * mb).astype(np.uint64))]
            api.hip_gemm_ext_batch_reduce_segments_sliced(h, C.byref(capi.GemmExtParam()), nblocks, d_blk.data_ptr(), nblocks, d_blk.data_ptr(), *[x.data_ptr() for x in lists],
                                                          ws.data_ptr(), nbytes)
        else:
            api.hip_gemm_batch_reduce_segments_sliced(h, C.byref(capi.GemmParam()), nblocks, d_blk.data_ptr(), nblocks, d_blk.data_ptr(), *[x.data_ptr() for x in lists],
                                                      ws.data_ptr(), nbytes)
        assert api.hip_launch_count(1) == 2
        api.hip_sync(); api.check()
        runs.append((np.ascontiguousarray(dC.cpu().numpy()).view(C0.dtype), np.ascontiguousarray(dM.cpu().numpy()).view(np.uint8)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "a second run gives other bits"
    got, gotm = widen(runs[0][0], c_type).reshape(nblocks, n, m), runs[0][1].reshape(nblocks, n, mask_ld // 8)
    ints = lambda x, t: widen(x, t).astype(np.int32)                              # noqa: E731
    Am, Bm = ints(A, DT.F16).reshape(npool, k, m), ints(B, DT.F16).reshape(npool, n, k)      # column-major blocks: as row-major arrays C^T = B^T A^T
    pre = np.einsum("bjk,aki->abji", Bm, Am).reshape(npool * npool, n, m)[ai * npool + bi]
    if fused:
        pre = pre + ints(D, c_type).reshape(nb, m)[di][:, None, :]
    if beta:
        pre = pre + ints(C0, c_type).reshape(nblocks, n, m)
    want = np.maximum(pre, 0) if fused else pre
    bad = np.flatnonzero((got.astype(np.float64) != want).any(axis=(1, 2)))
    assert bad.size == 0, f"{bad.size} of {nblocks} blocks differ from the numpy sum, first: block {bad[0]}"
    if fused:
        bits = np.unpackbits(M0.reshape(nblocks, n, mask_ld // 8), axis=2, bitorder="little")
        bits[:, :, :m] = pre > 0
        badm = np.flatnonzero((gotm != np.packbits(bits, axis=2, bitorder="little")).any(axis=(1, 2)))
        assert badm.size == 0, f"the masks of {badm.size} of {nblocks} blocks differ, first: block {badm[0]}"
    else:
        assert np.array_equal(gotm, M0.reshape(gotm.shape))


def test_the_second_pass_grid_strides():
    """A block of up to 16 x 16 is one run of pass 2, so its waves only grid-stride with more than 131 072 blocks (group_grid: 32 768 workgroups of four waves): the
    instances <5> (f16 C) and <6> (f32 C under beta = 1) of both pass-2 kernels in that regime, the fused ones in the run form (m % 8 == 0) and the byte form."""
    api = capi.load()
    _grid_stride(api, 131073, 4, 4, DT.F16, 1, False, 600)
    _grid_stride(api, 131073, 4, 4, DT.F32, 1, False, 601)
    _grid_stride(api, 131073, 16, 16, DT.F16, 1, True, 602)
    _grid_stride(api, 131073, 12, 16, DT.F32, 1, True, 603)


# ---- names, launches, modes -----------------------------------------------------------------------------------------------------------------------------------
NAMES = [("address", "NN", False, b"gemm_segments_f16_kernel"), ("ext_address", "NN", True, b"gemm_segments_f16_fused_kernel"),
         ("offset", "NN", False, b"gemm_segments_offs_f16_kernel<0,0>"), ("offset", "NT", False, b"gemm_segments_offs_f16_kernel<0,1>"),
         ("ext_offset", "NN", True, b"gemm_segments_offs_f16_fused_kernel<0,0>"), ("ext_offset", "NT", True, b"gemm_segments_offs_f16_fused_kernel<0,1>"),
         ("ext_offset", "NT", False, b"gemm_segments_offs_f16_kernel<0,1>"),                              # an ext handle without operators: the plain kernel
         ("sliced", "NN", False, b"gemm_segments_sliced_f16_kernel"), ("ext_sliced", "NN", True, b"gemm_segments_sliced_f16_kernel"),
         ("offset_sliced", "NN", False, b"gemm_segments_offs_sliced_f16_kernel<0,0>"), ("offset_sliced", "NT", False, b"gemm_segments_offs_sliced_f16_kernel<0,1>"),
         ("ext_offset_sliced", "NT", True, b"gemm_segments_offs_sliced_f16_kernel<0,1>")]


def test_kernel_names_and_launch_counts():
    api = capi.load()
    for entry, form, ops, name in NAMES:
        for c_type in (DT.F32, DT.F16):
            sg = make(api, entry, True, 100, m=40, n=24, k=20, c_type=c_type, form=form, beta=1, **(dict(colbias=ops, act=2 if ops else 0) if entry.startswith("ext_") else {}))
            out = sg.new_out() if entry.startswith("ext_") else sg.new_c()
            api.hip_launch_count(1)
            sg.run(out)
            assert api.hip_launch_count(1) == (2 if "sliced" in entry else 1), (entry, form, c_type)
            api.hip_sync(); api.check()
            handle = sg.ext_handle if entry in ("ext_address", "ext_offset") else sg.handle
            assert api.hip_kernel_name(handle, 1) == name, (entry, form, c_type, api.hip_kernel_name(handle, 1))


def test_modes_stream_pipeline_and_graph_keep_the_results():
    import torch
    api = capi.load()
    kw = dict(m=40, n=24, k=20, flags=V, beta=1)
    segs = [make(api, "address", False, 110, c_type=DT.F16, **kw), make(api, "ext_offset", False, 111, c_type=DT.F32, colbias=True, act=2, **kw),
            make(api, "ext_sliced", False, 112, c_type=DT.F16, colbias=True, act=2, **kw)]
    new = lambda sg: sg.new_out() if hasattr(sg, "new_out") else sg.new_c()       # noqa: E731
    res = lambda sg, o: sg.result(o) if hasattr(sg, "new_out") else (sg.C0.download(o[0]), None)      # noqa: E731
    want = []
    for sg in segs:                                                               # blocking
        o = new(sg); sg.run(o)
        api.hip_sync(); api.check()
        want.append(res(sg, o))
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)                   # stream-ordered on a torch stream
    outs = [new(sg) for sg in segs]
    for sg, o in zip(segs, outs):
        sg.run(o)
    api.hip_sync(); api.check()
    for sg, o, w in zip(segs, outs, want):
        assert same_out(res(sg, o), w), "stream-ordered"
    outs = [new(sg) for sg in segs]                                               # inside a pipeline section
    assert api.hip_pipeline_begin(4) == 0
    for sg, o in zip(segs, outs):
        sg.run(o)
    assert api.hip_pipeline_end() == 0
    api.hip_sync(); api.check()
    api.hip_set_async(0); api.hip_set_stream(None)
    for sg, o, w in zip(segs, outs, want):
        assert same_out(res(sg, o), w), "pipeline section"
    # a captured call, replayed after the operands were overwritten in place
    sg, fresh = make(api, "address", False, 113, c_type=DT.F16, **kw), make(api, "address", False, 114, c_type=DT.F16, **kw)
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
    for dev, pool in ((sg.dA, fresh.A), (sg.dB, fresh.B), (cset[0], fresh.C0)):
        for d, hst in zip(dev, pool.host):
            d.copy_(torch.from_numpy(hst.view(np.int16)))
    torch.cuda.synchronize()
    g.replay(); torch.cuda.synchronize()
    got = sg.C0.download(cset[0])
    sg.A, sg.B, sg.C0 = fresh.A, fresh.B, fresh.C0
    assert _same(got, sg.run_checked()), "the replay differs from a fresh call on the new operands"


def test_c_example_runs_a_block_sparse_f16_layer_with_bias_and_relu_in_one_call(tmp_path):
    libdir = os.path.join(ROOT, "libxsmm_amd", "lib")
    exe = str(tmp_path / "segments_f16_driver")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "segments_f16_driver.c"),
           "-L" + libdir, "-lxsmm_amd", "-lm", "-Wl,-rpath," + libdir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "normf_rel" in r.stdout and "1 launch" in r.stdout


GUARDED = "test_exact_data_is_bitwise or test_fused_exact_data or test_random_data_matches or test_sliced_exact_data"


def test_guarded_rerun_with_operands_flush_against_unmapped_memory():
    """The parity tests again with every upload flush against unmapped address space (tests/guard.py via tests/conftest.py): the pools, the last A, B, C, bias and
    mask block (arrays of their own), the lists and the workspace, which is exactly as large as the query says.  These are parity tests on valid inputs: an access
    outside an operand would fault the subprocess.  Why none is expected: the tile's address arithmetic is tile_bf16's, unchanged (gemm_group_tile.hpp: rows and
    columns clamped to m - 1 / n - 1, wide loads inside whole k steps, the ragged step element by element at min(k, K - 1)); the start-value loads that moved into
    acc_store read C under the predicates of the stores (i < m, j < n) and the bias at min(i, m - 1); pass 2 reads 16 bytes of a partial that is padded to 16
    and loads / stores four elements of C at once only when m, ldc and the pointer allow.  The second side only runs once the first has passed."""
    for side in ("end", "front"):
        env = dict(os.environ, LIBXSMM_TEST_GUARD=side)
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "-k", GUARDED, "-v", "--no-header"]
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
        print(f"guarded run ({side}): {time.time() - t0:.1f} s")
        assert r.returncode == 0, f"guarded run ({side}) ended with {r.returncode} (negative / 134: the GPU faulted on an out-of-bounds access):\n{tail}"
        assert "40 passed" in r.stdout, tail
