"""Block-sparse (BCSC) GEMM, every kernel plan_bcsc can pick and launch_bcsc then launches, held per element against a float64 restatement (tests/bcsc_parity_helpers.py).

BCSC is a table of (expected kernel name, case) rows.  The name of every row is derived from the conditions of plan_bcsc / run_bcsc (csrc/bcsc_plan.hpp,
csrc/runtime.cpp) and says in its comment which one it exercises (tests/test_bcsc_plan_cpu.py holds the plan alone to the same names, without a GPU); the test
asserts libxsmm_hip_kernel_name, every element of every M-block against
gemm_ld_helpers.bound64, and every margin around A, B's values and C bit for bit.  Data: bcsc_parity_helpers.wide (17 binades, full significands, exact zeros),
full-range bytes for the integer kernels; every M-block has its own A.  Patterns carry a block column with every k-block, one with none and one stored in
descending order (edge_columns), written out where a row needs a particular size of B.

The conditions, as plan_bcsc states them (nbl = 64 / bn n-blocks per wave, nkb = K / bk, tiles = ceil(M / 64) ceil(N / 64)):
  matrix cores   bf16: VNNI-2 A, bk % 32 == 0;  f32: bk % 16 == 0;  i8: VNNI-4 A, bk % 32 == 0;  all: bn in {16, 32, 64}, M % 16 == 0, nbl nkb <= 1024,
                 A % 4 == 0, values of B % 16 == 0 (i8: % 8), C % 16 == 0 -- else bcsc_generic_kernel
  LDS-DMA        nbl nkb <= 256 and A % 16 == 0 -- else the register kernels (bcsc_mfma_bf16_kernel / _i8_kernel; f32 has no dma kernel: bcsc_mfma_f32_kernel)
  streaming      beta = 0, nkb <= 64, mb tiles >= 4096 (f32: also A % 16 == 0 and nbl nkb <= 256)
  full           a pattern whose block count the host knows (host-resident or bound), B's values <= 10 KiB (f32: 16 KiB, i8: 8 KiB and values % 16 == 0), whole
                 64 x 64 tiles, bf16 C for bf16 operands; i8: beta = 0 and mb tiles >= 4096 (i8 has no general streaming kernel)

The last part pins the five bf16 store paths of these kernels bit for bit, as tests/test_bf16_store_exact_gpu.py does for dense GEMM."""
import numpy as np
import pytest

from bcsc_parity_helpers import BcscCase, assert_bcsc, run_gpu
from helpers import bf16_to_f32
from libxsmm_amd.capi import DT
from segments_sliced_helpers import f32_to_bf16
from test_bf16_store_exact_gpu import SPECIAL

pytestmark = pytest.mark.gpu

UNREACHABLE = {}            # kernel name -> why no row can reach it (tests/test_bcsc_parity_cpu.py holds BCSC and this against the kernel names in the source)

BF, F32 = DT.BF16, DT.F32
# the smallest M-block counts that stream, with a remainder so that waves get different numbers of M-blocks
MB1, MB2, MB4 = 4099, 2051, 1027           # at one, two and four 64 x 64 tiles per M-block
EDGE4 = [[0, 1, 2, 3], [], [3, 0], [1, 2]]  # four block columns over four k-blocks: full, empty, descending with the first and the last k-block, inner (8 blocks)


def bf(**kw):
    return dict(a_type=BF, **kw)


def f32(**kw):
    return dict(a_type=F32, **kw)


def i8(**kw):
    """Both signedness combinations of one row."""
    return [dict(a_type=DT.U8, **kw), dict(a_type=DT.I8, **kw)]


BCSC = [
    # ---- bf16 ---------------------------------------------------------------------------------------------------------------------------------------------------------
    # the generic kernel: whatever the matrix-core path refuses
    ("bcsc_generic_kernel", bf(vnni=False, M=32, N=48, K=64)),                                             # flat A (the matrix-core kernels read VNNI-2)
    ("bcsc_generic_kernel", bf(bk=16, M=32, N=48, K=64, c_type=F32, beta=1)),                              # bk % 32 != 0
    ("bcsc_generic_kernel", bf(bn=4, M=32, N=12, K=64, beta=1)),                                           # bn not in {16, 32, 64}
    ("bcsc_generic_kernel", bf(M=20, N=48, K=64, c_type=F32)),                                             # M % 16 != 0 (M = 20: one ragged 64-row tile)
    ("bcsc_generic_kernel", bf(M=80, N=48, K=64, skew_c=8, beta=1)),                                       # C % 16 != 0: the matrix-core kernels store 16-byte pieces
    ("bcsc_generic_kernel", bf(M=32, N=48, K=64, skew_a=2, c_type=F32, beta=1)),                           # A % 4 != 0: the register kernel reads VNNI dwords
    ("bcsc_generic_kernel", bf(M=32, N=48, K=64, skew_b=8)),                                               # values of B % 16 != 0: the matrix-core kernels read 16-byte fragments
    ("bcsc_generic_kernel", bf(bk=16, M=32, N=48, K=64, nnz0=True, beta=1)),                               # ... without any block: C keeps its start values
    # the register kernel: A off 16 bytes (no LDS-DMA), or more table entries than the dma kernel's LDS table holds
    ("bcsc_mfma_bf16_kernel", bf(M=80, N=96, K=96, bn=32, mb=3, skew_a=4, beta=1)),                        # A % 16 == 4, ragged i- and n-tiles
    ("bcsc_mfma_bf16_kernel", bf(mb=MB1, skew_a=4, cols=EDGE4)),                                           # the same skew at a streaming size: must not stream (the ring is fed by 16-byte DMA)
    ("bcsc_mfma_bf16_kernel", bf(M=16, N=64, K=257 * 32, bn=64, mb=2, c_type=F32, cols=[[256, 130, 64, 63, 0]])),     # nbl nkb = 257 > 256; five k-groups of 64
    ("bcsc_mfma_bf16_kernel", bf(M=16, N=64, K=65 * 32, bn=16, mb=2, c_type=F32, cols=[[0, 64], [], [64, 33, 0], [5]])),   # nbl nkb = 4 * 65 = 260 > 256
    ("bcsc_mfma_bf16_kernel", bf(M=16, N=64, K=65 * 32, bn=16, mb=2, nnz0=True, pattern_on="host")),       # ... without any block: zeros
    # the LDS-DMA kernel: one tile per wave, few M-blocks, or beta = 1
    ("bcsc_mfma_bf16_dma_kernel", bf(M=16, N=80, bn=16, bk=32, mb=5)),                                     # short last n-tile (16 of 64 columns), one 16-row tile
    ("bcsc_mfma_bf16_dma_kernel", bf(M=48, N=96, bn=32, bk=64, mb=3, beta=1, c_type=F32, pattern_on="host", hint=2)),
    ("bcsc_mfma_bf16_dma_kernel", bf(M=80, N=128, bn=64, bk=32, mb=2, beta=1, hint=2)),                    # whole and ragged i-tiles: C through LDS and direct
    ("bcsc_mfma_bf16_dma_kernel", bf(M=64, N=64, bn=16, bk=64, mb=7, pattern_on="host")),                  # whole tiles: the through-LDS store
    ("bcsc_mfma_bf16_dma_kernel", bf(M=64, N=64, bn=32, bk=32, mb=4, c_type=F32)),
    ("bcsc_mfma_bf16_dma_kernel", bf(M=32, N=64, K=256, bn=32, bk=128, mb=3, beta=1)),                     # four 32-deep steps per k-block
    ("bcsc_mfma_bf16_dma_kernel", bf(M=64, N=64, bn=16, bk=32, mb=MB1, beta=1, cols=EDGE4)),               # a streaming size with beta = 1: the streaming kernels never read C
    ("bcsc_mfma_bf16_dma_kernel", bf(M=16, N=64, K=65 * 32, bn=64, mb=2, c_type=F32, cols=[[64, 63, 1, 0]])),      # two k-groups (nkb = 65 <= 256 entries)
    ("bcsc_mfma_bf16_dma_kernel", bf(M=48, N=64, bn=16, mb=2, nnz0=True, pattern_on="host")),
    # waves streaming over M-blocks, general form
    ("bcsc_mfma_bf16_stream_kernel", bf(mb=MB1, cols=EDGE4)),                                              # device pattern: the block count is unknown, B stays in global memory
    ("bcsc_mfma_bf16_stream_kernel", bf(M=128, N=128, bn=32, mb=MB4, c_type=F32, hint=2)),                 # ... non-temporal A, four tiles, f32 C
    ("bcsc_mfma_bf16_stream_kernel", bf(bk=64, mb=MB1, pattern_on="host", cols=[[0, 1], [], [1, 0], [0, 1]])),     # host pattern, B = 6 blocks of 2 KiB > 10 KiB
    ("bcsc_mfma_bf16_stream_kernel", bf(M=80, N=96, K=96, bn=32, mb=MB4, pattern_on="host", cols=[[0, 1, 2], [], [2, 0]])),   # B = 10 KiB in LDS, ragged tiles: both epilogues
    ("bcsc_mfma_bf16_stream_kernel", bf(mb=MB1, pattern_on="host", c_type=F32, hint=2, cols=EDGE4)),       # B in LDS, whole tiles, f32 C
    ("bcsc_mfma_bf16_stream_kernel", bf(K=64, mb=MB1, pattern_on="host", nnz0=True)),                      # no block at all: every M-block becomes zero
    # ... whole tiles, bf16 C, B in LDS: one record per chunk
    ("bcsc_mfma_bf16_stream_full_kernel", bf(mb=MB1, pattern_on="host", cols=EDGE4)),                      # one n-tile (the first chunks requested from the host's k-block mask), bn = 16
    ("bcsc_mfma_bf16_stream_full_kernel", bf(N=128, bn=32, mb=MB2, pattern_on="host", hint=2, cols=[[3, 2, 1, 0], [], [], []])),     # two n-tiles, the second without blocks
    ("bcsc_mfma_bf16_stream_full_kernel", bf(N=128, K=64, bn=64, mb=MB2, pattern_on="host", cols=[[1, 0], []])),                   # bn = 64, B = 2 blocks of 4 KiB
    ("bcsc_mfma_bf16_stream_full_kernel", bf(N=128, bn=16, mb=MB2, pattern_on="host", cols=[[0, 1, 2, 3], [], [3, 0], [1], [2], [], [0], [3]])),   # B = 10 KiB exactly
    ("bcsc_mfma_bf16_stream_full_kernel", bf(K=192, bk=96, mb=MB1, pattern_on="host", cols=[[1, 0], [], [0], []])),          # three steps per k-block: chunk records of a step count that is no power of two
    ("bcsc_mfma_bf16_stream_full_kernel", bf(M=128, bk=64, mb=MB2, pattern_on="bound", hint=2, cols=[[0, 1], [], [1, 0], [1]])),     # a bound device pattern, two steps per k-block
    # ---- f32 ----------------------------------------------------------------------------------------------------------------------------------------------------------
    ("bcsc_generic_kernel", f32(M=16, N=48, K=40, bk=8, bn=16, beta=1)),                                   # bk % 16 != 0
    ("bcsc_generic_kernel", f32(M=16, N=24, K=64, bk=16, bn=8)),                                           # bn = 8
    ("bcsc_generic_kernel", f32(M=32, N=48, K=64, bk=16, bn=16, skew_c=8, beta=1)),                        # C % 16 != 0: the matrix-core kernels load and store 16 bytes of a column
    ("bcsc_generic_kernel", f32(M=32, N=48, K=64, bk=16, bn=16, skew_b=8)),                                # values of B % 16 != 0
    ("bcsc_mfma_f32_kernel", f32(M=48, N=80, K=64, bk=16, bn=16, mb=3)),                                   # few M-blocks, ragged tiles
    ("bcsc_mfma_f32_kernel", f32(M=64, N=64, K=64, bk=32, bn=32, mb=5, beta=1, pattern_on="host", hint=2)),         # non-temporal loads of A
    ("bcsc_mfma_f32_kernel", f32(M=64, N=64, K=64, bk=16, bn=16, mb=MB1, skew_a=4, cols=EDGE4)),           # A % 16 == 4 at a streaming size: must not stream
    ("bcsc_mfma_f32_kernel", f32(M=32, N=64, K=64, bk=16, bn=64, mb=2, nnz0=True)),
    ("bcsc_mfma_f32_stream_kernel", f32(M=64, N=64, K=64, bk=16, bn=16, mb=MB1, cols=EDGE4)),              # device pattern
    ("bcsc_mfma_f32_stream_kernel", f32(M=80, N=96, K=96, bk=48, bn=32, mb=MB4, pattern_on="host", hint=2)),      # ragged tiles keep a host pattern off the full kernel
    ("bcsc_mfma_f32_stream_full_kernel", f32(M=64, N=64, K=64, bk=16, bn=16, mb=MB1, pattern_on="host", cols=EDGE4)),
    ("bcsc_mfma_f32_stream_full_kernel", f32(M=64, N=64, K=64, bk=16, bn=64, mb=MB1, pattern_on="host", hint=2, cols=[[3, 2, 1, 0]])),    # B = 16 KiB exactly
    ("bcsc_mfma_f32_stream_full_kernel", f32(M=64, N=128, K=96, bk=48, bn=32, mb=MB2, pattern_on="host", cols=[[1], [], [0], []])),      # bk = 48: three steps per k-block, B = 2 blocks of 6 KiB
]
for _kernel, _rows in [
    # ---- 8-bit integers, exact ----------------------------------------------------------------------------------------------------------------------------------------
    ("bcsc_generic_kernel", i8(M=16, N=24, K=40, bk=8, bn=8, beta=1)),                                     # bk % 32 != 0
    ("bcsc_generic_kernel", i8(M=32, N=48, K=64, skew_b=4)),                                               # values of B % 8 != 0: the matrix-core kernels read 8 bytes
    ("bcsc_mfma_i8_kernel", i8(M=80, N=96, K=96, bn=32, mb=3, skew_a=4, beta=1, hint=2)),                  # A % 16 == 4; non-temporal loads of A
    ("bcsc_mfma_i8_kernel", i8(M=16, N=64, K=65 * 32, bn=16, mb=2, cols=[[0, 64], [], [64, 33, 0], [5]])),    # 260 table entries
    ("bcsc_mfma_i8_dma_kernel", i8(M=48, N=80, bn=16, mb=3)),
    ("bcsc_mfma_i8_dma_kernel", i8(M=64, N=128, bn=64, bk=64, mb=2, beta=1, pattern_on="host", hint=2)),
    ("bcsc_mfma_i8_dma_kernel", i8(mb=MB1, pattern_on="host", skew_b=8, cols=EDGE4)),                      # values of B % 16 == 8 at a streaming size: must not take the full kernel
    ("bcsc_mfma_i8_dma_kernel", i8(M=16, N=64, K=65 * 32, bn=64, mb=2, cols=[[64, 63, 1, 0]])),            # two k-groups
    ("bcsc_mfma_i8_dma_kernel", i8(M=64, N=64, bn=32, mb=2, nnz0=True, pattern_on="host")),
    ("bcsc_mfma_i8_stream_full_kernel", i8(mb=MB1, pattern_on="host", cols=EDGE4)),
    ("bcsc_mfma_i8_stream_full_kernel", i8(N=128, bn=32, mb=MB2, pattern_on="host", hint=2, cols=[[3, 2, 1, 0], [], [], [2]])),
]:
    BCSC += [(_kernel, _kw) for _kw in _rows]


def _id(row):
    kernel, kw = row
    names = {DT.BF16: "bf16", DT.F32: "f32", DT.U8: "u8", DT.I8: "i8"}
    parts = [f"{k}{names.get(v, v) if k.endswith('type') else ('x' if k == 'cols' else v)}" for k, v in kw.items()]
    return kernel.replace("bcsc_", "").replace("_kernel", "") + "-" + "-".join(parts)


def run_row(kernel, kw):
    case = BcscCase(**kw)
    got, margins, name = run_gpu(case)
    stats = {"ratio": None}
    assert name == kernel, f"expected {kernel}, library picked {name}"
    assert_bcsc(case, got, margins, stats)
    return name, stats


@pytest.mark.parametrize("row", BCSC, ids=_id)
def test_bcsc_kernels_per_element(row):
    kernel, kw = row
    name, stats = run_row(kernel, kw)
    print(f"BCSC_STAT {name} {stats}")


# ---- bf16 stores, bit for bit (SPECIAL: denormals of both signs, the smallest normals, infinities, zeros) -------------------------------------------------------------

# one case per bf16 store path that can take beta = 1: f2bf_rne (generic), cvt2 of the register kernel, cvt2 of the dma kernel (direct and through LDS)
START = [
    ("bcsc_generic_kernel", bf(M=32, N=12, K=64, bn=4, beta=1, cols=[[0, 1], [], [1]])),
    ("bcsc_mfma_bf16_kernel", bf(M=80, N=96, K=96, bn=32, mb=3, skew_a=4, beta=1)),
    ("bcsc_mfma_bf16_dma_kernel", bf(M=80, N=80, bn=16, mb=3, beta=1)),
]


@pytest.mark.parametrize("row", START, ids=_id)
def test_start_values_in_the_denormal_range_leave_as_the_reference_converts_them(row):
    """beta = 1, A all +0 and B positive: every product is +0, so C is its start value plus +0 -- the conversion of the start value (a column without blocks: the
    start value itself).  Bitwise against the oracle and against segments_sliced_helpers.f32_to_bf16."""
    kernel, kw = row
    case = BcscCase(data="zeros", **kw)
    rng = np.random.default_rng(71)
    case.bvals[:] = np.array([0x3f80, 0x4000, 0x3e80, 0x1c80], dtype=np.uint16)[rng.integers(0, 4, case.bvals.size)]
    case.C0[:] = SPECIAL[rng.integers(0, len(SPECIAL), case.C0.size)]
    case.repack()
    got, margins, name = run_gpu(case)
    assert name == kernel
    ref = case.run_oracle()
    start = bf16_to_f32(case.C0).reshape(case.mb, case.N, case.M)
    want = f32_to_bf16(np.where(case.has_block()[None, :, None], start + np.float32(0.0), start)).reshape(-1)
    assert np.array_equal(ref, want), (int(np.sum(ref != want)), [hex(int(x)) for x in ref[ref != want][:8]], [hex(int(x)) for x in want[ref != want][:8]])
    assert np.array_equal(got, ref), (name, int(np.sum(got != ref)), [hex(int(x)) for x in got[got != ref][:8]], [hex(int(x)) for x in ref[got != ref][:8]])
    for m in margins.values():
        assert np.array_equal(m[0], m[2]) and np.array_equal(m[1], m[3])


# every kernel that stores bf16 C; block columns of 1, 2 and 4 stored blocks of 32 k
K128 = dict(K=128, bk=32)
SUMS = [
    ("bcsc_generic_kernel", bf(M=32, N=12, bn=4, cols=[[2], [3, 0], [0, 1, 2, 3]], **K128)),
    ("bcsc_mfma_bf16_kernel", bf(M=80, N=64, bn=16, mb=3, skew_a=4, cols=[[1], [0, 3], [3, 2, 1, 0], [2, 1]], **K128)),
    ("bcsc_mfma_bf16_dma_kernel", bf(M=80, N=80, bn=16, mb=3, cols=[[1], [0, 3], [3, 2, 1, 0], [2, 1], [0]], **K128)),           # direct store and through LDS
    ("bcsc_mfma_bf16_stream_kernel", bf(M=80, N=64, bn=16, mb=MB2, cols=[[1], [0, 3], [3, 2, 1, 0], [2, 1]], **K128)),           # ragged tile: direct; whole tile: through LDS
    ("bcsc_mfma_bf16_stream_kernel", bf(M=80, N=64, bn=16, mb=MB2, pattern_on="host", cols=[[1], [0, 3], [3, 2, 1, 0], [2, 1]], **K128)),   # ... with B in LDS
    ("bcsc_mfma_bf16_stream_full_kernel", bf(M=64, N=64, bn=16, mb=MB1, pattern_on="host", cols=[[1], [0, 3], [3, 2, 1, 0], [2, 1]], **K128)),
]


@pytest.mark.parametrize("row", SUMS, ids=_id)
def test_sums_in_the_f32_denormal_range_are_flushed_like_the_reference_flushes_them(row):
    """beta = 0, A = 2^-70 everywhere, every column of B one of 2^-63, 2^-60, 0, -2^-63 over 32, 64 or 128 stored k: every product of a column is the same power of
    two, the sum is exact in any order; k 2^-133 is an f32 denormal for k <= 64 (flushed to a signed zero), k 2^-130 and 128 * 2^-133 are normal (they survive).
    Every M-block computes the same [N][M] image: the oracle runs on two of them, every M-block of the result must equal it."""
    kernel, kw = row
    case = BcscCase(data="zeros", **kw)
    codes = np.array([0x2000, 0x2180, 0x0000, 0xa000], dtype=np.uint16)
    col = codes[(np.arange(case.N) + np.arange(case.N) // case.bn) % 4]                                         # the value of column n: every code in every block column
    nb_of = np.repeat(np.arange(case.N // case.bn), np.diff(case.colptr.astype(np.int64)))                       # block -> block column
    case.bvals[:] = np.repeat(col.reshape(-1, case.bn)[nb_of].reshape(-1), case.bk)
    case.A[:] = 0x1c80
    case.repack()
    got, margins, name = run_gpu(case)
    assert name == kernel
    image = case.run_oracle(blocks=slice(0, 2)).reshape(2, -1)
    assert np.array_equal(image[0], image[1])
    stored_k = np.repeat(np.diff(case.colptr.astype(np.int64)), case.bn) * case.bk
    sums = (stored_k * bf16_to_f32(col).astype(np.float64) * 2.0 ** -70).astype(np.float32)                     # exact: a small integer times a power of two
    want = np.repeat(f32_to_bf16(sums), case.M)
    assert np.array_equal(image[0], want), (int(np.sum(image[0] != want)),)
    flushed = (np.abs(sums) > 0) & (np.abs(sums) < 2.0 ** -126)
    assert flushed.any() and np.all(f32_to_bf16(sums)[flushed] & 0x7fff == 0) and np.any(f32_to_bf16(sums) & 0x7fff != 0)     # both kinds occur
    g = got.reshape(case.mb, -1)
    bad = g != image[0][None, :]
    assert not bad.any(), (name, int(bad.sum()), [int(x) for x in np.argwhere(bad)[0]], [hex(int(x)) for x in g[bad][:8]], [hex(int(x)) for x in np.broadcast_to(image[0], g.shape)[bad][:8]])
    for m in margins.values():
        assert np.array_equal(m[0], m[2]) and np.array_equal(m[1], m[3])
