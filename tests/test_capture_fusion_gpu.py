"""Capture-time fusion: consecutive lean f32 strided-batch launches that are captured into a graph and are address-independent of each
other become ONE kernel node (gemm_f32_lean_multi_kernel, blockIdx.y = the launch).  By definition the result equals the same launches issued eagerly one
after the other, bit for bit; what was folded is read from libxsmm_hip_fused_launch_count."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libxsmm_amd import capi  # noqa: E402
from libxsmm_amd.capi import DT, GEMM_FLAG  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore_the_threads_launch_mode():
    api = capi.load()
    cap = api.hip_set_capture_fusion(1000)
    api.hip_set_capture_fusion(cap)
    yield
    api.hip_sync()
    api.hip_clear_last_error()
    api.hip_set_stream(None)
    api.hip_set_async(0)
    api.hip_set_streaming_hint(0)
    api.hip_set_capture_fusion(cap)


def fuse_cap(api):
    api.hip_set_capture_fusion(1000)
    return api.hip_set_capture_fusion(1000)


class Geometry:
    """f32 32 x 32 x 32 problems, `br` blocks per problem, leading dimensions lda / ldb / ldc; byte sizes of one launch's operands"""

    def __init__(self, api, form="NN", batch=5, lda=32, ldb=32, ldc=32, br=1):
        self.api, self.batch, self.br, self.ldc = api, batch, br, ldc
        self.blk_a, self.blk_b, self.blk_c = lda * 32 * 4, ldb * 32 * 4, ldc * 32 * 4
        self.sa, self.sb, self.sc = br * self.blk_a, br * self.blk_b, self.blk_c
        flags = GEMM_FLAG.BETA_0 | {"NN": 0, "TN": GEMM_FLAG.TRANS_A, "NT": GEMM_FLAG.TRANS_B, "TT": GEMM_FLAG.TRANS_A | GEMM_FLAG.TRANS_B}[form]
        shape = capi.gemm_shape(32, 32, 32, lda, ldb, ldc, DT.F32, DT.F32, DT.F32, DT.F32)
        self.handle = api.dispatch_brgemm(shape, flags, 0, capi.br_config(capi.BR_STRIDE, self.blk_a, self.blk_b, 0))
        assert self.handle
        self.bytes_a, self.bytes_b, self.bytes_c = batch * self.sa, batch * self.sb, batch * self.sc      # = the bounding intervals: the last element ends its range


GEOMETRIES = {"nn_b5": dict(form="NN", batch=5), "nn_b67_padded_br3": dict(form="NN", batch=67, lda=36, ldb=40, ldc=48, br=3),
              "tn_b5": dict(form="TN", batch=5), "nt_b67_padded_br3": dict(form="NT", batch=67, lda=36, ldb=40, ldc=48, br=3)}


class Arena:
    """One device buffer that the launches' operands are carved from (byte offsets), so that a test controls how their ranges lie to each other."""

    def __init__(self, nbytes, seed=1):
        import torch
        gen = torch.Generator(device="cuda").manual_seed(seed)
        self.buf = (torch.rand(nbytes // 4, device="cuda", generator=gen) - 0.5) * 0.4
        self.initial = self.buf.clone()
        self.top = 0

    def take(self, nbytes, align=256):
        off = (self.top + align - 1) // align * align
        self.top = off + nbytes
        assert self.top <= self.buf.numel() * 4
        return off

    def ptr(self, off):
        return self.buf.data_ptr() + off

    def view(self, off, nbytes):
        return self.buf[off // 4:(off + nbytes) // 4]

    def reset(self, image=None):
        self.buf.copy_(self.initial if image is None else image)


class Launch:
    def __init__(self, arena, geo, a, b, c, count=None, sa=None, sb=None, sc=None, br=None, handle=None):
        self.api, self.handle = geo.api, handle or geo.handle
        self.count = geo.batch if count is None else count
        self.sa, self.sb, self.sc = (geo.sa if sa is None else sa), (geo.sb if sb is None else sb), (geo.sc if sc is None else sc)
        self.brc = C.c_ulonglong(geo.br if br is None else br)
        self.p = capi.GemmParam()
        self.p.a.primary, self.p.b.primary, self.p.c.primary = arena.ptr(a), arena.ptr(b), arena.ptr(c)
        self.p.op.tertiary = C.addressof(self.brc)

    def __call__(self):
        self.api.hip_gemm_batch_strided(self.handle, C.byref(self.p), self.count, self.sa, self.sb, self.sc)


def disjoint_sets(arena, geo, n, slack=0):
    """n x (a, b, c) byte offsets, no two ranges overlapping"""
    return [(arena.take(geo.bytes_a + slack), arena.take(geo.bytes_b + slack), arena.take(geo.bytes_c + slack)) for _ in range(n)]


def eager(api, body):
    """the launches one after the other on torch's current stream; returns how many were folded (none, ever)"""
    import torch
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    api.hip_fused_launch_count(1)
    body()
    api.hip_sync(); api.check()
    torch.cuda.synchronize()
    return int(api.hip_fused_launch_count(1))


def captured(api, body):
    """the same body captured on a side stream; returns (graph, launches folded into a predecessor's node)"""
    import torch
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        api.hip_set_stream(side.cuda_stream)
        api.hip_fused_launch_count(1)
        g.capture_begin()
        body()
        g.capture_end()
        fused = int(api.hip_fused_launch_count(1))
    torch.cuda.current_stream().wait_stream(side)
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    api.check()
    return g, fused


def compare(api, arena, launches, want_fused, body=None):
    """eager vs captured on the same initial arena: equal bit for bit over the WHOLE arena (pad rows, gaps and inputs included); returns the eager image"""
    import torch
    body = body or (lambda: [l() for l in launches])
    arena.reset()
    assert eager(api, body) == 0
    want = arena.buf.clone()
    arena.reset()
    g, fused = captured(api, body)
    assert fused == want_fused, (fused, want_fused)
    assert torch.equal(arena.buf, arena.initial)               # capturing executes nothing
    g.replay()
    torch.cuda.synchronize(); api.check()
    assert torch.equal(arena.buf, want)
    return want, g


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_eight_disjoint_launches_become_one_node(geometry):
    import torch
    api = capi.load()
    geo = Geometry(api, **GEOMETRIES[geometry])
    arena = Arena(8 * (geo.bytes_a + geo.bytes_b + geo.bytes_c) + (1 << 16))
    sets = disjoint_sets(arena, geo, 8)
    launches = [Launch(arena, geo, a, b, c) for a, b, c in sets]
    want, g = compare(api, arena, launches, 7)
    assert not torch.equal(want, arena.initial)
    # the inputs change in place between replays: the node reads what is there when it runs
    second = arena.initial.clone()
    for a, b, _ in sets:
        second[a // 4:(a + geo.bytes_a) // 4] *= -1.5
        second[b // 4:(b + geo.bytes_b) // 4] += 0.125
    arena.reset(second)
    assert eager(api, lambda: [l() for l in launches]) == 0
    want2 = arena.buf.clone()
    assert not torch.equal(want2, want)
    for _ in range(2):
        arena.reset(second)
        g.replay()
        torch.cuda.synchronize(); api.check()
        assert torch.equal(arena.buf, want2)


@pytest.mark.parametrize("geometry", ["nn_b5", "nn_b67_padded_br3"])
def test_read_after_write_is_not_folded(geometry):
    """launch k + 1 reads C of launch k as its A (C's layout is A's when ldc = lda and br = 1; with padding the ranges still overlap, which is what counts)"""
    api = capi.load()
    geo = Geometry(api, **GEOMETRIES[geometry])
    n = 4
    arena = Arena(n * (geo.bytes_a + geo.bytes_b + geo.bytes_c) * 2 + (1 << 16))
    span = max(geo.bytes_a, geo.bytes_c)
    chain = [arena.take(span) for _ in range(n + 1)]
    bs = [arena.take(geo.bytes_b) for _ in range(n)]
    launches = [Launch(arena, geo, chain[i], bs[i], chain[i + 1]) for i in range(n)]
    compare(api, arena, launches, 0)


def test_write_after_write_is_not_folded_and_the_second_launch_wins():
    import torch
    api = capi.load()
    geo = Geometry(api, batch=5)
    arena = Arena(1 << 20)
    (a0, b0, c0), (a1, b1, c1) = disjoint_sets(arena, geo, 2)
    launches = [Launch(arena, geo, a0, b0, c0), Launch(arena, geo, a1, b1, c0)]
    want, _ = compare(api, arena, launches, 0)
    arena.reset()
    eager(api, launches[1])
    assert torch.equal(arena.buf, want)                        # what the second launch alone leaves


def test_write_after_read_is_not_folded():
    api = capi.load()
    geo = Geometry(api, batch=5)
    arena = Arena(1 << 20)
    (a0, b0, c0), (a1, b1, _) = disjoint_sets(arena, geo, 2)
    compare(api, arena, [Launch(arena, geo, a0, b0, c0), Launch(arena, geo, a1, b1, a0)], 0)      # overwrites the first launch's A
    compare(api, arena, [Launch(arena, geo, a0, b0, c0), Launch(arena, geo, a1, b1, b0)], 0)      # ... its B


@pytest.mark.parametrize("overlap,folded", [(0, 1), (16, 0), (4, 0)], ids=["touching", "four_elements", "one_element"])
def test_touching_ranges_fold_and_overlapping_ones_do_not(overlap, folded):
    """The second set's C begins at the byte where the first set's A ends: independent.  `overlap` bytes earlier it is not.  (One element, 4 bytes, also takes C off
    its 16-byte alignment and so off the kernels that can be folded; four elements keep the alignment, so there the predicate alone decides.)"""
    api = capi.load()
    geo = Geometry(api, batch=5)
    arena = Arena(1 << 20)
    a0 = arena.take(geo.bytes_a)
    c1 = a0 + geo.bytes_a - overlap
    arena.top = c1 + geo.bytes_c
    b0, c0, a1, b1 = (arena.take(geo.bytes_b), arena.take(geo.bytes_c), arena.take(geo.bytes_a), arena.take(geo.bytes_b))
    compare(api, arena, [Launch(arena, geo, a0, b0, c0), Launch(arena, geo, a1, b1, c1)], folded)


def test_shared_b_is_folded():
    api = capi.load()
    geo = Geometry(api, batch=67)
    arena = Arena(1 << 22)
    b = arena.take(geo.blk_b)
    sets = [(arena.take(geo.bytes_a), arena.take(geo.bytes_c)) for _ in range(4)]
    compare(api, arena, [Launch(arena, geo, a, b, c, sb=0) for a, c in sets], 3)


@pytest.mark.parametrize("what", ["handle", "count", "stride", "br_count"])
def test_a_different_launch_in_the_middle_breaks_the_run(what):
    api = capi.load()
    geo = Geometry(api, batch=5)
    other = Geometry(api, form="TN", batch=5)
    arena = Arena(1 << 21)
    sets = disjoint_sets(arena, geo, 5, slack=geo.bytes_a)      # room for twice the stride / two blocks per problem
    launches = [Launch(arena, geo, a, b, c) for a, b, c in sets]
    a, b, c = sets[2]
    launches[2] = {"handle": lambda: Launch(arena, geo, a, b, c, handle=other.handle),
                   "count": lambda: Launch(arena, geo, a, b, c, count=4),
                   "stride": lambda: Launch(arena, geo, a, b, c, sa=2 * geo.sa),
                   "br_count": lambda: Launch(arena, geo, a, b, c, br=2, sa=2 * geo.sa, sb=2 * geo.sb)}[what]()
    compare(api, arena, launches, 2)                            # {0, 1}, {2}, {3, 4}


def test_a_foreign_operation_between_two_launches_breaks_the_run():
    import torch
    api = capi.load()
    geo = Geometry(api, batch=5)
    arena = Arena(1 << 20)
    sets = disjoint_sets(arena, geo, 4)
    launches = [Launch(arena, geo, a, b, c) for a, b, c in sets]
    next_a = arena.view(sets[2][0], geo.bytes_a)

    def body():
        launches[0](); launches[1]()
        next_a.mul_(3.0)                                        # a torch kernel on the same stream rewrites the third launch's A
        launches[2](); launches[3]()
    want, _ = compare(api, arena, launches, 2, body)
    arena.reset()
    eager(api, lambda: [l() for l in launches])
    c2 = slice(sets[2][2] // 4, (sets[2][2] + geo.bytes_c) // 4)
    assert not torch.equal(arena.buf[c2], want[c2])             # its effect is seen


def test_an_event_between_two_fused_launches_completes_after_both():
    """A second captured stream waits on an event recorded after the first launch, copies that launch's C and joins again.  The second launch still folds into the
    first one's node (the event adds no node); the copy is ordered behind the node, so it sees the first launch's result; the launch after the join is not folded."""
    import torch
    api = capi.load()
    geo = Geometry(api, batch=5)
    arena = Arena(1 << 20)
    sets = disjoint_sets(arena, geo, 3)
    launches = [Launch(arena, geo, a, b, c) for a, b, c in sets]
    seen_off = arena.take(geo.bytes_c)
    seen, c0 = arena.view(seen_off, geo.bytes_c), arena.view(sets[0][2], geo.bytes_c)
    second = torch.cuda.Stream()

    def body():
        cur = torch.cuda.current_stream()
        launches[0]()
        ev = torch.cuda.Event()
        ev.record(cur)
        launches[1]()
        second.wait_event(ev)
        with torch.cuda.stream(second):
            seen.copy_(c0)
        cur.wait_stream(second)
        launches[2]()
    want, _ = compare(api, arena, launches, 1, body)
    assert torch.equal(want[seen_off // 4:(seen_off + geo.bytes_c) // 4], want[sets[0][2] // 4:(sets[0][2] + geo.bytes_c) // 4])


def test_more_launches_than_a_node_holds_give_two_nodes():
    api = capi.load()
    cap = fuse_cap(api)
    geo = Geometry(api, batch=5)
    n = cap + 3
    arena = Arena(n * (geo.bytes_a + geo.bytes_b + geo.bytes_c) + (1 << 16))
    launches = [Launch(arena, geo, a, b, c) for a, b, c in disjoint_sets(arena, geo, n)]
    compare(api, arena, launches, n - 2)
    assert api.hip_set_capture_fusion(3) == cap                 # a smaller limit: nodes of three
    compare(api, arena, launches, n - (n + 2) // 3)


def test_two_captures_in_a_row_do_not_share_state():
    import torch
    api = capi.load()
    geo = Geometry(api, batch=5)
    arena = Arena(1 << 21)
    sets = disjoint_sets(arena, geo, 6)
    launches = [Launch(arena, geo, a, b, c) for a, b, c in sets]
    arena.reset()
    eager(api, lambda: [l() for l in launches])
    want = arena.buf.clone()
    arena.reset()
    g1, fused1 = captured(api, lambda: [l() for l in launches[:3]])
    g2, fused2 = captured(api, lambda: [l() for l in launches[3:]])        # its first launch must not reach into the first graph's node
    assert (fused1, fused2) == (2, 2)
    g2.replay()
    torch.cuda.synchronize()
    first_c = slice(sets[0][2] // 4, (sets[0][2] + geo.bytes_c) // 4)
    assert not torch.equal(arena.buf[first_c], want[first_c])   # the first graph's launches have not run
    g1.replay()
    torch.cuda.synchronize(); api.check()
    assert torch.equal(arena.buf, want)
    arena.reset()
    g1.replay(); g2.replay()
    torch.cuda.synchronize(); api.check()
    assert torch.equal(arena.buf, want)


def test_fusion_off_eager_launches_and_pipeline_sections_fold_nothing():
    api = capi.load()
    cap = fuse_cap(api)
    geo = Geometry(api, batch=5)
    arena = Arena(1 << 21)
    launches = [Launch(arena, geo, a, b, c) for a, b, c in disjoint_sets(arena, geo, 6)]
    for off in (0, 1):
        assert api.hip_set_capture_fusion(off) in (cap, 0)
        compare(api, arena, launches, 0)                        # compare() also asserts that the eager launches fold nothing
    assert api.hip_set_capture_fusion(cap) == 0
    compare(api, arena, launches, 5)

    def body():
        assert api.hip_pipeline_begin(2) == 0
        for l in launches:
            l()
        assert api.hip_pipeline_end() == 0
    import torch
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    assert api.hip_pipeline_begin(2) == 0 and api.hip_pipeline_end() == 0      # the lanes are created outside the capture
    compare(api, arena, launches, 0, body)


def test_the_headline_shape():
    """bench.py's headline: 4096 problems per launch, a rotation over 12 input sets, 24 launches; launch k and launch k + 12 write the same C."""
    import torch
    import bench
    api = capi.load()
    cap = fuse_cap(api)
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    w = bench.Workload(api, torch.device("cuda:0"), "f32", 32, 4096, nsets=12)
    assert w.hint == 2
    api.hip_set_streaming_hint(w.hint)
    nodes = []                                                  # what the rules give: a launch joins the last node unless that is full or holds the launch's own set
    for i in range(24):
        if nodes and len(nodes[-1]) < cap and i % 12 not in nodes[-1]:
            nodes[-1].append(i % 12)
        else:
            nodes.append([i % 12])
    g, fused = captured(api, lambda: [w.step(i) for i in range(24)])
    assert fused == 24 - len(nodes) and fused >= 20
    for c in w.C:
        c.fill_(7.0)
    g.replay()
    torch.cuda.synchronize(); api.check()
    got = [c.clone() for c in w.C]
    for s in (0, 5, 11):
        ok, err, _ = w.verify(s)
        assert ok, (s, err)
    for c in w.C:
        c.fill_(7.0)
    assert eager(api, lambda: [w.step(i) for i in range(24)]) == 0
    for s in range(12):
        assert torch.equal(w.C[s], got[s]), s
