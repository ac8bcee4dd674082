"""libxsmm_hip_gemm_batch_grouped (include/libxsmm_hip.h): several strided (BR)GEMM batches of different shapes in one call equal the loop of
libxsmm_hip_gemm_batch_strided calls they replace.  f32 groups are bitwise the oracle's k-ordered fmaf chain, bf16 groups lie within the dense kernels'
tolerance and equal each group's own strided launch bit for bit on exact data; an eligible list of one precision is one launch; fallback groups (other
types, transposes, pointer-list batch-reduce, packed sparse) equal their own launches; the launch rule turns at its threshold for the entries and their
plans alike, the table computes the same in the kernel arguments and uploaded, and a captured call is refused; the table search and the grid hold at scale;
stream order and pipeline sections keep the results.  The last test re-runs the parity tests with every operand flush against unmapped memory (run this file with -x)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from helpers import GemmCase, TOL_BF16, normf_rel
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG
from sparse_helpers import random_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _up(x):
    """Device image of a host array: guarded (operand flush against unmapped memory) when the guard is on, as GemmCase.run_gpu uploads."""
    if helpers.UPLOAD_HOOK is not None:
        return helpers.UPLOAD_HOOK(x)
    import torch
    return torch.from_numpy(np.ascontiguousarray(x.view(np.int16) if x.dtype == np.uint16 else x)).to("cuda:0")


def _down(buf, like):
    return buf.cpu().numpy().view(like.dtype)


class Group:
    """One strided batch of a GemmCase on the device: its handle, its param struct (element 0) and the group entry for the grouped call."""

    def __init__(self, api, case, C0=None):
        self.case = case
        self.A, self.B = _up(case.A), _up(case.B)
        self.C0 = case.C0 if C0 is None else C0
        self.C = _up(self.C0.copy())
        self.addr = None
        if case.br_type == capi.BR_ADDRESS:
            self.addr = tuple(_up(x.view(np.int64)) for x in case.host_address_lists(self.A, self.B))
        self.handle = case.dispatch(api)
        assert self.handle
        self.param, self.keep = case.make_param(self.A, self.B, self.C, addr=self.addr)
        self.sa = case.nbr * 8 if case.br_type == capi.BR_ADDRESS else case.bs_a
        self.sb = case.nbr * 8 if case.br_type == capi.BR_ADDRESS else case.bs_b

    def entry(self):
        g = capi.GemmGroup()
        g.kernel, g.param, g.count = self.handle, self.param, self.case.batch
        g.stride_a, g.stride_b, g.stride_c = self.sa, self.sb, self.case.bs_c
        return g

    def result(self):
        return _down(self.C, self.C0)

    def run_own(self, api):
        """The group's own strided launch on a fresh copy of C."""
        Cown = _up(self.C0.copy())
        p, keep = self.case.make_param(self.A, self.B, Cown, addr=self.addr)
        api.hip_gemm_batch_strided(self.handle, C.byref(p), self.case.batch, self.sa, self.sb, self.case.bs_c)
        api.hip_sync(); api.check()
        return _down(Cown, self.C0)


def _grouped(api, entries):
    arr = (capi.GemmGroup * len(entries))(*entries)
    api.hip_gemm_batch_grouped(arr, len(entries))
    api.hip_sync(); api.check()


F32_CASES = [
    dict(m=32, n=32, k=32, batch=7, seed=1),                                   # whole 32-tiles
    dict(m=16, n=16, k=16, batch=9, seed=2),                                   # whole 16-tile
    dict(m=13, n=17, k=29, batch=5, seed=3),                                   # ragged (32-tile)
    dict(m=13, n=13, k=13, batch=4, seed=4),                                   # ragged (16-tile)
    dict(m=20, n=24, k=18, lda=23, ldb=21, ldc=29, batch=3, seed=5),           # padded leading dimensions
    dict(m=40, n=40, k=40, beta=1, batch=3, seed=6),                           # beta = 1, 2 x 2 tiles
    dict(m=24, n=48, k=32, br_type=capi.BR_STRIDE, br_count=3, batch=4, seed=7),    # STRIDE BRGEMM
    dict(m=16, n=16, k=16, shared_b=True, beta=1, batch=6, seed=8),            # shared B (stride 0)
    dict(m=64, n=64, k=64, batch=1, seed=9),                                   # count 1
    dict(m=9, n=5, k=3, batch=1, beta=1, seed=10),                             # count 1, tiny
]


def test_f32_mixed_list_is_bitwise_the_fma_chain():
    api = capi.load()
    groups = [Group(api, GemmCase(**kw)) for kw in F32_CASES]
    _grouped(api, [g.entry() for g in groups])
    for kw, g in zip(F32_CASES, groups):
        ref, _ = g.case.run_oracle(fma=True)
        got = g.result()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{kw}: differs from the k-ordered fmaf chain (or wrote outside m x n)"


BF16_CASES = [
    dict(m=32, n=32, k=32, a_type=DT.BF16, c_type=DT.F32, batch=5, seed=21),
    dict(m=16, n=16, k=16, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, batch=6, seed=22),
    dict(m=13, n=17, k=29, a_type=DT.BF16, c_type=DT.BF16, batch=3, seed=23),                          # ragged, flat A
    dict(m=48, n=48, k=48, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, beta=1, batch=3, seed=24),
    dict(m=24, n=40, k=34, a_type=DT.BF16, c_type=DT.F32, flags=GEMM_FLAG.VNNI_A, br_type=capi.BR_STRIDE, br_count=2,
         lda=27, ldb=37, ldc=30, batch=2, seed=25),                                                    # padded, BRGEMM, unaligned B columns
    dict(m=64, n=64, k=64, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, shared_b=True, batch=4, seed=26),
    dict(m=9, n=30, k=7, a_type=DT.BF16, c_type=DT.F32, beta=1, batch=1, seed=27),
]


def _exact_bf16(case, seed):
    """Small-integer operands: every partial sum is exact, so any summation order gives the same bits."""
    rng = np.random.default_rng(seed)
    ints = lambda n: rng.integers(-1, 2, n).astype(np.float32)
    case.A = helpers.f32_to_bf16_trunc(ints(case.A.size))
    case.B = helpers.f32_to_bf16_trunc(ints(case.B.size))
    case.C0 = helpers.f32_to_bf16_trunc(ints(case.C0.size)) if case.c_type == DT.BF16 else ints(case.C0.size)
    return case


def test_bf16_mixed_list_matches_the_oracle_and_the_own_launches():
    api = capi.load()
    groups = [Group(api, GemmCase(**kw)) for kw in BF16_CASES]
    _grouped(api, [g.entry() for g in groups])
    for kw, g in zip(BF16_CASES, groups):
        ref, _ = g.case.run_oracle()
        err = normf_rel(g.case.valid_region(ref), g.case.valid_region(g.result()), g.case.c_type)
        assert err < TOL_BF16, f"{kw}: normf_rel = {err}"
    exact = [Group(api, _exact_bf16(GemmCase(**kw), 100 + i)) for i, kw in enumerate(BF16_CASES)]
    _grouped(api, [g.entry() for g in exact])
    for kw, g in zip(BF16_CASES, exact):
        own = g.run_own(api)
        assert np.array_equal(g.result(), own), f"{kw}: differs from its own strided launch"


def test_an_eligible_list_of_one_precision_is_one_launch():
    api = capi.load()
    f32 = [Group(api, GemmCase(m, n, k, batch=b, seed=30 + i)) for i, (m, n, k, b) in
           enumerate([(8, 8, 8, 3), (13, 13, 13, 5), (16, 16, 16, 7), (23, 23, 23, 2), (32, 32, 32, 4), (17, 9, 31, 3), (40, 24, 16, 2), (5, 33, 12, 6)])]
    bf16 = [Group(api, GemmCase(m, m, m, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, batch=3, seed=50 + m)) for m in (16, 32, 48)]
    for groups in (f32, bf16):
        api.hip_launch_count(1)
        arr = (capi.GemmGroup * len(groups))(*[g.entry() for g in groups])
        api.hip_gemm_batch_grouped(arr, len(groups))
        assert api.hip_launch_count(1) == 1
        api.hip_sync(); api.check()
    for g in f32:
        ref, _ = g.case.run_oracle(fma=True)
        assert np.array_equal(g.result().view(np.uint32), ref.view(np.uint32))


def test_large_f32_tile32_groups_keep_their_own_kernel():
    """The launch rule: an f32 group on 32 x 32 tiles with 2048 work items or more leaves the grouped launch for its own kernel,
    small groups stay in it -- two launches here, each group still equal to what its path computes."""
    api = capi.load()
    small = [Group(api, GemmCase(m, m, m, batch=5, seed=40 + m)) for m in (13, 16)]
    big = Group(api, GemmCase(32, 32, 32, batch=2048, seed=45))
    api.hip_launch_count(1)
    _grouped(api, [small[0].entry(), big.entry(), small[1].entry()])
    assert api.hip_launch_count(1) == 2
    for g in small:
        ref, _ = g.case.run_oracle(fma=True)
        assert np.array_equal(g.result().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(big.result().view(np.uint32), big.run_own(api).view(np.uint32))


def _fused():
    """The ext-side helpers (their module imports this one, so they are looked up when a test runs)."""
    import test_gemm_grouped_fused_gpu as fused
    return fused


def _entry_then_plan(api, direct, planned, ext):
    """The entry on `direct` and a plan of the same list on `planned`: the launches of the entry, which the plan has to announce and to issue, and the plan's
    bits, which have to be the entry's."""
    fused = _fused()
    arr = ((capi.GemmExtGroup if ext else capi.GemmGroup) * len(direct))(*[g.entry() for g in direct])
    api.hip_launch_count(1)
    (api.hip_gemm_ext_batch_grouped if ext else api.hip_gemm_batch_grouped)(arr, len(direct))
    counted = api.hip_launch_count(1)
    api.hip_sync(); api.check()
    plan = fused._plan(api, planned, ext)
    assert api.hip_gemm_group_plan_launches(plan) == counted
    api.hip_launch_count(1)
    api.hip_gemm_group_plan_launch(plan)
    assert api.hip_launch_count(1) == counted
    api.hip_sync(); api.check()
    for i, (a, b) in enumerate(zip(direct, planned)):
        assert all(np.array_equal(x, y) for x, y in zip(fused._bits(a), fused._bits(b))), f"group {i}: the plan differs from the entry"
    api.hip_gemm_group_plan_destroy(plan); api.check()
    return counted


@pytest.mark.parametrize("n32,launches", [(2047, 1), (2048, 2)])
def test_the_f32_rule_turns_at_2048_items_for_the_entry_and_the_plan_alike(n32, launches):
    """Both sides of the launch rule's threshold (32^3: one item per problem): 2047 problems stay in the grouped launch, 2048 leave for their own kernel --
    and a plain plan of the same list issues the entry's launches and computes its bits."""
    api = capi.load()
    make = lambda: [Group(api, GemmCase(13, 13, 13, batch=5, seed=500)), Group(api, GemmCase(32, 32, 32, batch=n32, seed=501)),
                    Group(api, GemmCase(16, 16, 16, batch=5, seed=502))]
    direct, planned = make(), make()
    assert _entry_then_plan(api, direct, planned, False) == launches
    for i, g in enumerate(direct):
        if i == 1 and launches == 2:
            want = g.run_own(api)                                       # the group that left: bitwise its own strided launch
        else:
            want, _ = g.case.run_oracle(fma=True)
        assert np.array_equal(g.result().view(np.uint32), want.view(np.uint32)), f"group {i}"


@pytest.mark.parametrize("n48,launches", [(511, 1), (512, 2)])
def test_the_fused_f32_rule_turns_at_2048_items_for_the_entry_and_the_plan_alike(n48, launches):
    """The ext side: 48^3 is four 32-tiles with m and n multiples of 16, so 511 problems (2044 items) stay and 512 (2048 items) leave."""
    api = capi.load()
    fused = _fused()
    make = lambda: [fused.FusedGroup(api, GemmCase(13, 17, 29, colbias=True, act=1, batch=5, seed=510)),
                    fused.FusedGroup(api, GemmCase(48, 48, 48, colbias=True, act=1, batch=n48, seed=511)),
                    fused.FusedGroup(api, GemmCase(16, 16, 16, colbias=True, act=1, batch=5, seed=512))]
    direct, planned = make(), make()
    assert _entry_then_plan(api, direct, planned, True) == launches
    for i, g in enumerate(direct):
        if i == 1 and launches == 2:
            own, _ = g.run_own(api)
            assert np.array_equal(g.result().view(np.uint32), own.view(np.uint32)), "the group that left differs from its own ext strided launch"
        else:
            fused._assert_chain(g, f"group {i}")


INLINE_SHAPES = [(8, 8, 8), (13, 13, 13), (20, 12, 9), (32, 32, 32)]


@pytest.mark.parametrize("ngroups", [24, 25])
def test_plain_tables_at_and_past_the_inline_limit_are_one_launch_and_the_fma_chain(ngroups):
    """24 groups travel in the kernel arguments, 25 are uploaded: one launch and the same bits either way."""
    api = capi.load()
    groups = [Group(api, GemmCase(*INLINE_SHAPES[i % 4], batch=1 + i % 3, seed=600 + i)) for i in range(ngroups)]
    api.hip_launch_count(1)
    _grouped(api, [g.entry() for g in groups])
    assert api.hip_launch_count(1) == 1
    for i, g in enumerate(groups):
        ref, _ = g.case.run_oracle(fma=True)
        assert np.array_equal(g.result().view(np.uint32), ref.view(np.uint32)), f"group {i}"


@pytest.mark.parametrize("ngroups", [18, 19])
def test_fused_tables_at_and_past_the_inline_limit_are_one_launch_and_the_fma_chain(ngroups):
    """The fused limit: 18 groups (bias + ReLU + bitmask) in the kernel arguments, 19 uploaded; C and masks are the chain's either way."""
    api = capi.load()
    fused = _fused()
    groups = [fused.FusedGroup(api, GemmCase(*INLINE_SHAPES[i % 4], colbias=True, act=2, beta=(i // 4) % 2, batch=1 + i % 3, seed=700 + i), mask_seed=700 + i)
              for i in range(ngroups)]
    api.hip_launch_count(1)
    arr = (capi.GemmExtGroup * ngroups)(*[g.entry() for g in groups])
    api.hip_gemm_ext_batch_grouped(arr, ngroups)
    assert api.hip_launch_count(1) == 1
    api.hip_sync(); api.check()
    for i, g in enumerate(groups):
        fused._assert_chain(g, f"group {i}")


def test_the_plain_entry_under_capture_is_refused_and_leaves_the_graph_valid():
    """The group table of a call lives for the call only: under capture the plain entry sets -3, launches nothing and leaves the capture intact -- the plan
    of the same list, captured next to the refusal, replays to the chain's bits."""
    import torch
    api = capi.load()
    groups = [Group(api, GemmCase(13, 13, 13, batch=5, seed=800)), Group(api, GemmCase(16, 16, 16, batch=5, seed=801))]
    plan = _fused()._plan(api, groups, False)
    arr = (capi.GemmGroup * 2)(*[g.entry() for g in groups])
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        api.hip_set_stream(side.cuda_stream)
        api.hip_launch_count(1)
        graph.capture_begin()
        api.hip_gemm_batch_grouped(arr, 2)
        refused, msg, launched = api.hip_get_last_error(), api.hip_get_last_error_string(), api.hip_launch_count(0)
        api.hip_clear_last_error()
        api.hip_gemm_group_plan_launch(plan)
        graph.capture_end()
    api.check()
    torch.cuda.current_stream().wait_stream(side)
    api.hip_set_stream(None); api.hip_set_async(0)
    assert refused == -3 and b"one by one" in msg, (refused, msg)
    assert launched == 0
    torch.cuda.synchronize()
    for g in groups:                                                   # nothing ran during the capture
        assert np.array_equal(g.result().view(np.uint32), g.C0.view(np.uint32))
    graph.replay(); torch.cuda.synchronize()
    for i, g in enumerate(groups):
        ref, _ = g.case.run_oracle(fma=True)
        assert np.array_equal(g.result().view(np.uint32), ref.view(np.uint32)), f"group {i}"
    del graph
    api.hip_gemm_group_plan_destroy(plan); api.check()


def _csr_group(api, count=6, M=9, N=7, K=9, P=8, seed=61):
    """A packed CSR (A sparse) handle as a group: the values are shared (stride 0), B and C step per element."""
    import torch
    rng = np.random.default_rng(seed)
    rowptr, colidx = random_csr(rng, M, K, 0.3)
    vals = helpers.rand_values(rng, int(rowptr[-1]), DT.F32)
    B = helpers.rand_values(rng, count * K * N * P, DT.F32)
    C0 = helpers.rand_values(rng, count * M * N * P, DT.F32)
    h = api.create_packed_spgemm_csr(capi.gemm_shape(M, N, K, 0, N, N, DT.F32, DT.F32, DT.F32, DT.F32), 0, 0, P,
                                     rowptr.ctypes.data, colidx.ctypes.data, vals.ctypes.data)
    assert h
    dv, dB = torch.from_numpy(vals).to("cuda:0"), torch.from_numpy(B).to("cuda:0")
    sx, sc = K * N * P * 4, M * N * P * 4

    def entry(Cbuf):
        g = capi.GemmGroup()
        g.kernel, g.count, g.stride_a, g.stride_b, g.stride_c = h, count, 0, sx, sc
        g.param.a.primary, g.param.b.primary, g.param.c.primary = dv.data_ptr(), dB.data_ptr(), Cbuf.data_ptr()
        return g
    return h, C0, entry, (dv, dB)


def test_fallback_groups_equal_their_own_launches():
    import torch
    api = capi.load()
    cases = [dict(m=16, n=16, k=16, batch=5, seed=70),                                              # eligible
             dict(m=16, n=12, k=9, a_type=DT.F64, batch=4, seed=71),                                # f64
             dict(m=32, n=32, k=64, a_type=DT.I8, b_type=DT.I8, c_type=DT.I32, flags=GEMM_FLAG.VNNI_A, batch=3, seed=72),   # 8-bit
             dict(m=20, n=20, k=20, flags=GEMM_FLAG.TRANS_A, batch=3, seed=73),                     # f32 TRANS_A
             dict(m=32, n=32, k=32, br_type=capi.BR_ADDRESS, br_count=2, batch=3, seed=74),         # ADDRESS BRGEMM
             dict(m=23, n=23, k=23, batch=4, seed=75),                                              # eligible
             dict(m=32, n=16, k=16, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, batch=2, seed=76)]   # the only bf16 group
    groups = [Group(api, GemmCase(**kw)) for kw in cases]
    h, C0, entry, keep = _csr_group(api)
    dC, dOwn = torch.from_numpy(C0.copy()).to("cuda:0"), torch.from_numpy(C0.copy()).to("cuda:0")
    entries = [g.entry() for g in groups]
    entries.insert(3, entry(dC))
    _grouped(api, entries)
    for kw, g in zip(cases, groups):
        if kw.get("a_type", DT.F32) == DT.F32 and not kw.get("flags") and "br_type" not in kw:     # the two eligible f32 groups: the grouped kernel
            want, _ = g.case.run_oracle(fma=True)
        else:                                                                                    # fallback groups (and the only bf16 group): their own launch
            want = g.run_own(api)
        assert np.array_equal(g.result().view(np.uint8), want.view(np.uint8)), kw
    own = entry(dOwn)
    api.hip_gemm_batch_strided(h, C.byref(own.param), own.count, own.stride_a, own.stride_b, own.stride_c)
    api.hip_sync(); api.check()
    assert np.array_equal(dC.cpu().numpy().view(np.uint32), dOwn.cpu().numpy().view(np.uint32)), "packed CSR group"
    api.release_kernel(h)


def test_scale_ten_thousand_groups_of_one_problem():
    api = capi.load()
    shapes = [(8, 8, 8), (13, 13, 13), (20, 12, 9), (32, 32, 32)]
    per = 2500
    cases = [GemmCase(m, n, k, batch=per, seed=80 + i) for i, (m, n, k) in enumerate(shapes)]
    dev = []
    entries = []
    for case in cases:
        A, B, Cb = _up(case.A), _up(case.B), _up(case.C0.copy())
        h = case.dispatch(api)
        assert h
        dev.append((A, B, Cb))
        for e in range(per):
            p, _ = case.make_param(A, B, Cb, batch_index=e)
            g = capi.GemmGroup()
            g.kernel, g.param, g.count = h, p, 1
            entries.append(g)
    order = np.random.default_rng(89).permutation(len(entries))        # shapes interleaved: the search has to find every one
    _grouped(api, [entries[i] for i in order])
    for case, (_, _, Cb) in zip(cases, dev):
        ref, _ = case.run_oracle(fma=True)
        assert np.array_equal(_down(Cb, case.C0).view(np.uint32), ref.view(np.uint32)), (case.m, case.n, case.k)


def test_scale_a_million_problem_group_next_to_small_groups():
    """A 2^20-problem bf16 16^3 group (A and B shared, C steps: 2^20 items, the waves grid-stride) next to small groups in ONE grouped launch."""
    api = capi.load()
    big = 1 << 20
    case = _exact_bf16(GemmCase(16, 16, 16, a_type=DT.BF16, c_type=DT.F32, flags=GEMM_FLAG.VNNI_A, batch=1, seed=90), 190)
    one = Group(api, case)
    want = one.run_own(api)                                            # exact data: the own kernel's element is the reference bit for bit
    Cbig = _up(np.zeros(big * 256, dtype=np.float32))
    p, _ = case.make_param(one.A, one.B, Cbig)
    g = capi.GemmGroup()
    g.kernel, g.param, g.count, g.stride_a, g.stride_b, g.stride_c = one.handle, p, big, 0, 0, 1024
    small = [Group(api, GemmCase(**kw)) for kw in (dict(m=13, n=13, k=13, a_type=DT.BF16, c_type=DT.BF16, batch=5, seed=91),
                                                   dict(m=40, n=40, k=40, a_type=DT.BF16, c_type=DT.F32, flags=GEMM_FLAG.VNNI_A, batch=3, beta=1, seed=92))]
    api.hip_launch_count(1)
    _grouped(api, [small[0].entry(), g, small[1].entry()])
    assert api.hip_launch_count(1) == 1
    got = _down(Cbig, np.zeros(1, dtype=np.float32)).reshape(big, 256)
    assert np.array_equal(got.view(np.uint32), np.broadcast_to(want.view(np.uint32), (big, 256)))
    for s in small:
        ref, _ = s.case.run_oracle()
        assert normf_rel(s.case.valid_region(ref), s.case.valid_region(s.result()), s.case.c_type) < TOL_BF16


def test_stream_ordered_call_in_a_pipeline_section_equals_the_serial_launches():
    import torch
    api = capi.load()
    cases = [dict(m=32, n=32, k=32, batch=64, seed=100), dict(m=13, n=17, k=29, batch=33, seed=101), dict(m=40, n=40, k=40, batch=17, beta=1, seed=102),
             dict(m=32, n=32, k=32, a_type=DT.BF16, c_type=DT.BF16, flags=GEMM_FLAG.VNNI_A, batch=40, seed=103),
             dict(m=16, n=16, k=16, a_type=DT.BF16, c_type=DT.F32, batch=50, seed=104),
             dict(m=16, n=16, k=16, a_type=DT.F64, batch=9, seed=105)]
    groups = [Group(api, GemmCase(**kw)) for kw in cases]
    serial = [g.run_own(api) for g in groups]                         # blocking, one group after the other
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    assert api.hip_pipeline_begin(4) == 0
    arr = (capi.GemmGroup * len(groups))(*[g.entry() for g in groups])
    api.hip_gemm_batch_grouped(arr, len(groups))
    assert api.hip_pipeline_end() == 0
    api.hip_sync(); api.check()
    for kw, g, want in zip(cases, groups, serial):
        assert np.array_equal(g.result().view(np.uint8), want.view(np.uint8)), kw


def test_c_example_runs_three_shapes_as_one_grouped_call(tmp_path):
    libdir = os.path.join(ROOT, "libxsmm_amd", "lib")
    exe = str(tmp_path / "grouped_driver")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "grouped_driver.c"),
           "-L" + libdir, "-lxsmm_amd", "-lm", "-Wl,-rpath," + libdir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "normf_rel" in r.stdout


def test_parity_tests_with_operands_flush_against_unmapped_memory():
    """Tests 1 and 5 again, every operand flush against unmapped address space (tests/guard.py via tests/conftest.py): one access outside an operand
    faults the subprocess.  The second side only runs once the first has passed."""
    for side in ("end", "front"):
        env = dict(os.environ, LIBXSMM_TEST_GUARD=side)
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
               "-k", "f32_mixed_list or scale_", "-v", "--no-header"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
        tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
        assert r.returncode == 0, f"guarded run ({side}) ended with {r.returncode} (negative / 134: the GPU faulted on an out-of-bounds access):\n{tail}"
        assert "3 passed" in r.stdout, tail
