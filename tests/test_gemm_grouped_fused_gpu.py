"""libxsmm_hip_gemm_ext_batch_grouped and the group plans (include/libxsmm_hip.h) on the device: a list of strided ext (BR)GEMM batches of different shapes,
each with its bias / ReLU (+ bitmask) / sigmoid, equals the loop of libxsmm_hip_gemm_ext_batch_strided calls it replaces.  f32 groups are bitwise the
k-ordered fmaf chain started at the bias, masks included, and leave every mask bit outside m x n and every byte of C's padding alone; bf16 groups are bitwise
the ext oracle and their own launches on exact data and within the dense kernels' tolerance on random data; a fused class is one launch; the table beyond
the inline limit and a resident plan (launched, captured, replayed on new operand values) compute the same.  The last test re-runs the parity tests with every
operand, bias and mask flush against unmapped memory (run this file with -x)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import grouped_fused_helpers as gf
import helpers
from helpers import GemmCase, TOL_BF16, TOL_F32, normf_rel
from libxsmm_amd import capi
from libxsmm_amd.capi import DT
from test_gemm_grouped_gpu import BF16_CASES, F32_CASES, Group, _down, _up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


class FusedGroup(Group):
    """A Group through an ext handle: bias and (prefilled) mask blocks on the device next to A, B and C, and the entry for the ext grouped call.
    shared_bias: stride_d = 0 (the case's host bias repeats element 0's, gf.share_bias)."""

    def __init__(self, api, case, shared_bias=False, mask_seed=0):
        case.ext = True                                                # (an operator-free case dispatches an ext handle as well)
        super().__init__(api, case)
        self.D = _up(case.D) if case.colbias else None
        self.M0 = gf.mask_prefill(case, 7000 + mask_seed) if case.act == 2 else None
        self.M = _up(self.M0.copy()) if case.act == 2 else None
        self.sd = 0 if shared_bias else case.bs_d
        self.param, self.keep = case.make_param(self.A, self.B, self.C, D=self.D, mask=self.M)

    def entry(self):
        g = capi.GemmExtGroup()
        g.kernel, g.param, g.count = self.handle, self.param, self.case.batch
        g.stride_a, g.stride_b, g.stride_c, g.stride_d, g.stride_mask = self.sa, self.sb, self.case.bs_c, self.sd, self.case.mask_bytes
        return g

    def mask(self):
        return _down(self.M, self.M0) if self.M is not None else None

    def run_own(self, api):
        """The group's own ext strided launch on a fresh copy of C and of the prefilled masks."""
        Cown = _up(self.C0.copy())
        Mown = _up(self.M0.copy()) if self.M0 is not None else None
        p, keep = self.case.make_param(self.A, self.B, Cown, D=self.D, mask=Mown)
        api.hip_gemm_ext_batch_strided(self.handle, C.byref(p), self.case.batch, self.sa, self.sb, self.case.bs_c, self.sd, self.case.mask_bytes)
        api.hip_sync(); api.check()
        return _down(Cown, self.C0), (_down(Mown, self.M0) if Mown is not None else None)

    def overwrite(self, api, seed):
        """New values for A, B, bias, C and mask IN PLACE (the device addresses stay): what a replayed graph has to read."""
        c = self.case
        rng = np.random.default_rng(seed)
        c.A, c.B, c.C0 = helpers.rand_values(rng, c.A.size, c.a_type), helpers.rand_values(rng, c.B.size, c.b_type), helpers.rand_values(rng, c.C0.size, c.c_type)
        self.C0 = c.C0
        pairs = [(self.A, c.A), (self.B, c.B), (self.C, c.C0)]
        if c.colbias:
            c.D = helpers.rand_values(rng, c.D.size, c.c_type)
            pairs.append((self.D, c.D))
        if c.act == 2:
            self.M0 = rng.integers(0, 256, self.M0.size).astype(np.uint8)
            pairs.append((self.M, self.M0))
        for dev, host in pairs:
            assert api.hip_memcpy_h2d(dev.data_ptr(), host.ctypes.data, host.nbytes) == 0

    def reset_outputs(self, api):
        for dev, host in ((self.C, self.C0), (self.M, self.M0)):
            if dev is not None:
                assert api.hip_memcpy_h2d(dev.data_ptr(), host.ctypes.data, host.nbytes) == 0


def _ext_grouped(api, entries):
    arr = (capi.GemmExtGroup * len(entries))(*entries)
    api.hip_gemm_ext_batch_grouped(arr, len(entries))
    api.hip_sync(); api.check()


def _f32_groups(api):
    return [FusedGroup(api, case, shared_bias=(i == gf.SHARED_BIAS), mask_seed=i) for i, case in enumerate(gf.f32_cases())]


def _assert_chain(g, what):
    """C and mask bytes of an f32 group against the fmaf chain (whole buffers: padding and the mask bits outside m x n included).  A sigmoid group's C is
    compared outside m x n only (and by test 2 against the ext oracle)."""
    ref, refm = gf.fma_chain(g.case, g.C0, g.M0)
    got = g.result()
    if g.case.act == 3:
        inside = np.zeros(ref.shape, dtype=bool)
        g.case.valid_region(inside)[...] = True
        assert np.array_equal(got.view(np.uint32)[~inside], ref.view(np.uint32)[~inside]), f"{what}: C's padding was written"
    else:
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{what}: C differs from the fmaf chain started at the bias (or was written outside m x n)"
    if g.case.act == 2:
        assert np.array_equal(g.mask(), refm), f"{what}: mask differs from !(x <= 0) of the chain's sums (or a bit outside m x n changed)"


def test_f32_mixed_list_is_bitwise_the_fma_chain_started_at_the_bias():
    """Test 1: the ten F32_CASES with the epilogues rotated, one shared bias, as ONE ext grouped call.  (The sigmoid groups' C: test 2.)"""
    api = capi.load()
    groups = _f32_groups(api)
    _ext_grouped(api, [g.entry() for g in groups])
    for kw, g in zip(F32_CASES, groups):
        _assert_chain(g, f"{kw} colbias={g.case.colbias} act={g.case.act}")


def test_f32_mixed_list_keeps_mask_bits_and_padding_outside_m_x_n():
    """Test 2: masks prefilled with random bytes -- every bit outside m x n and every byte of C's padding stays the caller's; sigmoid groups lie within
    TOL_F32 of the ext oracle."""
    api = capi.load()
    groups = _f32_groups(api)
    _ext_grouped(api, [g.entry() for g in groups])
    seen_sigmoid = seen_mask = 0
    for kw, g in zip(F32_CASES, groups):
        c, got = g.case, g.result()
        inside = np.zeros(got.shape, dtype=bool)
        c.valid_region(inside)[...] = True
        assert np.array_equal(got.view(np.uint32)[~inside], g.C0.view(np.uint32)[~inside]), f"{kw}: a byte of C's padding changed"
        if c.act == 2:
            seen_mask += 1
            gotb = np.unpackbits(g.mask().reshape(c.batch, c.n, c.mask_ld // 8), axis=2, bitorder="little")
            preb = np.unpackbits(g.M0.reshape(c.batch, c.n, c.mask_ld // 8), axis=2, bitorder="little")
            assert np.array_equal(gotb[:, :, c.m:], preb[:, :, c.m:]), f"{kw}: a mask bit beyond m changed"
        else:
            assert g.M is None
        if c.act == 3:
            seen_sigmoid += 1
            ref, _ = c.run_oracle()
            err = normf_rel(c.valid_region(ref), c.valid_region(got), c.c_type)
            assert err < TOL_F32, f"{kw}: sigmoid group, normf_rel = {err}"
    assert seen_sigmoid >= 2 and seen_mask >= 2


def test_bf16_mixed_list_matches_the_ext_oracle_and_the_own_launches():
    """Test 3: BF16_CASES with bias + ReLU + bitmask."""
    api = capi.load()
    exact = [FusedGroup(api, case, mask_seed=20 + i) for i, case in enumerate(gf.bf16_cases(exact=True))]
    _ext_grouped(api, [g.entry() for g in exact])
    for kw, g in zip(BF16_CASES, exact):
        c = g.case
        ref, refm = c.run_oracle()
        assert np.array_equal(g.result().view(np.uint8), ref.view(np.uint8)), f"{kw}: exact data, C differs from the ext oracle"
        assert np.array_equal(c.valid_mask_bits(g.mask()), c.valid_mask_bits(refm)), f"{kw}: exact data, mask bits differ from the ext oracle"
        own, ownm = g.run_own(api)
        assert np.array_equal(g.result().view(np.uint8), own.view(np.uint8)), f"{kw}: C differs from its own ext strided launch"
        assert np.array_equal(g.mask(), ownm), f"{kw}: mask differs from its own ext strided launch"
    groups = [FusedGroup(api, case, mask_seed=40 + i) for i, case in enumerate(gf.bf16_cases())]
    _ext_grouped(api, [g.entry() for g in groups])
    for kw, g in zip(BF16_CASES, groups):
        c = g.case
        ref, _ = c.run_oracle()
        err = normf_rel(c.valid_region(ref), c.valid_region(g.result()), c.c_type)
        assert err < (TOL_BF16 if c.c_type == DT.BF16 else TOL_F32), f"{kw}: normf_rel = {err}"
        decided, positive = gf.decided_mask_bits(c)
        assert decided.mean() >= 0.5, f"{kw}: {1 - decided.mean():.2f} of the mask bits are undecided"
        bits = c.valid_mask_bits(g.mask())
        assert np.array_equal(bits[decided], positive[decided].astype(bits.dtype)), f"{kw}: {np.count_nonzero(bits[decided] != positive[decided])} decided mask bits differ"


def test_launch_counts_one_per_fused_class_and_one_per_fallback_group():
    """Test 4."""
    api = capi.load()
    one_class = [FusedGroup(api, GemmCase(m, n, k, colbias=True, act=2, batch=b, seed=200 + i), mask_seed=60 + i)
                 for i, (m, n, k, b) in enumerate([(8, 8, 8, 3), (13, 13, 13, 5), (32, 32, 32, 4), (17, 9, 31, 3), (40, 24, 16, 2)])]
    api.hip_launch_count(1)
    arr = (capi.GemmExtGroup * len(one_class))(*[g.entry() for g in one_class])
    api.hip_gemm_ext_batch_grouped(arr, len(one_class))
    assert api.hip_launch_count(1) == 1
    api.hip_sync(); api.check()
    for g in one_class:
        _assert_chain(g, (g.case.m, g.case.n, g.case.k))
    plain = [FusedGroup(api, GemmCase(m, m, m, batch=4, seed=210 + m)) for m in (13, 16)]                          # ext handles without operators
    f32 = [FusedGroup(api, GemmCase(m, m, m, colbias=True, act=1, batch=3, seed=220 + m)) for m in (20, 32)]
    bf16 = [FusedGroup(api, GemmCase(m, m, m, a_type=DT.BF16, c_type=DT.BF16, colbias=True, act=2, batch=3, seed=230 + m), mask_seed=m) for m in (16, 48)]
    f64 = FusedGroup(api, GemmCase(16, 12, 9, a_type=DT.F64, batch=4, seed=240))
    mixed = [plain[0], f32[0], bf16[0], f64, plain[1], f32[1], bf16[1]]
    api.hip_launch_count(1)
    arr = (capi.GemmExtGroup * len(mixed))(*[g.entry() for g in mixed])
    api.hip_gemm_ext_batch_grouped(arr, len(mixed))
    assert api.hip_launch_count(1) == 4                                 # plain f32, fused f32, fused bf16 classes + the f64 group's own launch
    api.hip_sync(); api.check()
    for g in plain + f32:
        _assert_chain(g, (g.case.m, g.case.colbias, g.case.act))
    for g in bf16:
        ref, _ = g.case.run_oracle()
        assert normf_rel(g.case.valid_region(ref), g.case.valid_region(g.result()), DT.BF16) < TOL_BF16
    own, _ = f64.run_own(api)
    assert np.array_equal(f64.result().view(np.uint8), own.view(np.uint8)), "the f64 group differs from its own launch"


def _many_groups(api, per, shapes, counts, seed):
    """`per` fused f32 groups (bias + ReLU + bitmask) of each shape, shapes interleaved."""
    groups = []
    for i in range(per * len(shapes)):
        m, n, k = shapes[i % len(shapes)]
        groups.append(FusedGroup(api, GemmCase(m, n, k, colbias=True, act=2, beta=(i // len(shapes)) % 2, batch=counts[i % len(counts)], seed=seed + i), mask_seed=seed + i))
    return groups


def test_table_beyond_the_inline_limit_equals_the_fma_chain():
    """Test 5: 40 fused groups of count 1-3 reach the uploaded table."""
    api = capi.load()
    groups = _many_groups(api, 10, [(8, 8, 8), (13, 17, 29), (32, 32, 32), (20, 12, 9)], (1, 2, 3), 1000)
    api.hip_launch_count(1)
    arr = (capi.GemmExtGroup * len(groups))(*[g.entry() for g in groups])
    api.hip_gemm_ext_batch_grouped(arr, len(groups))
    assert api.hip_launch_count(1) == 1
    api.hip_sync(); api.check()
    for i, g in enumerate(groups):
        _assert_chain(g, f"group {i}")


def _plan(api, groups, ext):
    """A plan from the groups' entries; the Python list is gone before the plan is returned."""
    cls = capi.GemmExtGroup if ext else capi.GemmGroup
    arr = (cls * len(groups))(*[g.entry() for g in groups])
    plan = (api.hip_gemm_ext_group_plan_create if ext else api.hip_gemm_group_plan_create)(arr, len(groups))
    api.check()
    assert plan
    C.memset(arr, 0xff, C.sizeof(arr))
    del arr
    return plan


def _bits(g):
    out = [g.result().view(np.uint8).copy()]
    if isinstance(g, FusedGroup) and g.M is not None:
        out.append(g.mask().copy())
    return out


def test_plans_equal_the_entries_resident_captured_and_replayed():
    """Test 6."""
    import torch
    api = capi.load()
    # (a) the plain and ext lists of tests 1 and 3 as plans: bits of the entries, launches as counted
    lists = [(False, lambda: [Group(api, GemmCase(**kw)) for kw in F32_CASES]), (False, lambda: [Group(api, GemmCase(**kw)) for kw in BF16_CASES]),
             (True, lambda: _f32_groups(api)), (True, lambda: [FusedGroup(api, case, mask_seed=20 + i) for i, case in enumerate(gf.bf16_cases())])]
    for ext, make in lists:
        direct, planned = make(), make()
        arr = ((capi.GemmExtGroup if ext else capi.GemmGroup) * len(direct))(*[g.entry() for g in direct])
        api.hip_launch_count(1)
        (api.hip_gemm_ext_batch_grouped if ext else api.hip_gemm_batch_grouped)(arr, len(direct))
        counted = api.hip_launch_count(1)
        api.hip_sync(); api.check()
        plan = _plan(api, planned, ext)
        for g in planned:                                              # the batch-reduce counts the params pointed at are gone as well
            for cnt in g.keep:
                cnt.value = 0
        assert api.hip_gemm_group_plan_launches(plan) == counted
        api.hip_launch_count(1)
        api.hip_gemm_group_plan_launch(plan)
        assert api.hip_launch_count(1) == counted
        api.hip_sync(); api.check()
        for i, (a, b) in enumerate(zip(direct, planned)):
            assert all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b))), f"{'ext' if ext else 'plain'} list, group {i}: the plan differs from the entry"
        api.hip_gemm_group_plan_destroy(plan)
    # (b) 600 one-problem groups over four shapes: pointer table, deep search
    groups = _many_groups(api, 150, [(8, 8, 8), (13, 13, 13), (20, 12, 9), (32, 32, 32)], (1,), 3000)
    order = np.random.default_rng(3999).permutation(len(groups))
    groups = [groups[i] for i in order]
    plan = _plan(api, groups, True)
    assert api.hip_gemm_group_plan_launches(plan) == 1
    api.hip_gemm_group_plan_launch(plan)
    api.hip_sync(); api.check()
    for i, g in enumerate(groups):
        _assert_chain(g, f"plan of 600, group {i}")
    # (c) captured on one stream; the direct entry under capture is refused and leaves the graph valid
    some = (capi.GemmExtGroup * 2)(groups[0].entry(), groups[1].entry())
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        api.hip_set_stream(side.cuda_stream)
        api.hip_launch_count(1)
        graph.capture_begin()
        api.hip_gemm_ext_batch_grouped(some, 2)
        refused, msg = api.hip_get_last_error(), api.hip_get_last_error_string()
        api.hip_clear_last_error()
        api.hip_gemm_group_plan_launch(plan)
        graph.capture_end()
        assert api.hip_launch_count(0) == 1
    api.check()
    assert refused == -3 and b"plan" in msg, (refused, msg)
    torch.cuda.current_stream().wait_stream(side)
    api.hip_set_stream(None); api.hip_set_async(0)
    for rep in range(2):
        for i, g in enumerate(groups):
            g.overwrite(api, 5000 + 1000 * rep + i)
        torch.cuda.synchronize()
        graph.replay(); torch.cuda.synchronize()
        replayed = [_bits(g) for g in groups]
        for g in groups:
            g.reset_outputs(api)
        api.hip_gemm_group_plan_launch(plan)                           # a fresh direct launch on the new values
        api.hip_sync(); api.check()
        for i, (g, r) in enumerate(zip(groups, replayed)):
            assert all(np.array_equal(x, y) for x, y in zip(_bits(g), r)), f"replay {rep}, group {i}: differs from a direct launch on the new values"
        for i in (0, 1, 2, 3, len(groups) - 1):                        # ... which is the chain on the new values
            _assert_chain(groups[i], f"replay {rep}, group {i}")
    del graph
    api.hip_gemm_group_plan_destroy(plan)


def _reset_outputs(api, g):
    for dev, host in ((g.C, g.C0), (getattr(g, "M", None), getattr(g, "M0", None))):
        if dev is not None:
            assert api.hip_memcpy_h2d(dev.data_ptr(), host.ctypes.data, host.nbytes) == 0


def _own_launch_lists(api):
    """(ext, groups, own indices, launches): lists whose launch rule sends groups to their OWN kernels next to a class of two or more.
    ext: 13x17x29, 16^3 x 2048 (2048 items on 16-tiles: stays) and 40^3 x 512 (2048 items, m and n no multiples of 16: stays) are the fused f32 class; 32^3 x 2048
    (2048 items, 32-tiles, m and n multiples of 16) leaves for its own ext kernel; the only fused bf16 group, a STRIDE BRGEMM, is a single-group class.
    plain: two small f32 groups are the class; 32^3 x 2048 leaves (the plain rule); the only bf16 group, a STRIDE BRGEMM, is a single-group class."""
    from libxsmm_amd.capi import GEMM_FLAG
    ext = [FusedGroup(api, GemmCase(13, 17, 29, colbias=True, act=2, batch=5, seed=400), mask_seed=400),
           FusedGroup(api, GemmCase(32, 32, 32, colbias=True, act=2, batch=2048, seed=401), mask_seed=401),
           FusedGroup(api, GemmCase(16, 16, 16, colbias=True, act=1, batch=2048, seed=402)),
           FusedGroup(api, GemmCase(24, 40, 34, a_type=DT.BF16, c_type=DT.F32, flags=GEMM_FLAG.VNNI_A, br_type=capi.BR_STRIDE, br_count=3, colbias=True, act=2,
                                    batch=4, seed=403), mask_seed=403),
           FusedGroup(api, GemmCase(40, 40, 40, colbias=True, act=0, beta=1, batch=512, seed=404))]
    plain = [Group(api, GemmCase(13, 17, 29, batch=5, seed=410)),
             Group(api, GemmCase(32, 32, 32, batch=2048, seed=411)),
             Group(api, GemmCase(24, 40, 34, a_type=DT.BF16, c_type=DT.F32, flags=GEMM_FLAG.VNNI_A, br_type=capi.BR_STRIDE, br_count=3, batch=4, seed=413)),
             Group(api, GemmCase(23, 23, 23, beta=1, batch=7, seed=414))]
    return [(True, ext, (1, 3), 3), (False, plain, (1, 2), 3)]


def test_plan_own_launches_run_from_the_stored_copies_and_follow_the_launch_rule():
    """The own-launch half of a plan and the launch rule: groups that the rule sends to their own kernels (a large f32 group; a single-group class through a
    STRIDE BRGEMM handle, whose batch-reduce count the plan has to keep by value) next to a class that stays.  The entry and the plan issue the launches the
    rule says; the plan, launched directly and replayed from a captured graph after the caller's list and counts are gone, has the bits of the entry; a
    destroy while the stream is being captured is refused and keeps the plan."""
    import torch
    api = capi.load()
    for (ext, direct, own, launches), (_, planned, _, _) in zip(_own_launch_lists(api), _own_launch_lists(api)):
        what = "ext" if ext else "plain"
        arr = ((capi.GemmExtGroup if ext else capi.GemmGroup) * len(direct))(*[g.entry() for g in direct])
        api.hip_launch_count(1)
        (api.hip_gemm_ext_batch_grouped if ext else api.hip_gemm_batch_grouped)(arr, len(direct))
        assert api.hip_launch_count(1) == launches, what                # one class + the two own launches
        api.hip_sync(); api.check()
        for i in own:                                                  # a group that left is bitwise its own strided launch
            want = direct[i].run_own(api)
            want = want if ext else (want, None)
            assert np.array_equal(direct[i].result().view(np.uint8), want[0].view(np.uint8)), f"{what} entry, group {i}: differs from its own launch"
            if want[1] is not None:
                assert np.array_equal(direct[i].mask(), want[1]), f"{what} entry, group {i}: mask differs from its own launch"
        plan = _plan(api, planned, ext)
        for g in planned:                                              # the counts the params pointed at now read 0: a plan that re-read them would store the start value
            for cnt in g.keep:
                cnt.value = 0
        assert api.hip_gemm_group_plan_launches(plan) == launches, what
        api.hip_launch_count(1)
        api.hip_gemm_group_plan_launch(plan)
        assert api.hip_launch_count(1) == launches, what
        api.hip_sync(); api.check()
        for i, (a, b) in enumerate(zip(direct, planned)):
            assert all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b))), f"{what} plan, group {i}: differs from the entry"
        for g in planned:
            _reset_outputs(api, g)
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            api.hip_set_stream(side.cuda_stream)
            graph.capture_begin()
            api.hip_gemm_group_plan_destroy(plan)                      # refused: the plan stays
            refused = api.hip_get_last_error()
            api.hip_clear_last_error()
            api.hip_gemm_group_plan_launch(plan)
            graph.capture_end()
        api.check()
        assert refused == -3, refused
        torch.cuda.current_stream().wait_stream(side)
        api.hip_set_stream(None); api.hip_set_async(0)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(direct, planned)):              # nothing ran during the capture
            assert not all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b))), f"{what} plan, group {i}: computed while being captured"
        graph.replay(); torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(direct, planned)):
            assert all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b))), f"{what} plan, group {i}: the replayed graph differs from the entry"
        del graph
        api.hip_gemm_group_plan_destroy(plan); api.check()


RELEASED_CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import torch
from helpers import GemmCase
from libxsmm_amd import capi
from test_gemm_grouped_gpu import Group
api = capi.load()
groups = [Group(api, GemmCase(13, 17, 29, batch=5, seed=1)), Group(api, GemmCase(16, 16, 16, batch=3, seed=2)), Group(api, GemmCase(32, 32, 32, batch=2048, seed=3))]
arr = (capi.GemmGroup * 3)(*[g.entry() for g in groups])
plan = api.hip_gemm_group_plan_create(arr, 3); api.check()
assert plan and api.hip_gemm_group_plan_launches(plan) == 2           # one class + the large group's own launch (a KernelCtx the plan points at)
api.hip_gemm_group_plan_launch(plan); api.hip_sync(); api.check()
ref, _ = groups[0].case.run_oracle(fma=True)
assert np.array_equal(groups[0].result().view(np.uint32), ref.view(np.uint32))
before = [g.result().copy() for g in groups]
api.finalize()                                                        # releases every handle of the plan
api.hip_launch_count(1)
api.hip_gemm_group_plan_launch(plan)
err, msg = api.hip_get_last_error(), api.hip_get_last_error_string().decode()
api.hip_clear_last_error()
launched = api.hip_launch_count(1)
torch.cuda.synchronize()
same = all(np.array_equal(a, g.result()) for a, g in zip(before, groups))
api.hip_gemm_group_plan_destroy(plan)
print("RESULT", err, launched, int(same), "released" in msg)
"""


def test_a_plan_whose_handles_were_released_is_refused_and_launches_nothing():
    """libxsmm_finalize frees the kernel contexts a plan's own launches point at: the plan keeps the registry generation, so a launch afterwards sets -3
    before it touches one of them and issues nothing.  In a child process: the finalize would take every other test's handles with it.  (The other -3 of a
    launch, another device being current, needs a second device and has no test.)"""
    r = subprocess.run([sys.executable, "-c", RELEASED_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
    assert line and line[0].split()[1:] == ["-3", "0", "1", "True"], r.stdout + r.stderr


def test_stream_ordered_call_in_a_pipeline_section_equals_the_serial_launches():
    """Test 7."""
    import torch
    api = capi.load()
    cases = [GemmCase(32, 32, 32, colbias=True, act=2, batch=64, seed=100), GemmCase(13, 17, 29, colbias=True, act=1, batch=33, seed=101),
             GemmCase(40, 40, 40, colbias=True, act=3, batch=17, beta=1, seed=102),
             GemmCase(32, 32, 32, a_type=DT.BF16, c_type=DT.BF16, flags=capi.GEMM_FLAG.VNNI_A, colbias=True, act=2, batch=40, seed=103),
             GemmCase(16, 16, 16, a_type=DT.BF16, c_type=DT.F32, colbias=True, act=0, batch=50, seed=104),
             GemmCase(16, 16, 16, a_type=DT.F64, batch=9, seed=105)]
    serial = [FusedGroup(api, c, mask_seed=80 + i) for i, c in enumerate(cases)]
    _ext_grouped(api, [g.entry() for g in serial])                    # blocking
    groups = [FusedGroup(api, c, mask_seed=80 + i) for i, c in enumerate(cases)]
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    assert api.hip_pipeline_begin(4) == 0
    arr = (capi.GemmExtGroup * len(groups))(*[g.entry() for g in groups])
    api.hip_gemm_ext_batch_grouped(arr, len(groups))
    assert api.hip_pipeline_end() == 0
    api.hip_sync(); api.check()
    api.hip_set_stream(None); api.hip_set_async(0)
    for i, (g, s) in enumerate(zip(groups, serial)):
        assert all(np.array_equal(x, y) for x, y in zip(_bits(g), _bits(s))), f"group {i}"


def test_c_example_runs_three_fused_shapes_as_one_call_and_as_a_captured_plan(tmp_path):
    """Test 8."""
    libdir = os.path.join(ROOT, "libxsmm_amd", "lib")
    exe = str(tmp_path / "grouped_fused_driver")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-isystem", "/opt/rocm/include",
           os.path.join(ROOT, "examples", "grouped_fused_driver.c"), "-L" + libdir, "-lxsmm_amd", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "normf_rel" in r.stdout and "replay" in r.stdout


def test_guarded_rerun_with_operands_bias_and_masks_flush_against_unmapped_memory():
    """Test 9: tests 1, 5 and 6 again, every operand, bias and mask flush against unmapped address space (tests/guard.py via tests/conftest.py; uploads go
    through helpers.UPLOAD_HOOK): the bias and operand loads are clamped, so no access leaves an operand.  The second side only runs once the first has passed."""
    for side in ("end", "front"):
        env = dict(os.environ, LIBXSMM_TEST_GUARD=side)
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
               "-k", "test_f32_mixed_list_is_bitwise or test_table_beyond or test_plans_equal", "-v", "--no-header"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
        assert r.returncode == 0, f"guarded run ({side}) ended with {r.returncode} (negative / 134: the GPU faulted on an out-of-bounds access):\n{tail}"
        assert "3 passed" in r.stdout, tail
