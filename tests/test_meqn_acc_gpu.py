"""Accumulating batches of matrix equations on the GPU (libxsmm_hip_meqn_batch_strided_accumulate).

The yardstick is the caller's loop: `count` stream-ordered single calls that all read and write the same output.  ORDER_LOOP must reproduce its bits in one
launch (the carried form); ORDER_ANY (the sliced form) must reproduce the bits of the documented order of additions, restated in numpy, and be no further
from the float64 sum than 1.5 x the loop's own distance; everything the fused forms do not cover runs the elements one after another."""
import ctypes as C

import numpy as np
import pytest

import test_meqn as tm
from helpers import normf_rel
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, MEQN_ORDER_ANY, MEQN_ORDER_LOOP
from meqn_acc_helpers import CASES, AccBatch, dbeta, gold_f64, sliced_restatement, slices_rule

pytestmark = pytest.mark.gpu
ll = C.c_longlong
GUARD = 64                                                     # guard words in front of and behind the output
# besides the carried position: positions that all elements share (stride 0)
SHARED = {"dgamma_bf16_in": (2,), "dgamma_f32_ld48": (3,)}


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.copy()).to("cuda:0")


def _dispatch(api, case, jit=2):
    tree, shapes, out_shape, _ = case
    api.hip_set_jit(jit)
    h = api.dispatch_meqn(tm.build(api, tree, shapes), capi.MeqnArgShape(*out_shape))
    api.hip_set_jit(1)
    assert h
    return h


class Output:
    """The output on the device between two guard regions, initialised with the carried operand's values."""

    def __init__(self, acc0):
        import torch
        self.bf16 = acc0.dtype == np.uint16
        self.guard = np.full(GUARD, 0x5A5A if self.bf16 else -77.0, dtype=acc0.dtype)
        self.size = acc0.size
        self.buf = _dev(np.concatenate([self.guard, acc0, self.guard]))
        self.ptr = self.buf.data_ptr() + GUARD * acc0.itemsize
        self.torch = torch

    def host(self):
        x = self.buf.cpu().numpy()
        return x.view(np.uint16) if self.bf16 else x

    def inside(self):
        return self.host()[GUARD:GUARD + self.size]

    def guards_intact(self):
        x = self.host()
        return np.array_equal(x[:GUARD], self.guard) and np.array_equal(x[-GUARD:], self.guard)


def _param(ptrs, carried, out_ptr):
    inputs = (capi.MatrixArg * len(ptrs))()
    for i, v in enumerate(ptrs):
        inputs[i].primary = out_ptr if i == carried else v
    p = capi.MeqnParam()
    p.inputs = inputs
    p.output.primary = out_ptr
    return p, inputs


def _accumulate(api, h, ptrs, b, out_ptr, order, count=None):
    p, keep = _param(ptrs, b.carried, out_ptr)
    sin = (ll * len(b.strides))(*b.strides)
    api.hip_meqn_batch_strided_accumulate(h, C.byref(p), b.count if count is None else count, len(b.strides), sin, 0, None, order)
    return keep


def _loop(api, h, ptrs, b, out_ptr):
    """The caller's loop: one stream-ordered single call per element, every one on the same output."""
    api.hip_set_async(1)
    keep = []
    for i in range(b.count):
        keep.append(_param([v + i * s for v, s in zip(ptrs, b.strides)], b.carried, out_ptr))
        capi.Api.call(h, keep[-1][0])
    api.hip_sync()
    api.hip_set_async(0)
    api.check()


def _valid(x, shape):
    m, n, ld, _ = shape
    return x.reshape(n, ld)[:, :m]


@pytest.mark.parametrize("count", [1, 7, 4096])
@pytest.mark.parametrize("name", sorted(CASES))
def test_order_loop_is_one_launch_with_the_bits_of_the_loop(name, count):
    api = capi.load()
    case = CASES[name]
    out_shape = case[2]
    m, n, ld, _ = out_shape
    h = _dispatch(api, case)
    b = AccBatch(case, count, shared=SHARED.get(name, ()), seed=count)
    assert sum(s == 0 for s in b.strides) == 1 + len(SHARED.get(name, ()))
    dev = [_dev(a) for a in b.inputs]
    ptrs = [d.data_ptr() for d in dev]
    out, ref = Output(b.acc0), Output(b.acc0)
    api.hip_launch_count(1)
    keep = _accumulate(api, h, ptrs, b, out.ptr, MEQN_ORDER_LOOP)
    api.check()
    assert api.hip_launch_count(0) == 1
    assert api.hip_kernel_name(h, 1).decode().endswith("_c"), api.hip_kernel_name(h, 1)
    _loop(api, h, ptrs, b, ref.ptr)
    assert out.torch.equal(out.buf, ref.buf)
    assert not np.array_equal(out.inside(), b.acc0)
    assert out.guards_intact()                                                                     # the output's neighbours ...
    assert np.array_equal(out.inside().reshape(n, ld)[:, m:], b.acc0.reshape(n, ld)[:, m:])        # ... and the rows between its padded columns
    del keep


def _check_order_any(api, name, case, count):
    """Items of the ORDER_ANY contract on one workload; prints the figures before it asserts."""
    import torch
    out_shape = case[2]
    m, n, ld, _ = out_shape
    h = _dispatch(api, case)
    b = AccBatch(case, count, seed=count + 3)
    dev = [_dev(a) for a in b.inputs]
    ptrs = [d.data_ptr() for d in dev]
    out, again, other, ref = (Output(b.acc0) for _ in range(4))
    _accumulate(api, h, ptrs, b, out.ptr, MEQN_ORDER_ANY)
    api.check()
    assert api.hip_kernel_name(h, 1).decode().endswith("_s"), api.hip_kernel_name(h, 1)
    _accumulate(api, h, ptrs, b, again.ptr, MEQN_ORDER_ANY)
    api.check()
    stream = torch.cuda.Stream()
    api.hip_set_stream(stream.cuda_stream); api.hip_set_async(1)
    _accumulate(api, h, ptrs, b, other.ptr, MEQN_ORDER_ANY)
    api.hip_sync(); api.hip_set_async(0); api.hip_set_stream(None)
    api.check()
    _loop(api, h, ptrs, b, ref.ptr)
    got, loop = _valid(out.inside(), out_shape), _valid(ref.inside(), out_shape)
    gold = gold_f64(b, name)
    e_got, e_loop, e_rel = normf_rel(gold, got, DT.F32), normf_rel(gold, loop, DT.F32), normf_rel(loop, got, DT.F32)
    slices = slices_rule(count, m, n)
    print(f"{name} x {count}: S = {slices}, normf_rel sliced vs f64 {e_got:.3e}, loop vs f64 {e_loop:.3e}, sliced vs loop {e_rel:.3e}")
    assert slices >= 2
    assert e_got <= 1.5 * e_loop
    assert e_rel < 1e-5
    assert torch.equal(out.buf, again.buf) and torch.equal(out.buf, other.buf)                    # two runs, and a run on a second stream
    want = sliced_restatement(b, name, slices)
    assert np.array_equal(out.inside().view(np.uint32), want.ravel().view(np.uint32))             # the documented order of additions, bit for bit
    assert out.guards_intact()


@pytest.mark.parametrize("name,count", [("dgamma_f32", 4096), ("dbeta_f32_64", 4096), ("dgamma_bf16_in", 4096), ("dgamma_f32_ld48", 1000), ("dbeta_f32", 1000)])
def test_order_any_is_the_documented_order_and_no_worse_than_the_loop(name, count):
    """64 x 64 x 4096 and 40 x 24 (ld 48) x 1000.  Gold: the same addends summed in float64.  Bound: normf_rel of the result against the gold at most 1.5 x
    the normf_rel of the loop's result against the gold (both differ from it by the order of the roundings only, and the loop's order is the yardstick);
    normf_rel against the loop's result below 1e-5 (the bound of re-associated f32 sums in tests/test_meqn.py)."""
    _check_order_any(capi.load(), name, CASES[name], count)


@pytest.mark.parametrize("order", [MEQN_ORDER_LOOP, MEQN_ORDER_ANY], ids=["loop", "any"])
def test_seventy_thousand_elements_of_an_8_x_1_tree(order):
    api = capi.load()
    case, count = dbeta(DT.F32, 8, 1, 8), 70000
    if order == MEQN_ORDER_ANY:
        _check_order_any(api, "dbeta_8x1", case, count)
        return
    h = _dispatch(api, case)
    b = AccBatch(case, count, seed=70)
    dev = [_dev(a) for a in b.inputs]
    ptrs = [d.data_ptr() for d in dev]
    out, ref = Output(b.acc0), Output(b.acc0)
    api.hip_launch_count(1)
    _accumulate(api, h, ptrs, b, out.ptr, order)
    api.check()
    assert api.hip_launch_count(0) == 1 and api.hip_kernel_name(h, 1).decode().endswith("_c")
    _loop(api, h, ptrs, b, ref.ptr)
    assert out.torch.equal(out.buf, ref.buf) and out.guards_intact()


def test_order_any_on_a_head_that_is_not_a_sum_takes_the_loop_order():
    """ORDER_ANY is a permission: max(out, x) has no re-associated form, the carried kernel runs and the bits are the loop's."""
    api = capi.load()
    case = CASES["running_max"]
    h = _dispatch(api, case)
    b = AccBatch(case, 100, seed=5)
    dev = [_dev(a) for a in b.inputs]
    ptrs = [d.data_ptr() for d in dev]
    out, ref = Output(b.acc0), Output(b.acc0)
    _accumulate(api, h, ptrs, b, out.ptr, MEQN_ORDER_ANY)
    api.check()
    assert api.hip_kernel_name(h, 1).decode().endswith("_c")
    _loop(api, h, ptrs, b, ref.ptr)
    assert out.torch.equal(out.buf, ref.buf)


@pytest.mark.parametrize("name,carried,count", [("softmax_bwd", 1, 5), ("matmul_mul", 0, 4)])
@pytest.mark.parametrize("order", [MEQN_ORDER_LOOP, MEQN_ORDER_ANY], ids=["loop", "any"])
def test_trees_without_a_fused_form_run_the_elements_one_after_another(name, carried, count, order):
    """A phased tree (a reduction to one number inside) and a tree with a GEMM node, each with an operand that is the output: the element loop."""
    api = capi.load()
    tree, shapes, out_shape = tm.CASES[name]
    assert tuple(shapes[carried]) == tuple(out_shape)
    case = (tree, shapes, out_shape, carried)
    h = _dispatch(api, case)
    single = api.hip_kernel_name(h, 0).decode()
    b = AccBatch(case, count, seed=41)
    dev = [_dev(a) for a in b.inputs]
    ptrs = [d.data_ptr() for d in dev]
    out, ref = Output(b.acc0), Output(b.acc0)
    _accumulate(api, h, ptrs, b, out.ptr, order)
    api.check()
    assert api.hip_kernel_name(h, 1).decode() == single
    _loop(api, h, ptrs, b, ref.ptr)
    bound = max(tm.BY_NORM[name], 1e-5 if name == "softmax_bwd" else 0.0)
    assert normf_rel(_valid(ref.inside(), out_shape), _valid(out.inside(), out_shape), DT.F32) <= bound
    assert not np.array_equal(out.inside(), b.acc0) and out.guards_intact()


@pytest.mark.parametrize("jit", [0, 2], ids=["element_loop", "carried"])
def test_per_element_scalars_may_live_in_host_memory_in_blocking_mode(jit):
    """a = var[s2], b = -a * mean[s2] as host arrays with stride 4 (blocking mode) give the bits of the device-resident case."""
    api = capi.load()
    case, count = CASES["dgamma_f32"], 9
    h = _dispatch(api, case, jit)
    b = AccBatch(case, count, seed=11)
    dev = [_dev(a) for a in b.inputs]
    ptrs = [d.data_ptr() for d in dev]
    on_device, on_host = Output(b.acc0), Output(b.acc0)
    _accumulate(api, h, ptrs, b, on_device.ptr, MEQN_ORDER_LOOP)
    api.check()
    assert api.hip_kernel_name(h, 1).decode().endswith("_c") == (jit == 2)
    mixed = list(ptrs)
    mixed[1], mixed[2] = b.inputs[1].ctypes.data, b.inputs[2].ctypes.data
    _accumulate(api, h, mixed, b, on_host.ptr, MEQN_ORDER_LOOP)
    api.check()
    assert on_host.torch.equal(on_host.buf, on_device.buf)
    assert not np.array_equal(on_host.inside(), b.acc0)


def test_misaligned_operands_run_the_elements_one_after_another():
    """A stepped operand whose stride is not a multiple of 16 bytes cannot enter the generated forms (16-byte accesses)."""
    api = capi.load()
    case, count = CASES["dbeta_f32"], 6
    h = _dispatch(api, case)
    b = AccBatch(case, count, seed=13)
    b.strides[3] = b.strides[3] - 8                              # still beyond the element's footprint, no longer a multiple of 16
    assert b.strides[3] % 16 == 8 and b.strides[3] >= 48 * 24 * 4
    dev = [_dev(a) for a in b.inputs]
    ptrs = [d.data_ptr() for d in dev]
    out, ref = Output(b.acc0), Output(b.acc0)
    _accumulate(api, h, ptrs, b, out.ptr, MEQN_ORDER_ANY)
    api.check()
    assert not api.hip_kernel_name(h, 1).decode().endswith(("_c", "_s"))
    _loop(api, h, ptrs, b, ref.ptr)
    assert out.torch.equal(out.buf, ref.buf) and out.guards_intact()
