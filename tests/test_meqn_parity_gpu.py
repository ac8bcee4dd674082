"""Matrix-equation parity on the GPU, per element (tests/meqn_parity_helpers.py): every row through the chain of TPP launches (LIBXSMM_HIP_JIT=0) and through the
generated kernel (=2) on the same bytes, twice per handle with different data, every kernel name asserted, every byte outside the result checked.

  chain against the oracle composition    same_bits, or the ref64 bound for trees with libm, a sum or a MATMUL
  generated kernel against the chain      same_bits for element-wise trees (libm included), per-row reductions and extrema, ref64 where a sum folds to one number
"""
import ctypes as C

import numpy as np
import pytest

import meqn_parity_helpers as mp
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, MEQN_ORDER_ANY, MEQN_ORDER_LOOP
from meltw_ew_helpers import FLT_MIN, bits_of
from meqn_acc_helpers import dgamma
from meqn_batch_helpers import round16

pytestmark = pytest.mark.gpu
ROWS = mp.rows()
ll = C.c_longlong


@pytest.mark.parametrize("name", sorted(ROWS))
def test_row_through_the_chain_and_the_generated_kernel(name):
    api = capi.load()
    case, tab = ROWS[name]
    h_chain, h_fused = case.dispatch(api, 0), case.dispatch(api, 2)                 # (the kernel names are asserted in there)
    rule_chain = mp.chain_rule(case.tree, case.shapes)
    rule_fused = mp.fused_rule(case.tree, case.shapes) if case.expect != "meqn_tpp_chain" else "same_bits"
    worst = {"chain": {}, "fused": {}}
    for seed in (1, 2):                                                             # the second call reuses handle and workspace
        bufs = case.pack(mp.values(case, tab, seed))
        te = case.ref64(bufs) if "ref64" in (rule_chain, rule_fused) else None
        chain = mp.run_gpu(case, api, h_chain, bufs)
        case.check(chain, rule_chain, case.oracle(bufs), te=te, what=f"{name} seed {seed}: chain against the oracle composition", stats=worst["chain"])
        fused = mp.run_gpu(case, api, h_fused, bufs)
        case.check(fused, rule_fused, case.logical(chain), te=te, what=f"{name} seed {seed}: {case.expect} against the chain", stats=worst["fused"])
    print(f"{name}: chain {rule_chain} err / bound {worst['chain'].get('ratio', 0.0):.3f}; {case.expect} {rule_fused} err / bound {worst['fused'].get('ratio', 0.0):.3f}")


@pytest.mark.parametrize("moved", ["argument", "output"])
@pytest.mark.parametrize("name", ["recip_mul_24x3", "case_softmax_bwd"])
def test_a_pointer_off_the_16_byte_grid_takes_the_chain_at_run_time(name, moved):
    """A handle with a generated kernel called with an f32 argument (or the output) 4 bytes off: run_meqn's host-side test sends the call down the chain -- no
    misaligned vector access is launched.  What shows it is case_softmax_bwd, whose generated kernel adds its sum as a tree in LDS and so differs from the
    chain in bits: the aligned call on the handle has the kernel's bits, the misaligned call on the SAME handle has those of the LIBXSMM_HIP_JIT=0 handle.
    (libxsmm_hip_launch_count cannot show it: it counts calls -- a chain of three nodes reports 1.)  recip_mul_24x3, bit-identical on both paths, covers the
    element-wise form's argument order and padding on that route."""
    api = capi.load()
    case, tab = ROWS[name]
    h_chain, h_fused = case.dispatch(api, 0), case.dispatch(api, 2)
    bufs = case.pack(mp.values(case, tab, 3))
    want = mp.run_gpu(case, api, h_chain, bufs)
    if name == "case_softmax_bwd":
        aligned = mp.run_gpu(case, api, h_fused, bufs)
        assert not np.array_equal(bits_of(aligned), bits_of(want))                    # otherwise the bits below would say nothing
    got = mp.run_gpu(case, api, h_fused, bufs, arg_offset=(1, 1) if moved == "argument" else None, out_offset=1 if moved == "output" else 0)
    case.check(got, "same_bits", case.logical(want), what=f"{moved} moved by 4 bytes")
    assert np.array_equal(bits_of(got), bits_of(want))


def _batch_layout(case, count):
    """per argument (elements per batch element, byte stride), then the output's: strides beyond the footprint, multiples of 16 bytes."""
    lay = []
    for k, (m, n, ld, dt) in enumerate(case.shapes):
        size = np.dtype(mp.NPDT[dt]).itemsize
        stride = round16(case.arg_elems(k) * size + 16 * (k + 1))
        lay.append((stride // size, stride))
    size = np.dtype(mp.NPDT[case.odt]).itemsize
    stride = round16(case.out_elems * size + 32)
    return lay, (stride // size, stride)


@pytest.mark.parametrize("name", ["bias_relu_bf16_24x3", "softmax_fwd_8x3", "col_softmax_64x12"])
def test_batched_form_equals_the_single_calls_and_leaves_the_gaps(name):
    """libxsmm_hip_meqn_batch_strided on an element-wise, a scalar-phased and a vector-phased tree: three elements whose strides exceed their footprint, NaN
    between the elements of every argument and -7 between those of the output.  Every element has the bits of the single call; no gap is written."""
    api = capi.load()
    case, tab = ROWS[name]
    h = case.dispatch(api, 2)
    count = 3
    lay, (out_per, out_stride) = _batch_layout(case, count)
    per_elem = [case.pack(mp.values(case, tab, 10 + i)) for i in range(count)]
    ins = []
    for k, (per, _) in enumerate(lay):
        dt = case.shapes[k][3]
        b = np.full(count * per, mp._nan(dt), dtype=mp.NPDT[dt])
        for i in range(count):
            b[i * per: i * per + case.arg_elems(k)] = per_elem[i][k]
        ins.append(b)
    out0 = np.full(count * out_per, mp._gap(case.odt), dtype=mp.NPDT[case.odt])
    dev, out = [mp.upload(b) for b in ins], mp.upload(out0)
    inputs = (capi.MatrixArg * len(dev))()
    for k, d in enumerate(dev):
        inputs[k].primary = d.data_ptr()
    p = capi.MeqnParam()
    p.inputs = inputs
    p.output.primary = out.data_ptr()
    sin = (ll * len(lay))(*[s for _, s in lay])
    api.hip_meqn_batch_strided(h, C.byref(p), count, len(lay), sin, out_stride, 0, 0, None)
    api.hip_sync(); api.check()
    assert api.hip_kernel_name(h, 1).decode() == api.hip_kernel_name(h, 0).decode() + "_b"
    got = out.cpu().numpy().view(out0.dtype)
    for k, (d, b) in enumerate(zip(dev, ins)):
        assert np.array_equal(bits_of(d.cpu().numpy().view(b.dtype)), bits_of(b)), f"argument {k} was written"
    for i in range(count):
        single = mp.run_gpu(case, api, h, per_elem[i])
        block = got[i * out_per: (i + 1) * out_per]
        assert np.array_equal(bits_of(block[:case.out_elems]), bits_of(single)), f"element {i} differs from the single call"
        assert np.array_equal(bits_of(block[case.out_elems:]), bits_of(out0[:out_per - case.out_elems])), f"the gap behind element {i} was written"


class _Acc:
    """dgamma += (a * inp + b) * dout over `count` elements: inp / dout bf16 with denormal codes over the wide range, NaN between the elements; a, b one f32 per
    element; the accumulator f32 between two guard regions."""
    GUARD = 64

    def __init__(self, count, seed):
        self.tree, self.shapes, self.out_shape, self.carried = dgamma(DT.BF16, 64, 64, 64)
        self.count, m, n, ld = count, 64, 64, 64
        self.case = mp.EqCase(self.tree, self.shapes, self.out_shape, "meqn_jit_e")
        self.per = round16(ld * n * 2 + 48) // 2
        self.big = []
        for k in (0, 3):
            b = np.full(count * self.per, mp._nan(DT.BF16), dtype=np.uint16)
            for i in range(count):
                b[i * self.per: i * self.per + ld * n] = mp.table("mild" if k == 0 else "wide", DT.BF16, m, n, seed * 1000 + 2 * i + (k > 0)).ravel()
            self.big.append(b)
        self.a = mp.table("nonzero", DT.F32, count + 1, 1, seed + 7).ravel()
        self.b = mp.table("mild", DT.F32, count + 1, 1, seed + 8).ravel()
        self.acc0 = mp.table("wide", DT.F32, m, n, seed + 9).ravel()
        self.strides = [self.per * 2, 4, 4, self.per * 2, 0]
        self.dev = [mp.upload(x) for x in (self.big[0], self.a, self.b, self.big[1])]

    def element(self, i):
        ld_n = 64 * 64
        return [self.big[0][i * self.per: i * self.per + ld_n], self.a[i:i + 1], self.b[i:i + 1], self.big[1][i * self.per: i * self.per + ld_n]]

    def new_out(self):
        g = np.full(self.GUARD, -7.0, dtype=np.float32)
        return mp.upload(np.concatenate([g, self.acc0, g]))

    def param(self, out, i=0):
        inputs = (capi.MatrixArg * 5)()
        for k, d in enumerate(self.dev):
            inputs[k].primary = d.data_ptr() + i * self.strides[k]
        inputs[4].primary = out.data_ptr() + self.GUARD * 4
        p = capi.MeqnParam()
        p.inputs = inputs
        p.output.primary = inputs[4].primary
        return p, inputs

    def accumulate(self, api, h, out, order):
        p, keep = self.param(out)
        api.hip_meqn_batch_strided_accumulate(h, C.byref(p), self.count, 5, (ll * 5)(*self.strides), 0, None, order)
        api.hip_sync(); api.check()
        return keep

    def host(self, out):
        x = out.cpu().numpy()
        assert (x[:self.GUARD] == -7.0).all() and (x[-self.GUARD:] == -7.0).all(), "the accumulator's neighbours were written"
        return x[self.GUARD:-self.GUARD]


@pytest.mark.parametrize("count,order", [(5, MEQN_ORDER_LOOP), (130, MEQN_ORDER_LOOP), (5, MEQN_ORDER_ANY)], ids=["5-loop", "130-loop", "5-any"])
def test_carried_form_has_the_bits_of_the_callers_loop_over_the_full_range(count, order):
    """ORDER_LOOP, and ORDER_ANY below the 128 elements from which the sliced form runs: the carried form `_c`, the bits of the caller's loop."""
    api = capi.load()
    acc = _Acc(count, count)
    h = acc.case.dispatch(api, 2)
    out, ref = acc.new_out(), acc.new_out()
    acc.accumulate(api, h, out, order)
    assert api.hip_kernel_name(h, 1).decode().endswith("_c"), api.hip_kernel_name(h, 1)
    api.hip_set_async(1)
    keep = []
    for i in range(count):
        keep.append(acc.param(ref, i))
        capi.Api.call(h, keep[-1][0])
    api.hip_sync(); api.hip_set_async(0); api.check()
    assert np.array_equal(bits_of(acc.host(out)), bits_of(acc.host(ref)))
    assert not np.array_equal(bits_of(acc.host(out)), bits_of(acc.acc0))


@pytest.mark.parametrize("count", [5, 130])
def test_carried_bf16_accumulator_has_the_bits_of_the_callers_loop(count):
    """dbeta += dout with a BF16 accumulator (meqn_acc_helpers: dbeta_bf16_acc): the accumulator is rounded to bf16 after every element and reloaded.  The
    accumulator's start values and the addends hold bf16 denormal codes: the carried form loads them as signed zeros, as each single call of the loop does."""
    import torch
    from meqn_acc_helpers import dbeta
    api = capi.load()
    m, n, ld = 64, 32, 64
    tree, shapes, out_shape, carried = dbeta(DT.BF16, m, n, ld, DT.BF16)
    case = mp.EqCase(tree, shapes, out_shape, "meqn_jit_e")
    h = case.dispatch(api, 2)
    per = round16(ld * n * 2 + 48) // 2
    dout = np.full(count * per, mp._nan(DT.BF16), dtype=np.uint16)
    for i in range(count):
        dout[i * per: i * per + ld * n] = mp.table("wide", DT.BF16, m, n, 300 + i).ravel()
    acc0 = mp.table("wide", DT.BF16, m, n, 299).ravel()
    assert ((acc0 & 0x7f80) == 0).any() and ((dout & 0x7f80) == 0).any()
    guard = np.full(64, mp._gap(DT.BF16), dtype=np.uint16)
    d_dout, pad = mp.upload(dout), torch.zeros(16, dtype=torch.float32, device="cuda:0")
    strides = [0, 0, 0, per * 2, 0, 0]

    def param(out, i):
        inputs = (capi.MatrixArg * 6)()
        for k in (0, 1, 2, 4):
            inputs[k].primary = pad.data_ptr()
        inputs[3].primary = d_dout.data_ptr() + i * per * 2
        inputs[5].primary = out.data_ptr() + guard.size * 2
        p = capi.MeqnParam()
        p.inputs = inputs
        p.output.primary = inputs[5].primary
        return p, inputs
    out, ref = (mp.upload(np.concatenate([guard, acc0, guard])) for _ in range(2))
    p, keep = param(out, 0)
    api.hip_meqn_batch_strided_accumulate(h, C.byref(p), count, 6, (ll * 6)(*strides), 0, None, MEQN_ORDER_LOOP)
    api.hip_sync(); api.check()
    assert api.hip_kernel_name(h, 1).decode().endswith("_c"), api.hip_kernel_name(h, 1)
    api.hip_set_async(1)
    held = []
    for i in range(count):
        held.append(param(ref, i))
        capi.Api.call(h, held[-1][0])
    api.hip_sync(); api.hip_set_async(0); api.check()
    got, want = out.cpu().numpy().view(np.uint16), ref.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want)
    assert np.array_equal(got[:64], guard) and np.array_equal(got[-64:], guard)
    assert not ((got[64:-64] & 0x7f80 == 0) & (got[64:-64] & 0x7f != 0)).any()        # no denormal survives a flushing load and a flushing store


def test_sliced_form_lies_inside_the_ref64_sum_bound_over_the_full_range():
    """ORDER_ANY on 130 elements (8 slices): every output against the float64 sum of the addends, each addend with its own ref64 bound, the sum of count + 1
    terms in any order: sum e_i + (k + 1) 2^-24 sum |t_i| + k FLT_MIN."""
    api = capi.load()
    count = 130
    acc = _Acc(count, 77)
    h = acc.case.dispatch(api, 2)
    out = acc.new_out()
    acc.accumulate(api, h, out, MEQN_ORDER_ANY)
    assert api.hip_kernel_name(h, 1).decode().endswith("_s"), api.hip_kernel_name(h, 1)
    addend = ("b", capi.BINARY.MUL, 0, acc.tree[3], mp.A(3))                            # (a * inp + b) * dout, the product rounded before it is added
    t, e = acc.acc0.reshape(64, 64).astype(np.float64), np.zeros((64, 64))
    mag = np.abs(t)
    for i in range(count):
        ti, ei = mp.ref64(addend, acc.shapes[:4], acc.element(i))
        t, e, mag = t + ti, e + ei, mag + np.abs(ti)
    k = count + 1
    e = e + (k + 1) * mp.U * mag + k * FLT_MIN
    got = acc.host(out).reshape(64, 64).astype(np.float64)
    stats = {}
    mp.assert_ref64(got, t, e, DT.F32, what="sliced form", stats=stats)
    share = mp.empty_share(t, e, DT.F32)
    print(f"sliced form, {count} elements: worst err / bound {stats['ratio']:.3f}, empty share {share:.3f}")
    assert share <= mp.MAX_EMPTY
