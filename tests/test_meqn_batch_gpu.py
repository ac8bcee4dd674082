"""Strided batches of matrix equations on the GPU (libxsmm_hip_meqn_batch_strided): the fused kernels' batched forms, the batched step chain,
host-resident scalars, chunking of the chain's workspace and stream-ordered mode.  The yardstick is the caller's loop of single calls on the same
stepped pointers (bit for bit where the single call is bit-identical to itself) and the oracle composition of tests/test_meqn.py."""
import ctypes as C

import numpy as np
import pytest

import test_meqn as tm
from helpers import normf_rel, rand_values
from libxsmm_amd import capi
from libxsmm_amd.capi import BINARY, BINARY_FLAG, DT, UNARY, UNARY_FLAG
from meqn_batch_helpers import ESIZE, NPDT, Batch, round16

pytestmark = pytest.mark.gpu
ll = C.c_longlong
# a mix of stepped and shared (stride 0) input positions per case
SHARED = {"simple": (1,), "layernorm_affine": (3, 4), "bias_relu_bf16": (0,), "ternary_muladd": (2,), "mixed_precision": (2,), "dot_to_scalar": (1,)}


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.copy()).to("cuda:0")


def _host(t, dt):
    return t.cpu().numpy().view(NPDT[dt])


def _param(ptrs, out, out_aux=None, ops=None, secondary=None):
    inputs = (capi.MatrixArg * len(ptrs))()
    for i, v in enumerate(ptrs):
        inputs[i].primary = v
        if secondary and i in secondary:
            inputs[i].secondary = secondary[i]
    p = capi.MeqnParam()
    p.inputs = inputs
    if ops is not None:
        p.ops_args = ops
    p.output.primary = out
    if out_aux is not None:
        p.output.secondary = out_aux
    return p, inputs


def _batch(api, h, p, count, strides, s_out, s_aux=0, s_ops=None):
    sin = (ll * len(strides))(*strides)
    sops = (ll * len(s_ops))(*s_ops) if s_ops else None
    api.hip_meqn_batch_strided(h, C.byref(p), count, len(strides), sin, s_out, s_aux, len(s_ops) if s_ops else 0, sops)


def _dispatch(api, name, jit):
    tree, shapes, out_shape = tm.CASES[name]
    api.hip_set_jit(jit)
    h = api.dispatch_meqn(tm.build(api, tree, shapes), capi.MeqnArgShape(*out_shape))
    api.hip_set_jit(1)
    assert h
    return h


def _loop(api, h, ptrs, strides, out, s_out, count, out_aux=None, s_aux=0, ops_of=None):
    """The caller's loop: one stream-ordered single call per element on the stepped pointers."""
    api.hip_set_async(1)
    keep = []
    for i in range(count):
        p, inputs = _param([v + i * s for v, s in zip(ptrs, strides)], out + i * s_out, None if out_aux is None else out_aux + i * s_aux,
                           ops=ops_of(i) if ops_of else None)
        keep.append((p, inputs))
        capi.Api.call(h, p)
    api.hip_sync()
    api.hip_set_async(0)
    api.check()


@pytest.mark.parametrize("count", [1, 7, 4096])
@pytest.mark.parametrize("name", sorted(tm.FUSABLE))
def test_fused_batch_equals_the_loop_of_single_calls(name, count):
    import torch
    api = capi.load()
    tree, shapes, out_shape = tm.CASES[name]
    h = _dispatch(api, name, 2)
    assert api.hip_kernel_name(h, 0).decode().startswith("meqn_jit")
    b = Batch(shapes, out_shape, count, shared=SHARED.get(name, ()), seed=count)
    dev = [_dev(a) for a in b.inputs]
    ptrs = [d.data_ptr() for d in dev]
    odt = out_shape[3]
    tdt = torch.int16 if odt == DT.BF16 else torch.float32
    out = torch.zeros(b.out_elems, dtype=tdt, device="cuda:0")
    ref = torch.zeros(b.out_elems, dtype=tdt, device="cuda:0")
    p, _keep = _param(ptrs, out.data_ptr())
    api.hip_launch_count(1)
    _batch(api, h, p, count, b.strides, b.out_stride)
    api.check()
    assert api.hip_launch_count(0) == 1
    assert api.hip_kernel_name(h, 1).decode().endswith("_b"), api.hip_kernel_name(h, 1)
    assert api.hip_kernel_name(h, 0).decode().startswith("meqn_jit") and not api.hip_kernel_name(h, 0).decode().endswith("_b")
    _loop(api, h, ptrs, b.strides, ref.data_ptr(), b.out_stride, count)
    assert torch.equal(out, ref)
    got = _host(out, odt)
    for i in {0, count - 1}:                                   # the composition, on the first and last element
        want = tm.evaluate(tree, shapes, [b.element(k, i) for k in range(len(shapes))], out_shape)
        g = b.out_element(got, i)
        if name in tm.BY_NORM:
            assert normf_rel(tm._valid(want, out_shape), tm._valid(g, out_shape), odt) < tm.BY_NORM[name]
        else:
            assert np.array_equal(tm._valid(g, out_shape), tm._valid(want, out_shape))


@pytest.mark.parametrize("form", ["elementwise", "phased"])
def test_count_beyond_the_grid_limit_of_one_dimension(form):
    """70 000 elements of an 8 x 1 tree: more elements than a y (element-wise form) grid dimension holds."""
    import torch
    api = capi.load()
    count, m = 70000, 8
    idx = api.meqn_create()
    md = capi.MeqnMetadata(idx, -1)
    if form == "elementwise":
        assert api.meqn_push_back_binary_op(md, BINARY.ADD, DT.F32, 0) == 0
        out_shape = (m, 1, m, DT.F32)
    else:
        assert api.meqn_push_back_unary_op(md, UNARY.REDUCE_X_OP_ADD, DT.F32, UNARY_FLAG.REDUCE_ROWS) == 0
        assert api.meqn_push_back_unary_op(md, UNARY.REDUCE_X_OP_ADD, DT.F32, UNARY_FLAG.REDUCE_COLS) == 0
        assert api.meqn_push_back_binary_op(md, BINARY.ADD, DT.F32, 0) == 0
        out_shape = (1, 1, 1, DT.F32)
    for k in range(2):
        assert api.meqn_push_back_arg(capi.MeqnMetadata(idx, k), capi.MeqnArgShape(m, 1, m, DT.F32), tm.SINGULAR) == 0
    api.hip_set_jit(2)
    h = api.dispatch_meqn(idx, capi.MeqnArgShape(*out_shape))
    api.hip_set_jit(1)
    assert h and api.hip_kernel_name(h, 0).decode().startswith("meqn_jit_" + ("e" if form == "elementwise" else "r"))
    rng = np.random.default_rng(70)
    x, y = (rand_values(rng, m * count, DT.F32) for _ in range(2))
    dx, dy = _dev(x), _dev(y)
    s_out = 32 if form == "elementwise" else 16
    out = torch.full((count * s_out // 4,), -1.0, dtype=torch.float32, device="cuda:0")
    p, _keep = _param([dx.data_ptr(), dy.data_ptr()], out.data_ptr())
    api.hip_launch_count(1)
    _batch(api, h, p, count, [m * 4, m * 4], s_out)
    api.check()
    assert api.hip_launch_count(0) == 1 and api.hip_kernel_name(h, 1).decode().endswith("_b")
    got = out.cpu().numpy().reshape(count, s_out // 4)
    s = (x.reshape(count, m) + y.reshape(count, m))
    if form == "elementwise":
        assert np.array_equal(got[:, :m], s) and (got[:, m:] == -1.0).all()
    else:
        assert np.abs(got[:, 0] - s.astype(np.float64).sum(axis=1)).max() <= 1e-5 * np.abs(s).sum(axis=1).max()
        assert (got[:, 1:] == -1.0).all()


def _softmax_equation(api, m, n, ld, dt):
    """The forward tree of samples/equation/equation_softmax.c:527-538: argument 0 is the scratch the DUMP node (op argument 31) writes."""
    idx = api.meqn_create()
    OP, DUMP_AT = capi.MeqnMetadata(idx, -1), capi.MeqnMetadata(idx, 31)
    rows, cols = UNARY_FLAG.REDUCE_ROWS, UNARY_FLAG.REDUCE_COLS
    assert api.meqn_push_back_binary_op(OP, BINARY.MUL, DT.F32, BINARY_FLAG.BCAST_SCALAR_IN_1) == 0
    assert api.meqn_push_back_arg(capi.MeqnMetadata(idx, 0), capi.MeqnArgShape(m, n, m, DT.F32), tm.SINGULAR) == 0
    assert api.meqn_push_back_unary_op(OP, UNARY.RECIPROCAL, DT.F32, 0) == 0
    assert api.meqn_push_back_unary_op(OP, UNARY.REDUCE_X_OP_ADD, DT.F32, rows) == 0
    assert api.meqn_push_back_unary_op(OP, UNARY.REDUCE_X_OP_ADD, DT.F32, cols) == 0
    assert api.meqn_push_back_unary_op(DUMP_AT, UNARY.DUMP, DT.F32, 0) == 0
    assert api.meqn_push_back_unary_op(OP, UNARY.EXP, DT.F32, 0) == 0
    assert api.meqn_push_back_binary_op(OP, BINARY.SUB, DT.F32, BINARY_FLAG.BCAST_SCALAR_IN_1) == 0
    assert api.meqn_push_back_arg(capi.MeqnMetadata(idx, 1), capi.MeqnArgShape(m, n, ld, dt), tm.SINGULAR) == 0
    assert api.meqn_push_back_unary_op(OP, UNARY.REDUCE_X_OP_MAX, DT.F32, rows) == 0
    assert api.meqn_push_back_unary_op(OP, UNARY.REDUCE_X_OP_MAX, DT.F32, cols) == 0
    assert api.meqn_push_back_arg(capi.MeqnMetadata(idx, 1), capi.MeqnArgShape(m, n, ld, dt), tm.SINGULAR) == 0
    return idx


@pytest.mark.parametrize("jit", [0, 2], ids=["tpp_chain", "fused_jit"])
@pytest.mark.parametrize("dt", [DT.F32, DT.BF16], ids=["f32", "bf16"])
def test_softmax_forward_with_its_dump_scratch_stepped_with_argument_0(dt, jit):
    import torch
    api = capi.load()
    m, n, ld, count = 64, 12, 128, 33
    api.hip_set_jit(jit)
    h = api.dispatch_meqn(_softmax_equation(api, m, n, ld, dt), capi.MeqnArgShape(m, n, ld, dt))
    api.hip_set_jit(1)
    assert h and api.hip_kernel_name(h, 0).decode().startswith("meqn_jit_r") == (jit == 2)
    x = rand_values(np.random.default_rng(33), ld * n * count, dt)
    dx = _dev(x)
    sx, sk, so = ld * n * ESIZE[dt], round16(m * n * 4 + 64), round16(ld * n * ESIZE[dt] + 16)
    tdt = torch.int16 if dt == DT.BF16 else torch.float32
    kept, kept2 = (torch.zeros(count * sk // 4, dtype=torch.float32, device="cuda:0") for _ in range(2))
    out, out2 = (torch.zeros(count * so // ESIZE[dt], dtype=tdt, device="cuda:0") for _ in range(2))
    ops = (capi.MatrixOpArg * 32)()
    ops[31].primary = kept.data_ptr()
    p, _keep = _param([kept.data_ptr(), dx.data_ptr()], out.data_ptr(), ops=ops)
    s_ops = [0] * 31 + [sk]
    api.hip_launch_count(1)
    _batch(api, h, p, count, [sk, sx], so, s_ops=s_ops)
    api.check()
    assert api.hip_launch_count(0) == 1
    assert api.hip_kernel_name(h, 1).decode() == ("meqn_tpp_chain" if jit == 0 else api.hip_kernel_name(h, 0).decode() + "_b")

    def ops_of(i):
        o = (capi.MatrixOpArg * 32)()
        o[31].primary = kept2.data_ptr() + i * sk
        return o
    _loop(api, h, [kept2.data_ptr(), dx.data_ptr()], [sk, sx], out2.data_ptr(), so, count, ops_of=ops_of)
    assert torch.equal(out, out2) and torch.equal(kept, kept2)
    got, k = _host(out, dt), kept.cpu().numpy()
    for i in range(count):
        xf = tm._valid(tm._f32(x[i * ld * n:(i + 1) * ld * n], dt), (m, n, ld, dt)).astype(np.float64)
        ex = np.exp(xf - xf.max())
        want = ex / ex.sum()
        g = tm._valid(tm._f32(got[i * so // ESIZE[dt]:][:ld * n], dt), (m, n, ld, dt))
        assert np.abs(k[i * sk // 4:][:m * n].reshape(n, m) - ex).max() < 1e-6 * ex.max()
        assert np.linalg.norm(g - want) / np.linalg.norm(want) < (4e-3 if dt == DT.BF16 else 1e-6)


@pytest.mark.parametrize("jit", [0, 2], ids=["tpp_chain", "fused_jit"])
def test_per_element_scalars_in_host_memory(jit):
    """Blocking mode: a 1 x 1 input per element on the caller's stack / heap (stride 16 bytes), and a 1 x 1 result per element in host memory."""
    import torch
    api = capi.load()
    count = 7
    tree, shapes, out_shape = tm.CASES["mixed_precision"]
    h = _dispatch(api, "mixed_precision", jit)
    b = Batch(shapes, out_shape, count, seed=5)
    dev = [_dev(a) for a in b.inputs[:2]]
    scal = np.zeros(count * 4, dtype=np.float32)                             # plain host memory, one value every 16 bytes
    scal[::4] = b.inputs[2][::b.strides[2] // 4][:count]
    out = torch.zeros(b.out_elems, dtype=torch.int16, device="cuda:0")
    p, _keep = _param([dev[0].data_ptr(), dev[1].data_ptr(), scal.ctypes.data], out.data_ptr())
    _batch(api, h, p, count, [b.strides[0], b.strides[1], 16], b.out_stride)
    api.check()
    got = _host(out, DT.BF16)
    for i in range(count):
        want = tm.evaluate(tree, shapes, [b.element(0, i), b.element(1, i), scal[4 * i:4 * i + 1].copy()], out_shape)
        assert np.array_equal(tm._valid(b.out_element(got, i), out_shape), tm._valid(want, out_shape)), i
    # one number per element, written to host memory 8 bytes apart
    tree, shapes, out_shape = tm.CASES["dot_to_scalar"]
    h = _dispatch(api, "dot_to_scalar", jit)
    b = Batch(shapes, out_shape, count, seed=6)
    dev = [_dev(a) for a in b.inputs]
    res = np.full(2 * count, -5.0, dtype=np.float32)
    p, _keep = _param([d.data_ptr() for d in dev], res.ctypes.data)
    _batch(api, h, p, count, b.strides, 8)
    api.check()
    for i in range(count):
        want = tm.evaluate(tree, shapes, [b.element(k, i) for k in range(2)], out_shape)
        assert abs(res[2 * i] - want[0]) <= tm.BY_NORM["dot_to_scalar"] * abs(want[0]), i
        assert res[2 * i + 1] == -5.0


@pytest.mark.parametrize("name", sorted(tm.CASES))
def test_chain_batch_of_every_case_matches_the_composition(name):
    """Every test_meqn.py case as the step chain (JIT off): each step runs once for all elements; MATMUL nodes through the GEMM handle's strided batch."""
    import torch
    api = capi.load()
    tree, shapes, out_shape = tm.CASES[name]
    h = _dispatch(api, name, 0)
    assert api.hip_kernel_name(h, 0).decode() == "meqn_tpp_chain"
    count = 7
    b = Batch(shapes, out_shape, count, shared=SHARED.get(name, ()), seed=11)
    dev = [_dev(a) for a in b.inputs]
    odt = out_shape[3]
    out = torch.zeros(b.out_elems, dtype=torch.int16 if odt == DT.BF16 else torch.float32, device="cuda:0")
    p, _keep = _param([d.data_ptr() for d in dev], out.data_ptr())
    api.hip_launch_count(1)
    _batch(api, h, p, count, b.strides, b.out_stride)
    api.check()
    launches = api.hip_launch_count(0)
    if "matmul" not in name:
        assert launches == 1
    assert api.hip_kernel_name(h, 1).decode() == "meqn_tpp_chain"
    got = _host(out, odt)
    for i in range(count):
        want = tm.evaluate(tree, shapes, [b.element(k, i) for k in range(len(shapes))], out_shape)
        g = b.out_element(got, i)
        if name in tm.BY_NORM:
            assert normf_rel(tm._valid(want, out_shape), tm._valid(g, out_shape), odt) < tm.BY_NORM[name], i
        else:
            assert np.array_equal(tm._valid(g, out_shape), tm._valid(want, out_shape)), i


def test_chain_batch_with_gather_nodes_shares_the_index_list():
    import torch
    api = capi.load()
    m, n, ld, big_n, count = 37, 21, 40, 105, 9
    rng = np.random.default_rng(3)
    X = rand_values(rng, ld * big_n * count, DT.F32)
    cols = rng.permutation(big_n)[:n].astype(np.uint32)
    idx = api.meqn_create()
    md = capi.MeqnMetadata(idx, -1)
    assert api.meqn_push_back_unary_op(md, UNARY.REDUCE_X_OP_ADD, DT.F32, UNARY_FLAG.REDUCE_COLS) == 0
    assert api.meqn_push_back_unary_op(md, UNARY.GATHER, DT.F32, UNARY_FLAG.GS_COLS | UNARY_FLAG.IDX_SIZE_4BYTES) == 0
    assert api.meqn_push_back_arg(capi.MeqnMetadata(idx, 0), capi.MeqnArgShape(m, n, ld, DT.F32), tm.SINGULAR) == 0
    h = api.dispatch_meqn(idx, capi.MeqnArgShape(m, 1, ld, DT.F32))
    assert h
    xd, idd = _dev(X), _dev(cols.view(np.int32))
    out = torch.zeros(ld * count, dtype=torch.float32, device="cuda:0")
    p, _keep = _param([xd.data_ptr()], out.data_ptr(), secondary={0: idd.data_ptr()})
    api.hip_launch_count(1)
    _batch(api, h, p, count, [ld * big_n * 4], ld * 4)
    api.check()
    assert api.hip_launch_count(0) == 1
    got = out.cpu().numpy().reshape(count, ld)[:, :m].astype(np.float64)
    for i in range(count):
        Xf = X[i * ld * big_n:(i + 1) * ld * big_n].reshape(big_n, ld)[:, :m].astype(np.float64)
        gold = Xf[cols.astype(np.int64)].sum(axis=0)
        assert np.sqrt(((got[i] - gold) ** 2).sum() / (gold ** 2).sum()) < 1e-6


@pytest.mark.parametrize("per_element_index", [False, True], ids=["shared_index", "index_per_element"])
def test_chain_batch_with_a_scatter_head(per_element_index):
    import torch
    api = capi.load()
    m, n, ld, big_n, count = 40, 13, 48, 40, 6
    shapes = [(m, n, ld, DT.F32), (m, n, m, DT.F32)]
    rng = np.random.default_rng(4)
    idx = api.meqn_create()
    md = capi.MeqnMetadata(idx, -1)
    assert api.meqn_push_back_unary_op(md, UNARY.SCATTER, DT.F32, UNARY_FLAG.GS_COLS | UNARY_FLAG.IDX_SIZE_4BYTES) == 0
    assert api.meqn_push_back_binary_op(md, BINARY.ADD, DT.F32, 0) == 0
    for k in range(2):
        assert api.meqn_push_back_arg(capi.MeqnMetadata(idx, k), capi.MeqnArgShape(*shapes[k]), tm.SINGULAR) == 0
    h = api.dispatch_meqn(idx, capi.MeqnArgShape(m, big_n, ld, DT.F32))
    assert h
    b = Batch(shapes, (m, big_n, ld, DT.F32), count, seed=12)
    dev = [_dev(a) for a in b.inputs]
    nidx = count if per_element_index else 1
    cols = np.concatenate([rng.permutation(big_n)[:16].astype(np.uint32) for _ in range(nidx)])      # 16 entries per list: 64-byte stride
    before = rand_values(rng, b.out_elems, DT.F32)
    out, idd = _dev(before), _dev(cols.view(np.int32))
    p, _keep = _param([d.data_ptr() for d in dev], out.data_ptr(), out_aux=idd.data_ptr())
    api.hip_launch_count(1)
    _batch(api, h, p, count, b.strides, b.out_stride, s_aux=64 if per_element_index else 0)
    api.check()
    if not per_element_index:
        assert api.hip_launch_count(0) == 1
    got = out.cpu().numpy()
    for i in range(count):
        c = cols[16 * i:16 * i + n] if per_element_index else cols[:n]
        A, B = (tm._valid(b.element(k, i), shapes[k]) for k in range(2))
        gold = tm._mat(b.out_element(before, i), m, big_n, ld, DT.F32)[0].copy()
        gold[c.astype(np.int64)] = A + B                                      # the f32 sum
        assert np.array_equal(tm._mat(b.out_element(got, i), m, big_n, ld, DT.F32)[0], gold), i


def test_chain_batch_with_a_relu_bitmask_head_steps_output_secondary():
    import torch
    api = capi.load()
    m, n, count = 64, 16, 5
    shapes = [(m, n, m, DT.F32), (m, n, m, DT.F32)]
    idx = api.meqn_create()
    md = capi.MeqnMetadata(idx, -1)
    assert api.meqn_push_back_unary_op(md, UNARY.RELU, DT.F32, UNARY_FLAG.BITMASK_2BYTEMULT) == 0
    assert api.meqn_push_back_binary_op(md, BINARY.ADD, DT.F32, 0) == 0
    for k in range(2):
        assert api.meqn_push_back_arg(capi.MeqnMetadata(idx, k), capi.MeqnArgShape(*shapes[k]), tm.SINGULAR) == 0
    h = api.dispatch_meqn(idx, capi.MeqnArgShape(m, n, m, DT.F32))
    assert h
    b = Batch(shapes, (m, n, m, DT.F32), count, seed=13)
    dev = [_dev(a) for a in b.inputs]
    mask_bytes, s_mask = m // 8 * n, round16(m // 8 * n + 16)
    out, out2 = (torch.zeros(b.out_elems, dtype=torch.float32, device="cuda:0") for _ in range(2))
    mask, mask2 = (torch.zeros(count * s_mask, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    ptrs = [d.data_ptr() for d in dev]
    p, _keep = _param(ptrs, out.data_ptr(), out_aux=mask.data_ptr())
    api.hip_launch_count(1)
    _batch(api, h, p, count, b.strides, b.out_stride, s_aux=s_mask)
    api.check()
    assert api.hip_launch_count(0) == 1
    _loop(api, h, ptrs, b.strides, out2.data_ptr(), b.out_stride, count, out_aux=mask2.data_ptr(), s_aux=s_mask)
    assert torch.equal(out, out2) and torch.equal(mask, mask2)
    mk = mask.cpu().numpy().reshape(count, s_mask)
    assert mk[:, :mask_bytes].any() and not mk[:, mask_bytes:].any()
    got = out.cpu().numpy()
    for i in range(count):
        s = b.element(0, i) + b.element(1, i)
        assert np.array_equal(b.out_element(got, i), np.where(s <= 0, 0, s).astype(np.float32))


def test_chain_batch_with_a_brgemm_node():
    import torch
    api = capi.load()
    m, n, k, blocks, count = 32, 16, 24, 5, 6
    idx = api.meqn_create()
    md = lambda pos=-1: capi.MeqnMetadata(idx, pos)    # noqa: E731
    assert api.meqn_push_back_binary_op(md(), BINARY.ADD, DT.F32, 0) == 0
    assert api.meqn_push_back_arg(md(0), capi.MeqnArgShape(m, n, m, DT.F32), tm.SINGULAR) == 0
    assert api.meqn_push_back_binary_op(md(3), BINARY.BRGEMM, DT.F32, 0) == 0
    assert api.meqn_push_back_arg(md(2), capi.MeqnArgShape(m, k, m, DT.F32), capi.MatrixArgAttributes(1, 3, blocks, m * k * 4)) == 0
    assert api.meqn_push_back_arg(md(3), capi.MeqnArgShape(k, n, k, DT.F32), capi.MatrixArgAttributes(1, 3, blocks, k * n * 4)) == 0
    h = api.dispatch_meqn(idx, capi.MeqnArgShape(m, n, m, DT.F32))
    assert h
    rng = np.random.default_rng(9)
    A0 = rand_values(rng, m * n * count, DT.F32)
    As = rand_values(rng, m * k * blocks * count, DT.F32)
    Bs = rand_values(rng, k * n * blocks, DT.F32)                              # B shared by every element
    dev = [_dev(A0), _dev(As), _dev(Bs)]
    out = torch.zeros(m * n * count, dtype=torch.float32, device="cuda:0")
    nblk = C.c_ulonglong(blocks)
    ops = (capi.MatrixOpArg * 4)()
    ops[3].tertiary = C.addressof(nblk)
    inputs = (capi.MatrixArg * 4)()
    inputs[0].primary, inputs[2].primary, inputs[3].primary = dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr()
    p = capi.MeqnParam()
    p.inputs, p.ops_args = inputs, ops
    p.output.primary = out.data_ptr()
    sin = (ll * 4)(m * n * 4, 0, m * k * blocks * 4, 0)
    api.hip_meqn_batch_strided(h, C.byref(p), count, 4, sin, m * n * 4, 0, 4, None)
    api.check()
    got = out.cpu().numpy().astype(np.float64)
    Bb = Bs.astype(np.float64).reshape(blocks, n, k)
    for i in range(count):
        Ab = As[i * m * k * blocks:(i + 1) * m * k * blocks].astype(np.float64).reshape(blocks, k, m)
        gold = A0[i * m * n:(i + 1) * m * n].astype(np.float64).reshape(n, m) + sum(Bb[r] @ Ab[r] for r in range(blocks))
        g = got[i * m * n:(i + 1) * m * n].reshape(n, m)
        assert np.sqrt(((g - gold) ** 2).sum() / (gold ** 2).sum()) < 2e-6, i
    sops = (ll * 4)(0, 0, 0, 8)                                                # the block count is shared: a stride on it is refused
    api.hip_meqn_batch_strided(h, C.byref(p), count, 4, sin, m * n * 4, 0, 4, sops)
    assert api.hip_get_last_error() == -3
    api.hip_clear_last_error()


def test_chain_batch_is_chunked_to_bound_the_workspace():
    """"simple" as a chain: four intermediate slots of 40 x 24 x 8 bytes per element -> 8738 elements per 256 MiB chunk; 20 000 elements are three chunks,
    one launch each."""
    import torch
    api = capi.load()
    tree, shapes, out_shape = tm.CASES["simple"]
    h = _dispatch(api, "simple", 0)
    count = 20000
    b = Batch(shapes, out_shape, count, seed=3)
    dev = [_dev(a) for a in b.inputs]
    out = torch.zeros(b.out_elems, dtype=torch.float32, device="cuda:0")
    p, _keep = _param([d.data_ptr() for d in dev], out.data_ptr())
    api.hip_launch_count(1)
    _batch(api, h, p, count, b.strides, b.out_stride)
    api.check()
    chunk = (256 << 20) // (4 * ((40 * 24 * 8 + 255) // 256 * 256))
    assert api.hip_launch_count(0) == -(-count // chunk) == 3
    got = out.cpu().numpy()
    m, n, ld, _ = out_shape
    for i in (0, chunk - 1, chunk, 2 * chunk, count - 1):
        a = [tm._valid(b.element(k, i), shapes[k]) for k in range(4)]
        want = (a[0] + (a[1] + np.float32(1))) * (a[2] * a[2] + a[3])
        assert np.array_equal(tm._valid(b.out_element(got, i), out_shape), want), i


@pytest.mark.parametrize("jit", [0, 2], ids=["tpp_chain", "fused_jit"])
def test_stream_ordered_and_coalescing_batches_give_the_same_bytes(jit):
    import torch
    api = capi.load()
    name = "layernorm_affine"
    tree, shapes, out_shape = tm.CASES[name]
    h = _dispatch(api, name, jit)
    count = 300
    b = Batch(shapes, out_shape, count, shared=SHARED[name], seed=8)
    dev = [_dev(a) for a in b.inputs]
    ptrs = [d.data_ptr() for d in dev]
    outs = [torch.zeros(b.out_elems, dtype=torch.int16, device="cuda:0") for _ in range(3)]
    for mode, out in zip((0, 1, 2), outs):                                   # blocking, stream-ordered, coalescing
        api.hip_set_async(mode)
        p, _keep = _param(ptrs, out.data_ptr())
        _batch(api, h, p, count, b.strides, b.out_stride)
        api.hip_sync()
        api.check()
    api.hip_set_async(0)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    got = _host(outs[1], DT.BF16)
    want = tm.evaluate(tree, shapes, [b.element(k, count - 1) for k in range(len(shapes))], out_shape)
    assert np.array_equal(tm._valid(b.out_element(got, count - 1), out_shape), tm._valid(want, out_shape))
