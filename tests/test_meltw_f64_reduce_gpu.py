"""The all-f64 reduction TPPs on the GPU: over rows and columns, over listed columns, with a recorded argop, through the
single call, the strided batch, the stream-ordered and coalescing modes, host operands and matrix equations.

The yardstick is the reference's f64 loop [ref: src/generator_mateltwise_reference_impl.c:1143-1295] restated serially in numpy doubles below
(`serial`), with one deviation: the x^2 sums are stored (the reference's loop leaves zeros there).  MAX / MIN / ABSMAX and the sums the kernels
add in serial order are compared bit for bit; other sums within 1e-12 * sum |x| per output.  The data reach beyond the f32 range (+-1e300) and
into the subnormals, so an f32 accumulator or an f32 start value would show."""
import ctypes as C

import numpy as np
import pytest

from libxsmm_amd import capi
from libxsmm_amd.capi import DT, UNARY, UNARY_FLAG

pytestmark = pytest.mark.gpu
FLT_MAX = float(np.finfo(np.float32).max)
ADD_T = (UNARY.REDUCE_X_OP_ADD, UNARY.REDUCE_X2_OP_ADD, UNARY.REDUCE_X_X2_OP_ADD)
CMP_T = (UNARY.REDUCE_X_OP_MAX, UNARY.REDUCE_X_OP_MIN, UNARY.REDUCE_X_OP_ABSMAX)
LISTED_T = (UNARY.REDUCE_COLS_IDX_OP_ADD, UNARY.REDUCE_COLS_IDX_OP_MAX, UNARY.REDUCE_COLS_IDX_OP_MIN)


def _abs(a):                      # LIBXSMM_ABS: 0 <= a ? a : -a
    return np.where(0.0 <= a, a, -a)


def serial(x, m, n, ldi, typ, rows, init=None, cols=None):
    """The reference's loop over one matrix (flat, ld ldi) in doubles, vectorised over the results: returns (x results, x^2 results)."""
    X = x[:ldi * n].reshape(n, ldi)[:, :m].T if n else x.reshape(-1, ldi)[:, :m].T       # m x n view
    if cols is not None:
        X = X[:, np.asarray(cols, dtype=np.int64)]
    steps = [X[i, :] for i in range(m)] if rows else [X[:, j] for j in range(X.shape[1])]
    size = n if rows else m
    op = {UNARY.REDUCE_X_OP_MAX: "max", UNARY.REDUCE_COLS_IDX_OP_MAX: "max", UNARY.REDUCE_X_OP_MIN: "min", UNARY.REDUCE_COLS_IDX_OP_MIN: "min",
          UNARY.REDUCE_X_OP_ABSMAX: "absmax"}.get(typ, "add")
    s2 = np.zeros(size)
    if op == "add":
        s = np.zeros(size)
        for v in steps:
            s = s + v
            with np.errstate(over="ignore"):          # x^2 of +-1e300 is inf where only the x sums are checked
                s2 = s2 + v * v
        if init is not None:
            s, s2 = s + init[0], s2 + init[1]
        return s, s2
    if rows:                       # starts at the column's first element; MAX(acc, x), MIN(acc, x), MAX(ABS(acc), ABS(x))
        s = steps[0].copy()
        for v in steps:
            if op == "max":
                s = np.where(s < v, v, s)
            elif op == "min":
                s = np.where(s < v, s, v)
            else:
                a, b = _abs(s), _abs(v)
                s = np.where(a < b, b, a)
        return s, s2
    s = np.full(size, -FLT_MAX if op == "max" else FLT_MAX if op == "min" else 0.0)      # the float bounds, widened
    for v in steps:
        if op == "absmax":
            v = _abs(v)
        s = np.where(v < s, s, v) if op != "min" else np.where(v < s, v, s)
    return s, s2


def argop(x, m, ldi, typ, cols):
    """Recorded columns of the listed / argop loop: a later equal extremum wins (>= / <=)."""
    best = np.full(m, -FLT_MAX if typ in (UNARY.REDUCE_X_OP_MAX, UNARY.REDUCE_COLS_IDX_OP_MAX) else FLT_MAX if typ != UNARY.REDUCE_X_OP_ABSMAX else 0.0)
    arg = np.zeros(m, dtype=np.int64)
    for j in cols:
        v = x[j * ldi:j * ldi + m]
        if typ == UNARY.REDUCE_X_OP_ABSMAX:
            v = _abs(v)
        take = (v <= best) if typ in (UNARY.REDUCE_X_OP_MIN, UNARY.REDUCE_COLS_IDX_OP_MIN) else (v >= best)
        best, arg = np.where(take, v, best), np.where(take, j, arg)
    return best, arg


def data(rng, count, typ=None):
    """Normal values with +-1e300 (+-1e150 where squares are summed), values in (FLT_MAX, 1e300], and subnormals sprinkled in."""
    x = rng.standard_normal(count)
    big = 1e150 if typ in (UNARY.REDUCE_X2_OP_ADD, UNARY.REDUCE_X_X2_OP_ADD) else 1e300
    pick = rng.random(count)
    x = np.where(pick < 0.03, big * np.sign(x), x)
    x = np.where((pick >= 0.03) & (pick < 0.05), rng.uniform(1e39, big, count) * np.sign(x), x)
    x = np.where((pick >= 0.05) & (pick < 0.08), np.sign(x) * 5e-324 * rng.integers(1, 1000, count), x)
    return x


def check(typ, got, want, absx, serial_order):
    """Bit for bit for MAX / MIN / ABSMAX and serially added sums, else within 1e-12 * sum |x| per output."""
    if typ in ADD_T + (UNARY.REDUCE_COLS_IDX_OP_ADD,) and not serial_order:
        assert np.all(np.abs(got - want) <= 1e-12 * absx), np.max(np.abs(got - want) / np.maximum(absx, 1e-300))
    else:
        assert np.array_equal(got, want), (got[got != want][:4], want[got != want][:4])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _sums_abs(x, m, n, ldi, rows, sq=False):
    X = np.abs(x[:ldi * n].reshape(n, ldi)[:, :m])
    with np.errstate(over="ignore"):
        X = X * X if sq else X
    return X.sum(axis=1) if rows else X.sum(axis=0)


def run(typ, m, n, ldi, rows, init=False, batch=1, offset=0, seed=0, mode=0, host=False):
    """Dispatches the f64 TPP, runs it on `batch` matrices (one call, the strided batch, or a loop of calls in async `mode`) and returns
    (inputs, results before, results after, kernel name)."""
    import torch
    api = capi.load()
    rng = np.random.default_rng(seed)
    res = n if rows else m
    ldo = m if not rows else n
    out_elems = (2 * res if typ == UNARY.REDUCE_X_X2_OP_ADD else res) + (ldo - res if typ == UNARY.REDUCE_X_X2_OP_ADD else 0)
    in_elems = ldi * n + 2                   # room for the misaligned base
    X = data(rng, batch * in_elems, typ)
    Y0 = rng.standard_normal(batch * out_elems)
    flags = (UNARY_FLAG.REDUCE_ROWS if rows else UNARY_FLAG.REDUCE_COLS) | (UNARY_FLAG.REDUCE_INIT_ACC if init else 0)
    h = api.dispatch_meltw_unary(typ, capi.UnaryShape(m, n, ldi, ldo, DT.F64, DT.F64, DT.F64), flags)
    assert h, "f64 reduction refused"
    if host:
        dX, Y = X.copy(), Y0.copy()
        px, py = dX.ctypes.data + 8 * offset, Y.ctypes.data
    else:
        dX, Y = _dev(X), _dev(Y0)
        px, py = dX.data_ptr() + 8 * offset, Y.data_ptr()
    p = capi.UnaryParam()
    p.in_.primary, p.out.primary = px, py
    if mode:
        api.hip_set_async(mode)
        keep = []
        for b in range(batch):
            q = capi.UnaryParam(); q.in_.primary, q.out.primary = px + 8 * b * in_elems, py + 8 * b * out_elems; keep.append(q)
            capi.Api.call(h, q)
        api.hip_sync()
        api.hip_set_async(0)
    elif batch == 1:
        capi.Api.call(h, p)
    else:
        api.hip_meltw_unary_batch_strided(h, C.byref(p), batch, 8 * in_elems, 8 * out_elems, 0)
    api.hip_sync(); api.check()
    got = Y.copy() if host else Y.cpu().numpy()
    name = api.hip_kernel_name(h, 1 if batch > 1 and not mode else 0)
    return X, Y0, got, in_elems, out_elems, (name or b"").decode()


def verify(typ, m, n, ldi, rows, X, Y0, got, in_elems, out_elems, batch, offset, init, serial_order):
    res = n if rows else m
    ldo = m if not rows else n
    for b in range(batch):
        x = X[b * in_elems + offset:(b + 1) * in_elems]
        y0, y = Y0[b * out_elems:(b + 1) * out_elems], got[b * out_elems:(b + 1) * out_elems]
        x2_at = ldo if typ == UNARY.REDUCE_X_X2_OP_ADD else 0
        init_v = (y0[:res], y0[x2_at:x2_at + res]) if init and typ in ADD_T else None
        s, s2 = serial(x, m, n, ldi, typ, rows, init_v)
        absx, absx2 = _sums_abs(x, m, n, ldi, rows), _sums_abs(x, m, n, ldi, rows, sq=True)
        if init_v is not None:
            absx, absx2 = absx + np.abs(init_v[0]), absx2 + np.abs(init_v[1])
        if typ != UNARY.REDUCE_X2_OP_ADD:
            check(typ, y[:res], s, absx, serial_order)
        if typ in (UNARY.REDUCE_X2_OP_ADD, UNARY.REDUCE_X_X2_OP_ADD):
            check(typ, y[x2_at:x2_at + res], s2, absx2, serial_order)
        untouched = np.ones(out_elems, bool)
        untouched[:res] = False
        untouched[x2_at:x2_at + res] = False
        assert np.array_equal(y[untouched], y0[untouched]), "wrote outside the results"


SHAPES = [(64, 48, 64, 0), (33, 17, 40, 0), (63, 20, 63, 0), (64, 48, 64, 1)]     # aligned, ragged with ldi 40, odd m, misaligned base


@pytest.mark.parametrize("typ", ADD_T + CMP_T)
@pytest.mark.parametrize("rows", [True, False])
@pytest.mark.parametrize("m,n,ldi,offset", SHAPES)
def test_f64_reduction_single_call(typ, rows, m, n, ldi, offset):
    X, Y0, got, ie, oe, name = run(typ, m, n, ldi, rows, offset=offset, seed=m * 7 + n + offset)
    assert name == ("reduce_vec_f64_kernel" if m % 2 == 0 and offset == 0 else "reduce_f64_kernel"), name      # two doubles per access need an even m and a 16-byte base
    # the column form with one slice and the general kernel add in the serial order
    verify(typ, m, n, ldi, rows, X, Y0, got, ie, oe, 1, offset, False, serial_order=not rows)


@pytest.mark.parametrize("typ", ADD_T)
@pytest.mark.parametrize("rows", [True, False])
@pytest.mark.parametrize("m,n,ldi,offset", [(64, 48, 64, 0), (33, 17, 40, 0), (64, 300, 64, 0)])
def test_f64_reduction_init_acc(typ, rows, m, n, ldi, offset):
    X, Y0, got, ie, oe, _ = run(typ, m, n, ldi, rows, init=True, offset=offset, seed=3)
    verify(typ, m, n, ldi, rows, X, Y0, got, ie, oe, 1, offset, True, serial_order=not rows and n < 256)


@pytest.mark.parametrize("typ", [UNARY.REDUCE_X_OP_ADD, UNARY.REDUCE_X_X2_OP_ADD, UNARY.REDUCE_X_OP_MAX, UNARY.REDUCE_X_OP_MIN, UNARY.REDUCE_X_OP_ABSMAX])
@pytest.mark.parametrize("rows", [True, False])
def test_f64_reduction_of_one_big_matrix(typ, rows):
    """4096 x 4096: over columns the two-pass form (column chunks, then the chunks folded in order)."""
    m = n = 4096
    X, Y0, got, ie, oe, name = run(typ, m, n, m, rows, seed=11)
    if not rows:
        assert name == "reduce_vec_f64_kernel+combine", name
    verify(typ, m, n, m, rows, X, Y0, got, ie, oe, 1, 0, False, serial_order=False)


@pytest.mark.parametrize("typ", [UNARY.REDUCE_X_OP_ADD, UNARY.REDUCE_X_X2_OP_ADD, UNARY.REDUCE_X_OP_ABSMAX, UNARY.REDUCE_X_OP_MIN])
@pytest.mark.parametrize("rows", [True, False])
@pytest.mark.parametrize("m,n,ldi", [(64, 48, 64), (33, 17, 40)])
def test_f64_reduction_strided_batch(typ, rows, m, n, ldi):
    X, Y0, got, ie, oe, _ = run(typ, m, n, ldi, rows, batch=1000, seed=5)
    verify(typ, m, n, ldi, rows, X, Y0, got, ie, oe, 1000, 0, False, serial_order=not rows)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("rows", [True, False])
def test_f64_reduction_async_modes(mode, rows):
    X, Y0, got, ie, oe, _ = run(UNARY.REDUCE_X_X2_OP_ADD, 64, 48, 64, rows, batch=24, seed=7, mode=mode)
    verify(UNARY.REDUCE_X_X2_OP_ADD, 64, 48, 64, rows, X, Y0, got, ie, oe, 24, 0, False, serial_order=not rows)


@pytest.mark.parametrize("typ", [UNARY.REDUCE_X_X2_OP_ADD, UNARY.REDUCE_X_OP_MAX])
@pytest.mark.parametrize("rows", [True, False])
@pytest.mark.parametrize("m,n,ldi,offset", [(64, 48, 64, 0), (33, 17, 40, 1)])
def test_f64_reduction_host_operands(typ, rows, m, n, ldi, offset):
    """Plain host memory (the reference's driver mallocs): staged with 8-byte elements, results copied back."""
    X, Y0, got, ie, oe, _ = run(typ, m, n, ldi, rows, offset=offset, seed=9, host=True)
    verify(typ, m, n, ldi, rows, X, Y0, got, ie, oe, 1, offset, False, serial_order=not rows)


def test_f64_column_max_starts_at_minus_flt_max_and_row_max_at_the_first_element():
    """Every value below -FLT_MAX: the column MAX stays at -FLT_MAX (the reference's start), the row MAX is the largest value (it starts at
    the column's first element); a value in (FLT_MAX, 1e300] is found exactly by both."""
    m, n = 64, 48
    api = capi.load()
    x = -np.linspace(1e300, 1e299, m * n)
    x2 = x.copy(); x2[5 * m + 7] = 3.5e38
    for v, want_cols_7 in ((x, -FLT_MAX), (x2, 3.5e38)):
        for rows in (True, False):
            res = n if rows else m
            h = api.dispatch_meltw_unary(UNARY.REDUCE_X_OP_MAX, capi.UnaryShape(m, n, m, res, DT.F64, DT.F64, DT.F64),
                                         UNARY_FLAG.REDUCE_ROWS if rows else UNARY_FLAG.REDUCE_COLS)
            dX, dY = _dev(v), _dev(np.zeros(res))
            p = capi.UnaryParam(); p.in_.primary, p.out.primary = dX.data_ptr(), dY.data_ptr()
            capi.Api.call(h, p); api.hip_sync(); api.check()
            got = dY.cpu().numpy()
            if rows:
                assert np.array_equal(got, v.reshape(n, m).max(axis=1))
            else:
                assert got[7] == want_cols_7 and np.all(got[np.arange(m) != 7] == -FLT_MAX)


def _listed(typ, m, ldi, ncols, idx8, record, seed, batch=1, host=False, argop_type=None):
    import torch
    api = capi.load()
    rng = np.random.default_rng(seed)
    width = 40
    cols = rng.integers(0, width, ncols)
    X = data(rng, batch * ldi * width)
    flags = UNARY_FLAG.REDUCE_COLS | (UNARY_FLAG.IDX_SIZE_8BYTES if idx8 else UNARY_FLAG.IDX_SIZE_4BYTES) | (UNARY_FLAG.REDUCE_RECORD_ARGOP if record else 0)
    t = argop_type if argop_type is not None else typ
    n = width if argop_type is not None else 0
    h = api.dispatch_meltw_unary(t, capi.UnaryShape(m, n, ldi, m, DT.F64, DT.F64, DT.F64), flags)
    assert h
    idx = cols.astype(np.uint64 if idx8 else np.uint32)
    if host:
        dX, dY, dI = X.copy(), np.zeros(batch * m), idx.copy()
        dA = np.full(m, 77, dtype=np.uint64 if idx8 else np.uint32)
        ptr = lambda a: a.ctypes.data    # noqa: E731
    else:
        dX, dY, dI = _dev(X), _dev(np.zeros(batch * m)), _dev(idx.view(np.int64 if idx8 else np.int32))
        dA = _dev(np.full(m, 77, dtype=np.int64 if idx8 else np.int32))
        ptr = lambda a: a.data_ptr()     # noqa: E731
    cnt = C.c_ulonglong(ncols)
    p = capi.UnaryParam()
    p.in_.primary, p.out.primary = ptr(dX), ptr(dY)
    if argop_type is None:
        p.in_.secondary, p.in_.tertiary = ptr(dI), C.addressof(cnt)
    if record:
        p.out.secondary = ptr(dA)
    if batch == 1:
        capi.Api.call(h, p)
    else:
        api.hip_meltw_unary_batch_strided(h, C.byref(p), batch, 8 * ldi * width, 8 * m, 0)
    api.hip_sync(); api.check()
    got = dY.copy() if host else dY.cpu().numpy()
    got_arg = (dA.copy() if host else dA.cpu().numpy()).astype(np.int64)
    return X, cols if argop_type is None else np.arange(width), got, got_arg, width, api.hip_kernel_name(h, 0).decode()


@pytest.mark.parametrize("typ", LISTED_T)
@pytest.mark.parametrize("idx8", [False, True])
@pytest.mark.parametrize("record", [False, True])
@pytest.mark.parametrize("m,ldi", [(64, 64), (33, 40)])
def test_f64_listed_columns(typ, idx8, record, m, ldi):
    X, cols, got, got_arg, width, name = _listed(typ, m, ldi, 12, idx8, record, seed=m + ldi + 2 * idx8 + record)
    assert name == "reduce_cols_listed_f64_kernel"
    s, _ = serial(X, m, width, ldi, typ, False, cols=cols)
    check(typ, got, s, None, serial_order=True)
    if record and typ != UNARY.REDUCE_COLS_IDX_OP_ADD:
        best, arg = argop(X, m, ldi, typ, cols)
        assert np.array_equal(got, best) and np.array_equal(got_arg, arg)


@pytest.mark.parametrize("typ", CMP_T)
@pytest.mark.parametrize("idx8", [False, True])
def test_f64_column_extremum_records_the_argop(typ, idx8):
    X, cols, got, got_arg, width, name = _listed(None, 64, 64, 0, idx8, True, seed=21 + idx8, argop_type=typ)
    assert name == "reduce_cols_listed_f64_kernel"
    best, arg = argop(X, 64, 64, typ, cols)
    s, _ = serial(X, 64, width, 64, typ, False)
    assert np.array_equal(got, best) and np.array_equal(got, s) and np.array_equal(got_arg, arg)


def test_f64_listed_columns_batched_and_from_host_memory():
    X, cols, got, _, width, _ = _listed(UNARY.REDUCE_COLS_IDX_OP_ADD, 64, 64, 9, False, False, seed=31, batch=1000)
    for b in range(0, 1000, 97):
        s, _ = serial(X[b * 64 * width:(b + 1) * 64 * width], 64, width, 64, UNARY.REDUCE_COLS_IDX_OP_ADD, False, cols=cols)
        assert np.array_equal(got[b * 64:(b + 1) * 64], s)
    X, cols, got, got_arg, width, _ = _listed(UNARY.REDUCE_COLS_IDX_OP_MAX, 33, 40, 12, True, True, seed=32, host=True)
    best, arg = argop(X, 33, 40, UNARY.REDUCE_COLS_IDX_OP_MAX, cols)
    assert np.array_equal(got, best) and np.array_equal(got_arg, arg)


@pytest.mark.parametrize("typ,rows", [(UNARY.REDUCE_X_OP_ADD, True), (UNARY.REDUCE_X_OP_ADD, False), (UNARY.REDUCE_X_OP_MAX, True), (UNARY.REDUCE_X_OP_MAX, False),
                                      (UNARY.REDUCE_X_OP_MIN, False), (UNARY.REDUCE_X_OP_ABSMAX, True), (UNARY.REDUCE_X_OP_ABSMAX, False)])
def test_f64_reduction_pinned_against_the_reference(reference, typ, rows):
    """The reference's own f64 loop (through the built reference library) on the same data: MAX / MIN / ABSMAX bit for bit, sums in bound."""
    m, n, ldi = 33, 17, 40
    X, Y0, got, ie, oe, _ = run(typ, m, n, ldi, rows, seed=41)
    res = n if rows else m
    ref = Y0.copy()
    p = capi.UnaryParam()
    p.in_.primary, p.out.primary = X.ctypes.data, ref.ctypes.data
    reference.lib.xref_reference_meltw_unary(C.byref(p), typ, capi.UnaryShape(m, n, ldi, res, DT.F64, DT.F64, DT.F64),
                                             UNARY_FLAG.REDUCE_ROWS if rows else UNARY_FLAG.REDUCE_COLS)
    check(typ, got[:res], ref[:res], _sums_abs(X, m, n, ldi, rows), serial_order=not rows)


def test_f64_x2_sums_are_stored_where_the_reference_loop_leaves_zeros(reference):
    """The one deviation from the reference's loop: its X2 results are zeroed and copied onto themselves; these are the real sums."""
    m, n, ldi = 64, 48, 64
    X, Y0, got, ie, oe, _ = run(UNARY.REDUCE_X2_OP_ADD, m, n, ldi, False, seed=43)
    ref = Y0.copy()
    p = capi.UnaryParam()
    p.in_.primary, p.out.primary = X.ctypes.data, ref.ctypes.data
    reference.lib.xref_reference_meltw_unary(C.byref(p), UNARY.REDUCE_X2_OP_ADD, capi.UnaryShape(m, n, ldi, m, DT.F64, DT.F64, DT.F64), UNARY_FLAG.REDUCE_COLS)
    assert np.all(ref[:m] == 0.0)
    _, s2 = serial(X, m, n, ldi, UNARY.REDUCE_X2_OP_ADD, False)
    assert np.array_equal(got[:m], s2) and np.any(s2 != 0.0)


@pytest.mark.parametrize("batched", [False, True])
def test_f64_equations_with_reduction_nodes(batched):
    """sqrt(reduce_cols(x^2)) and a max-abs over rows as f64 equations: the fused generated kernel (f32 / bf16 only) declines them, the step
    chain runs the f64 TPPs; single calls and libxsmm_hip_meqn_batch_strided against numpy."""
    import test_meqn as tm
    api = capi.load()
    m, n, ld, count = 64, 48, 66, (300 if batched else 1)
    R, Cf = UNARY_FLAG.REDUCE_ROWS, UNARY_FLAG.REDUCE_COLS
    norms = ("u", UNARY.SQRT, 0, ("u", UNARY.REDUCE_X_OP_ADD, Cf, ("u", UNARY.X2, 0, ("arg", 0))))
    amax = ("u", UNARY.REDUCE_X_OP_ABSMAX, R, ("arg", 0))
    rng = np.random.default_rng(61)
    x = rng.standard_normal(count * ld * n) * 1e100
    x[rng.random(x.size) < 0.05] = -1e150
    dx = _dev(x)
    for tree, res in ((norms, m), (amax, n)):
        h = api.dispatch_meqn(tm.build(api, tree, {0: (m, n, ld, DT.F64)}, comp=DT.F64), capi.MeqnArgShape(res, 1, res, DT.F64))
        assert h, "f64 equation refused"
        dy = _dev(np.full(count * res, -7.0))
        inputs = (capi.MatrixArg * 1)()
        inputs[0].primary = dx.data_ptr()
        p = capi.MeqnParam(); p.inputs = inputs; p.output.primary = dy.data_ptr()
        if batched:
            strides = (C.c_longlong * 1)(8 * ld * n)
            api.hip_meqn_batch_strided(h, C.byref(p), count, 1, strides, 8 * res, 0, 0, None)
        else:
            capi.Api.call(h, p)
        api.hip_sync(); api.check()
        assert not api.hip_kernel_name(h, 1 if batched else 0).decode().startswith("meqn_jit_")
        got = dy.cpu().numpy().reshape(count, res)
        X = x.reshape(count, n, ld)[:, :, :m]                        # [element][column][row]
        if tree is norms:
            want = np.sqrt((X * X).sum(axis=1))
            assert np.all(np.abs(got - want) <= 1e-12 * want)
        else:
            assert np.array_equal(got, np.abs(X).max(axis=2))


@pytest.mark.parametrize("typ", LISTED_T)
@pytest.mark.parametrize("record", [False, True])
def test_f64_listed_columns_pinned_against_the_reference(reference, typ, record):
    """Listed columns and their recorded argop against the reference's own f64 loop (through the built reference library): bit for bit."""
    m, ldi, ncols = 33, 40, 12
    X, cols, got, got_arg, width, _ = _listed(typ, m, ldi, ncols, True, record, seed=51 + record)
    ref, idx, arg, cnt = np.zeros(m), cols.astype(np.uint64), np.full(m, 77, dtype=np.uint64), C.c_ulonglong(ncols)
    p = capi.UnaryParam()
    p.in_.primary, p.in_.secondary, p.in_.tertiary, p.out.primary = X.ctypes.data, idx.ctypes.data, C.addressof(cnt), ref.ctypes.data
    if record:
        p.out.secondary = arg.ctypes.data
    flags = UNARY_FLAG.REDUCE_COLS | UNARY_FLAG.IDX_SIZE_8BYTES | (UNARY_FLAG.REDUCE_RECORD_ARGOP if record else 0)
    reference.lib.xref_reference_meltw_unary(C.byref(p), typ, capi.UnaryShape(m, 0, ldi, m, DT.F64, DT.F64, DT.F64), flags)
    assert np.array_equal(got, ref)
    if record and typ != UNARY.REDUCE_COLS_IDX_OP_ADD:
        assert np.array_equal(got_arg, arg.astype(np.int64))
