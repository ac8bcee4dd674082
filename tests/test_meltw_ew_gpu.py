"""GPU parity of the element-wise TPPs over the whole input range (tests/meltw_ew_helpers.py): every row builds padded operands whose gaps hold NaN, asserts the
kernel launch_meltw picked (libxsmm_hip_kernel_name against expected_kernel's restatement of ew8_ok and the vec4 condition), and ends in assert_exact (same bits as
the oracle inside, the oracle's bytes outside) or assert_approx (per-element bound against float64 for the operations that call libm).

Paths (every table runs on each one its types can reach):
  stream    256-byte aligned operands, m % 8 == 0: meltw_ew8_kernel, eight elements per thread (bf16 / mixed) or four (all f32; once more under the streaming hint 2,
            the non-temporal instantiation)
  vec4      bf16 -> bf16 through pointers 8 bytes into their allocations, or m = 12: meltw_unary_vec4_kernel
  general   pointers one element into their allocations, odd m, or batch strides that are no multiple of 16 bytes: meltw_unary / binary / ternary_kernel
An all-f32 TPP whose pointers are 8 bytes off is refused by BOTH vector kernels (each wants 16 bytes for f32), so that row expects the general kernel: the f32
instantiation of meltw_unary_vec4_kernel is only reachable by a descriptor ew8_ok turns down for its element count (2^32 threads); the name is asserted on bf16.

NAMES maps every name launch_meltw can report to the row / test that asserts it or to the reason nothing does (tests/test_meltw_ew_cpu.py holds it against the
literals of csrc/meltw_kernels.hip)."""
import functools

import numpy as np
import pytest

import meltw_ew_helpers as H
from meltw_ew_helpers import COL, NONE, OP_BINARY, OP_TERNARY, OP_UNARY, ROW, SCALAR, EwCase
from helpers import as_float
from libxsmm_amd.capi import BINARY, DT, TERNARY, UNARY

pytestmark = pytest.mark.gpu

HERE = "tests/test_meltw_ew_gpu.py"
OLD = "tests/test_meltw_gpu.py"
F64R = "tests/test_meltw_f64_reduce_gpu.py"
NAMES = {
    "meltw_ew8_kernel": HERE, "meltw_unary_vec4_kernel": HERE, "meltw_unary_kernel": HERE, "meltw_binary_kernel": HERE, "meltw_ternary_kernel": HERE,
    "(empty)": "reason: reported for a launch of zero elements (m <= 0, n <= 0 or an empty batch), no kernel runs; dispatch refuses such shapes before a handle exists",
    "mul_reduce_scalar_kernel": OLD + "::test_dot_product_to_scalar", "reduce_scalar_kernel": OLD + "::test_reduce_to_scalar",
    "reduce_ncnc_kernel": OLD + "::test_reduce_ncnc_format_bit_exact", "dropout_kernel": OLD + "::test_dropout_bit_exact", "dropout_inv_kernel": OLD + "::test_dropout_bit_exact",
    "nvfp4_quant_kernel": "tests/test_mx_quant.py::test_gpu_nvfp4_quant_is_bit_identical", "mx_quant_kernel": "tests/test_mx_quant.py::test_gpu_mx_quant_is_bit_identical",
    "transpose_vec_kernel": OLD + "::test_transforms_bit_exact", "vnni2_vec_kernel": OLD + "::test_transforms_bit_exact", "vnni2_quad_kernel": OLD + "::test_transforms_bit_exact",
    "vnni2_pair_kernel": OLD + "::test_transforms_bit_exact", "vnni4_vec_kernel": OLD + "::test_transforms_bit_exact", "transpose_kernel": OLD + "::test_transforms_bit_exact",
    "xform_kernel": OLD + "::test_transforms_bit_exact",
    "gather_cols_vec_kernel": OLD + "::test_gather_scatter_bit_exact", "gs_rows_lds_kernel": OLD + "::test_gather_scatter_bit_exact",
    "gs_offs_vec4_kernel": OLD + "::test_gather_scatter_bit_exact", "gather_scatter_kernel": OLD + "::test_gather_scatter_bit_exact",
    "gs_rows_lds_multi_kernel": OLD + "::test_row_gather_of_many_columns_bit_exact",
    "reduce_vec_kernel": OLD + "::test_reductions_vector_kernel", "reduce_vec_kernel+combine": OLD + "::test_column_reduction_of_one_big_matrix_two_pass",
    "reduce_kernel": OLD + "::test_reductions", "reduce_cols_listed_kernel": OLD + "::test_listed_column_sum_batched_embedding_bags",
    "reduce_f64_kernel": F64R + "::test_f64_reduction_single_call", "reduce_vec_f64_kernel": F64R + "::test_f64_reduction_single_call",
    "reduce_vec_f64_kernel+combine": F64R + "::test_f64_reduction_of_one_big_matrix", "reduce_cols_listed_f64_kernel": F64R + "::test_f64_listed_columns",
}
# combinations of the issue's tables dispatch refuses (none so far: every listed one returns a handle)
REFUSED = {}

# ---- tables ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unary_table(name, in_dt):
    """(values [n][m] in the storage type, m, n)"""
    if name == "bf16all":
        v = H.all_bf16()
        return (v if in_dt == DT.BF16 else H.bf16_to_f32(v)).reshape(256, 256), 256, 256
    assert name == "wide" and in_dt == DT.F32
    return H.f32_wide(np.random.default_rng(11), 64 * 256).reshape(256, 64), 64, 256


UNARY_COMBOS = [("bf16all", DT.BF16, DT.BF16), ("bf16all", DT.F32, DT.F32), ("bf16all", DT.BF16, DT.F32), ("wide", DT.F32, DT.F32), ("wide", DT.F32, DT.BF16)]
PATH_OFF = {"stream": 0, "vec4": 8, "general": None}      # None: one element


def unary_rows():
    rows = []
    for typ in H.EXACT_UNARY + H.APPROX_UNARY:
        for table, in_dt, out_dt in UNARY_COMBOS:
            for path in ("stream", "general") + (("vec4",) if in_dt == out_dt == DT.BF16 else ()):
                rows.append((typ, table, in_dt, out_dt, path))
    return rows


def unary_case(typ, table, in_dt, out_dt, path, **kw):
    v, m, n = unary_table(table, in_dt)
    off = PATH_OFF[path] if PATH_OFF[path] is not None else max(H.capi.DT_SIZE[in_dt], H.capi.DT_SIZE[out_dt])
    alpha = H.ALPHA if typ in (UNARY.LEAKY_RELU, UNARY.ELU) else None
    return EwCase(OP_UNARY, typ, (in_dt,), out_dt, m, n, [v], (m + 8, m + 16), off_bytes=off, alpha=alpha, **kw)


PATH_KERNEL = {"stream": "meltw_ew8_kernel", "vec4": "meltw_unary_vec4_kernel"}


def _run(case, want=None, pure=False, what="", **kw):
    ref = case.run_oracle()
    got, h, name = case.run_gpu(**kw)
    assert name == case.expected(), f"{what}: {name} ran, the conditions of launch_meltw say {case.expected()}"
    if want is not None:
        assert name == want, f"{what}: {name} ran, the row is meant for {want}"
    if case.op == OP_UNARY and case.typ in H.APPROX_UNARY:
        stats = {}
        try:
            case.check_approx(ref, got, what=f"{what} [{name}]", stats=stats)
        finally:
            print(f"{what} [{name}]: worst err / (2^-24 S) = {stats.get('ratio', float('nan')):.3f} (K = {H.K_OP[case.typ]:.2f})")
    else:
        case.check_exact(ref, got, pure=pure, what=f"{what} [{name}]")
    return ref, got, name


@pytest.mark.parametrize("typ,table,in_dt,out_dt,path", unary_rows(), ids=lambda x: str(int(x)) if isinstance(x, int) else x)
def test_unary_over_the_tables(typ, table, in_dt, out_dt, path):
    case = unary_case(typ, table, in_dt, out_dt, path)
    want = PATH_KERNEL.get(path, "meltw_unary_kernel")
    _run(case, want, pure=(typ == UNARY.IDENTITY and in_dt == out_dt), what=f"unary {int(typ)} {table} {int(in_dt)}->{int(out_dt)} {path}")


@pytest.mark.parametrize("typ", [UNARY.IDENTITY, UNARY.TANH, UNARY.RELU, UNARY.ELU])
def test_unary_f32_non_temporal_instantiation(typ):
    """all f32, four elements per thread, under the streaming hint 2: meltw_ew8_kernel<1, true, 4>."""
    case = unary_case(typ, "wide", DT.F32, DT.F32, "stream")
    _run(case, "meltw_ew8_kernel", pure=(typ == UNARY.IDENTITY), what=f"unary {int(typ)} nt", hint=2)


@pytest.mark.parametrize("typ", [UNARY.IDENTITY, UNARY.X2])
def test_f32_to_bf16_on_every_rounding_boundary(typ):
    """v_cvt_pk_bf16_f32 behind a denormal flush (streaming kernel) and mw_f2bf (general kernel) agree with the oracle and with each other on every upper half x
    the lower halves around the tie: all NaN shapes, 0x7f7f8000 -> inf, denormals."""
    v = H.f32_on_bf16_boundaries().reshape(-1, 512)
    outs = {}
    for path, off in (("stream", 0), ("general", 4)):
        case = EwCase(OP_UNARY, typ, (DT.F32,), DT.BF16, 512, v.shape[0], [v], (520, 528), off_bytes=off)
        _, got, name = _run(case, PATH_KERNEL.get(path, "meltw_unary_kernel"), what=f"boundaries {int(typ)} {path}")
        outs[path] = case.out.logical(got)
    assert H.same_bits(outs["stream"], outs["general"], DT.BF16).all()


@pytest.mark.parametrize("dt", [DT.F16, DT.BF8, DT.HF8])
def test_narrow_floats_decode_and_round_like_the_tables(dt):
    """every code of F16 / E5M2 / E4M3 through IDENTITY to f32 against helpers.as_float (a decode table that does not come from the oracle), and f32 -> the type over
    every value, every tie and the f32 neighbours of every tie."""
    codes = H.all_f16() if dt == DT.F16 else H.all_fp8(dt)
    m = 256 if dt == DT.F16 else 16
    v = codes.reshape(-1, m)
    case = EwCase(OP_UNARY, UNARY.IDENTITY, (dt,), DT.F32, m, v.shape[0], [v], (m + 3, m + 5))
    _, got, _ = _run(case, "meltw_unary_kernel", what=f"decode {int(dt)}")
    g, want = H.decode(case.out.logical(got), DT.F32).ravel(), as_float(codes, dt)
    assert np.array_equal(np.isnan(g), np.isnan(want)) and np.array_equal(g[~np.isnan(want)], want[~np.isnan(want)]) and np.array_equal(np.signbit(g[~np.isnan(want)]), np.signbit(want[~np.isnan(want)]))
    b = H.f32_on_narrow_boundaries(dt)
    m = 64
    b = np.concatenate([b, np.zeros(-b.size % m, dtype=np.float32)]).reshape(-1, m)
    case = EwCase(OP_UNARY, UNARY.IDENTITY, (DT.F32,), dt, m, b.shape[0], [b], (m + 1, m + 3))
    _run(case, "meltw_unary_kernel", what=f"narrow to {int(dt)}")


@pytest.mark.parametrize("typ", [UNARY.IDENTITY, UNARY.X2, UNARY.NEGATE, UNARY.INC, UNARY.SQRT, UNARY.RECIPROCAL, UNARY.RECIPROCAL_SQRT])
def test_unary_f64_over_wide_doubles(typ):
    v = H.f64_wide(np.random.default_rng(12), 70 * 33).reshape(33, 70)
    case = EwCase(OP_UNARY, typ, (DT.F64,), DT.F64, 70, 33, [np.tile(v, (2, 1, 1))], (72, 75), batch=2)
    _run(case, "meltw_unary_kernel", pure=(typ == UNARY.IDENTITY), what=f"f64 unary {int(typ)}")


@pytest.mark.parametrize("dt", [DT.BF16, DT.F32])
@pytest.mark.parametrize("typ", [UNARY.IDENTITY, UNARY.RELU, UNARY.X2, UNARY.TANH])
def test_unary_short_rows_on_the_vec4_kernel(typ, dt):
    """m = 12, ldi = 12, ldo = 20: too short for eight bf16 per thread, four fit.  All f32 with m % 4 == 0 is the streaming kernel's (four per thread)."""
    v = H.interesting(dt, 3 * 7 * 12, seed=3).reshape(3, 7, 12)
    case = EwCase(OP_UNARY, typ, (dt,), dt, 12, 7, [v], (12, 20), batch=3)
    _run(case, "meltw_unary_vec4_kernel" if dt == DT.BF16 else "meltw_ew8_kernel", pure=(typ == UNARY.IDENTITY), what=f"m = 12 {int(typ)} {int(dt)}")


SMALL_PATHS = {          # name -> (m, lds of inputs, ldo, off_bytes or None = one element, odd_stride)
    "odd_m_33": (33, 40, 35, 0, False), "odd_m_70": (70, 72, 72, 0, False), "off_one_element": (64, 64, 72, None, False), "odd_stride": (64, 64, 64, 0, True),
    "off_8_bytes": (64, 64, 72, 8, False),
}


def small_case(op, typ, dt, path, batch=3, n=7, seed=5, **kw):
    m, ldi, ldo, off, odd = SMALL_PATHS[path]
    nin = op
    vals = [H.interesting(dt, batch * n * m, seed=seed + o).reshape(batch, n, m) for o in range(nin)]
    prev = H.interesting(dt, batch * n * m, seed=seed + 9).reshape(batch, n, m) if (op == OP_BINARY and typ == BINARY.MULADD) else None
    off = H.capi.DT_SIZE[dt] if off is None else off
    alpha = H.ALPHA if op == OP_UNARY and typ in (UNARY.LEAKY_RELU, UNARY.ELU) else None
    return EwCase(op, typ, (dt,) * nin, dt, m, n, vals, (ldi,) * nin + (ldo,), batch=batch, off_bytes=off, odd_stride=odd, prev=prev, alpha=alpha, **kw)


GENERAL = {OP_UNARY: "meltw_unary_kernel", OP_BINARY: "meltw_binary_kernel", OP_TERNARY: "meltw_ternary_kernel"}


@pytest.mark.parametrize("path", list(SMALL_PATHS))
@pytest.mark.parametrize("dt", [DT.F32, DT.BF16])
@pytest.mark.parametrize("op,typ", [(OP_UNARY, UNARY.IDENTITY), (OP_UNARY, UNARY.RELU), (OP_UNARY, UNARY.SIGMOID), (OP_BINARY, BINARY.SUB), (OP_BINARY, BINARY.MULADD),
                                    (OP_BINARY, BINARY.MAX), (OP_TERNARY, TERNARY.NMULADD)])
def test_refusals_of_the_vector_kernels(op, typ, dt, path):
    """What sends a TPP to the general kernels: odd m, a pointer one element into a tensor, a batch stride that is no multiple of 16 bytes -- and the pointer 8
    bytes into a tensor, which bf16 unary TPPs keep on four elements per thread."""
    case = small_case(op, typ, dt, path)
    want = "meltw_unary_vec4_kernel" if (path == "off_8_bytes" and op == OP_UNARY and dt == DT.BF16) else GENERAL[op]
    _run(case, want, pure=(op == OP_UNARY and typ == UNARY.IDENTITY), what=f"{path} op {op} {int(typ)} {int(dt)}")


# ---- binary ---------------------------------------------------------------------------------------------------------------------------------------------
BINARY_DTS = {"f32": (DT.F32, DT.F32, DT.F32), "bf16": (DT.BF16, DT.BF16, DT.BF16), "bf16_f32_f32": (DT.BF16, DT.F32, DT.F32), "bf16_f32_bf16": (DT.BF16, DT.F32, DT.BF16),
              "f64": (DT.F64, DT.F64, DT.F64)}


@functools.lru_cache(maxsize=None)
def _pairs(dt):
    return H.pair_grid(dt)


def binary_case(typ, dts_name, path, **kw):
    d0, d1, do = BINARY_DTS[dts_name]
    a, b = _pairs(d0)[0], _pairs(d1)[1]
    prev = None
    if typ == BINARY.MULADD:
        v = H.interesting(do, 256, seed=8)
        i, j = np.arange(256)[None, :], np.arange(256)[:, None]
        prev = v[(7 * i + 3 * j) % 256]
    off = 0 if path == "stream" else max(H.capi.DT_SIZE[d] for d in (d0, d1, do))
    return EwCase(OP_BINARY, typ, (d0, d1), do, 256, 256, [a, b], (264, 272, 280), off_bytes=off, prev=prev, **kw)


ARITH = [BINARY.ADD, BINARY.SUB, BINARY.MUL, BINARY.DIV, BINARY.MULADD, BINARY.MAX, BINARY.MIN]


@pytest.mark.parametrize("path", ["stream", "general"])
@pytest.mark.parametrize("dts_name", list(BINARY_DTS))
@pytest.mark.parametrize("typ", ARITH, ids=lambda t: str(int(t)))
def test_binary_over_the_pair_grid(typ, dts_name, path):
    """256 interesting values of the type crossed with themselves: NaN and +-0 under MAX / MIN, x / 0, inf - inf, 0 * inf, denormals, overflow."""
    case = binary_case(typ, dts_name, path)
    want = "meltw_ew8_kernel" if (path == "stream" and dts_name != "f64") else "meltw_binary_kernel"
    _run(case, want, what=f"binary {int(typ)} {dts_name} {path}")


@pytest.mark.parametrize("typ", [BINARY.ADD, BINARY.MULADD, BINARY.MIN], ids=lambda t: str(int(t)))
def test_binary_f32_non_temporal_instantiation(typ):
    _run(binary_case(typ, "f32", "stream"), "meltw_ew8_kernel", what=f"binary {int(typ)} nt", hint=2)


@pytest.mark.parametrize("dts_name", ["f32", "bf16"])
@pytest.mark.parametrize("typ", [BINARY.CMP_OP_GT, BINARY.CMP_OP_GE, BINARY.CMP_OP_LT, BINARY.CMP_OP_LE, BINARY.CMP_OP_EQ, BINARY.CMP_OP_NE], ids=lambda t: str(int(t)))
def test_compares_over_the_pair_grid(typ, dts_name):
    d0, d1, _ = BINARY_DTS[dts_name]
    case = EwCase(OP_BINARY, typ, (d0, d1), DT.F32 if d0 == DT.F32 else DT.BF16, 256, 256, [_pairs(d0)[0], _pairs(d1)[1]], (259, 261, 270), out_bits=True)
    ref, got, _ = _run(case, "meltw_binary_kernel", what=f"compare {int(typ)} {dts_name}")
    a, b = case.x64(0)[0], case.x64(1)[0]
    with np.errstate(invalid="ignore"):
        want = {BINARY.CMP_OP_GT: a > b, BINARY.CMP_OP_GE: a >= b, BINARY.CMP_OP_LT: a < b, BINARY.CMP_OP_LE: a <= b, BINARY.CMP_OP_EQ: a == b, BINARY.CMP_OP_NE: a != b}[typ]
    assert np.array_equal(case.out.logical_bits(got)[0].astype(bool), want)       # IEEE compares of the decoded values: NaN unordered, -0 == +0


@pytest.mark.parametrize("path", ["stream", "general"])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("dts_name", ["f32", "bf16"])
def test_binary_in_place(dts_name, which, path):
    d0, d1, do = BINARY_DTS[dts_name]
    off = 0 if path == "stream" else H.capi.DT_SIZE[d0]
    case = EwCase(OP_BINARY, BINARY.SUB, (d0, d1), do, 256, 256, [_pairs(d0)[0], _pairs(d1)[1]], (264, 264, 264), off_bytes=off, inplace=which)
    _run(case, "meltw_ew8_kernel" if path == "stream" else "meltw_binary_kernel", what=f"in place out == in{which} {dts_name} {path}")


# ---- ternary --------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _triples(dt):
    return H.triple_grid(dt)


@pytest.mark.parametrize("path", ["stream", "general", "stream_batch3", "general_batch3"])
@pytest.mark.parametrize("dt", [DT.F32, DT.BF16])
@pytest.mark.parametrize("typ", [TERNARY.MULADD, TERNARY.NMULADD], ids=lambda t: str(int(t)))
def test_ternary_over_the_triple_grid(typ, dt, path):
    vals = list(_triples(dt))
    n, batch = 1600, 1
    if path.endswith("batch3"):          # 3 x 534 columns: the grid and its first two columns once more
        vals = [np.concatenate([v, v[:2]]) for v in vals]
        n, batch = 534, 3
    off = 0 if path.startswith("stream") else H.capi.DT_SIZE[dt]
    case = EwCase(OP_TERNARY, typ, (dt,) * 3, dt, 40, n, vals, (48, 56, 64, 72), batch=batch, off_bytes=off)
    _run(case, "meltw_ew8_kernel" if path.startswith("stream") else "meltw_ternary_kernel", what=f"ternary {int(typ)} {int(dt)} {path}")


def test_ternary_f32_non_temporal_instantiation():
    case = EwCase(OP_TERNARY, TERNARY.NMULADD, (DT.F32,) * 3, DT.F32, 40, 1600, list(_triples(DT.F32)), (48, 56, 64, 72))
    _run(case, "meltw_ew8_kernel", what="ternary nt", hint=2)


@pytest.mark.parametrize("dt", [DT.F32, DT.BF16, DT.F64])
def test_select_over_the_grid(dt):
    a, b, _ = _triples(dt)
    bits = np.random.default_rng(13).integers(0, 256, 4 * 1600 * 16, dtype=np.uint8)
    case = EwCase(OP_TERNARY, TERNARY.SELECT, (dt, dt), dt, 40, 534, [np.concatenate([a, a[:2]]), np.concatenate([b, b[:2]])], (43, 45, 50, 47), batch=3, select_bits=bits)
    _run(case, "meltw_ternary_kernel", pure=True, what=f"select {int(dt)}")


# ---- broadcasts -----------------------------------------------------------------------------------------------------------------------------------------
BC_SHAPES = {"stream": (40, 48), "general": (37, 41)}
BC_DTS = {OP_UNARY: {"f32": (DT.F32, DT.F32), "bf16": (DT.BF16, DT.BF16), "f32_bf16": (DT.F32, DT.BF16)},
          OP_BINARY: {"f32": (DT.F32,) * 3, "bf16": (DT.BF16,) * 3, "bf16_f32_f32": (DT.BF16, DT.F32, DT.F32), "f32_bf16_bf16": (DT.F32, DT.BF16, DT.BF16)},
          OP_TERNARY: {"f32": (DT.F32,) * 4, "bf16": (DT.BF16,) * 4, "bf16_f32_bf16_f32": (DT.BF16, DT.F32, DT.BF16, DT.F32)}}


def bcast_case(op, typ, dts, path, kinds, batch=2):
    m, ld = BC_SHAPES[path]
    n = 9
    rng = np.random.default_rng(21)
    vals = [H.encode(rng.standard_normal(batch * n * m) * 2.0 ** rng.integers(-3, 4, batch * n * m), dts[o]).reshape(batch, n, m) for o in range(op)]
    lds = tuple(ld + 8 * o for o in range(op)) + (ld + (8 if path == "stream" else 5),)
    return EwCase(op, typ, dts[:-1], dts[-1], m, n, vals, lds, kinds=kinds, batch=batch)


def kind_tuples(op):
    import itertools
    return list(itertools.product(H.KINDS, repeat=op))


BC_OPS = [(OP_UNARY, UNARY.X2), (OP_UNARY, UNARY.IDENTITY), (OP_BINARY, BINARY.SUB), (OP_BINARY, BINARY.DIV), (OP_TERNARY, TERNARY.NMULADD)]


def bcast_rows():
    return [(op, typ, name, path) for op, typ in BC_OPS for name in BC_DTS[op] for path in BC_SHAPES]


@pytest.mark.parametrize("op,typ,dts_name,path", bcast_rows(), ids=lambda x: str(int(x)) if isinstance(x, int) else x)
def test_every_broadcast_combination(op, typ, dts_name, path):
    """unary: ROW / COL / SCALAR; binary: all 16 operand-kind pairs of the asymmetric SUB and DIV; ternary: all 64 triples of NMULADD.  Broadcast operands span
    their minimal extent plus a poisoned tail (a wrong ld in bc_index / ew8_load reads NaN).  bc_index of the general kernels and ew8_load of the streaming
    kernel are two implementations: both paths run every combination."""
    dts = BC_DTS[op][dts_name]
    for kinds in kind_tuples(op):
        if op == OP_UNARY and kinds == (NONE,):
            continue
        case = bcast_case(op, typ, dts, path, kinds)
        _run(case, "meltw_ew8_kernel" if path == "stream" else GENERAL[op], what=f"op {op} {int(typ)} {dts_name} {path} kinds {kinds}")


@pytest.mark.parametrize("op,typ,kinds,host", [(OP_UNARY, UNARY.X2, (ROW,), (0,)), (OP_UNARY, UNARY.IDENTITY, (COL,), (0,)), (OP_BINARY, BINARY.SUB, (NONE, COL), (1,)),
                                                (OP_BINARY, BINARY.DIV, (ROW, SCALAR), (0, 1)), (OP_TERNARY, TERNARY.NMULADD, (ROW, COL, SCALAR), (0, 1, 2))],
                         ids=lambda x: str(x))
@pytest.mark.parametrize("path", list(BC_SHAPES))
def test_broadcast_operands_in_host_memory_are_staged_at_their_extent(op, typ, kinds, host, path):
    """A synchronous single call takes a broadcast operand from plain host memory: the runtime stages extent() elements of it (tests/meltw_ew_helpers.py: extent);
    too few and the kernel reads what the staging buffer held before, too many is a read past the caller's array."""
    case = bcast_case(op, typ, BC_DTS[op]["f32"], path, kinds, batch=1)
    _run(case, "meltw_ew8_kernel" if path == "stream" else GENERAL[op], what=f"host op {op} {int(typ)} kinds {kinds} {path}", host=host)
