"""The data-movement parity checks of tests/meltw_move_helpers.py proved without a GPU: every row of tests/test_meltw_move_gpu.py gives the same bytes in move_numpy
(the reference's loop nests as index arithmetic) and in the oracle, over the whole allocation, and the oracle touches no byte outside move_numpy's mask; every
(kernel, instantiation) launch_meltw can start for this family is expected by at least one row or carries the reason why none can; every name expected_kernel returns
is a literal of csrc/meltw_kernels.hip; no transform type is absent from both the table and REFUSED."""
import os
import re

import numpy as np
import pytest

import meltw_move_helpers as H
import test_meltw_move_gpu as G
from meltw_move_helpers import COLS, GATHER, I4, I8, OFFS, ROWS, SCATTER, MoveCase
from libxsmm_amd.capi import DT, UNARY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = UNARY


# ---- a. move_numpy == oracle ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", G.TABLES)
def test_move_numpy_equals_the_oracle_on_every_row(table):
    rows = G.rows_of(table)
    assert rows
    for row in rows:
        case = G.make(row)
        want, mask = H.move_numpy(case)
        got = case.run_oracle()
        assert np.array_equal(got[~mask], case.out0[~mask]), f"{G.row_id(row)}: the oracle wrote outside the bytes the operation owns"
        assert np.array_equal(got, want), f"{G.row_id(row)}: {np.count_nonzero(got != want)} bytes differ; first at {int(np.flatnonzero(got != want)[0])}"
        assert mask.any() and not mask[:case.off_out].any() and not mask[-H.SLACK:].any()
        if case.batch > 1:                                                 # the gap between two batch elements is not written
            end = case.off_out + case.out_elems * case.sz
            assert not mask[end: case.off_out + case.bs_out].any()


def test_move_numpy_by_hand():
    """3 x 2 BF16 (elements a0 a1 a2 / b0 b1 b2 at ldi = 4) through the transpose, NORM -> VNNI2 and VNNI2T -> NORM; a row gather with a repeat."""
    def elems(case, buf):
        return buf[case.off_out:].view(np.uint16)

    def src(case):
        return case.inp[case.off_in:].view(np.uint16)
    c = MoveCase(T.TRANSFORM_NORM_TO_NORMT, DT.BF16, 3, 2, 4, 5, off_out=2)
    out, mask = H.move_numpy(c)
    x, y = src(c), elems(c, out)
    assert [y[0], y[1], y[5], y[6], y[10], y[11]] == [x[0], x[4], x[1], x[5], x[2], x[6]]
    assert mask.view(np.uint8).sum() == 12 and np.flatnonzero(mask)[0] == 2
    c = MoveCase(T.TRANSFORM_NORM_TO_VNNI2, DT.BF16, 3, 3, 4, 5)          # n odd: the pad row is zero, and so are the positions m .. ldo - 1
    out, mask = H.move_numpy(c)
    x, y = src(c), elems(c, out)
    assert y[:20].tolist() == [x[0], x[4], x[1], x[5], x[2], x[6], 0, 0, 0, 0, x[8], 0, x[9], 0, x[10], 0, 0, 0, 0, 0]
    assert mask.sum() == 40
    c = MoveCase(T.TRANSFORM_VNNI2T_TO_NORM, DT.BF16, 3, 2, 3, 2)         # M = desc.n = 2, N = desc.m = 3: out[j * ldo + i2] = in[j * 2 + i2]
    out, _ = H.move_numpy(c)
    assert elems(c, out)[:6].tolist() == src(c)[:6].tolist()
    c = MoveCase(GATHER, DT.F32, 4, 2, 8, 5, flags=ROWS | I4)
    out, mask = H.move_numpy(c)
    x, y = c.inp.view(np.uint32), out.view(np.uint32)
    assert c.idx[0] == c.idx[1] == c.idx[2] == c.idx[3]                    # (count <= 3 + 1: the forced repeat fills the list)
    assert [y[i + 5 * j] for j in range(2) for i in range(4)] == [x[c.idx[i] + 8 * j] for j in range(2) for i in range(4)]
    assert c.in_elems == 16 and mask.sum() == 32                           # ld * n elements of the staged side


def test_input_values_are_distinct():
    rng = np.random.default_rng(0)
    for sz, count in ((8, 1 << 18), (4, 1 << 20), (2, 1 << 16)):
        v = H.distinct_values(count, sz, rng).view({8: np.uint64, 4: np.uint32, 2: np.uint16}[sz])
        assert np.unique(v).size == count
    v = H.distinct_values(200000, 2, rng).view(np.uint16)
    assert np.unique(v[70000: 70000 + 65536]).size == 65536                # any 65536 consecutive elements


def test_gather_lists_repeat_and_scatter_lists_do_not():
    seen = set()
    for row in G.ROWS_:
        if row[1][0] not in (GATHER, SCATTER):
            continue
        case = G.make(row)
        assert case.idx.min() >= 0 and case.idx.max() < case.span
        if case.typ == SCATTER:
            assert np.unique(case.idx).size == case.idx.size
        elif row[2].get("idx", "random") == "random" and case.idx.size > 1:
            assert np.unique(case.idx).size < case.idx.size, G.row_id(row)
        seen.add(row[2].get("idx", "random"))
    assert seen == {"random", "equal", "reversed"}


# ---- b. every instantiation is reached ------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 4, 8)
NC4 = ("reason: the launcher's columns-per-workgroup constant nc_env is 2 (four columns measured slower: 64 KiB of LDS leave two workgroups per CU), and "
       "`nc_env >= 4` is the only way to NC = 4: the instantiation is compiled but cannot be started")
REACH = {}
for _sz in WIDTHS:
    REACH[("transpose_kernel", (_sz,))] = None
    REACH[("transpose_vec_kernel", (_sz,))] = None
    REACH[("transpose_vec_kernel", (_sz, "nt"))] = None
    for _way in ("gather", "scatter"):
        REACH[("gather_cols_vec_kernel", (_sz, _way))] = None
        REACH[("gs_rows_lds_kernel", (_sz, _way))] = None
        for _mode in ("COLS", "ROWS", "OFFS"):
            REACH[("gather_scatter_kernel", (_sz, _way, _mode))] = None
REACH[("vnni2_vec_kernel", (4,))] = None
REACH[("vnni2_vec_kernel", (4, "nt"))] = None
REACH[("vnni2_vec_kernel", (8,))] = ("reason: the eight-position form is kept in the source but launch_meltw starts vnni2_vec_kernel<4> only -- its condition (ldi % 4 == 0 and a "
                                     "16-byte aligned base) already makes every row start 8-byte aligned, so nothing is left for <8>")
for _name in ("vnni2_quad_kernel", "vnni2_pair_kernel", "vnni4_vec_kernel"):
    REACH[(_name, ())] = None
for _mode, _vs in H.XF_MODES.items():
    for _v in _vs:
        REACH[("xform_kernel", (_mode, _v))] = None
for _sz in (2, 4):
    REACH[("gs_rows_lds_multi_kernel", (_sz, 2))] = None
    REACH[("gs_rows_lds_multi_kernel", (_sz, 4))] = NC4
    for _way in ("gather", "scatter"):
        REACH[("gs_offs_vec4_kernel", (_sz, _way))] = None


def _key(exp):
    name, args = exp
    return (name, args[1:]) if name == "xform_kernel" else exp          # xform_kernel: mode and v (every width runs through the TRANSFORMS table)


def test_every_instantiation_is_reached_by_a_row_or_excused():
    """expected_kernel at the nominal addresses (allocation base % 256 == 0, plus the row's offsets)."""
    hit, xform_widths = {}, set()
    for row in G.ROWS_:
        case = G.make(row)
        exp = case.expected()
        assert row[2].get("want") in (None, exp[0]), f"{G.row_id(row)}: written for {row[2].get('want')}, expected_kernel says {exp}"
        assert _key(exp) in REACH, exp
        hit.setdefault(_key(exp), G.row_id(row))
        if exp[0] == "xform_kernel":
            xform_widths.add(exp[1][0])
    for key, why in REACH.items():
        if why is None:
            assert key in hit, f"no row reaches {key}"
        else:
            assert key not in hit and why.startswith("reason: ") and len(why) > 60, key
    assert xform_widths == set(WIDTHS)
    assert sum(1 for v in REACH.values() if v is None) == len(hit)


def test_the_rows_the_issue_names_land_where_it_says():
    """every broken clause on the refusing kernel, every threshold from both sides (the `want` of each row is checked above; this counts them)."""
    by = {}
    for row in G.ROWS_:
        by.setdefault((row[0], row[2].get("want")), []).append(row)
    assert len(by[("TRANSPOSES", "transpose_kernel")]) >= 4 + 6 and len(by[("TRANSPOSES", "transpose_vec_kernel")]) == 8
    assert len(by[("VNNI2Q", "vnni2_quad_kernel")]) == 2 * 2 * 4 * 3 * 4
    assert len(by[("VNNI2", "vnni2_quad_kernel")]) >= 7 and len(by[("VNNI2", "xform_kernel")]) >= 1 and len(by[("VNNI2", "vnni2_pair_kernel")]) >= 1
    assert len(by[("VNNI4", "vnni4_vec_kernel")]) >= 4 and len(by[("VNNI4", "xform_kernel")]) >= 7
    notes = {(r[0], r[2].get("note")) for r in G.ROWS_}
    for n in ("2m==rows", "2m==rows-2", "64KiB", "64KiB+16", "staged-base"):
        assert ("GS_ROWS", n) in notes
    for n in ("n=63", "2x32KiB", "2x32KiB+16"):
        assert ("GS_ROWS2", n) in notes
    for n in ("m%4", "8-byte-offsets", "index-pointer", "contiguous-side", "ld%4"):
        assert ("GS_OFFS", n) in notes
    assert {r[1][0] for r in G.rows_of("HOST")} == {GATHER, SCATTER} and all(r[2]["host_idx"] for r in G.rows_of("HOST"))
    assert all(r[2]["batch"] == 3 for r in G.rows_of("BATCH")) and len({r[2]["want"] for r in G.rows_of("BATCH")}) == 10


def test_expected_kernel_against_hand_written_cases():
    def ek(typ, dt, m, n, ldi, ldo, in_addr=0, out_addr=0, idx_addr=0, **kw):
        return H.expected_kernel(MoveCase(typ, dt, m, n, ldi, ldo, **kw), in_addr, out_addr, idx_addr)
    NT, V2, V4 = T.TRANSFORM_NORM_TO_NORMT, T.TRANSFORM_NORM_TO_VNNI2, T.TRANSFORM_NORM_TO_VNNI4
    assert ek(NT, DT.BF16, 64, 64, 64, 64) == ("transpose_vec_kernel", (2,))
    assert ek(NT, DT.BF16, 64, 64, 64, 64, hint=2) == ("transpose_vec_kernel", (2, "nt"))
    assert ek(NT, DT.BF16, 64, 60, 64, 64) == ("transpose_kernel", (2,))                          # n % 8
    assert ek(NT, DT.F64, 66, 10, 66, 12) == ("transpose_vec_kernel", (8,))                       # two doubles per access
    assert ek(NT, DT.F64, 66, 10, 66, 12, in_addr=8) == ("transpose_kernel", (8,))
    assert ek(V2, DT.BF16, 32, 16, 32, 32) == ("vnni2_vec_kernel", (4,))
    assert ek(V2, DT.BF16, 32, 16, 32, 32, out_addr=4) == ("vnni2_quad_kernel", ())
    assert ek(V2, DT.BF16, 32, 16, 32, 32, out_addr=2) == ("xform_kernel", (2, "NORM_TO_VNNI", 2))
    assert ek(V2, DT.BF16, 32, 16, 32, 32, in_addr=1) == ("vnni2_pair_kernel", ())               # an odd byte address: no 4-position loads
    assert ek(V2, DT.BF16, 13, 8, 16, 14) == ("vnni2_pair_kernel", ())
    assert ek(V2, DT.F32, 32, 16, 32, 32) == ("xform_kernel", (4, "NORM_TO_VNNI", 2))
    assert ek(V4, DT.I8, 20, 12, 24, 20) == ("vnni4_vec_kernel", ())
    assert ek(V4, DT.BF16, 16, 8, 16, 16) == ("xform_kernel", (2, "NORM_TO_VNNI", 4))
    assert ek(T.TRANSFORM_PADN_MOD4, DT.I8, 9, 6, 10, 12) == ("xform_kernel", (1, "PAD", 4))
    assert ek(T.TRANSFORM_PADM_MOD4, DT.I8, 9, 6, 10, 12) == ("xform_kernel", (1, "PAD", 1))
    assert ek(T.TRANSFORM_VNNI8T_TO_NORM, DT.BF16, 3, 8, 3, 8) == ("xform_kernel", (2, "VNNIT_TO_NORM", 8))
    # the shapes of tests/test_meltw_gpu.py::test_gather_scatter_bit_exact (m, n, big = 24, 10, 40)
    assert ek(GATHER, DT.F32, 24, 10, 40, 24, flags=COLS | I4) == ("gather_cols_vec_kernel", (4, "gather"))
    assert ek(GATHER, DT.I8, 24, 10, 40, 24, flags=COLS | I4) == ("gather_scatter_kernel", (1, "gather", "COLS"))
    assert ek(GATHER, DT.BF16, 24, 10, 40, 24, flags=ROWS | I8) == ("gs_rows_lds_kernel", (2, "gather"))
    assert ek(GATHER, DT.I8, 24, 10, 40, 24, flags=ROWS | I4) == ("gather_scatter_kernel", (1, "gather", "ROWS"))          # 40 bytes are not 16-byte granular
    assert ek(SCATTER, DT.F32, 24, 10, 24, 40, flags=OFFS | I4) == ("gs_offs_vec4_kernel", (4, "scatter"))
    assert ek(SCATTER, DT.F32, 24, 10, 24, 40, flags=OFFS | I8) == ("gather_scatter_kernel", (4, "scatter", "OFFS"))
    assert ek(GATHER, DT.F32, 24, 10, 24, 24, flags=OFFS | I4, idx_addr=8) == ("gather_scatter_kernel", (4, "gather", "OFFS"))
    assert ek(GATHER, DT.F32, 24, 10, 24, 24, flags=OFFS | I4, idx_addr=8, host_idx=True) == ("gs_offs_vec4_kernel", (4, "gather"))
    assert ek(GATHER, DT.F32, 500, 70, 512, 500, flags=ROWS | I4) == ("gs_rows_lds_multi_kernel", (4, 2))                  # ::test_row_gather_of_many_columns_bit_exact
    assert ek(GATHER, DT.F32, 200, 70, 512, 200, flags=ROWS | I4) == ("gather_scatter_kernel", (4, "gather", "ROWS"))      # fewer than half of the rows


# ---- c. names ---------------------------------------------------------------------------------------------------------------------------------------------
def test_every_expected_name_is_a_literal_of_the_launcher():
    src = open(os.path.join(ROOT, "libxsmm_amd", "csrc", "meltw_kernels.hip")).read()
    names = {k[0] for k in REACH}
    assert len(names) == 12
    for name in names:
        assert f'*name = "{name}"' in src, name
        assert re.search(r"void " + name + r"\(MeltwArgs", src), name
    # the instantiations REACH lists are the ones the source compiles: the payload switch has the four widths, the multi kernel <S, NC> for S in {2, 4} x NC in {2, 4}
    assert re.findall(r"gs_rows_lds_multi_kernel<(\d), (\d)>", src).count(("4", "2")) == 1 and "nc_env = 2;" in src
    assert sorted(set(re.findall(r"gs_rows_lds_multi_kernel<(\d), (\d)>", src))) == [("2", "2"), ("2", "4"), ("4", "2"), ("4", "4")]
    assert set(re.findall(r"vnni2_vec_kernel<(\d)>", src)) == {"4"}
    assert set(re.findall(r"gs_offs_vec4_kernel<(\d)>", src)) == {"2", "4"}
    modes = re.search(r"enum XformMode \{([^}]*)\}", src).group(1)
    assert [s.strip().split(" ")[0].replace("XF_", "") for s in modes.split(",")] == list(H.XF_MODES)


def test_xform_mode_restates_the_launchers_table():
    src = open(os.path.join(ROOT, "libxsmm_amd", "csrc", "meltw_kernels.hip")).read()
    body = src[src.index("static int xform_mode("): src.index("static bool is_reduce_type(")]
    seen = {}
    for line in body.splitlines():
        types = re.findall(r"case LIBXSMM_MELTW_TYPE_UNARY_(TRANSFORM_\w+):", line)
        m = re.search(r"\*v = (\d); return XF_(\w+);", line)
        for t in types:
            seen[UNARY[t]] = (m.group(2), int(m.group(1)))
    assert len(seen) == 23
    for typ, want in seen.items():
        assert H.xform_mode(typ) == want, UNARY.name(typ)
    assert H.xform_mode(T.TRANSFORM_NORM_TO_NORMT) == (None, 0) and H.xform_mode(T.TRANSFORM_VNNI8_TO_NORM) == (None, 0)


def test_no_transform_type_is_absent_from_both_the_table_and_refused():
    every = {v for k, v in UNARY._items.items() if k.startswith("TRANSFORM_")}
    in_table = {r[1][0] for r in G.rows_of("TRANSFORMS")}
    refused = {k[0] for k in G.REFUSED}
    assert in_table == set(H.ALL_TRANSFORMS) and len(in_table) == 24
    assert every == in_table | refused and not (in_table & refused)
    assert all(len(why) > 40 for why in G.REFUSED.values())
    for typ in H.ALL_TRANSFORMS:                                            # two shapes at each of the four widths
        rows = [r for r in G.rows_of("TRANSFORMS") if r[1][0] == typ]
        assert {(H.capi.DT_SIZE[r[1][1]], r[2]["note"]) for r in rows} >= {(sz, k) for sz in WIDTHS for k in ("min", "big")}
        big = [r for r in rows if r[2]["note"] == "big"][0][1]
        assert big[2] * big[3] > 256
    assert {r[1][1] for r in G.rows_of("TRANSFORMS")} >= {DT.BF8, DT.HF8, DT.F16}
