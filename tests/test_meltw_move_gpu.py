"""GPU parity of the data-movement TPPs (tests/meltw_move_helpers.py): every row runs the oracle and the device on the same bytes, asserts the kernel launch_meltw
picked (libxsmm_hip_kernel_name against expected_kernel's restatement of the launcher, and against the kernel the row was written for) and ends in np.array_equal over
the WHOLE output allocation -- the poisoned bytes in front of the pointer, between batch elements and behind the footprint included.

Tables (tests/test_meltw_move_cpu.py holds every row against move_numpy and the REACH table without a GPU):
  TRANSFORMS   all 24 transform types x the four payload widths x a minimal shape and one of more than 256 outputs with padded leading dimensions (NORM -> VNNIv:
               n % v != 0, so the pad rows are zero filled); BF8 / HF8 / F16 once each: only the width matters
  TRANSPOSES   transpose_kernel and transpose_vec_kernel at every width with partial tiles on both axes, the vector form under the streaming hint 2, and one row per
               clause of the vector form's condition broken, each on transpose_kernel
  VNNI2        NORM -> VNNI2 of 16-bit payloads: vnni2_vec_kernel (plain, hint 2), one row per broken clause on vnni2_quad_kernel, the full cross of the alignment
               cases inside vnni2_quad_kernel, a batch whose stride changes the case per element, vnni2_pair_kernel below ldo = 16, xform_kernel for a 2-byte aligned output
  VNNI4        NORM -> VNNI4 of 8-bit payloads: vnni4_vec_kernel with n % 4 in 0..3, one row per broken clause on xform_kernel
  GS_*         GATHER / SCATTER in all three modes at 1 / 2 / 4 / 8 bytes with 4- and 8-byte indices; gather lists are drawn WITH repeats (an embedding look-up), scatter lists
               without (the last writer of a repeated index is not defined on a GPU); both sides of every clause and threshold of the vector, LDS and four-offset paths
  BATCH, HOST  every path once as a batch of 3 with padded strides and the shared index list; the index list in plain host memory once per mode

REFUSED: what dispatch turns down, with the reason; the test asserts the NULL."""
import pytest

import meltw_move_helpers as H
from meltw_move_helpers import COLS, GATHER, I4, I8, OFFS, ROWS, SCATTER, MoveCase
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, UNARY

pytestmark = pytest.mark.gpu
T = UNARY
W = {1: DT.I8, 2: DT.BF16, 4: DT.F32, 8: DT.F64}          # one payload type per width

# (type, payload type) -> why dispatch returns NULL
REFUSED = {
    (T.TRANSFORM_VNNI8_TO_NORM, DT.BF16): "csrc/meltw_kernels.hip: xform_mode has no entry for VNNI8_TO_NORM, and the reference's libxsmm_elementwise_transform_kernel has "
                                          "no loop for it either (it falls through to its `should not happen` branch): there is nothing to restate",
}

ROWS_ = []      # (table, args, kwargs)


def R(table, typ, dt, m, n, ldi, ldo, **kw):
    ROWS_.append((table, (typ, dt, m, n, ldi, ldo), kw))


def make(row):
    return MoveCase(*row[1], seed=ROWS_.index(row), **row[2])


def row_id(row):
    typ, dt, m, n, ldi, ldo = row[1]
    kw = row[2]
    s = f"{row[0]}-{UNARY.name(typ).replace('TRANSFORM_', '')}-{DT.name(dt)}-{m}x{n}ld{ldi}_{ldo}"
    if "flags" in kw:
        f = kw["flags"]
        s += "-" + ("COLS" if f & COLS else "ROWS" if f & ROWS else "OFFS") + ("-i8" if f & I8 else "-i4")
    for k in ("batch", "off_in", "off_out", "off_idx", "hint", "idx", "note"):
        if k in kw:
            s += f"-{k}{kw[k]}" if k != "note" else f"-{kw[k]}"
    if kw.get("host_idx"):
        s += "-hostidx"
    if "bs_in" in kw or "bs_out" in kw:
        s += "-stride"
    return s


# ---- TRANSFORMS: every type, two shapes, four widths ------------------------------------------------------------------------------------------------------
def transform_shapes(typ):
    """[(m, n, ldi, ldo)] minimal, then more than 256 outputs with padded leading dimensions."""
    if typ == T.TRANSFORM_NORM_TO_NORMT:
        return [(5, 3, 6, 4), (37, 19, 40, 21)]
    if typ in H.NORM_TO_VNNI:
        v = H.NORM_TO_VNNI[typ]
        return [(3, v, 4, 5), (45, 3 * v + 1, 48, 47)]
    if typ in H.VNNI_TO_VNNIT:
        v = H.VNNI_TO_VNNIT[typ]
        return [(v, v, v, v), (12 * v, 6 * v, 12 * v + 3, 6 * v + 5)]
    if typ in H.NORM_TO_VNNIT:
        v = H.NORM_TO_VNNIT[typ]
        return [(v, 3, v, 3), (6 * v, 23, 6 * v + 2, 26)]
    if typ in H.VNNIT_TO_NORM:
        v = H.VNNIT_TO_NORM[typ]
        return [(3, v, 3, v), (23, 6 * v, 25, 6 * v + 3)]
    if typ in (T.TRANSFORM_VNNI4_TO_NORM, T.TRANSFORM_VNNI4_TO_VNNI2):
        return [(3, 4, 3, 3), (37, 10, 40, 39)]
    assert typ in H.PAD_N
    return [(3, 3, 4, 5), (37, 9, 40, 43)]


for _typ in H.ALL_TRANSFORMS:
    for _k, _s in enumerate(transform_shapes(_typ)):
        for _sz in (1, 2, 4, 8):
            R("TRANSFORMS", _typ, W[_sz], *_s, note=("min", "big")[_k])
R("TRANSFORMS", T.TRANSFORM_NORM_TO_VNNI4, DT.BF8, 45, 13, 48, 47, note="bf8")
R("TRANSFORMS", T.TRANSFORM_VNNI4_TO_NORM, DT.HF8, 37, 10, 40, 39, note="hf8")
R("TRANSFORMS", T.TRANSFORM_NORM_TO_VNNI2, DT.F16, 45, 7, 48, 47, note="f16")

# ---- TRANSPOSES -------------------------------------------------------------------------------------------------------------------------------------------
NT = T.TRANSFORM_NORM_TO_NORMT
for _sz in (1, 2, 4, 8):
    R("TRANSPOSES", NT, W[_sz], 37, 70, 40, 72, want="transpose_kernel")                   # partial 32-tiles on both axes
    R("TRANSPOSES", NT, W[_sz], 80, 96, 96, 112, want="transpose_vec_kernel")              # 64 + 16 rows, 64 + 32 columns
    R("TRANSPOSES", NT, W[_sz], 80, 96, 96, 112, hint=2, want="transpose_vec_kernel")      # the non-temporal instantiation
_V = (NT, DT.F32, 80, 96, 96, 112)       # vec = 4; the stride of a batch element is 96 * 95 + 80 = 9200 elements in, 112 * 79 + 96 = 8944 out, padded
R("TRANSPOSES", *_V, off_in=4, want="transpose_kernel", note="in-pointer")
R("TRANSPOSES", *_V, off_out=4, want="transpose_kernel", note="out-pointer")
R("TRANSPOSES", *_V, batch=2, bs_in=37124, bs_out=36096, want="transpose_kernel", note="bs_in%16")
R("TRANSPOSES", *_V, batch=2, bs_in=37120, bs_out=36100, want="transpose_kernel", note="bs_out%16")
R("TRANSPOSES", NT, DT.F32, 82, 96, 96, 112, want="transpose_kernel", note="m%vec")
R("TRANSPOSES", NT, DT.F32, 80, 96, 96, 114, want="transpose_kernel", note="ldo%vec")
R("TRANSPOSES", NT, DT.F32, 80, 98, 96, 112, want="transpose_kernel", note="n%vec")
R("TRANSPOSES", NT, DT.F32, 80, 96, 98, 112, want="transpose_kernel", note="ldi%vec")

# ---- VNNI2: NORM -> VNNI2, 16-bit -------------------------------------------------------------------------------------------------------------------------
V2 = T.TRANSFORM_NORM_TO_VNNI2
R("VNNI2", V2, DT.BF16, 64, 7, 64, 72, want="vnni2_vec_kernel")
R("VNNI2", V2, DT.BF16, 64, 7, 64, 72, hint=2, want="vnni2_vec_kernel")
R("VNNI2", T.TRANSFORM_NORM_TO_VNNI2_PAD, DT.BF16, 136, 131, 144, 136, want="vnni2_vec_kernel")
_Q = (V2, DT.BF16, 64, 7, 64, 72)        # a batch element: 64 * 6 + 64 = 448 elements in, 72 * 8 = 576 dwords out
R("VNNI2", *_Q, off_in=8, want="vnni2_quad_kernel", note="in-pointer")
R("VNNI2", *_Q, off_out=8, want="vnni2_quad_kernel", note="out-pointer")
R("VNNI2", *_Q, batch=2, bs_in=1032, bs_out=2560, want="vnni2_quad_kernel", note="bs_in%16")
R("VNNI2", *_Q, batch=2, bs_in=1024, bs_out=2568, want="vnni2_quad_kernel", note="bs_out%16")
R("VNNI2", V2, DT.BF16, 62, 7, 64, 72, want="vnni2_quad_kernel", note="m%4")
R("VNNI2", V2, DT.BF16, 64, 7, 66, 72, want="vnni2_quad_kernel", note="ldi%4")
R("VNNI2", V2, DT.BF16, 64, 7, 64, 74, want="vnni2_quad_kernel", note="ldo%4")
# inside vnni2_quad_kernel: the row start 4- or 2-byte aligned (pointer on an even / odd element x ldi even / odd), ldo % 4 (the short last thread of a row),
# 16- / 8- / 4-byte stores (output pointer), m % 4 (the partial load), m < ldo (zero-filled positions), n odd (the zero-filled pad row)
for _oi in (0, 2):
    for _ldi in (38, 39):
        for _r in range(4):
            for _oo in (0, 8, 4):
                for _k in range(4):
                    R("VNNI2Q", V2, DT.BF16, 32 + _k, 5, _ldi, 40 + _r, off_in=_oi, off_out=_oo, want="vnni2_quad_kernel")
# three batch elements, every one on another load and store branch: bs_in % 8 == 2 (rows 8-, 2-, 4-byte aligned), bs_out % 16 == 4 (16-, 4-, 8-byte stores)
R("VNNI2", V2, DT.BF16, 33, 5, 36, 40, batch=3, bs_in=402, bs_out=1044, want="vnni2_quad_kernel", note="stride-changes-case")
R("VNNI2", V2, DT.BF16, 11, 5, 13, 14, want="vnni2_pair_kernel", note="ldo<16")
R("VNNI2", V2, DT.BF16, 11, 5, 13, 14, batch=3, bs_in=132, bs_out=172, want="vnni2_pair_kernel", note="ldo<16")
R("VNNI2", V2, DT.BF16, 33, 5, 36, 40, off_out=2, want="xform_kernel", note="out-2-byte-aligned")
R("VNNI2", V2, DT.BF16, 33, 5, 36, 40, batch=2, bs_in=512, bs_out=1026, want="xform_kernel", note="bs_out-2-byte-aligned")

# ---- VNNI4: NORM -> VNNI4, 8-bit --------------------------------------------------------------------------------------------------------------------------
V4 = T.TRANSFORM_NORM_TO_VNNI4
for _r in range(4):
    R("VNNI4", V4, DT.I8, 132, 12 + _r, 136, 140, want="vnni4_vec_kernel")
R("VNNI4", T.TRANSFORM_NORM_TO_VNNI4_PAD, DT.I8, 132, 13, 136, 140, want="vnni4_vec_kernel")
_F = (V4, DT.I8, 132, 13, 136, 140)       # a batch element: 136 * 12 + 132 = 1764 bytes in, 140 * 16 = 2240 bytes out
R("VNNI4", *_F, off_in=1, want="xform_kernel", note="in-pointer+1")
R("VNNI4", *_F, off_in=4, want="xform_kernel", note="in-pointer+4")
R("VNNI4", *_F, off_out=1, want="xform_kernel", note="out-pointer+1")
R("VNNI4", *_F, off_out=4, want="xform_kernel", note="out-pointer+4")
R("VNNI4", *_F, batch=2, bs_in=2052, bs_out=2304, want="xform_kernel", note="bs_in%16")
R("VNNI4", *_F, batch=2, bs_in=2048, bs_out=2308, want="xform_kernel", note="bs_out%16")
R("VNNI4", V4, DT.I8, 130, 13, 136, 140, want="xform_kernel", note="m%4")
R("VNNI4", V4, DT.I8, 132, 13, 138, 140, want="xform_kernel", note="ldi%4")
R("VNNI4", V4, DT.I8, 132, 13, 136, 142, want="xform_kernel", note="ldo%4")

# ---- GATHER / SCATTER -------------------------------------------------------------------------------------------------------------------------------------
GS = (GATHER, SCATTER)
# COLS: 16-byte pieces of whole columns
for _sz in (1, 2, 4, 8):
    for _typ in GS:
        for _ix in (I4, I8):
            R("GS_COLS", _typ, W[_sz], 48, 90, 64, 80, flags=COLS | _ix, span=97, want="gather_cols_vec_kernel")
_C = (DT.F32, 48, 23, 64, 80)             # 16 bytes = 4 elements
for _typ in GS:
    R("GS_COLS", _typ, DT.F32, 46, 23, 64, 80, flags=COLS | I4, want="gather_scatter_kernel", note="m*sz%16")
    R("GS_COLS", _typ, DT.F32, 48, 23, 66, 80, flags=COLS | I4, want="gather_scatter_kernel", note="ldi*sz%16")
    R("GS_COLS", _typ, DT.F32, 48, 23, 64, 82, flags=COLS | I8, want="gather_scatter_kernel", note="ldo*sz%16")
    R("GS_COLS", _typ, *_C, flags=COLS | I4, off_in=4, want="gather_scatter_kernel", note="in-pointer")
    R("GS_COLS", _typ, *_C, flags=COLS | I8, off_out=8, want="gather_scatter_kernel", note="out-pointer")
R("GS_COLS", GATHER, *_C, flags=COLS | I4, span=30, batch=2, bs_in=8196, bs_out=7424, want="gather_scatter_kernel", note="bs_in%16")
R("GS_COLS", GATHER, *_C, flags=COLS | I4, span=30, batch=2, bs_in=8192, bs_out=7432, want="gather_scatter_kernel", note="bs_out%16")
R("GS_COLS", SCATTER, *_C, flags=COLS | I4, span=30, batch=2, bs_in=5896, bs_out=9728, want="gather_scatter_kernel", note="bs_in%16")
R("GS_COLS", SCATTER, *_C, flags=COLS | I4, span=30, batch=2, bs_in=5888, bs_out=9732, want="gather_scatter_kernel", note="bs_out%16")
R("GS_COLS", GATHER, DT.BF16, 48, 90, 64, 80, flags=COLS | I4, span=97, idx="equal", want="gather_cols_vec_kernel")          # every column the same one
# the generic kernel: every width x direction x mode, odd extents, more than one block
for _sz in (1, 2, 4, 8):
    for _typ in GS:
        for _mode in (COLS, ROWS, OFFS):
            _ix = I8 if (_sz in (2, 8)) == (_typ == GATHER) else I4
            _ld = (41, 39) if _typ == GATHER else (39, 41)          # the indexed side is the wider one
            R("GS_GENERIC", _typ, W[_sz], 37, 9, *_ld, flags=_mode | _ix, want="gather_scatter_kernel")

# ROWS through LDS, one column per workgroup: the staged side has ld = 48 (a multiple of 16 bytes at every width), 30 of its rows are named
for _sz in (1, 2, 4, 8):
    for _ix in (I4, I8):
        R("GS_ROWS", GATHER, W[_sz], 30, 7, 48, 33, flags=ROWS | _ix, want="gs_rows_lds_kernel")
        R("GS_ROWS", SCATTER, W[_sz], 30, 7, 33, 48, flags=ROWS | _ix, want="gs_rows_lds_kernel")
R("GS_ROWS", GATHER, DT.F32, 300, 3, 512, 301, flags=ROWS | I4, want="gs_rows_lds_kernel", note="two-trips")               # more than 256 indices, 128 vectors
R("GS_ROWS", SCATTER, DT.F32, 300, 3, 301, 512, flags=ROWS | I4, want="gs_rows_lds_kernel", note="two-trips")
R("GS_ROWS", GATHER, DT.F32, 24, 7, 48, 33, flags=ROWS | I4, want="gs_rows_lds_kernel", note="2m==rows")
R("GS_ROWS", GATHER, DT.F32, 23, 7, 48, 33, flags=ROWS | I4, want="gather_scatter_kernel", note="2m==rows-2")
R("GS_ROWS", SCATTER, DT.F32, 24, 7, 33, 48, flags=ROWS | I4, want="gs_rows_lds_kernel", note="2m==rows")
R("GS_ROWS", SCATTER, DT.F32, 23, 7, 33, 48, flags=ROWS | I4, want="gather_scatter_kernel", note="2m==rows-2")
R("GS_ROWS", GATHER, DT.F32, 8192, 2, 16384, 8192, flags=ROWS | I4, want="gs_rows_lds_kernel", note="64KiB")               # rows * sz == 65536 exactly
R("GS_ROWS", GATHER, DT.F32, 8194, 2, 16388, 8194, flags=ROWS | I4, want="gather_scatter_kernel", note="64KiB+16")
R("GS_ROWS", SCATTER, DT.F32, 8192, 2, 8192, 16384, flags=ROWS | I4, want="gs_rows_lds_kernel", note="64KiB")
R("GS_ROWS", GATHER, DT.F32, 30, 7, 46, 33, flags=ROWS | I4, want="gather_scatter_kernel", note="rows*sz%16")
R("GS_ROWS", GATHER, DT.F32, 30, 7, 48, 33, flags=ROWS | I4, off_in=4, want="gather_scatter_kernel", note="staged-base")
R("GS_ROWS", SCATTER, DT.F32, 30, 7, 33, 48, flags=ROWS | I4, off_out=4, want="gather_scatter_kernel", note="staged-base")
R("GS_ROWS", GATHER, DT.F32, 30, 7, 48, 33, flags=ROWS | I4, off_out=4, want="gs_rows_lds_kernel", note="other-side-off")  # only the staged side has to be aligned
R("GS_ROWS", GATHER, DT.F32, 30, 7, 48, 33, flags=ROWS | I4, batch=2, bs_in=1352, bs_out=1024, want="gather_scatter_kernel", note="staged-stride")
R("GS_ROWS", GATHER, DT.BF16, 40, 7, 48, 41, flags=ROWS | I4, idx="reversed", want="gs_rows_lds_kernel")
# ROWS, two columns per workgroup (gather of 2- and 4-byte payloads from n = 64 on)
for _dt in (DT.BF16, DT.F32):
    for _ix in (I4, I8):
        R("GS_ROWS2", GATHER, _dt, 30, 64, 48, 33, flags=ROWS | _ix, want="gs_rows_lds_multi_kernel")
        R("GS_ROWS2", GATHER, _dt, 30, 65, 48, 33, flags=ROWS | _ix, want="gs_rows_lds_multi_kernel")                     # a short last workgroup
    R("GS_ROWS2", GATHER, _dt, 30, 63, 48, 33, flags=ROWS | I4, want="gs_rows_lds_kernel", note="n=63")
    R("GS_ROWS2", GATHER, _dt, 300, 64, 512, 301, flags=ROWS | I4, want="gs_rows_lds_multi_kernel", note="two-trips")
R("GS_ROWS2", SCATTER, DT.F32, 30, 64, 33, 48, flags=ROWS | I4, want="gs_rows_lds_kernel", note="scatter-has-one-column-form-only")
R("GS_ROWS2", GATHER, DT.F64, 30, 64, 48, 33, flags=ROWS | I4, want="gs_rows_lds_kernel", note="8-byte-has-one-column-form-only")
R("GS_ROWS2", GATHER, DT.F32, 4096, 64, 8192, 4096, flags=ROWS | I4, want="gs_rows_lds_multi_kernel", note="2x32KiB")      # 2 * rows * sz == 65536 exactly
R("GS_ROWS2", GATHER, DT.F32, 4098, 64, 8196, 4098, flags=ROWS | I4, want="gs_rows_lds_kernel", note="2x32KiB+16")         # falls back to one column
R("GS_ROWS2", GATHER, DT.BF16, 8192, 64, 16384, 8192, flags=ROWS | I8, want="gs_rows_lds_multi_kernel", note="2x32KiB")

# OFFS, four offsets per thread (2- and 4-byte payloads, 4-byte offsets): 44 x 25 / 4 = 275 threads
for _dt in (DT.BF16, DT.F32):
    _sz = 2 if _dt == DT.BF16 else 4
    for _typ in GS:
        R("GS_OFFS", _typ, _dt, 44, 25, 48, 48, flags=OFFS | I4, want="gs_offs_vec4_kernel")
        R("GS_OFFS", _typ, _dt, 42, 25, 48, 48, flags=OFFS | I4, want="gather_scatter_kernel", note="m%4")
        R("GS_OFFS", _typ, _dt, 44, 25, 48, 48, flags=OFFS | I8, want="gather_scatter_kernel", note="8-byte-offsets")
        R("GS_OFFS", _typ, _dt, 44, 25, 48, 48, flags=OFFS | I4, off_idx=4, want="gather_scatter_kernel", note="index-pointer")
        _side = "off_out" if _typ == GATHER else "off_in"
        R("GS_OFFS", _typ, _dt, 44, 25, 48, 48, flags=OFFS | I4, want="gather_scatter_kernel", note="contiguous-side", **{_side: _sz})
        R("GS_OFFS", _typ, _dt, 44, 25, 48, 48, flags=OFFS | I4, want="gs_offs_vec4_kernel", note="random-side-off", **{("off_in" if _typ == GATHER else "off_out"): _sz})
        _ld = (48, 46) if _typ == GATHER else (46, 48)
        R("GS_OFFS", _typ, _dt, 44, 25, *_ld, flags=OFFS | I4, want="gather_scatter_kernel", note="ld%4")
for _typ in GS:
    R("GS_OFFS", _typ, DT.F64, 44, 25, 48, 48, flags=OFFS | I4, want="gather_scatter_kernel", note="8-byte-payload")
    R("GS_OFFS", _typ, DT.I8, 44, 25, 48, 48, flags=OFFS | I4, want="gather_scatter_kernel", note="1-byte-payload")

# ---- BATCH: every path once as a batch of 3 with padded strides; the index list is shared -----------------------------------------------------------------------
R("BATCH", NT, DT.F32, 80, 96, 96, 112, batch=3, want="transpose_vec_kernel")
R("BATCH", NT, DT.BF16, 37, 70, 40, 72, batch=3, want="transpose_kernel")
R("BATCH", V2, DT.BF16, 64, 7, 64, 72, batch=3, want="vnni2_vec_kernel")
R("BATCH", V4, DT.I8, 132, 13, 136, 140, batch=3, want="vnni4_vec_kernel")
R("BATCH", T.TRANSFORM_VNNI4T_TO_NORM, DT.BF16, 23, 24, 25, 27, batch=3, want="xform_kernel")
R("BATCH", T.TRANSFORM_PADNM_MOD4, DT.I8, 37, 9, 40, 43, batch=3, want="xform_kernel")
for _typ in GS:
    R("BATCH", _typ, DT.F32, 48, 23, 64, 80, flags=COLS | I4, batch=3, want="gather_cols_vec_kernel")
    R("BATCH", _typ, DT.BF16, 37, 9, *((41, 39) if _typ == GATHER else (39, 41)), flags=COLS | I8, batch=3, want="gather_scatter_kernel")
    R("BATCH", _typ, DT.I8, 37, 9, *((41, 39) if _typ == GATHER else (39, 41)), flags=ROWS | I4, batch=3, want="gather_scatter_kernel")
    R("BATCH", _typ, DT.F32, 37, 9, *((41, 39) if _typ == GATHER else (39, 41)), flags=OFFS | I8, batch=3, want="gather_scatter_kernel")
    R("BATCH", _typ, DT.F32, 30, 7, *((48, 33) if _typ == GATHER else (33, 48)), flags=ROWS | I4, batch=3, want="gs_rows_lds_kernel")
    R("BATCH", _typ, DT.BF16, 44, 25, 48, 48, flags=OFFS | I4, batch=3, want="gs_offs_vec4_kernel")
R("BATCH", GATHER, DT.BF16, 30, 65, 48, 33, flags=ROWS | I8, batch=3, want="gs_rows_lds_multi_kernel")

# ---- HOST: the index list in plain host memory (the runtime stages it), device operands --------------------------------------------------------------------------
for _typ in GS:
    R("HOST", _typ, DT.F32, 48, 23, 64, 80, flags=COLS | I4, host_idx=True, want="gather_cols_vec_kernel")
    R("HOST", _typ, DT.F32, 30, 7, *((48, 33) if _typ == GATHER else (33, 48)), flags=ROWS | I8, host_idx=True, want="gs_rows_lds_kernel")
    # (the staged copy is 16-byte aligned whatever the caller's pointer is: the four-offset kernel runs although the host list starts 4 bytes into its allocation)
    R("HOST", _typ, DT.F32, 44, 25, 48, 48, flags=OFFS | I4, host_idx=True, off_idx=4, want="gs_offs_vec4_kernel")
    R("HOST", _typ, DT.I8, 37, 9, *((41, 39) if _typ == GATHER else (39, 41)), flags=OFFS | I8, host_idx=True, want="gather_scatter_kernel")

TABLES = sorted({r[0] for r in ROWS_})


def rows_of(table):
    return [r for r in ROWS_ if r[0] == table]


@pytest.mark.parametrize("row", ROWS_, ids=[row_id(r) for r in ROWS_])
def test_move_bit_exact(row):
    H.run_case(make(row))


@pytest.mark.parametrize("key", sorted(REFUSED), ids=lambda k: f"{UNARY.name(k[0])}-{DT.name(k[1])}")
def test_refused_by_dispatch(key):
    typ, dt = key
    assert not capi.load().dispatch_meltw_unary(typ, capi.UnaryShape(16, 16, 16, 16, dt, dt, DT.F32), 0), REFUSED[key]
