"""Parity of the data-movement TPPs (the transposes, the VNNI re-layouts, the padding copies, GATHER / SCATTER) byte for byte over WHOLE allocations, on every path of
csrc/meltw_kernels.hip: launch_meltw -- what tests/meltw_ew_helpers.py and tests/meltw_reduce_helpers.py do for the element-wise and the reduction TPPs.

  MoveCase         one TPP call: type, flags, payload type, m, n, ldi, ldo, batch count and byte strides, byte offsets of the in / out / index pointers into their
                   allocations, index width, index list on the host or the device, streaming hint.  The footprint of every operand follows from move_numpy's index
                   arithmetic (not from ld * n: the VNNI layouts interleave rows, the padded forms write past n, VNNIvT_TO_NORM swaps m and n); an allocation is
                   offset + (batch - 1) * stride + footprint + SLACK bytes.  A row gather / scatter owns ld * n elements of its indexed side: the staged kernels move
                   [j * ld, j * ld + ld) of every column, the last one included ("Gather / scatter: what the indexed operand must own").
  input values     4- and 8-byte payloads: a hashed counter, all distinct; 2-byte: a counter times an odd number mod 2^16, distinct over any 65536 consecutive
                   elements; 1-byte: random.  An element routed from the wrong place cannot compare equal by accident (1-byte: not all of them can).
  poison           the output allocation starts from random bytes, the ones in front of the pointer and behind the footprint included; the oracle and the device
                   start from the same bytes.
  move_numpy       every operation as numpy index arithmetic, from the reference's loop nests [ref: src/generator_mateltwise_reference_impl.c]: transpose :376-422,
                   VNNIv -> VNNIvT :424-530, NORM -> VNNIv (and _PAD) :532-557 / :686-784, NORM -> VNNIvT :558-578 / :644-684, VNNIvT -> NORM :580-642 (M = desc.n,
                   N = desc.m), VNNI4 -> NORM :786-803, VNNI4 -> VNNI2 :805-822, the padding copies :824-964, gather / scatter :1444-1790.  One deviation, the oracle's:
                   NORM -> VNNIv with n % v != 0 reads the rows n .. Nn - 1 of the input in the reference (whatever lies behind the matrix); the contract here is
                   the zero fill the same function starts with.  Returns the expected bytes of the whole output allocation and the mask of the bytes written.
  expected_kernel  launch_meltw's branch for this family restated, gs_rows_lds_ok included: (name, instantiation) from the REAL addresses.
  run_case         oracle once per batch element on host copies; one call (batch 1) or libxsmm_hip_meltw_unary_batch_strided (aux stride 0: the index list is shared);
                   the kernel name against expected_kernel; np.array_equal over the whole output allocation; the input comes back untouched.
"""
import ctypes as C

import numpy as np

from libxsmm_amd import capi
from libxsmm_amd.capi import DT, UNARY, UNARY_FLAG
from oracle import pyoracle

OP_UNARY = 1
SLACK = 64                      # bytes behind the last footprint of every allocation
GATHER, SCATTER = UNARY.GATHER, UNARY.SCATTER
COLS, ROWS, OFFS = UNARY_FLAG.GS_COLS, UNARY_FLAG.GS_ROWS, UNARY_FLAG.GS_OFFS
MODE_NAME = {COLS: "COLS", ROWS: "ROWS", OFFS: "OFFS"}
I4, I8 = UNARY_FLAG.IDX_SIZE_4BYTES, UNARY_FLAG.IDX_SIZE_8BYTES

T = UNARY
NORM_TO_VNNI = {T.TRANSFORM_NORM_TO_VNNI2: 2, T.TRANSFORM_NORM_TO_VNNI2_PAD: 2, T.TRANSFORM_NORM_TO_VNNI4: 4, T.TRANSFORM_NORM_TO_VNNI4_PAD: 4,
                T.TRANSFORM_NORM_TO_VNNI8: 8, T.TRANSFORM_NORM_TO_VNNI8_PAD: 8}
VNNI_TO_VNNIT = {T.TRANSFORM_VNNI2_TO_VNNI2T: 2, T.TRANSFORM_VNNI4_TO_VNNI4T: 4, T.TRANSFORM_VNNI8_TO_VNNI8T: 8}
NORM_TO_VNNIT = {T.TRANSFORM_NORM_TO_VNNI2T: 2, T.TRANSFORM_NORM_TO_VNNI4T: 4, T.TRANSFORM_NORM_TO_VNNI8T: 8}
VNNIT_TO_NORM = {T.TRANSFORM_VNNI2T_TO_NORM: 2, T.TRANSFORM_VNNI4T_TO_NORM: 4, T.TRANSFORM_VNNI8T_TO_NORM: 8}
PAD_N = {T.TRANSFORM_PADM_MOD2: 1, T.TRANSFORM_PADM_MOD4: 1, T.TRANSFORM_PADN_MOD2: 2, T.TRANSFORM_PADNM_MOD2: 2, T.TRANSFORM_PADN_MOD4: 4, T.TRANSFORM_PADNM_MOD4: 4}
# the seven modes of xform_kernel (csrc/meltw_kernels.hip: XformMode) and the v each one is launched with
XF_MODES = {"NORM_TO_VNNI": (2, 4, 8), "VNNI_TO_VNNIT": (2, 4, 8), "NORM_TO_VNNIT": (2, 4, 8), "VNNIT_TO_NORM": (2, 4, 8), "VNNI4_TO_NORM": (4,), "VNNI4_TO_VNNI2": (4,),
            "PAD": (1, 2, 4)}
ALL_TRANSFORMS = ([T.TRANSFORM_NORM_TO_NORMT] + list(NORM_TO_VNNI) + list(VNNI_TO_VNNIT) + list(NORM_TO_VNNIT) + list(VNNIT_TO_NORM)
                  + [T.TRANSFORM_VNNI4_TO_NORM, T.TRANSFORM_VNNI4_TO_VNNI2] + list(PAD_N))
assert len(ALL_TRANSFORMS) == 24 and len(set(ALL_TRANSFORMS)) == 24


def xform_mode(typ):
    """(mode name, v) as csrc/meltw_kernels.hip: xform_mode maps the type; (None, 0) for a type it does not know."""
    for table, name in ((NORM_TO_VNNI, "NORM_TO_VNNI"), (VNNI_TO_VNNIT, "VNNI_TO_VNNIT"), (NORM_TO_VNNIT, "NORM_TO_VNNIT"), (VNNIT_TO_NORM, "VNNIT_TO_NORM"), (PAD_N, "PAD")):
        if typ in table:
            return name, table[typ]
    if typ == T.TRANSFORM_VNNI4_TO_NORM:
        return "VNNI4_TO_NORM", 4
    if typ == T.TRANSFORM_VNNI4_TO_VNNI2:
        return "VNNI4_TO_VNNI2", 4
    return None, 0


def _up(x, q):
    return (x + q - 1) // q * q


def _grid(*extents):
    """index arrays of a loop nest, flattened."""
    return [g.ravel() for g in np.meshgrid(*[np.arange(e, dtype=np.int64) for e in extents], indexing="ij")]


def transform_moves(typ, m, n, ldi, ldo):
    """(src, dst, zeroed): element indices the reference's loop nest reads and writes, and the number of leading output elements it zeroes first."""
    M, N = m, n
    if typ == T.TRANSFORM_NORM_TO_NORMT:                                   # [ref: :376-422]
        i, j = _grid(N, M)
        return i * ldi + j, j * ldo + i, 0
    if typ in NORM_TO_VNNI:                                                 # [ref: :532-557, :686-784]
        v = NORM_TO_VNNI[typ]
        Nn = _up(N, v)
        j, i, j2 = _grid(Nn // v, M, v)
        keep = j * v + j2 < N                                               # (the rows past N: see the module docstring)
        return ((j * v + j2) * ldi + i)[keep], (j * ldo * v + i * v + j2)[keep], ldo * Nn
    if typ in VNNI_TO_VNNIT:                                                # [ref: :424-530]
        v = VNNI_TO_VNNIT[typ]
        j, i, j2, i2 = _grid(M // v, N // v, v, v)
        return i * ldi * v + i2 + (j * v + j2) * v, j * ldo * v + j2 + (i * v + i2) * v, 0
    if typ in NORM_TO_VNNIT:                                                # [ref: :558-578, :644-684]
        v = NORM_TO_VNNIT[typ]
        i, j, i2 = _grid(M // v, N, v)
        return j * ldi + i * v + i2, i * ldo * v + j * v + i2, 0
    if typ in VNNIT_TO_NORM:                                                # [ref: :580-642]: M = desc.n, N = desc.m
        v = VNNIT_TO_NORM[typ]
        i, j, i2 = _grid(n // v, m, v)
        return i * ldi * v + j * v + i2, j * ldo + i * v + i2, 0
    if typ == T.TRANSFORM_VNNI4_TO_NORM:                                    # [ref: :786-803]
        i, j = _grid(N, M)
        return (i // 4) * ldi * 4 + j * 4 + i % 4, i * ldo + j, 0
    if typ == T.TRANSFORM_VNNI4_TO_VNNI2:                                   # [ref: :805-822]
        i, j = _grid(N, M)
        return (i // 4) * ldi * 4 + j * 4 + i % 4, (i // 2) * ldo * 2 + j * 2 + i % 2, 0
    if typ in PAD_N:                                                        # [ref: :824-964]
        j, i = _grid(N, M)
        return j * ldi + i, j * ldo + i, ldo * _up(N, PAD_N[typ])
    raise ValueError(typ)


def gs_moves(typ, mode, m, n, ldi, ldo, idx):
    """(src, dst) of GATHER / SCATTER [ref: :1444-1790]; idx: the index list as int64."""
    if mode == COLS:
        a, b = _grid(n, m)
        return (b + idx[a] * ldi, b + a * ldo) if typ == GATHER else (b + a * ldi, b + idx[a] * ldo)
    if mode == ROWS:
        a, b = _grid(m, n)
        return (idx[a] + b * ldi, a + b * ldo) if typ == GATHER else (a + b * ldi, idx[a] + b * ldo)
    b, a = _grid(n, m)
    return (idx[a + b * m], a + b * ldo) if typ == GATHER else (a + b * ldi, idx[a + b * m])


def distinct_values(count, sz, rng):
    """count elements of sz bytes as a uint8 array (see the module docstring)."""
    k = np.arange(count, dtype=np.uint64)
    if sz == 8:
        v = (k * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567)).astype(np.uint64)           # an odd multiplier: a bijection of 2^64
    elif sz == 4:
        v = ((k * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xffffffff)).astype(np.uint32)
    elif sz == 2:
        v = ((k * np.uint64(40503) + np.uint64(77)) & np.uint64(0xffff)).astype(np.uint16)
    else:
        v = rng.integers(0, 256, count, dtype=np.uint8)
    return v.view(np.uint8).copy()


class MoveCase:
    """One data-movement TPP (see the module docstring).

    flags      GATHER / SCATTER: COLS | ROWS | OFFS, or-ed with I4 | I8; transforms: 0
    bs_in/out  batch strides in bytes (default: the footprint + 64, rounded up to 256)
    off_*      bytes between the allocation (256-byte aligned on the device) and the pointer
    span       the extent of the indexed side the indices are drawn from: columns (COLS; default n + 7), elements (OFFS; default 2 m n + 9); ROWS: always the leading
               dimension of that side
    idx        'random' (gather: WITH repeats; scatter: without) | 'equal' | 'reversed'
    want       the kernel name the row was written for"""

    def __init__(self, typ, dt, m, n, ldi, ldo, flags=0, batch=1, bs_in=None, bs_out=None, off_in=0, off_out=0, off_idx=0, host_idx=False, hint=None,
                 span=None, idx="random", seed=0, want=None, note=""):
        self.typ, self.dt, self.m, self.n, self.ldi, self.ldo, self.flags, self.batch = typ, dt, m, n, ldi, ldo, flags, batch
        self.off_in, self.off_out, self.off_idx, self.host_idx, self.hint, self.want, self.note = off_in, off_out, off_idx, host_idx, hint, want, note
        self.sz = sz = capi.DT_SIZE[dt]
        self.gs = typ in (GATHER, SCATTER)
        rng = np.random.default_rng(1000 + seed)
        assert off_in % sz == 0 and off_out % sz == 0
        self.idx_buf = None
        if self.gs:
            self.mode = COLS if flags & COLS else ROWS if flags & ROWS else OFFS
            self.isz = 8 if flags & I8 else 4
            assert off_idx % self.isz == 0
            count = {COLS: n, ROWS: m, OFFS: m * n}[self.mode]
            ld_idx = ldi if typ == GATHER else ldo                                      # the indexed side
            self.span = ld_idx if self.mode == ROWS else span if span is not None else (n + 7 if self.mode == COLS else 2 * m * n + 9)
            if idx == "equal":
                assert typ == GATHER
                lst = np.full(count, self.span // 2)
            elif idx == "reversed":
                assert self.span >= count
                lst = np.arange(count)[::-1]
            elif typ == GATHER:
                lst = rng.integers(0, self.span, count)
                lst[: min(3, count)] = lst[-1]                                          # a repeat whatever the draw
            else:
                assert self.span >= count
                lst = rng.permutation(self.span)[:count]
            self.idx = np.asarray(lst, dtype=np.int64)
            self.idx_buf = rng.integers(0, 256, off_idx + count * self.isz + 16, dtype=np.uint8)
            self.idx_buf[off_idx: off_idx + count * self.isz] = self.idx.astype(np.uint64 if self.isz == 8 else np.uint32).view(np.uint8)
            self.src, self.dst = gs_moves(typ, self.mode, m, n, ldi, ldo, self.idx)
            self.zeroed = 0
            plain = ldi * (n - 1) + m if typ == SCATTER else ldo * (n - 1) + m
            indexed = {COLS: ld_idx * (self.span - 1) + m, ROWS: ld_idx * n, OFFS: self.span}[self.mode]
            self.in_elems, self.out_elems = (indexed, plain) if typ == GATHER else (plain, indexed)
        else:
            self.src, self.dst, self.zeroed = transform_moves(typ, m, n, ldi, ldo)
            self.in_elems = int(self.src.max()) + 1
            self.out_elems = max(int(self.dst.max()) + 1, self.zeroed)
        assert int(self.src.max()) < self.in_elems and int(self.dst.max()) < self.out_elems and self.src.min() >= 0 and self.dst.min() >= 0
        assert np.unique(self.dst).size == self.dst.size, "two writes to one element: the result would depend on their order"
        pad = lambda b: _up(b + 64, 256)
        self.bs_in = 0 if batch == 1 else pad(self.in_elems * sz) if bs_in is None else bs_in
        self.bs_out = 0 if batch == 1 else pad(self.out_elems * sz) if bs_out is None else bs_out
        assert self.bs_in % sz == 0 and self.bs_out % sz == 0
        assert batch == 1 or (self.bs_in >= self.in_elems * sz and self.bs_out >= self.out_elems * sz), "batch elements overlap"
        in_bytes = off_in + (batch - 1) * self.bs_in + self.in_elems * sz + SLACK
        out_bytes = off_out + (batch - 1) * self.bs_out + self.out_elems * sz + SLACK
        assert max(in_bytes, out_bytes) < 4 << 20
        self.inp = distinct_values(_up(in_bytes, sz) // sz, sz, rng)[:in_bytes]
        self.out0 = rng.integers(0, 256, out_bytes, dtype=np.uint8)

    def __repr__(self):
        return self.id()

    def id(self):
        s = f"{UNARY.name(self.typ).replace('TRANSFORM_', '')}-{DT.name(self.dt)}-{self.m}x{self.n}ld{self.ldi}_{self.ldo}"
        if self.gs:
            s += f"-{MODE_NAME[self.mode]}-i{self.isz}"
        if self.batch > 1:
            s += f"-b{self.batch}"
        return s + (f"-{self.note}" if self.note else "")

    # -- descriptors
    def desc(self):
        return pyoracle.MeltwDesc(self.m, self.n, self.ldi, self.ldo, 0, 0, self.dt, DT.UNSUPPORTED, DT.UNSUPPORTED, DT.F32, self.dt, self.flags, self.typ, OP_UNARY)

    def shape(self):
        return capi.UnaryShape(self.m, self.n, self.ldi, self.ldo, self.dt, self.dt, DT.F32)

    def param(self, in_base, out_base, idx_base, b=0):
        p = capi.UnaryParam()
        p.in_.primary = in_base + self.off_in + b * self.bs_in
        p.out.primary = out_base + self.off_out + b * self.bs_out
        if self.gs:
            if self.typ == GATHER:
                p.in_.secondary = idx_base + self.off_idx
            else:
                p.out.secondary = idx_base + self.off_idx
        return p

    def run_oracle(self):
        """the oracle's whole output allocation."""
        x, out = self.inp.copy(), self.out0.copy()
        ib = self.idx_buf.ctypes.data if self.gs else 0
        for b in range(self.batch):
            pyoracle.oracle().meltw(self.param(x.ctypes.data, out.ctypes.data, ib, b), self.desc())
        assert np.array_equal(x, self.inp)
        return out

    def run_reference(self, ref):
        x, out = self.inp.copy(), self.out0.copy()
        ib = self.idx_buf.ctypes.data if self.gs else 0
        for b in range(self.batch):
            p = self.param(x.ctypes.data, out.ctypes.data, ib, b)
            ref.lib.xref_reference_meltw_unary(C.byref(p), self.typ, self.shape(), self.flags)
        return out

    def expected(self, in_base=0, out_base=0, idx_base=0):
        """expected_kernel for allocations at these addresses (default: the nominal ones, allocation base % 256 == 0)."""
        return expected_kernel(self, in_base + self.off_in, out_base + self.off_out, idx_base + self.off_idx)


def move_numpy(case):
    """(expected bytes of the whole output allocation, mask of the bytes the operation writes)."""
    sz = case.sz
    out, mask = case.out0.copy(), np.zeros(case.out0.size, dtype=bool)
    e = np.arange(sz, dtype=np.int64)[None, :]
    for b in range(case.batch):
        pi, po = case.off_in + b * case.bs_in, case.off_out + b * case.bs_out
        if case.zeroed:
            out[po: po + case.zeroed * sz] = 0
            mask[po: po + case.zeroed * sz] = True
        d = (po + case.dst[:, None] * sz + e).ravel()
        out[d] = case.inp[(pi + case.src[:, None] * sz + e).ravel()]
        mask[d] = True
    return out, mask


# ---- which kernel ---------------------------------------------------------------------------------------------------------------------------------------
def gs_rows_lds_ok(case, in_addr, out_addr):
    """csrc/meltw_kernels.hip: gs_rows_lds_ok."""
    gather = case.typ == GATHER
    rows = case.ldi if gather else case.ldo
    if rows <= 0 or (rows * case.sz) % 16 != 0 or rows * case.sz > 65536 or 2 * case.m < rows or case.n <= 0 or case.n > 65535 * 16 or case.batch >= 65536:
        return False
    base = (in_addr | case.bs_in) if gather else (out_addr | case.bs_out)
    return base & 15 == 0


def expected_kernel(case, in_addr, out_addr, idx_addr=0):
    """(name, instantiation) launch_meltw starts for this case with the pointers at these addresses.  The instantiation is what the launcher switches on: the payload
    width, `nt` (the streaming hint 2) where the kernel has a non-temporal form, xform_kernel's mode and v, the direction and mode of a gather / scatter, the
    columns per workgroup of the two-column row gather.  An index list in plain host memory is staged by the runtime into a 256-byte aligned scratch block.
    Left out: the launcher's element-count clauses (2^31 tiles, 2^32 - 256 threads, 65536 batch elements in grid.y) -- MoveCase keeps every operand below 4 MiB -- and
    the non-temporal choice the runtime makes on its own under hint 0 (256 MiB per launch, or recent operands beyond the cache): `nt` is claimed for hint 2 only, and
    the kernel NAME does not depend on it."""
    sz, m, n, ldi, ldo, typ = case.sz, case.m, case.n, case.ldi, case.ldo, case.typ
    bs_in, bs_out = case.bs_in, case.bs_out
    nt = ("nt",) if case.hint == 2 else ()
    mode, v = xform_mode(typ)
    base16 = (in_addr | out_addr | bs_in | bs_out) & 15 == 0
    vec = 16 // sz
    if typ == T.TRANSFORM_NORM_TO_NORMT and base16 and m % vec == 0 and n % vec == 0 and ldi % vec == 0 and ldo % vec == 0:
        return "transpose_vec_kernel", (sz,) + nt
    if mode == "NORM_TO_VNNI" and v == 2 and sz == 2 and base16 and m % 4 == 0 and ldi % 4 == 0 and ldo % 4 == 0:
        return "vnni2_vec_kernel", (4,) + nt
    if mode == "NORM_TO_VNNI" and v == 2 and sz == 2 and (out_addr | bs_out) % 4 == 0 and case.batch < 65536:
        if ldo >= 16 and (in_addr | bs_in) % 2 == 0:
            return "vnni2_quad_kernel", ()
        return "vnni2_pair_kernel", ()
    if mode == "NORM_TO_VNNI" and v == 4 and sz == 1 and base16 and m % 4 == 0 and ldi % 4 == 0 and ldo % 4 == 0:
        return "vnni4_vec_kernel", ()
    if typ == T.TRANSFORM_NORM_TO_NORMT:
        return "transpose_kernel", (sz,)
    if mode is not None:
        return "xform_kernel", (sz, mode, v)
    assert case.gs
    gather = typ == GATHER
    way = "gather" if gather else "scatter"
    if case.host_idx:
        idx_addr = 0
    if (case.flags & COLS) and (m * sz) % 16 == 0 and (ldi * sz) % 16 == 0 and (ldo * sz) % 16 == 0 and base16 and case.batch < 65536:
        return "gather_cols_vec_kernel", (sz, way)
    if (case.flags & ROWS) and gs_rows_lds_ok(case, in_addr, out_addr):
        lds_bytes = (ldi if gather else ldo) * sz
        if gather and sz in (2, 4) and n >= 64 and (ldi * sz) % 16 == 0 and lds_bytes * 2 <= 65536:      # nc_env = 2: four columns are never chosen
            return "gs_rows_lds_multi_kernel", (sz, 2)
        return "gs_rows_lds_kernel", (sz, way)
    if not (case.flags & (COLS | ROWS | I8)) and sz in (2, 4) and m % 4 == 0 and idx_addr % 16 == 0:
        side, ld = ((out_addr | bs_out), ldo) if gather else ((in_addr | bs_in), ldi)
        if side % (4 * sz) == 0 and (ld * sz) % (4 * sz) == 0:
            return "gs_offs_vec4_kernel", (sz, way)
    return "gather_scatter_kernel", (sz, way, MODE_NAME[case.mode])


# ---- one call -------------------------------------------------------------------------------------------------------------------------------------------
def _upload(x):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    assert t.data_ptr() % 256 == 0
    return t


def dispatch(case):
    return capi.load().dispatch_meltw_unary(case.typ, case.shape(), case.flags)


def run_case(case):
    """Runs the oracle and the device on the same bytes and asserts the kernel that ran and the WHOLE output allocation.  Returns (got, expected bytes)."""
    api = capi.load()
    ref = case.run_oracle()
    h = dispatch(case)
    assert h, "dispatch returned NULL"
    d_in, d_out = _upload(case.inp), _upload(case.out0)
    d_idx = _upload(case.idx_buf) if (case.gs and not case.host_idx) else None
    idx_base = 0 if not case.gs else case.idx_buf.ctypes.data if case.host_idx else d_idx.data_ptr()
    want = case.expected(d_in.data_ptr(), d_out.data_ptr(), idx_base)
    assert case.want is None or want[0] == case.want, f"{case.id()}: expected_kernel says {want}, the row was written for {case.want}"
    p = case.param(d_in.data_ptr(), d_out.data_ptr(), idx_base)
    old = api.hip_get_streaming_hint()
    try:
        if case.hint is not None:
            api.hip_set_streaming_hint(case.hint)
        if case.batch == 1:
            capi.Api.call(h, p)
        else:
            api.hip_meltw_unary_batch_strided(h, C.byref(p), case.batch, case.bs_in, case.bs_out, 0)
        api.hip_sync(); api.check()
    finally:
        if case.hint is not None:
            api.hip_set_streaming_hint(old)
    ran = api.hip_kernel_name(h, 1 if case.batch > 1 else 0).decode()
    assert ran == want[0], f"{case.id()}: {ran} ran, expected {want}"
    got = d_out.cpu().numpy()
    assert np.array_equal(d_in.cpu().numpy(), case.inp), f"{case.id()}: the input was written"
    if not np.array_equal(got, ref):
        bad = np.flatnonzero(got != ref)
        raise AssertionError(f"{case.id()} on {want}: {bad.size} of {got.size} bytes differ from the oracle's allocation; first at byte {int(bad[0])} "
                             f"(the pointer is at byte {case.off_out}): oracle 0x{int(ref[bad[0]]):02x}, device 0x{int(got[bad[0]]):02x}")
    return got, ref
