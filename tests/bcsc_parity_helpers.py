"""Block-sparse (BCSC) GEMM parity, per element: what tests/gemm_ld_helpers.py does for the dense kernels, for libxsmm_create_packed_spgemm_bcsc.

  wide(rng, count, dt)     bf16 / f32 normal numbers: a full random significand times 2^e, e uniform in [-8, 8], both signs, one value in eight an exact zero
                           (no denormals, infinities or NaNs).
  edge_columns(...)        sparse_helpers.make_bcsc plus the pattern edges: a block column holding every k-block, one without any block, one whose row indices are
                           stored in DESCENDING order and use the first and the last k-block; never a duplicate row index within a column.
  BcscCase(**kw)           one problem: pattern, values of B, every M-block its own random A, start values of C; run_oracle() is the reference's loop.
  place(arr, skew, ...)    the array inside a larger device buffer, `margin + skew` bytes in and `margin` bytes in front of the buffer's end: the margins of A and of
                           B's values hold the type's NaN (0x7f bytes for integers), the margins of C a finite sentinel; all of them must come back bit for bit.
  ref64(case)              (ref, mag, terms) in float64 from the dense K x N matrix of the pattern: ref = einsum("bkm,kn->bnm", A, dense) (+ C0 with beta = 1), mag the
                           same on absolute values, terms[n] = stored blocks of n's block column * bk (+ 1 with beta = 1).  8-bit integers: int64, exact.
  assert_bcsc(...)         every element of every M-block inside gemm_ld_helpers.bound64 -- |got - ref| <= e + u_c (|ref| + e) + 2^-126, e = (terms + 2) 2^-24 mag, the
                           bound of a float32 sum in ANY order followed by one rounding to nearest --, no non-finite result, an element of a column without a stored
                           block exactly 0 (beta = 0) or exactly its start value (beta = 1), every margin unchanged.
"""
import ctypes as C

import numpy as np

from gemm_ld_helpers import C_GAP_INT, GAP_CODE, NAN_CODE, bound64
from helpers import as_float
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG
from sparse_helpers import C_GAP, make_bcsc, pack_vnni2, pack_vnni4

INT8 = (DT.I8, DT.U8)
NP_OF = {DT.F32: np.float32, DT.BF16: np.uint16, DT.I8: np.int8, DT.U8: np.uint8, DT.I32: np.int32}
MARGIN = 4096
ALIGN = 256                       # the placed array starts `skew` bytes behind a multiple of ALIGN


# ---- data ----------------------------------------------------------------------------------------------------------------------------------------------------------
def wide(rng, count, dt):
    """count values of dt (bf16 as uint16, f32): sign * 1.significand * 2^e, the significand's bits all random, e uniform in [-8, 8]; one in eight is +0."""
    assert dt in (DT.BF16, DT.F32)
    ut, sbits = (np.uint16, 7) if dt == DT.BF16 else (np.uint32, 23)                               # storage type, significand bits below the exponent
    r = rng.integers(0, 1 << (sbits + 4), count, dtype=ut)                                         # significand | sign | three bits that decide the zeros
    bits = rng.integers(127 - 8, 127 + 9, count, dtype=ut)
    bits <<= ut(sbits)
    bits |= r & ut((1 << sbits) - 1)
    bits |= (r & ut(1 << sbits)) << ut(8)                                                          # the sign: from above the significand to above the exponent
    bits *= (r >> ut(sbits + 1)) != 0                                                              # the top three bits all clear: one value in eight is +0
    return bits if dt == DT.BF16 else bits.view(np.float32)


def full_bytes(rng, count, dt):
    """Full-range bytes, as test_bcsc_int8 builds them: 0 .. 255 for the unsigned operand, -128 .. 127 for the signed one."""
    return rng.integers(0, 256, count).astype(np.uint8) if dt == DT.U8 else rng.integers(-128, 128, count).astype(np.int8)


def edge_columns(rng, K, N, bk, bn, keep):
    """Block rows of every block column: make_bcsc's random choice with the edges planted.  Three columns or more: column 0 holds every k-block, column 1 none,
    column 2 is stored in descending order and uses the first and the last k-block.  Two columns: every k-block in descending order, then none.  One column: a
    descending column with the first and the last k-block."""
    colptr, rowidx, _ = make_bcsc(rng, K, N, bk, bn, keep, DT.F32)
    nkb, nnb = K // bk, N // bn
    cols = [[int(x) for x in rowidx[colptr[nb]:colptr[nb + 1]]] for nb in range(nnb)]
    if nnb >= 3:
        cols[0], cols[1], cols[2] = list(range(nkb)), [], sorted(set(cols[2]) | {0, nkb - 1}, reverse=True)
    elif nnb == 2:
        cols[0], cols[1] = list(range(nkb - 1, -1, -1)), []
    else:
        cols[0] = sorted(set(cols[0]) | {0, nkb - 1}, reverse=True)
    return cols


def nan_of(dt):
    """What the margins of an input hold: the type's quiet NaN, 0x7f bytes for integers."""
    if dt == DT.F32:
        return np.array(np.nan, dtype=np.float32)
    if dt == DT.BF16:
        return np.array(NAN_CODE[DT.BF16], dtype=np.uint16)
    return np.array(0x7f, dtype=NP_OF[dt])


def gap_of(dt):
    """What the margins of C hold: -7 in C's type, gemm_ld_helpers.C_GAP_INT for int32."""
    if dt == DT.F32:
        return np.array(C_GAP, dtype=np.float32)
    if dt == DT.BF16:
        return np.array(GAP_CODE[DT.BF16], dtype=np.uint16)
    return np.array(C_GAP_INT, dtype=np.int32)


class BcscCase:
    """C[mb][n][i] (+)= sum over the stored blocks of n's block column of A[mb][k][i] * B[k][n].

    cols: the block rows of every block column (None: edge_columns(keep)); nnz0: a pattern without any block.  pattern_on: "device", "host" or "bound" (device
    arrays bound with libxsmm_hip_bcsc_bind_pattern).  hint: the streaming hint of the call.  skew_a / skew_b / skew_c: bytes the operand starts behind a 256-byte
    boundary.  data: "wide" / "zeros" (the caller fills A, bvals and C0 itself and calls repack())."""

    def __init__(self, a_type=DT.BF16, c_type=None, M=64, N=64, K=128, mb=3, bk=32, bn=16, vnni=None, beta=0, cols=None, keep=0.5, nnz0=False, pattern_on="device",
                 hint=0, skew_a=0, skew_b=0, skew_c=0, seed=2025, data="wide"):
        self.ints = a_type in INT8
        self.a_type, self.b_type = a_type, ((DT.I8 if a_type == DT.U8 else DT.U8) if self.ints else a_type)
        self.c_type = c_type if c_type is not None else (DT.I32 if self.ints else a_type)
        self.M, self.N, self.K, self.mb, self.bk, self.bn, self.beta = M, N, K, mb, bk, bn, beta
        self.vnni = (a_type != DT.F32) if vnni is None else vnni
        self.pattern_on, self.hint, self.skew = pattern_on, hint, {"A": skew_a, "B": skew_b, "C": skew_c}
        assert K % bk == 0 and N % bn == 0
        rng = np.random.default_rng(seed)
        if nnz0:
            cols = [[] for _ in range(N // bn)]
        elif cols is None:
            cols = edge_columns(rng, K, N, bk, bn, keep)
        assert len(cols) == N // bn and all(len(set(c)) == len(c) and all(0 <= x < K // bk for x in c) for c in cols), cols
        self.cols = cols
        self.colptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.uint32)
        self.nnzb = int(self.colptr[-1])
        self.rowidx = np.array([x for c in cols for x in c] + ([0] if self.nnzb == 0 else []), dtype=np.uint32)      # (never an empty array: the pointer must not be NULL)
        nb, na, nc = self.nnzb * bn * bk, mb * K * M, mb * N * M
        if data == "zeros":
            self.bvals, self.A, self.C0 = (np.zeros(n, dtype=NP_OF[t]) for n, t in ((nb, self.b_type), (na, a_type), (nc, self.c_type)))
        elif self.ints:
            self.bvals, self.A = full_bytes(rng, nb, self.b_type), full_bytes(rng, na, a_type)
            self.C0 = rng.integers(-1000, 1000, nc).astype(np.int32)
        else:
            self.bvals, self.A, self.C0 = wide(rng, nb, a_type), wide(rng, na, a_type), wide(rng, nc, self.c_type)
        self.repack()

    def repack(self):
        """A as the kernel reads it ([mb][K][M], VNNI-2 / VNNI-4 packed where the case says so); forgets the cached restatement."""
        if not self.vnni:
            self.A_run = self.A
        else:
            self.A_run = (pack_vnni4 if self.ints else pack_vnni2)(self.A, self.mb, self.K, self.M)
        self._ref = None

    def has_block(self):
        """[N] bool: column n's block column stores a block."""
        return np.repeat(np.diff(self.colptr.astype(np.int64)) > 0, self.bn)

    def dense(self):
        """float64 K x N matrix of the pattern (exact for every type here)."""
        d = np.zeros((self.K, self.N))
        bv = as_float(self.bvals, self.b_type).reshape(-1, self.bn, self.bk) if self.nnzb else None
        b = 0
        for nb, col in enumerate(self.cols):
            for kb in col:
                d[kb * self.bk:(kb + 1) * self.bk, nb * self.bn:(nb + 1) * self.bn] = bv[b].T
                b += 1
        return d

    def run_oracle(self, c_type=None, C0=None, colptr=None, rowidx=None, bvals=None, blocks=None):
        """The reference's loop on the case's data (or on the replacements given); blocks: a slice of M-blocks."""
        from oracle import pyoracle
        c_type = self.c_type if c_type is None else c_type
        sl = slice(0, self.mb) if blocks is None else blocks
        nblk = len(range(*sl.indices(self.mb)))
        a = np.ascontiguousarray(self.A_run.reshape(self.mb, -1)[sl]).reshape(-1)
        out = np.ascontiguousarray((self.C0 if C0 is None else C0).reshape(self.mb, -1)[sl]).reshape(-1).copy()
        colptr, rowidx, bvals = (self.colptr if colptr is None else colptr), (self.rowidx if rowidx is None else rowidx), (self.bvals if bvals is None else bvals)
        bvals = bvals if bvals.size else np.zeros(1, dtype=bvals.dtype)
        pyoracle.oracle().lib.oracle_packed_spgemm_bcsc(self.a_type, c_type, self.M, self.N, self.K, nblk, self.bk, self.bn, int(self.vnni), a.ctypes.data, bvals.ctypes.data,
                                                        colptr.ctypes.data, rowidx.ctypes.data, out.ctypes.data, int(self.beta == 0))
        return out


# ---- restatement and bound ------------------------------------------------------------------------------------------------------------------------------------------
def ref64(case):
    """(ref, mag, terms): [mb][N][M] float64 (integers: int64 and mag None), terms [1][N][1]; computed once per case."""
    if case._ref is not None:
        return case._ref
    dT = np.ascontiguousarray(case.dense().T)
    adT = np.abs(dT)
    A = case.A.reshape(case.mb, case.K, case.M)
    ref = np.empty((case.mb, case.N, case.M))
    mag = None if case.ints else np.empty_like(ref)
    for s in range(0, case.mb, 256):                                   # == einsum("bkm,kn->bnm", A, dense), a slab of M-blocks at a time
        a = as_float(A[s:s + 256], case.a_type)
        np.matmul(dT, a, out=ref[s:s + 256])
        if mag is not None:
            np.matmul(adT, np.abs(a), out=mag[s:s + 256])
    terms = (np.diff(case.colptr.astype(np.int64)).repeat(case.bn) * case.bk)[None, :, None]
    if case.beta:
        c0 = as_float(case.C0, case.c_type).reshape(ref.shape)
        ref += c0
        if mag is not None:
            mag += np.abs(c0)
        terms = terms + 1
    if case.ints:                                                      # every partial sum is an integer below 2^53: the float64 product IS the int64 one
        assert np.abs(ref).max(initial=0) < 2.0 ** 52
        ref = ref.astype(np.int64)
    case._ref = (ref, mag, terms)
    return case._ref


def bound_of(case):
    ref, mag, terms = ref64(case)
    return bound64(case, ref, mag, terms)[0]


def assert_bcsc(case, got, margins, stats=None):
    """got: C as the kernel (or the oracle) left it, case.C0's type and size.  margins: {"A" | "B" | "C": (front, back, front as placed, back as placed)} byte arrays.
    stats: receives "ratio" = the worst err / bound."""
    for name, (front, back, want_front, want_back) in margins.items():
        for side, g, w in (("front", front, want_front), ("back", back, want_back)):
            assert np.array_equal(g, w), f"the {side} margin of {name} changed: {np.count_nonzero(g != w)} bytes, the first at {int(np.flatnonzero(g != w)[0])} of {g.size}"
    ref, mag, terms = ref64(case)
    shape = ref.shape
    if case.ints:
        g = got.reshape(shape).astype(np.int64)
        bad = g != ref
        if stats is not None:
            stats["ratio"] = float(bad.any())
        assert not bad.any(), f"{np.count_nonzero(bad)} integer results differ, the first at (mb, n, i) = {tuple(int(x) for x in np.argwhere(bad)[0])}"
        return
    g = as_float(got, case.c_type).reshape(shape)
    assert np.all(np.isfinite(g)), f"{np.count_nonzero(~np.isfinite(g))} non-finite results (a margin was read?), the first at (mb, n, i) = {tuple(int(x) for x in np.argwhere(~np.isfinite(g))[0])}"
    bound = bound64(case, ref, mag, terms)[0]
    ratio = np.abs(g - ref) / bound
    worst = tuple(int(x) for x in np.unravel_index(np.argmax(ratio), shape))
    if stats is not None:
        stats["ratio"] = float(ratio[worst])
    assert ratio[worst] <= 1.0, f"{np.count_nonzero(ratio > 1.0)} elements outside the per-element bound; worst err / bound {float(ratio[worst]):.3f} at (mb, n, i) = {worst}"
    empty = ~case.has_block()
    if empty.any():                                                    # no product at all: exactly 0, or exactly the start value
        raw = got.reshape(shape)[:, empty, :]
        if case.beta:
            want = case.C0.reshape(shape)[:, empty, :]
            same = raw.view(np.uint8).reshape(raw.shape + (-1,)) == want.view(np.uint8).reshape(raw.shape + (-1,))
            bad = ~same.all(axis=-1)
        else:
            bad = g[:, empty, :] != 0
        where = [int(x) for x in np.argwhere(bad)[0]] if bad.any() else None
        assert not bad.any(), (f"{np.count_nonzero(bad)} elements of columns without a stored block are not exactly {'their start value' if case.beta else 'zero'}, "
                               f"the first at (mb, n, i) = ({where[0]}, {int(np.flatnonzero(empty)[where[1]])}, {where[2]})")


# ---- placement -------------------------------------------------------------------------------------------------------------------------------------------------------
def fill_bytes(fill, nbytes, ends_aligned):
    """nbytes of the element `fill` repeated; ends_aligned: the LAST byte is an element's last byte (a front margin), else the first byte an element's first."""
    pat = np.frombuffer(np.asarray(fill).tobytes(), dtype=np.uint8)
    reps = np.tile(pat, nbytes // pat.size + 2)
    return reps[reps.size - nbytes:].copy() if ends_aligned else reps[:nbytes].copy()


def host_margins(arr, skew_bytes=0, margin=MARGIN, fill=0):
    """(front, back) as place() writes them."""
    return fill_bytes(fill, margin + skew_bytes, True), fill_bytes(fill, margin, False)


class Placed:
    """An array inside a larger device buffer: .ptr, read() -> the array, margins() -> (front, back, front as placed, back as placed)."""

    def __init__(self, buf, lead, nbytes, dtype, want_front, want_back):
        self.buf, self.lead, self.nbytes, self.dtype, self.want_front, self.want_back = buf, lead, nbytes, dtype, want_front, want_back
        self.start = lead + want_front.size
        self.ptr = buf.data_ptr() + self.start

    def read(self):
        return self.buf[self.start:self.start + self.nbytes].cpu().numpy().view(self.dtype)

    def margins(self):
        front = self.buf[self.lead:self.start].cpu().numpy()
        back = self.buf[self.start + self.nbytes:self.start + self.nbytes + self.want_back.size].cpu().numpy()
        return front, back, self.want_front, self.want_back


def place(arr, skew_bytes=0, margin=MARGIN, fill=0):
    """arr in a device buffer, `margin + skew_bytes` bytes behind a 256-byte boundary and with `margin` bytes behind it; both margins hold `fill`."""
    import torch
    raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
    front, back = host_margins(arr, skew_bytes, margin, fill)
    buf = torch.empty(ALIGN + front.size + raw.size + back.size, dtype=torch.uint8, device="cuda:0")
    lead = (-buf.data_ptr()) % ALIGN
    image = np.concatenate([front, raw, back])
    buf[lead:lead + image.size].copy_(torch.from_numpy(image))
    placed = Placed(buf, lead, raw.size, arr.dtype, front, back)
    assert placed.ptr % ALIGN == (margin + skew_bytes) % ALIGN
    return placed


def fills(case):
    return {"A": nan_of(case.a_type), "B": nan_of(case.b_type), "C": gap_of(case.c_type)}


def pristine_margins(case, margin=MARGIN):
    """The margins dict of a run that touched none of them (the CPU checks of assert_bcsc)."""
    out = {}
    for name, arr in (("A", case.A_run), ("B", case.bvals), ("C", case.C0)):
        front, back = host_margins(arr, case.skew[name], margin, fills(case)[name])
        out[name] = (front.copy(), back.copy(), front, back)
    return out


# ---- the call --------------------------------------------------------------------------------------------------------------------------------------------------------
def run_gpu(case):
    """One call of the library on the placed operands: (C as it came back, margins for assert_bcsc, kernel name)."""
    import torch
    api = capi.load()
    shape = capi.gemm_shape(case.mb, 0, case.K, case.K, 0, case.N, case.a_type, case.b_type, case.c_type, DT.I32 if case.ints else DT.F32)
    flags = (GEMM_FLAG.BETA_0 if case.beta == 0 else 0) | (GEMM_FLAG.VNNI_A if case.vnni else 0)
    h = api.create_packed_spgemm_bcsc(shape, flags, 0, capi.SpgemmConfig(case.M, case.bk, case.bn))
    assert h, "libxsmm_create_packed_spgemm_bcsc refused the case"
    f = fills(case)
    pa, pb, pc = place(case.A_run, case.skew["A"], fill=f["A"]), place(case.bvals, case.skew["B"], fill=f["B"]), place(case.C0, case.skew["C"], fill=f["C"])
    nblk = C.c_ulonglong(case.N // case.bn)
    p = capi.GemmParam()
    p.a.primary, p.b.primary, p.b.quaternary, p.c.primary = pa.ptr, pb.ptr, C.addressof(nblk), pc.ptr
    try:
        if case.pattern_on == "host":
            p.b.secondary, p.b.tertiary = case.colptr.ctypes.data, case.rowidx.ctypes.data
        else:
            dcp = torch.from_numpy(case.colptr.view(np.int32)).to("cuda:0")
            dri = torch.from_numpy(case.rowidx.view(np.int32)).to("cuda:0")
            p.b.secondary, p.b.tertiary = dcp.data_ptr(), dri.data_ptr()
            if case.pattern_on == "bound":
                assert api.hip_bcsc_bind_pattern(h, dcp.data_ptr(), dri.data_ptr(), case.N // case.bn) == 0
        api.hip_set_streaming_hint(case.hint)
        capi.Api.call(h, p)
        api.hip_sync(); api.check()
        name = api.hip_kernel_name(h, 0).decode()
        got = pc.read()
        margins = {"A": pa.margins(), "B": pb.margins(), "C": pc.margins()}
    finally:
        api.hip_set_streaming_hint(0)
        api.release_kernel(h)
    return got, margins, name
