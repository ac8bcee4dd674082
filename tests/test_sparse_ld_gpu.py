"""GPU parity of the packed / sparse kernels at PADDED leading dimensions (ldb > n, ldc > n, lda > k, ...): the caller hands panels of wider matrices.

Every dense operand is a padded buffer whose gaps (between the logical width and the leading dimension) hold NaN, and C's gaps hold C_GAP: a kernel that
reads a gap shows NaN in its output, one that writes a gap changes C_GAP.  Results are compared with a float64 restatement of the operation on the
logical sub-arrays, element by element (tests/sparse_helpers.py: assert_componentwise), and with the oracle's gold loop at the bounds of
tests/test_sparse_gpu.py.  The shapes are chosen so that padding alone changes the vector width of the kernel that runs, and so that every kernel
family of the packed CSR path is reached (asserted by name; the expected vector width is noted next to each case, the name does not carry it)."""
import ctypes as C

import numpy as np
import pytest

from helpers import normf_rel, rand_values
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG
from oracle import pyoracle
from sparse_helpers import (C_GAP, assert_componentwise, assert_gaps_untouched, csr_to_csc, dense_of_csr, gapped, random_csr,
                            ref_asparse, ref_bsparse)

pytestmark = pytest.mark.gpu
NP = {DT.F32: np.float32, DT.F64: np.float64}
TOL = {DT.F32: 1e-5, DT.F64: 1e-12}


@pytest.fixture(params=[0, 2], ids=["precompiled", "jit"])
def jit_mode(request):
    api = capi.load()
    api.hip_set_jit(request.param)
    yield request.param
    api.hip_set_jit(1)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _host(t, shape, dtype):
    return t.cpu().numpy().view(dtype).reshape(shape)


def _jit_fits(inner_idx, nnz, rows, dt):
    """The generated kernel's envelope (jit.cpp: jit_spmm_create / choose_vec at one element per lane); inner_idx: the X row of every non-zero."""
    touched = len(np.unique(inner_idx))
    return 0 < nnz <= 16384 and rows <= 4096 and touched * (2 if dt == DT.F64 else 1) <= 176


def _call(api, h, a, b, c):
    p = capi.GemmParam()
    p.a.primary, p.b.primary, p.c.primary = a, b, c
    capi.Api.call(h, p)


# ---- packed CSR, A sparse: B [K][ldb][P], C [M][ldc][P] ---------------------------------------------------------------------------------------
ASPARSE = [
    # family, dt, M, N, K, P, density, beta0, ldb, ldc
    # spmm_stream_kernel: pattern + K x slab fit 160 KiB of LDS (one column per lane whatever the padding)
    ("stream", DT.F32, 35, 4, 35, 3, 0.15, 0, 5, 4),
    ("stream", DT.F32, 35, 4, 35, 3, 0.15, 1, 4, 6),
    ("stream", DT.F32, 20, 3, 50, 33, 0.1, 0, 5, 7),
    ("stream", DT.F64, 35, 4, 35, 3, 0.15, 1, 6, 6),
    ("stream", DT.F64, 96, 4, 48, 8, 0.02, 1, 7, 5),               # empty rows: untouched with beta = 0 too
    # spmm_panel_kernel<lds>: ~19.5k non-zeros overflow the stream kernel's LDS; K * VEC <= 256 stages the slice at 64 threads
    ("lds", DT.F32, 320, 4, 64, 3, 0.95, 0, 4, 4),                 # ld_x = ld_y = 12: VEC 4
    ("lds", DT.F32, 320, 4, 64, 3, 0.95, 1, 5, 4),                 # ld_x = 15: VEC 1
    ("lds", DT.F32, 320, 4, 64, 3, 0.95, 0, 6, 6),                 # ld_x = ld_y = 18: VEC 2
    ("lds", DT.F32, 320, 4, 64, 3, 0.95, 1, 4, 5),                 # ld_y = 15: VEC 1
    ("lds", DT.F64, 160, 4, 64, 3, 1.0, 0, 4, 4),                  # ld_x = ld_y = 12: VEC 2
    ("lds", DT.F64, 160, 4, 64, 3, 1.0, 1, 5, 6),                  # ld_x = 15: VEC 1
    # spmm_panel_kernel<direct>: K = 700 fits neither the stream kernel's LDS nor the panel's stage
    ("direct", DT.F32, 16, 4, 700, 3, 0.05, 0, 6, 6),              # VEC 2
    ("direct", DT.F32, 16, 4, 700, 3, 0.05, 1, 5, 4),              # VEC 1
    ("direct", DT.F64, 16, 4, 700, 3, 0.05, 0, 4, 6),              # VEC 2
    # a wide packed axis: the generated kernel chooses its width from ld (choose_vec; jit name _v<width>), the precompiled one streams
    ("wide", DT.F32, 8, 4, 8, 131075, 0.3, 1, 4, 4),               # jit _v4
    ("wide", DT.F32, 8, 4, 8, 131075, 0.3, 0, 6, 4),               # ld_x = 6P = 2 mod 4: jit _v2
    ("wide", DT.F32, 8, 4, 8, 131075, 0.3, 1, 4, 5),               # ld_y = 5P odd: jit _v1
]
FAMILY = {("stream", DT.F32): "spmm_stream_kernel<f32,4x1>", ("stream", DT.F64): "spmm_stream_kernel<f64,4x2>",
          ("wide", DT.F32): "spmm_stream_kernel<f32,4x1>", ("lds", DT.F32): "spmm_panel_kernel<lds>", ("lds", DT.F64): "spmm_panel_kernel<lds>",
          ("direct", DT.F32): "spmm_panel_kernel<direct>", ("direct", DT.F64): "spmm_panel_kernel<direct>"}
WIDE_VEC = {(4, 4): 4, (6, 4): 2, (4, 5): 1}


def _asparse_case(dt, M, N, K, P, density, beta0, ldb, ldc, seed=42):
    rng = np.random.default_rng(seed)
    rowptr, colidx = random_csr(rng, M, K, density)
    vals = rand_values(rng, len(colidx), dt) + NP[dt](0.05)
    B = rand_values(rng, K * N * P, dt).reshape(K, N, P)
    C0 = rand_values(rng, M * N * P, dt).reshape(M, N, P)
    return rowptr, colidx, vals, B, C0, gapped(B, ldb, 1, np.nan), gapped(C0, ldc, 1, C_GAP)


def _check_asparse(got, rowptr, colidx, vals, B, C0, Bp, beta0, ldb, ldc, dt, skip_empty=True):
    M, (K, N, P) = len(rowptr) - 1, B.shape
    assert_gaps_untouched(got, N, 1)
    g = got[:, :N]
    ref, mag, terms, untouched = ref_asparse(rowptr, colidx, vals, B, C0, beta0, skip_empty)
    assert_componentwise(g, ref, mag, terms, NP[dt], untouched, C0)
    orc = gapped(C0, ldc, 1, C_GAP)
    pyoracle.oracle().lib.oracle_packed_spgemm_csr_asparse(dt, M, N, K, P, rowptr.ctypes.data, colidx.ctypes.data, vals.ctypes.data,
                                                           Bp.ctypes.data, ldb, orc.ctypes.data, ldc, beta0)
    assert normf_rel(orc[:, :N], g, dt) <= TOL[dt]


@pytest.mark.parametrize("family,dt,M,N,K,P,density,beta0,ldb,ldc", ASPARSE)
def test_packed_csr_asparse_padded(family, dt, M, N, K, P, density, beta0, ldb, ldc, jit_mode):
    api = capi.load()
    rowptr, colidx, vals, B, C0, Bp, Cp = _asparse_case(dt, M, N, K, P, density, beta0, ldb, ldc)
    h = api.create_packed_spgemm_csr(capi.gemm_shape(M, N, K, 0, ldb, ldc, dt, dt, dt, dt), GEMM_FLAG.BETA_0 if beta0 else 0, 0, P,
                                     rowptr.ctypes.data, colidx.ctypes.data, vals.ctypes.data)
    assert h
    dv, dB, dC = _dev(vals), _dev(Bp), _dev(Cp)
    _call(api, h, dv.data_ptr(), dB.data_ptr(), dC.data_ptr())
    api.hip_sync(); api.check()
    name = api.hip_kernel_name(h, 0).decode()
    if jit_mode == 2 and _jit_fits(colidx, len(colidx), M, dt):
        assert name.startswith("spmm_jit"), name
        if family == "wide":
            assert f"_v{WIDE_VEC[(ldb, ldc)]}_" in name, name
    else:
        assert name == FAMILY[(family, dt)], name
    _check_asparse(_host(dC, Cp.shape, NP[dt]), rowptr, colidx, vals, B, C0, Bp, beta0, ldb, ldc, dt)
    api.release_kernel(h)


# ---- packed CSR / CSC, B sparse: A [M][lda][P], C [M][ldc][P] -------------------------------------------------------------------------------
# (the vector width of the B-sparse form divides P, hence lda * P and ldc * P: padding cannot change it; the cases change P instead)
BSPARSE = [
    # family, dt, M, N, K, P, density, beta0, lda, ldc
    ("stream", DT.F32, 9, 35, 20, 64, 0.2, 0, 21, 35),
    ("stream", DT.F32, 9, 35, 20, 6, 0.2, 1, 20, 37),
    ("stream", DT.F32, 5, 12, 7, 10, 0.5, 0, 9, 13),
    ("stream", DT.F64, 9, 4, 84, 16, 0.1, 1, 85, 7),
    ("stream", DT.F64, 5, 12, 7, 3, 0.5, 0, 8, 12),
    ("lds", DT.F32, 3, 320, 64, 6, 0.95, 1, 67, 323),            # VEC 2
    ("lds", DT.F32, 3, 320, 64, 4, 0.95, 0, 65, 321),            # VEC 4
    ("direct", DT.F64, 4, 6, 700, 2, 0.3, 0, 701, 9),            # VEC 2
]


@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("family,dt,M,N,K,P,density,beta0,lda,ldc", BSPARSE)
def test_packed_bsparse_padded(fmt, family, dt, M, N, K, P, density, beta0, lda, ldc, jit_mode):
    api, orc = capi.load(), pyoracle.oracle()
    rng = np.random.default_rng(7)
    rowptr, colidx = random_csr(rng, K, N, density)
    vals = rand_values(rng, len(colidx), dt) + NP[dt](0.05)
    A = rand_values(rng, M * K * P, dt).reshape(M, K, P)
    C0 = rand_values(rng, M * N * P, dt).reshape(M, N, P)
    Ap, Cp = gapped(A, lda, 1, np.nan), gapped(C0, ldc, 1, C_GAP)
    shape = capi.gemm_shape(M, N, K, lda, 0, ldc, dt, dt, dt, dt)
    flags = GEMM_FLAG.BETA_0 if beta0 else 0
    orc_c = Cp.copy()
    if fmt == "csr":
        h = api.create_packed_spgemm_csr(shape, flags, 0, P, rowptr.ctypes.data, colidx.ctypes.data, vals.ctypes.data)
        run_vals = vals
        orc.lib.oracle_packed_spgemm_csr_bsparse(dt, M, N, K, P, rowptr.ctypes.data, colidx.ctypes.data, vals.ctypes.data, Ap.ctypes.data, lda, orc_c.ctypes.data, ldc, beta0)
    else:
        colptr, rowidx, run_vals = csr_to_csc(rowptr, colidx, vals, K, N)
        h = api.create_packed_spgemm_csc(shape, flags, 0, P, colptr.ctypes.data, rowidx.ctypes.data, run_vals.ctypes.data)
        orc.lib.oracle_packed_spgemm_csc_bsparse(dt, M, N, K, P, colptr.ctypes.data, rowidx.ctypes.data, run_vals.ctypes.data, Ap.ctypes.data, lda, orc_c.ctypes.data, ldc, beta0)
    assert h
    dv, dA, dC = _dev(run_vals), _dev(Ap), _dev(Cp)
    _call(api, h, dA.data_ptr(), dv.data_ptr(), dC.data_ptr())
    api.hip_sync(); api.check()
    name = api.hip_kernel_name(h, 0).decode()
    k_of = np.repeat(np.arange(K), np.diff(rowptr))                  # B sparse: the X rows are the k of the non-zeros
    if jit_mode == 2 and _jit_fits(k_of, len(colidx), N, dt):
        assert name.startswith("spmm_jit"), name
    else:
        assert name == FAMILY[(family, dt)], name
    got = _host(dC, Cp.shape, NP[dt])
    assert_gaps_untouched(got, N, 1)
    ref, mag, terms, untouched = ref_bsparse(dense_of_csr(rowptr, colidx, vals, K, N), A, C0, beta0)
    assert_componentwise(got[:, :N], ref, mag, terms, NP[dt], untouched, C0)
    assert normf_rel(orc_c[:, :N], got[:, :N], dt) <= TOL[dt]
    api.release_kernel(h)


# ---- packed CSC, C sparse (f32 only): A [K][lda][P], B [K][ldb][P] ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,P,density,beta0,lda,ldb", [(9, 9, 9, 16, 0.3, 1, 10, 9), (9, 9, 9, 16, 0.3, 0, 9, 12), (20, 9, 7, 64, 0.5, 1, 23, 11),
                                                          (12, 7, 3, 10, 0.4, 0, 13, 8), (35, 35, 4, 33, 0.1, 1, 40, 36)])
def test_packed_csc_csparse_padded(M, N, K, P, density, beta0, lda, ldb):
    api = capi.load()
    rng = np.random.default_rng(19)
    colptr, rowidx = random_csr(rng, N, M, density)                 # C's pattern by columns n, rows m
    nnz = int(colptr[-1])
    A = rand_values(rng, K * M * P, DT.F32).reshape(K, M, P)
    B = rand_values(rng, K * N * P, DT.F32).reshape(K, N, P)
    C0 = rand_values(rng, nnz, DT.F32)
    Ap, Bp = gapped(A, lda, 1, np.nan), gapped(B, ldb, 1, np.nan)
    h = api.create_packed_spgemm_csc(capi.gemm_shape(M, N, K, lda, ldb, 0, DT.F32, DT.F32, DT.F32, DT.F32), GEMM_FLAG.BETA_0 if beta0 else 0, 0, P,
                                     colptr.ctypes.data, rowidx.ctypes.data, C0.ctypes.data)
    assert h and api.hip_kernel_name(h, 0).decode() == "csparse_kernel"
    dA, dB, dC = _dev(Ap), _dev(Bp), _dev(C0)
    _call(api, h, dA.data_ptr(), dB.data_ptr(), dC.data_ptr())
    api.hip_sync(); api.check()
    got = dC.cpu().numpy()
    cols = np.repeat(np.arange(N), np.diff(colptr))
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    ref = np.einsum("kzp,kzp->z", A64[:, rowidx], B64[:, cols])
    mag = np.einsum("kzp,kzp->z", np.abs(A64[:, rowidx]), np.abs(B64[:, cols]))
    if not beta0:
        ref, mag = ref + C0, mag + np.abs(C0.astype(np.float64))
    assert_componentwise(got, ref, mag, K * P, np.float32)
    orc = C0.copy()
    pyoracle.oracle().lib.oracle_packed_spgemm_csc_csparse(N, K, P, colptr.ctypes.data, rowidx.ctypes.data, Ap.ctypes.data, lda, Bp.ctypes.data, ldb, orc.ctypes.data, beta0)
    assert normf_rel(orc, got, DT.F32) <= 1e-5
    api.release_kernel(h)


# ---- dense packed GEMMs ------------------------------------------------------------------------------------------------------------------
def pgemm_case(kind, rng, dt, M, N, K, P, lda, ldb, ldc):
    """Logical operands, padded buffers, the float64 result / magnitude (without C0) and the padded axis of C.
    packed: A [K][lda][P], B [N][ldb][P], C [N][ldc][P] (column-major, P innermost); ac_rm: A [M][lda][P], B [K][ldb] row-major, C [M][ldc][P];
    bc_rm: A [M][lda] row-major, B [K][ldb][P], C [M][ldc][P]."""
    shapes = {"packed": ((K, M, P), (N, K, P), (N, M, P)), "ac_rm": ((M, K, P), (K, N), (M, N, P)), "bc_rm": ((M, K), (K, N, P), (M, N, P))}[kind]
    A, B, C0 = (rand_values(rng, int(np.prod(s)), dt).reshape(s) for s in shapes)
    Ap, Bp, Cp = gapped(A, lda, 1, np.nan), gapped(B, ldb, 1, np.nan), gapped(C0, ldc, 1, C_GAP)
    eq = {"packed": "kmp,nkp->nmp", "ac_rm": "mkp,kn->mnp", "bc_rm": "mk,knp->mnp"}[kind]
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    return A, B, C0, Ap, Bp, Cp, np.einsum(eq, A64, B64), np.einsum(eq, np.abs(A64), np.abs(B64))


PGEMM = [
    # kind, M, N, K, P, beta0, lda, ldb, ldc
    ("packed", 9, 9, 9, 64, 0, 11, 10, 12), ("packed", 4, 7, 5, 24, 1, 4, 6, 5), ("packed", 3, 2, 4, 7, 0, 5, 4, 3), ("packed", 20, 9, 20, 16, 1, 21, 23, 22),
    ("ac_rm", 9, 9, 9, 64, 0, 10, 9, 11), ("ac_rm", 4, 7, 5, 24, 1, 5, 9, 7), ("ac_rm", 20, 9, 20, 6, 1, 23, 12, 10),
    ("bc_rm", 9, 9, 9, 64, 0, 9, 10, 11), ("bc_rm", 4, 7, 5, 24, 1, 8, 7, 9), ("bc_rm", 3, 2, 4, 3, 0, 7, 5, 4),
]


@pytest.mark.parametrize("dt", [DT.F32, DT.F64])
@pytest.mark.parametrize("kind,M,N,K,P,beta0,lda,ldb,ldc", PGEMM)
def test_packed_gemm_padded(kind, dt, M, N, K, P, beta0, lda, ldb, ldc, jit_mode):
    api = capi.load()
    rng = np.random.default_rng(23)
    A, B, C0, Ap, Bp, Cp, ref, mag = pgemm_case(kind, rng, dt, M, N, K, P, lda, ldb, ldc)
    fn = {"packed": api.create_packed_gemm, "ac_rm": api.create_packed_gemm_ac_rm, "bc_rm": api.create_packed_gemm_bc_rm}[kind]
    h = fn(capi.gemm_shape(M, N, K, lda, ldb, ldc, dt, dt, dt, dt), GEMM_FLAG.BETA_0 if beta0 else 0, 0, P)
    assert h
    dA, dB, dC = _dev(Ap), _dev(Bp), _dev(Cp)
    _call(api, h, dA.data_ptr(), dB.data_ptr(), dC.data_ptr())
    api.hip_sync(); api.check()
    got = _host(dC, Cp.shape, NP[dt])
    n_c = C0.shape[1]
    assert_gaps_untouched(got, n_c, 1)
    if not beta0:
        ref, mag = ref + C0, mag + np.abs(C0.astype(np.float64))
    assert_componentwise(got[:, :n_c], ref, mag, K, NP[dt])
    orc = Cp.copy()
    ofn = {"packed": pyoracle.oracle().lib.oracle_packed_gemm, "ac_rm": pyoracle.oracle().lib.oracle_packed_gemm_ac_rm,
           "bc_rm": pyoracle.oracle().lib.oracle_packed_gemm_bc_rm}[kind]
    ofn(dt, M, N, K, P, Ap.ctypes.data, lda, Bp.ctypes.data, ldb, orc.ctypes.data, ldc, beta0)
    assert normf_rel(orc[:, :n_c], got[:, :n_c], dt) <= TOL[dt]
    api.release_kernel(h)


# ---- FsSpMDM and libxsmm_create_spgemm_csr_areg on device operands: B [K][ldb], C [M][ldc] row-major --------------------------------------
@pytest.mark.parametrize("dt", [DT.F32, DT.F64])
@pytest.mark.parametrize("M,N,K,density,beta,lda,ldb,ldc", [(35, 64, 35, 0.15, 0.0, 37, 65, 64), (35, 64, 35, 0.15, 1.0, 35, 64, 66),
                                                           (28, 48, 49, 0.14, 1.0, 50, 51, 53), (192, 96, 96, 0.03, 0.0, 100, 98, 97)])
def test_fsspmdm_padded(dt, M, N, K, density, beta, lda, ldb, ldc, jit_mode):
    api = capi.load()
    rng = np.random.default_rng(3)
    rowptr, colidx = random_csr(rng, M, K, density)
    vals = rand_values(rng, len(colidx), dt) + NP[dt](0.05)
    a_dense = gapped(dense_of_csr(rowptr, colidx, vals, M, K).astype(NP[dt]), lda, 1, np.nan)      # a gap read at creation would become a NaN value
    alpha = NP[dt](1.5)
    B = rand_values(rng, K * N, dt).reshape(K, N)
    C0 = rand_values(rng, M * N, dt).reshape(M, N)
    Bp, Cp = gapped(B, ldb, 1, np.nan), gapped(C0, ldc, 1, C_GAP)
    ct = C.c_double if dt == DT.F64 else C.c_float
    cal, cbe = ct(float(alpha)), ct(beta)
    h = api.fsspmdm_create(dt, M, N, K, lda, ldb, ldc, C.addressof(cal), C.addressof(cbe), a_dense.ctypes.data, 0, None)
    assert h
    dB, dC = _dev(Bp), _dev(Cp)
    api.fsspmdm_execute(h, dB.data_ptr(), dC.data_ptr())
    api.hip_sync(); api.check()
    got = _host(dC, Cp.shape, NP[dt])
    api.fsspmdm_destroy(h)
    sv = (alpha * vals).astype(NP[dt])                                  # the handle's values: alpha folded in, rounded to the element type
    beta0 = int(beta == 0.0)
    _check_rowmajor(got, rowptr, colidx, sv, B, C0, Bp, beta0, ldb, ldc, dt)


def _check_rowmajor(got, rowptr, colidx, vals, B, C0, Bp, beta0, ldb, ldc, dt):
    M, (K, N) = len(rowptr) - 1, B.shape
    assert_gaps_untouched(got, N, 1)
    ref, mag, terms, untouched = ref_asparse(rowptr, colidx, vals, B[:, :, None], C0[:, :, None], beta0, skip_empty=False)
    assert_componentwise(got[:, :N], ref[:, :, 0], mag[:, :, 0], terms[:, :, 0], NP[dt], untouched[:, :, 0], C0)
    orc = gapped(C0, ldc, 1, C_GAP)
    pyoracle.oracle().lib.oracle_fsspmdm(dt, M, N, K, rowptr.ctypes.data, colidx.ctypes.data, vals.ctypes.data, Bp.ctypes.data, ldb, orc.ctypes.data, ldc, beta0)
    assert normf_rel(orc[:, :N], got[:, :N], dt) <= TOL[dt]


@pytest.mark.parametrize("dt", [DT.F32, DT.F64])
@pytest.mark.parametrize("M,N,K,density,beta0,ldb,ldc", [(35, 40, 35, 0.15, 1, 41, 40), (35, 40, 35, 0.15, 0, 40, 43), (64, 12, 49, 0.1, 0, 14, 14),
                                                        (16, 30, 700, 0.05, 1, 33, 31), (96, 8, 48, 0.02, 1, 9, 10)])
def test_spgemm_csr_areg_padded(dt, M, N, K, density, beta0, ldb, ldc, jit_mode):
    """K = 700: spmm_panel_kernel<direct>; the others stream (or run generated in jit mode).  Empty rows are zeroed with beta = 0 (not skipped)."""
    api = capi.load()
    rng = np.random.default_rng(13)
    rowptr, colidx = random_csr(rng, M, K, density)
    vals64 = rng.standard_normal(len(colidx)) + 0.05
    vals = vals64.astype(NP[dt])
    B = rand_values(rng, K * N, dt).reshape(K, N)
    C0 = rand_values(rng, M * N, dt).reshape(M, N)
    Bp, Cp = gapped(B, ldb, 1, np.nan), gapped(C0, ldc, 1, C_GAP)
    h = api.create_spgemm_csr_areg(capi.gemm_shape(M, N, K, 0, ldb, ldc, dt, dt, dt, dt), GEMM_FLAG.BETA_0 if beta0 else 0, 0, N,
                                   rowptr.ctypes.data, colidx.ctypes.data, vals64.ctypes.data)
    assert h
    dB, dC = _dev(Bp), _dev(Cp)
    _call(api, h, None, dB.data_ptr(), dC.data_ptr())
    api.hip_sync(); api.check()
    name = api.hip_kernel_name(h, 0).decode()
    if jit_mode == 2 and _jit_fits(colidx, len(colidx), M, dt):
        assert name.startswith("spmm_jit"), name
    else:
        assert name == ("spmm_panel_kernel<direct>" if K == 700 else f"spmm_stream_kernel<{'f64,4x2' if dt == DT.F64 else 'f32,4x1'}>"), name
    _check_rowmajor(_host(dC, Cp.shape, NP[dt]), rowptr, colidx, vals, B, C0, Bp, beta0, ldb, ldc, dt)
    api.release_kernel(h)


# ---- batched launches at padded leading dimensions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,dt,M,N,K,P,count,lda_or_ldb,ldc,extra", [
    ("a", DT.F32, 35, 4, 35, 3, 5, 5, 6, 0),
    ("a", DT.F64, 20, 3, 50, 33, 4, 4, 5, 0),
    ("a", DT.F32, 35, 4, 35, 3, 3, 6, 6, 1),            # element stride = natural + 1 element
    ("a", DT.F32, 8, 4, 8, 131075, 2, 8, 8, 0),         # jit _v4 for the batch (ld_x = ld_y = 8P)
    ("a", DT.F32, 8, 4, 8, 131075, 2, 8, 8, 1),         # ... a stride of 8KNP + 1 floats is not a multiple of 4: the precompiled kernel runs
    ("b", DT.F32, 9, 35, 20, 64, 6, 22, 36, 0),
    ("b", DT.F64, 5, 12, 7, 10, 3, 9, 13, 1),
    ("b", DT.F32, 64, 6, 8, 8192, 2, 9, 7, 0),          # jit _v4 (P / 4 * M / 64 = 2048 waves)
    ("b", DT.F32, 64, 6, 8, 8192, 2, 9, 7, 1),          # odd stride: precompiled
])
def test_packed_sparse_batched_padded(side, dt, M, N, K, P, count, lda_or_ldb, ldc, extra, jit_mode):
    """libxsmm_hip_gemm_batch_strided: element e of the batch is bit-identical to a single call on element e (beta = 0 when the batch and the
    single calls may run different kernels, whose beta = 1 sums round differently), and matches the float64 restatement."""
    api = capi.load()
    rng = np.random.default_rng(11)
    es = np.dtype(NP[dt]).itemsize
    beta0 = extra
    if side == "a":
        rowptr, colidx = random_csr(rng, M, K, 0.15)
        xshape, ld = (K, N, P), (0, lda_or_ldb, ldc)
    else:
        rowptr, colidx = random_csr(rng, K, N, 0.2)
        xshape, ld = (M, K, P), (lda_or_ldb, 0, ldc)
    vals = rand_values(rng, len(colidx), dt) + NP[dt](0.05)
    X = [rand_values(rng, int(np.prod(xshape)), dt).reshape(xshape) for _ in range(count)]
    C0 = [rand_values(rng, M * N * P, dt).reshape(M, N, P) for _ in range(count)]
    Xp = [gapped(x, lda_or_ldb, 1, np.nan) for x in X]
    Cp = [gapped(c, ldc, 1, C_GAP) for c in C0]
    sx_el, sc_el = Xp[0].size + extra, Cp[0].size + extra                   # element strides (elements); the extra element is a gap too
    Xb = np.full(count * sx_el, np.nan, dtype=NP[dt]); Cb = np.full(count * sc_el, C_GAP, dtype=NP[dt])
    for e in range(count):
        Xb[e * sx_el:e * sx_el + Xp[e].size] = Xp[e].ravel(); Cb[e * sc_el:e * sc_el + Cp[e].size] = Cp[e].ravel()
    h = api.create_packed_spgemm_csr(capi.gemm_shape(M, N, K, ld[0], ld[1], ld[2], dt, dt, dt, dt), GEMM_FLAG.BETA_0 if beta0 else 0, 0, P,
                                     rowptr.ctypes.data, colidx.ctypes.data, vals.ctypes.data)
    assert h
    dv, dX, dC, dL = _dev(vals), _dev(Xb), _dev(Cb), _dev(Cb)
    p = capi.GemmParam()
    if side == "a":
        p.a.primary, p.b.primary, p.c.primary = dv.data_ptr(), dX.data_ptr(), dC.data_ptr()
        api.hip_gemm_batch_strided(h, C.byref(p), count, 0, sx_el * es, sc_el * es)
    else:
        p.a.primary, p.b.primary, p.c.primary = dX.data_ptr(), dv.data_ptr(), dC.data_ptr()
        api.hip_gemm_batch_strided(h, C.byref(p), count, sx_el * es, 0, sc_el * es)
    api.hip_sync(); api.check()
    batched_name = api.hip_kernel_name(h, 1).decode()
    inner_idx = colidx if side == "a" else np.repeat(np.arange(K), np.diff(rowptr))
    jit_fits = jit_mode == 2 and _jit_fits(inner_idx, len(colidx), M if side == "a" else N, dt)
    if jit_fits and P in (131075, 8192):                 # the generated kernel is 4 wide: an odd stride refuses it
        assert batched_name.startswith("spmm_jit") != bool(extra), batched_name
        if not extra:
            assert "_v4_" in batched_name, batched_name
    for e in range(count):                          # the loop the batched call replaces
        if side == "a":
            _call(api, h, dv.data_ptr(), dX.data_ptr() + e * sx_el * es, dL.data_ptr() + e * sc_el * es)
        else:
            _call(api, h, dX.data_ptr() + e * sx_el * es, dv.data_ptr(), dL.data_ptr() + e * sc_el * es)
    api.hip_sync(); api.check()
    got, loop = dC.cpu().numpy().view(NP[dt]), dL.cpu().numpy().view(NP[dt])
    assert np.array_equal(got.view(np.uint8), loop.view(np.uint8))
    Bs = dense_of_csr(rowptr, colidx, vals, K, N) if side == "b" else None
    for e in range(count):
        ge = got[e * sc_el:e * sc_el + Cp[e].size].reshape(Cp[e].shape)
        assert_gaps_untouched(ge, N, 1)
        if extra:
            assert got[e * sc_el + Cp[e].size] == NP[dt](C_GAP)
        if side == "a":
            ref, mag, terms, untouched = ref_asparse(rowptr, colidx, vals, X[e], C0[e], beta0)
        else:
            ref, mag, terms, untouched = ref_bsparse(Bs, X[e], C0[e], beta0)
        assert_componentwise(ge[:, :N], ref, mag, terms, NP[dt], untouched, C0[e])
    api.release_kernel(h)


# ---- synchronous calls on plain host memory: only the touched bytes of each row / slab are staged ---------------------------------------------
@pytest.mark.parametrize("dt", [DT.F32, DT.F64])
@pytest.mark.parametrize("kind,M,N,K,P,ld_x,ldc", [("asparse", 9, 12, 20, 8, 13, 15), ("asparse", 35, 4, 35, 3, 5, 6),
                                                   ("bsparse", 9, 12, 20, 8, 23, 14), ("bsparse", 5, 12, 7, 10, 9, 12)])
def test_packed_sparse_host_operands_padded(kind, dt, M, N, K, P, ld_x, ldc, jit_mode):
    api = capi.load()
    rng = np.random.default_rng(21)
    beta0 = 0
    if kind == "asparse":
        rowptr, colidx = random_csr(rng, M, K, 0.2)
        X, ld = rand_values(rng, K * N * P, dt).reshape(K, N, P), (0, ld_x, ldc)
    else:
        rowptr, colidx = random_csr(rng, K, N, 0.2)
        X, ld = rand_values(rng, M * K * P, dt).reshape(M, K, P), (ld_x, 0, ldc)
    vals = rand_values(rng, len(colidx), dt) + NP[dt](0.05)
    C0 = rand_values(rng, M * N * P, dt).reshape(M, N, P)
    Xp, got = gapped(X, ld_x, 1, np.nan), gapped(C0, ldc, 1, C_GAP)
    h = api.create_packed_spgemm_csr(capi.gemm_shape(M, N, K, ld[0], ld[1], ld[2], dt, dt, dt, dt), 0, 0, P, rowptr.ctypes.data, colidx.ctypes.data, vals.ctypes.data)
    assert h
    if kind == "asparse":
        _call(api, h, vals.ctypes.data, Xp.ctypes.data, got.ctypes.data)
    else:
        _call(api, h, Xp.ctypes.data, vals.ctypes.data, got.ctypes.data)
    api.check()
    assert_gaps_untouched(got, N, 1)
    if kind == "asparse":
        ref, mag, terms, untouched = ref_asparse(rowptr, colidx, vals, X, C0, beta0)
    else:
        ref, mag, terms, untouched = ref_bsparse(dense_of_csr(rowptr, colidx, vals, K, N), X, C0, beta0)
    assert_componentwise(got[:, :N], ref, mag, terms, NP[dt], untouched, C0)
    api.release_kernel(h)


@pytest.mark.parametrize("dt", [DT.F32, DT.F64])
@pytest.mark.parametrize("kind,M,N,K,P,lda,ldb,ldc", [("ac_rm", 9, 9, 9, 16, 11, 12, 10), ("ac_rm", 4, 7, 5, 6, 5, 9, 7),
                                                      ("bc_rm", 9, 9, 9, 16, 12, 10, 11), ("bc_rm", 4, 7, 5, 6, 8, 7, 9)])
def test_row_major_packed_gemm_host_operands_padded(kind, dt, M, N, K, P, lda, ldb, ldc, jit_mode):
    """The row-major operand of _ac_rm / _bc_rm is the kernel's value array, read at k * ldb + n / m * lda + k: a synchronous call on host memory
    must stage it up to its last element read, not just K * N / M * K of it."""
    api = capi.load()
    rng = np.random.default_rng(29)
    A, B, C0, Ap, Bp, got, ref, mag = pgemm_case(kind, rng, dt, M, N, K, P, lda, ldb, ldc)
    fn = api.create_packed_gemm_ac_rm if kind == "ac_rm" else api.create_packed_gemm_bc_rm
    h = fn(capi.gemm_shape(M, N, K, lda, ldb, ldc, dt, dt, dt, dt), 0, 0, P)
    assert h
    _call(api, h, Ap.ctypes.data, Bp.ctypes.data, got.ctypes.data)
    api.check()
    assert_gaps_untouched(got, N, 1)
    assert_componentwise(got[:, :N], ref + C0, mag + np.abs(C0.astype(np.float64)), K, NP[dt])
    api.release_kernel(h)
