"""Sparse test inputs: random CSR patterns, CSR->CSC, BCSC block patterns (samples/xgemm_sparse/
spmm_kernel.c:219-375 layouts), VNNI-2 packing of per-block A, and a Matrix-Market reader for the
fixture patterns under tests/golden/."""
import numpy as np

from helpers import rand_values
from libxsmm_amd.capi import DT


def random_csr(rng, rows, cols, density):
    nnz_target = max(1, int(round(rows * cols * density)))
    flat = np.sort(rng.choice(rows * cols, size=nnz_target, replace=False))
    r, c = flat // cols, flat % cols
    rowptr = np.zeros(rows + 1, dtype=np.uint32)
    np.add.at(rowptr, r + 1, 1)
    rowptr = np.cumsum(rowptr).astype(np.uint32)
    return rowptr, c.astype(np.uint32)


def csr_to_csc(rowptr, colidx, vals, rows, cols):
    order = np.lexsort((np.repeat(np.arange(rows), np.diff(rowptr)), colidx))
    r_of = np.repeat(np.arange(rows), np.diff(rowptr))
    colptr = np.zeros(cols + 1, dtype=np.uint32)
    np.add.at(colptr, colidx + 1, 1)
    colptr = np.cumsum(colptr).astype(np.uint32)
    return colptr, r_of[order].astype(np.uint32), vals[order].copy()


def make_bcsc(rng, K, N, bk, bn, keep, dtype):
    """Block-sparse K x N matrix in BCSC: vals[blk][dn][dk] (k fastest), colptr over N/bn, rowidx = k-block."""
    nkb, nnb = K // bk, N // bn
    colptr = [0]
    rowidx = []
    for nb in range(nnb):
        kept = np.sort(rng.choice(nkb, size=max(1, int(round(nkb * keep))), replace=False)) if keep < 1.0 else np.arange(nkb)
        rowidx += list(kept)
        colptr.append(len(rowidx))
    vals = rand_values(rng, len(rowidx) * bn * bk, dtype)
    return np.array(colptr, dtype=np.uint32), np.array(rowidx, dtype=np.uint32), vals


def structured_2_of_8(K, N, bk, bn):
    """BASELINE config #4 pattern: 2 of every 8 K-blocks per N-block are non-zero."""
    nkb, nnb = K // bk, N // bn
    colptr, rowidx = [0], []
    for nb in range(nnb):
        for g in range(0, nkb, 8):
            grp = [g + (nb % 8), g + ((nb + 3) % 8)]
            rowidx += sorted(x for x in set(grp) if x < nkb)
        colptr.append(len(rowidx))
    return np.array(colptr, dtype=np.uint32), np.array(rowidx, dtype=np.uint32)


def pack_vnni2(A, mb, K, M):
    """[mb][K][M] (M fastest) -> [mb][K/2][M][2]."""
    a = A.reshape(mb, K // 2, 2, M)
    return np.ascontiguousarray(a.transpose(0, 1, 3, 2)).reshape(-1)


def pack_vnni4(A, mb, K, M):
    """[mb][K][M] (M fastest) -> [mb][K/4][M][4] (8-bit operands, [ref: samples/xgemm_sparse/spmm_kernel.c:254-262])."""
    a = A.reshape(mb, K // 4, 4, M)
    return np.ascontiguousarray(a.transpose(0, 1, 3, 2)).reshape(-1)


def read_mtx(path):
    """Matrix-Market coordinate file -> dense float64 array (fixtures: sparsity patterns + values)."""
    with open(path) as f:
        lines = [ln for ln in f if not ln.startswith("%")]
    rows, cols, nnz = (int(x) for x in lines[0].split()[:3])
    dense = np.zeros((rows, cols))
    for ln in lines[1:1 + nnz]:
        parts = ln.split()
        dense[int(parts[0]) - 1, int(parts[1]) - 1] = float(parts[2]) if len(parts) > 2 else 1.0
    return dense


# ---- padded leading dimensions: poisoned gaps and a float64 restatement -------------------------------------------------------------------------
# Dense operands are built with their leading axis widened to ld.  Input gaps hold NaN, so a kernel that reads one shows NaN in its output; C gaps
# hold C_GAP, a finite pattern that must come back bit for bit.
C_GAP = -7.0


def gapped(x, ld, axis, fill):
    """x with `axis` widened to ld; the added elements hold `fill`."""
    shape = list(x.shape)
    shape[axis] = ld
    buf = np.full(shape, fill, dtype=x.dtype)
    buf[logical_slice(x.ndim, axis, x.shape[axis])] = x
    return buf


def logical_slice(ndim, axis, width):
    sl = [slice(None)] * ndim
    sl[axis] = slice(0, width)
    return tuple(sl)


def gap_slice(ndim, axis, width):
    sl = [slice(None)] * ndim
    sl[axis] = slice(width, None)
    return tuple(sl)


def assert_gaps_untouched(got, width, axis, fill=C_GAP):
    """The elements between the logical width and the leading dimension are bit-identical to `fill`."""
    gap = got[gap_slice(got.ndim, axis, width)]
    want = np.full(gap.shape, fill, dtype=got.dtype)
    assert np.array_equal(gap.view(np.uint8), want.view(np.uint8)), f"{np.count_nonzero(gap != want)} gap elements of C were written"


def dense_of_csr(rowptr, colidx, vals, rows, cols):
    """float64 rows x cols matrix of a CSR pattern (no duplicate entries)."""
    a = np.zeros((rows, cols))
    a[np.repeat(np.arange(rows), np.diff(rowptr)), colidx] = np.asarray(vals, dtype=np.float64)
    return a


def assert_componentwise(got, ref, mag, terms, dt_np, untouched=None, c0=None):
    """|got - ref| <= (terms + 2) * u * mag elementwise, u the unit round-off of dt_np; mag = sum |a| |x| (+ |C0| when beta = 1).
    `untouched`: boolean mask (broadcast against got) of elements that must be bit-identical to c0."""
    u = np.finfo(dt_np).eps / 2
    g = got.astype(np.float64)
    assert np.all(np.isfinite(g)), f"{np.count_nonzero(~np.isfinite(g))} non-finite results (a gap was read?)"
    bound = (np.asarray(terms, dtype=np.float64) + 2) * u * mag
    err = np.abs(g - ref)
    bad = err > bound
    assert not bad.any(), f"{np.count_nonzero(bad)} elements outside the componentwise bound; worst excess {float(np.max(err - bound)):.3e}"
    if untouched is not None:
        mask = np.broadcast_to(untouched, got.shape)
        assert np.array_equal(got[mask].view(np.uint8), c0[mask].view(np.uint8)), "rows the operation leaves untouched were written"


def ref_asparse(rowptr, colidx, vals, B, C0, beta0, skip_empty=True):
    """A sparse (M x K, CSR) times packed B [K][N][P] -> C [M][N][P] in float64: (ref, mag, terms, untouched rows).
    Empty rows are left untouched when skip_empty (packed CSR) or beta = 1 (every form)."""
    M, (K, N, P) = len(rowptr) - 1, B.shape
    A = dense_of_csr(rowptr, colidx, vals, M, K)
    B64 = B.astype(np.float64).reshape(K, N * P)
    ref, mag = (A @ B64).reshape(M, N, P), (np.abs(A) @ np.abs(B64)).reshape(M, N, P)
    if not beta0:
        ref, mag = ref + C0, mag + np.abs(C0.astype(np.float64))
    nnz = np.diff(rowptr).astype(np.int64)
    untouched = (nnz == 0) & (bool(skip_empty) or not beta0)
    ref[untouched], mag[untouched] = C0[untouched], 0
    return ref, mag, nnz[:, None, None], untouched[:, None, None]


def ref_bsparse(Bs, A, C0, beta0):
    """packed A [M][K][P] times dense-ified sparse B (K x N, float64) -> C [M][N][P]: (ref, mag, terms, untouched columns).
    An empty column n is written as zeros with beta = 0 and left untouched with beta = 1."""
    A64 = A.astype(np.float64)
    ref, mag = np.einsum("mkp,kn->mnp", A64, Bs), np.einsum("mkp,kn->mnp", np.abs(A64), np.abs(Bs))
    if not beta0:
        ref, mag = ref + C0, mag + np.abs(C0.astype(np.float64))
    nnz = np.count_nonzero(Bs, axis=0)
    untouched = (nnz == 0) & (not beta0)
    ref[:, untouched], mag[:, untouched] = C0[:, untouched], 0
    return ref, mag, nnz[None, :, None], untouched[None, :, None]
