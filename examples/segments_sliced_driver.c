/* segments_sliced_driver.c -- the weight gradient of a block-sparse layer as ONE libxsmm_hip_gemm_batch_reduce_segments_offsets_sliced call, checked against a
 * plain host loop.  W is RB x CB blocks of BS x BS, about half of them stored; dY and X are dense, PB block columns (the minibatch):
 *   dW(r, c) = sum_p dY(r, p) X(c, p)^T    TRANS_B, one C block per stored block, PB products each
 * The unsliced entry gives every block's chain of PB products to one wave.  Here every chain is cut into slices of SL products: a slice is summed by a wave of
 * its own into the workspace, and a second launch adds a block's partial sums in ascending slice order -- the same bits on every run
 * [ref: src/generator_gemm_reference_impl.c:509-513 for the OFFSET lists].
 *
 *   segments_sliced_driver      exit 0 if dW matches its host loop (normf_rel < 1e-5); 2 without a device
 */
#include <libxsmm.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define BS 16          /* block edge */
#define RB 6           /* block rows of W */
#define CB 5           /* block columns of W */
#define PB 24          /* block columns of X and dY: products per block of dW */
#define SL 4           /* products per slice */
#define BLK ((size_t)BS * BS)
#define BYTES(nblocks) (sizeof(float) * BLK * (size_t)(nblocks))
#define MAXB (RB * CB)
#define MAXS (MAXB * ((PB + SL - 1) / SL))

static float frand(void) { return (float)((int)(libxsmm_rng_f64() * 10.0) - 5) / 10.0f; }   /* multiples of 0.1 */

static void* upload(const void* host, size_t bytes) {
  void* dev = libxsmm_hip_malloc(bytes > 0 ? bytes : 1);
  if (NULL == dev || (bytes > 0 && libxsmm_hip_memcpy_h2d(dev, host, bytes) != 0)) { fprintf(stderr, "device allocation or copy failed\n"); exit(3); }
  return dev;
}

/* element (i, j) of block (br, bc) of a dense matrix stored as column-major blocks, `ncb` blocks per block row */
static double at(const float* x, int ncb, int br, int bc, int i, int j) { return (double)x[BLK * ((size_t)br * ncb + bc) + (size_t)j * BS + i]; }

int main(void) {
  static float x[CB * PB * BS * BS], dy[RB * PB * BS * BS], dw[RB * CB * BS * BS];
  static unsigned long long blk_ptr[MAXB + 1], seg_ptr[MAXS + 1];
  static long long a_offs[MAXB * PB], b_offs[MAXB * PB], c_offs[MAXB];
  int brow[MAXB], bcol[MAXB];
  int nnz = 0, r, c, p, i, j, k, z;
  size_t nslices = 0, nprod = 0, ws_bytes;
  unsigned long long launches;
  double err = 0.0, ref = 0.0, rel;
  void *d_x, *d_dy, *d_dw, *d_blk, *d_seg, *d_a, *d_b, *d_c, *d_ws;
  libxsmm_gemm_param param;
  libxsmm_gemmfunction kernel;
  const libxsmm_gemm_shape shape = libxsmm_create_gemm_shape(BS, BS, BS, BS, BS, BS, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32);
  const libxsmm_gemm_batch_reduce_config brcfg = libxsmm_create_gemm_batch_reduce_config(LIBXSMM_GEMM_BATCH_REDUCE_OFFSET, 0, 0, 0);
  if (libxsmm_hip_device_count() <= 0) { printf("no HIP device\n"); return 2; }
  libxsmm_rng_set_seed(4242);
  for (r = 0; r < RB; ++r) for (c = 0; c < CB; ++c) if (libxsmm_rng_f64() < 0.5) { brow[nnz] = r; bcol[nnz] = c; ++nnz; }
  for (i = 0; i < (int)(BLK * CB * PB); ++i) x[i] = frand();
  for (i = 0; i < (int)(BLK * RB * PB); ++i) dy[i] = frand();
  /* the two-level CSR, from the pattern alone: block z owns the slices blk_ptr[z] .. blk_ptr[z + 1], a slice owns up to SL products */
  blk_ptr[0] = 0; seg_ptr[0] = 0;
  for (z = 0; z < nnz; ++z) {
    for (p = 0; p < PB; ++p) {
      a_offs[nprod] = (long long)BYTES((size_t)brow[z] * PB + p); b_offs[nprod] = (long long)BYTES((size_t)bcol[z] * PB + p); ++nprod;
      if ((p + 1) % SL == 0 || p + 1 == PB) seg_ptr[++nslices] = nprod;
    }
    c_offs[z] = (long long)BYTES(z);
    blk_ptr[z + 1] = nslices;
  }
  kernel = libxsmm_dispatch_brgemm(shape, (libxsmm_bitfield)(LIBXSMM_GEMM_FLAG_BETA_0 | LIBXSMM_GEMM_FLAG_TRANS_B), LIBXSMM_GEMM_PREFETCH_NONE, brcfg);
  if (NULL == kernel) { fprintf(stderr, "dispatch returned NULL\n"); return 3; }
  ws_bytes = libxsmm_hip_gemm_batch_reduce_segments_sliced_workspace(kernel, nslices);     /* the only authority on the size */
  d_ws = libxsmm_hip_malloc(ws_bytes > 0 ? ws_bytes : 16);
  if (NULL == d_ws) { fprintf(stderr, "workspace allocation failed\n"); return 3; }
  d_x = upload(x, BYTES(CB * PB)); d_dy = upload(dy, BYTES(RB * PB)); d_dw = upload(dw, BYTES(nnz));
  d_blk = upload(blk_ptr, sizeof(unsigned long long) * ((size_t)nnz + 1)); d_seg = upload(seg_ptr, sizeof(unsigned long long) * (nslices + 1));
  d_a = upload(a_offs, sizeof(long long) * nprod); d_b = upload(b_offs, sizeof(long long) * nprod); d_c = upload(c_offs, sizeof(long long) * (size_t)nnz);
  memset(&param, 0, sizeof(param));
  param.a.primary = d_dy; param.b.primary = d_x; param.c.primary = d_dw;                  /* the three bases */
  (void)libxsmm_hip_launch_count(1);
  libxsmm_hip_gemm_batch_reduce_segments_offsets_sliced(kernel, &param, (size_t)nnz, (const unsigned long long*)d_blk, nslices, (const unsigned long long*)d_seg,
    (const long long*)d_a, (const long long*)d_b, (const long long*)d_c, d_ws, ws_bytes);
  if (libxsmm_hip_get_last_error() != 0) { fprintf(stderr, "sliced call failed: %s\n", libxsmm_hip_get_last_error_string()); return 1; }
  launches = libxsmm_hip_launch_count(0);
  if (nnz > 0 && libxsmm_hip_memcpy_d2h(dw, d_dw, BYTES(nnz)) != 0) return 3;
  for (z = 0; z < nnz; ++z) for (j = 0; j < BS; ++j) for (i = 0; i < BS; ++i) {            /* dW(r, c) = sum_p dY(r, p) X(c, p)^T */
    double gold = 0.0, got = at(dw, 1, z, 0, i, j);
    for (p = 0; p < PB; ++p) for (k = 0; k < BS; ++k) gold += at(dy, PB, brow[z], p, i, k) * at(x, PB, bcol[z], p, j, k);
    err += (got - gold) * (got - gold); ref += gold * gold;
  }
  rel = sqrt(err / (ref > 0 ? ref : 1));
  printf("block-sparse dW: %d of %d x %d blocks of %d x %d stored, %d products per block cut into slices of %d\n", nnz, RB, CB, BS, BS, PB, SL);
  printf("dW = dY X^T  %d blocks, %zu slices, %zu products, one call, %llu launches (%s), workspace %zu bytes: normf_rel = %.3g\n", nnz, nslices, nprod, launches,
    libxsmm_hip_kernel_name((const void*)kernel, 1), ws_bytes, rel);
  libxsmm_hip_free(d_ws); libxsmm_hip_free(d_x); libxsmm_hip_free(d_dy); libxsmm_hip_free(d_dw);
  libxsmm_hip_free(d_blk); libxsmm_hip_free(d_seg); libxsmm_hip_free(d_a); libxsmm_hip_free(d_b); libxsmm_hip_free(d_c);
  return (rel < 1e-5 && launches == 2) ? 0 : 1;
}
