/* segments_backward_driver.c -- a block-sparse layer forward AND backward, one libxsmm_hip_gemm_batch_reduce_segments_offsets call per pass, checked against
 * plain host loops.  W is RB x CB blocks of BS x BS in BSR form (row pointer, block columns, values block row by block row); X and dY are dense, PB block columns:
 *   Y  = W   X      NN        segment (r, p): the blocks of block row r,    A = W(r, c),  B = X(c, p)
 *   dX = W^T dY     TRANS_A   segment (c, p): the blocks of block column c, A = W(r, c) read transposed -- the SAME value buffer, lists in block-column order
 *   dW = dY  X^T    TRANS_B   segment z = (r, c), PB products,              A = dY(r, p), B = X(c, p) read transposed, C = the gradient's BSR values
 * The lists hold byte OFFSETS [ref: src/generator_gemm_reference_impl.c:509-513]: they are built once from the pattern and serve both of two operand sets
 * (two mini-batches, the halves of a double buffer) -- only the three bases of a call move.
 *
 *   segments_backward_driver      exit 0 if every pass matches its host loop (normf_rel < 1e-5); 2 without a device
 */
#include <libxsmm.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define BS 16          /* block edge */
#define RB 6           /* block rows of W */
#define CB 5           /* block columns of W */
#define PB 4           /* block columns of X, Y, dX, dY */
#define BLK ((size_t)BS * BS)
#define BYTES(nblocks) (sizeof(float) * BLK * (size_t)(nblocks))

static float frand(void) { return (float)((int)(libxsmm_rng_f64() * 10.0) - 5) / 10.0f; }   /* multiples of 0.1 */

static void* upload(const void* host, size_t bytes) {
  void* dev = libxsmm_hip_malloc(bytes > 0 ? bytes : 1);
  if (NULL == dev || (bytes > 0 && libxsmm_hip_memcpy_h2d(dev, host, bytes) != 0)) { fprintf(stderr, "device allocation or copy failed\n"); exit(3); }
  return dev;
}

/* one pass: seg_ptr / a_offs / b_offs are the pattern's lists; C block s lies at s blocks from its base */
typedef struct pass { size_t nseg, nprod; unsigned long long seg_ptr[RB * CB * PB + 1]; long long a_offs[RB * CB * PB], b_offs[RB * CB * PB], c_offs[RB * CB * PB];
  void *d_seg, *d_a, *d_b, *d_c; libxsmm_gemmfunction kernel; } pass;

static void pass_begin(pass* q) { q->nseg = 0; q->nprod = 0; q->seg_ptr[0] = 0; }
static void pass_product(pass* q, size_t a_block, size_t b_block) { q->a_offs[q->nprod] = (long long)BYTES(a_block); q->b_offs[q->nprod] = (long long)BYTES(b_block); ++q->nprod; }
static void pass_segment(pass* q) { q->c_offs[q->nseg] = (long long)BYTES(q->nseg); q->seg_ptr[++q->nseg] = q->nprod; }
static void pass_finish(pass* q, int flags) {
  const libxsmm_gemm_shape shape = libxsmm_create_gemm_shape(BS, BS, BS, BS, BS, BS, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32);
  const libxsmm_gemm_batch_reduce_config brcfg = libxsmm_create_gemm_batch_reduce_config(LIBXSMM_GEMM_BATCH_REDUCE_OFFSET, 0, 0, 0);
  q->kernel = libxsmm_dispatch_brgemm(shape, (libxsmm_bitfield)(LIBXSMM_GEMM_FLAG_BETA_0 | flags), LIBXSMM_GEMM_PREFETCH_NONE, brcfg);
  if (NULL == q->kernel) { fprintf(stderr, "dispatch returned NULL\n"); exit(3); }
  q->d_seg = upload(q->seg_ptr, sizeof(unsigned long long) * (q->nseg + 1));
  q->d_a = upload(q->a_offs, sizeof(long long) * q->nprod); q->d_b = upload(q->b_offs, sizeof(long long) * q->nprod); q->d_c = upload(q->c_offs, sizeof(long long) * q->nseg);
}
static void pass_run(const pass* q, const void* a, const void* b, void* c) {
  libxsmm_gemm_param param;
  memset(&param, 0, sizeof(param));
  param.a.primary = (void*)a; param.b.primary = (void*)b; param.c.primary = c;          /* the three bases: all that changes between operand sets */
  libxsmm_hip_gemm_batch_reduce_segments_offsets(q->kernel, &param, q->nseg, (const unsigned long long*)q->d_seg, (const long long*)q->d_a, (const long long*)q->d_b,
    (const long long*)q->d_c);
  if (libxsmm_hip_get_last_error() != 0) { fprintf(stderr, "offsets call failed: %s\n", libxsmm_hip_get_last_error_string()); exit(1); }
}
static void pass_free(pass* q) { libxsmm_hip_free(q->d_seg); libxsmm_hip_free(q->d_a); libxsmm_hip_free(q->d_b); libxsmm_hip_free(q->d_c); }

/* element (i, j) of block (br, bc) of a dense matrix stored as column-major blocks, `ncb` blocks per block row */
static double at(const float* x, int ncb, int br, int bc, int i, int j) { return (double)x[BLK * ((size_t)br * ncb + bc) + (size_t)j * BS + i]; }

static void accumulate(double got, double gold, double* err, double* ref) { *err += (got - gold) * (got - gold); *ref += gold * gold; }

int main(void) {
  static pass fwd, bwd_data, bwd_weights;
  static float w[RB * CB * BS * BS], x[2][CB * PB * BS * BS], dy[2][RB * PB * BS * BS], y[RB * PB * BS * BS], dx[CB * PB * BS * BS], dw[RB * CB * BS * BS];
  int pos[RB][CB], brow[RB * CB], bcol[RB * CB];   /* block (r, c) -> its place in the value buffer, or -1; and back */
  int nnz = 0, r, c, p, t, i, j, k, z;
  double worst[3] = {0.0, 0.0, 0.0};
  void *d_w, *d_x[2], *d_dy[2], *d_y, *d_dx, *d_dw;
  if (libxsmm_hip_device_count() <= 0) { printf("no HIP device\n"); return 2; }
  libxsmm_rng_set_seed(4242);
  for (r = 0; r < RB; ++r) for (c = 0; c < CB; ++c) {   /* about half the blocks; block row 2 is empty: segments of count 0 */
    pos[r][c] = (r != 2 && libxsmm_rng_f64() < 0.5) ? nnz : -1;
    if (pos[r][c] >= 0) { brow[nnz] = r; bcol[nnz] = c; ++nnz; }
  }
  for (i = 0; i < (int)(BLK * nnz); ++i) w[i] = frand();
  for (t = 0; t < 2; ++t) {
    for (i = 0; i < (int)(BLK * CB * PB); ++i) x[t][i] = frand();
    for (i = 0; i < (int)(BLK * RB * PB); ++i) dy[t][i] = frand();
  }
  /* the three sets of lists, from the pattern alone */
  pass_begin(&fwd);
  for (r = 0; r < RB; ++r) for (p = 0; p < PB; ++p) {
    for (c = 0; c < CB; ++c) if (pos[r][c] >= 0) pass_product(&fwd, (size_t)pos[r][c], (size_t)c * PB + p);
    pass_segment(&fwd);
  }
  pass_finish(&fwd, 0);
  pass_begin(&bwd_data);
  for (c = 0; c < CB; ++c) for (p = 0; p < PB; ++p) {
    for (r = 0; r < RB; ++r) if (pos[r][c] >= 0) pass_product(&bwd_data, (size_t)pos[r][c], (size_t)r * PB + p);
    pass_segment(&bwd_data);
  }
  pass_finish(&bwd_data, LIBXSMM_GEMM_FLAG_TRANS_A);
  pass_begin(&bwd_weights);
  for (z = 0; z < nnz; ++z) {
    for (p = 0; p < PB; ++p) pass_product(&bwd_weights, (size_t)brow[z] * PB + p, (size_t)bcol[z] * PB + p);
    pass_segment(&bwd_weights);
  }
  pass_finish(&bwd_weights, LIBXSMM_GEMM_FLAG_TRANS_B);
  d_w = upload(w, BYTES(nnz));
  for (t = 0; t < 2; ++t) { d_x[t] = upload(x[t], BYTES(CB * PB)); d_dy[t] = upload(dy[t], BYTES(RB * PB)); }
  d_y = upload(y, BYTES(RB * PB)); d_dx = upload(dx, BYTES(CB * PB)); d_dw = upload(dw, BYTES(nnz));
  for (t = 0; t < 2; ++t) {                       /* the same lists on two operand sets */
    double err[3] = {0.0, 0.0, 0.0}, ref[3] = {0.0, 0.0, 0.0};
    pass_run(&fwd, d_w, d_x[t], d_y);
    pass_run(&bwd_data, d_w, d_dy[t], d_dx);
    pass_run(&bwd_weights, d_dy[t], d_x[t], d_dw);
    if (libxsmm_hip_memcpy_d2h(y, d_y, BYTES(RB * PB)) != 0 || libxsmm_hip_memcpy_d2h(dx, d_dx, BYTES(CB * PB)) != 0 || (nnz > 0 && libxsmm_hip_memcpy_d2h(dw, d_dw, BYTES(nnz)) != 0)) return 3;
    for (r = 0; r < RB; ++r) for (p = 0; p < PB; ++p) for (j = 0; j < BS; ++j) for (i = 0; i < BS; ++i) {       /* Y = W X */
      double gold = 0.0;
      for (c = 0; c < CB; ++c) if (pos[r][c] >= 0) for (k = 0; k < BS; ++k) gold += at(w, 1, pos[r][c], 0, i, k) * at(x[t], PB, c, p, k, j);
      accumulate(at(y, PB, r, p, i, j), gold, &err[0], &ref[0]);
    }
    for (c = 0; c < CB; ++c) for (p = 0; p < PB; ++p) for (j = 0; j < BS; ++j) for (i = 0; i < BS; ++i) {       /* dX = W^T dY */
      double gold = 0.0;
      for (r = 0; r < RB; ++r) if (pos[r][c] >= 0) for (k = 0; k < BS; ++k) gold += at(w, 1, pos[r][c], 0, k, i) * at(dy[t], PB, r, p, k, j);
      accumulate(at(dx, PB, c, p, i, j), gold, &err[1], &ref[1]);
    }
    for (z = 0; z < nnz; ++z) for (j = 0; j < BS; ++j) for (i = 0; i < BS; ++i) {                               /* dW(r, c) = sum_p dY(r, p) X(c, p)^T */
      double gold = 0.0;
      for (p = 0; p < PB; ++p) for (k = 0; k < BS; ++k) gold += at(dy[t], PB, brow[z], p, i, k) * at(x[t], PB, bcol[z], p, j, k);
      accumulate(at(dw, 1, z, 0, i, j), gold, &err[2], &ref[2]);
    }
    for (i = 0; i < 3; ++i) { const double e = sqrt(err[i] / (ref[i] > 0 ? ref[i] : 1)); if (e > worst[i]) worst[i] = e; }
  }
  printf("block-sparse W: %d x %d blocks of %d x %d, %d stored; X, dY: %d block columns; two operand sets, one set of offset lists\n", RB, CB, BS, BS, nnz, PB);
  printf("Y  = W X     %zu segments, %zu products, one call (%s): normf_rel = %.3g\n", fwd.nseg, fwd.nprod, libxsmm_hip_kernel_name((const void*)fwd.kernel, 1), worst[0]);
  printf("dX = W^T dY  %zu segments, %zu products, one call (TRANS_A): normf_rel = %.3g\n", bwd_data.nseg, bwd_data.nprod, worst[1]);
  printf("dW = dY X^T  %zu segments, %zu products, one call (TRANS_B): normf_rel = %.3g\n", bwd_weights.nseg, bwd_weights.nprod, worst[2]);
  pass_free(&fwd); pass_free(&bwd_data); pass_free(&bwd_weights);
  libxsmm_hip_free(d_w); libxsmm_hip_free(d_y); libxsmm_hip_free(d_dx); libxsmm_hip_free(d_dw);
  for (t = 0; t < 2; ++t) { libxsmm_hip_free(d_x[t]); libxsmm_hip_free(d_dy[t]); }
  return (worst[0] < 1e-5 && worst[1] < 1e-5 && worst[2] < 1e-5) ? 0 : 1;
}
