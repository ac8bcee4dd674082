/* segments_fused_driver.c -- a block-sparse layer with bias + ReLU as ONE libxsmm_hip_gemm_ext_batch_reduce_segments call, checked against the plain host loop.
 * A is MB x KB blocks of 32 x 32 with a random pattern of 0 - 8 blocks per block row, B is KB x NB dense blocks, C = A * B is MB x NB blocks.  Every block of C
 * is one ADDRESS batch-reduce call of the reference whose count is the number of blocks in its block row of A [ref: src/generator_gemm_reference_impl.c:490-498];
 * here the whole product is one call: segment (ib, jb) lists the blocks A(ib, kb) and B(kb, jb) of that row's pattern.  The handle comes from
 * libxsmm_dispatch_brgemm_ext with a column bias and a ReLU: block row ib has a bias vector of its own (d_list repeats it for the NB segments of the row), and
 * an empty block row stores relu(bias).  All lists live in device memory.
 *
 *   segments_fused_driver      exit 0 if C matches the host loop (normf_rel < 1e-5); 2 without a device
 */
#include <libxsmm.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define BS 32          /* block edge */
#define MB 48          /* block rows of A and C */
#define KB 24          /* block columns of A = block rows of B */
#define NB 6           /* block columns of B and C */
#define MAXROW 8       /* most blocks in a block row of A */

static float frand(void) { return (float)((int)(libxsmm_rng_f64() * 10.0) - 5) / 10.0f; }   /* multiples of 0.1 */

int main(void) {
  const size_t blk = (size_t)BS * BS, nseg = (size_t)MB * NB;
  const libxsmm_gemm_shape shape = libxsmm_create_gemm_shape(BS, BS, BS, BS, BS, BS, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32);
  const libxsmm_gemm_batch_reduce_config brcfg = libxsmm_create_gemm_batch_reduce_config(LIBXSMM_GEMM_BATCH_REDUCE_ADDRESS, 0, 0, 0);
  const libxsmm_gemm_ext_unary_argops argops = libxsmm_create_gemm_ext_unary_argops(0, LIBXSMM_MELTW_TYPE_UNARY_NONE, LIBXSMM_MELTW_FLAG_UNARY_NONE, 0,
    0, LIBXSMM_MELTW_TYPE_UNARY_NONE, LIBXSMM_MELTW_FLAG_UNARY_NONE, 0, BS, LIBXSMM_MELTW_TYPE_UNARY_RELU, LIBXSMM_MELTW_FLAG_UNARY_NONE, 0);
  const libxsmm_gemm_ext_binary_postops postops = libxsmm_create_gemm_ext_binary_postops(BS, LIBXSMM_DATATYPE_F32, LIBXSMM_MELTW_TYPE_BINARY_ADD,
    LIBXSMM_MELTW_FLAG_BINARY_BCAST_COL_IN_0);
  libxsmm_gemmfunction_ext kernel;
  libxsmm_gemm_ext_param param;
  int rowcnt[MB], rowcol[MB][MAXROW];
  size_t rowfirst[MB + 1];                       /* A's blocks are stored block row by block row */
  unsigned long long* seg_ptr;
  const void **a_list, **b_list, **d_list;
  void** c_list;
  float *ha, *hb, *hc, *hd;
  char *da, *db, *dc, *dd;
  void *d_seg, *d_al, *d_bl, *d_cl, *d_dl;
  size_t nblocks = 0, nprod, i, s;
  int ib, jb, r, empty = 0;
  double err = 0.0, ref = 0.0;
  if (libxsmm_hip_device_count() <= 0) { printf("no HIP device\n"); return 2; }
  kernel = libxsmm_dispatch_brgemm_ext(shape, LIBXSMM_GEMM_FLAG_BETA_0, LIBXSMM_GEMM_PREFETCH_NONE, brcfg, argops, postops);
  if (NULL == kernel) { fprintf(stderr, "dispatch returned NULL\n"); return 3; }
  libxsmm_rng_set_seed(777);
  for (ib = 0; ib < MB; ++ib) {                  /* the pattern: 0 - 8 distinct block columns per block row, ascending */
    int used[KB], want = (int)(libxsmm_rng_f64() * (MAXROW + 1)), kb;
    memset(used, 0, sizeof(used));
    if (want > MAXROW) want = MAXROW;
    for (r = 0; r < want; ++r) used[(int)(libxsmm_rng_f64() * KB) % KB] = 1;
    rowcnt[ib] = 0;
    for (kb = 0; kb < KB; ++kb) if (used[kb]) rowcol[ib][rowcnt[ib]++] = kb;
    rowfirst[ib] = nblocks; nblocks += (size_t)rowcnt[ib];
    if (rowcnt[ib] == 0) ++empty;
  }
  rowfirst[MB] = nblocks;
  nprod = nblocks * NB;
  ha = (float*)malloc(sizeof(float) * blk * (nblocks + 1)); hb = (float*)malloc(sizeof(float) * blk * KB * NB); hc = (float*)malloc(sizeof(float) * blk * nseg);
  hd = (float*)malloc(sizeof(float) * BS * MB); d_list = (const void**)malloc(sizeof(void*) * nseg);
  seg_ptr = (unsigned long long*)malloc(sizeof(unsigned long long) * (nseg + 1));
  a_list = (const void**)malloc(sizeof(void*) * (nprod + 1)); b_list = (const void**)malloc(sizeof(void*) * (nprod + 1)); c_list = (void**)malloc(sizeof(void*) * nseg);
  da = (char*)libxsmm_hip_malloc(sizeof(float) * blk * (nblocks + 1)); db = (char*)libxsmm_hip_malloc(sizeof(float) * blk * KB * NB); dc = (char*)libxsmm_hip_malloc(sizeof(float) * blk * nseg);
  d_seg = libxsmm_hip_malloc(sizeof(unsigned long long) * (nseg + 1));
  d_al = libxsmm_hip_malloc(sizeof(void*) * (nprod + 1)); d_bl = libxsmm_hip_malloc(sizeof(void*) * (nprod + 1)); d_cl = libxsmm_hip_malloc(sizeof(void*) * nseg);
  dd = (char*)libxsmm_hip_malloc(sizeof(float) * BS * MB); d_dl = libxsmm_hip_malloc(sizeof(void*) * nseg);
  if (!hd || !d_list || !dd || !d_dl) return 3;
  if (!ha || !hb || !hc || !seg_ptr || !a_list || !b_list || !c_list || !da || !db || !dc || !d_seg || !d_al || !d_bl || !d_cl) return 3;
  for (i = 0; i < blk * nblocks; ++i) ha[i] = frand();
  for (i = 0; i < blk * KB * NB; ++i) hb[i] = frand();
  for (i = 0; i < (size_t)BS * MB; ++i) hd[i] = frand();
  /* segment s = (ib, jb): the products A(ib, kb) * B(kb, jb) over the pattern of block row ib, in ascending kb; B's block (kb, jb) is stored at kb + jb * KB */
  seg_ptr[0] = 0;
  for (ib = 0, s = 0; ib < MB; ++ib) for (jb = 0; jb < NB; ++jb, ++s) {
    size_t at = (size_t)seg_ptr[s];
    for (r = 0; r < rowcnt[ib]; ++r, ++at) {
      a_list[at] = da + sizeof(float) * blk * (rowfirst[ib] + (size_t)r);
      b_list[at] = db + sizeof(float) * blk * ((size_t)rowcol[ib][r] + (size_t)jb * KB);
    }
    seg_ptr[s + 1] = at;
    c_list[s] = dc + sizeof(float) * blk * s;
    d_list[s] = dd + sizeof(float) * BS * (size_t)ib;      /* one bias vector per block row, shared by the row's NB segments */
  }
  if (libxsmm_hip_memcpy_h2d(da, ha, sizeof(float) * blk * nblocks) != 0 || libxsmm_hip_memcpy_h2d(db, hb, sizeof(float) * blk * KB * NB) != 0
    || libxsmm_hip_memcpy_h2d(dd, hd, sizeof(float) * BS * MB) != 0 || libxsmm_hip_memcpy_h2d(d_dl, d_list, sizeof(void*) * nseg) != 0
    || libxsmm_hip_memcpy_h2d(d_seg, seg_ptr, sizeof(unsigned long long) * (nseg + 1)) != 0 || libxsmm_hip_memcpy_h2d(d_cl, c_list, sizeof(void*) * nseg) != 0
    || (nprod > 0 && (libxsmm_hip_memcpy_h2d(d_al, a_list, sizeof(void*) * nprod) != 0 || libxsmm_hip_memcpy_h2d(d_bl, b_list, sizeof(void*) * nprod) != 0))) return 3;
  memset(&param, 0, sizeof(param));              /* the primary slots and op.tertiary are ignored: the lists carry everything (no bitmask: mask_list is NULL) */
  libxsmm_hip_gemm_ext_batch_reduce_segments(kernel, &param, nseg, (const unsigned long long*)d_seg, (const void* const*)d_al, (const void* const*)d_bl, (void* const*)d_cl,
    (const void* const*)d_dl, NULL);
  if (libxsmm_hip_get_last_error() != 0) { fprintf(stderr, "segments call failed: %s\n", libxsmm_hip_get_last_error_string()); return 1; }
  if (libxsmm_hip_memcpy_d2h(hc, dc, sizeof(float) * blk * nseg) != 0) return 3;
  for (ib = 0, s = 0; ib < MB; ++ib) for (jb = 0; jb < NB; ++jb, ++s) {   /* the plain loop */
    const float* c = hc + blk * s;
    int ii, jj, kk;
    for (jj = 0; jj < BS; ++jj) for (ii = 0; ii < BS; ++ii) {
      double gold = hd[(size_t)ib * BS + ii];         /* the bias indexes C's rows */
      for (r = 0; r < rowcnt[ib]; ++r) {
        const float *a = ha + blk * (rowfirst[ib] + (size_t)r), *b = hb + blk * ((size_t)rowcol[ib][r] + (size_t)jb * KB);
        for (kk = 0; kk < BS; ++kk) gold += (double)a[ii + kk * BS] * b[kk + jj * BS];
      }
      if (gold < 0.0) gold = 0.0;
      err += (c[ii + jj * BS] - gold) * (c[ii + jj * BS] - gold); ref += gold * gold;
    }
  }
  err = sqrt(err / (ref > 0 ? ref : 1));
  printf("block-sparse A: %d x %d blocks of %d x %d, %zu stored (%d empty block rows); B: %d x %d blocks\n", MB, KB, BS, BS, nblocks, empty, KB, NB);
  printf("%zu segments, %zu products, bias + ReLU, one call (%s): normf_rel = %.3g\n", nseg, nprod, libxsmm_hip_kernel_name((const void*)kernel, 1), err);
  free(ha); free(hb); free(hc); free(seg_ptr); free((void*)a_list); free((void*)b_list); free((void*)c_list); free(hd); free((void*)d_list);
  libxsmm_hip_free(dd); libxsmm_hip_free(d_dl); libxsmm_hip_free(da); libxsmm_hip_free(db); libxsmm_hip_free(dc); libxsmm_hip_free(d_seg); libxsmm_hip_free(d_al); libxsmm_hip_free(d_bl); libxsmm_hip_free(d_cl);
  return err < 1e-5 ? 0 : 1;
}
