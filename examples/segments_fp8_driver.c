/* segments_fp8_driver.c -- a block-sparse layer quantised to 8-bit floats, Y = W * X, as ONE libxsmm_hip_gemm_batch_reduce_segments call, checked against a
 * host loop that widens the same bytes with the conversions of libxsmm_utils.h.
 * W is MB x KB blocks of 64 x 64 HF8 (E4M3) values with a random pattern of 0 - 8 blocks per block row, each block stored as the VNNI-4 image the matrix core
 * reads, A(i, k) at ((k / 4) * 64 + i) * 4 + k % 4 (LIBXSMM_GEMM_FLAG_VNNI_A); X is KB x NB dense HF8 blocks, flat; Y is MB x NB f32 blocks.  Every block of Y is
 * one ADDRESS batch-reduce call of the reference whose count is the number of blocks in its block row of W [ref: src/generator_gemm_reference_impl.c:490-498];
 * here the layer is one launch.  Products of 8-bit floats are exact in f32; the matrix core adds the products of one instruction after aligning them, so the
 * result is the serial sum within a tolerance, not bit for bit.
 *
 *   segments_fp8_driver      exit 0 if Y matches the host loop (normf_rel < 1e-4); 2 without a device
 */
#include <libxsmm.h>
#include <libxsmm_utils.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define BS 64          /* block edge */
#define MB 24          /* block rows of W and Y */
#define KB 16          /* block columns of W = block rows of X */
#define NB 4           /* block columns of X and Y */
#define MAXROW 8       /* most blocks in a block row of W */

static libxsmm_hfloat8 hrand(void) { return libxsmm_convert_f32_to_hf8_rne((float)((int)(libxsmm_rng_f64() * 10.0) - 5) / 10.0f); }   /* multiples of 0.1, rounded to E4M3 */

int main(void) {
  const size_t blk = (size_t)BS * BS, nseg = (size_t)MB * NB;
  const libxsmm_gemm_shape shape = libxsmm_create_gemm_shape(BS, BS, BS, BS, BS, BS, LIBXSMM_DATATYPE_HF8, LIBXSMM_DATATYPE_HF8, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32);
  const libxsmm_gemm_batch_reduce_config brcfg = libxsmm_create_gemm_batch_reduce_config(LIBXSMM_GEMM_BATCH_REDUCE_ADDRESS, 0, 0, 0);
  libxsmm_gemmfunction kernel;
  libxsmm_gemm_param param;
  int rowcnt[MB], rowcol[MB][MAXROW];
  size_t rowfirst[MB + 1];                       /* W's blocks are stored block row by block row */
  unsigned long long* seg_ptr;
  const void **a_list, **b_list;
  void** c_list;
  libxsmm_hfloat8 *hw, *hx;
  float *hy, widen[256];
  char *dw, *dx, *dy;
  void *d_seg, *d_al, *d_bl, *d_cl;
  size_t nblocks = 0, nprod, i, s;
  unsigned long long launches;
  int ib, jb, r;
  double err = 0.0, ref = 0.0;
  if (libxsmm_hip_device_count() <= 0) { printf("no HIP device\n"); return 2; }
  kernel = libxsmm_dispatch_brgemm(shape, LIBXSMM_GEMM_FLAG_BETA_0 | LIBXSMM_GEMM_FLAG_VNNI_A, LIBXSMM_GEMM_PREFETCH_NONE, brcfg);
  if (NULL == kernel) { fprintf(stderr, "dispatch returned NULL\n"); return 3; }
  libxsmm_rng_set_seed(555);
  for (ib = 0; ib < MB; ++ib) {                  /* the pattern: 0 - 8 distinct block columns per block row, ascending */
    int used[KB], want = (int)(libxsmm_rng_f64() * (MAXROW + 1)), kb;
    memset(used, 0, sizeof(used));
    if (want > MAXROW) want = MAXROW;
    for (r = 0; r < want; ++r) used[(int)(libxsmm_rng_f64() * KB) % KB] = 1;
    rowcnt[ib] = 0;
    for (kb = 0; kb < KB; ++kb) if (used[kb]) rowcol[ib][rowcnt[ib]++] = kb;
    rowfirst[ib] = nblocks; nblocks += (size_t)rowcnt[ib];
  }
  rowfirst[MB] = nblocks;
  nprod = nblocks * NB;
  hw = (libxsmm_hfloat8*)malloc(blk * (nblocks + 1)); hx = (libxsmm_hfloat8*)malloc(blk * KB * NB); hy = (float*)malloc(sizeof(float) * blk * nseg);
  seg_ptr = (unsigned long long*)malloc(sizeof(unsigned long long) * (nseg + 1));
  a_list = (const void**)malloc(sizeof(void*) * (nprod + 1)); b_list = (const void**)malloc(sizeof(void*) * (nprod + 1)); c_list = (void**)malloc(sizeof(void*) * nseg);
  dw = (char*)libxsmm_hip_malloc(blk * (nblocks + 1)); dx = (char*)libxsmm_hip_malloc(blk * KB * NB); dy = (char*)libxsmm_hip_malloc(sizeof(float) * blk * nseg);
  d_seg = libxsmm_hip_malloc(sizeof(unsigned long long) * (nseg + 1));
  d_al = libxsmm_hip_malloc(sizeof(void*) * (nprod + 1)); d_bl = libxsmm_hip_malloc(sizeof(void*) * (nprod + 1)); d_cl = libxsmm_hip_malloc(sizeof(void*) * nseg);
  if (!hw || !hx || !hy || !seg_ptr || !a_list || !b_list || !c_list || !dw || !dx || !dy || !d_seg || !d_al || !d_bl || !d_cl) return 3;
  for (i = 0; i < blk * nblocks; ++i) hw[i] = hrand();     /* every byte of a block is one element: filling the VNNI-4 image in memory order draws them all */
  for (i = 0; i < blk * KB * NB; ++i) hx[i] = hrand();
  for (i = 0; i < 256; ++i) widen[i] = libxsmm_convert_hf8_to_f32((libxsmm_hfloat8)i);
  /* segment s = (ib, jb): the products W(ib, kb) * X(kb, jb) over the pattern of block row ib, in ascending kb; X's block (kb, jb) is stored at kb + jb * KB */
  seg_ptr[0] = 0;
  for (ib = 0, s = 0; ib < MB; ++ib) for (jb = 0; jb < NB; ++jb, ++s) {
    size_t at = (size_t)seg_ptr[s];
    for (r = 0; r < rowcnt[ib]; ++r, ++at) {
      a_list[at] = dw + blk * (rowfirst[ib] + (size_t)r);
      b_list[at] = dx + blk * ((size_t)rowcol[ib][r] + (size_t)jb * KB);
    }
    seg_ptr[s + 1] = at;
    c_list[s] = dy + sizeof(float) * blk * s;
  }
  if (libxsmm_hip_memcpy_h2d(dw, hw, blk * (nblocks + 1)) != 0 || libxsmm_hip_memcpy_h2d(dx, hx, blk * KB * NB) != 0
    || libxsmm_hip_memcpy_h2d(d_seg, seg_ptr, sizeof(unsigned long long) * (nseg + 1)) != 0 || libxsmm_hip_memcpy_h2d(d_cl, c_list, sizeof(void*) * nseg) != 0
    || (nprod > 0 && (libxsmm_hip_memcpy_h2d(d_al, a_list, sizeof(void*) * nprod) != 0 || libxsmm_hip_memcpy_h2d(d_bl, b_list, sizeof(void*) * nprod) != 0))) return 3;
  memset(&param, 0, sizeof(param));              /* the primary slots and op.tertiary are ignored: the lists carry everything */
  (void)libxsmm_hip_launch_count(1);
  libxsmm_hip_gemm_batch_reduce_segments(kernel, &param, nseg, (const unsigned long long*)d_seg, (const void* const*)d_al, (const void* const*)d_bl, (void* const*)d_cl);
  launches = libxsmm_hip_launch_count(0);
  if (libxsmm_hip_get_last_error() != 0) { fprintf(stderr, "segments call failed: %s\n", libxsmm_hip_get_last_error_string()); return 1; }
  if (libxsmm_hip_memcpy_d2h(hy, dy, sizeof(float) * blk * nseg) != 0) return 3;
  for (ib = 0, s = 0; ib < MB; ++ib) for (jb = 0; jb < NB; ++jb, ++s) {   /* the plain loop on the widened bytes */
    const float* c = hy + blk * s;
    int ii, jj, kk;
    for (jj = 0; jj < BS; ++jj) for (ii = 0; ii < BS; ++ii) {
      double gold = 0.0;
      for (r = 0; r < rowcnt[ib]; ++r) {
        const libxsmm_hfloat8 *a = hw + blk * (rowfirst[ib] + (size_t)r), *b = hx + blk * ((size_t)rowcol[ib][r] + (size_t)jb * KB);
        for (kk = 0; kk < BS; ++kk) gold += (double)widen[a[((kk / 4) * BS + ii) * 4 + kk % 4]] * widen[b[kk + jj * BS]];
      }
      err += (c[ii + jj * BS] - gold) * (c[ii + jj * BS] - gold); ref += gold * gold;
    }
  }
  err = sqrt(err / (ref > 0 ? ref : 1));
  printf("block-sparse HF8 W: %d x %d blocks of %d x %d, %zu stored (%zu bytes); X: %d x %d blocks\n", MB, KB, BS, BS, nblocks, blk * nblocks, KB, NB);
  printf("%zu segments, %zu products, %llu launch (%s): normf_rel = %.3g\n", nseg, nprod, launches, libxsmm_hip_kernel_name((const void*)kernel, 1), err);
  free(hw); free(hx); free(hy); free(seg_ptr); free((void*)a_list); free((void*)b_list); free((void*)c_list);
  libxsmm_hip_free(dw); libxsmm_hip_free(dx); libxsmm_hip_free(dy); libxsmm_hip_free(d_seg); libxsmm_hip_free(d_al); libxsmm_hip_free(d_bl); libxsmm_hip_free(d_cl);
  return (err < 1e-4 && launches == 1) ? 0 : 1;
}
