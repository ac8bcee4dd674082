/* segments_f16_driver.c -- a block-sparse layer in IEEE halves with its bias and ReLU, Y = relu(W * X + b), as ONE
 * libxsmm_hip_gemm_ext_batch_reduce_segments_offsets call, checked against a host loop that widens the same halves with the conversions of libxsmm_utils.h.
 * W is MB x KB blocks of 64 x 64 f16 values with a random pattern of 0 - 8 blocks per block row, each block stored as the VNNI-2 image the matrix core reads,
 * A(i, k) at ((k / 2) * 64 + i) * 2 + k % 2 (LIBXSMM_GEMM_FLAG_VNNI_A); X is KB x NB dense f16 blocks, flat; Y is MB x NB f16 blocks; b has 64 halves per block
 * row.  Every operand is ONE buffer and the lists hold byte offsets into it, so the lists of a pattern serve every buffer [ref:
 * src/generator_gemm_reference_impl.c:509-513].  Every block of Y is one fused OFFSET batch-reduce call of the reference whose count is the number of blocks in its
 * block row of W [:294-372]; here the layer is one launch.  The arithmetic is the reference's F16 loop [:2025-2124]: the products are summed in f32 from +0, the
 * bias -- a half -- is added behind the sum, then ReLU, then one rounding to f16.  A block row without blocks stores relu(b).
 *
 *   segments_f16_driver      exit 0 if Y matches the host loop (normf_rel < 1e-3, the bound of an f16 result); 2 without a device
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

static libxsmm_float16 hrand(void) { return libxsmm_convert_f32_to_f16((float)((int)(libxsmm_rng_f64() * 10.0) - 5) / 10.0f); }   /* multiples of 0.1, rounded to f16 */

int main(void) {
  const size_t blk = (size_t)BS * BS, nseg = (size_t)MB * NB, esz = sizeof(libxsmm_float16);
  const libxsmm_gemm_shape shape = libxsmm_create_gemm_shape(BS, BS, BS, BS, BS, BS, LIBXSMM_DATATYPE_F16, LIBXSMM_DATATYPE_F16, LIBXSMM_DATATYPE_F16, LIBXSMM_DATATYPE_F32);
  const libxsmm_gemm_batch_reduce_config brcfg = libxsmm_create_gemm_batch_reduce_config(LIBXSMM_GEMM_BATCH_REDUCE_OFFSET, 0, 0, 0);
  const libxsmm_gemm_ext_unary_argops argops = libxsmm_create_gemm_ext_unary_argops(0, LIBXSMM_MELTW_TYPE_UNARY_NONE, LIBXSMM_MELTW_FLAG_UNARY_NONE, 0,
    0, LIBXSMM_MELTW_TYPE_UNARY_NONE, LIBXSMM_MELTW_FLAG_UNARY_NONE, 0, BS, LIBXSMM_MELTW_TYPE_UNARY_RELU, LIBXSMM_MELTW_FLAG_UNARY_NONE, 0);
  const libxsmm_gemm_ext_binary_postops postops = libxsmm_create_gemm_ext_binary_postops(BS, LIBXSMM_DATATYPE_F16, LIBXSMM_MELTW_TYPE_BINARY_ADD,
    LIBXSMM_MELTW_FLAG_BINARY_BCAST_COL_IN_0);
  libxsmm_gemmfunction_ext kernel;
  libxsmm_gemm_ext_param param;
  int rowcnt[MB], rowcol[MB][MAXROW];
  size_t rowfirst[MB + 1];                       /* W's blocks are stored block row by block row */
  unsigned long long* seg_ptr;
  long long *a_offs, *b_offs, *c_offs, *d_offs;
  libxsmm_float16 *hw, *hx, *hb, *hy;
  char *dw, *dx, *db, *dy;
  void *d_seg, *d_ao, *d_bo, *d_co, *d_do;
  size_t nblocks = 0, nprod, i, s;
  unsigned long long launches;
  int ib, jb, r;
  double err = 0.0, ref = 0.0;
  if (libxsmm_hip_device_count() <= 0) { printf("no HIP device\n"); return 2; }
  kernel = libxsmm_dispatch_brgemm_ext(shape, LIBXSMM_GEMM_FLAG_BETA_0 | LIBXSMM_GEMM_FLAG_VNNI_A, LIBXSMM_GEMM_PREFETCH_NONE, brcfg, argops, postops);
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
  hw = (libxsmm_float16*)malloc(esz * blk * (nblocks + 1)); hx = (libxsmm_float16*)malloc(esz * blk * KB * NB);
  hb = (libxsmm_float16*)malloc(esz * BS * MB); hy = (libxsmm_float16*)malloc(esz * blk * nseg);
  seg_ptr = (unsigned long long*)malloc(sizeof(unsigned long long) * (nseg + 1));
  a_offs = (long long*)malloc(sizeof(long long) * (nprod + 1)); b_offs = (long long*)malloc(sizeof(long long) * (nprod + 1));
  c_offs = (long long*)malloc(sizeof(long long) * nseg); d_offs = (long long*)malloc(sizeof(long long) * nseg);
  dw = (char*)libxsmm_hip_malloc(esz * blk * (nblocks + 1)); dx = (char*)libxsmm_hip_malloc(esz * blk * KB * NB);
  db = (char*)libxsmm_hip_malloc(esz * BS * MB); dy = (char*)libxsmm_hip_malloc(esz * blk * nseg);
  d_seg = libxsmm_hip_malloc(sizeof(unsigned long long) * (nseg + 1));
  d_ao = libxsmm_hip_malloc(sizeof(long long) * (nprod + 1)); d_bo = libxsmm_hip_malloc(sizeof(long long) * (nprod + 1));
  d_co = libxsmm_hip_malloc(sizeof(long long) * nseg); d_do = libxsmm_hip_malloc(sizeof(long long) * nseg);
  if (!hw || !hx || !hb || !hy || !seg_ptr || !a_offs || !b_offs || !c_offs || !d_offs || !dw || !dx || !db || !dy || !d_seg || !d_ao || !d_bo || !d_co || !d_do) return 3;
  /* every half of a block is one element: filling the VNNI-2 image in memory order draws them all (one spare block, so that a pattern without blocks still
   * has a buffer: it is filled too, the whole allocation is copied) */
  for (i = 0; i < blk * (nblocks + 1); ++i) hw[i] = hrand();
  for (i = 0; i < blk * KB * NB; ++i) hx[i] = hrand();
  for (i = 0; i < (size_t)BS * MB; ++i) hb[i] = hrand();
  /* segment s = (ib, jb): the products W(ib, kb) * X(kb, jb) over the pattern of block row ib, in ascending kb; X's block (kb, jb) is stored at kb + jb * KB */
  seg_ptr[0] = 0;
  for (ib = 0, s = 0; ib < MB; ++ib) for (jb = 0; jb < NB; ++jb, ++s) {
    size_t at = (size_t)seg_ptr[s];
    for (r = 0; r < rowcnt[ib]; ++r, ++at) {
      a_offs[at] = (long long)(esz * blk * (rowfirst[ib] + (size_t)r));
      b_offs[at] = (long long)(esz * blk * ((size_t)rowcol[ib][r] + (size_t)jb * KB));
    }
    seg_ptr[s + 1] = at;
    c_offs[s] = (long long)(esz * blk * s);
    d_offs[s] = (long long)(esz * BS * (size_t)ib);          /* the NB segments of a block row share its bias */
  }
  if (libxsmm_hip_memcpy_h2d(dw, hw, esz * blk * (nblocks + 1)) != 0 || libxsmm_hip_memcpy_h2d(dx, hx, esz * blk * KB * NB) != 0
    || libxsmm_hip_memcpy_h2d(db, hb, esz * BS * MB) != 0
    || libxsmm_hip_memcpy_h2d(d_seg, seg_ptr, sizeof(unsigned long long) * (nseg + 1)) != 0 || libxsmm_hip_memcpy_h2d(d_co, c_offs, sizeof(long long) * nseg) != 0
    || libxsmm_hip_memcpy_h2d(d_do, d_offs, sizeof(long long) * nseg) != 0
    || (nprod > 0 && (libxsmm_hip_memcpy_h2d(d_ao, a_offs, sizeof(long long) * nprod) != 0 || libxsmm_hip_memcpy_h2d(d_bo, b_offs, sizeof(long long) * nprod) != 0))) return 3;
  memset(&param, 0, sizeof(param));              /* the bases the offsets are added to; op.tertiary is ignored: seg_ptr carries the counts */
  param.a.primary = dw; param.b.primary = dx; param.c.primary = dy; param.d.primary = db;
  (void)libxsmm_hip_launch_count(1);
  libxsmm_hip_gemm_ext_batch_reduce_segments_offsets(kernel, &param, nseg, (const unsigned long long*)d_seg, (const long long*)d_ao, (const long long*)d_bo,
    (const long long*)d_co, (const long long*)d_do, NULL);
  launches = libxsmm_hip_launch_count(0);
  if (libxsmm_hip_get_last_error() != 0) { fprintf(stderr, "segments call failed: %s\n", libxsmm_hip_get_last_error_string()); return 1; }
  if (libxsmm_hip_memcpy_d2h(hy, dy, esz * blk * nseg) != 0) return 3;
  for (ib = 0, s = 0; ib < MB; ++ib) for (jb = 0; jb < NB; ++jb, ++s) {   /* the plain loop on the widened halves */
    const libxsmm_float16* c = hy + blk * s;
    int ii, jj, kk;
    for (jj = 0; jj < BS; ++jj) for (ii = 0; ii < BS; ++ii) {
      double gold = 0.0, got;
      for (r = 0; r < rowcnt[ib]; ++r) {
        const libxsmm_float16 *a = hw + blk * (rowfirst[ib] + (size_t)r), *b = hx + blk * ((size_t)rowcol[ib][r] + (size_t)jb * KB);
        for (kk = 0; kk < BS; ++kk) gold += (double)libxsmm_convert_f16_to_f32(a[((kk / 2) * BS + ii) * 2 + kk % 2]) * libxsmm_convert_f16_to_f32(b[kk + jj * BS]);
      }
      gold += libxsmm_convert_f16_to_f32(hb[(size_t)ib * BS + ii]);
      if (gold <= 0.0) gold = 0.0;
      got = libxsmm_convert_f16_to_f32(c[ii + jj * BS]);
      err += (got - gold) * (got - gold); ref += gold * gold;
    }
  }
  err = sqrt(err / (ref > 0 ? ref : 1));
  printf("block-sparse f16 W: %d x %d blocks of %d x %d, %zu stored (%zu bytes); X: %d x %d blocks; bias + ReLU fused\n", MB, KB, BS, BS, nblocks, esz * blk * nblocks, KB, NB);
  printf("%zu segments, %zu products, %llu launch (%s): normf_rel = %.3g\n", nseg, nprod, launches, libxsmm_hip_kernel_name((const void*)kernel, 1), err);
  free(hw); free(hx); free(hb); free(hy); free(seg_ptr); free(a_offs); free(b_offs); free(c_offs); free(d_offs);
  libxsmm_hip_free(dw); libxsmm_hip_free(dx); libxsmm_hip_free(db); libxsmm_hip_free(dy); libxsmm_hip_free(d_seg);
  libxsmm_hip_free(d_ao); libxsmm_hip_free(d_bo); libxsmm_hip_free(d_co); libxsmm_hip_free(d_do);
  return (err < 1e-3 && launches == 1) ? 0 : 1;
}
