/* segments_sliced_fused_driver.c -- a 3 x 3 convolution forward on a SMALL image with bias + ReLU + bitmask as ONE
 * libxsmm_hip_gemm_ext_batch_reduce_segments_offsets_sliced call per image, with chains cut by the caller: a small image has few output row blocks (here 14) and
 * each has a long chain (Cb x 9 products), so the unsliced entry would keep 14 waves busy; here every (row block, input-channel block) is a slice of 9 (6 at the
 * border) products that a wave of its own walks, and the second launch adds a row block's Cb partials in order onto the bias and applies ReLU + bitmask.  Checked against the direct seven-loop convolution (image, output channel, row, pixel, input channel, tap row, tap column; the channel loops split into
 * blocks) on the host.  The layouts are the reference's blocked ones: input [Cb][H][W + 2][bc], physically padded in W
 * only; weights [Kb][Cb][3][3][bc][bk]; output [Kb][H][W][bk].  One output row block (kb, h) is one OFFSET batch-reduce call of the reference
 * [ref: src/generator_gemm_reference_impl.c:509-513] with m = bk, n = W, k = bc: A is the weight block of a tap (bk contiguous: flat, lda = bk), B the W pixels
 * of the input row the tap sees, shifted by the tap's column (bc contiguous: flat, ldb = bc), and the count is Cb x (taps that exist) -- the top and the bottom
 * row have no row above / below them and see 6 of the 9 taps.  Here the H x Kb calls are the BLOCKS of one sliced call, block (kb, h) owns the Cb slices
 * blk_ptr[s] .. blk_ptr[s + 1], slice (kb, h, cb) the taps of one input-channel block; the bias is the vector of the output-channel block (d_offs repeats it
 * over the rows), and every block writes the ReLU bitmask of its row block.  The lists depend on the layer geometry only: they are built ONCE and serve two
 * images by moving the input, output and mask bases; the workspace is reused.
 *
 *   segments_sliced_fused_driver      exit 0 if both outputs and masks match the host convolution (normf_rel < 1e-5, every mask bit) in 2 launches per
 *                                     image; 2 without a device
 */
#include <libxsmm.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CB 3           /* input-channel blocks */
#define KB 2           /* output-channel blocks */
#define BC 16          /* input channels per block */
#define BK 16          /* output channels per block */
#define H 7
#define W 12
#define WP (W + 2)     /* padded row */
#define NIMG 2

static float frand(void) { return (float)((int)(libxsmm_rng_f64() * 9.0) - 4) / 8.0f; }   /* multiples of 1 / 8: every sum is exact */

int main(void) {
  const size_t in_elems = (size_t)CB * H * WP * BC, wt_elems = (size_t)KB * CB * 9 * BC * BK, out_elems = (size_t)KB * H * W * BK, nseg = (size_t)KB * H;
  const size_t mask_blk = (size_t)((BK + 15) / 16 * 16 / 8) * W, mask_bytes = mask_blk * nseg;
  const libxsmm_gemm_shape shape = libxsmm_create_gemm_shape(BK, W, BC, BK, BC, BK, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32);
  const libxsmm_gemm_batch_reduce_config brcfg = libxsmm_create_gemm_batch_reduce_config(LIBXSMM_GEMM_BATCH_REDUCE_OFFSET, 0, 0, 0);
  const libxsmm_gemm_ext_unary_argops argops = libxsmm_create_gemm_ext_unary_argops(0, LIBXSMM_MELTW_TYPE_UNARY_NONE, LIBXSMM_MELTW_FLAG_UNARY_NONE, 0,
    0, LIBXSMM_MELTW_TYPE_UNARY_NONE, LIBXSMM_MELTW_FLAG_UNARY_NONE, 0, BK, LIBXSMM_MELTW_TYPE_UNARY_RELU, LIBXSMM_MELTW_FLAG_UNARY_BITMASK_2BYTEMULT, 0);
  const libxsmm_gemm_ext_binary_postops postops = libxsmm_create_gemm_ext_binary_postops(BK, LIBXSMM_DATATYPE_F32, LIBXSMM_MELTW_TYPE_BINARY_ADD,
    LIBXSMM_MELTW_FLAG_BINARY_BCAST_COL_IN_0);
  libxsmm_gemmfunction_ext kernel;
  libxsmm_gemm_ext_param param;
  unsigned long long blk_ptr[KB * H + 1], seg_ptr[KB * H * CB + 1], launches = 0;
  long long a_offs[KB * H * CB * 9], b_offs[KB * H * CB * 9], c_offs[KB * H], d_offs[KB * H], mask_offs[KB * H];
  float *hin[NIMG], *hwt, *hbias, *hout;
  unsigned char* hmask;
  char *din[NIMG], *dout[NIMG], *dmask[NIMG], *dwt, *dbias;
  void *d_blk, *d_seg, *d_ao, *d_bo, *d_co, *d_do, *d_mo, *d_ws;
  const size_t nslices = (size_t)KB * H * CB;
  size_t i, s, j, nprod, ws_bytes, border = 0;
  int kb, cb, h, w, r, t, ci, ko, img, ok = 1;
  double worst = 0.0;
  if (libxsmm_hip_device_count() <= 0) { printf("no HIP device\n"); return 2; }
  kernel = libxsmm_dispatch_brgemm_ext(shape, LIBXSMM_GEMM_FLAG_BETA_0, LIBXSMM_GEMM_PREFETCH_NONE, brcfg, argops, postops);
  if (NULL == kernel) { fprintf(stderr, "dispatch returned NULL\n"); return 3; }
  /* the lists: block (kb, h) owns one slice per cb; a slice walks the tap rows r with 0 <= h + r - 1 < H and the tap columns t; byte offsets from the start of
   * each buffer */
  blk_ptr[0] = 0; seg_ptr[0] = 0;
  for (kb = 0, s = 0, j = 0; kb < KB; ++kb) for (h = 0; h < H; ++h, ++s) {
    for (cb = 0; cb < CB; ++cb, ++j) {
      size_t at = (size_t)seg_ptr[j];
      for (r = 0; r < 3; ++r) {
        if (h + r - 1 < 0 || h + r - 1 >= H) continue;           /* no such input row: the tap is not there */
        for (t = 0; t < 3; ++t, ++at) {
          a_offs[at] = (long long)(sizeof(float) * BC * BK * (size_t)(((kb * CB + cb) * 3 + r) * 3 + t));
          b_offs[at] = (long long)(sizeof(float) * BC * (size_t)((cb * H + h + r - 1) * WP + t));    /* pixel w reads padded column w + t */
        }
      }
      seg_ptr[j + 1] = at;
    }
    blk_ptr[s + 1] = j;
    if (seg_ptr[j] - seg_ptr[j - CB] == (unsigned long long)CB * 6) ++border;
    c_offs[s] = (long long)(sizeof(float) * BK * W * s);
    d_offs[s] = (long long)(sizeof(float) * BK * (size_t)kb);    /* one bias vector per output-channel block, repeated over its H rows */
    mask_offs[s] = (long long)(mask_blk * s);
  }
  nprod = (size_t)seg_ptr[nslices];
  ws_bytes = libxsmm_hip_gemm_ext_batch_reduce_segments_sliced_workspace(kernel, nslices);
  if (ws_bytes == 0) { fprintf(stderr, "workspace query failed: %s\n", libxsmm_hip_get_last_error_string()); return 1; }
  hwt = (float*)malloc(sizeof(float) * wt_elems); hbias = (float*)malloc(sizeof(float) * KB * BK); hout = (float*)malloc(sizeof(float) * out_elems);
  hmask = (unsigned char*)malloc(mask_bytes);
  dwt = (char*)libxsmm_hip_malloc(sizeof(float) * wt_elems); dbias = (char*)libxsmm_hip_malloc(sizeof(float) * KB * BK);
  d_blk = libxsmm_hip_malloc(sizeof(blk_ptr)); d_ws = libxsmm_hip_malloc(ws_bytes);
  d_seg = libxsmm_hip_malloc(sizeof(seg_ptr)); d_ao = libxsmm_hip_malloc(sizeof(long long) * nprod); d_bo = libxsmm_hip_malloc(sizeof(long long) * nprod);
  d_co = libxsmm_hip_malloc(sizeof(c_offs)); d_do = libxsmm_hip_malloc(sizeof(d_offs)); d_mo = libxsmm_hip_malloc(sizeof(mask_offs));
  if (!hwt || !hbias || !hout || !hmask || !dwt || !dbias || !d_blk || !d_ws || !d_seg || !d_ao || !d_bo || !d_co || !d_do || !d_mo) return 3;
  libxsmm_rng_set_seed(4242);
  for (i = 0; i < wt_elems; ++i) hwt[i] = frand();
  for (i = 0; i < (size_t)KB * BK; ++i) hbias[i] = frand();
  for (img = 0; img < NIMG; ++img) {
    hin[img] = (float*)calloc(in_elems, sizeof(float));
    din[img] = (char*)libxsmm_hip_malloc(sizeof(float) * in_elems); dout[img] = (char*)libxsmm_hip_malloc(sizeof(float) * out_elems); dmask[img] = (char*)libxsmm_hip_malloc(mask_bytes);
    if (!hin[img] || !din[img] || !dout[img] || !dmask[img]) return 3;
    for (cb = 0; cb < CB; ++cb) for (h = 0; h < H; ++h) for (w = 1; w <= W; ++w) for (ci = 0; ci < BC; ++ci)      /* columns 0 and W + 1 stay zero: the padding */
      hin[img][(((size_t)cb * H + h) * WP + w) * BC + ci] = frand();
    memset(hmask, 0, mask_bytes);
    if (libxsmm_hip_memcpy_h2d(din[img], hin[img], sizeof(float) * in_elems) != 0 || libxsmm_hip_memcpy_h2d(dmask[img], hmask, mask_bytes) != 0) return 3;
  }
  if (libxsmm_hip_memcpy_h2d(dwt, hwt, sizeof(float) * wt_elems) != 0 || libxsmm_hip_memcpy_h2d(dbias, hbias, sizeof(float) * KB * BK) != 0
    || libxsmm_hip_memcpy_h2d(d_blk, blk_ptr, sizeof(blk_ptr)) != 0 || libxsmm_hip_memcpy_h2d(d_seg, seg_ptr, sizeof(seg_ptr)) != 0 || libxsmm_hip_memcpy_h2d(d_ao, a_offs, sizeof(long long) * nprod) != 0
    || libxsmm_hip_memcpy_h2d(d_bo, b_offs, sizeof(long long) * nprod) != 0 || libxsmm_hip_memcpy_h2d(d_co, c_offs, sizeof(c_offs)) != 0
    || libxsmm_hip_memcpy_h2d(d_do, d_offs, sizeof(d_offs)) != 0 || libxsmm_hip_memcpy_h2d(d_mo, mask_offs, sizeof(mask_offs)) != 0) return 3;
  printf("conv 3 x 3: %d x %d pixels, %d -> %d channels in blocks of %d / %d; %zu blocks, %zu slices, %zu products (%zu border rows with %d of %d), workspace %zu bytes\n",
    H, W, CB * BC, KB * BK, BC, BK, nseg, nslices, nprod, border, CB * 6, CB * 9, ws_bytes);
  for (img = 0; img < NIMG; ++img) {
    double err = 0.0, ref = 0.0;
    size_t badbits = 0;
    /* the same seven lists and the same workspace for every image: only the bases move (a: the weights, d: the biases stay) */
    memset(&param, 0, sizeof(param));
    param.a.primary = dwt; param.b.primary = din[img]; param.c.primary = dout[img]; param.d.primary = dbias; param.c.secondary = dmask[img];
    (void)libxsmm_hip_launch_count(1);
    libxsmm_hip_gemm_ext_batch_reduce_segments_offsets_sliced(kernel, &param, nseg, (const unsigned long long*)d_blk, nslices, (const unsigned long long*)d_seg,
      (const long long*)d_ao, (const long long*)d_bo, (const long long*)d_co, (const long long*)d_do, (const long long*)d_mo, d_ws, ws_bytes);
    if (libxsmm_hip_get_last_error() != 0) { fprintf(stderr, "sliced segments call failed: %s\n", libxsmm_hip_get_last_error_string()); return 1; }
    launches = libxsmm_hip_launch_count(0);
    if (libxsmm_hip_memcpy_d2h(hout, dout[img], sizeof(float) * out_elems) != 0 || libxsmm_hip_memcpy_d2h(hmask, dmask[img], mask_bytes) != 0) return 3;
    /* the direct convolution: output channel block, row, pixel, channel; input channel block, tap row, tap column, input channel */
    for (kb = 0; kb < KB; ++kb) for (h = 0; h < H; ++h) for (w = 0; w < W; ++w) for (ko = 0; ko < BK; ++ko) {
      const size_t seg = (size_t)kb * H + h, o = (seg * W + w) * BK + ko;
      double gold = hbias[kb * BK + ko];
      int bit;
      for (cb = 0; cb < CB; ++cb) for (r = 0; r < 3; ++r) for (t = 0; t < 3; ++t) for (ci = 0; ci < BC; ++ci) {
        const int hi = h + r - 1;
        if (hi < 0 || hi >= H) continue;
        gold += (double)hwt[((size_t)(((kb * CB + cb) * 3 + r) * 3 + t) * BC + ci) * BK + ko] * hin[img][(((size_t)cb * H + hi) * WP + w + t) * BC + ci];
      }
      bit = (hmask[seg * mask_blk + (size_t)w * (mask_blk / W) + ko / 8] >> (ko % 8)) & 1;
      if (bit != (gold > 0.0)) ++badbits;
      if (gold < 0.0) gold = 0.0;
      err += (hout[o] - gold) * (hout[o] - gold); ref += gold * gold;
    }
    err = sqrt(err / (ref > 0 ? ref : 1));
    printf("image %d, bias + ReLU + bitmask, one call, %llu launches (%s, then the blocks' sums): normf_rel = %.3g, %zu mask bits differ\n", img, launches,
      libxsmm_hip_kernel_name((const void*)kernel, 1), err, badbits);
    if (err > worst) worst = err;
    if (badbits != 0 || launches != 2) ok = 0;
  }
  for (img = 0; img < NIMG; ++img) { free(hin[img]); libxsmm_hip_free(din[img]); libxsmm_hip_free(dout[img]); libxsmm_hip_free(dmask[img]); }
  free(hwt); free(hbias); free(hout); free(hmask);
  libxsmm_hip_free(dwt); libxsmm_hip_free(dbias); libxsmm_hip_free(d_blk); libxsmm_hip_free(d_ws); libxsmm_hip_free(d_seg); libxsmm_hip_free(d_ao); libxsmm_hip_free(d_bo); libxsmm_hip_free(d_co); libxsmm_hip_free(d_do); libxsmm_hip_free(d_mo);
  return (ok && worst < 1e-5) ? 0 : 1;
}
