/* grouped_driver.c -- three GEMM shapes as ONE libxsmm_hip_gemm_batch_grouped call, checked against the host loop it replaces.
 * The caller of the reference runs such a mix as several handles inside its own OpenMP loop (samples/xgemm/gemm_kernel.c:4063-4066); here every shape is a
 * group: its handle, the param struct of its first problem, a problem count and byte strides.  Operands live in device memory (libxsmm_hip_malloc).
 *
 *   grouped_driver      exit 0 if every problem of every group matches the gold loop (normf_rel < 1e-5); 2 without a device
 */
#include <libxsmm.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NGROUPS 3

static float frand(void) { return (float)((int)(libxsmm_rng_f64() * 10.0) - 5) / 10.0f; }   /* multiples of 0.1 */

int main(void) {
  const int M[NGROUPS] = {16, 23, 40}, N[NGROUPS] = {16, 23, 24}, K[NGROUPS] = {16, 23, 32};
  const size_t count[NGROUPS] = {256, 128, 64};
  libxsmm_hip_gemm_group groups[NGROUPS];
  float *ha[NGROUPS], *hb[NGROUPS], *hc[NGROUPS];
  void *da[NGROUPS], *db[NGROUPS], *dc[NGROUPS];
  double err = 0.0, ref = 0.0;
  int g, status = 0;
  if (libxsmm_hip_device_count() <= 0) { printf("no HIP device\n"); return 2; }
  libxsmm_rng_set_seed(555);
  for (g = 0; g < NGROUPS; ++g) {
    const size_t na = (size_t)M[g] * K[g], nb = (size_t)K[g] * N[g], nc = (size_t)M[g] * N[g];
    const libxsmm_gemm_shape shape = libxsmm_create_gemm_shape(M[g], N[g], K[g], M[g], K[g], M[g],
      LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32);
    const libxsmm_gemmfunction kernel = libxsmm_dispatch_gemm(shape, LIBXSMM_GEMM_FLAG_BETA_0, LIBXSMM_GEMM_PREFETCH_NONE);
    size_t i;
    if (NULL == kernel) { fprintf(stderr, "dispatch returned NULL\n"); return 3; }
    ha[g] = (float*)malloc(sizeof(float) * na * count[g]);
    hb[g] = (float*)malloc(sizeof(float) * nb * count[g]);
    hc[g] = (float*)malloc(sizeof(float) * nc * count[g]);
    da[g] = libxsmm_hip_malloc(sizeof(float) * na * count[g]);
    db[g] = libxsmm_hip_malloc(sizeof(float) * nb * count[g]);
    dc[g] = libxsmm_hip_malloc(sizeof(float) * nc * count[g]);
    if (!ha[g] || !hb[g] || !hc[g] || !da[g] || !db[g] || !dc[g]) return 3;
    for (i = 0; i < na * count[g]; ++i) ha[g][i] = frand();
    for (i = 0; i < nb * count[g]; ++i) hb[g][i] = frand();
    if (libxsmm_hip_memcpy_h2d(da[g], ha[g], sizeof(float) * na * count[g]) != 0 || libxsmm_hip_memcpy_h2d(db[g], hb[g], sizeof(float) * nb * count[g]) != 0) return 3;
    memset(&groups[g], 0, sizeof(groups[g]));
    groups[g].kernel = kernel;
    groups[g].param.a.primary = da[g]; groups[g].param.b.primary = db[g]; groups[g].param.c.primary = dc[g];
    groups[g].count = count[g];
    groups[g].stride_a = (long long)(sizeof(float) * na); groups[g].stride_b = (long long)(sizeof(float) * nb); groups[g].stride_c = (long long)(sizeof(float) * nc);
  }
  libxsmm_hip_gemm_batch_grouped(groups, NGROUPS);        /* blocking thread: every group is done on return */
  if (libxsmm_hip_get_last_error() != 0) { fprintf(stderr, "grouped call failed: %s\n", libxsmm_hip_get_last_error_string()); return 1; }
  for (g = 0; g < NGROUPS; ++g) {
    const size_t na = (size_t)M[g] * K[g], nb = (size_t)K[g] * N[g], nc = (size_t)M[g] * N[g];
    size_t e;
    int i, j, s;
    if (libxsmm_hip_memcpy_d2h(hc[g], dc[g], sizeof(float) * nc * count[g]) != 0) return 3;
    for (e = 0; e < count[g]; ++e) {                       /* the loop the grouped call replaces */
      const float *a = ha[g] + e * na, *b = hb[g] + e * nb, *c = hc[g] + e * nc;
      for (j = 0; j < N[g]; ++j) for (i = 0; i < M[g]; ++i) {
        double gold = 0.0;
        for (s = 0; s < K[g]; ++s) gold += (double)a[i + s * M[g]] * b[s + j * K[g]];
        err += (c[i + j * M[g]] - gold) * (c[i + j * M[g]] - gold); ref += gold * gold;
      }
    }
    printf("group %d: %d x %d x %d, %zu problems\n", g, M[g], N[g], K[g], count[g]);
    free(ha[g]); free(hb[g]); free(hc[g]); libxsmm_hip_free(da[g]); libxsmm_hip_free(db[g]); libxsmm_hip_free(dc[g]);
  }
  err = sqrt(err / (ref > 0 ? ref : 1));
  printf("grouped call of %d shapes: normf_rel = %.3g\n", NGROUPS, err);
  if (err >= 1e-5) status = 1;
  return status;
}
