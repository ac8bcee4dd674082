/* grouped_fused_driver.c -- a layer of three GEMM shapes, each followed by its bias, ReLU and ReLU bitmask (the reference's fused BRGEMM call,
 * src/generator_gemm_reference_impl.c:294-372), as ONE libxsmm_hip_gemm_ext_batch_grouped call; then the same list as a group plan whose launch is captured
 * into a HIP graph and replayed.  Every result is checked against the host loop the call replaces.  Operands live in device memory (libxsmm_hip_malloc).
 *
 *   grouped_fused_driver      exit 0 if the call and both replays match the gold loop (normf_rel < 1e-5, mask bits where the sum is not near 0); 2 without a device
 */
#include <libxsmm.h>
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NGROUPS 3

static const int M[NGROUPS] = {16, 23, 40}, N[NGROUPS] = {16, 23, 24}, K[NGROUPS] = {16, 23, 32};
static const size_t count[NGROUPS] = {96, 64, 32};
static float *ha[NGROUPS], *hb[NGROUPS], *hd[NGROUPS], *hc[NGROUPS];
static unsigned char* hm[NGROUPS];
static void *da[NGROUPS], *db[NGROUPS], *dd[NGROUPS], *dc[NGROUPS], *dm[NGROUPS];

static float frand(void) { return (float)((int)(libxsmm_rng_f64() * 10.0) - 5) / 10.0f; }   /* multiples of 0.1 */
static size_t mask_bytes(int g) { return (size_t)((M[g] + 15) / 16 * 16 / 8) * (size_t)N[g]; }

/* C and masks of every group against the loop the grouped call replaces; returns normf_rel, *mask_errors = wrong mask bits */
static double check(int* mask_errors) {
  double err = 0.0, ref = 0.0;
  int g;
  *mask_errors = 0;
  for (g = 0; g < NGROUPS; ++g) {
    const size_t na = (size_t)M[g] * K[g], nb = (size_t)K[g] * N[g], nc = (size_t)M[g] * N[g], mb = mask_bytes(g);
    const int mld8 = (M[g] + 15) / 16 * 16 / 8;
    size_t e;
    int i, j, s;
    if (libxsmm_hip_memcpy_d2h(hc[g], dc[g], sizeof(float) * nc * count[g]) != 0 || libxsmm_hip_memcpy_d2h(hm[g], dm[g], mb * count[g]) != 0) return 1.0;
    for (e = 0; e < count[g]; ++e) {
      const float *a = ha[g] + e * na, *b = hb[g] + e * nb, *d = hd[g] + e * M[g], *c = hc[g] + e * nc;
      const unsigned char* mask = hm[g] + e * mb;
      for (j = 0; j < N[g]; ++j) for (i = 0; i < M[g]; ++i) {
        double sum = d[i], gold;
        const int bit = (mask[i / 8 + j * mld8] >> (i % 8)) & 1;
        for (s = 0; s < K[g]; ++s) sum += (double)a[i + s * M[g]] * b[s + j * K[g]];
        gold = sum > 0.0 ? sum : 0.0;
        err += (c[i + j * M[g]] - gold) * (c[i + j * M[g]] - gold); ref += gold * gold;
        if (fabs(sum) > 1e-4 && bit != (sum > 0.0 ? 1 : 0)) ++*mask_errors;
      }
    }
  }
  return sqrt(err / (ref > 0 ? ref : 1));
}

static int clear_outputs(void) {
  int g;
  for (g = 0; g < NGROUPS; ++g) {
    if (libxsmm_hip_memset(dc[g], 0xff, sizeof(float) * (size_t)M[g] * N[g] * count[g]) != 0 || libxsmm_hip_memset(dm[g], 0, mask_bytes(g) * count[g]) != 0) return 1;
  }
  return 0;
}

int main(void) {
  libxsmm_hip_gemm_ext_group groups[NGROUPS];
  libxsmm_hip_gemm_group_plan* plan;
  hipStream_t stream;
  hipGraph_t graph;
  hipGraphExec_t exec;
  double err;
  int g, bad, replay, status = 0;
  if (libxsmm_hip_device_count() <= 0) { printf("no HIP device\n"); return 2; }
  libxsmm_rng_set_seed(557);
  for (g = 0; g < NGROUPS; ++g) {
    const size_t na = (size_t)M[g] * K[g], nb = (size_t)K[g] * N[g], nc = (size_t)M[g] * N[g], mb = mask_bytes(g);
    const libxsmm_gemm_shape shape = libxsmm_create_gemm_shape(M[g], N[g], K[g], M[g], K[g], M[g],
      LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32, LIBXSMM_DATATYPE_F32);
    const libxsmm_gemm_batch_reduce_config brcfg = libxsmm_create_gemm_batch_reduce_config(LIBXSMM_GEMM_BATCH_REDUCE_NONE, 0, 0, 0);
    const libxsmm_gemm_ext_unary_argops argops = libxsmm_create_gemm_ext_unary_argops(0, LIBXSMM_MELTW_TYPE_UNARY_NONE, LIBXSMM_MELTW_FLAG_UNARY_NONE, 0,
      0, LIBXSMM_MELTW_TYPE_UNARY_NONE, LIBXSMM_MELTW_FLAG_UNARY_NONE, 0, M[g], LIBXSMM_MELTW_TYPE_UNARY_RELU, LIBXSMM_MELTW_FLAG_UNARY_BITMASK_2BYTEMULT, 0);
    const libxsmm_gemm_ext_binary_postops postops = libxsmm_create_gemm_ext_binary_postops(M[g], LIBXSMM_DATATYPE_F32, LIBXSMM_MELTW_TYPE_BINARY_ADD,
      LIBXSMM_MELTW_FLAG_BINARY_BCAST_COL_IN_0);
    const libxsmm_gemmfunction_ext kernel = libxsmm_dispatch_brgemm_ext(shape, LIBXSMM_GEMM_FLAG_BETA_0, LIBXSMM_GEMM_PREFETCH_NONE, brcfg, argops, postops);
    size_t i;
    if (NULL == kernel) { fprintf(stderr, "dispatch returned NULL\n"); return 3; }
    ha[g] = (float*)malloc(sizeof(float) * na * count[g]); hb[g] = (float*)malloc(sizeof(float) * nb * count[g]);
    hd[g] = (float*)malloc(sizeof(float) * M[g] * count[g]); hc[g] = (float*)malloc(sizeof(float) * nc * count[g]);
    hm[g] = (unsigned char*)malloc(mb * count[g]);
    da[g] = libxsmm_hip_malloc(sizeof(float) * na * count[g]); db[g] = libxsmm_hip_malloc(sizeof(float) * nb * count[g]);
    dd[g] = libxsmm_hip_malloc(sizeof(float) * M[g] * count[g]); dc[g] = libxsmm_hip_malloc(sizeof(float) * nc * count[g]);
    dm[g] = libxsmm_hip_malloc(mb * count[g]);
    if (!ha[g] || !hb[g] || !hd[g] || !hc[g] || !hm[g] || !da[g] || !db[g] || !dd[g] || !dc[g] || !dm[g]) return 3;
    for (i = 0; i < na * count[g]; ++i) ha[g][i] = frand();
    for (i = 0; i < nb * count[g]; ++i) hb[g][i] = frand();
    for (i = 0; i < (size_t)M[g] * count[g]; ++i) hd[g][i] = frand() + 0.05f;        /* (keeps the sums away from 0) */
    if (libxsmm_hip_memcpy_h2d(da[g], ha[g], sizeof(float) * na * count[g]) != 0 || libxsmm_hip_memcpy_h2d(db[g], hb[g], sizeof(float) * nb * count[g]) != 0 ||
        libxsmm_hip_memcpy_h2d(dd[g], hd[g], sizeof(float) * M[g] * count[g]) != 0) return 3;
    memset(&groups[g], 0, sizeof(groups[g]));
    groups[g].kernel = kernel;
    groups[g].param.a.primary = da[g]; groups[g].param.b.primary = db[g]; groups[g].param.c.primary = dc[g];
    groups[g].param.d.primary = dd[g];                     /* the bias of element 0 */
    groups[g].param.c.secondary = dm[g];                   /* the ReLU bitmask of element 0 */
    groups[g].count = count[g];
    groups[g].stride_a = (long long)(sizeof(float) * na); groups[g].stride_b = (long long)(sizeof(float) * nb); groups[g].stride_c = (long long)(sizeof(float) * nc);
    groups[g].stride_d = (long long)(sizeof(float) * M[g]); groups[g].stride_mask = (long long)mb;
  }
  /* 1. one call, blocking thread: every group is done on return */
  if (clear_outputs() != 0) return 3;
  libxsmm_hip_gemm_ext_batch_grouped(groups, NGROUPS);
  if (libxsmm_hip_get_last_error() != 0) { fprintf(stderr, "ext grouped call failed: %s\n", libxsmm_hip_get_last_error_string()); return 1; }
  err = check(&bad);
  printf("ext grouped call of %d shapes: normf_rel = %.3g, %d wrong mask bits\n", NGROUPS, err, bad);
  if (err >= 1e-5 || bad != 0) status = 1;
  /* 2. the same list as a plan: the tables are built once and stay on the device, so the launch can be captured; a replay reads the operands' current values */
  plan = libxsmm_hip_gemm_ext_group_plan_create(groups, NGROUPS);
  if (NULL == plan) { fprintf(stderr, "plan create failed: %s\n", libxsmm_hip_get_last_error_string()); return 1; }
  memset(groups, 0, sizeof(groups));                       /* the plan keeps what it needs */
  if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return 3;
  libxsmm_hip_set_stream(stream);                          /* stream-ordered from here on */
  if (hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return 3;
  libxsmm_hip_gemm_group_plan_launch(plan);
  if (hipStreamEndCapture(stream, &graph) != hipSuccess || libxsmm_hip_get_last_error() != 0) { fprintf(stderr, "capture failed: %s\n", libxsmm_hip_get_last_error_string()); return 1; }
  if (hipGraphInstantiate(&exec, graph, NULL, NULL, 0) != hipSuccess) return 3;
  for (replay = 0; replay < 2; ++replay) {
    if (clear_outputs() != 0) return 3;
    if (hipGraphLaunch(exec, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return 3;
    err = check(&bad);
    printf("replay %d of the captured plan (%d kernel launch(es)): normf_rel = %.3g, %d wrong mask bits\n", replay, libxsmm_hip_gemm_group_plan_launches(plan), err, bad);
    if (err >= 1e-5 || bad != 0) status = 1;
  }
  (void)hipGraphExecDestroy(exec); (void)hipGraphDestroy(graph);      /* before the plan: a graph that captured it must not be replayed after destroy */
  libxsmm_hip_gemm_group_plan_destroy(plan);
  libxsmm_hip_set_stream(NULL); libxsmm_hip_set_async(0);
  (void)hipStreamDestroy(stream);
  for (g = 0; g < NGROUPS; ++g) {
    free(ha[g]); free(hb[g]); free(hd[g]); free(hc[g]); free(hm[g]);
    libxsmm_hip_free(da[g]); libxsmm_hip_free(db[g]); libxsmm_hip_free(dd[g]); libxsmm_hip_free(dc[g]); libxsmm_hip_free(dm[g]);
  }
  return status;
}
