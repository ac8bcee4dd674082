// gemm_lean_kernels.hip -- the lean f32 streaming kernel (the headline workload: f32 32^3, one 1-D batch of thousands of problems, streamed from HBM) and its
// launcher.  A translation unit of its own because it is compiled with kernel-argument preloading (csrc/Makefile: LEAN_FLAGS), which must not reach the
// other kernels: their by-value argument blocks get nothing from it.
#include "gemm_device.hpp"
#include "gemm_tile.hpp"

namespace xamd {

// ------------------------------------------------------------------------------------------------
// The same algorithm as gemm_f32_stream_kernel for the case the headline benchmark is: a 1-D batch of independent 32x32x(32 br kchunks) problems with 16-byte
// aligned strided operands, beta = 0 and no fused epilogue.  A launch of 4096 such problems is ONE round of waves that lasts ~10 us, so the time every wave
// spends before its first load is issued is on the critical path of the whole launch.  The general kernel reads a 280-byte argument block in several dependent
// scalar loads, divides by the tile count and walks the batch / batch-reduce / epilogue options; this one has no option left to test, and in its single-chunk
// form (br = 1, k = 32) has no loop either.
// Arguments: separate scalar / pointer parameters, not a by-value struct, so that the compiler can PRELOAD them: with -amdgpu-kernarg-preload-count the
// dispatch writes the first kernarg dwords into user SGPRs and the first operand load does not wait for a scalar load of the argument block.  Of the 16 user
// SGPRs two hold the kernarg segment pointer; everything the single-chunk form reads -- a, b, c, the three batch strides, nbatch, lda, ldb, ldc -- is the
// first 13 dwords when the batch strides are 32-bit (S = unsigned int: the launcher's choice whenever they fit).  S = long long (batch strides of 4 GiB and
// more, or negative) preloads the pointers, the strides, nbatch and lda and reads ldb / ldc from memory.  The chunked form's fields come after them.
// NTL: non-temporal operand loads.  Measured (tools/headline_probe.hip, profiles/r02_copy_floor.csv): with operands coming from HBM they save 0.5 us of a
// 9.9 us launch (they do not displace the Infinity Cache's contents), but operands that ARE resident in the 256 MiB Infinity Cache -- the normal case for a
// 48 MiB batch produced by the previous kernel -- are then not kept there: 8.7 instead of 5.8 us.  The launcher therefore asks for them only when one launch
// moves more than the Infinity Cache holds (they cannot be resident then).
// ------------------------------------------------------------------------------------------------
// 16-byte operand load through a wave-uniform buffer resource with gfx950 cache-policy bits (aux: 1 = sc0, 2 = nt, 16 = sc1)
template <int AUX> __device__ __forceinline__ f32x4 ld16_pol(__amdgpu_buffer_rsrc_t r, unsigned int voffset) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voffset, 0, AUX));
}
// Cache policy of the streaming case (POL 3): operand loads `nt` (aux 2), C stores `sc1` (aux 16).  Measured on the kernel itself, headline leg of bench.py,
// three alternating rounds (profiles/r07_lean_policy_ab.txt): nt stores 9.83 us, sc1 9.35, sc0 sc1 9.34; sc0 nt loads (aux 3) instead of nt: 9.34 with sc1
// stores, 9.85 with nt stores -- no difference, so the loads stay nt.  An nt store keeps the line in the XCD's L2, which the next dependent launch pays for at its
// boundary (16 MiB of C per launch); an sc1 store does not keep the line there.  The copy of this footprint shows the same (profiles/r07_policy_floor.txt: nt loads,
// nt stores 8.78 us; nt loads, sc1 stores 8.36).  Compile-time switches for A/B builds (tools/build_variant.sh: pass the Makefile's LEAN_FLAGS with them).
#ifndef XAMD_LEAN_LD_AUX
#define XAMD_LEAN_LD_AUX 2
#endif
#ifndef XAMD_LEAN_ST_AUX
#define XAMD_LEAN_ST_AUX 16
#endif
// POL 0: operands loaded `sc0 sc1`, C leaves as whole 16-byte pieces through the wave's LDS image, non-temporal.  Measured on the headline
//        footprint (tools/policy_probe.hip, profiles/r02_cache_policy.txt): against plain loads + dword nt stores 9.95 vs 10.88 us with the
//        operands in HBM AND 6.25 vs 6.7 us with the operands resident in the Infinity Cache -- no trade-off, so it is the default.
// POL 1: operands loaded `nt`, C as dword nt stores: 9.65 us from HBM but 8.4 us on resident operands (an nt read is not kept in the
//        Infinity Cache): only for launches that move more than the Infinity Cache holds, whose operands cannot be resident anyway.
// POL 2: plain loads, dword nt stores (C not 16-byte aligned).
// POL 3 (round 4): POL 1's nt loads with POL 0's 16-byte stores through the LDS image -- tools/headline_probe: a copy of this footprint with nt loads and
//        16-byte nt stores takes 8.99 us where the POL 1 kernel takes 9.99 (dword stores: four times the store instructions).  The stores are sc1, not nt
//        (above).  POL 0 keeps its nt stores: with cacheable operands the sc1 form is slower from HBM (tools/policy_probe gemm mode: 10.84 vs 9.85 us).
// The kernel's body: the launch whose problem bases are pa / pb / pc (the whole kernel of a single launch; one blockIdx.y slice of a fused one, below)
template <bool TA, bool TB, bool SINGLE, int POL, typename S>
__device__ __forceinline__ void lean_launch_body(const char* pa, const char* pb, char* pc, S bs_a, S bs_b, S bs_c, unsigned int nbatch,
                                                 unsigned int lda, unsigned int ldb, unsigned int ldc,
                                                 unsigned int nchunks, unsigned int kchunks, long long brs_a, long long brs_b) {
  constexpr int AUX = POL == 0 ? 17 : (POL == 1 ? 2 : (POL == 3 ? XAMD_LEAN_LD_AUX : 0));
  constexpr int ST_AUX = POL == 3 ? XAMD_LEAN_ST_AUX : 2;
  __shared__ __attribute__((aligned(16))) float lds_all[4][2048];
  const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned int bidx = blockIdx.x * 4u + wave;
  if (bidx >= nbatch) return;
  const unsigned int lane = threadIdx.x & 63u, li = lane & 31u, h = lane >> 5;
  float* lds = lds_all[wave];
  gcptr ar = (gcptr)pa + (long long)bidx * (long long)bs_a, br = (gcptr)pb + (long long)bidx * (long long)bs_b;
  const unsigned int offA = ((lane >> 3) * lda + (lane & 7u) * 4u) * 4u;
  const unsigned int offB = ((lane >> 3) * ldb + (lane & 7u) * 4u) * 4u;
  const unsigned int stepA = 32u * lda, stepB = 32u * ldb;          // bytes per 8 rows
  f32x4 ga[4], gb[4];
  {
    const __amdgpu_buffer_rsrc_t ra = wave_rsrc(ar), rb = wave_rsrc(br);
#pragma unroll
    for (int x = 0; x < 4; ++x) ga[x] = ld16_pol<AUX>(ra, x * stepA + offA);
#pragma unroll
    for (int x = 0; x < 4; ++x) gb[x] = ld16_pol<AUX>(rb, x * stepB + offB);
  }
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  if (SINGLE) {
    float af[16], bf[16];
    tile_to_frag<TA>(af, ga, lds, (int)lane);
    tile_to_frag<!TB>(bf, gb, lds + 1024, (int)lane);
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[s], af[s], acc, 0, 0, 0);
  } else {
    const unsigned long long kstepA = TA ? 128ull : 128ull * lda, kstepB = TB ? 128ull * ldb : 128ull;
    unsigned int kc = 0;
    for (unsigned int t = 0; t < nchunks; ++t) {
      float af[16], bf[16];
      tile_to_frag<TA>(af, ga, lds, (int)lane);
      tile_to_frag<!TB>(bf, gb, lds + 1024, (int)lane);
      if (++kc == kchunks) { kc = 0; ar += brs_a; br += brs_b; }
      if (t + 1 < nchunks) {        // chunk t+1 is in flight while the matrix core works on chunk t
        const __amdgpu_buffer_rsrc_t ra = wave_rsrc(ar + kc * kstepA), rb = wave_rsrc(br + kc * kstepB);
#pragma unroll
        for (int x = 0; x < 4; ++x) ga[x] = ld16_pol<AUX>(ra, x * stepA + offA);
#pragma unroll
        for (int x = 0; x < 4; ++x) gb[x] = ld16_pol<AUX>(rb, x * stepB + offB);
      }
#pragma unroll
      for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[s], af[s], acc, 0, 0, 0);
    }
  }
  gptr ctile = (gptr)pc + (long long)bidx * (long long)bs_c;
  if (POL == 0 || POL == 3) {
    // C tile -> column-major LDS image (lanes along i: conflict free) -> whole 128-byte columns, 16 bytes per lane
#pragma unroll
    for (int r2 = 0; r2 < 16; ++r2) lds[li + (unsigned int)jl_of(r2, (int)h) * 32u] = acc[r2];
    const __amdgpu_buffer_rsrc_t rc = wave_rsrc((gcptr)ctile);
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const unsigned int L = lane + 64u * x;
      __builtin_amdgcn_raw_buffer_store_b128(((const u32x4*)lds)[L], rc, (int)(((L >> 3) * ldc + (L & 7u) * 4u) * 4u), 0, ST_AUX);
    }
  } else {
    const unsigned int offC = (4u * h * ldc + li) * 4u;
#pragma unroll
    for (int r2 = 0; r2 < 16; ++r2)
      st_stream((GM float*)(ctile + (unsigned long long)(((r2 & 3) + 8 * (r2 >> 2)) * ldc) * 4ull + offC), acc[r2]);
  }
}

template <bool TA, bool TB, bool SINGLE, int POL, typename S>
__global__ __launch_bounds__(256) void gemm_f32_stream_kernel_lean(const char* pa, const char* pb, char* pc, S bs_a, S bs_b, S bs_c, unsigned int nbatch,
                                                                   unsigned int lda, unsigned int ldb, unsigned int ldc,
                                                                   unsigned int nchunks, unsigned int kchunks, long long brs_a, long long brs_b) {
  lean_launch_body<TA, TB, SINGLE, POL, S>(pa, pb, pc, bs_a, bs_b, bs_c, nbatch, lda, ldb, ldc, nchunks, kchunks, brs_a, brs_b);
}

// ------------------------------------------------------------------------------------------------
// Several EQUAL launches in one grid (capture-time fusion): launches that differ in their three bases only, folded into one graph node
// while the graph is built.  Grid (ceil(nbatch / 4), G): blockIdx.y selects the launch, everything else is the kernel above -- the same function, so the
// results are bit for bit those of G separate launches; what goes is G - 1 dependent kernel boundaries and G - 1 fills and drains of the chip.
// Arguments: the scalars first, so that the dispatch still preloads them (the three 32-bit batch strides, nbatch, lda, ldb, ldc, the chunk fields: 14
// dwords); the table of bases travels by value behind them and one entry is read with uniform scalar loads indexed by blockIdx.y (no scratch).  32-bit strides and
// 16-byte aligned C (POL 0 and 3) only: everything else stays unfused.
// ------------------------------------------------------------------------------------------------
struct LeanMultiTable { FuseEntry e[kFuseCap]; };
static_assert(sizeof(FuseEntry) == 32, "table entries are 32 bytes apart");
template <bool TA, bool TB, bool SINGLE, int POL>
__global__ __launch_bounds__(256) void gemm_f32_lean_multi_kernel(unsigned int bs_a, unsigned int bs_b, unsigned int bs_c, unsigned int nbatch,
                                                                  unsigned int lda, unsigned int ldb, unsigned int ldc, unsigned int nchunks, unsigned int kchunks,
                                                                  long long brs_a, long long brs_b, const LeanMultiTable table) {
  const FuseEntry e = table.e[blockIdx.y];
  lean_launch_body<TA, TB, SINGLE, POL, unsigned int>((const char*)e.a, (const char*)e.b, (char*)e.c, bs_a, bs_b, bs_c, nbatch, lda, ldb, ldc, nchunks, kchunks, brs_a, brs_b);
}

template <bool TA, bool TB, bool SINGLE> static const void* lean_multi_pol(int pol) {
  return pol == 0 ? (const void*)gemm_f32_lean_multi_kernel<TA, TB, SINGLE, 0> : (const void*)gemm_f32_lean_multi_kernel<TA, TB, SINGLE, 3>;
}
template <bool TA, bool TB> static const void* lean_multi_single(bool single, int pol) { return single ? lean_multi_pol<TA, TB, true>(pol) : lean_multi_pol<TA, TB, false>(pol); }
static const void* lean_multi_function(bool ta, bool tb, bool single, int pol) {
  return !ta ? (!tb ? lean_multi_single<false, false>(single, pol) : lean_multi_single<false, true>(single, pol))
             : (!tb ? lean_multi_single<true, false>(single, pol) : lean_multi_single<true, true>(single, pol));
}

// The capture state of `st` as the fusion needs it: true when the stream is being captured and everything issued to it so far ends in exactly ONE node.
// (The dependency array belongs to the runtime and is valid until the next HIP call only: the one node is copied out here.)
static bool lean_capture_tail(hipStream_t st, unsigned long long* id, hipGraphNode_t* node, bool* capturing) {
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  const hipGraphNode_t* deps = nullptr;
  size_t ndeps = 0;
  hipGraph_t graph = nullptr;
  *capturing = false;
  const hipError_t e = hipStreamGetCaptureInfo_v2(st, &status, id, &graph, &deps, &ndeps);
  if (e != hipSuccess) { (void)hipGetLastError(); return false; }
  if (status != hipStreamCaptureStatusActive) return false;
  *capturing = true;
  if (ndeps != 1 || deps == nullptr) return false;
  *node = deps[0];
  return true;
}

// pol: 0..3 as above (chosen by launch_gemm); the operands are 16-byte aligned exact 32 x 32 tiles (f32_lean_ok)
int launch_gemm_f32_lean(const GemmArgs& a, int pol, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned int)((a.nbatch + 3u) / 4u));
  const bool ta = a.flags & LIBXSMM_GEMM_FLAG_TRANS_A, tb = a.flags & LIBXSMM_GEMM_FLAG_TRANS_B;
  const long long brs_a = a.br_mode == 3 ? a.br_stride_a : 0, brs_b = a.br_mode == 3 ? a.br_stride_b : 0;
  const unsigned int kchunks = (unsigned int)a.k >> 5, nchunks = (unsigned int)a.br_count * kchunks;
  const unsigned int nbatch = (unsigned int)a.nbatch, lda = (unsigned int)a.lda, ldb = (unsigned int)a.ldb, ldc = (unsigned int)a.ldc;
  auto fits32 = [](long long s) { return s >= 0 && s < (1ll << 32); };
  const bool narrow = fits32(a.bs_a) && fits32(a.bs_b) && fits32(a.bs_c);
  // ---- capture-time fusion: on a stream that is being captured, a launch that equals the one before it apart from its bases and is address-independent of
  // every launch in that one's graph node joins the node instead of becoming a node of its own (rules: DESIGN.md section 5c, include/libxsmm_hip.h)
  FuseState& f = tls().fuse;
  const int limit = f.handle ? capture_fusion_limit() : 0;
  // never asked of the NULL stream: it cannot be captured, and the query would invalidate another stream's global-mode capture
  bool candidate = limit >= 2 && st != nullptr && narrow && (pol == 0 || pol == 3) && tls().pipe_lanes <= 1 && brs_a >= 0 && brs_b >= 0;
  FuseKey key; FuseEntry entry{a.a, a.b, a.c, 0ull}; FuseLaunch range;
  unsigned long long capture_id = 0;
  if (candidate) {
    size_t ea = 0, eb = 0, ec = 0;
    key.handle = f.handle; key.bs_a = (unsigned int)a.bs_a; key.bs_b = (unsigned int)a.bs_b; key.bs_c = (unsigned int)a.bs_c; key.nbatch = nbatch;
    key.lda = lda; key.ldb = ldb; key.ldc = ldc; key.nchunks = nchunks; key.kchunks = kchunks; key.brs_a = brs_a; key.brs_b = brs_b; key.pol = pol; key.ta = ta; key.tb = tb;
    candidate = fuse_extent(a.br_count, brs_a, lda, (unsigned long long)(ta ? a.m : a.k), 4, &ea) && fuse_extent(a.br_count, brs_b, ldb, (unsigned long long)(tb ? a.k : a.n), 4, &eb) &&
                fuse_extent(1, 0, ldc, (unsigned long long)a.n, 4, &ec) && fuse_range((uintptr_t)a.a, nbatch, a.bs_a, ea, &range.a) &&
                fuse_range((uintptr_t)a.b, nbatch, a.bs_b, eb, &range.b) && fuse_range((uintptr_t)a.c, nbatch, a.bs_c, ec, &range.c);
  }
  if (candidate) {
    hipGraphNode_t tail = nullptr;
    bool capturing = false;
    const bool one_tail = lean_capture_tail(st, &capture_id, &tail, &capturing);
    if (!capturing) { candidate = false; f.n = 0; }
    else if (one_tail && f.n > 0 && f.n < limit && f.n < kFuseCap && f.capture_id == capture_id && f.stream == (void*)st && f.node == (void*)tail && f.key == key &&
             fuse_independent(range, f.range, f.n)) {
      LeanMultiTable table{};
      for (int i = 0; i < f.n; ++i) table.e[i] = f.entry[i];
      table.e[f.n] = entry;
      unsigned int bs[3] = {key.bs_a, key.bs_b, key.bs_c}, nb = nbatch, ld[3] = {lda, ldb, ldc}, nch = nchunks, kch = kchunks;
      long long brs[2] = {brs_a, brs_b};
      void* params[12] = {&bs[0], &bs[1], &bs[2], &nb, &ld[0], &ld[1], &ld[2], &nch, &kch, &brs[0], &brs[1], &table};
      hipKernelNodeParams np{};
      np.func = const_cast<void*>(lean_multi_function(ta, tb, nchunks == 1, pol));
      np.gridDim = dim3(grid.x, (unsigned int)(f.n + 1), 1); np.blockDim = dim3(256, 1, 1);
      np.sharedMemBytes = 0; np.kernelParams = params; np.extra = nullptr;
      const hipError_t e = hipGraphKernelNodeSetParams(tail, &np);
      if (e == hipSuccess) {
        f.entry[f.n] = entry; f.range[f.n] = range; ++f.n; ++f.folded;
        return 0;
      }
      (void)hipGetLastError();
      f.n = 0; candidate = false;
      capture_fusion_disable(hipGetErrorString(e));          // no other way is tried: the launch leaves on its own below
    }
  }
#define LEAN_ARGS_(S_) (const char*)a.a, (const char*)a.b, (char*)a.c, (S_)a.bs_a, (S_)a.bs_b, (S_)a.bs_c, nbatch, lda, ldb, ldc, nchunks, kchunks, brs_a, brs_b
#define LAUNCH_LEAN__(TA_, TB_, S_, P_) do { if (narrow) hipLaunchKernelGGL((gemm_f32_stream_kernel_lean<TA_, TB_, S_, P_, unsigned int>), grid, dim3(256), 0, st, LEAN_ARGS_(unsigned int)); \
                                             else hipLaunchKernelGGL((gemm_f32_stream_kernel_lean<TA_, TB_, S_, P_, long long>), grid, dim3(256), 0, st, LEAN_ARGS_(long long)); } while (0)
#define LAUNCH_LEAN_S_(TA_, TB_, S_) do { if (pol == 0) LAUNCH_LEAN__(TA_, TB_, S_, 0); else if (pol == 1) LAUNCH_LEAN__(TA_, TB_, S_, 1); else if (pol == 3) LAUNCH_LEAN__(TA_, TB_, S_, 3); else LAUNCH_LEAN__(TA_, TB_, S_, 2); } while (0)
#define LAUNCH_LEAN_(TA_, TB_) do { if (nchunks == 1) LAUNCH_LEAN_S_(TA_, TB_, true); else LAUNCH_LEAN_S_(TA_, TB_, false); } while (0)
  if (!ta && !tb) LAUNCH_LEAN_(false, false); else if (ta && !tb) LAUNCH_LEAN_(true, false); else if (!ta && tb) LAUNCH_LEAN_(false, true); else LAUNCH_LEAN_(true, true);
#undef LAUNCH_LEAN_
#undef LAUNCH_LEAN_S_
#undef LAUNCH_LEAN__
#undef LEAN_ARGS_
  const int err = (int)hipGetLastError();
  if (candidate) {          // captured as a node of its own: the node the next equal, independent launch may join
    hipGraphNode_t tail = nullptr;
    bool capturing = false;
    unsigned long long id_now = 0;
    f.n = 0;
    if (err == 0 && lean_capture_tail(st, &id_now, &tail, &capturing) && id_now == capture_id) {
      f.n = 1; f.capture_id = capture_id; f.stream = (void*)st; f.node = (void*)tail; f.key = key; f.entry[0] = entry; f.range[0] = range;
    }
  }
  return err;
}

}  // namespace xamd
