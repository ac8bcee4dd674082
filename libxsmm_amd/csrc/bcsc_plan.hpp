// bcsc_plan.hpp -- which BCSC kernel a call gets, and on what grid: host arithmetic on BcscArgs only (shapes, the residues of three pointers, what the host knows of
// the pattern).  No HIP type and no HIP call: launch_bcsc (bcsc_kernels.hip) launches what plan_bcsc returns, and a stand-alone program (tests/bcsc_plan_main.cpp)
// prints it on any machine.
#pragma once
#include "internal.hpp"
#include <algorithm>

namespace xamd {

// ---- limits the decision and the kernels share ----
constexpr int kBcscTbl = 1024;       // table entries per wave (n-blocks per wave x k-blocks)
constexpr int kBcscTblDma = 256;     // same for the LDS-DMA kernel, which spends its LDS on the A ring instead
constexpr int kBcscBLds = 10240;     // bytes of LDS for a copy of the whole B value array (BL): 2 : 8 of 256 x 64 in bf16 is 8 KiB
constexpr int kBcscRecs = 64;        // chunk records per wave (ring depth 3; depth 2: half)

// ---- A/B build switches of the ring depth of bcsc_mfma_bf16_stream_full_kernel (3 in the shipped library) ----
#if !defined(XAMD_BCSC_THREE)
#define XAMD_BCSC_THREE 0           // ring depth 2 on three workgroups per CU when B and the record list fit the smaller LDS plan:
#endif                              // measured equal to ring depth 3 on two workgroups per CU (config #4 52.1-52.3 against 52.3-52.4 us, 32 768 M-blocks 213.8 against 209.4: the kernel is
                                    // bound by the memory system, not by what a wave does between its waits; profiles/r06_bcsc_three.jsonl) -- not instantiated unless built with -DXAMD_BCSC_THREE=1
#if !defined(XAMD_BCSC_DEEP)
#define XAMD_BCSC_DEEP 0            // ring depth 4 where B (<= 8 KiB) and the record list (<= 32) leave room for it: built, verified (124 parity tests) and measured equal on
                                    // config #4 (51.8-52.8 against 51.5-52.4 us), worse on short tiles (bn = 64: 30.5 against 26.7 us, the eight-pass epilogue): not instantiated
                                    // unless built with -DXAMD_BCSC_DEEP=1 (profiles/r06_bcsc_deep.jsonl).  The copy floor with LDS-DMA reads equals the one with register loads.
#endif

enum BcscFamily { kBcscGeneric, kBcscBf16, kBcscF32, kBcscI8 };   // the operands a kernel reads
enum BcscForm {
  kBcscRegister,   // one tile of C per wave, A loaded into registers, the pattern rows built by every wave
  kBcscDma,        // one tile per wave, A through an LDS-DMA ring, the inverted pattern read from BcscArgs::table
  kBcscStream,     // waves streaming over M-blocks
  kBcscFull        // ... on whole 64 x 64 tiles with B in LDS: one record per chunk
};

struct BcscPlan {
  BcscFamily family; BcscForm form;
  // template selectors (a kernel without the parameter leaves its selector 0)
  int bn_sel;            // 0, 1, 2: bn = 16, 32, 64
  int nt_a;              // A requested non-temporal
  int early;             // one n-tile: the first chunks are requested from the host's k-block mask (kmask0 describes the first n-tile)
  int b_lds;             // the general bf16 streaming kernel keeps B's values in LDS
  int ua;                // 8-bit integers: A unsigned
  int depth;             // ring depth of the bf16 full kernel
  unsigned int tiles_i, tiles_n;
  long long total;       // waves of a one-tile form: tiles_i tiles_n m_blocks (the generic kernel: 64-row column pieces)
  long long mbg, waves;  // streaming forms: the M-blocks worked on at a time, and the waves that do it
  int nkb;               // K / bk
  bool invert;           // bcsc_invert_kernel fills BcscArgs::table first
  const char* name;
};

inline bool bcsc_empty(const BcscArgs& a) { return a.m_blocks <= 0 || a.M <= 0 || a.N <= 0; }

// Waves streaming over M-blocks: `slots` waves are resident at a time; each of the tt (i-tile, n-tile) pairs gets mbg of them, wave g taking M-blocks g, g + mbg, ...
// mbg is then lowered to the smallest count that needs the same number of M-blocks per wave.
inline void bcsc_stream_waves(BcscPlan& p, long long m_blocks, long long tt, long long slots) {
  const long long fit = std::min<long long>(m_blocks, std::max<long long>(1, slots / tt));
  const long long per = (m_blocks + fit - 1) / fit;
  p.mbg = (m_blocks + per - 1) / per;
  p.waves = p.mbg * tt;
}

// a (not empty) with nt_a set.  The families in their order of precedence; within one, the most special form first.
inline BcscPlan plan_bcsc(const BcscArgs& a) {
  BcscPlan p{};
  p.depth = 3;
  p.tiles_i = (unsigned int)((a.M + 63ll) / 64); p.tiles_n = (unsigned int)((a.N + 63ll) / 64);
  const long long tt = (long long)p.tiles_i * p.tiles_n;
  const bool blocks_ok = a.bk > 0 && a.K >= a.bk && (a.bn == 16 || a.bn == 32 || a.bn == 64);      // (no k-block at all: nothing for a matrix-core kernel to stream)
  p.nkb = a.bk > 0 ? a.K / a.bk : 0;
  const int nkb = p.nkb;
  const long long entries = blocks_ok ? (long long)(64 / a.bn) * nkb : 0;                          // table entries of a wave: its n-blocks x the k-blocks
  const size_t a_at = (size_t)a.a, b_at = (size_t)a.bvals, c_at = (size_t)a.c;
  const bool whole = a.M % 64 == 0 && a.N % 64 == 0;
  // a total >= 2^31 leaves every matrix-core family to the generic kernel
  const bool tiles_ok = blocks_ok && a.M % 16 == 0 && entries <= kBcscTbl && a_at % 4 == 0 && c_at % 16 == 0 && tt < (1ll << 31) && tt * a.m_blocks < (1ll << 31);
  // many M-blocks per (i-tile, n-tile): waves that stream over M-blocks (two per SIMD: 2048 on the chip), each taking every mbg-th block.  They never read C.
  const bool many = a.beta0 && nkb <= 64 && tt <= 2048 && (long long)a.m_blocks * tt >= 4096;
  const bool dma_ok = a.table != nullptr && entries <= kBcscTblDma && a_at % 16 == 0;              // the A ring is fed by 16-byte LDS-DMA; the wave's pattern rows fit its LDS table
  p.bn_sel = a.bn == 16 ? 0 : (a.bn == 32 ? 1 : 2);
  p.total = tiles_ok ? tt * a.m_blocks : 0;

  // bf16 on the matrix cores: VNNI-2 A, 32-deep k steps, 16-wide n sub-tiles, 16-row i tiles, 8-byte aligned C columns
  if (tiles_ok && a.a_type == LIBXSMM_DATATYPE_BF16 && a.vnni_a && a.bk % 32 == 0 && b_at % 16 == 0) {
    p.family = kBcscBf16;
    if (!(dma_ok && a.M % 4 == 0 && (long long)(a.K / 2) * a.M < (1ll << 30))) { p.form = kBcscRegister; p.name = "bcsc_mfma_bf16_kernel"; return p; }
    // the inverted pattern: already in place when the pattern came from host memory (built there, cached per kernel: run_bcsc)
    p.invert = !a.table_ready;
    // A is read exactly once: stream it non-temporally when it cannot be cache resident anyway (or the caller says so)
    p.nt_a = a.nt_a != 0;
    if (!(many && ((long long)(a.K / 2) * a.M) * (long long)a.m_blocks < (1ll << 40))) { p.form = kBcscDma; p.name = "bcsc_mfma_bf16_dma_kernel"; return p; }
    const long long b_bytes = (long long)a.nnzb * a.bn * a.bk * 2, recs = (long long)nkb * (a.bk / 32);
    // a value array that fits beside the rings: every workgroup keeps its own LDS copy of B and no wave asks the L2 for a
    // fragment again (bn = 32: 39.5 -> 35.7 us on 8192 M-blocks of 64 x 256, bn = 16 unchanged; profiles/r06_bcsc_b_in_lds.jsonl)
    p.b_lds = a.nnzb > 0 && b_bytes <= kBcscBLds && b_at % 16 == 0;
    // ... and whole 64 x 64 tiles with bf16 C: the kernel with one record per chunk
    const bool full = p.b_lds && a.c_type == LIBXSMM_DATATYPE_BF16 && whole && c_at % 16 == 0 && recs <= kBcscRecs;
    // ... on three workgroups per CU (ring depth 2) or at ring depth 4 when B and the record list fit the smaller LDS plan (XAMD_BCSC_THREE before XAMD_BCSC_DEEP)
    const bool small = b_bytes <= 8192 && recs <= kBcscRecs / 2;
    if (full && small) p.depth = XAMD_BCSC_THREE != 0 ? 2 : (XAMD_BCSC_DEEP != 0 ? 4 : 3);
    // 32 rows per wave (RT = 2: 161 VGPRs, three waves per SIMD) measured 72 us against 61 us: every B fragment then feeds two MFMAs instead of four
    // waves per round: two per SIMD (the general kernel: 245 VGPRs; three spill inside the chunk loop: 105 instead of 61 us), three at ring depth 2
    bcsc_stream_waves(p, a.m_blocks, tt, p.depth == 2 ? 3072 : 2048);
    if (!full) { p.form = kBcscStream; p.name = "bcsc_mfma_bf16_stream_kernel"; return p; }
    p.form = kBcscFull; p.b_lds = 0; p.early = p.tiles_n == 1; p.name = "bcsc_mfma_bf16_stream_full_kernel";
    return p;
  }

  // f32 on the matrix cores: 16-deep k steps, 16-wide n sub-tiles, 16-row i tiles, 16-byte aligned B blocks and C columns
  if (tiles_ok && a.a_type == LIBXSMM_DATATYPE_F32 && a.c_type == LIBXSMM_DATATYPE_F32 && a.bk % 16 == 0 && a.N % a.bn == 0 && b_at % 16 == 0 && a.M % 4 == 0) {
    p.family = kBcscF32;
    // many M-blocks per (i-tile, n-tile): the bf16 kernel's waves streaming over M-blocks, on f32 operands (round 3; the one-tile-per-wave kernel
    // builds its pattern rows in every wave and fetches A one 16-deep step ahead: 0.65 of the HBM roofline on config #4's shape)
    if (!(dma_ok && many && (long long)a.K * a.M < (1ll << 30) && ((long long)a.K * a.M) * (long long)a.m_blocks < (1ll << 40))) { p.form = kBcscRegister; p.name = "bcsc_mfma_f32_kernel"; return p; }
    p.invert = !a.table_ready;
    p.nt_a = a.nt_a != 0;
    // two waves per SIMD (182 registers); three (168: ten spills) measured 139.7 us against 119.1 us
    bcsc_stream_waves(p, a.m_blocks, tt, 2048);
    // host-resident / bound pattern, whole 64 x 64 tiles, B up to 16 KiB: the kernel with one record per chunk (see bcsc_mfma_bf16_stream_full_kernel)
    if (!(a.nnzb > 0 && (long long)a.nnzb * a.bn * a.bk * 4 <= 16384 && whole && (long long)nkb * (a.bk / 16) <= kBcscRecs)) { p.form = kBcscStream; p.name = "bcsc_mfma_f32_stream_kernel"; return p; }
    p.form = kBcscFull; p.early = p.tiles_n == 1; p.name = "bcsc_mfma_f32_stream_full_kernel";
    return p;
  }

  // 8-bit integers on the matrix cores: VNNI-4 A, 32-deep k steps, 16-wide n sub-tiles, 16-row i tiles, dword / 8-byte / 16-byte aligned A / B / C
  const bool i8 = (a.a_type == LIBXSMM_DATATYPE_U8 && a.b_type == LIBXSMM_DATATYPE_I8) || (a.a_type == LIBXSMM_DATATYPE_I8 && a.b_type == LIBXSMM_DATATYPE_U8);
  if (tiles_ok && i8 && a.c_type == LIBXSMM_DATATYPE_I32 && a.vnni_a && a.bk % 32 == 0 && a.N % a.bn == 0 && b_at % 8 == 0) {
    p.family = kBcscI8;
    p.ua = a.a_type == LIBXSMM_DATATYPE_U8;
    if (!(dma_ok && a.M % 4 == 0 && (long long)(a.K / 4) * a.M < (1ll << 30))) { p.form = kBcscRegister; p.name = "bcsc_mfma_i8_kernel"; return p; }
    p.invert = !a.table_ready;
    p.nt_a = a.nt_a != 0;
    // host-resident / bound pattern, whole 64 x 64 tiles, beta = 0, B up to 8 KiB, many M-blocks per tile: waves streaming over M-blocks with one record per chunk.
    // (Anything else that is dma_ok takes the dma kernel: a general streaming kernel for integers was measured and not kept -- the figures stand at the table of
    // bcsc_mfma_i8_dma_kernel in bcsc_kernels.hip.)
    if (!(many && a.nnzb > 0 && (long long)a.nnzb * a.bn * a.bk <= 8192 && b_at % 16 == 0 && whole && (long long)nkb * (a.bk / 32) <= kBcscRecs)) { p.form = kBcscDma; p.name = "bcsc_mfma_i8_dma_kernel"; return p; }
    bcsc_stream_waves(p, a.m_blocks, tt, 2048);          // two waves per SIMD
    p.form = kBcscFull; p.early = p.tiles_n == 1; p.name = "bcsc_mfma_i8_stream_full_kernel";
    return p;
  }

  // whatever the matrix cores refuse: one thread per (i, n) of one M-block
  p.family = kBcscGeneric; p.form = kBcscRegister; p.bn_sel = 0;
  p.total = (long long)p.tiles_i * a.N * a.m_blocks;
  p.name = "bcsc_generic_kernel";
  return p;
}

}  // namespace xamd
