// gemm_group_tile.hpp -- the one-wave C tiles shared by the grouped kernels (gemm_grouped_kernels.hip) and the segment kernels
// (gemm_segments_kernels.hip): a wave owns a T x T tile of C (T = 32 or 16) and walks a CHAIN of (A, B) block pairs, one accumulator over (block, k).
// Where the blocks of the chain lie is the only thing the two users differ in, so it is a template parameter:
//   StrideChain   block r = base + r * stride                                   (STRIDE batch-reduce; count 1 for plain GEMM handles)
//   ListChain     block r = a_list[r], b_list[r], read with scalar loads         (ADDRESS batch-reduce with a count of its own per segment)
//   OffsetChain   block r = a + a_offs[r], b + b_offs[r], read the same way      (OFFSET batch-reduce segments: two bases by value, signed byte offsets)
// A chain hands out block r + 1 while block r is being multiplied (fetch), so a list chain's dependent address -> data round trip overlaps the MFMAs, and it
// answers the alignment questions of the wider loads per block (a stride chain answers with what the host worked out for the whole group).
//
// Both operands enter the MFMA swapped (B as the first operand, A as the second), as gemm_tile.hpp does: the accumulator then holds a column of C per register
// and the ROWS of C on the lanes, so every store of a register is a contiguous run of 16 or 32 rows.
//   f32 : v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32 with k in natural order -- the result is the k-ordered fmaf chain bit for bit
//         (cdna_hip_programming.md, "FP32-input MFMA"), which is what oracle_gemm_f32_fma computes [ref: src/generator_gemm_reference_impl.c:1359-1426].
//   bf16: v_mfma_f32_32x32x16_bf16 / v_mfma_f32_16x16x16_bf16, A flat or VNNI-2, B flat, C f32 or bf16 (bf16_cvt.hpp: the reference's conversion exactly).
//   f16 : v_mfma_f32_32x32x16_f16 / v_mfma_f32_16x16x16_f16 through the bf16 tile (template argument H16: same lane layout, same loads, same padding -- 0x8000 is
//         -0 and 0 is +0 in both formats), A flat or VNNI-2, B flat, C f32 or f16.  The start rule is the reference's F16 loop, NOT the bf16 one
//         [ref: src/generator_gemm_reference_impl.c:2025-2124, :296-317]: the chain starts at +0, the start value (C, the bias, bias + C in one f32 add) is
//         rounded to f16, widened and added AFTER the sum in one f32 add; an f16 C leaves through the hardware RNE conversion (cvt_pk_f16).
//   f64 : v_mfma_f64_16x16x4_f64, T = 16 only, k in natural order, four k per instruction [ref: src/generator_gemm_reference_impl.c:1322-1358].
//   fp8 : v_mfma_f32_32x32x16_{bf8_bf8,fp8_fp8} / v_mfma_f32_16x16x32_{bf8_bf8,fp8_fp8} (BF8 = E5M2, HF8 = E4M3), A VNNI-4, B flat, NN only, C f32 or the
//         operands' type (gemm_8bit.hpp: the reference's two-step rounding) [ref: src/generator_gemm_reference_impl.c:2420-2619].  The matrix core aligns the
//         products of one instruction before it adds them: the reference's serial chain within a tolerance, bitwise where every partial sum is exact.
// beta = 1 starts the chain at C.  Ragged k is padded with A = -0.0 and B = +0.0: adding the product -0 is an exact identity for every accumulator
// (+0 + -0 = +0 under round-to-nearest), so the f32 chain stays bitwise.  Rows and columns beyond m / n load the last valid row / column and are never
// stored, so no access leaves the caller's operands.
// Transposed operands (template arguments TA / TB, NN by default: the instances without them are instruction for instruction what they were) swap the two load
// forms a tile has.  An operand is either contiguous over the LANES and strided in k (flat A: A(i, k) at k * lda + i; TRANS_B: B(k, j) at k * ldb + j) or
// contiguous in K per lane (flat B: B(k, j) at j * ldb + k; TRANS_A: A(i, k) at i * lda + k).  A transposed A therefore takes B's loads -- 16-byte pieces of
// the lane's k run for f32 (each lane half picks its odd or even k), one 16- or 8-byte load per MFMA step for bf16, chosen per product from the pointer and
// the leading dimension -- and a transposed B takes flat A's element loads.  f64 loads elements in both forms: lane s of a 16 x 16 x 4 step owns the k with
// k % 4 == s, so no two k of a lane are neighbours and a pair load would fetch one element it cannot use; the four lanes of a row still cover one 32-byte sector.
// The clamping is that of the NN forms: a wide load starts at i * lda + kk inside a whole k block (kk + its width <= K <= lda), rows and columns beyond m / n
// read row m - 1 / column n - 1, ragged k reads k = K - 1 -- the last element touched is (m - 1) * lda + K - 1 of a TRANS_A block, (K - 1) * ldb + n - 1 of a
// TRANS_B block.
#pragma once
#include <hip/hip_runtime.h>
#include "internal.hpp"
#include "gemm_device.hpp"
#include "bf16_cvt.hpp"
#include "gemm_tile.hpp"                           // act_fixed: the fused activations; bf8_to_f32 / hf8_to_f32
#include "gemm_8bit.hpp"                           // f32x2_to_fp8_ref: the store of an 8-bit float C

namespace xamd {
namespace group_tile {

struct StrideChain {
  gcptr a, b; long long sa, sb; unsigned long long count;
  int va4, vb16, vb8;                              // the host's verdict for every block of the group (GemmGroupDesc::a_vec4 / b_vec16 / b_vec8)
  __device__ __forceinline__ void fetch(unsigned long long r, gcptr& pa, gcptr& pb) const { pa = a + (long long)r * sa; pb = b + (long long)r * sb; }
  __device__ __forceinline__ bool a_vec4(gcptr) const { return va4 != 0; }
  __device__ __forceinline__ bool b_vec16(gcptr) const { return vb16 != 0; }
  __device__ __forceinline__ bool b_vec8(gcptr) const { return vb8 != 0; }
};
__device__ __forceinline__ StrideChain stride_chain(const GemmGroupDesc& g, gcptr a, gcptr b) {
  return StrideChain{a, b, g.br_sa, g.br_sb, g.br_count, g.a_vec4, g.b_vec16, g.b_vec8};
}

// `la` / `lb` point at the chain's first list entry.  The lists are only read at entries < count: fetch(count) re-reads the last entry, whose value is dropped.
// A block pointer is only known to be element-aligned, so the wider loads are chosen per block by a wave-uniform test of the pointer; `va4` / `vb16` / `vb8`
// say whether the leading dimension allows them at all.
struct ListChain {
  const void* la; const void* lb; unsigned long long count;
  int va4, vb16, vb8;
  __device__ __forceinline__ void fetch(unsigned long long r, gcptr& pa, gcptr& pb) const {
    const unsigned long long rc = r < count ? r : count - 1;
    pa = list_entry(la, rc); pb = list_entry(lb, rc);
  }
  __device__ __forceinline__ bool a_vec4(gcptr p) const { return va4 != 0 && ((unsigned int)(size_t)p & 3u) == 0; }
  __device__ __forceinline__ bool b_vec16(gcptr p) const { return vb16 != 0 && ((unsigned int)(size_t)p & 15u) == 0; }
  __device__ __forceinline__ bool b_vec8(gcptr p) const { return vb8 != 0 && ((unsigned int)(size_t)p & 7u) == 0; }
};

// The OFFSET form of a list chain [ref: src/generator_gemm_reference_impl.c:186-188]: `oa` / `ob` point at the chain's first signed byte offset, `a` / `b` are the
// bases every offset is added to.  Same prefetch, same re-read of the last entry at fetch(count).  The alignment questions are asked of the resulting pointer;
// `va16` / `va8` say whether the leading dimension of a TRANSPOSED A allows 16- / 8-byte loads of a row's k run.
struct OffsetChain {
  gcptr a, b; const void* oa; const void* ob; unsigned long long count;
  int va4, vb16, vb8, va16, va8;
  __device__ __forceinline__ void fetch(unsigned long long r, gcptr& pa, gcptr& pb) const {
    const unsigned long long rc = r < count ? r : count - 1;
    pa = a + (long long)uniform_u64(((GM const unsigned long long*)oa)[rc]); pb = b + (long long)uniform_u64(((GM const unsigned long long*)ob)[rc]);
  }
  __device__ __forceinline__ bool a_vec4(gcptr p) const { return va4 != 0 && ((unsigned int)(size_t)p & 3u) == 0; }
  __device__ __forceinline__ bool a_vec16(gcptr p) const { return va16 != 0 && ((unsigned int)(size_t)p & 15u) == 0; }
  __device__ __forceinline__ bool a_vec8(gcptr p) const { return va8 != 0 && ((unsigned int)(size_t)p & 7u) == 0; }
  __device__ __forceinline__ bool b_vec16(gcptr p) const { return vb16 != 0 && ((unsigned int)(size_t)p & 15u) == 0; }
  __device__ __forceinline__ bool b_vec8(gcptr p) const { return vb8 != 0 && ((unsigned int)(size_t)p & 7u) == 0; }
};

// element index of k in a lane's operand pointer: KC (contiguous in k: flat B, TRANS_A) k itself, else (contiguous over the lanes: flat A, TRANS_B) k * ld;
// and of the lane's row / column x where that pointer starts
template <bool KC> __device__ __forceinline__ int k_index(int k, int ld) { if constexpr (KC) return k; else return k * ld; }
template <bool KC> __device__ __forceinline__ long long lane_index(int x, int ld) { if constexpr (KC) return (long long)x * ld; else return x; }

// accumulator register r of lane `lane` holds C column (j0 +) acc_col<T>(r, lane), C row (i0 +) lane % T
template <int T> __device__ __forceinline__ int acc_col(int r, unsigned int lane) {
  if constexpr (T == 32) return (r & 3) + 8 * (r >> 2) + 4 * (int)(lane >> 5);
  else return 4 * (int)(lane >> 4) + r;
}

typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <int T> struct Acc;
template <> struct Acc<32> { typedef f32x16 type; static constexpr int N = 16; };
template <> struct Acc<16> { typedef f32x4 type; static constexpr int N = 4; };

__device__ __forceinline__ f32x16 mfma_f32(float x, float y, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, acc, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma_f32(float x, float y, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, acc, 0, 0, 0); }

__device__ __forceinline__ float bf16_bits_to_f32(unsigned short v) { return __uint_as_float((unsigned int)v << 16); }

// What happens around the chain is a template parameter of the tiles.  NoEpilogue (the default: the grouped kernels and the plain segment kernels) adds
// nothing -- every use of it sits behind `if constexpr`, so those instances compile to the code they had before the parameter existed.  FusedEpilogue is the
// ext ABI's epilogue [ref: src/generator_gemm_reference_impl.c:294-372] for one C block: a column bias of C's type added into the start value, the ReLU
// bitmask taken from the sums, the activation, then the store.  All of its members are wave-uniform (one C block per wave), so they are runtime bits.
struct NoEpilogue { static constexpr bool fused = false; };
struct FusedEpilogue {
  static constexpr bool fused = true;
  gcptr d;                                         // the block's m-vector bias (colbias != 0)
  GM unsigned char* mask;                          // the block's ReLU bitmask (act == 2)
  int colbias, act, mask_ld;                       // act: 0 none, 1 ReLU, 2 ReLU + bitmask, 3 sigmoid (gemm_tile.hpp: act_fixed)
};

// the accumulator's start value: C (beta = 1) or +0; fused: bias, or bias + C in one f32 add.  C8 (the 8-bit float tiles only: 1 BF8, 2 HF8): C is f32 or,
// with g.c_kind >= 2, of the operands' type and widened; the other instances know c_kind as 0 or 1 and keep the code they had with a single bf16 bit.
// H16 (the f16 tiles only): the chain starts at +0 and nothing is loaded -- the start value is added behind the sum, in acc_store.
template <int T, typename Epi = NoEpilogue, int C8 = 0, bool H16 = false>
__device__ __forceinline__ typename Acc<T>::type acc_start(const GemmGroupDesc& g, gptr c, int i, int j0, bool mv, unsigned int lane, const Epi& e = Epi()) {
  typename Acc<T>::type acc;
  if constexpr (H16) {
    static_for<Acc<T>::N>([&](auto r) { acc[r.value] = 0.0f; });
    return acc;
  }
  float bias = 0.0f;
  bool biased = false;
  if constexpr (Epi::fused) {
    biased = e.colbias != 0;
    if (biased) {                                  // one load per lane, clamped like the operand loads: rows beyond m read row m - 1 and are never stored
      const int il = min(i, g.m - 1);
      bias = g.c_kind != 0 ? bf16_bits_to_f32(((GM const unsigned short*)e.d)[il]) : ((GM const float*)e.d)[il];
    }
  }
  static_for<Acc<T>::N>([&](auto r) {
    const int j = j0 + acc_col<T>(r, lane);
    float v = 0.0f;
    if (g.beta1 && mv && j < g.n) {
      const long long o = (long long)j * g.ldc + i;
      if constexpr (C8 != 0) {
        if (g.c_kind >= 2) { const unsigned char x = ((GM const unsigned char*)c)[o]; v = C8 == 2 ? hf8_to_f32(x) : bf8_to_f32(x); }
        else v = ((GM const float*)c)[o];
      } else v = g.c_kind != 0 ? bf16_bits_to_f32(((GM const unsigned short*)c)[o]) : ((GM const float*)c)[o];
    }
    if constexpr (Epi::fused) { if (biased) v = g.beta1 ? bias + v : bias; }
    acc[r.value] = v;
  });
  return acc;
}

// ReLU bitmask of one tile: bit i % 8 of byte i / 8 + j * (mask_ld / 8) is !(x <= 0) of the sum [ref: mateltwise ref :150-157, :2142].  The lanes hold rows,
// so a register's ballot is the mask of its two (T = 32) or four (T = 16) columns; the lane with (lane & 7) == 0 owns the byte of its 8 rows.  Tile origins are
// multiples of 16: a byte never straddles tiles.  Only bits of rows < m, columns < n change: the byte that holds row m - 1 is read, merged and written back.
// (H16: the f16 tiles take an instance of their own.  The body is the same; sharing one instance -- and so one lambda, the one function here that the
// inliner weighs -- with more callers changed the register allocation of the existing fused kernels.  Marking the lambda always_inline instead was tried: it
// changes the code of the ten existing fused segment kernels too, so it would have to come with a re-measurement of those; tools/code_diff.py is the check.)
template <int T, bool H16 = false>
__device__ __forceinline__ void acc_relu_mask(const GemmGroupDesc& g, const FusedEpilogue& e, const typename Acc<T>::type& acc, int i, int j0, bool mv, unsigned int lane) {
  static_for<Acc<T>::N>([&](auto r) {
    const int j = j0 + acc_col<T>(r, lane);
    const bool ok = mv && j < g.n;
    const unsigned long long pos = __ballot(ok && !(acc[r.value] <= 0.0f));
    const unsigned long long val = __ballot(ok);
    if ((lane & 7u) == 0 && ok) {
      GM unsigned char* byte = e.mask + i / 8 + (long long)j * (e.mask_ld / 8);
      const unsigned char vm = (unsigned char)((val >> lane) & 0xffu), nb = (unsigned char)((pos >> lane) & 0xffu);
      *byte = vm == 0xffu ? nb : (unsigned char)((*byte & ~vm) | (nb & vm));
    }
  });
}

// H16 (the f16 tiles only; g.c_kind == 4: C and the bias are f16, else f32): `acc` is the sum from +0.  The start value -- C under beta = 1, the bias, or
// bias + C in one f32 add -- is loaded here under the predicates of the stores (i < m, j < n; the bias row clamped to m - 1 as in acc_start), rounded to f16
// (the identity for a lone f16 value, a real rounding for an f32 C, an f32 bias or a sum), widened and added in one f32 add; without a start nothing is added.
// Then mask, activation and store as for every class; an f16 C is converted two results at a time (v_cvt_pk_f16_f32: RNE, registers 2 q and 2 q + 1 are two
// columns of the lane's row) and stored element by element, as the bf16 C is.
template <int T, typename Epi = NoEpilogue, int C8 = 0, bool H16 = false>
__device__ __forceinline__ void acc_store(const GemmGroupDesc& g, gptr c, typename Acc<T>::type acc, int i, int j0, bool mv, unsigned int lane, const Epi& e = Epi()) {
  constexpr int N = Acc<T>::N;
  if constexpr (H16) {
    const bool c16 = g.c_kind == 4;
    float bias = 0.0f;
    bool biased = false;
    if constexpr (Epi::fused) {
      biased = e.colbias != 0;
      if (biased) {
        const int il = min(i, g.m - 1);
        bias = c16 ? (float)((GM const _Float16*)e.d)[il] : ((GM const float*)e.d)[il];
      }
    }
    if (g.beta1 || biased) {
      static_for<N>([&](auto r) {
        const int j = j0 + acc_col<T>(r, lane);
        float v = 0.0f;
        if (g.beta1 && mv && j < g.n) {
          const long long o = (long long)j * g.ldc + i;
          v = c16 ? (float)((GM const _Float16*)c)[o] : ((GM const float*)c)[o];
        }
        if (biased) v = g.beta1 ? bias + v : bias;
        acc[r.value] = acc[r.value] + (float)(_Float16)v;
      });
    }
    if constexpr (Epi::fused) {
      if (e.act == 2) acc_relu_mask<T, true>(g, e, acc, i, j0, mv, lane);
      if (e.act == 3) static_for<N>([&](auto r) { acc[r.value] = act_fixed<3>(acc[r.value]); });
      else if (e.act != 0) static_for<N>([&](auto r) { acc[r.value] = act_fixed<1>(acc[r.value]); });
    }
    if (c16) {
      static_for<N / 2>([&](auto q) {
        constexpr int r0 = 2 * q.value, r1 = r0 + 1;
        const unsigned int w = cvt_pk_f16(acc[r0], acc[r1]);
        const int ja = j0 + acc_col<T>(r0, lane), jb = j0 + acc_col<T>(r1, lane);
        if (mv && ja < g.n) ((GM unsigned short*)c)[(long long)ja * g.ldc + i] = (unsigned short)(w & 0xffffu);
        if (mv && jb < g.n) ((GM unsigned short*)c)[(long long)jb * g.ldc + i] = (unsigned short)(w >> 16);
      });
    } else {
      static_for<N>([&](auto r) {
        const int j = j0 + acc_col<T>(r, lane);
        if (mv && j < g.n) ((GM float*)c)[(long long)j * g.ldc + i] = acc[r.value];
      });
    }
    return;
  }
  if constexpr (Epi::fused) {                      // the mask from the sums, then the activation, then the store below
    if (e.act == 2) acc_relu_mask<T>(g, e, acc, i, j0, mv, lane);
    if (e.act == 3) static_for<N>([&](auto r) { acc[r.value] = act_fixed<3>(acc[r.value]); });
    else if (e.act != 0) static_for<N>([&](auto r) { acc[r.value] = act_fixed<1>(acc[r.value]); });
  }
  if constexpr (C8 != 0) {
    if (g.c_kind >= 2) {                           // two results per conversion (f32 -> f16 -> 8 bits, NaNs in software), one byte store each
      static_for<N / 2>([&](auto q) {
        constexpr int r0 = 2 * q.value, r1 = r0 + 1;
        const unsigned int w = f32x2_to_fp8_ref(acc[r0], acc[r1], C8 == 2);
        const int ja = j0 + acc_col<T>(r0, lane), jb = j0 + acc_col<T>(r1, lane);
        if (mv && ja < g.n) ((GM unsigned char*)c)[(long long)ja * g.ldc + i] = (unsigned char)(w & 0xffu);
        if (mv && jb < g.n) ((GM unsigned char*)c)[(long long)jb * g.ldc + i] = (unsigned char)(w >> 8);
      });
      return;
    }
  }
  if (C8 == 0 && g.c_kind != 0) {
    float x[N]; unsigned int pk[N / 2];
    static_for<N>([&](auto r) { x[r] = acc[r.value]; });
    bf16_pk_exact_n<N / 2>(x, pk);
    static_for<N>([&](auto r) {
      const int j = j0 + acc_col<T>(r, lane);
      if (mv && j < g.n) ((GM unsigned short*)c)[(long long)j * g.ldc + i] = (unsigned short)((r & 1) ? (pk[r / 2] >> 16) : (pk[r / 2] & 0xffffu));
    });
  } else {
    static_for<N>([&](auto r) {
      const int j = j0 + acc_col<T>(r, lane);
      if (mv && j < g.n) ((GM float*)c)[(long long)j * g.ldc + i] = acc[r.value];
    });
  }
}

// U consecutive MFMA steps of an f32 tile from k = kk on: all operand requests of the steps go out before the first MFMA, so a block of U steps pays the
// memory latency once.  b_vec: B(kk .. kk + 2 U - 1) of the lane's column in 16-byte pieces (32-tiles); lane half h takes the odd or even k of a piece.
// TA: A's k run is the contiguous one and takes the same pieces under a_vec; TB: B is read like flat A, element by element at k * ldb.
template <int T, int U, bool TA = false, bool TB = false>
__device__ __forceinline__ void steps_f32(typename Acc<T>::type& acc, GM const float* ap, GM const float* bp, int kk, int lda, int h, bool b_vec, int ldb = 0, bool a_vec = false) {
  constexpr int KS = (T == 32) ? 2 : 4;
  float av[U], bv[U];
  if constexpr (TA) {
    if (T == 32 && a_vec) {
#pragma unroll
      for (int q = 0; q < U / 2; ++q) {
        const f32x4 v = *(GM const f32x4*)(ap + kk + 4 * q);
        av[2 * q] = h ? v[1] : v[0]; av[2 * q + 1] = h ? v[3] : v[2];
      }
    } else {
#pragma unroll
      for (int s = 0; s < U; ++s) av[s] = ap[kk + s * KS + h];
    }
  } else {
#pragma unroll
    for (int s = 0; s < U; ++s) av[s] = ap[(kk + s * KS + h) * lda];
  }
  if constexpr (TB) {
#pragma unroll
    for (int s = 0; s < U; ++s) bv[s] = bp[(kk + s * KS + h) * ldb];
  } else if (T == 32 && b_vec) {
#pragma unroll
    for (int q = 0; q < U / 2; ++q) {
      const f32x4 v = *(GM const f32x4*)(bp + kk + 4 * q);
      bv[2 * q] = h ? v[1] : v[0]; bv[2 * q + 1] = h ? v[3] : v[2];
    }
  } else {
#pragma unroll
    for (int s = 0; s < U; ++s) bv[s] = bp[kk + s * KS + h];
  }
#pragma unroll
  for (int s = 0; s < U; ++s) acc = mfma_f32(bv[s], av[s], acc);
}

// one C tile of T x T of an f32 element: lane (i = lane % T, h = lane / T) feeds A(i, k0 + h) and B(k0 + h, j0 + lane % T) per MFMA.
// Loads carry no predicate (a predicated load is a branch around it in the code): rows / columns beyond m / n read the last valid row / column -- in bounds,
// never stored -- and k beyond K reads k = K - 1 and replaces the value by the -0 / +0 padding.  k advances in blocks of 4 MFMA steps, then one block of up to
// 4 ragged steps; DEEP puts blocks of 16 steps in front (32 k on a 32-tile: a 32^3 block is ONE round of requests, at 72 more registers) for the kernels
// whose waves walk long chains alone (segments).  The MFMAs always follow k in natural order.
template <int T, bool DEEP, typename Chain, typename Epi = NoEpilogue, bool TA = false, bool TB = false>
__device__ __forceinline__ void tile_f32(const GemmGroupDesc& g, const Chain& ch, gptr c, int i0, int j0, unsigned int lane, const Epi& e = Epi()) {
  constexpr int KS = (T == 32) ? 2 : 4;
  const int lr = (int)(lane & (T - 1)), h = (int)(lane / T);
  const int i = i0 + lr, j = j0 + lr;
  const bool mv = i < g.m;
  typename Acc<T>::type acc = acc_start<T, Epi>(g, c, i, j0, mv, lane, e);
  const int K = g.k, lda = g.lda, ldb = g.ldb;
  const int kbig = K - K % (16 * KS), kfull = K - K % (4 * KS);
  gcptr an = nullptr, bn = nullptr;
  if (ch.count) ch.fetch(0, an, bn);
  for (unsigned long long r = 0; r < ch.count; ++r) {
    const gcptr a = an, b = bn;
    ch.fetch(r + 1, an, bn);                   // the next block's addresses are on their way while this block is multiplied
    GM const float* ap = (GM const float*)a + lane_index<TA>(min(i, g.m - 1), lda);
    GM const float* bp = (GM const float*)b + lane_index<!TB>(min(j, g.n - 1), g.ldb);
    bool b_vec = false, a_vec = false;
    if constexpr (!TB) b_vec = T == 32 && ch.b_vec16(b);
    if constexpr (TA) a_vec = T == 32 && ch.a_vec16(a);
    int kk = 0;
    if constexpr (DEEP) for (; kk < kbig; kk += 16 * KS) steps_f32<T, 16, TA, TB>(acc, ap, bp, kk, lda, h, b_vec, ldb, a_vec);
    for (; kk < kfull; kk += 4 * KS) steps_f32<T, 4, TA, TB>(acc, ap, bp, kk, lda, h, b_vec, ldb, a_vec);
    if (kk < K) {                              // ragged k, up to four steps: A = -0, B = +0 beyond K
      float av[4], bv[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int kx = kk + s * KS + h, kc = min(kx, K - 1);
        const float va = ap[k_index<TA>(kc, lda)], vb = bp[k_index<!TB>(kc, ldb)];
        av[s] = kx < K ? va : -0.0f; bv[s] = kx < K ? vb : 0.0f;
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) if (kk + s * KS < K) acc = mfma_f32(bv[s], av[s], acc);
    }
  }
  acc_store<T, Epi>(g, c, acc, i, j0, mv, lane, e);
}

// bf16: lane (i = lane % T, h = lane / T) feeds A(i, k0 + E h + e) and B(k0 + E h + e, j0 + lane % T), e < E, per MFMA: E = 8 for the 32 x 32 x 16
// instruction, E = 4 for the 16 x 16 x 16 one (a 16-deep k step: a 16^3 problem is one whole step, no padding)
__device__ __forceinline__ unsigned short a_bf16(const GemmGroupDesc& g, GM const unsigned short* ap, int i, int kx) {
  return g.vnni_a ? ap[((long long)(kx >> 1) * g.lda + i) * 2 + (kx & 1)] : ap[(long long)kx * g.lda + i];
}
template <int E> struct Frag;
template <> struct Frag<8> { typedef bf16x8 type; typedef u32x4 words; };
template <> struct Frag<4> { typedef bf16x4 type; typedef u32x2 words; };
__device__ __forceinline__ f32x16 mfma_bf16(bf16x8 x, bf16x8 y, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, y, acc, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma_bf16(bf16x4 x, bf16x4 y, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(x, y, acc, 0, 0, 0); }
// the same steps on IEEE halves (H16): v_mfma_f32_32x32x16_f16 / v_mfma_f32_16x16x16_f16 take the operands of their bf16 siblings lane for lane
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
template <bool H16> __device__ __forceinline__ f32x16 mfma_16(bf16x8 x, bf16x8 y, f32x16 acc) {
  if constexpr (H16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, x), __builtin_bit_cast(f16x8_t, y), acc, 0, 0, 0);
  else return mfma_bf16(x, y, acc);
}
template <bool H16> __device__ __forceinline__ f32x4 mfma_16(bf16x4 x, bf16x4 y, f32x4 acc) {
  if constexpr (H16) return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4_t, x), __builtin_bit_cast(f16x4_t, y), acc, 0, 0, 0);
  else return mfma_bf16(x, y, acc);
}
// U consecutive MFMA steps (16 k each) of a bf16 tile from k = kk on, every operand request ahead of the first MFMA; VEC: both operands are known to take
// the wide loads (no element-wise code in the instance)
// TA: `ap` is the lane's row of a transposed A and a step is ONE 16- / 8-byte load of its k run under a_vec (B's form); TB: `bp` is the lane's column of a
// transposed B, read element by element at k * ldb (flat A's form)
template <int T, int U, bool VEC, bool TA = false, bool TB = false, bool H16 = false> __device__ __forceinline__ void steps_bf16(const GemmGroupDesc& g, typename Acc<T>::type& acc, GM const unsigned short* ap, GM const unsigned short* bp,
  int kk, int il, int h, bool a_vec, bool b_vec) {
  constexpr int E = (T == 32) ? 8 : 4, KS = 16;
  typedef typename Frag<E>::type frag;
  typedef typename Frag<E>::words words;
  frag x[U], y[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int k0 = kk + u * KS + E * h;
    if constexpr (TB) {
#pragma unroll
      for (int e = 0; e < E; ++e) x[u][e] = (short)bp[(k0 + e) * g.ldb];
    } else if (VEC || b_vec) x[u] = __builtin_bit_cast(frag, *(GM const words*)(bp + k0));
    else {
#pragma unroll
      for (int e = 0; e < E; ++e) x[u][e] = (short)bp[k0 + e];
    }
    if constexpr (TA) {
      if (VEC || a_vec) y[u] = __builtin_bit_cast(frag, *(GM const words*)(ap + k0));
      else {
#pragma unroll
        for (int e = 0; e < E; ++e) y[u][e] = (short)ap[k0 + e];
      }
    } else if (VEC || a_vec) {
      GM const unsigned int* ap4 = (GM const unsigned int*)ap;
      words w;
#pragma unroll
      for (int e = 0; e < E / 2; ++e) w[e] = ap4[(long long)((k0 >> 1) + e) * g.lda + il];
      y[u] = __builtin_bit_cast(frag, w);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) y[u][e] = (short)a_bf16(g, ap, il, k0 + e);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) acc = mfma_16<H16>(x[u], y[u], acc);
}
// H16: the elements are IEEE halves -- the f16 instructions, and the f16 start rule of acc_start / acc_store; everything else is the bf16 tile
template <int T, bool DEEP, typename Chain, typename Epi = NoEpilogue, bool TA = false, bool TB = false, bool H16 = false>
__device__ __forceinline__ void tile_bf16(const GemmGroupDesc& g, const Chain& ch, gptr c, int i0, int j0, unsigned int lane, const Epi& e = Epi()) {
  constexpr int E = (T == 32) ? 8 : 4, KS = 16;
  typedef typename Frag<E>::type frag;
  const int lr = (int)(lane & (T - 1)), h = (int)(lane / T);
  const int i = i0 + lr, j = j0 + lr;
  const bool mv = i < g.m;
  const int il = min(i, g.m - 1);
  typename Acc<T>::type acc = acc_start<T, Epi, 0, H16>(g, c, i, j0, mv, lane, e);
  const int K = g.k;
  const int kbig = K - K % (4 * KS), kfull = K - K % KS;
  gcptr an = nullptr, bn = nullptr;
  if (ch.count) ch.fetch(0, an, bn);
  for (unsigned long long r = 0; r < ch.count; ++r) {
    const gcptr a = an, b = bn;
    ch.fetch(r + 1, an, bn);
    GM const unsigned short* ap = (GM const unsigned short*)a;
    if constexpr (TA) ap += (long long)il * g.lda;             // the lane's row
    GM const unsigned short* bp = (GM const unsigned short*)b + lane_index<!TB>(min(j, g.n - 1), g.ldb);
    bool b_vec = false, a_vec;
    if constexpr (!TB) b_vec = (T == 32) ? ch.b_vec16(b) : ch.b_vec8(b);
    if constexpr (TA) a_vec = (T == 32) ? ch.a_vec16(a) : ch.a_vec8(a); else a_vec = g.vnni_a && ch.a_vec4(a);
    int kk = 0;
    if constexpr (DEEP && !TB) {               // segments: 64 k per round of requests when both operands take the wide loads (32 more registers)
      if (a_vec && b_vec) for (; kk < kbig; kk += 4 * KS) steps_bf16<T, 4, true, TA, TB, H16>(g, acc, ap, bp, kk, il, h, true, true);
    }
    for (; kk < kfull; kk += KS) steps_bf16<T, 1, false, TA, TB, H16>(g, acc, ap, bp, kk, il, h, a_vec, b_vec);
    if (kk < K) {                              // ragged k: A = -0 (0x8000), B = +0 beyond K
      const int k0 = kk + E * h;
      frag x, y;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int kx = k0 + e, kc = min(kx, K - 1);
        unsigned short vb, va;
        if constexpr (TB) vb = bp[kc * g.ldb]; else vb = bp[kc];
        if constexpr (TA) va = ap[kc]; else va = a_bf16(g, ap, il, kc);
        x[e] = (short)(kx < K ? vb : 0);
        y[e] = (short)(kx < K ? va : 0x8000);
      }
      acc = mfma_16<H16>(x, y, acc);
    }
  }
  acc_store<T, Epi, 0, H16>(g, c, acc, i, j0, mv, lane, e);
}

// 8-bit floats (HF8: E4M3, else BF8 = E5M2): lane (i = lane % T, h = lane / T) feeds A(i, k0 + 8 h + e) and B(k0 + 8 h + e, j0 + lane % T), e < 8, per MFMA -- 8
// consecutive k of its row / column, one 64-bit operand: a step is 16 k deep on a 32-tile (32 x 32 x 16, h < 2) and 32 k deep on a 16-tile (16 x 16 x 32, h < 4).
// A is the VNNI-4 image, A(i, k) at byte ((k / 4) * lda + i) * 4 + k % 4, so a lane's 8 k are the two dwords (k0 / 4 + e) * lda + i, e < 2, of a 4-byte aligned
// block (a_vec: wave-uniform, per block), else eight byte loads.  B is flat, B(k, j) at j * ldb + k: one 8-byte load of the column's k run when the block pointer
// and ldb are multiples of 8 (b_vec8), else eight byte loads.  k is a multiple of 4 (dispatch refuses every other k).  Clamping as above: rows / columns beyond
// m / n read row m - 1 / column n - 1 and are never stored; a wide load lies inside a whole step (k0 + 8 <= K); the ragged step reads k = K - 1 beyond K, byte by
// byte, and replaces the value by the padding A = -0 (0x80 in both formats), B = +0.  The last byte touched is ((K / 4 - 1) * lda + m - 1) * 4 + 3 of an A block
// and (n - 1) * ldb + K - 1 of a B block, in the wide and in the byte forms alike; the first is byte 0 of each.
template <bool HF8> __device__ __forceinline__ f32x16 mfma_fp8(long x, long y, f32x16 acc) {
  if constexpr (HF8) return __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(x, y, acc, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf8_bf8(x, y, acc, 0, 0, 0);
}
template <bool HF8> __device__ __forceinline__ f32x4 mfma_fp8(long x, long y, f32x4 acc) {
  if constexpr (HF8) return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(x, y, acc, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8(x, y, acc, 0, 0, 0);
}
__device__ __forceinline__ unsigned char a_fp8(GM const unsigned char* ap, int lda, int i, int kx) { return ap[((long long)(kx >> 2) * lda + i) * 4 + (kx & 3)]; }
// U consecutive MFMA steps of an 8-bit float tile from k = kk on, every operand request ahead of the first MFMA; VEC: both operands are known to take the
// wide loads (no byte-wise code in the instance)
template <int T, int U, bool VEC, bool HF8> __device__ __forceinline__ void steps_fp8(const GemmGroupDesc& g, typename Acc<T>::type& acc, GM const unsigned char* ap, GM const unsigned char* bp,
  int kk, int il, int h, bool a_vec, bool b_vec) {
  constexpr int KS = (T == 32) ? 16 : 32;
  u32x2 x[U], y[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int k0 = kk + u * KS + 8 * h;
    if (VEC || b_vec) x[u] = *(GM const u32x2*)(bp + k0);
    else {
      unsigned int w[2] = {0u, 0u};
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e >> 2] |= (unsigned int)bp[k0 + e] << (8 * (e & 3));
      x[u][0] = w[0]; x[u][1] = w[1];
    }
    if (VEC || a_vec) {
      GM const unsigned int* ap4 = (GM const unsigned int*)ap;
#pragma unroll
      for (int e = 0; e < 2; ++e) y[u][e] = ap4[(long long)((k0 >> 2) + e) * g.lda + il];
    } else {
      unsigned int w[2] = {0u, 0u};
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e >> 2] |= (unsigned int)a_fp8(ap, g.lda, il, k0 + e) << (8 * (e & 3));
      y[u][0] = w[0]; y[u][1] = w[1];
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) acc = mfma_fp8<HF8>(__builtin_bit_cast(long, x[u]), __builtin_bit_cast(long, y[u]), acc);
}
template <int T, bool DEEP, bool HF8, typename Chain>
__device__ __forceinline__ void tile_fp8(const GemmGroupDesc& g, const Chain& ch, gptr c, int i0, int j0, unsigned int lane) {
  constexpr int KS = (T == 32) ? 16 : 32, C8 = HF8 ? 2 : 1;
  const int lr = (int)(lane & (T - 1)), h = (int)(lane / T);
  const int i = i0 + lr, j = j0 + lr;
  const bool mv = i < g.m;
  const int il = min(i, g.m - 1);
  typename Acc<T>::type acc = acc_start<T, NoEpilogue, C8>(g, c, i, j0, mv, lane);
  const int K = g.k;
  const int kbig = K - K % (4 * KS), kfull = K - K % KS;
  gcptr an = nullptr, bn = nullptr;
  if (ch.count) ch.fetch(0, an, bn);
  for (unsigned long long r = 0; r < ch.count; ++r) {
    const gcptr a = an, b = bn;
    ch.fetch(r + 1, an, bn);
    GM const unsigned char* ap = (GM const unsigned char*)a;
    GM const unsigned char* bp = (GM const unsigned char*)b + (long long)min(j, g.n - 1) * g.ldb;
    const bool a_vec = ch.a_vec4(a), b_vec = ch.b_vec8(b);
    int kk = 0;
    if constexpr (DEEP) {                      // segments: four steps per round of requests when both operands take the wide loads (12 more registers)
      if (a_vec && b_vec) for (; kk < kbig; kk += 4 * KS) steps_fp8<T, 4, true, HF8>(g, acc, ap, bp, kk, il, h, true, true);
    }
    for (; kk < kfull; kk += KS) steps_fp8<T, 1, false, HF8>(g, acc, ap, bp, kk, il, h, a_vec, b_vec);
    if (kk < K) {                              // ragged k (whole quads): A = -0 (0x80), B = +0 beyond K
      const int k0 = kk + 8 * h;
      unsigned int xw[2] = {0u, 0u}, yw[2] = {0u, 0u};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int kx = k0 + e, kc = min(kx, K - 1);
        const unsigned int vb = bp[kc], va = a_fp8(ap, g.lda, il, kc);
        xw[e >> 2] |= (kx < K ? vb : 0u) << (8 * (e & 3));
        yw[e >> 2] |= (kx < K ? va : 0x80u) << (8 * (e & 3));
      }
      const u32x2 x = {xw[0], xw[1]}, y = {yw[0], yw[1]};
      acc = mfma_fp8<HF8>(__builtin_bit_cast(long, x), __builtin_bit_cast(long, y), acc);
    }
  }
  acc_store<T, NoEpilogue, C8>(g, c, acc, i, j0, mv, lane);
}

// f64, one 16 x 16 tile: lane (g = lane % 16, s = lane / 16) feeds A(i0 + g, k0 + s) and B(k0 + s, j0 + g) per MFMA and holds C(i0 + g, j0 + s + 4 r) in
// register pair r (the f64 instruction's own map, gemm_f64_kernels.hip).  Same clamping and padding as the f32 tile; k advances in blocks of 32, then 16, then one
// block of up to four ragged steps, every request of a block in flight before its MFMAs.
template <int U, bool TA = false, bool TB = false> __device__ __forceinline__ void steps_f64(f64x4& acc, GM const double* ap, GM const double* bp, int kk, int lda, int s, int ldb = 0) {
  double av[U], bv[U];
#pragma unroll
  for (int e = 0; e < U; ++e) av[e] = ap[k_index<TA>(kk + 4 * e + s, lda)];
#pragma unroll
  for (int e = 0; e < U; ++e) bv[e] = bp[k_index<!TB>(kk + 4 * e + s, ldb)];
#pragma unroll
  for (int e = 0; e < U; ++e) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(bv[e], av[e], acc, 0, 0, 0);
}
template <typename Chain, bool TA = false, bool TB = false> __device__ __forceinline__ void tile_f64(const GemmGroupDesc& g, const Chain& ch, gptr c, int i0, int j0, unsigned int lane) {
  const int lr = (int)(lane & 15u), s = (int)(lane >> 4);
  const int i = i0 + lr, j = j0 + lr;
  const bool mv = i < g.m;
  f64x4 acc;
  static_for<4>([&](auto r) {
    const int jc = j0 + s + 4 * r.value;
    acc[r.value] = (g.beta1 && mv && jc < g.n) ? ((GM const double*)c)[(long long)jc * g.ldc + i] : 0.0;
  });
  const int K = g.k, lda = g.lda, ldb = g.ldb;
  const int kbig = K - K % 32, kfull = K - K % 16;
  gcptr an = nullptr, bn = nullptr;
  if (ch.count) ch.fetch(0, an, bn);
  for (unsigned long long r = 0; r < ch.count; ++r) {
    const gcptr a = an, b = bn;
    ch.fetch(r + 1, an, bn);
    GM const double* ap = (GM const double*)a + lane_index<TA>(min(i, g.m - 1), lda);
    GM const double* bp = (GM const double*)b + lane_index<!TB>(min(j, g.n - 1), g.ldb);
    int kk = 0;
    for (; kk < kbig; kk += 32) steps_f64<8, TA, TB>(acc, ap, bp, kk, lda, s, ldb);
    for (; kk < kfull; kk += 16) steps_f64<4, TA, TB>(acc, ap, bp, kk, lda, s, ldb);
    if (kk < K) {                              // ragged k, up to four steps: A = -0, B = +0 beyond K
      double av[4], bv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kx = kk + 4 * e + s, kc = min(kx, K - 1);
        const double va = ap[k_index<TA>(kc, lda)], vb = bp[k_index<!TB>(kc, ldb)];
        av[e] = kx < K ? va : -0.0; bv[e] = kx < K ? vb : 0.0;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) if (kk + 4 * e < K) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(bv[e], av[e], acc, 0, 0, 0);
    }
  }
  static_for<4>([&](auto r) {
    const int jc = j0 + s + 4 * r.value;
    if (mv && jc < g.n) ((GM double*)c)[(long long)jc * g.ldc + i] = acc[r.value];
  });
}

}  // namespace group_tile
}  // namespace xamd
