// gemm_grouped_kernels.hip -- libxsmm_hip_gemm_batch_grouped: strided batches of SEVERAL (BR)GEMM shapes in one launch.
//
// The host (runtime.cpp) builds one GemmGroupDesc per eligible group -- operands of element 0, element and batch-reduce strides, the shape, the C tile edge
// chosen for it and the exclusive prefix of its work items -- and uploads the table.  A work item is (group, element, C tile); every wave owns one item at a
// time and grid-strides over the rest.  The wave finds its group by a binary search over the prefix column of the table: the item index is wave-uniform, so
// the table is read with scalar loads.  Operands go straight from memory to registers; a wave's tile is private (no LDS, no barrier).
//
// Both operands enter the MFMA swapped (B as the first operand, A as the second), as gemm_tile.hpp does: the accumulator then holds a column of C per register
// and the ROWS of C on the lanes, so every store of a register is a contiguous run of 16 or 32 rows.
//   f32 : v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32 with k in natural order -- the result is the k-ordered fmaf chain bit for bit
//         (cdna_hip_programming.md, "FP32-input MFMA"), which is what oracle_gemm_f32_fma computes [ref: src/generator_gemm_reference_impl.c:1359-1426].
//   bf16: v_mfma_f32_32x32x16_bf16 / v_mfma_f32_16x16x16_bf16, A flat or VNNI-2, B flat, C f32 or bf16 (bf16_cvt.hpp: the reference's conversion exactly).
// STRIDE batch-reduce blocks continue one accumulator chain over (r, k) in the reference's order; beta = 1 starts the chain at C.
// Ragged k is padded with A = -0.0 and B = +0.0: adding the product -0 is an exact identity for every accumulator (+0 + -0 = +0 under round-to-nearest), so the
// f32 chain stays bitwise.  Rows and columns beyond m / n load the last valid row / column and are never stored, so no access leaves the caller's operands.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "internal.hpp"
#include "gemm_device.hpp"
#include "bf16_cvt.hpp"

namespace xamd {

namespace {

// accumulator register r of lane `lane` holds C column (j0 +) acc_col<T>(r, lane), C row (i0 +) lane % T
template <int T> __device__ __forceinline__ int acc_col(int r, unsigned int lane) {
  if constexpr (T == 32) return (r & 3) + 8 * (r >> 2) + 4 * (int)(lane >> 5);
  else return 4 * (int)(lane >> 4) + r;
}

typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <int T> struct Acc;
template <> struct Acc<32> { typedef f32x16 type; static constexpr int N = 16; };
template <> struct Acc<16> { typedef f32x4 type; static constexpr int N = 4; };

__device__ __forceinline__ f32x16 mfma_f32(float x, float y, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, acc, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma_f32(float x, float y, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, acc, 0, 0, 0); }

__device__ __forceinline__ float bf16_bits_to_f32(unsigned short v) { return __uint_as_float((unsigned int)v << 16); }

// the accumulator's start value: C (beta = 1) or +0
template <int T> __device__ __forceinline__ typename Acc<T>::type acc_start(const GemmGroupDesc& g, gptr c, int i, int j0, bool mv, unsigned int lane) {
  typename Acc<T>::type acc;
  static_for<Acc<T>::N>([&](auto r) {
    const int j = j0 + acc_col<T>(r, lane);
    float v = 0.0f;
    if (g.beta1 && mv && j < g.n) {
      const long long o = (long long)j * g.ldc + i;
      v = g.c_bf16 ? bf16_bits_to_f32(((GM const unsigned short*)c)[o]) : ((GM const float*)c)[o];
    }
    acc[r.value] = v;
  });
  return acc;
}

template <int T> __device__ __forceinline__ void acc_store(const GemmGroupDesc& g, gptr c, typename Acc<T>::type acc, int i, int j0, bool mv, unsigned int lane) {
  constexpr int N = Acc<T>::N;
  if (g.c_bf16) {
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

// one C tile of T x T of an f32 element: lane (i = lane % T, h = lane / T) feeds A(i, k0 + h) and B(k0 + h, j0 + lane % T) per MFMA.
// Loads carry no predicate (a predicated load is a branch around it in the code): rows / columns beyond m / n read the last valid row / column -- in bounds,
// never stored -- and k beyond K reads k = K - 1 and replaces the value by the -0 / +0 padding.
template <int T> __device__ __forceinline__ void tile_f32(const GemmGroupDesc& g, gcptr a, gcptr b, gptr c, int i0, int j0, unsigned int lane) {
  constexpr int KS = (T == 32) ? 2 : 4;
  const int lr = (int)(lane & (T - 1)), h = (int)(lane / T);
  const int i = i0 + lr, j = j0 + lr;
  const bool mv = i < g.m;
  typename Acc<T>::type acc = acc_start<T>(g, c, i, j0, mv, lane);
  const int K = g.k, lda = g.lda;
  const int kfull = K - K % (4 * KS);
  for (unsigned long long r = 0; r < g.br_count; ++r) {
    GM const float* ap = (GM const float*)(a + (long long)r * g.br_sa) + min(i, g.m - 1);
    GM const float* bp = (GM const float*)(b + (long long)r * g.br_sb) + (long long)min(j, g.n - 1) * g.ldb;
    int kk = 0;
    for (; kk < kfull; kk += 4 * KS) {
      float av[4], bv[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) av[s] = ap[(kk + s * KS + h) * lda];
      if (T == 32 && g.b_vec16) {              // B(kk .. kk + 7) of the lane's column in two 16-byte pieces; lane half h takes the odd or even k
        const f32x4 q0 = *(GM const f32x4*)(bp + kk), q1 = *(GM const f32x4*)(bp + kk + 4);
        bv[0] = h ? q0[1] : q0[0]; bv[1] = h ? q0[3] : q0[2]; bv[2] = h ? q1[1] : q1[0]; bv[3] = h ? q1[3] : q1[2];
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) bv[s] = bp[kk + s * KS + h];
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = mfma_f32(bv[s], av[s], acc);
    }
    for (; kk < K; kk += KS) {                 // ragged k: A = -0, B = +0 beyond K
      const int kx = kk + h, kc = min(kx, K - 1);
      const float va = ap[kc * lda], vb = bp[kc];
      acc = mfma_f32(kx < K ? vb : 0.0f, kx < K ? va : -0.0f, acc);
    }
  }
  acc_store<T>(g, c, acc, i, j0, mv, lane);
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
template <int T> __device__ __forceinline__ void tile_bf16(const GemmGroupDesc& g, gcptr a, gcptr b, gptr c, int i0, int j0, unsigned int lane) {
  constexpr int E = (T == 32) ? 8 : 4, KS = 16;
  typedef typename Frag<E>::type frag;
  typedef typename Frag<E>::words words;
  const int lr = (int)(lane & (T - 1)), h = (int)(lane / T);
  const int i = i0 + lr, j = j0 + lr;
  const bool mv = i < g.m;
  const int il = min(i, g.m - 1);
  typename Acc<T>::type acc = acc_start<T>(g, c, i, j0, mv, lane);
  const int K = g.k;
  const int kfull = K - K % KS;
  const bool b_vec = (T == 32) ? g.b_vec16 : g.b_vec8;
  for (unsigned long long r = 0; r < g.br_count; ++r) {
    GM const unsigned short* ap = (GM const unsigned short*)(a + (long long)r * g.br_sa);
    GM const unsigned short* bp = (GM const unsigned short*)(b + (long long)r * g.br_sb) + (long long)min(j, g.n - 1) * g.ldb;
    int kk = 0;
    for (; kk < kfull; kk += KS) {
      const int k0 = kk + E * h;
      frag x, y;
      if (b_vec) x = __builtin_bit_cast(frag, *(GM const words*)(bp + k0));
      else {
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = (short)bp[k0 + e];
      }
      if (g.vnni_a && g.a_vec4) {
        GM const unsigned int* ap4 = (GM const unsigned int*)ap;
        words w;
#pragma unroll
        for (int e = 0; e < E / 2; ++e) w[e] = ap4[(long long)((k0 >> 1) + e) * g.lda + il];
        y = __builtin_bit_cast(frag, w);
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) y[e] = (short)a_bf16(g, ap, il, k0 + e);
      }
      acc = mfma_bf16(x, y, acc);
    }
    if (kk < K) {                              // ragged k: A = -0 (0x8000), B = +0 beyond K
      const int k0 = kk + E * h;
      frag x, y;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int kx = k0 + e, kc = min(kx, K - 1);
        const unsigned short vb = bp[kc], va = a_bf16(g, ap, il, kc);
        x[e] = (short)(kx < K ? vb : 0);
        y[e] = (short)(kx < K ? va : 0x8000);
      }
      acc = mfma_bf16(x, y, acc);
    }
  }
  acc_store<T>(g, c, acc, i, j0, mv, lane);
}

}  // namespace

template <bool BF16, typename Table>
__device__ __forceinline__ void grouped_body(const Table& groups, int ngroups, unsigned long long total) {
  const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned int lane = threadIdx.x & 63u;
  const unsigned long long step = (unsigned long long)gridDim.x * 4u;
  for (unsigned long long item = (unsigned long long)blockIdx.x * 4u + wave; item < total; item += step) {
    int lo = 0, hi = ngroups - 1;                // the last group whose first item is <= item (wave-uniform: scalar loads)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (groups[mid].first <= item) lo = mid; else hi = mid - 1;
    }
    const GemmGroupDesc g = groups[lo];
    const unsigned int local = (unsigned int)(item - g.first);        // the host keeps every group below 2^32 items
    const unsigned int tiles = (unsigned int)(g.tiles_m * g.tiles_n);
    const unsigned int e = local / tiles, t = local - e * tiles;
    const unsigned int tm = t % (unsigned int)g.tiles_m, tn = t / (unsigned int)g.tiles_m;
    gcptr a = (gcptr)g.a + (long long)e * g.sa;
    gcptr b = (gcptr)g.b + (long long)e * g.sb;
    gptr c = (gptr)g.c + (long long)e * g.sc;
    if (g.tile == 32) {
      if constexpr (BF16) tile_bf16<32>(g, a, b, c, (int)tm * 32, (int)tn * 32, lane); else tile_f32<32>(g, a, b, c, (int)tm * 32, (int)tn * 32, lane);
    } else {
      if constexpr (BF16) tile_bf16<16>(g, a, b, c, (int)tm * 16, (int)tn * 16, lane); else tile_f32<16>(g, a, b, c, (int)tm * 16, (int)tn * 16, lane);
    }
  }
}

// The table travels in the kernel arguments when it fits (kGroupedInline groups, 3.4 KiB of the 4 KiB argument segment): it arrives with the dispatch packet,
// where an upload is one more command on the stream that the kernel waits for (measured: 7 us of a 14 us call of one 13^3 x 4096 group).  Longer tables
// are uploaded (stage_host) and read through a pointer.  Either way the wave-uniform reads are scalar loads.
struct GroupedInline { GemmGroupDesc g[kGroupedInline]; };
__global__ __launch_bounds__(256) void gemm_grouped_f32_kernel(const GemmGroupDesc* __restrict__ groups, int ngroups, unsigned long long total) { grouped_body<false>(groups, ngroups, total); }
__global__ __launch_bounds__(256) void gemm_grouped_bf16_kernel(const GemmGroupDesc* __restrict__ groups, int ngroups, unsigned long long total) { grouped_body<true>(groups, ngroups, total); }
__global__ __launch_bounds__(256) void gemm_grouped_f32_inline_kernel(GroupedInline tab, int ngroups, unsigned long long total) { grouped_body<false>(tab.g, ngroups, total); }
__global__ __launch_bounds__(256) void gemm_grouped_bf16_inline_kernel(GroupedInline tab, int ngroups, unsigned long long total) { grouped_body<true>(tab.g, ngroups, total); }

const char* gemm_grouped_kernel_name(int bf16) { return bf16 ? "gemm_grouped_bf16_kernel" : "gemm_grouped_f32_kernel"; }

int launch_gemm_grouped(const GemmGroupDesc* table, int ngroups, unsigned long long items, int bf16, void* stream) {
  if (ngroups <= 0 || items == 0) return 0;
  // one wave per item up to 32 768 workgroups (16 rounds of the chip's resident waves); beyond that the waves grid-stride
  const unsigned int grid = (unsigned int)std::min<unsigned long long>((items + 3) / 4, 32768ull);
  hipStream_t st = (hipStream_t)stream;
  if (bf16) hipLaunchKernelGGL(gemm_grouped_bf16_kernel, dim3(grid), dim3(256), 0, st, table, ngroups, items);
  else hipLaunchKernelGGL(gemm_grouped_f32_kernel, dim3(grid), dim3(256), 0, st, table, ngroups, items);
  return (int)hipGetLastError();
}
int launch_gemm_grouped_inline(const GemmGroupDesc* host_table, int ngroups, unsigned long long items, int bf16, void* stream) {
  if (ngroups <= 0 || items == 0) return 0;
  if (ngroups > kGroupedInline) return (int)hipErrorInvalidValue;
  GroupedInline tab;
  std::memset(&tab, 0, sizeof(tab));
  std::memcpy(tab.g, host_table, (size_t)ngroups * sizeof(GemmGroupDesc));
  const unsigned int grid = (unsigned int)std::min<unsigned long long>((items + 3) / 4, 32768ull);
  hipStream_t st = (hipStream_t)stream;
  if (bf16) hipLaunchKernelGGL(gemm_grouped_bf16_inline_kernel, dim3(grid), dim3(256), 0, st, tab, ngroups, items);
  else hipLaunchKernelGGL(gemm_grouped_f32_inline_kernel, dim3(grid), dim3(256), 0, st, tab, ngroups, items);
  return (int)hipGetLastError();
}

}  // namespace xamd
