// capture_fuse.hpp -- when may a launch that is being captured into a graph be folded into the kernel node of the launch before it?  
// Host arithmetic only, no HIP types: the launcher (gemm_lean_kernels.hip), the coalescing queue (runtime.cpp) and a stand-alone test program
// (tests/test_capture_fusion_cpu.py) include it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace xamd {

// launches one graph node holds at most (the kernel's by-value table has this many entries of 32 bytes)
#ifndef XAMD_FUSE_CAP
#define XAMD_FUSE_CAP 16
#endif
constexpr int kFuseCap = XAMD_FUSE_CAP;

// half-open byte ranges [a0, a0 + an) and [b0, b0 + bn): ranges that only touch (one ends where the other begins) do not overlap
inline bool ranges_overlap(uintptr_t a0, size_t an, uintptr_t b0, size_t bn) { return a0 < b0 + bn && b0 < a0 + an; }

struct FuseRange { uintptr_t lo = 0; size_t len = 0; };
// the bytes one strided launch reads through A and B and writes through C, as bounding intervals
struct FuseLaunch { FuseRange a, b, c; };

// Bounding interval of `count` elements that lie `stride` bytes apart and span `extent` bytes each: base ... base + (count - 1) * stride + extent.
// It covers the gaps between the elements as well: overestimating can only refuse a fold.  false: a negative stride (such launches are never folded).
inline bool fuse_range(uintptr_t base, unsigned long long count, long long stride, size_t extent, FuseRange* out) {
  if (stride < 0 || count == 0) return false;
  out->lo = base;
  out->len = (size_t)(count - 1) * (size_t)stride + extent;
  return true;
}

// bytes one problem reads through A / B (a chain of `br_count` blocks `br_stride` bytes apart, each `ld` x `cols` elements) or writes through C (br_count 1)
inline bool fuse_extent(unsigned long long br_count, long long br_stride, unsigned long long ld, unsigned long long cols, size_t typesize, size_t* out) {
  if (br_count == 0 || (br_count > 1 && br_stride < 0)) return false;
  *out = (size_t)(br_count - 1) * (size_t)(br_count > 1 ? br_stride : 0) + (size_t)ld * (size_t)cols * typesize;
  return true;
}

// `next` may run concurrently with the `n` launches already in the node: it writes nothing they read or write, and reads nothing they write
inline bool fuse_independent(const FuseLaunch& next, const FuseLaunch* node, int n) {
  for (int i = 0; i < n; ++i) {
    const FuseLaunch& q = node[i];
    if (ranges_overlap(next.c.lo, next.c.len, q.a.lo, q.a.len) || ranges_overlap(next.c.lo, next.c.len, q.b.lo, q.b.len) ||
        ranges_overlap(next.c.lo, next.c.len, q.c.lo, q.c.len)) return false;                              // write-after-read, write-after-write
    if (ranges_overlap(q.c.lo, q.c.len, next.a.lo, next.a.len) || ranges_overlap(q.c.lo, q.c.len, next.b.lo, next.b.len)) return false;   // read-after-write
  }
  return true;
}

// What a thread remembers of the last lean launch it issued into a stream capture: the kernel node the launch became and everything a later launch has to
// match to be folded into that node.  HIP handles are kept as plain pointers (this header has no HIP dependency).
struct FuseKey {           // the kernel arguments apart from the three bases, and what selects the kernel instance
  const void* handle = nullptr;
  unsigned int bs_a = 0, bs_b = 0, bs_c = 0, nbatch = 0, lda = 0, ldb = 0, ldc = 0, nchunks = 0, kchunks = 0;
  long long brs_a = 0, brs_b = 0;
  int pol = 0, ta = 0, tb = 0;
  bool operator==(const FuseKey& o) const {
    return handle == o.handle && bs_a == o.bs_a && bs_b == o.bs_b && bs_c == o.bs_c && nbatch == o.nbatch && lda == o.lda && ldb == o.ldb && ldc == o.ldc &&
           nchunks == o.nchunks && kchunks == o.kchunks && brs_a == o.brs_a && brs_b == o.brs_b && pol == o.pol && ta == o.ta && tb == o.tb;
  }
};
struct FuseEntry { const void* a; const void* b; void* c; unsigned long long pad; };       // one launch's bases: 32 bytes of the kernel's table
struct FuseState {
  int n = 0;                              // launches in the node (0: nothing to fold into)
  unsigned long long capture_id = 0;
  void* stream = nullptr;                 // hipStream_t
  void* node = nullptr;                   // hipGraphNode_t
  FuseKey key;
  FuseEntry entry[kFuseCap];
  FuseLaunch range[kFuseCap];
  const void* handle = nullptr;           // set by run_gemm around the one launch of a plain strided-batch call; nullptr: this launch is not a candidate
  unsigned long long folded = 0;          // libxsmm_hip_fused_launch_count
};

}  // namespace xamd
