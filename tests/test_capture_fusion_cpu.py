"""Capture-time fusion of independent strided-batch launches, the parts that need no GPU.

The independence predicate lives in a header without HIP dependencies (libxsmm_amd/csrc/capture_fuse.hpp): a small C++ program is compiled against it and
checks a table of cases.  The interface (libxsmm_hip_set_capture_fusion, libxsmm_hip_fused_launch_count, LIBXSMM_HIP_CAPTURE_FUSION) is exercised through
the ctypes bindings in dry-run mode."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libxsmm_amd", "csrc")
LIB = os.path.join(ROOT, "libxsmm_amd", "lib", "libxsmm_amd.so")

PROGRAM = r"""
#include "capture_fuse.hpp"
#include <cstdio>
using namespace xamd;
static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// one launch of `count` f32 32 x 32 x (32 kchunks) problems, NN, as the lean launcher describes it
static bool launch(FuseLaunch* l, uintptr_t a, uintptr_t b, uintptr_t c, unsigned long long count, long long sa, long long sb, long long sc,
                   unsigned lda = 32, unsigned ldb = 32, unsigned ldc = 32, unsigned long long br = 1, long long brs = 4096) {
  size_t ea, eb, ec;
  if (!fuse_extent(br, brs, lda, 32, 4, &ea) || !fuse_extent(br, brs, ldb, 32, 4, &eb) || !fuse_extent(1, 0, ldc, 32, 4, &ec)) return false;
  return fuse_range(a, count, sa, ea, &l->a) && fuse_range(b, count, sb, eb, &l->b) && fuse_range(c, count, sc, ec, &l->c);
}

int main() {
  const uintptr_t base = 0x7f0000000000ull;
  const long long blk = 4096;
  // ranges_overlap itself: half-open intervals
  CHECK(ranges_overlap(100, 10, 105, 10));
  CHECK(!ranges_overlap(100, 10, 110, 10));            // touching
  CHECK(ranges_overlap(100, 10, 109, 10));             // one byte
  CHECK(!ranges_overlap(110, 10, 100, 10));
  CHECK(ranges_overlap(100, 1, 100, 1));
  {  // disjoint sets
    FuseLaunch p, q;
    CHECK(launch(&p, base, base + 0x100000, base + 0x200000, 64, blk, blk, blk));
    CHECK(launch(&q, base + 0x300000, base + 0x400000, base + 0x500000, 64, blk, blk, blk));
    CHECK(p.a.len == 64 * 4096 && p.c.len == 64 * 4096);
    CHECK(fuse_independent(q, &p, 1) && fuse_independent(p, &q, 1));
  }
  {  // touching: q's C begins at the byte where p's A ends; one element earlier it overlaps; one byte earlier too
    FuseLaunch p, q;
    CHECK(launch(&p, base, base + 0x100000, base + 0x200000, 5, blk, blk, blk));
    CHECK(launch(&q, base + 0x300000, base + 0x400000, base + 5 * blk, 5, blk, blk, blk));
    CHECK(fuse_independent(q, &p, 1));
    CHECK(launch(&q, base + 0x300000, base + 0x400000, base + 5 * blk - 4, 5, blk, blk, blk));
    CHECK(!fuse_independent(q, &p, 1));                // write-after-read
    CHECK(!fuse_independent(p, &q, 1));                // the other order: read-after-write
    CHECK(launch(&q, base + 0x300000, base + 0x400000, base + 5 * blk - 1, 5, blk, blk, blk));
    CHECK(!fuse_independent(q, &p, 1));
    // q's C ENDS where p's B begins
    CHECK(launch(&q, base + 0x300000, base + 0x400000, base + 0x100000 - 5 * blk, 5, blk, blk, blk));
    CHECK(fuse_independent(q, &p, 1));
  }
  {  // hazards by kind
    FuseLaunch p, q;
    CHECK(launch(&p, base, base + 0x100000, base + 0x200000, 16, blk, blk, blk));
    CHECK(launch(&q, base + 0x200000, base + 0x400000, base + 0x500000, 16, blk, blk, blk));      // reads p's C through A
    CHECK(!fuse_independent(q, &p, 1));
    CHECK(launch(&q, base + 0x300000, base + 0x200000, base + 0x500000, 16, blk, blk, blk));      // reads p's C through B
    CHECK(!fuse_independent(q, &p, 1));
    CHECK(launch(&q, base + 0x300000, base + 0x400000, base + 0x200000, 16, blk, blk, blk));      // writes p's C
    CHECK(!fuse_independent(q, &p, 1));
    CHECK(launch(&q, base + 0x300000, base + 0x400000, base + 0x100000, 16, blk, blk, blk));      // writes p's B
    CHECK(!fuse_independent(q, &p, 1));
    CHECK(launch(&q, base, base + 0x100000, base + 0x500000, 16, blk, blk, blk));                 // shares both inputs: reads never conflict
    CHECK(fuse_independent(q, &p, 1));
  }
  {  // a hazard with ANY launch of the node counts, not only with the last one
    FuseLaunch node[3], q;
    for (int i = 0; i < 3; ++i) CHECK(launch(&node[i], base + i * 0x1000000ull, base + i * 0x1000000ull + 0x100000, base + i * 0x1000000ull + 0x200000, 16, blk, blk, blk));
    CHECK(launch(&q, base + 0x8000000, base + 0x8100000, base + 0x200000, 16, blk, blk, blk));    // C of the FIRST
    CHECK(!fuse_independent(q, node, 3));
    CHECK(fuse_independent(q, node + 1, 2));
    CHECK(fuse_independent(q, node, 0));
  }
  {  // stride 0 (one B for the whole batch): its range is one block; count 1: the stride does not matter
    FuseLaunch p, q;
    CHECK(launch(&p, base, base + 0x100000, base + 0x200000, 64, blk, 0, blk));
    CHECK(p.b.len == 4096);
    CHECK(launch(&q, base + 0x300000, base + 0x100000, base + 0x100000 + blk, 64, blk, 0, blk));  // q writes just behind the shared B
    CHECK(fuse_independent(q, &p, 1));
    CHECK(launch(&q, base + 0x300000, base + 0x100000, base + 0x100000 + blk - 4, 64, blk, 0, blk));
    CHECK(!fuse_independent(q, &p, 1));
    CHECK(launch(&p, base, base + 0x100000, base + 0x200000, 1, 1ll << 40, 1ll << 40, 1ll << 40));
    CHECK(p.a.len == 4096 && p.b.len == 4096 && p.c.len == 4096);
  }
  {  // padded leading dimensions and a chain of three blocks: extent = (br - 1) * br_stride + ld * 32 * 4, the pad rows of the last column included
    FuseLaunch p, q;
    const long long sa = 3 * 36 * 32 * 4, sb = 3 * 40 * 32 * 4, sc = 48 * 32 * 4;
    CHECK(launch(&p, base, base + 0x1000000, base + 0x2000000, 67, sa, sb, sc, 36, 40, 48, 3, 36 * 32 * 4));
    CHECK(p.a.len == (size_t)(66 * sa + 2 * 36 * 32 * 4 + 36 * 32 * 4));
    CHECK(launch(&p, base, base + 0x1000000, base + 0x2000000, 67, sa, sb, sc, 36, 40, 48, 3, 40 * 32 * 4));
    CHECK(p.b.len == (size_t)(66 * sb + 2 * 40 * 32 * 4 + 40 * 32 * 4));
    CHECK(p.c.len == (size_t)(66 * sc + 48 * 32 * 4));
    CHECK(launch(&q, base + 0x3000000, base + 0x4000000, base + 0x2000000 + 67 * sc, 67, sa, sb, sc, 36, 40, 48, 3, 36 * 32 * 4));
    CHECK(fuse_independent(q, &p, 1));
    CHECK(launch(&q, base + 0x3000000, base + 0x4000000, base + 0x2000000 + 67 * sc - 4, 67, sa, sb, sc, 36, 40, 48, 3, 36 * 32 * 4));
    CHECK(!fuse_independent(q, &p, 1));                // only pad rows overlap: the bounding interval still refuses
  }
  {  // negative strides are refused, a zero count as well
    FuseLaunch p;
    CHECK(!launch(&p, base, base + 0x100000, base + 0x200000, 16, -blk, blk, blk));
    CHECK(!launch(&p, base, base + 0x100000, base + 0x200000, 16, blk, blk, -blk));
    CHECK(!launch(&p, base, base + 0x100000, base + 0x200000, 16, blk, blk, blk, 32, 32, 32, 3, -4096));
    CHECK(launch(&p, base, base + 0x100000, base + 0x200000, 16, blk, blk, blk, 32, 32, 32, 1, -4096));   // one block: the chain stride is not used
    CHECK(!launch(&p, base, base + 0x100000, base + 0x200000, 0, blk, blk, blk));
  }
  CHECK(kFuseCap >= 2 && kFuseCap * 32 <= 1024);
  std::printf("%s\n", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
"""


def test_independence_predicate_table(tmp_path):
    src = tmp_path / "fuse_cases.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "fuse_cases")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + CSRC, str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
from libxsmm_amd import capi
api = capi.load()
api.init()
cap = api.hip_set_capture_fusion(0)
print("default", cap)
print("after_off", api.hip_set_capture_fusion(1))
print("after_one", api.hip_set_capture_fusion(1000))
print("capped", api.hip_set_capture_fusion(5))
print("five", api.hip_set_capture_fusion(-3))
print("negative", api.hip_set_capture_fusion(cap))
print("fused", api.hip_fused_launch_count(1), api.hip_fused_launch_count(0))
"""


@pytest.mark.skipif(not os.path.exists(LIB), reason="needs the built library")
@pytest.mark.parametrize("env_value", [None, "0", "1", "4", "1000"])
def test_interface_in_dry_run_mode(env_value):
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1")
    env.pop("LIBXSMM_HIP_CAPTURE_FUSION", None)
    if env_value is not None:
        env["LIBXSMM_HIP_CAPTURE_FUSION"] = env_value
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.split()}
    cap = got["default"][0] if env_value in (None, "1000") else None
    if env_value is None or env_value == "1000":
        assert cap in (8, 16)                                   # on by default, at the cap; an environment value above the cap is capped
    elif env_value == "4":
        assert got["default"] == [4]
    else:
        assert got["default"] == [0]                            # 0 and 1 both mean off
    assert got["after_off"] == [0]                              # the setter returns the previous value
    assert got["after_one"] == [0]                              # 1 is off as well
    assert got["capped"][0] in (8, 16) and (cap is None or got["capped"][0] == cap)
    assert got["five"] == [5]
    assert got["negative"] == [0]                               # negative values mean off
    assert got["fused"] == [0, 0]
