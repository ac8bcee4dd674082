"""Strided batches of matrix equations (libxsmm_hip_meqn_batch_strided) without a GPU.

Host emulation: the dry-run library generates the single-call kernel at dispatch and its batched form (`..._b`) at the first batched call
(LIBXSMM_HIP_JIT_DUMP keeps both); clang builds each for x86-64 with the JIT's -ffp-contract=off (as tests/test_jit_emulated_cpu.py does), and a
loop over (element blocks x workgroups x threads) is the launch.  The phased form runs its workgroups one after another, each as 256 host threads
with a pthread barrier for __syncthreads.  Both forms are emulated with fewer element blocks than elements, so the kernels' grid-stride loop over
elements runs too.  Every element of the batch must equal, bit for bit, the single-call kernel run on that element's pointers, and lie within the
tests' bound of the oracle composition.

Validation: the refusals of the batched entry set the documented error codes in dry-run mode, before the missing device is noticed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import normf_rel
from libxsmm_amd.capi import DT
from meqn_batch_helpers import Batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
needs_hiprtc = pytest.mark.skipif(not (os.path.exists("/opt/rocm/lib/libhiprtc.so") and os.path.exists(CLANG)), reason="needs hiprtc and clang")
COUNT = 5

CHILD = r"""
import sys
import ctypes as C
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from libxsmm_amd import capi
import test_meqn as tm
api = capi.load()
tree, shapes, out = tm.CASES[%(case)r]
h = api.dispatch_meqn(tm.build(api, tree, shapes), capi.MeqnArgShape(*out))
print("KERNEL " + (api.hip_kernel_name(h, 0).decode() if h else "NULL"))
inputs = (capi.MatrixArg * len(shapes))()
for i in range(len(shapes)):
    inputs[i].primary = 4096 * (i + 1)
p = capi.MeqnParam()
p.inputs = inputs
p.output.primary = 65536
strides = (C.c_longlong * len(shapes))(*([16] * len(shapes)))
api.hip_meqn_batch_strided(h, C.byref(p), %(count)d, len(shapes), strides, 1024, 0, 0, None)
print("ERROR %%d" %% api.hip_get_last_error())
"""

PRELUDE = """
#include <cmath>
#include <cstring>
struct Idx3 { unsigned int x, y, z; };
static Idx3 blockIdx, gridDim, threadIdx;
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(n)
static inline unsigned int __float_as_uint(float x) { unsigned int u; std::memcpy(&u, &x, 4); return u; }
static inline float __uint_as_float(unsigned int u) { float x; std::memcpy(&x, &u, 4); return x; }
"""
PHASED_PRELUDE = PRELUDE.replace("static Idx3 blockIdx, gridDim, threadIdx;", "static Idx3 blockIdx, gridDim; static thread_local Idx3 threadIdx;") + """
#include <pthread.h>
static pthread_barrier_t g_barrier;
#define __shared__ static
#define __syncthreads() pthread_barrier_wait(&g_barrier)
"""
# element-wise: blocks of 256 threads along x (the units), element blocks along y
EW_DRIVER = """
extern "C" int emulate(void** a, long long* s, long long count, unsigned int gy) {
  gridDim.x = BLOCKS; gridDim.y = gy;
  for (unsigned int y = 0; y < gy; ++y) for (long long t = 0; t < BLOCKS * 256LL; ++t) {
    blockIdx.x = (unsigned int)(t / 256); blockIdx.y = y; threadIdx.x = (unsigned int)(t % 256);
    KERNEL(ARGS);
  }
  return 0;
}
"""
# phased: one workgroup of 256 threads per element block, the workgroups one after another
PHASED_DRIVER = """
struct Launch { void** a; long long* s; long long count; unsigned int tid; };
static void* thread_main(void* p) { Launch* l = (Launch*)p; threadIdx.x = l->tid; void** a = l->a; long long* s = l->s; long long count = l->count; (void)s; (void)count; KERNEL(ARGS); return nullptr; }
extern "C" int emulate(void** a, long long* s, long long count, unsigned int gx) {
  gridDim.x = gx; gridDim.y = 1;
  for (unsigned int bx = 0; bx < gx; ++bx) {
    blockIdx.x = bx;
    pthread_t th[256]; Launch l[256];
    pthread_attr_t attr; pthread_attr_init(&attr); pthread_attr_setstacksize(&attr, 256 * 1024);
    pthread_barrier_init(&g_barrier, nullptr, 256);
    for (unsigned int t = 0; t < 256; ++t) { l[t].a = a; l[t].s = s; l[t].count = count; l[t].tid = t; if (pthread_create(&th[t], &attr, thread_main, &l[t]) != 0) return 1; }
    for (unsigned int t = 0; t < 256; ++t) pthread_join(th[t], nullptr);
    pthread_barrier_destroy(&g_barrier);
  }
  return 0;
}
"""


def _dry_env(tmp_path):
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1", LIBXSMM_HIP_JIT="2", LIBXSMM_HIP_JIT_DUMP=str(tmp_path))
    env.pop("LIBXSMM_VERBOSE", None)
    return env


def _params(src, kernel):
    sig = re.search(r"void " + kernel + r"\(([^)]*)\)", src).group(1)
    return [p.strip().split()[-1] for p in sig.split(",")]


def _build(tmp_path, src, kernel, phased, nptr, nstride, tag):
    host = re.sub(r"#define GM .*", "#define GM", src)
    if kernel.endswith("_b"):
        args = ", ".join([f"a[{i}]" for i in range(nptr)] + [f"s[{i}]" for i in range(nstride)] + ["count"])
    else:
        args = ", ".join(f"a[{i}]" for i in range(nptr))
    if phased:
        driver = PHASED_DRIVER.replace("KERNEL", kernel).replace("ARGS", args)
    else:
        total = int(re.search(r"if \(t >= (\d+)LL\) return;", src).group(1))
        driver = EW_DRIVER.replace("KERNEL", kernel).replace("ARGS", args).replace("BLOCKS", str((total + 255) // 256))
    cpp = tmp_path / f"{tag}.cpp"
    cpp.write_text((PHASED_PRELUDE if phased else PRELUDE) + host + driver)
    so = str(tmp_path / f"{tag}.so")
    c = subprocess.run([CLANG, "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off", "-mfma", "-shared", "-fPIC", "-pthread", str(cpp), "-o", so],
                       capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-3000:]
    lib = C.CDLL(so)
    lib.emulate.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_uint]
    lib.emulate.restype = C.c_int
    return lib


# the shared (stride 0) input positions of each case: a mix of stepped and shared operands, per-element and shared scalars
SHARED = {"simple": (1,), "layernorm_affine": (2, 3, 4), "bias_relu_bf16": (0,), "softmax_fwd": (), "reduce_bcast": (), "dot_to_scalar": (1,)}


@needs_hiprtc
@pytest.mark.parametrize("case", sorted(SHARED))
def test_batched_equation_kernel_equals_the_single_call_kernel_per_element(tmp_path, case):
    import test_meqn as tm
    tree, shapes, out_shape = tm.CASES[case]
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "case": case, "count": COUNT}],
                       capture_output=True, text=True, timeout=600, env=_dry_env(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    kernel = [ln for ln in r.stdout.splitlines() if ln.startswith("KERNEL ")][-1][7:]
    assert kernel.startswith("meqn_jit_"), kernel
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("ERROR ")][-1] == "ERROR -4"        # generated, then refused: no device
    phased = kernel.startswith("meqn_jit_r")
    single_src = open(tmp_path / (kernel + ".hip")).read()
    batch_src = open(tmp_path / (kernel + "_b.hip")).read()
    nin = len(shapes)
    assert _params(single_src, kernel) == [f"in{i}" for i in range(nin)] + ["out"]
    assert _params(batch_src, kernel + "_b") == [f"in{i}_" for i in range(nin)] + ["out_"] + [f"s_in{i}" for i in range(nin)] + ["s_out", "count"]
    single = _build(tmp_path, single_src, kernel, phased, nin + 1, 0, "single")
    batched = _build(tmp_path, batch_src, kernel + "_b", phased, nin + 1, nin + 1, "batched")

    b = Batch(shapes, out_shape, COUNT, shared=SHARED[case], seed=17)
    assert any(s == 0 for s in b.strides) == bool(SHARED[case]) and b.out_stride > b.out_foot
    out = b.new_out()
    ptrs = (C.c_void_p * (nin + 1))(*[a.ctypes.data for a in b.inputs], out.ctypes.data)
    strides = (C.c_longlong * (nin + 1))(*b.strides, b.out_stride)
    assert batched.emulate(ptrs, strides, COUNT, 2) == 0           # two element blocks for five elements: the grid-stride loop runs
    odt = out_shape[3]
    bound = tm.BY_NORM.get(case, 1e-6 if odt == DT.F32 else 8e-3)
    if phased:
        bound = max(bound, 1e-5 if odt == DT.F32 else 8e-3)
    gap = np.ones(out.size, dtype=bool)
    for i in range(COUNT):
        arrays = [b.element(k, i) for k in range(nin)]
        want = np.zeros(b.out_foot // out.itemsize, dtype=out.dtype)
        one = (C.c_void_p * (nin + 1))(*[a.ctypes.data for a in arrays], want.ctypes.data)
        assert single.emulate(one, None, 1, 1) == 0
        got = b.out_element(out, i)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"element {i} differs from the single call"
        ref = tm.evaluate(tree, shapes, arrays, out_shape)
        assert normf_rel(tm._valid(ref, out_shape), tm._valid(got, out_shape), odt) <= bound, i
        off = i * b.out_stride // out.itemsize
        gap[off:off + want.size] = False
    assert not out[gap].any()                                                # nothing written between the elements' outputs


VALIDATION_CHILD = r"""
import sys
import ctypes as C
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from libxsmm_amd import capi
from libxsmm_amd.capi import BINARY, DT
import test_meqn as tm
api = capi.load()
ll = C.c_longlong
def err():
    e = api.hip_get_last_error(); api.hip_clear_last_error(); return e
tree, shapes, out = tm.CASES["simple"]
h = api.dispatch_meqn(tm.build(api, tree, shapes), capi.MeqnArgShape(*out))
assert h
inputs = (capi.MatrixArg * 4)()
for i in range(4):
    inputs[i].primary = 4096 * (i + 1)
p = capi.MeqnParam(); p.inputs = inputs; p.output.primary = 65536
s4 = (ll * 4)(16, 0, 32, 48)
api.hip_meqn_batch_strided(h, C.byref(p), 0, 4, s4, 64, 0, 0, None); print("count0", err())
api.hip_meqn_batch_strided(h, C.byref(p), 3, 3, s4, 64, 0, 0, None); print("ninputs", err())
api.hip_meqn_batch_strided(h, C.byref(p), 3, 4, None, 64, 0, 0, None); print("nostrides", err())
api.hip_meqn_batch_strided(h, C.byref(p), 3, 4, s4, 64, 0, 0, None); print("valid", err())
api.hip_meqn_batch_strided(None, C.byref(p), 3, 4, s4, 64, 0, 0, None); print("null", err())
g = api.dispatch_gemm(capi.gemm_shape(32, 32, 32, 32, 32, 32, DT.F32, DT.F32, DT.F32, DT.F32), 0, 0)
assert g
api.hip_meqn_batch_strided(g, C.byref(p), 3, 4, s4, 64, 0, 0, None); print("gemm_handle", err())
# a BRGEMM node: its block count (ops_args[3].tertiary) is shared by all elements
m, n, k, blocks = 32, 16, 24, 5
idx = api.meqn_create()
md = lambda pos=-1: capi.MeqnMetadata(idx, pos)
assert api.meqn_push_back_binary_op(md(), BINARY.ADD, DT.F32, 0) == 0
assert api.meqn_push_back_arg(md(0), capi.MeqnArgShape(m, n, m, DT.F32), tm.SINGULAR) == 0
assert api.meqn_push_back_binary_op(md(3), BINARY.BRGEMM, DT.F32, 0) == 0
assert api.meqn_push_back_arg(md(2), capi.MeqnArgShape(m, k, m, DT.F32), capi.MatrixArgAttributes(1, 3, blocks, m * k * 4)) == 0
assert api.meqn_push_back_arg(md(3), capi.MeqnArgShape(k, n, k, DT.F32), capi.MatrixArgAttributes(1, 3, blocks, k * n * 4)) == 0
hb = api.dispatch_meqn(idx, capi.MeqnArgShape(m, n, m, DT.F32))
assert hb
ops = (ll * 4)(0, 0, 0, 0)
api.hip_meqn_batch_strided(hb, C.byref(p), 3, 4, s4, 64, 0, 4, ops); print("brgemm_shared", err())
ops[3] = 8
api.hip_meqn_batch_strided(hb, C.byref(p), 3, 4, s4, 64, 0, 4, ops); print("brgemm_stepped", err())
api.hip_meqn_batch_strided(hb, C.byref(p), 3, 4, s4, 64, 0, 3, ops); print("brgemm_beyond_nops", err())
"""


def test_batched_entry_refusals_set_the_documented_error_codes(tmp_path):
    r = subprocess.run([sys.executable, "-c", VALIDATION_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                       capture_output=True, text=True, timeout=600, env=_dry_env(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(ln.split() for ln in r.stdout.splitlines() if len(ln.split()) == 2)
    assert got == {"count0": "0",               # nothing to do
                   "ninputs": "-2",             # fewer input strides than the equation's input positions
                   "nostrides": "-2",
                   "valid": "-4",               # accepted and generated; then: no device
                   "null": "-3", "gemm_handle": "-3",          # not an equation handle
                   "brgemm_shared": "-4",
                   "brgemm_stepped": "-3",      # a stride on the shared BRGEMM block count
                   "brgemm_beyond_nops": "-4"}, r.stdout + r.stderr   # positions from nops_args on have stride 0
