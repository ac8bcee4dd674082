"""Accumulating batches of matrix equations (libxsmm_hip_meqn_batch_strided_accumulate) without a GPU.

Host emulation as in tests/test_meqn_batch_cpu.py: the dry-run library generates the single-call kernel at dispatch and the carried (`_c`), sliced (`_s`)
and combine kernels at the first accumulating call (LIBXSMM_HIP_JIT_DUMP keeps them); clang builds each for x86-64 with the JIT's -ffp-contract=off and a
loop over (grid.y x workgroups x threads) is the launch.

1. The carried kernel on 5 elements (one full group of 4 whose loads are issued ahead, and the remainder loop) equals, bit for bit, 5 successive
   emulations of the single-call kernel that read and write the same output.  A thread of the carried form owns its 8-row unit for the whole batch, so the
   grid is exactly the units (there is no loop over units that a smaller grid would exercise); the sliced kernel's loop over slices is run with fewer
   blocks along y than slices.
2. The sliced kernel followed by the combine kernel, S in {1, 2, 3} over 7 elements (slices of unequal length), equals the numpy restatement of the
   documented order of additions, bit for bit.
3. Every refusal of the entry sets its documented error code in dry-run mode, before the missing device is noticed.
4. (The single-call and `_b` sources of the existing cases are unchanged: tests/test_meqn_batch_cpu.py pins their signatures.)"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from meqn_acc_helpers import CASES, SLICEABLE, AccBatch, leaf_order, sliced_restatement
from test_meqn_batch_cpu import CLANG, PRELUDE, ROOT, _dry_env, _params, needs_hiprtc

CHILD = r"""
import sys
import ctypes as C
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from libxsmm_amd import capi
import test_meqn as tm
from meqn_acc_helpers import CASES
api = capi.load()
tree, shapes, out, carried = CASES[%(case)r]
h = api.dispatch_meqn(tm.build(api, tree, shapes), capi.MeqnArgShape(*out))
print("KERNEL " + (api.hip_kernel_name(h, 0).decode() if h else "NULL"))
inputs = (capi.MatrixArg * len(shapes))()
for i in range(len(shapes)):
    inputs[i].primary = 4096 * (i + 1)
p = capi.MeqnParam()
p.inputs = inputs
p.output.primary = inputs[carried].primary
strides = (C.c_longlong * len(shapes))(*[0 if i == carried else 16 for i in range(len(shapes))])
api.hip_meqn_batch_strided_accumulate(h, C.byref(p), 7, len(shapes), strides, 0, None, %(order)d)
print("ERROR %%d" %% api.hip_get_last_error())
"""

DRIVER = """
extern "C" int emulate(void** a, long long* s, long long count, long long slices, unsigned int gy) {
  (void)s; (void)count; (void)slices;
  gridDim.x = BLOCKS; gridDim.y = gy;
  for (unsigned int y = 0; y < gy; ++y) for (long long t = 0; t < BLOCKS * 256LL; ++t) {
    blockIdx.x = (unsigned int)(t / 256); blockIdx.y = y; threadIdx.x = (unsigned int)(t % 256);
    KERNEL(ARGS);
  }
  return 0;
}
"""


def _generate(tmp_path, case, order):
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "case": case, "order": order}],
                       capture_output=True, text=True, timeout=600, env=_dry_env(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    kernel = [ln for ln in r.stdout.splitlines() if ln.startswith("KERNEL ")][-1][7:]
    assert kernel.startswith("meqn_jit_e"), kernel
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("ERROR ")][-1] == "ERROR -4"        # generated, then refused: no device
    return kernel


def _build(tmp_path, kernel, args):
    src = open(tmp_path / (kernel + ".hip")).read()
    host = re.sub(r"#define GM .*", "#define GM", src)
    total = int(re.search(r"if \(t >= (\d+)LL\) return;", src).group(1))
    driver = DRIVER.replace("KERNEL", kernel).replace("ARGS", ", ".join(args)).replace("BLOCKS", str((total + 255) // 256))
    cpp = tmp_path / f"{kernel}.cpp"
    cpp.write_text(PRELUDE + host + driver)
    so = str(tmp_path / f"{kernel}.so")
    c = subprocess.run([CLANG, "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off", "-mfma", "-shared", "-fPIC", str(cpp), "-o", so], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-3000:]
    lib = C.CDLL(so)
    lib.emulate.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_uint]
    lib.emulate.restype = C.c_int
    return lib, src


class Guarded:
    """The output between two guard regions; `inside` is the (n, ld) view the kernels see."""
    GUARD = 64

    def __init__(self, acc0):
        guard = np.full(self.GUARD, 0x5A5A if acc0.dtype == np.uint16 else -77.0, dtype=acc0.dtype)
        self.buf = np.concatenate([guard, acc0, guard])
        self.before, self.after = guard.copy(), guard.copy()
        self.inside = self.buf[self.GUARD:self.GUARD + acc0.size]

    def intact(self):
        return np.array_equal(self.buf[:self.GUARD], self.before) and np.array_equal(self.buf[-self.GUARD:], self.after)


def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


@needs_hiprtc
@pytest.mark.parametrize("case", sorted(CASES))
def test_carried_kernel_equals_the_loop_of_single_calls_bit_for_bit(tmp_path, case):
    tree, shapes, out_shape, carried = CASES[case]
    count = 5
    kernel = _generate(tmp_path, case, 0)
    order_c, order_1 = leaf_order(tree, skip=(carried,)), leaf_order(tree)
    nc = len(order_c)
    carried_lib, src_c = _build(tmp_path, kernel + "_c", [f"a[{i}]" for i in range(nc + 1)] + [f"s[{i}]" for i in range(nc)] + ["count"])
    assert _params(src_c, kernel + "_c") == [f"in{i}_" for i in range(nc)] + ["out_"] + [f"s_in{i}" for i in range(nc)] + ["count"]
    single_lib, _ = _build(tmp_path, kernel, [f"a[{i}]" for i in range(len(order_1) + 1)])

    b = AccBatch(CASES[case], count, seed=23)
    m, n, ld, _ = out_shape
    got = Guarded(b.acc0)
    strides = (C.c_longlong * nc)(*[b.strides[k] for k in order_c])
    assert carried_lib.emulate(_ptrs([b.inputs[k] for k in order_c] + [got.inside]), strides, count, 0, 1) == 0
    want = b.acc0.copy()
    for i in range(count):       # the caller's loop: every call reads the output the previous call wrote
        arrays = [want if k == carried else b.element(k, i) for k in order_1]
        assert single_lib.emulate(_ptrs(arrays + [want]), None, 1, 0, 1) == 0
    assert not np.array_equal(want, b.acc0)
    assert np.array_equal(got.inside.view(np.uint8), want.view(np.uint8))
    assert got.intact()                                                                   # nothing outside the output
    pad = got.inside.reshape(n, ld)[:, m:]
    assert np.array_equal(pad, b.acc0.reshape(n, ld)[:, m:])                              # ... nor between its padded columns


@needs_hiprtc
@pytest.mark.parametrize("case", SLICEABLE)
def test_sliced_kernels_equal_the_documented_order_of_additions_bit_for_bit(tmp_path, case):
    tree, shapes, out_shape, carried = CASES[case]
    count = 7
    kernel = _generate(tmp_path, case, 1)
    order_s = leaf_order(tree, skip=(carried,))
    ns = len(order_s)
    m, n, ld, _ = out_shape
    sliced_lib, src_s = _build(tmp_path, kernel + "_s", [f"a[{i}]" for i in range(ns + 1)] + [f"s[{i}]" for i in range(ns)] + ["count", "slices"])
    assert _params(src_s, kernel + "_s") == [f"in{i}_" for i in range(ns)] + ["part_"] + [f"s_in{i}" for i in range(ns)] + ["count", "slices"]
    combine_lib, _ = _build(tmp_path, f"meqn_jit_combine_{m}x{n}_ld{ld}", ["a[0]", "a[1]", "slices"])
    b = AccBatch(CASES[case], count, seed=29)
    strides = (C.c_longlong * ns)(*[b.strides[k] for k in order_s])
    results = []
    for slices in (1, 2, 3):
        part = np.full(slices * n * m + 32, np.float32(-55.0))
        got = Guarded(b.acc0)
        # two blocks along y for three slices: the kernel's loop over slices runs
        assert sliced_lib.emulate(_ptrs([b.inputs[k] for k in order_s] + [part]), strides, count, slices, min(slices, 2)) == 0
        assert np.all(part[slices * n * m:] == np.float32(-55.0))
        assert combine_lib.emulate(_ptrs([part, got.inside]), None, count, slices, 1) == 0
        want = sliced_restatement(b, case, slices)
        assert np.array_equal(got.inside.view(np.uint32), want.ravel().view(np.uint32)), slices
        assert got.intact()
        results.append(got.inside.copy())
    if case.startswith("dgamma"):      # the slicings really are different orders of the same sum
        assert not (np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2]))


VALIDATION_CHILD = r"""
import sys
import ctypes as C
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from libxsmm_amd import capi
from libxsmm_amd.capi import BINARY, DT, UNARY, UNARY_FLAG
import test_meqn as tm
from meqn_acc_helpers import CASES
api = capi.load()
ll = C.c_longlong
def err():
    e = api.hip_get_last_error(); api.hip_clear_last_error(); return e
def param(n, carried):
    inputs = (capi.MatrixArg * n)()
    for i in range(n):
        inputs[i].primary = 4096 * (i + 1)
    p = capi.MeqnParam(); p.inputs = inputs; p.output.primary = inputs[carried].primary if carried is not None else 65536
    ops = (capi.MatrixOpArg * 4)()
    ops[1].primary = 131072
    p.ops_args = ops
    p._keep = (inputs, ops)
    return p
acc = api.hip_meqn_batch_strided_accumulate
tree, shapes, out, carried = CASES["dgamma_f32"]
h = api.dispatch_meqn(tm.build(api, tree, shapes), capi.MeqnArgShape(*out))
assert h
s5 = (ll * 5)(16384, 4, 4, 16384, 0)
p = param(5, 4)
acc(h, C.byref(p), 0, 5, s5, 0, None, 0); print("count0", err())
acc(h, C.byref(p), 3, 4, s5, 0, None, 0); print("ninputs", err())
acc(h, C.byref(p), 3, 5, None, 0, None, 0); print("nostrides", err())
acc(h, C.byref(p), 3, 5, s5, 0, None, 0); print("valid_loop", err())
acc(h, C.byref(p), 3, 5, s5, 0, None, 1); print("valid_any", err())
acc(h, C.byref(p), 3, 5, s5, 0, None, 2); print("order", err())
acc(None, C.byref(p), 3, 5, s5, 0, None, 0); print("null", err())
g = api.dispatch_gemm(capi.gemm_shape(32, 32, 32, 32, 32, 32, DT.F32, DT.F32, DT.F32, DT.F32), 0, 0)
assert g
acc(g, C.byref(p), 3, 5, s5, 0, None, 0); print("gemm_handle", err())
q = param(5, None)
acc(h, C.byref(q), 3, 5, s5, 0, None, 0); print("no_carried", err())
s5b = (ll * 5)(16384, 4, 4, 16384, 16)
acc(h, C.byref(p), 3, 5, s5b, 0, None, 0); print("carried_stepped", err())
# the carried operand declared with another leading dimension / type than the output
for label, shape in (("carried_ld", (40, 24, 40, DT.F32)), ("carried_type", (40, 24, 48, DT.BF16))):
    tr = ("b", BINARY.ADD, 0, tm.A(0), tm.A(1))
    hh = api.dispatch_meqn(tm.build(api, tr, [(40, 24, 48, DT.F32), shape]), capi.MeqnArgShape(40, 24, 48, DT.F32))
    assert hh
    acc(hh, C.byref(param(2, 1)), 3, 2, (ll * 2)(8192, 0), 0, None, 0); print(label, err())
# a head with a side channel: ReLU that also writes its bitmask to output.secondary
tr = ("u", UNARY.RELU, UNARY_FLAG.BITMASK_2BYTEMULT, ("b", BINARY.ADD, 0, tm.A(0), tm.A(1)))
hh = api.dispatch_meqn(tm.build(api, tr, [(64, 24, 64, DT.F32)] * 2), capi.MeqnArgShape(64, 24, 64, DT.F32))
assert hh
acc(hh, C.byref(param(2, 1)), 3, 2, (ll * 2)(8192, 0), 0, None, 0); print("side_channel", err())
# a DUMP destination that every element would overwrite
idx = api.meqn_create()
md = lambda pos=-1: capi.MeqnMetadata(idx, pos)
assert api.meqn_push_back_binary_op(md(), BINARY.ADD, DT.F32, 0) == 0
assert api.meqn_push_back_unary_op(md(1), UNARY.DUMP, DT.F32, 0) == 0
assert api.meqn_push_back_unary_op(md(), UNARY.X2, DT.F32, 0) == 0
assert api.meqn_push_back_arg(md(0), capi.MeqnArgShape(40, 24, 48, DT.F32), tm.SINGULAR) == 0
assert api.meqn_push_back_arg(md(1), capi.MeqnArgShape(40, 24, 48, DT.F32), tm.SINGULAR) == 0
hd = api.dispatch_meqn(idx, capi.MeqnArgShape(40, 24, 48, DT.F32))
assert hd
pd = param(2, 1)
acc(hd, C.byref(pd), 3, 2, (ll * 2)(8192, 0), 2, (ll * 2)(0, 0), 0); print("dump_shared", err())
acc(hd, C.byref(pd), 1, 2, (ll * 2)(8192, 0), 2, (ll * 2)(0, 0), 0); print("dump_shared_count1", err())
acc(hd, C.byref(pd), 3, 2, (ll * 2)(8192, 0), 2, (ll * 2)(0, 4096), 0); print("dump_stepped", err())
# a BRGEMM node: its block count (ops_args[3].tertiary) is shared by all elements
m, n, k, blocks = 32, 16, 24, 5
idx = api.meqn_create()
assert api.meqn_push_back_binary_op(md(), BINARY.ADD, DT.F32, 0) == 0
assert api.meqn_push_back_arg(md(0), capi.MeqnArgShape(m, n, m, DT.F32), tm.SINGULAR) == 0
assert api.meqn_push_back_binary_op(md(3), BINARY.BRGEMM, DT.F32, 0) == 0
assert api.meqn_push_back_arg(md(2), capi.MeqnArgShape(m, k, m, DT.F32), capi.MatrixArgAttributes(1, 3, blocks, m * k * 4)) == 0
assert api.meqn_push_back_arg(md(3), capi.MeqnArgShape(k, n, k, DT.F32), capi.MatrixArgAttributes(1, 3, blocks, k * n * 4)) == 0
hb = api.dispatch_meqn(idx, capi.MeqnArgShape(m, n, m, DT.F32))
assert hb
pb = param(4, 0)
s4 = (ll * 4)(0, 0, 32768, 32768)
ops = (ll * 4)(0, 0, 0, 0)
acc(hb, C.byref(pb), 3, 4, s4, 4, ops, 0); print("brgemm_shared", err())
ops[3] = 8
acc(hb, C.byref(pb), 3, 4, s4, 4, ops, 0); print("brgemm_stepped", err())
"""


def test_accumulating_entry_refusals_set_the_documented_error_codes(tmp_path):
    r = subprocess.run([sys.executable, "-c", VALIDATION_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                       capture_output=True, text=True, timeout=600, env=_dry_env(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(ln.split() for ln in r.stdout.splitlines() if len(ln.split()) == 2)
    assert got == {"count0": "0",                                  # nothing to do
                   "ninputs": "-2", "nostrides": "-2",             # fewer input strides than the equation's input positions
                   "valid_loop": "-4", "valid_any": "-4",          # accepted and generated; then: no device
                   "order": "-3",                                  # neither ORDER_LOOP nor ORDER_ANY
                   "null": "-3", "gemm_handle": "-3",              # not an equation handle
                   "no_carried": "-3", "carried_stepped": "-3",    # no input position is the output with stride 0
                   "carried_ld": "-3", "carried_type": "-3",       # the carried operand is not declared as the output is
                   "side_channel": "-3",                           # the head writes output.secondary
                   "dump_shared": "-3", "dump_shared_count1": "-4", "dump_stepped": "-4",      # a DUMP destination with stride 0 while count > 1
                   "brgemm_shared": "-4", "brgemm_stepped": "-3"}, r.stdout + r.stderr        # a stride on the shared BRGEMM block count
