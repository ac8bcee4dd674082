#!/usr/bin/env python
"""The dgamma / dbeta sums of a layernorm backward pass (samples/equation/equation_layernorm.c) as ONE accumulating batch
(libxsmm_hip_meqn_batch_strided_accumulate) against the caller's loop of `count` stream-ordered single calls that all read and write the same output.
Per workload the forms are alternated in one run (device events, warm): the loop, the carried form (ORDER_LOOP), the sliced form (ORDER_ANY) at the
candidate slice counts (LIBXSMM_HIP_MEQN_ACC_SLICES) and at the count the library's rule picks.  After the timed region every form runs once more on a
fresh output and is compared with the loop's: the carried form bit for bit, the sliced form by norm.  Algorithmic bytes: the stepped inputs once, the
output once.

  python tools/bench_meqn_acc.py [--out profiles/r11_meqn_acc.jsonl] [--reps 7]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from libxsmm_amd import capi  # noqa: E402
from libxsmm_amd.capi import DT, MEQN_ORDER_ANY, MEQN_ORDER_LOOP  # noqa: E402
import test_meqn as tm  # noqa: E402
from meqn_acc_helpers import dbeta, dgamma  # noqa: E402

ll = C.c_longlong
ES = {DT.F32: 4, DT.BF16: 2}
TDT = {DT.F32: torch.float32, DT.BF16: torch.bfloat16}
CANDIDATES = (2, 4, 8, 16, 32, 64, 128, 256, 512)
ENV = "LIBXSMM_HIP_MEQN_ACC_SLICES"


class Workload:
    """inputs[k]: (tensor or None, byte stride); the carried position is the output."""

    def __init__(self, api, name, case, count, gen):
        tree, shapes, out_shape, carried = case
        self.name, self.count, self.carried, self.out_shape = name, count, carried, out_shape
        self.h = api.dispatch_meqn(tm.build(api, tree, shapes), capi.MeqnArgShape(*out_shape))
        assert self.h
        self.inputs, self.bytes = [], 0
        used = set()
        walk = lambda t: used.add(t[1]) if t[0] == "arg" else [walk(c) for c in t[3:]]     # noqa: E731
        walk(tree)
        for k, (m, n, ld, dt) in enumerate(shapes):
            if k == carried or k not in used:
                self.inputs.append((None, 0))
                continue
            foot = ld * n * ES[dt]
            x = (torch.rand(ld * n * count, device="cuda", generator=gen) - 0.45).to(TDT[dt])
            self.inputs.append((x, foot))
            self.bytes += foot * count
        m, n, ld, dt = out_shape
        self.acc0 = torch.rand(ld * n, device="cuda", generator=gen).to(TDT[dt])
        self.bytes += ld * n * ES[dt]
        self.pad = torch.zeros(64, device="cuda")                        # what the unused input positions point at

    def param(self, i, out):
        inputs = (capi.MatrixArg * len(self.inputs))()
        for k, (t, s) in enumerate(self.inputs):
            inputs[k].primary = out.data_ptr() if k == self.carried else (self.pad.data_ptr() if t is None else t.data_ptr() + i * s)
        p = capi.MeqnParam()
        p.inputs = inputs
        p.output.primary = out.data_ptr()
        p._keep = inputs
        return p


def run(api, w, reps):
    out = w.acc0.clone()
    singles = [w.param(i, out) for i in range(w.count)]
    bp = w.param(0, out)
    sin = (ll * len(w.inputs))(*[s for (_, s) in w.inputs])
    call = capi.Api.call

    def loop():
        for p in singles:
            call(w.h, p)

    def acc(order, slices=None):
        def fn():
            if slices is None:
                os.environ.pop(ENV, None)
            else:
                os.environ[ENV] = str(slices)
            api.hip_meqn_batch_strided_accumulate(w.h, C.byref(bp), w.count, len(w.inputs), sin, 0, None, order)
            os.environ.pop(ENV, None)
        return fn
    forms = [("loop", loop), ("carried", acc(MEQN_ORDER_LOOP))]
    forms += [(f"sliced S={s}", acc(MEQN_ORDER_ANY, s)) for s in CANDIDATES if s <= w.count]
    forms.append(("rule", acc(MEQN_ORDER_ANY)))
    for _, fn in forms:                                                  # warm-up (the kernels are generated at the first accumulating calls)
        fn()
    torch.cuda.synchronize(); api.check()
    times = {name: [] for name, _ in forms}
    for _ in range(reps):                                                # the forms alternate inside one run
        for name, fn in forms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3)
    torch.cuda.synchronize(); api.check()
    results, kernels = {}, {}
    for name, fn in forms:                                               # outputs compared after the timed region, each form on a fresh output
        out.copy_(w.acc0); fn(); torch.cuda.synchronize(); api.check()
        results[name] = out.clone()
        kernels[name] = api.hip_kernel_name(w.h, 0 if name == "loop" else 1).decode()
    ref = results["loop"].double()
    recs = []
    t_loop = float(np.median(times["loop"]))
    for name, _ in forms:
        t = float(np.median(times[name]))
        rec = {"workload": w.name, "count": w.count, "form": name, "kernel": kernels[name], "us": round(t, 2), "speedup_over_loop": round(t_loop / t, 1),
               "algorithmic_bytes": w.bytes, "frac_8TBs": round(w.bytes / (t * 1e-6) / 8e12, 4),
               "equal_to_loop": bool(torch.equal(results[name].view(torch.int8), results["loop"].view(torch.int8))),
               "normf_rel_to_loop": float(((results[name].double() - ref).norm() / ref.norm()).item())}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    api = capi.load()
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)       # stream-ordered single calls and batches on torch's stream
    api.hip_set_jit(2)
    gen = torch.Generator(device="cuda").manual_seed(11)
    m = n = 64
    recs = []
    for name, case, count in (("dgamma 64x64 f32", dgamma(DT.F32, m, n, m), 4096), ("dgamma 64x64 bf16 in", dgamma(DT.BF16, m, n, m), 4096),
                              ("dbeta 64x64 f32", dbeta(DT.F32, m, n, m), 4096), ("dbeta 64x64 bf16 in", dbeta(DT.BF16, m, n, m), 4096),
                              ("dgamma 64x64 f32", dgamma(DT.F32, m, n, m), 256), ("dbeta 64x64 f32", dbeta(DT.F32, m, n, m), 256),
                              ("dgamma 64x64 f32", dgamma(DT.F32, m, n, m), 128), ("dbeta 64x64 f32", dbeta(DT.F32, m, n, m), 128),
                              ("dgamma 64x64 f32", dgamma(DT.F32, m, n, m), 64), ("dbeta 64x64 f32", dbeta(DT.F32, m, n, m), 64),
                              ("dgamma 64x64 f32", dgamma(DT.F32, m, n, m), 16), ("dbeta 64x64 f32", dbeta(DT.F32, m, n, m), 16)):
        w = Workload(api, name, case, count, gen)
        recs += run(api, w, args.reps)
        del w
        torch.cuda.empty_cache()
    api.hip_set_jit(1)
    if args.out:
        with open(args.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
    api.hip_sync()
    api.hip_set_stream(None)
    api.hip_set_async(0)


if __name__ == "__main__":
    main()
