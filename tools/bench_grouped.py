"""Grouped GEMM batches (libxsmm_hip_gemm_batch_grouped) against the launches they replace, on two fixed mixed workloads.

Modes per workload: `grouped` (one call), `serial` (the per-group libxsmm_hip_gemm_batch_strided launches back to back on one stream) and `pipeline8`
(the same launches inside an 8-lane pipeline section).  Every step is timed with device events on torch's stream; the median over --steps warm steps is
reported with the fraction of 8 TB/s on algorithmic bytes (A, B read once per problem, C written; beta = 0).  One JSON line per workload and mode.

  python tools/bench_grouped.py --steps 200 --warmup 20 --out profiles/r10_grouped.jsonl
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from libxsmm_amd import capi  # noqa: E402
from libxsmm_amd.capi import DT, GEMM_FLAG  # noqa: E402

PEAK = 8e12
WORKLOADS = {
    "f32_mix": dict(a=DT.F32, c=DT.F32, flags=0,
                    shapes=[(13, 13, 13, 4096), (16, 16, 16, 4096), (23, 23, 23, 4096), (32, 32, 32, 4096), (40, 40, 40, 2048), (64, 64, 64, 1024), (24, 48, 32, 2048)]),
    "bf16_vnni_mix_c_bf16": dict(a=DT.BF16, c=DT.BF16, flags=GEMM_FLAG.VNNI_A,
                                 shapes=[(16, 16, 16, 4096), (32, 32, 32, 4096), (48, 48, 48, 2048), (64, 64, 64, 1024), (72, 72, 72, 512)]),
    "bf16_vnni_mix_c_f32": dict(a=DT.BF16, c=DT.F32, flags=GEMM_FLAG.VNNI_A,
                                shapes=[(16, 16, 16, 4096), (32, 32, 32, 4096), (48, 48, 48, 2048), (64, 64, 64, 1024), (72, 72, 72, 512)]),
}


def build(api, wl):
    groups, keep, nbytes = [], [], 0
    asz, csz = capi.DT_SIZE[wl["a"]], capi.DT_SIZE[wl["c"]]
    for (m, n, k, count) in wl["shapes"]:
        h = api.dispatch_gemm(capi.gemm_shape(m, n, k, m, k, m, wl["a"], wl["a"], wl["c"], DT.F32), wl["flags"] | GEMM_FLAG.BETA_0, 0)
        assert h, (m, n, k)
        A = torch.randint(-4, 5, (count * m * k,), device="cuda", dtype=torch.int32).to(torch.float32 if wl["a"] == DT.F32 else torch.bfloat16)
        B = torch.randint(-4, 5, (count * k * n,), device="cuda", dtype=torch.int32).to(A.dtype)
        Cb = torch.zeros(count * m * n, device="cuda", dtype=torch.float32 if wl["c"] == DT.F32 else torch.bfloat16)
        keep += [A, B, Cb]
        g = capi.GemmGroup()
        g.kernel, g.count = h, count
        g.param.a.primary, g.param.b.primary, g.param.c.primary = A.data_ptr(), B.data_ptr(), Cb.data_ptr()
        g.stride_a, g.stride_b, g.stride_c = m * k * asz, k * n * asz, m * n * csz
        groups.append(g)
        nbytes += count * ((m * k + k * n) * asz + m * n * csz)
    return (capi.GemmGroup * len(groups))(*groups), keep, nbytes


def step_fn(api, arr, mode):
    n = len(arr)
    if mode == "grouped":
        return lambda: api.hip_gemm_batch_grouped(arr, n)

    def serial():
        for g in arr:
            api.hip_gemm_batch_strided(g.kernel, C.byref(g.param), g.count, g.stride_a, g.stride_b, g.stride_c)

    if mode == "serial":
        return serial

    def pipelined():
        assert api.hip_pipeline_begin(8) == 0
        serial()
        assert api.hip_pipeline_end() == 0
    return pipelined


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_grouped.jsonl"))
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    args = ap.parse_args()
    api = capi.load()
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    api.hip_set_async(1)
    lines = []
    for name in args.workloads.split(","):
        wl = WORKLOADS[name]
        arr, keep, nbytes = build(api, wl)
        for mode in ("grouped", "serial", "pipeline8"):
            fn = step_fn(api, arr, mode)
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            api.hip_launch_count(1)
            for s, e in ev:
                s.record(); fn(); e.record()
            torch.cuda.synchronize()
            api.check()
            launches = api.hip_launch_count(1) / args.steps
            us = statistics.median(s.elapsed_time(e) * 1e3 for s, e in ev)
            rec = dict(workload=name, mode=mode, groups=len(arr), problems=int(sum(g.count for g in arr)), launches_per_step=launches,
                       us_per_step=round(us, 3), algorithmic_bytes=nbytes, fraction_of_8TBs=round(nbytes / (us * 1e-6) / PEAK, 4), steps=args.steps)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del keep
    api.hip_sync()
    api.hip_set_async(0)
    api.hip_set_stream(None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
