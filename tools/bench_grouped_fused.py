"""Fused grouped batches (libxsmm_hip_gemm_ext_batch_grouped) and group plans against what they replace.

  (a) the workloads of tools/bench_grouped.py with bias + ReLU: `ext_grouped` (one call) against `ext_serial` (the loop of libxsmm_hip_gemm_ext_batch_strided
      launches), and per f32 shape and problem count `grouped` (the shape cut into groups below the own-kernel threshold, so that all of it runs in the fused
      grouped kernel) against `own` (its one ext strided launch): the table that sets the fused f32 threshold
  (b) 10 000 one-problem f32 groups: `call` (libxsmm_hip_gemm_batch_grouped) against `plan` (a resident plan launched directly) and `graph` (the plan's launch
      captured and replayed), device time and host time per call
  (c) the plain bf16 workload as `plan` against `call`

The variants of one comparison alternate step by step inside one process; every step is timed with device events on torch's stream and, on the host, with
perf_counter around the call (stream-ordered mode: the time to issue it).  Reported: the median over --steps warm steps, the quartiles, and over --repeats
repetitions of the whole comparison the lowest and highest median (the run-to-run spread).  One JSON line per comparison and variant.

  python tools/bench_grouped_fused.py --steps 200 --warmup 20 --out profiles/r17_grouped_fused.jsonl
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_grouped import WORKLOADS  # noqa: E402
from libxsmm_amd import capi  # noqa: E402
from libxsmm_amd.capi import DT, GEMM_FLAG, UNARY  # noqa: E402

OWN_ITEMS = 2048                                     # the launch rule's threshold (runtime.cpp: kGroupedOwnF32Items / kGroupedOwnF32FusedItems)


def tensors(a, c, m, n, k, count, bias):
    ta, tc = (torch.float32 if a == DT.F32 else torch.bfloat16), (torch.float32 if c == DT.F32 else torch.bfloat16)
    A = torch.randint(-4, 5, (count * m * k,), device="cuda", dtype=torch.int32).to(ta)
    B = torch.randint(-4, 5, (count * k * n,), device="cuda", dtype=torch.int32).to(ta)
    Cb = torch.zeros(count * m * n, device="cuda", dtype=tc)
    D = torch.randint(-4, 5, (count * m,), device="cuda", dtype=torch.int32).to(tc) if bias else None
    return A, B, Cb, D


def ext_groups(api, a, c, flags, shapes, max_items=None):
    """One ext group (bias + ReLU) per shape -- or, with max_items, per slice of a shape of at most that many work items."""
    groups, keep = [], []
    asz, csz = capi.DT_SIZE[a], capi.DT_SIZE[c]
    for (m, n, k, count) in shapes:
        h = api.dispatch_brgemm_ext(capi.gemm_shape(m, n, k, m, k, m, a, a, c, DT.F32), flags | GEMM_FLAG.BETA_0, 0, capi.br_config(),
                                    capi.argops_cp(m, UNARY.RELU), capi.postops_colbias(m, c))
        assert h, (m, n, k)
        A, B, Cb, D = tensors(a, c, m, n, k, count, True)
        keep += [A, B, Cb, D]
        tile = 16 if (m <= 16 and n <= 16) else 32
        tiles = ((m + tile - 1) // tile) * ((n + tile - 1) // tile)
        per = count if max_items is None else max(1, min((count + 1) // 2, max_items // tiles))      # (at least two slices: a single group leaves for its own kernel)
        for e0 in range(0, count, per):
            g = capi.GemmExtGroup()
            g.kernel, g.count = h, min(per, count - e0)
            g.stride_a, g.stride_b, g.stride_c, g.stride_d = m * k * asz, k * n * asz, m * n * csz, m * csz
            g.param.a.primary, g.param.b.primary = A.data_ptr() + e0 * g.stride_a, B.data_ptr() + e0 * g.stride_b
            g.param.c.primary, g.param.d.primary = Cb.data_ptr() + e0 * g.stride_c, D.data_ptr() + e0 * g.stride_d
            groups.append(g)
    return (capi.GemmExtGroup * len(groups))(*groups), keep


def plain_groups(api, a, c, flags, shapes, one_problem=False):
    groups, keep = [], []
    asz, csz = capi.DT_SIZE[a], capi.DT_SIZE[c]
    for (m, n, k, count) in shapes:
        h = api.dispatch_gemm(capi.gemm_shape(m, n, k, m, k, m, a, a, c, DT.F32), flags | GEMM_FLAG.BETA_0, 0)
        assert h, (m, n, k)
        A, B, Cb, _ = tensors(a, c, m, n, k, count, False)
        keep += [A, B, Cb]
        per = 1 if one_problem else count
        for e0 in range(0, count, per):
            g = capi.GemmGroup()
            g.kernel, g.count = h, per
            g.stride_a, g.stride_b, g.stride_c = m * k * asz, k * n * asz, m * n * csz
            g.param.a.primary, g.param.b.primary, g.param.c.primary = A.data_ptr() + e0 * g.stride_a, B.data_ptr() + e0 * g.stride_b, Cb.data_ptr() + e0 * g.stride_c
            groups.append(g)
    if one_problem:                                  # shapes interleaved
        order = torch.randperm(len(groups), generator=torch.Generator().manual_seed(1)).tolist()
        groups = [groups[i] for i in order]
    return (capi.GemmGroup * len(groups))(*groups), keep


def ext_serial(api, arr):
    def fn():
        for g in arr:
            api.hip_gemm_ext_batch_strided(g.kernel, C.byref(g.param), g.count, g.stride_a, g.stride_b, g.stride_c, g.stride_d, g.stride_mask)
    return fn


def captured(api, fn):
    """fn's launches captured on a side stream; returns the replay."""
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        api.hip_set_stream(side.cuda_stream)
        graph.capture_begin(); fn(); graph.capture_end()
    api.check()
    torch.cuda.current_stream().wait_stream(side)
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    return graph


def compare(api, name, variants, args, extra=None):
    """variants: {label: fn}.  Alternates them step by step; returns one record per variant."""
    medians = {v: [] for v in variants}
    last = {}
    for _ in range(args.repeats):
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        ev = {v: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)] for v in variants}
        host = {v: [] for v in variants}
        launches = {v: 0 for v in variants}
        for i in range(args.steps):
            for v, fn in variants.items():
                s, e = ev[v][i]
                api.hip_launch_count(1)
                s.record(); t0 = time.perf_counter(); fn(); t1 = time.perf_counter(); e.record()
                host[v].append((t1 - t0) * 1e6)
                launches[v] = api.hip_launch_count(1)
            if i % 16 == 15:
                torch.cuda.synchronize()                 # keeps the host at most 16 steps ahead: host time is the time to issue, not to queue behind a full ring
        torch.cuda.synchronize()
        api.check()
        for v in variants:
            dev = sorted(s.elapsed_time(e) * 1e3 for s, e in ev[v])
            q = statistics.quantiles(dev, n=4)
            medians[v].append(q[1])
            last[v] = dict(us_p25=round(q[0], 3), us_p75=round(q[2], 3), host_us_per_call=round(statistics.median(host[v]), 3), launches_per_step=launches[v])
    recs = []
    for v in variants:
        rec = dict(comparison=name, variant=v, us_per_step=round(statistics.median(medians[v]), 3), us_median_lowest=round(min(medians[v]), 3),
                   us_median_highest=round(max(medians[v]), 3), steps=args.steps, repeats=args.repeats, **last[v])
        if extra:
            rec.update(extra)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_grouped_fused.jsonl"))
    args = ap.parse_args()
    api = capi.load()
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    api.hip_set_async(1)
    lines = []
    parts = args.parts.split(",")
    if "a" in parts:
        for name, wl in WORKLOADS.items():
            arr, keep = ext_groups(api, wl["a"], wl["c"], wl["flags"], wl["shapes"])
            lines += compare(api, f"a:{name}+bias+relu", {"ext_grouped": lambda: api.hip_gemm_ext_batch_grouped(arr, len(arr)), "ext_serial": ext_serial(api, arr)}, args,
                             dict(groups=len(arr)))
            del keep
        for (m, n, k) in [(13, 13, 13), (16, 16, 16), (23, 23, 23), (32, 32, 32), (40, 40, 40), (48, 48, 48), (64, 64, 64), (24, 48, 32)]:
            for count in (512, 2048, 4096):
                sliced, keep1 = ext_groups(api, DT.F32, DT.F32, 0, [(m, n, k, count)], max_items=OWN_ITEMS // 2)
                whole, keep2 = ext_groups(api, DT.F32, DT.F32, 0, [(m, n, k, count)])
                lines += compare(api, f"a:f32_shape_{m}x{n}x{k}x{count}", {"grouped": lambda: api.hip_gemm_ext_batch_grouped(sliced, len(sliced)), "own": ext_serial(api, whole)},
                                 args, dict(groups=len(sliced)))
                del keep1, keep2
    if "b" in parts:
        arr, keep = plain_groups(api, DT.F32, DT.F32, 0, [(8, 8, 8, 2500), (13, 13, 13, 2500), (20, 12, 9, 2500), (32, 32, 32, 2500)], one_problem=True)
        plan = api.hip_gemm_group_plan_create(arr, len(arr)); api.check()
        assert plan
        graph = captured(api, lambda: api.hip_gemm_group_plan_launch(plan))
        lines += compare(api, "b:10000_one_problem_f32_groups", {"call": lambda: api.hip_gemm_batch_grouped(arr, len(arr)), "plan": lambda: api.hip_gemm_group_plan_launch(plan),
                                                                  "graph": graph.replay}, args, dict(groups=len(arr)))
        torch.cuda.synchronize()
        del graph
        api.hip_gemm_group_plan_destroy(plan)
        del keep
    if "c" in parts:
        wl = WORKLOADS["bf16_vnni_mix_c_bf16"]
        arr, keep = plain_groups(api, wl["a"], wl["c"], wl["flags"], wl["shapes"])
        plan = api.hip_gemm_group_plan_create(arr, len(arr)); api.check()
        assert plan
        lines += compare(api, "c:bf16_vnni_mix_c_bf16", {"call": lambda: api.hip_gemm_batch_grouped(arr, len(arr)), "plan": lambda: api.hip_gemm_group_plan_launch(plan)}, args,
                         dict(groups=len(arr)))
        torch.cuda.synchronize()
        api.hip_gemm_group_plan_destroy(plan)
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
