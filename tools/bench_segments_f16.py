"""IEEE-half segments (F16 handles in libxsmm_hip_gemm_batch_reduce_segments) against what a caller had before and against the bf16 segments call, on the
method and the workload of tools/bench_segments_fp8.py (its OperandSet, counts and densities are used as they are).

Workload: the count pattern of a block-sparse layer Y = W X of 64 x 64 blocks -- 4096 segments of 64^3 products at three densities, 5 % of the block rows four
times as long.  Kinds: F16 -> f32 and F16 -> f16.  Modes per workload:
  segments        one call through the f16 handle
  per_count       what the library offered for these handles before: one libxsmm_hip_gemm_batch_strided launch per distinct count over re-sorted lists (the
                  re-sort is outside the timed region, and the segments call runs on the same re-sorted memory: generous to this baseline)
  bf16_segments   the bf16 (VNNI-2 A) segments call on the same pattern with C of the same width (f32, or bf16 for an f16 C): the same bytes, the same
                  instruction rate
Operand sets rotate past the Infinity Cache; a step is timed with device events; the median over --steps warm steps is reported with the fraction of 8 TB/s on
the algorithmic bytes.  Every mode is measured --repeats times, interleaved; the spread of the baseline's medians is recorded in every line: a ratio inside it
is "equal".  The data are exact (0, +-1, +-2), so the two f16 modes must agree bit for bit: checked before anything is timed.
--fused measures the fused ext OFFSET entry (bias + ReLU) against the plain offsets call plus two TPP passes, on the workloads, modes and checks of
tools/bench_segments_offsets_fused.py (DESIGN.md section 9.3's comparison), with the bf16 rows next to the f16 ones.

  python tools/bench_segments_f16.py --steps 200 --warmup 20 --out profiles/r23_segments_f16.jsonl
  python tools/bench_segments_f16.py --fused profiles/r23_segments_f16_fused.jsonl
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_segments_fp8 as base  # noqa: E402
from bench_segments_fp8 import DENSITIES, E, LLC, NSEG, PEAK, OperandSet, draw_counts  # noqa: E402
from libxsmm_amd import capi  # noqa: E402
from libxsmm_amd.capi import DT, GEMM_FLAG  # noqa: E402

base.TORCH_OF[DT.F16] = torch.float16
KINDS = {"f16_f32": dict(c=DT.F32, bf16_c=DT.F32), "f16_f16": dict(c=DT.F16, bf16_c=DT.BF16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_segments_f16.jsonl"))
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--densities", default=",".join(DENSITIES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_segments_f16.py needs a GPU: nothing is measured without one")
    api = capi.load()
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    api.hip_set_async(1)
    adr = capi.br_config(capi.BR_ADDRESS, 0, 0, 0)
    lines = []
    for kname in args.kinds.split(","):
        kind = KINDS[kname]
        h = api.dispatch_brgemm(capi.gemm_shape(E, E, E, E, E, E, DT.F16, DT.F16, kind["c"], DT.F32), GEMM_FLAG.VNNI_A | GEMM_FLAG.BETA_0, 0, adr)
        hb = api.dispatch_brgemm(capi.gemm_shape(E, E, E, E, E, E, DT.BF16, DT.BF16, kind["bf16_c"], DT.F32), GEMM_FLAG.VNNI_A | GEMM_FLAG.BETA_0, 0, adr)
        assert h and hb, kname
        for dname in args.densities.split(","):
            counts = draw_counts(DENSITIES[dname], np.random.default_rng(21))
            first = OperandSet(DT.F16, kind["c"], counts)
            nsets = max(2, -(-2 * LLC // first.bytes) + 1)
            sets = [first] + [OperandSet(DT.F16, kind["c"], counts) for _ in range(nsets - 1)]
            bsets = [OperandSet(DT.BF16, kind["bf16_c"], counts) for _ in range(nsets)]
            empty = capi.GemmParam()

            def segments(i):
                s = sets[i % nsets]
                api.hip_gemm_batch_reduce_segments(h, C.byref(empty), NSEG, s.seg_ptr.data_ptr(), s.la.data_ptr(), s.lb.data_ptr(), s.lc.data_ptr())

            def bf16_segments(i):
                s = bsets[i % nsets]
                api.hip_gemm_batch_reduce_segments(hb, C.byref(empty), NSEG, s.seg_ptr.data_ptr(), s.la.data_ptr(), s.lb.data_ptr(), s.lc.data_ptr())

            def per_count(i):
                s = sets[i % nsets]
                for d, n, p0, c0 in s.launches:
                    p = capi.GemmParam(); cnt = C.c_ulonglong(d)
                    p.a.primary, p.b.primary = s.sla.data_ptr() + p0 * 8, s.slb.data_ptr() + p0 * 8
                    p.c.primary = s.C.data_ptr() + c0 * s.blk * s.csz; p.op.tertiary = C.addressof(cnt)
                    api.hip_gemm_batch_strided(h, C.byref(p), n, d * 8, d * 8, s.blk * s.csz)

            def measure(fn):
                for i in range(args.warmup):
                    fn(i)
                torch.cuda.synchronize(); api.check()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
                api.hip_launch_count(1)
                for i, (s, t) in enumerate(ev):
                    s.record(); fn(i); t.record()
                torch.cuda.synchronize(); api.check()
                return statistics.median(s.elapsed_time(t) * 1e3 for s, t in ev), api.hip_launch_count(1) / args.steps

            # the two f16 modes give the same C (exact data): checked once per workload before anything is timed
            segments(0); torch.cuda.synchronize(); api.check(); got = first.C.clone(); first.C.zero_()
            seg_kernel = api.hip_kernel_name(h, 1).decode()
            per_count(0); torch.cuda.synchronize(); api.check()
            base_kernel = api.hip_kernel_name(h, 1).decode()
            assert torch.equal(got.view(torch.uint8), first.C.view(torch.uint8)), f"{kname} {dname}: segments call and per-count launches disagree"
            assert got.view(torch.uint8).any()
            us = {"segments": [], "per_count": [], "bf16_segments": []}
            launches = {}
            for _ in range(args.repeats):                        # interleaved repeats: the baseline's own spread
                for mode, fn in (("segments", segments), ("per_count", per_count), ("bf16_segments", bf16_segments)):
                    t, launches[mode] = measure(fn); us[mode].append(t)
            spread = (max(us["per_count"]) - min(us["per_count"])) / min(us["per_count"])
            bspread = (max(us["bf16_segments"]) - min(us["bf16_segments"])) / min(us["bf16_segments"])
            med = {m: statistics.median(v) for m, v in us.items()}
            common = dict(workload=f"{kname}_{dname}", segments=NSEG, products=int(counts.sum()), distinct_counts=len(first.launches), operand_sets=nsets,
                          baseline_spread=round(spread, 4), bf16_spread=round(bspread, 4))
            for mode, nbytes, kernel in (("segments", first.bytes, seg_kernel), ("per_count", first.bytes, base_kernel),
                                         ("bf16_segments", bsets[0].bytes, api.hip_kernel_name(hb, 1).decode())):
                rec = dict(common, mode=mode, kernel=kernel, algorithmic_bytes=nbytes, launches_per_step=launches[mode], us_per_step=round(med[mode], 3),
                           us_medians=[round(x, 3) for x in us[mode]], fraction_of_8TBs=round(nbytes / (med[mode] * 1e-6) / PEAK, 4),
                           time_over_segments=round(med[mode] / med["segments"], 3), steps=args.steps)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            del sets, bsets, first
            torch.cuda.empty_cache()
    api.hip_sync()
    api.hip_set_async(0)
    api.hip_set_stream(None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def fused(out, steps, warmup):
    """The fused ext OFFSET entry (bias + ReLU, F16 -> f16, 64^3, NN and NT) against the plain offsets call plus two TPP passes, and the bf16 rows next to it:
    tools/bench_segments_offsets_fused.py as it is (its 8192-segment workloads, its modes, its checks), with one more kind."""
    import bench_segments_offsets as offs
    import bench_segments_offsets_fused as offs_fused
    offs.KINDS["f16_64_c_f16"] = dict(t=DT.F16, c=DT.F16, e=64, vnni=GEMM_FLAG.VNNI_A, torch=torch.float16)
    argv = sys.argv
    sys.argv = [argv[0], "--kinds", "f16_64_c_f16,bf16_64_c_bf16", "--forms", "NN,NT", "--steps", str(steps), "--warmup", str(warmup), "--out", out]
    try:
        offs_fused.main()
    finally:
        sys.argv = argv


if __name__ == "__main__":
    if "--fused" in sys.argv:       # python tools/bench_segments_f16.py --fused [out.jsonl]: only the fused comparison
        rest = [a for a in sys.argv[1:] if a != "--fused"]
        fused(rest[0] if rest else os.path.join(ROOT, "profiles", "r23_segments_f16_fused.jsonl"), 200, 20)
    else:
        main()
