"""Segments (libxsmm_hip_gemm_batch_reduce_segments) against what the library offered for the same work before, on fixed workloads of 8192 segments.

Workloads: f32 32^3, f64 23^3 and bf16 (VNNI A) 64^3 -> bf16, each with four count patterns: `uniform4` (every segment 4 products), `uniform0_8` (counts drawn
uniformly from 0..8), `skewed` (1 % of the segments 64 products, the rest 2, in list order) and `skewed_sorted` (the same segments, longest first).
Modes per workload:
  segments    one call
  per_count   one libxsmm_hip_gemm_batch_strided launch per distinct count, over lists and C blocks that the script re-sorted so that equal counts are
              contiguous (the re-sort is outside the timed region, and the segments call runs on the same re-sorted memory: generous to this baseline)
  loop        the stream-ordered loop of single calls, one per segment (--loop-steps steps: it is host bound)
Every product has A and B blocks of its own; the byte count charges every listed A / B block once per use plus C once (beta = 0).  The operands are
allocated as several sets, together more than twice the 256 MiB Infinity Cache, and a step takes the next set, so no step finds its operands cached.
A step is timed with device events on torch's stream; the median over --steps warm steps is reported with the fraction of 8 TB/s on algorithmic bytes.
`per_count` is measured --repeats times per workload, interleaved with `segments`: the spread of its medians (max - min) / min is the run-to-run spread
that a difference has to exceed, and is recorded in every line.

  python tools/bench_segments.py --steps 200 --warmup 20 --out profiles/r11_segments.jsonl
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from libxsmm_amd import capi  # noqa: E402
from libxsmm_amd.capi import DT, GEMM_FLAG  # noqa: E402

PEAK = 8e12
LLC = 256 << 20
NSEG = 8192
KINDS = {
    "f32_32": dict(t=DT.F32, c=DT.F32, comp=DT.F32, e=32, flags=0, torch=torch.float32, ctorch=torch.float32),
    "f64_23": dict(t=DT.F64, c=DT.F64, comp=DT.F64, e=23, flags=0, torch=torch.float64, ctorch=torch.float64),
    "bf16_vnni_64_c_bf16": dict(t=DT.BF16, c=DT.BF16, comp=DT.F32, e=64, flags=GEMM_FLAG.VNNI_A, torch=torch.bfloat16, ctorch=torch.bfloat16),
}
PATTERNS = ("uniform4", "uniform0_8", "skewed", "skewed_sorted")


def draw_counts(pattern, rng):
    if pattern == "uniform4":
        return np.full(NSEG, 4, dtype=np.int64)
    if pattern == "uniform0_8":
        return rng.integers(0, 9, NSEG).astype(np.int64)
    counts = np.where(rng.random(NSEG) < 0.01, 64, 2).astype(np.int64)
    return np.sort(counts)[::-1].copy() if pattern == "skewed_sorted" else counts


class OperandSet:
    """One set of operands and lists on the device.  Product r owns A block r and B block r; C is laid out in count-sorted order (rank), so the segments of
    one count are a strided batch for the baseline, and the sorted lists are the segment lists gathered in that order."""

    def __init__(self, kind, counts):
        e, dt = kind["e"], kind["torch"]
        blk = e * e
        esz, csz = capi.DT_SIZE[kind["t"]], capi.DT_SIZE[kind["c"]]
        total = int(counts.sum())
        self.A = torch.randint(-4, 5, (max(total, 1) * blk,), device="cuda", dtype=torch.int32).to(dt)
        self.B = torch.randint(-4, 5, (max(total, 1) * blk,), device="cuda", dtype=torch.int32).to(dt)
        self.C = torch.zeros(NSEG * blk, device="cuda", dtype=kind["ctorch"])
        seg_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        order = np.argsort(-counts, kind="stable")                   # segments by descending count: equal counts contiguous
        rank = np.empty(NSEG, dtype=np.int64); rank[order] = np.arange(NSEG)
        prod = np.arange(total, dtype=np.int64)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to("cuda")
        self.seg_ptr = dev(seg_ptr)
        self.la, self.lb = dev(self.A.data_ptr() + prod * blk * esz), dev(self.B.data_ptr() + prod * blk * esz)
        self.lc = dev(self.C.data_ptr() + rank * blk * csz)
        # the re-sorted lists of the baseline: the products of the segments in `order`
        gather = np.concatenate([np.arange(seg_ptr[s], seg_ptr[s + 1]) for s in order]) if total else prod
        self.sla, self.slb = dev(self.A.data_ptr() + gather * blk * esz), dev(self.B.data_ptr() + gather * blk * esz)
        self.launches = []                                           # (count, elements, first product in the sorted lists, first C rank)
        sc = counts[order]
        first_prod = np.concatenate([[0], np.cumsum(sc)])
        for d in sorted(set(sc.tolist()), reverse=True):
            idx = np.flatnonzero(sc == d)
            self.launches.append((int(d), len(idx), int(first_prod[idx[0]]), int(idx[0])))
        self.blk, self.esz, self.csz = blk, esz, csz
        self.bytes = total * 2 * blk * esz + NSEG * blk * csz
        self.counts, self.seg_ptr_host, self.rank = counts, seg_ptr, rank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loop-steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_segments.jsonl"))
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--patterns", default=",".join(PATTERNS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_segments.py needs a GPU: nothing is measured without one")
    api = capi.load()
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    api.hip_set_async(1)
    lines = []
    for kname in args.kinds.split(","):
        kind = KINDS[kname]
        e = kind["e"]
        h = api.dispatch_brgemm(capi.gemm_shape(e, e, e, e, e, e, kind["t"], kind["t"], kind["c"], kind["comp"]), kind["flags"] | GEMM_FLAG.BETA_0, 0,
                                capi.br_config(capi.BR_ADDRESS, 0, 0, 0))
        assert h, kname
        for pattern in args.patterns.split(","):
            counts = draw_counts(pattern, np.random.default_rng(11))
            first = OperandSet(kind, counts)
            nsets = max(2, -(-2 * LLC // first.bytes) + 1)
            sets = [first] + [OperandSet(kind, counts) for _ in range(nsets - 1)]
            empty = capi.GemmParam()
            keep = []

            def segments(s):
                api.hip_gemm_batch_reduce_segments(h, C.byref(empty), NSEG, s.seg_ptr.data_ptr(), s.la.data_ptr(), s.lb.data_ptr(), s.lc.data_ptr())

            def per_count(s):
                for d, n, p0, c0 in s.launches:
                    p = capi.GemmParam(); cnt = C.c_ulonglong(d)
                    p.a.primary, p.b.primary = s.sla.data_ptr() + p0 * 8, s.slb.data_ptr() + p0 * 8
                    p.c.primary = s.C.data_ptr() + c0 * s.blk * s.csz; p.op.tertiary = C.addressof(cnt)
                    api.hip_gemm_batch_strided(h, C.byref(p), n, d * 8, d * 8, s.blk * s.csz)

            def loop(s):
                for i in range(NSEG):
                    p = capi.GemmParam(); cnt = C.c_ulonglong(int(s.counts[i]))
                    p.a.primary, p.b.primary = s.la.data_ptr() + int(s.seg_ptr_host[i]) * 8, s.lb.data_ptr() + int(s.seg_ptr_host[i]) * 8
                    p.c.primary = s.C.data_ptr() + int(s.rank[i]) * s.blk * s.csz; p.op.tertiary = C.addressof(cnt)
                    capi.Api.call(h, p)

            def measure(fn, steps, warmup):
                for i in range(warmup):
                    fn(sets[i % nsets])
                torch.cuda.synchronize(); api.check()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
                api.hip_launch_count(1)
                for i, (s, t) in enumerate(ev):
                    s.record(); fn(sets[i % nsets]); t.record()
                torch.cuda.synchronize(); api.check()
                return statistics.median(s.elapsed_time(t) * 1e3 for s, t in ev), api.hip_launch_count(1) / steps

            # the two modes give the same C (exact small-integer data): checked once per workload before anything is timed
            segments(first); torch.cuda.synchronize(); got = first.C.clone(); first.C.zero_()
            seg_kernel = api.hip_kernel_name(h, 1).decode()
            per_count(first); torch.cuda.synchronize(); api.check()
            assert torch.equal(got, first.C), f"{kname} {pattern}: segments call and per-count launches disagree"
            seg_us, base_us = [], []
            for _ in range(args.repeats):                        # interleaved repeats: the baseline's own spread
                us, seg_launches = measure(segments, args.steps, args.warmup); seg_us.append(us)
                us, base_launches = measure(per_count, args.steps, args.warmup); base_us.append(us)
            loop_us, loop_launches = measure(loop, args.loop_steps, 2)
            spread = (max(base_us) - min(base_us)) / min(base_us)
            common = dict(workload=f"{kname}_{pattern}", segments=NSEG, products=int(counts.sum()), distinct_counts=len(first.launches), operand_sets=nsets,
                          algorithmic_bytes=first.bytes, baseline_spread=round(spread, 4), kernel=seg_kernel)
            for mode, us_all, launches, steps in (("segments", seg_us, seg_launches, args.steps), ("per_count", base_us, base_launches, args.steps),
                                                  ("loop", [loop_us], loop_launches, args.loop_steps)):
                us = statistics.median(us_all)
                rec = dict(common, mode=mode, launches_per_step=launches, us_per_step=round(us, 3), us_medians=[round(x, 3) for x in us_all],
                           fraction_of_8TBs=round(first.bytes / (us * 1e-6) / PEAK, 4), steps=steps)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            del sets, first, keep
            torch.cuda.empty_cache()
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
