"""Fused segments (libxsmm_hip_gemm_ext_batch_reduce_segments, bias + ReLU) against what the library offered for the same result before, on the fixed workloads
of tools/bench_segments.py: 8192 segments with the count patterns `uniform4`, `uniform0_8`, `skewed` and `skewed_sorted`, f32 32^3 and bf16 (VNNI A) 64^3 -> bf16.

Modes per workload:
  fused        one call: the bias starts the accumulator, the ReLU sits in front of the store
  three_pass   the plain segments call, then libxsmm_hip_meltw_binary_batch_strided (column-broadcast add of the segment's bias) and
               libxsmm_hip_meltw_unary_batch_strided (ReLU) in place over the contiguous C blocks: three launches, C is traversed three times
  loop         the stream-ordered loop of single fused calls, one per segment (--loop-steps steps: it is host bound)
Every segment has a bias vector of its own (d_list has no repeated entry: nothing of the bias traffic is saved by a cache).  The byte count charges every listed
A / B block once per use plus C and the bias once (beta = 0) -- the fused call's traffic; three_pass moves C five times.  The operands are allocated as several
sets, together more than twice the 256 MiB Infinity Cache, and a step takes the next set.  A step is timed with device events on torch's stream; the median over
--steps warm steps is reported.  `three_pass` is measured --repeats times per workload, interleaved with `fused`: the spread of its medians (max - min) / min is
the run-to-run spread that a difference has to exceed, and is recorded in every line.

  python tools/bench_segments_fused.py --steps 200 --warmup 20 --out profiles/r12_segments_fused.jsonl
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

from bench_segments import KINDS, LLC, NSEG, PATTERNS, PEAK, OperandSet, draw_counts  # noqa: E402
from libxsmm_amd import capi  # noqa: E402
from libxsmm_amd.capi import BINARY, BINARY_FLAG, DT, GEMM_FLAG, UNARY  # noqa: E402

FUSED_KINDS = ("f32_32", "bf16_vnni_64_c_bf16")


class FusedSet(OperandSet):
    """The plain workload's operand set plus one bias vector per C block (in C's order, so the un-fused passes are strided batches) and d_list."""

    def __init__(self, kind, counts):
        super().__init__(kind, counts)
        e = kind["e"]
        self.D = torch.randint(-4, 5, (NSEG * e,), device="cuda", dtype=torch.int32).to(kind["ctorch"])
        self.ld = torch.from_numpy(np.ascontiguousarray(self.D.data_ptr() + self.rank * e * self.csz, dtype=np.int64)).to("cuda")
        self.bytes += NSEG * e * self.csz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loop-steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_segments_fused.jsonl"))
    ap.add_argument("--kinds", default=",".join(FUSED_KINDS))
    ap.add_argument("--patterns", default=",".join(PATTERNS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_segments_fused.py needs a GPU: nothing is measured without one")
    api = capi.load()
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    api.hip_set_async(1)
    lines = []
    for kname in args.kinds.split(","):
        kind = KINDS[kname]
        e = kind["e"]
        shape = capi.gemm_shape(e, e, e, e, e, e, kind["t"], kind["t"], kind["c"], kind["comp"])
        adr = capi.br_config(capi.BR_ADDRESS, 0, 0, 0)
        flags = kind["flags"] | GEMM_FLAG.BETA_0
        h = api.dispatch_brgemm(shape, flags, 0, adr)
        hx = api.dispatch_brgemm_ext(shape, flags, 0, adr, capi.argops_cp(e, UNARY.RELU), capi.postops_colbias(e, kind["c"]))
        hb = api.dispatch_meltw_binary(BINARY.ADD, capi.BinaryShape(e, e, e, e, e, kind["c"], kind["c"], kind["c"], DT.F32), BINARY_FLAG.BCAST_COL_IN_0)
        hu = api.dispatch_meltw_unary(UNARY.RELU, capi.UnaryShape(e, e, e, e, kind["c"], kind["c"], DT.F32), 0)
        assert h and hx and hb and hu, kname
        for pattern in args.patterns.split(","):
            counts = draw_counts(pattern, np.random.default_rng(11))
            first = FusedSet(kind, counts)
            nsets = max(2, -(-2 * LLC // first.bytes) + 1)
            sets = [first] + [FusedSet(kind, counts) for _ in range(nsets - 1)]
            empty, emptyx = capi.GemmParam(), capi.GemmExtParam()

            def fused(s):
                api.hip_gemm_ext_batch_reduce_segments(hx, C.byref(emptyx), NSEG, s.seg_ptr.data_ptr(), s.la.data_ptr(), s.lb.data_ptr(), s.lc.data_ptr(), s.ld.data_ptr(), None)

            def three_pass(s):
                api.hip_gemm_batch_reduce_segments(h, C.byref(empty), NSEG, s.seg_ptr.data_ptr(), s.la.data_ptr(), s.lb.data_ptr(), s.lc.data_ptr())
                tile = s.blk * s.csz
                p = capi.BinaryParam(); p.in0.primary, p.in1.primary, p.out.primary = s.D.data_ptr(), s.C.data_ptr(), s.C.data_ptr()
                api.hip_meltw_binary_batch_strided(hb, C.byref(p), NSEG, e * s.csz, tile, tile)
                q = capi.UnaryParam(); q.in_.primary, q.out.primary = s.C.data_ptr(), s.C.data_ptr()
                api.hip_meltw_unary_batch_strided(hu, C.byref(q), NSEG, tile, tile, 0)

            def loop(s):
                for i in range(NSEG):
                    p = capi.GemmExtParam(); cnt = C.c_ulonglong(int(s.counts[i]))
                    p.a.primary, p.b.primary = s.la.data_ptr() + int(s.seg_ptr_host[i]) * 8, s.lb.data_ptr() + int(s.seg_ptr_host[i]) * 8
                    p.c.primary = s.C.data_ptr() + int(s.rank[i]) * s.blk * s.csz; p.op.tertiary = C.addressof(cnt)
                    p.d.primary = s.D.data_ptr() + int(s.rank[i]) * e * s.csz
                    capi.Api.call(hx, p)

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

            # the two modes give the same C, checked once per workload before anything is timed: small-integer data, so f32 is exact in any order; a bf16 C is
            # rounded once by the fused call and three times by the passes, which may move a result by one unit of bf16 per rounding
            fused(first); torch.cuda.synchronize(); api.check(); got = first.C.clone(); first.C.zero_()
            fused_kernel = api.hip_kernel_name(hx, 1).decode()
            three_pass(first); torch.cuda.synchronize(); api.check()
            if kind["c"] == DT.F32:
                assert torch.equal(got, first.C), f"{kname} {pattern}: the fused call and the three passes disagree"
            else:
                a, b = got.float(), first.C.float()
                assert bool(((a - b).abs() <= 2.0 ** -6 * b.abs()).all()), f"{kname} {pattern}: the fused call and the three passes disagree beyond bf16 rounding"
            assert bool((got >= 0).all()) and bool((got > 0).any())
            fused_us, base_us = [], []
            for _ in range(args.repeats):                        # interleaved repeats: the baseline's own spread
                us, fused_launches = measure(fused, args.steps, args.warmup); fused_us.append(us)
                us, base_launches = measure(three_pass, args.steps, args.warmup); base_us.append(us)
            loop_us, loop_launches = measure(loop, args.loop_steps, 2)
            spread = (max(base_us) - min(base_us)) / min(base_us)
            common = dict(workload=f"{kname}_{pattern}", epilogue="bias+relu", segments=NSEG, products=int(counts.sum()), operand_sets=nsets,
                          algorithmic_bytes=first.bytes, baseline_spread=round(spread, 4), kernel=fused_kernel)
            for mode, us_all, launches, steps in (("fused", fused_us, fused_launches, args.steps), ("three_pass", base_us, base_launches, args.steps),
                                                  ("loop", [loop_us], loop_launches, args.loop_steps)):
                us = statistics.median(us_all)
                rec = dict(common, mode=mode, launches_per_step=launches, us_per_step=round(us, 3), us_medians=[round(x, 3) for x in us_all],
                           fraction_of_8TBs=round(first.bytes / (us * 1e-6) / PEAK, 4), steps=steps)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            del sets, first
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
