"""Offset segments (libxsmm_hip_gemm_batch_reduce_segments_offsets) against what the library offered for the same result before, on workloads of 8192 segments.

Workloads: f32 32^3 and bf16 64^3 -> bf16, with two count patterns: `uniform0_8` (counts drawn uniformly from 0..8) and `skewed_sorted` (1 % of the segments
64 products, the rest 2, longest first).  Forms and their yardsticks:
  NN   (bf16: VNNI A)  the ADDRESS segments call on the same blocks (pointer lists = base + offset): an unchanged kernel; the offsets form adds one 64-bit
                       add per product
  TN   (A transposed)  one libxsmm_hip_meltw_unary_batch_strided transpose pass over the listed A blocks into scratch, then the ADDRESS call on the scratch
  NT   (B transposed)  the same with the listed B blocks (bf16: A stays VNNI)
Every product has A and B blocks of its own, so the listed blocks of an operand are one strided batch for the transpose pass.  The byte count charges every
listed A / B block once plus C once (beta = 0); the yardstick's extra traffic through the scratch is NOT charged: both modes are rated on the bytes the result
needs.  The operands are allocated as several sets, together more than twice the 256 MiB Infinity Cache, and a step takes the next set.  A step is timed with
device events on torch's stream; the median over --steps warm steps is reported.  Both modes are measured --repeats times, interleaved: the spread of the
yardstick's medians (max - min) / min is the run-to-run spread that a difference has to exceed, and is recorded in every line.  The two modes' results are
compared bit for bit (exact small-integer data) before anything is timed.

  python tools/bench_segments_offsets.py --steps 200 --warmup 20 --out profiles/r13_segments_offsets.jsonl
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
from libxsmm_amd.capi import DT, GEMM_FLAG, UNARY  # noqa: E402

PEAK = 8e12
LLC = 256 << 20
NSEG = 8192
KINDS = {
    "f32_32": dict(t=DT.F32, c=DT.F32, e=32, vnni=0, torch=torch.float32),
    "bf16_64_c_bf16": dict(t=DT.BF16, c=DT.BF16, e=64, vnni=GEMM_FLAG.VNNI_A, torch=torch.bfloat16),
}
PATTERNS = ("uniform0_8", "skewed_sorted")
FORMS = {"NN": 0, "TN": GEMM_FLAG.TRANS_A, "NT": GEMM_FLAG.TRANS_B}


def draw_counts(pattern, rng):
    if pattern == "uniform0_8":
        return rng.integers(0, 9, NSEG).astype(np.int64)
    counts = np.where(rng.random(NSEG) < 0.01, 64, 2).astype(np.int64)
    return np.sort(counts)[::-1].copy()


class OperandSet:
    """One set of operands on the device: product r owns A block r and B block r, segment s owns C block s; a scratch the size of one operand for the yardstick's
    transposed copies; the ADDRESS lists of this set.  The OFFSET lists are shared by all sets (they do not depend on the addresses)."""

    def __init__(self, kind, counts, form):
        e, dt = kind["e"], kind["torch"]
        self.blk, self.esz = e * e, capi.DT_SIZE[kind["t"]]
        self.total = total = int(counts.sum())
        n = max(total, 1) * self.blk
        self.A = torch.randint(-2, 3, (n,), device="cuda", dtype=torch.int32).to(dt)
        self.B = torch.randint(-2, 3, (n,), device="cuda", dtype=torch.int32).to(dt)
        self.C = torch.zeros(NSEG * self.blk, device="cuda", dtype=dt)
        self.scratch = torch.zeros(n, device="cuda", dtype=dt) if form != "NN" else None
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to("cuda")
        prod = np.arange(total, dtype=np.int64) * self.blk * self.esz
        a_src = self.scratch if form == "TN" else self.A                 # the ADDRESS call reads the transposed copies
        b_src = self.scratch if form == "NT" else self.B
        self.la, self.lb = dev(a_src.data_ptr() + prod), dev(b_src.data_ptr() + prod)
        self.lc = dev(self.C.data_ptr() + np.arange(NSEG, dtype=np.int64) * self.blk * self.esz)
        self.bytes = total * 2 * self.blk * self.esz + NSEG * self.blk * self.esz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_segments_offsets.jsonl"))
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--patterns", default=",".join(PATTERNS))
    ap.add_argument("--forms", default=",".join(FORMS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_segments_offsets.py needs a GPU: nothing is measured without one")
    api = capi.load()
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    api.hip_set_async(1)
    lines = []
    for kname in args.kinds.split(","):
        kind = KINDS[kname]
        e, t = kind["e"], kind["t"]
        shape = capi.gemm_shape(e, e, e, e, e, e, t, t, kind["c"], DT.F32)
        transpose = api.dispatch_meltw_unary(UNARY.TRANSFORM_NORM_TO_NORMT, capi.UnaryShape(e, e, e, e, t, t, t), 0)
        assert transpose, kname
        for form in args.forms.split(","):
            # a transposed A is flat (VNNI-2 and TRANS_A exclude each other); the yardstick then reads the flat transposed copies
            vnni = 0 if form == "TN" else kind["vnni"]
            h_off = api.dispatch_brgemm(shape, vnni | FORMS[form] | GEMM_FLAG.BETA_0, 0, capi.br_config(capi.BR_OFFSET, 0, 0, 0))
            h_adr = api.dispatch_brgemm(shape, vnni | GEMM_FLAG.BETA_0, 0, capi.br_config(capi.BR_ADDRESS, 0, 0, 0))
            assert h_off and h_adr, (kname, form)
            for pattern in args.patterns.split(","):
                counts = draw_counts(pattern, np.random.default_rng(13))
                first = OperandSet(kind, counts, form)
                nsets = max(2, -(-2 * LLC // first.bytes) + 1)
                sets = [first] + [OperandSet(kind, counts, form) for _ in range(nsets - 1)]
                dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to("cuda")
                step_b = first.blk * first.esz
                seg_ptr = dev(np.concatenate([[0], np.cumsum(counts)]))
                o_ab, o_c = dev(np.arange(first.total, dtype=np.int64) * step_b), dev(np.arange(NSEG, dtype=np.int64) * step_b)
                empty = capi.GemmParam()

                def offsets(s):
                    p = capi.GemmParam()
                    p.a.primary, p.b.primary, p.c.primary = s.A.data_ptr(), s.B.data_ptr(), s.C.data_ptr()
                    api.hip_gemm_batch_reduce_segments_offsets(h_off, C.byref(p), NSEG, seg_ptr.data_ptr(), o_ab.data_ptr(), o_ab.data_ptr(), o_c.data_ptr())

                def yardstick(s):
                    if form != "NN" and s.total:
                        u = capi.UnaryParam()
                        u.in_.primary, u.out.primary = (s.A if form == "TN" else s.B).data_ptr(), s.scratch.data_ptr()
                        api.hip_meltw_unary_batch_strided(transpose, C.byref(u), s.total, step_b, step_b, 0)
                    api.hip_gemm_batch_reduce_segments(h_adr, C.byref(empty), NSEG, seg_ptr.data_ptr(), s.la.data_ptr(), s.lb.data_ptr(), s.lc.data_ptr())

                def measure(fn, steps, warmup):
                    for i in range(warmup):
                        fn(sets[i % nsets])
                    torch.cuda.synchronize(); api.check()
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
                    api.hip_launch_count(1)
                    for i, (s, t_) in enumerate(ev):
                        s.record(); fn(sets[i % nsets]); t_.record()
                    torch.cuda.synchronize(); api.check()
                    return statistics.median(s.elapsed_time(t_) * 1e3 for s, t_ in ev), api.hip_launch_count(1) / steps

                # the two modes give the same C (exact small-integer data): checked once per workload before anything is timed
                offsets(first); torch.cuda.synchronize(); api.check(); got = first.C.clone(); first.C.zero_()
                kernel = api.hip_kernel_name(h_off, 1).decode()
                yardstick(first); torch.cuda.synchronize(); api.check()
                assert torch.equal(got, first.C) and (got != 0).any(), f"{kname} {form} {pattern}: the offsets call and its yardstick disagree"
                off_us, base_us = [], []
                for _ in range(args.repeats):                        # interleaved repeats: the yardstick's own spread
                    us, off_launches = measure(offsets, args.steps, args.warmup); off_us.append(us)
                    us, base_launches = measure(yardstick, args.steps, args.warmup); base_us.append(us)
                spread = (max(base_us) - min(base_us)) / min(base_us)
                common = dict(workload=f"{kname}_{form}_{pattern}", segments=NSEG, products=int(counts.sum()), operand_sets=nsets, algorithmic_bytes=first.bytes,
                              yardstick_spread=round(spread, 4), kernel=kernel)
                for mode, us_all, launches in (("offsets", off_us, off_launches), ("address" if form == "NN" else "transpose_then_address", base_us, base_launches)):
                    us = statistics.median(us_all)
                    rec = dict(common, mode=mode, launches_per_step=launches, us_per_step=round(us, 3), us_medians=[round(x, 3) for x in us_all],
                               fraction_of_8TBs=round(first.bytes / (us * 1e-6) / PEAK, 4), steps=args.steps)
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
