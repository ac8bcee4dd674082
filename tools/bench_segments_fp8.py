"""8-bit float segments (BF8 / HF8 handles in libxsmm_hip_gemm_batch_reduce_segments) against what a caller had before and against the bf16 segments call.

Workload: the count pattern of a block-sparse layer Y = W X of 64 x 64 blocks -- 256 block rows of W, 64 block columns, 16 block columns of X, so 4096 segments
of 64^3 products -- at three densities of W (1/16, 1/8, 1/4 of a block row's 64 blocks stored).  The counts are skewed: 5 % of the block rows hold four times
the blocks of the others (4 / 16, 8 / 32, 16 / 64 products per segment), in list order.  Kinds: HF8 -> f32, HF8 -> HF8, BF8 -> f32.
Modes per workload:
  segments        one call through the 8-bit float handle
  per_count       what the library offered for these handles before: one libxsmm_hip_gemm_batch_strided launch per distinct count over lists and C blocks
                  that the script re-sorted so that equal counts are contiguous (the re-sort is outside the timed region, and the segments call runs on the
                  same re-sorted memory: generous to this baseline)
  bf16_segments   the bf16 (VNNI-2 A) segments call on the same pattern with C of the matching width (f32, or bf16 for an 8-bit C): twice the operand bytes
Every product has A and B blocks of its own, so nothing is re-read from a cache inside a step; the byte count charges every listed A / B block once plus C
once (beta = 0).  The operands are allocated as several sets, together more than twice the 256 MiB Infinity Cache, and a step takes the next set.  A step is
timed with device events on torch's stream; the median over --steps warm steps is reported with the fraction of 8 TB/s on the mode's own algorithmic bytes.
Every mode is measured --repeats times, interleaved: the spread of the baseline's medians (max - min) / min is the run-to-run spread that a difference has to
exceed, and is recorded in every line.  The data are exact (0, +-1/2, +-1, +-2), so the 8-bit modes must agree bit for bit: checked before anything is timed.

  python tools/bench_segments_fp8.py --steps 200 --warmup 20 --out profiles/r21_segments_fp8.jsonl
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
E, MB, KB, NB = 64, 256, 64, 16
NSEG = MB * NB
# the bytes of 0, +-1/2, +-1, +-2
CODES = {DT.HF8: [0x00, 0x30, 0xb0, 0x38, 0xb8, 0x40, 0xc0], DT.BF8: [0x00, 0x38, 0xb8, 0x3c, 0xbc, 0x40, 0xc0]}
KINDS = {
    "hf8_f32": dict(t=DT.HF8, c=DT.F32, bf16_c=DT.F32),
    "hf8_hf8": dict(t=DT.HF8, c=DT.HF8, bf16_c=DT.BF16),
    "bf8_f32": dict(t=DT.BF8, c=DT.F32, bf16_c=DT.F32),
}
TORCH_OF = {DT.F32: torch.float32, DT.BF16: torch.bfloat16, DT.HF8: torch.uint8, DT.BF8: torch.uint8}
DENSITIES = {"d1_16": 4, "d1_8": 8, "d1_4": 16}


def draw_counts(base, rng):
    """Products per segment: a block row's count for each of its NB segments; 5 % of the block rows hold 4 x base blocks."""
    rows = np.where(rng.random(MB) < 0.05, min(4 * base, KB), base).astype(np.int64)
    return np.repeat(rows, NB)


class OperandSet:
    """One set of operands and lists on the device.  Product r owns A block r and B block r; C is laid out in count-sorted order (rank), so the segments of
    one count are a strided batch for the baseline, and the sorted lists are the segment lists gathered in that order."""

    def __init__(self, t, c, counts):
        blk = E * E
        esz, csz = capi.DT_SIZE[t], capi.DT_SIZE[c]
        total = int(counts.sum())
        if t in CODES:
            table = torch.tensor(CODES[t], dtype=torch.uint8, device="cuda")
            self.A = table[torch.randint(0, len(CODES[t]), (total * blk,), device="cuda")]
            self.B = table[torch.randint(0, len(CODES[t]), (total * blk,), device="cuda")]
        else:
            self.A = torch.randint(-2, 3, (total * blk,), device="cuda", dtype=torch.int32).to(TORCH_OF[t])
            self.B = torch.randint(-2, 3, (total * blk,), device="cuda", dtype=torch.int32).to(TORCH_OF[t])
        self.C = torch.zeros(NSEG * blk, device="cuda", dtype=TORCH_OF[c])
        seg_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        order = np.argsort(-counts, kind="stable")                   # segments by descending count: equal counts contiguous
        rank = np.empty(NSEG, dtype=np.int64); rank[order] = np.arange(NSEG)
        prod = np.arange(total, dtype=np.int64)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to("cuda")      # noqa: E731
        self.seg_ptr = dev(seg_ptr)
        self.la, self.lb = dev(self.A.data_ptr() + prod * blk * esz), dev(self.B.data_ptr() + prod * blk * esz)
        self.lc = dev(self.C.data_ptr() + rank * blk * csz)
        gather = np.concatenate([np.arange(seg_ptr[s], seg_ptr[s + 1]) for s in order])
        self.sla, self.slb = dev(self.A.data_ptr() + gather * blk * esz), dev(self.B.data_ptr() + gather * blk * esz)
        self.launches = []                                           # (count, elements, first product in the sorted lists, first C rank)
        sc = counts[order]
        first_prod = np.concatenate([[0], np.cumsum(sc)])
        for d in sorted(set(sc.tolist()), reverse=True):
            idx = np.flatnonzero(sc == d)
            self.launches.append((int(d), len(idx), int(first_prod[idx[0]]), int(idx[0])))
        self.blk, self.csz = blk, csz
        self.bytes = total * 2 * blk * esz + NSEG * blk * csz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_segments_fp8.jsonl"))
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--densities", default=",".join(DENSITIES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_segments_fp8.py needs a GPU: nothing is measured without one")
    api = capi.load()
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    api.hip_set_async(1)
    adr = capi.br_config(capi.BR_ADDRESS, 0, 0, 0)
    lines = []
    for kname in args.kinds.split(","):
        kind = KINDS[kname]
        h = api.dispatch_brgemm(capi.gemm_shape(E, E, E, E, E, E, kind["t"], kind["t"], kind["c"], DT.F32), GEMM_FLAG.VNNI_A | GEMM_FLAG.BETA_0, 0, adr)
        hb = api.dispatch_brgemm(capi.gemm_shape(E, E, E, E, E, E, DT.BF16, DT.BF16, kind["bf16_c"], DT.F32), GEMM_FLAG.VNNI_A | GEMM_FLAG.BETA_0, 0, adr)
        assert h and hb, kname
        for dname in args.densities.split(","):
            counts = draw_counts(DENSITIES[dname], np.random.default_rng(21))
            first = OperandSet(kind["t"], kind["c"], counts)
            nsets = max(2, -(-2 * LLC // first.bytes) + 1)
            sets = [first] + [OperandSet(kind["t"], kind["c"], counts) for _ in range(nsets - 1)]
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

            # the two 8-bit modes give the same C (exact data): checked once per workload before anything is timed
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
            med = {m: statistics.median(v) for m, v in us.items()}
            common = dict(workload=f"{kname}_{dname}", segments=NSEG, products=int(counts.sum()), distinct_counts=len(first.launches), operand_sets=nsets,
                          baseline_spread=round(spread, 4))
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


if __name__ == "__main__":
    main()
