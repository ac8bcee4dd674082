"""Fused offset segments (libxsmm_hip_gemm_ext_batch_reduce_segments_offsets, bias + ReLU) against what the library offered for the same result before, on
workloads of 8192 segments -- tools/bench_segments_offsets.py's method and workloads with tools/bench_segments_fused.py's epilogue.

Workloads: f32 32^3 and bf16 64^3 -> bf16 (VNNI A where A is not transposed), with two count patterns: `uniform0_8` (counts drawn uniformly from 0..8) and
`skewed_sorted` (1 % of the segments 64 products, the rest 2, longest first), in the forms NN, TN and NT.  Modes:
  offsets_fused         one call: the bias starts the accumulator, the ReLU sits in front of the store
  offsets_then_passes   the yardstick of every row: the plain offsets call, then libxsmm_hip_meltw_binary_batch_strided (column-broadcast add of the segment's
                        bias) and libxsmm_hip_meltw_unary_batch_strided (ReLU) in place over the contiguous C blocks -- three launches, C traversed three times
  address_fused         NN only, a second yardstick: libxsmm_hip_gemm_ext_batch_reduce_segments on the same blocks (pointer lists = base + offset)
Every product has A and B blocks of its own and every segment a bias vector of its own.  The byte count charges every listed A / B block once plus C and the
bias once (beta = 0): the fused call's traffic.  The operands are allocated as several sets, together more than twice the 256 MiB Infinity Cache, and a step
takes the next set.  A step is timed with device events on torch's stream; the median over --steps warm steps is reported.  All modes are measured --repeats
times, interleaved: the spread of the yardstick's medians (max - min) / min is the run-to-run spread that a difference has to exceed, and is recorded in every
line.  The results are compared before anything is timed: bit for bit for f32 (exact small-integer data) and against address_fused; a bf16 C is rounded once by
the fused call and three times by the passes, which may move a result by one unit of bf16 per rounding.

  python tools/bench_segments_offsets_fused.py --steps 200 --warmup 20 --out profiles/r14_segments_offsets_fused.jsonl
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

from bench_segments_offsets import FORMS, KINDS, LLC, NSEG, PATTERNS, PEAK, draw_counts  # noqa: E402
from libxsmm_amd import capi  # noqa: E402
from libxsmm_amd.capi import BINARY, BINARY_FLAG, DT, GEMM_FLAG, UNARY  # noqa: E402


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to("cuda")


class FusedOffsetSet:
    """One set of operands on the device: product r owns A block r and B block r, segment s owns C block s and bias vector s; for NN the ADDRESS lists of this
    set.  The OFFSET lists are shared by all sets (they do not depend on the addresses)."""

    def __init__(self, kind, counts, form):
        e, dt = kind["e"], kind["torch"]
        self.blk, self.esz = e * e, capi.DT_SIZE[kind["t"]]
        self.total = total = int(counts.sum())
        n = max(total, 1) * self.blk
        self.A = torch.randint(-2, 3, (n,), device="cuda", dtype=torch.int32).to(dt)
        self.B = torch.randint(-2, 3, (n,), device="cuda", dtype=torch.int32).to(dt)
        self.C = torch.zeros(NSEG * self.blk, device="cuda", dtype=dt)
        self.D = torch.randint(-4, 5, (NSEG * e,), device="cuda", dtype=torch.int32).to(dt)
        if form == "NN":
            prod, seg = np.arange(total, dtype=np.int64) * self.blk * self.esz, np.arange(NSEG, dtype=np.int64)
            self.la, self.lb = dev(self.A.data_ptr() + prod), dev(self.B.data_ptr() + prod)
            self.lc, self.ld = dev(self.C.data_ptr() + seg * self.blk * self.esz), dev(self.D.data_ptr() + seg * e * self.esz)
        self.bytes = total * 2 * self.blk * self.esz + NSEG * self.blk * self.esz + NSEG * e * self.esz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_segments_offsets_fused.jsonl"))
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--patterns", default=",".join(PATTERNS))
    ap.add_argument("--forms", default=",".join(FORMS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_segments_offsets_fused.py needs a GPU: nothing is measured without one")
    api = capi.load()
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    api.hip_set_async(1)
    lines = []
    for kname in args.kinds.split(","):
        kind = KINDS[kname]
        e, t, c = kind["e"], kind["t"], kind["c"]
        shape = capi.gemm_shape(e, e, e, e, e, e, t, t, c, DT.F32)
        relu, bias = capi.argops_cp(e, UNARY.RELU), capi.postops_colbias(e, c)
        hb = api.dispatch_meltw_binary(BINARY.ADD, capi.BinaryShape(e, e, e, e, e, c, c, c, DT.F32), BINARY_FLAG.BCAST_COL_IN_0)
        hu = api.dispatch_meltw_unary(UNARY.RELU, capi.UnaryShape(e, e, e, e, c, c, DT.F32), 0)
        assert hb and hu, kname
        for form in args.forms.split(","):
            vnni = 0 if form == "TN" else kind["vnni"]                  # a transposed A is flat (VNNI-2 and TRANS_A exclude each other)
            flags = vnni | FORMS[form] | GEMM_FLAG.BETA_0
            off, adr = capi.br_config(capi.BR_OFFSET, 0, 0, 0), capi.br_config(capi.BR_ADDRESS, 0, 0, 0)
            hx_off = api.dispatch_brgemm_ext(shape, flags, 0, off, relu, bias)
            h_off = api.dispatch_brgemm(shape, flags, 0, off)
            hx_adr = api.dispatch_brgemm_ext(shape, flags, 0, adr, relu, bias) if form == "NN" else None
            assert hx_off and h_off and (hx_adr or form != "NN"), (kname, form)
            for pattern in args.patterns.split(","):
                counts = draw_counts(pattern, np.random.default_rng(13))
                first = FusedOffsetSet(kind, counts, form)
                nsets = max(2, -(-2 * LLC // first.bytes) + 1)
                sets = [first] + [FusedOffsetSet(kind, counts, form) for _ in range(nsets - 1)]
                tile, vec = first.blk * first.esz, e * first.esz
                seg_ptr = dev(np.concatenate([[0], np.cumsum(counts)]))
                o_ab, o_c, o_d = dev(np.arange(first.total, dtype=np.int64) * tile), dev(np.arange(NSEG, dtype=np.int64) * tile), dev(np.arange(NSEG, dtype=np.int64) * vec)
                emptyx = capi.GemmExtParam()

                def fused(s):
                    p = capi.GemmExtParam()
                    p.a.primary, p.b.primary, p.c.primary, p.d.primary = s.A.data_ptr(), s.B.data_ptr(), s.C.data_ptr(), s.D.data_ptr()
                    api.hip_gemm_ext_batch_reduce_segments_offsets(hx_off, C.byref(p), NSEG, seg_ptr.data_ptr(), o_ab.data_ptr(), o_ab.data_ptr(), o_c.data_ptr(),
                                                                   o_d.data_ptr(), None)

                def passes(s):
                    p = capi.GemmParam()
                    p.a.primary, p.b.primary, p.c.primary = s.A.data_ptr(), s.B.data_ptr(), s.C.data_ptr()
                    api.hip_gemm_batch_reduce_segments_offsets(h_off, C.byref(p), NSEG, seg_ptr.data_ptr(), o_ab.data_ptr(), o_ab.data_ptr(), o_c.data_ptr())
                    b = capi.BinaryParam(); b.in0.primary, b.in1.primary, b.out.primary = s.D.data_ptr(), s.C.data_ptr(), s.C.data_ptr()
                    api.hip_meltw_binary_batch_strided(hb, C.byref(b), NSEG, vec, tile, tile)
                    q = capi.UnaryParam(); q.in_.primary, q.out.primary = s.C.data_ptr(), s.C.data_ptr()
                    api.hip_meltw_unary_batch_strided(hu, C.byref(q), NSEG, tile, tile, 0)

                def address(s):
                    api.hip_gemm_ext_batch_reduce_segments(hx_adr, C.byref(emptyx), NSEG, seg_ptr.data_ptr(), s.la.data_ptr(), s.lb.data_ptr(), s.lc.data_ptr(),
                                                           s.ld.data_ptr(), None)

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

                # the modes give the same C, checked once per workload before anything is timed
                fused(first); torch.cuda.synchronize(); api.check(); got = first.C.clone(); first.C.zero_()
                kernel = api.hip_kernel_name(hx_off, 1).decode()
                passes(first); torch.cuda.synchronize(); api.check()
                if c == DT.F32:
                    assert torch.equal(got, first.C), f"{kname} {form} {pattern}: the fused call and the three passes disagree"
                else:
                    a, b = got.float(), first.C.float()
                    assert bool(((a - b).abs() <= 2.0 ** -6 * b.abs()).all()), f"{kname} {form} {pattern}: the fused call and the three passes disagree beyond bf16 rounding"
                assert bool((got >= 0).all()) and bool((got > 0).any())
                modes = [("offsets_fused", fused), ("offsets_then_passes", passes)]
                if form == "NN":
                    first.C.zero_(); address(first); torch.cuda.synchronize(); api.check()
                    assert torch.equal(got, first.C), f"{kname} {form} {pattern}: the fused offsets call and the fused ADDRESS call disagree"
                    modes.append(("address_fused", address))
                us_all, launches = {m: [] for m, _ in modes}, {}
                for _ in range(args.repeats):                        # interleaved repeats: the yardstick's own spread
                    for m, fn in modes:
                        us, launches[m] = measure(fn, args.steps, args.warmup); us_all[m].append(us)
                base = us_all["offsets_then_passes"]
                spread = (max(base) - min(base)) / min(base)
                common = dict(workload=f"{kname}_{form}_{pattern}", epilogue="bias+relu", segments=NSEG, products=int(counts.sum()), operand_sets=nsets,
                              algorithmic_bytes=first.bytes, yardstick_spread=round(spread, 4), kernel=kernel)
                for m, _ in modes:
                    us = statistics.median(us_all[m])
                    rec = dict(common, mode=m, launches_per_step=launches[m], us_per_step=round(us, 3), us_medians=[round(x, 3) for x in us_all[m]],
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
