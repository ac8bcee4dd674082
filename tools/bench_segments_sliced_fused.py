"""Sliced segments with a fused epilogue (libxsmm_hip_gemm_ext_batch_reduce_segments_offsets_sliced) against two yardsticks measured in the same process:
  (a) unsliced_fused       the unsliced ext entry on the same lists (libxsmm_hip_gemm_ext_batch_reduce_segments_offsets): one launch, one wave per chain
  (b) sliced_then_passes   what a caller did before: the plain sliced entry on the matching plain handle, then two TPP passes over C -- the column-bias add and
                           the ReLU (with its bitmask where the workload has one): four launches and one more round trip of C

Workloads (OFFSET NN, beta = 0, one bias vector per block):
  conv_f32             a 3 x 3 convolution forward on a 7 x 7 image with 512 channels in 32-wide blocks, as f32 32^3 products: 16 x 7 = 112 C blocks, each a chain
                       of 16 x 9 = 144 products (the weight block of an (output block, input block, tap) is shared by the 7 rows, the input block of an (input
                       block, row, tap) by the 16 output blocks); bias + ReLU + bitmask; chains cut into slices of 8 and of 16 products
  conv_bf16            the same lists on bf16 VNNI-A 64^3 -> bf16 products
  skew_f32             8192 blocks, 1 % of them 64 products, the rest 2, in list order (the list of DESIGN.md section 9.5); bias + ReLU; only the long chains
                       are cut, into 8 slices
  uniform4_f32         8192 blocks of 4 products, one slice per block; bias + ReLU + bitmask: the fused sliced call does the work of (a) plus its second pass --
                       the expected loss
The method is that of tools/bench_segments_sliced.py: the operands are allocated as several sets, together more than twice the 256 MiB Infinity Cache, and a step
takes the next set; the lists and the ONE workspace a caller would reuse are shared by the sets; a step is timed with device events on torch's stream; the median
over --steps warm steps is reported; every mode is measured --repeats times, interleaved, and the spread of a yardstick's medians (max - min) / min is what a
difference has to exceed.  All modes of a workload are compared before anything is timed: exact small-integer data, so C and the mask agree bit for bit
(the passes of (b) round a bf16 C three times where the fused calls round once: compared within bf16 rounding there).

  python tools/bench_segments_sliced_fused.py --steps 200 --warmup 20 --out profiles/r20_segments_sliced_fused.jsonl
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
from libxsmm_amd.capi import BINARY, BINARY_FLAG, DT, GEMM_FLAG, UNARY, UNARY_FLAG  # noqa: E402

LLC = 256 << 20
F32 = dict(t=DT.F32, c=DT.F32, e=32, vnni=0, torch=torch.float32)
BF16 = dict(t=DT.BF16, c=DT.BF16, e=64, vnni=GEMM_FLAG.VNNI_A, torch=torch.bfloat16)


def csr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def conv_lists(kb=16, cb=16, h=7, taps=9):
    """Block (k, row) walks (c, tap): A = the weight block (k, c, tap), shared by the rows; B = the input block (c, row, tap), shared by the output blocks."""
    k, r, c, t = np.meshgrid(np.arange(kb), np.arange(h), np.arange(cb), np.arange(taps), indexing="ij")
    a_idx, b_idx = ((k * cb + c) * taps + t).ravel(), ((c * h + r) * taps + t).ravel()
    return np.full(kb * h, cb * taps, dtype=np.int64), (a_idx, b_idx, kb * cb * taps, cb * h * taps)


def own_blocks(counts):
    total = int(counts.sum())
    return np.arange(total, dtype=np.int64), np.arange(total, dtype=np.int64), total, total


def workloads():
    rng = np.random.default_rng(16)
    w = {}
    counts, ops = conv_lists()
    w["conv_f32"] = dict(kind=F32, counts=counts, ops=ops, mask=True, cuts={f"slices_of_{n}": ("length", n) for n in (8, 16)})
    w["conv_bf16"] = dict(kind=BF16, counts=counts, ops=ops, mask=True, cuts={f"slices_of_{n}": ("length", n) for n in (8, 16)})
    c = np.where(rng.random(8192) < 0.01, 64, 2).astype(np.int64)
    w["skew_f32"] = dict(kind=F32, counts=c, ops=own_blocks(c), mask=False, cuts={"long_into_8": ("long", 8)})
    c = np.full(8192, 4, dtype=np.int64)
    w["uniform4_f32"] = dict(kind=F32, counts=c, ops=own_blocks(c), mask=True, cuts={"one_slice_per_block": ("length", 4)})
    return w


def cut(counts, how):
    """The products of every block cut into slices: ("length", n) slices of n products; ("long", n) chains of 64 and more into n slices, the others one slice."""
    per_block, lengths = [], []
    for cnt in counts.tolist():
        if how[0] == "length":
            ls = [how[1]] * (cnt // how[1]) + ([cnt % how[1]] if cnt % how[1] else [])
        else:
            ls = [cnt // how[1]] * how[1] if cnt >= 64 else [cnt]
        per_block.append(len(ls)); lengths += ls
    return csr(np.asarray(per_block)), csr(np.asarray(lengths))


class OperandSet:
    def __init__(self, wl):
        kind = wl["kind"]
        e = kind["e"]
        self.blk, self.esz = e * e, capi.DT_SIZE[kind["t"]]
        _, _, na, nb = wl["ops"]
        nblocks = len(wl["counts"])
        mk = lambda n: torch.randint(-1, 2, (n,), device="cuda", dtype=torch.int32).to(kind["torch"])
        self.A, self.B, self.D = mk(na * self.blk), mk(nb * self.blk), mk(nblocks * e)
        self.C = torch.zeros(nblocks * self.blk, device="cuda", dtype=kind["torch"])
        self.M = torch.zeros(nblocks * (e // 8) * e, device="cuda", dtype=torch.uint8)
        # every block of the operands and the bias once, C once (beta = 0), the mask once
        self.bytes = (na + nb + nblocks) * self.blk * self.esz + nblocks * e * self.esz + (self.M.numel() if wl["mask"] else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_segments_sliced_fused.jsonl"))
    ap.add_argument("--workloads", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_segments_sliced_fused.py needs a GPU: nothing is measured without one")
    api = capi.load()
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    api.hip_set_async(1)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to("cuda")
    lines = []
    todo = workloads()
    for name in (args.workloads.split(",") if args.workloads else list(todo)):
        wl = todo[name]
        kind, counts, mask = wl["kind"], wl["counts"], wl["mask"]
        e, t, c = kind["e"], kind["t"], kind["c"]
        nblocks = len(counts)
        shape = capi.gemm_shape(e, e, e, e, e, e, t, t, c, DT.F32)
        off = capi.br_config(capi.BR_OFFSET, 0, 0, 0)
        flags = kind["vnni"] | GEMM_FLAG.BETA_0
        relu_flag = UNARY_FLAG.BITMASK_2BYTEMULT if mask else 0
        hx = api.dispatch_brgemm_ext(shape, flags, 0, off, capi.argops_cp(e, UNARY.RELU, relu_flag), capi.postops_colbias(e, c))
        hp = api.dispatch_brgemm(shape, flags, 0, off)
        hb = api.dispatch_meltw_binary(BINARY.ADD, capi.BinaryShape(e, e, e, e, e, c, c, c, DT.F32), BINARY_FLAG.BCAST_COL_IN_0)
        hu = api.dispatch_meltw_unary(UNARY.RELU, capi.UnaryShape(e, e, e, e, c, c, DT.F32), relu_flag)
        assert hx and hp and hb and hu, name
        first = OperandSet(wl)
        nsets = max(2, -(-2 * LLC // first.bytes) + 1)
        sets = [first] + [OperandSet(wl) for _ in range(nsets - 1)]
        tile, vec, mblk = first.blk * first.esz, e * first.esz, (e // 8) * e
        seq = np.arange(nblocks, dtype=np.int64)
        seg_unsliced = dev(csr(counts))
        o_a, o_b, o_c, o_d, o_m = dev(wl["ops"][0] * tile), dev(wl["ops"][1] * tile), dev(seq * tile), dev(seq * vec), dev(seq * mblk)
        lm = o_m.data_ptr() if mask else None

        def xparam(s):
            p = capi.GemmExtParam()
            p.a.primary, p.b.primary, p.c.primary, p.d.primary, p.c.secondary = s.A.data_ptr(), s.B.data_ptr(), s.C.data_ptr(), s.D.data_ptr(), s.M.data_ptr()
            return p

        def unsliced_fused(s):
            api.hip_gemm_ext_batch_reduce_segments_offsets(hx, C.byref(xparam(s)), nblocks, seg_unsliced.data_ptr(), o_a.data_ptr(), o_b.data_ptr(), o_c.data_ptr(),
                                                           o_d.data_ptr(), lm)

        modes = {"unsliced_fused": unsliced_fused}
        info = {"unsliced_fused": dict(slices=nblocks, workspace_bytes=0)}
        keep = []
        for cname, how in wl["cuts"].items():
            blk_ptr, seg_ptr = cut(counts, how)
            nslices = len(seg_ptr) - 1
            nbytes = api.hip_gemm_ext_batch_reduce_segments_sliced_workspace(hx, nslices)
            assert nbytes == api.hip_gemm_batch_reduce_segments_sliced_workspace(hp, nslices)
            ws = torch.empty(max(nbytes, 16), device="cuda", dtype=torch.uint8)
            d_blk, d_seg = dev(blk_ptr), dev(seg_ptr)
            keep += [ws, d_blk, d_seg]

            def sliced_fused(s, d_blk=d_blk, d_seg=d_seg, ws=ws, nslices=nslices, nbytes=nbytes):
                api.hip_gemm_ext_batch_reduce_segments_offsets_sliced(hx, C.byref(xparam(s)), nblocks, d_blk.data_ptr(), nslices, d_seg.data_ptr(), o_a.data_ptr(),
                                                                      o_b.data_ptr(), o_c.data_ptr(), o_d.data_ptr(), lm, ws.data_ptr(), nbytes)

            def sliced_then_passes(s, d_blk=d_blk, d_seg=d_seg, ws=ws, nslices=nslices, nbytes=nbytes):
                p = capi.GemmParam()
                p.a.primary, p.b.primary, p.c.primary = s.A.data_ptr(), s.B.data_ptr(), s.C.data_ptr()
                api.hip_gemm_batch_reduce_segments_offsets_sliced(hp, C.byref(p), nblocks, d_blk.data_ptr(), nslices, d_seg.data_ptr(), o_a.data_ptr(), o_b.data_ptr(),
                                                                  o_c.data_ptr(), ws.data_ptr(), nbytes)
                b = capi.BinaryParam(); b.in0.primary, b.in1.primary, b.out.primary = s.D.data_ptr(), s.C.data_ptr(), s.C.data_ptr()
                api.hip_meltw_binary_batch_strided(hb, C.byref(b), nblocks, vec, tile, tile)
                q = capi.UnaryParam(); q.in_.primary, q.out.primary = s.C.data_ptr(), s.C.data_ptr()
                if mask:
                    q.out.secondary = s.M.data_ptr()
                api.hip_meltw_unary_batch_strided(hu, C.byref(q), nblocks, tile, tile, mblk if mask else 0)

            modes[cname + "_fused"] = sliced_fused
            modes[cname + "_then_passes"] = sliced_then_passes
            info[cname + "_fused"] = info[cname + "_then_passes"] = dict(slices=nslices, workspace_bytes=int(nbytes))

        def measure(fn):
            for i in range(args.warmup):
                fn(sets[i % nsets])
            torch.cuda.synchronize(); api.check()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            api.hip_launch_count(1)
            for i, (s, t_) in enumerate(ev):
                s.record(); fn(sets[i % nsets]); t_.record()
            torch.cuda.synchronize(); api.check()
            return statistics.median(s.elapsed_time(t_) * 1e3 for s, t_ in ev), api.hip_launch_count(1) / args.steps

        # every mode gives the same C and the same mask (exact small-integer data): checked once per workload before anything is timed
        want = None
        for mname, fn in modes.items():
            first.C.fill_(0.5); first.M.fill_(0xA5)
            fn(first); torch.cuda.synchronize(); api.check()
            if want is None:
                want = (first.C.clone(), first.M.clone())
                assert bool((want[0] >= 0).all()) and bool((want[0] > 0).any()) and (not mask or bool((want[1] != 0xA5).any()))
            if c == DT.BF16 and mname.endswith("_then_passes"):                 # the passes round a bf16 C three times, the fused calls once
                a, b = want[0].float(), first.C.float()
                assert bool(((a - b).abs() <= 2.0 ** -6 * a.abs()).all()), f"{name}: {mname} and the unsliced fused call disagree beyond bf16 rounding"
                continue
            assert torch.equal(want[0], first.C), f"{name}: {mname} and the unsliced fused call disagree on C"
            assert torch.equal(want[1], first.M), f"{name}: {mname} and the unsliced fused call disagree on the mask"
        us = {m: [] for m in modes}
        launches = {}
        for _ in range(args.repeats):                                            # interleaved repeats
            for mname, fn in modes.items():
                one, launches[mname] = measure(fn)
                us[mname].append(one)
        spread = lambda m: (max(us[m]) - min(us[m])) / min(us[m])
        for mname in modes:
            med = statistics.median(us[mname])
            passes = mname.replace("_fused", "_then_passes") if mname != "unsliced_fused" and mname.endswith("_fused") else None
            rec = dict(workload=name, epilogue="bias+relu+bitmask" if mask else "bias+relu", mode=mname, blocks=nblocks, products=int(counts.sum()), operand_sets=nsets,
                       algorithmic_bytes=first.bytes, launches_per_step=launches[mname], us_per_step=round(med, 3), us_medians=[round(x, 3) for x in us[mname]],
                       spread=round(spread(mname), 4), vs_unsliced_fused=round(med / statistics.median(us["unsliced_fused"]), 4),
                       vs_sliced_then_passes=round(med / statistics.median(us[passes]), 4) if passes else None, steps=args.steps, **info[mname])
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del sets, first, keep, modes
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
