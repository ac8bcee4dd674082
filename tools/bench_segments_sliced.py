"""Sliced segments (libxsmm_hip_gemm_batch_reduce_segments_sliced / ..._offsets_sliced) against the unsliced entry on the same lists.

Workloads (f32 32^3 unless said otherwise):
  dw_f32_nt            the weight gradient of a block-sparse layer: 256 stored blocks of a 32 x 32 block grid, 256 products each (dW_b = sum_p dY(r, p) X(c, p)^T,
                       OFFSET, TRANS_B; the blocks of a block row share their dY blocks, those of a block column their X blocks); every chain cut into slices of
                       4, 8, 16 and 32 products
  skew_f32_nn          8192 segments, 1 % of them 64 products, the rest 2, in list order (ADDRESS); only the long chains are cut, into 8 slices
  skew_f32_tn_sorted   the same counts, longest first, A transposed (OFFSET); only the long chains are cut, into 8 slices
  skew_bf16_nt_sorted  bf16 VNNI-A 64^3 -> bf16, the same counts, longest first, B transposed (OFFSET); only the long chains are cut, into 8 slices
  uniform4_f32_nn      8192 blocks of 4 products, one slice per block (ADDRESS): the sliced call does the same work plus its second pass -- the pure overhead
The method is that of tools/bench_segments_offsets.py: the operands are allocated as several sets, together more than twice the 256 MiB Infinity Cache, and a step
takes the next set; the lists (and, sliced, the ONE workspace a caller would reuse) are shared by the sets; a step is timed with device events on torch's stream;
the median over --steps warm steps is reported; every mode is measured --repeats times, interleaved, and the spread of the unsliced medians (max - min) / min is
what a difference has to exceed.  All modes of a workload are compared bit for bit (exact small-integer data) before anything is timed.  --lib measures another
build of the library (the parent commit's, which has the unsliced entries only: --modes unsliced) in the same session; --build names it in the records.

  python tools/bench_segments_sliced.py --steps 200 --warmup 20 --out profiles/r16_segments_sliced.jsonl
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

LLC = 256 << 20
FORMS = {None: 0, "NN": 0, "TN": GEMM_FLAG.TRANS_A, "NT": GEMM_FLAG.TRANS_B}
F32 = dict(t=DT.F32, c=DT.F32, e=32, vnni=0, torch=torch.float32)
BF16 = dict(t=DT.BF16, c=DT.BF16, e=64, vnni=GEMM_FLAG.VNNI_A, torch=torch.bfloat16)


class OlderApi(capi.Api):
    """A build of the library that lacks some of the mirrored entries (the parent commit's): binds what it has."""

    def _f(self, name, restype, argtypes):
        return super()._f(name, restype, argtypes) if hasattr(self.lib, self.prefix + name) else None


def csr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def skewed(rng, nseg=8192):
    return np.where(rng.random(nseg) < 0.01, 64, 2).astype(np.int64)


def own_blocks(counts):
    """Every product has an A and a B block of its own."""
    total = int(counts.sum())
    return np.arange(total, dtype=np.int64), np.arange(total, dtype=np.int64), total, total


def workloads():
    rng = np.random.default_rng(16)
    w = {}
    # dW: a 32 x 32 block grid, 256 blocks stored (8 per block row), 256 block columns of the minibatch
    grid, pb = 32, 256
    rows = np.repeat(np.arange(grid), 8)
    cols = np.concatenate([(r * 5 + np.arange(8) * 4) % grid for r in range(grid)])
    a_idx = (rows[:, None] * pb + np.arange(pb)[None, :]).ravel()                # dY(r, p)
    b_idx = (cols[:, None] * pb + np.arange(pb)[None, :]).ravel()                # X(c, p)
    counts = np.full(len(rows), pb, dtype=np.int64)
    w["dw_f32_nt"] = dict(kind=F32, form="NT", counts=counts, ops=(a_idx, b_idx, grid * pb, grid * pb), cuts={f"slices_of_{n}": ("length", n) for n in (4, 8, 16, 32)})
    c = skewed(rng)
    w["skew_f32_nn"] = dict(kind=F32, form=None, counts=c, ops=own_blocks(c), cuts={"long_into_8": ("long", 8)})
    c = np.sort(skewed(rng))[::-1].copy()
    w["skew_f32_tn_sorted"] = dict(kind=F32, form="TN", counts=c, ops=own_blocks(c), cuts={"long_into_8": ("long", 8)})
    w["skew_bf16_nt_sorted"] = dict(kind=BF16, form="NT", counts=c, ops=own_blocks(c), cuts={"long_into_8": ("long", 8)})
    c = np.full(8192, 4, dtype=np.int64)
    w["uniform4_f32_nn"] = dict(kind=F32, form=None, counts=c, ops=own_blocks(c), cuts={"one_slice_per_block": ("length", 4)})
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
        self.blk, self.esz = kind["e"] * kind["e"], capi.DT_SIZE[kind["t"]]
        a_idx, b_idx, na, nb = wl["ops"]
        nblocks = len(wl["counts"])
        mk = lambda n: torch.randint(-1, 2, (n * self.blk,), device="cuda", dtype=torch.int32).to(kind["torch"])
        self.A, self.B = mk(na), mk(nb)
        self.C = torch.zeros(nblocks * self.blk, device="cuda", dtype=kind["torch"])
        self.bytes = (na + nb + nblocks) * self.blk * self.esz                   # every block of the operands once, C once (beta = 0)
        if wl["form"] is None:                                                   # ADDRESS: the pointer lists of this set
            dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to("cuda")
            step = self.blk * self.esz
            self.la, self.lb = dev(self.A.data_ptr() + a_idx * step), dev(self.B.data_ptr() + b_idx * step)
            self.lc = dev(self.C.data_ptr() + np.arange(nblocks, dtype=np.int64) * step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_segments_sliced.jsonl"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--workloads", default="")
    ap.add_argument("--modes", default="all", choices=("all", "unsliced"))
    ap.add_argument("--lib", default="", help="another build of the library (e.g. the parent commit's, with --modes unsliced)")
    ap.add_argument("--build", default="this", help="the name of the measured build in the records")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_segments_sliced.py needs a GPU: nothing is measured without one")
    api = OlderApi(args.lib, "libxsmm_") if args.lib else capi.load()
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    api.hip_set_async(1)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to("cuda")
    lines = []
    todo = workloads()
    for name in (args.workloads.split(",") if args.workloads else list(todo)):
        wl = todo[name]
        kind, form, counts = wl["kind"], wl["form"], wl["counts"]
        e, t = kind["e"], kind["t"]
        nblocks = len(counts)
        shape = capi.gemm_shape(e, e, e, e, e, e, t, t, kind["c"], DT.F32)
        br = capi.br_config(capi.BR_ADDRESS if form is None else capi.BR_OFFSET, 0, 0, 0)
        h = api.dispatch_brgemm(shape, kind["vnni"] | FORMS[form] | GEMM_FLAG.BETA_0, 0, br)
        assert h, name
        first = OperandSet(wl)
        nsets = max(2, -(-2 * LLC // first.bytes) + 1)
        sets = [first] + [OperandSet(wl) for _ in range(nsets - 1)]
        step_b = first.blk * first.esz
        seg_unsliced = dev(csr(counts))
        if form is not None:                                                     # OFFSET: one set of lists for every operand set
            o_a, o_b, o_c = dev(wl["ops"][0] * step_b), dev(wl["ops"][1] * step_b), dev(np.arange(nblocks, dtype=np.int64) * step_b)

        def lists(s):
            return (s.la, s.lb, s.lc) if form is None else (o_a, o_b, o_c)

        def param(s):
            p = capi.GemmParam()
            if form is not None:
                p.a.primary, p.b.primary, p.c.primary = s.A.data_ptr(), s.B.data_ptr(), s.C.data_ptr()
            return p

        def unsliced(s):
            fn = api.hip_gemm_batch_reduce_segments if form is None else api.hip_gemm_batch_reduce_segments_offsets
            fn(h, C.byref(param(s)), nblocks, seg_unsliced.data_ptr(), *[x.data_ptr() for x in lists(s)])

        modes = {"unsliced": unsliced}
        info = {"unsliced": dict(slices=nblocks, workspace_bytes=0)}
        keep = []
        if args.modes == "all":
            for cname, how in wl["cuts"].items():
                blk_ptr, seg_ptr = cut(counts, how)
                nslices = len(seg_ptr) - 1
                nbytes = api.hip_gemm_batch_reduce_segments_sliced_workspace(h, nslices)
                ws = torch.empty(max(nbytes, 16), device="cuda", dtype=torch.uint8)
                d_blk, d_seg = dev(blk_ptr), dev(seg_ptr)
                keep += [ws, d_blk, d_seg]

                def sliced(s, d_blk=d_blk, d_seg=d_seg, ws=ws, nslices=nslices, nbytes=nbytes):
                    fn = api.hip_gemm_batch_reduce_segments_sliced if form is None else api.hip_gemm_batch_reduce_segments_offsets_sliced
                    la, lb, lc = lists(s)
                    fn(h, C.byref(param(s)), nblocks, d_blk.data_ptr(), nslices, d_seg.data_ptr(), la.data_ptr(), lb.data_ptr(), lc.data_ptr(), ws.data_ptr(), nbytes)

                modes[cname] = sliced
                info[cname] = dict(slices=nslices, workspace_bytes=int(nbytes))

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

        # every mode gives the same C (exact small-integer data): checked once per workload before anything is timed
        want, kernels = None, {}
        for mname, fn in modes.items():
            first.C.fill_(0.5)                                                  # no sum of integers
            fn(first); torch.cuda.synchronize(); api.check()
            kernels[mname] = api.hip_kernel_name(h, 1).decode()
            if want is None:
                want = first.C.clone()
                assert (want != 0.5).all()
            assert torch.equal(want, first.C), f"{name}: {mname} and the unsliced call disagree"
        us = {m: [] for m in modes}
        launches = {}
        for _ in range(args.repeats):                                            # interleaved repeats
            for mname, fn in modes.items():
                one, launches[mname] = measure(fn)
                us[mname].append(one)
        spread = (max(us["unsliced"]) - min(us["unsliced"])) / min(us["unsliced"])
        for mname in modes:
            med = statistics.median(us[mname])
            rec = dict(workload=name, build=args.build, mode=mname, blocks=nblocks, products=int(counts.sum()), operand_sets=nsets, algorithmic_bytes=first.bytes,
                       kernel=kernels[mname], launches_per_step=launches[mname], us_per_step=round(med, 3), us_medians=[round(x, 3) for x in us[mname]],
                       unsliced_spread=round(spread, 4), vs_unsliced=round(med / statistics.median(us["unsliced"]), 4), steps=args.steps, **info[mname])
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del sets, first, keep, modes
        torch.cuda.empty_cache()
    api.hip_sync()
    api.hip_set_async(0)
    api.hip_set_stream(None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
