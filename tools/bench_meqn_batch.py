#!/usr/bin/env python
"""One strided batch of a matrix equation (libxsmm_hip_meqn_batch_strided) against the caller's loop of `count` stream-ordered single calls on the
same stepped pointers.  Device events around each form, warm-up first, outputs compared after the timed region (bit for bit; the chain-only
tree within 1e-6).  Algorithmic bytes: every input once (a shared operand once for the whole batch), every output, every DUMP image.

  python tools/bench_meqn_batch.py [--out profiles/r08_meqn_batch.jsonl] [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from libxsmm_amd import capi  # noqa: E402
from libxsmm_amd.capi import BINARY, BINARY_FLAG, DT, UNARY, UNARY_FLAG  # noqa: E402
import test_meqn as tm  # noqa: E402

ll = C.c_longlong
ES = {DT.F32: 4, DT.BF16: 2}
TDT = {DT.F32: torch.float32, DT.BF16: torch.bfloat16}


def softmax_eqn(api, m, n, dt):
    """samples/equation/equation_softmax.c's forward tree: argument 0 is the scratch the DUMP node (op argument 31) writes."""
    idx = api.meqn_create()
    OP, DUMP_AT = capi.MeqnMetadata(idx, -1), capi.MeqnMetadata(idx, 31)
    rows, cols = UNARY_FLAG.REDUCE_ROWS, UNARY_FLAG.REDUCE_COLS
    api.meqn_push_back_binary_op(OP, BINARY.MUL, DT.F32, BINARY_FLAG.BCAST_SCALAR_IN_1)
    api.meqn_push_back_arg(capi.MeqnMetadata(idx, 0), capi.MeqnArgShape(m, n, m, DT.F32), tm.SINGULAR)
    api.meqn_push_back_unary_op(OP, UNARY.RECIPROCAL, DT.F32, 0)
    api.meqn_push_back_unary_op(OP, UNARY.REDUCE_X_OP_ADD, DT.F32, rows)
    api.meqn_push_back_unary_op(OP, UNARY.REDUCE_X_OP_ADD, DT.F32, cols)
    api.meqn_push_back_unary_op(DUMP_AT, UNARY.DUMP, DT.F32, 0)
    api.meqn_push_back_unary_op(OP, UNARY.EXP, DT.F32, 0)
    api.meqn_push_back_binary_op(OP, BINARY.SUB, DT.F32, BINARY_FLAG.BCAST_SCALAR_IN_1)
    api.meqn_push_back_arg(capi.MeqnMetadata(idx, 1), capi.MeqnArgShape(m, n, m, dt), tm.SINGULAR)
    api.meqn_push_back_unary_op(OP, UNARY.REDUCE_X_OP_MAX, DT.F32, rows)
    api.meqn_push_back_unary_op(OP, UNARY.REDUCE_X_OP_MAX, DT.F32, cols)
    api.meqn_push_back_arg(capi.MeqnMetadata(idx, 1), capi.MeqnArgShape(m, n, m, dt), tm.SINGULAR)
    return api.dispatch_meqn(idx, capi.MeqnArgShape(m, n, m, dt))


class Workload:
    """inputs: list of (torch tensor, byte stride, element bytes); dumps: {op position: (tensor, stride, bytes)}; out: (tensor, stride, bytes)."""

    def __init__(self, name, h, inputs, out, dumps=None, dump_aliases=None, tol=0.0):
        self.name, self.h, self.inputs, self.out, self.dumps, self.tol = name, h, inputs, out, dumps or {}, tol
        self.dump_aliases = dump_aliases or {}       # input position -> op position whose DUMP image it reads back (same buffer, same stride)

    def count(self):
        return self.out[0].numel() * self.out[0].element_size() // self.out[1]

    def alg_bytes(self):
        n = self.count()
        b = sum(nb * (n if s else 1) for k, (t, s, nb) in enumerate(self.inputs) if k not in self.dump_aliases)
        return b + self.out[2] * n + sum(nb * n for (_, _, nb) in self.dumps.values())

    def param(self, i, out_t, dump_t):
        """single call i (i = None: the batch's element-0 param) into out_t / dump_t (the result buffers of this form)"""
        k = 0 if i is None else i
        ptrs = []
        for pos, (t, s, _) in enumerate(self.inputs):
            base = dump_t[self.dump_aliases[pos]].data_ptr() if pos in self.dump_aliases else t.data_ptr()
            ptrs.append(base + k * s)
        inputs = (capi.MatrixArg * len(ptrs))()
        for pos, v in enumerate(ptrs):
            inputs[pos].primary = v
        ops = (capi.MatrixOpArg * 32)()
        for pos, (_, s, _) in self.dumps.items():
            ops[pos].primary = dump_t[pos].data_ptr() + k * s
        p = capi.MeqnParam()
        p.inputs, p.ops_args = inputs, ops
        p.output.primary = out_t.data_ptr() + k * self.out[1]
        p._keep = (inputs, ops)
        return p


def run(api, w, reps):
    n = w.count()
    outs = [torch.zeros_like(w.out[0]) for _ in range(2)]
    dumps = [{pos: torch.zeros_like(t) for pos, (t, _, _) in w.dumps.items()} for _ in range(2)]
    singles = [w.param(i, outs[0], dumps[0]) for i in range(n)]
    bp = w.param(None, outs[1], dumps[1])
    sin = (ll * len(w.inputs))(*[s for (_, s, _) in w.inputs])
    sops = (ll * 32)(*[w.dumps[p][1] if p in w.dumps else 0 for p in range(32)])
    call = capi.Api.call

    def loop():
        for p in singles:
            call(w.h, p)

    def batch():
        api.hip_meqn_batch_strided(w.h, C.byref(bp), n, len(w.inputs), sin, w.out[1], 0, 32, sops)

    def timed(fn):
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts))
    loop(); batch(); torch.cuda.synchronize(); api.check()     # warm-up (the batched kernel is generated at the first batched call)
    t_loop, t_batch = timed(loop), timed(batch)
    torch.cuda.synchronize(); api.check()
    if w.tol == 0.0:
        same = torch.equal(outs[0].view(torch.int8), outs[1].view(torch.int8)) and all(torch.equal(dumps[0][p], dumps[1][p]) for p in dumps[0])
    else:
        a, b = outs[0].double(), outs[1].double()
        same = bool(((a - b).norm() / a.norm()).item() <= w.tol)
    alg = w.alg_bytes()
    rec = {"workload": w.name, "count": n, "kernel_single": api.hip_kernel_name(w.h, 0).decode(), "kernel_batched": api.hip_kernel_name(w.h, 1).decode(),
           "loop_us": round(t_loop, 1), "batch_us": round(t_batch, 2), "speedup": round(t_loop / t_batch, 1), "algorithmic_bytes": alg,
           "batch_frac_8TBs": round(alg / (t_batch * 1e-6) / 8e12, 3), "loop_frac_8TBs": round(alg / (t_loop * 1e-6) / 8e12, 3), "outputs_equal": same}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    api = capi.load()
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)       # stream-ordered singles and batches on torch's stream
    api.hip_set_jit(2)
    g = torch.Generator(device="cuda").manual_seed(8)
    rnd = lambda n, dt=DT.F32: (torch.rand(n, device="cuda", generator=g) * 4 - 2).to(TDT[dt])     # noqa: E731
    works = []
    for dt in (DT.F32, DT.BF16):                  # softmax forward, 64 x 64, 4096 elements: three phases, scalar reductions, the DUMP image read back
        m = n = 64; count = 4096
        x = rnd(m * n * count, dt)
        kept = torch.zeros(m * n * count, device="cuda")
        out = torch.zeros(m * n * count, dtype=TDT[dt], device="cuda")
        works.append(Workload(f"softmax fwd (equation_softmax.c) {m}x{n} {'f32' if dt == DT.F32 else 'bf16'}", softmax_eqn(api, m, n, dt),
                              [(kept, m * n * 4, m * n * 4), (x, m * n * ES[dt], m * n * ES[dt])], (out, m * n * ES[dt], m * n * ES[dt]),
                              dumps={31: (kept, m * n * 4, m * n * 4)}, dump_aliases={0: 31}))
    # layernorm affine forward (equation_simple_layernorm.c): per-element x, s, b; gamma / beta shared
    m = n = 64; count = 4096
    tree = tm.CASES["layernorm_affine"][0]
    shapes = [(m, n, m, DT.BF16), (1, 1, 1, DT.F32), (1, 1, 1, DT.F32), (m, n, m, DT.BF16), (m, n, m, DT.BF16)]
    h = api.dispatch_meqn(tm.build(api, tree, shapes), capi.MeqnArgShape(m, n, m, DT.BF16))
    x, s, b = rnd(m * n * count, DT.BF16), rnd(4 * count), rnd(4 * count)
    gam, bet = rnd(m * n, DT.BF16), rnd(m * n, DT.BF16)
    works.append(Workload(f"layernorm affine fwd {m}x{n} bf16", h, [(x, m * n * 2, m * n * 2), (s, 16, 4), (b, 16, 4), (gam, 0, m * n * 2), (bet, 0, m * n * 2)],
                          (torch.zeros(m * n * count, dtype=torch.bfloat16, device="cuda"), m * n * 2, m * n * 2)))
    # column sums broadcast back (test_meqn.py's reduce_bcast): a phase with a vector reduction
    m, n, count = 64, 128, 2048
    h = api.dispatch_meqn(tm.build(api, tm.CASES["reduce_bcast"][0], [(m, n, m, DT.F32)]), capi.MeqnArgShape(m, n, m, DT.F32))
    works.append(Workload(f"x * colsum(x^2) {m}x{n} f32", h, [(rnd(m * n * count), m * n * 4, m * n * 4)],
                          (torch.zeros(m * n * count, device="cuda"), m * n * 4, m * n * 4)))
    # a chain-only tree: the column sums of x * y (a reduction head has no fused form), 256 x 256
    m, n, count = 256, 256, 256
    tree = ("u", UNARY.REDUCE_X_OP_ADD, UNARY_FLAG.REDUCE_COLS, ("b", BINARY.MUL, 0, ("arg", 0), ("arg", 1)))
    h = api.dispatch_meqn(tm.build(api, tree, [(m, n, m, DT.F32)] * 2), capi.MeqnArgShape(m, 1, m, DT.F32))
    works.append(Workload(f"colsum(x * y) {m}x{n} f32 (chain)", h, [(rnd(m * n * count), m * n * 4, m * n * 4), (rnd(m * n * count), m * n * 4, m * n * 4)],
                          (torch.zeros(m * count, device="cuda"), m * 4, m * 4), tol=1e-6))
    api.hip_set_jit(1)
    recs = [run(api, w, args.reps) for w in works]
    if args.out:
        with open(args.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
    api.hip_sync()
    api.hip_set_stream(None)
    api.hip_set_async(0)


if __name__ == "__main__":
    main()
