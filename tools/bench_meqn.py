#!/usr/bin/env python
"""Fused (one generated kernel) vs chained (one TPP launch per node) evaluation of the equation of
samples/equation/equation_simple.c:516-538, (a0 + inc(a1)) * (x2(a2) + a3), on an m x n f32 problem.
Algorithmic bytes = 4 inputs + 1 output, each m*n*4 (what a perfectly fused kernel moves).
--bf16: the bias_relu_bf16 and layernorm_affine trees of tests/test_meqn.py on bf16 operands instead."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import bench  # noqa: E402
from libxsmm_amd import capi  # noqa: E402
from libxsmm_amd.capi import BINARY, DT, UNARY  # noqa: E402
import test_meqn as tm  # noqa: E402


def workloads(variant, m, n):
    """(label, tree, argument shapes, output shape, algorithmic bytes, flops per element) -- f32: equation_simple.c's five-node tree; bf16: the two bf16 trees
    of tests/test_meqn.py, whose generated loads flush bf16 denormals as the TPP kernels do (DESIGN.md section 7 (f1) holds the cost of that flush)."""
    if variant == "f32":
        return [("(a0 + inc(a1)) * (x2(a2) + a3)", tm.CASES["simple"][0], [(m, n, m, DT.F32)] * 4, (m, n, m, DT.F32), 5 * m * n * 4, 4.0)]
    full = (m, n, m, DT.BF16)
    one = (1, 1, 1, DT.F32)
    return [("bias_relu_bf16: relu(bias + x)", tm.CASES["bias_relu_bf16"][0], [(m, 1, m, DT.BF16), full], full, 2 * m * n * 2 + m * 2, 2.0),
            ("layernorm_affine: (x * s + b) * gamma + beta", tm.CASES["layernorm_affine"][0], [full, one, one, full, full], full, 4 * m * n * 2, 4.0)]


def main():
    m, n = 4096, 4096
    variant = "bf16" if "--bf16" in sys.argv[1:] else "f32"
    torch.cuda.set_device(0)
    api = capi.load()
    api.hip_set_stream(torch.cuda.current_stream().cuda_stream)
    nsets = 3
    for text, tree, shapes, out_shape, alg, flops in workloads(variant, m, n):
        def operand(shape):
            x = torch.rand(shape[2] * shape[1] + 1, device="cuda") - 0.5           # (+1: a 1 x 1 operand is read as 8 bytes when it is staged)
            return x if shape[3] == DT.F32 else x.to(torch.bfloat16)
        ins = [[operand(s) for s in shapes] for _ in range(nsets)]
        out = operand(out_shape)
        for mode, label in ((0, "tpp_chain"), (2, "fused_jit")):
            api.hip_set_jit(mode)
            idx = tm.build(api, tree, shapes)
            h = api.dispatch_meqn(idx, capi.MeqnArgShape(*out_shape))
            params = []
            for s in range(nsets):
                arr = (capi.MatrixArg * len(shapes))()
                for i in range(len(shapes)):
                    arr[i].primary = ins[s][i].data_ptr()
                p = capi.MeqnParam(); p.inputs = arr; p.output.primary = out.data_ptr(); p._keep = arr
                params.append(p)

            class W:
                pass
            w = W(); w.api = api
            w.nsets, w.hint, w.dtype, w.alg_bytes_per_step, w.flops_per_step = nsets, 0, variant, alg, flops * m * n
            w.label = lambda: label; w.kernel = lambda: api.hip_kernel_name(h, 0).decode()
            w.step = lambda i: capi.Api.call(h, params[i % nsets])
            for i in range(3):
                w.step(i)
            torch.cuda.synchronize(); api.check()
            _, _, us = bench.timed(w, 20, 0.15)
            print(json.dumps({"workload": f"meqn {text}, {m}x{n} {variant}", "mode": label, "kernel": api.hip_kernel_name(h, 0).decode(),
                              "us": round(us, 1), "algorithmic_GBs": round(alg / us / 1e3, 1), "frac_hbm_peak": round(alg / us / 1e3 / 8000, 3)}), flush=True)
    api.hip_set_jit(1)


if __name__ == "__main__":
    main()
