"""Writes tests/golden/mx_quant_reference.npz: the reference's QUANT TPP outputs (MXFP4 / MXBF8 / NVFP4) for the CPU cases of
tests/test_mx_quant.py, so that those tests run where oracle/_ref could not be built.  Needs oracle/_ref/libxsmm_ref.so:
    python tests/golden/make_mx_quant_golden.py"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from libxsmm_amd import capi  # noqa: E402
from libxsmm_amd.capi import DT, UNARY  # noqa: E402
from oracle import pyoracle  # noqa: E402
import test_mx_quant as t  # noqa: E402


def run(bits, shape, data, scales):
    p = capi.UnaryParam()
    p.in_.primary, p.out.primary, p.out.secondary = bits.ctypes.data, data.ctypes.data, scales.ctypes.data
    return pyoracle.reference().lib.xref_reference_meltw_unary(C.byref(p), UNARY.QUANT, shape, 0)


def main():
    pyoracle.build()
    assert pyoracle.have_reference(), "needs oracle/_ref/libxsmm_ref.so"
    out = {}
    for m, n, ldi, ldo, fp4 in t.CASES:
        bits, _ = t._inputs(m, n, ldi, 7, specials=n >= 7)
        data, scales = np.zeros(n * (ldo // 2 if fp4 else ldo), np.uint8), np.zeros(n * (ldo // 32), np.uint8)
        key = f"mx_{m}_{n}_{ldi}_{ldo}_{int(fp4)}"
        out[key + "_rc"] = np.int32(run(bits, capi.UnaryShape(m, n, ldi, ldo, DT.BF16, DT.MXFP4X2 if fp4 else DT.MXBF8, DT.BF16), data, scales))
        out[key + "_data"], out[key + "_scales"] = data, scales
    for m, n, ldi, ldo in t.NV_CASES:
        bits, _ = t._inputs(m, n, ldi, 7, specials=n >= 7)
        data, scales = np.zeros(n * (ldo // 2), np.uint8), np.zeros(n * (ldo // 16), np.uint8)
        key = f"nv_{m}_{n}_{ldi}_{ldo}"
        out[key + "_rc"] = np.int32(run(bits, capi.UnaryShape(m, n, ldi, ldo, DT.BF16, DT.NVFP4X2, DT.BF16), data, scales))
        out[key + "_data"], out[key + "_scales"] = data, scales
    np.savez_compressed(t.GOLDEN, **out)
    print(t.GOLDEN, os.path.getsize(t.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
