"""Operand layouts for strided batches of matrix equations (libxsmm_hip_meqn_batch_strided): one buffer per input position holding `count` elements
`stride` bytes apart (stride 0: one element shared by all), and an output buffer with a stride of its own.  Strides are multiples of 16 bytes and larger
than the element's footprint, so that a kernel stepping by the footprint instead of the stride reads the wrong bytes."""
import numpy as np

from helpers import rand_values
from libxsmm_amd.capi import DT

NPDT = {DT.F32: np.float32, DT.BF16: np.uint16}
ESIZE = {DT.F32: 4, DT.BF16: 2}


def round16(x):
    return (x + 15) // 16 * 16


class Batch:
    """inputs[k]: flat host buffer of input position k; strides[k]: its byte stride; element(k, i): element i's array (a copy)."""

    def __init__(self, shapes, out_shape, count, shared=(), seed=0):
        rng = np.random.default_rng(seed)
        self.shapes, self.out_shape, self.count = shapes, out_shape, count
        self.inputs, self.strides = [], []
        for k, (m, n, ld, dt) in enumerate(shapes):
            foot = ld * n * ESIZE[dt]
            stride = 0 if k in shared else round16(foot + 16 * (k + 1))
            total = ((count - 1) * stride + foot) // ESIZE[dt]
            self.inputs.append(rand_values(rng, total, dt))
            self.strides.append(stride)
        m, n, ld, dt = out_shape
        self.out_foot = ld * n * ESIZE[dt]
        self.out_stride = round16(self.out_foot + 32)
        self.out_elems = ((count - 1) * self.out_stride + self.out_foot) // ESIZE[dt]

    def element(self, k, i):
        m, n, ld, dt = self.shapes[k]
        off = i * self.strides[k] // ESIZE[dt]
        return self.inputs[k][off:off + ld * n].copy()

    def out_element(self, out, i):
        dt = self.out_shape[3]
        off = i * self.out_stride // ESIZE[dt]
        return out[off:off + self.out_foot // ESIZE[dt]]

    def new_out(self):
        return np.zeros(self.out_elems, dtype=NPDT[self.out_shape[3]])
