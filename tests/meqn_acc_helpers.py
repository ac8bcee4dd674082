"""Trees, operand layouts and numpy restatements for accumulating batches of matrix equations (libxsmm_hip_meqn_batch_strided_accumulate).

A case is (tree, input shapes, output shape, carried position): the carried position is the input that IS the output.  The layouts come from
meqn_batch_helpers.Batch (padded strides, shared positions); 1 x 1 inputs become arrays of one value per element with stride 4, as the caller's
`a = var[s2]`, `b = -a * mean[s2]` of a layernorm backward pass."""
import numpy as np

from helpers import rand_values
from libxsmm_amd.capi import BINARY, DT, TERNARY, TERNARY_FLAG
from meqn_batch_helpers import ESIZE, NPDT, Batch

A = lambda i: ("arg", i)   # noqa: E731


def dgamma(in_dt, m, n, ld):
    """equation_layernorm.c: dgamma += (a * inp + b) * dout; inputs 0 inp, 1 a, 2 b, 3 dout, 4 dgamma."""
    tree = ("t", TERNARY.MULADD, TERNARY_FLAG.REUSE_IN_2_AS_OUT,
            ("t", TERNARY.MULADD, TERNARY_FLAG.BCAST_SCALAR_IN_1 | TERNARY_FLAG.BCAST_SCALAR_IN_2 | TERNARY_FLAG.REUSE_IN_2_AS_OUT, A(0), A(1), A(2)), A(3), A(4))
    return tree, [(m, n, ld, in_dt), (1, 1, 1, DT.F32), (1, 1, 1, DT.F32), (m, n, ld, in_dt), (m, n, ld, DT.F32)], (m, n, ld, DT.F32), 4


def dbeta(in_dt, m, n, ld, acc_dt=DT.F32):
    """equation_layernorm.c: dbeta += dout; the tree reads input positions 3 (dout) and 5 (dbeta) of the six the caller passes."""
    pad = (8, 1, 8, DT.F32)
    return ("b", BINARY.ADD, 0, A(3), A(5)), [pad, pad, pad, (m, n, ld, in_dt), pad, (m, n, ld, acc_dt)], (m, n, ld, acc_dt), 5


def running_max(m, n, ld):
    """out = max(out, x): not a sum -- only the loop's own order of operations computes it."""
    return ("b", BINARY.MAX, 0, A(0), A(1)), [(m, n, ld, DT.F32), (m, n, ld, DT.F32)], (m, n, ld, DT.F32), 0


CASES = {
    "dgamma_f32": dgamma(DT.F32, 64, 64, 64),
    "dgamma_bf16_in": dgamma(DT.BF16, 64, 64, 64),
    "dgamma_f32_ld48": dgamma(DT.F32, 40, 24, 48),
    "dbeta_f32": dbeta(DT.F32, 40, 24, 48),
    "dbeta_f32_64": dbeta(DT.F32, 64, 64, 64),
    "dbeta_bf16_acc": dbeta(DT.BF16, 64, 32, 64, DT.BF16),      # a BF16 accumulator: rounded after every element
    "running_max": running_max(40, 24, 48),
}
SLICEABLE = ("dgamma_f32", "dgamma_bf16_in", "dgamma_f32_ld48", "dbeta_f32", "dbeta_f32_64")


def slices_rule(count, m, n):
    """The library's rule for the number of slices of the sliced form (csrc/meqn.cpp): from 128 elements on, a slice holds at
    least 16 elements, the grid stays at or below 256 workgroups; fewer than 2 slices: the carried form (0)."""
    blocks = (m // 8 * n + 255) // 256
    s = min(count // 16, max(1, 256 // blocks))
    return s if count >= 128 and s >= 2 else 0


def leaf_order(tree, skip=()):
    """Input positions in the order the generated kernels take them: first visit, operands left to right."""
    order = []

    def walk(t):
        if t[0] == "arg":
            if t[1] not in order and t[1] not in skip:
                order.append(t[1])
        else:
            for c in t[3:]:
                walk(c)
    walk(tree)
    return order


class AccBatch(Batch):
    """Batch whose carried position is shared (it is the output) and whose 1 x 1 positions are arrays with stride 4."""

    def __init__(self, case, count, shared=(), seed=0):
        tree, shapes, out_shape, carried = case
        super().__init__(shapes, out_shape, count, shared=tuple(shared) + (carried,), seed=seed)
        rng = np.random.default_rng(seed + 1000)
        self.tree, self.carried = tree, carried
        for k, (m, n, ld, dt) in enumerate(shapes):
            if m == 1 and n == 1 and k not in shared:
                self.inputs[k] = rand_values(rng, count + 1, dt)      # (+1: a host-resident scalar is staged 8 bytes at a time)
                self.strides[k] = ESIZE[dt]
        self.acc0 = self.inputs[carried].copy()                        # the output's value before the first element

    def f32(self, k, i):
        """Element i of input k as an (n, ld) float32 array."""
        m, n, ld, dt = self.shapes[k]
        x = self.element(k, i)
        if dt == DT.BF16:
            x = (x.astype(np.uint32) << 16).view(np.float32)
        return x.reshape(n, ld)


def addend(b, name, i):
    """g(element i) of a SLICEABLE case with the kernel's own roundings: every product and sum rounded to f32, nothing contracted."""
    if name.startswith("dgamma"):
        prod = b.f32(0, i) * b.f32(1, i)[0, 0]
        v = b.f32(2, i)[0, 0] + prod
        return (v * b.f32(3, i)).astype(np.float32)
    return b.f32(3, i)


def sliced_restatement(b, name, slices):
    """The documented order of the sliced form: slice s sums its elements [s * count / S, (s + 1) * count / S) in ascending order starting from +0,
    the partial sums are added in ascending slice order, the output's original value is added last.  Returns the (n, ld) float32 output."""
    m, n, ld, _ = b.out_shape
    total = None
    for s in range(slices):
        part = np.zeros((n, ld), dtype=np.float32)
        for i in range(s * b.count // slices, (s + 1) * b.count // slices):
            part = part + addend(b, name, i)
        total = part if total is None else total + part
    out = b.acc0.reshape(n, ld).copy()
    out[:, :m] = (out + total)[:, :m]
    return out


def gold_f64(b, name):
    """The same addends summed in float64, plus the output's original value."""
    m, n, ld, _ = b.out_shape
    total = np.zeros((n, ld), dtype=np.float64)
    for i in range(b.count):
        total += addend(b, name, i).astype(np.float64)
    return (b.acc0.reshape(n, ld).astype(np.float64) + total)[:, :m]


__all__ = ["A", "AccBatch", "CASES", "SLICEABLE", "NPDT", "addend", "gold_f64", "leaf_order", "sliced_restatement", "slices_rule"]
