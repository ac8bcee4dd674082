"""The reference's own reduction driver (samples/eltwise/eltwise_unary_reduce.c, built by oracle/Makefile into oracle/_ref/drivers) in F64: it
generates its data with libxsmm_rng, allocates with plain malloc (synchronous calls stage host operands), dispatches through the public API
and checks against its f64 gold (reference_reduce_kernel_f64).  A driver is its own judge: exit code 0 and no failure marker in its output."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
DRV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "_ref", "drivers")
FAIL_MARKERS = ("FAILED", "ERROR", "JIT failed", "failed. Bailing", "not supported")


def check(binary, *args, timeout=120):
    exe = os.path.join(DRV, binary)
    if not os.path.exists(exe):
        pytest.skip(f"{exe} not built (make -C oracle drivers needs the reference sources)")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, LIBXSMM_VERBOSE="0"))
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"{binary} {args}: exit {r.returncode}\n{out[-2000:]}"
    bad = [m for m in FAIL_MARKERS if m in out]
    assert not bad, f"{binary} {args}: {bad}\n{out[-2000:]}"
    return out


# M N ldi reduce_x reduce_x2 reduce_rows op(0 add, 1 max, 2 min) dtype n_cols_idx idx_type(0: 8-byte, 1: 4-byte) record_idx reduce_on_outputs iters
# No listed-column lines (n_cols_idx > 0): in F64 the driver hands its kernel the low-precision buffers and compares the f64 result buffer the kernel
# never writes (eltwise_unary_reduce.c:467-475, :769), so it cannot pass against any implementation; tests/test_meltw_f64_reduce_gpu.py pins the
# listed f64 forms against the reference's loop instead.
@pytest.mark.parametrize("args", ["64 48 64 1 0 1 0 F64 0 0 0 0 1", "64 48 64 1 1 0 0 F64 0 0 0 0 1", "33 17 40 1 0 0 1 F64 0 0 0 0 1",
                                  "64 48 64 1 1 1 0 F64 0 0 0 1 1", "64 48 64 0 1 1 0 F64 0 0 0 0 1", "64 48 64 1 0 1 1 F64 0 0 0 0 1",
                                  "64 48 64 1 0 1 2 F64 0 0 0 0 1", "64 48 64 1 0 0 2 F64 0 0 0 0 1", "64 48 64 1 0 0 1 F64 0 0 1 0 1",
                                  "64 48 64 1 0 0 2 F64 0 1 1 0 1", "33 17 40 1 1 0 0 F64 0 0 0 1 1"])
def test_reference_reduce_driver_f64(args):
    check("eltwise_unary_reduce", *args.split())
