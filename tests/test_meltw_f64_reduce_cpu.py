"""Which all-f64 reduction TPPs the dispatcher accepts and which it keeps refusing -- host logic, checked without a GPU through the
dry-run mode (LIBXSMM_HIP_DRYRUN=1: a machine without a device dispatches, handles cannot be called).  The accepted rows are the f64
branch of the reference's reduction loop (src/generator_mateltwise_reference_impl.c, in / out F64, comp F64 or F32); the refused ones are
the f64 TPPs the reference defines nothing for or this library does not offer in f64."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys
sys.path.insert(0, %r)
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, UNARY, UNARY_FLAG as UF, BINARY
api = capi.load()
D = lambda comp=DT.F64, m=64, n=48, ldi=64, ldo=64, i=DT.F64, o=DT.F64: capi.UnaryShape(m, n, ldi, ldo, i, o, comp)
out = {}
def u(name, typ, shape, flags=0): out[name] = bool(api.dispatch_meltw_unary(typ, shape, flags))
R, C, INIT, ARG, I4, I8 = UF.REDUCE_ROWS, UF.REDUCE_COLS, UF.REDUCE_INIT_ACC, UF.REDUCE_RECORD_ARGOP, UF.IDX_SIZE_4BYTES, UF.IDX_SIZE_8BYTES
for tn in ("REDUCE_X_OP_ADD", "REDUCE_X2_OP_ADD", "REDUCE_X_X2_OP_ADD"):
    typ = getattr(UNARY, tn)
    for fn, f in (("rows", R), ("cols", C)):
        u(f"{tn}_{fn}", typ, D(), f)
        u(f"{tn}_{fn}_init_acc", typ, D(), f | INIT)
        u(f"{tn}_{fn}_comp_f32", typ, D(DT.F32), f)
    u(f"{tn}_ragged_cols", typ, D(m=33, n=17, ldi=40, ldo=33), C)
for tn in ("REDUCE_X_OP_MAX", "REDUCE_X_OP_MIN", "REDUCE_X_OP_ABSMAX"):
    typ = getattr(UNARY, tn)
    u(f"{tn}_rows", typ, D(), R)
    u(f"{tn}_cols", typ, D(), C)
    u(f"{tn}_cols_comp_f32", typ, D(DT.F32), C)
    u(f"{tn}_cols_argop_idx4", typ, D(), C | ARG | I4)
    u(f"{tn}_cols_argop_idx8", typ, D(), C | ARG | I8)
    u(f"{tn}_cols_argop_idx8_default", typ, D(), C | ARG)
    u(f"no:{tn}_rows_argop", typ, D(), R | ARG | I4)
for tn in ("REDUCE_COLS_IDX_OP_ADD", "REDUCE_COLS_IDX_OP_MAX", "REDUCE_COLS_IDX_OP_MIN"):
    typ = getattr(UNARY, tn)
    u(f"{tn}_idx4", typ, D(n=0), C | I4)
    u(f"{tn}_idx8", typ, D(n=0), C | I8)
    u(f"{tn}_idx4_argop", typ, D(n=0), C | I4 | ARG)
    u(f"{tn}_idx8_argop", typ, D(n=0), C | I8 | ARG)
# unchanged: what stays refused in f64
out["no:dot_to_scalar_f64"] = bool(api.dispatch_meltw_binary(BINARY.MUL_AND_REDUCE_TO_SCALAR_OP_ADD, capi.BinaryShape(64, 48, 64, 64, 64, DT.F64, DT.F64, DT.F64, DT.F64), 0))
out["no:cmp_gt_f64"] = bool(api.dispatch_meltw_binary(BINARY.CMP_OP_GT, capi.BinaryShape(64, 48, 64, 64, 64, DT.F64, DT.F64, DT.F64, DT.F64), 0))
u("no:relu_f64", UNARY.RELU, D())
u("no:dropout_f64", UNARY.DROPOUT, D(), UF.BITMASK_2BYTEMULT)
u("no:reduce_ncnc_f64", UNARY.REDUCE_X_OP_ADD_NCNC_FORMAT, D())
u("no:reduce_mul_rows_f64", UNARY.REDUCE_X_OP_MUL, D(), R)
u("no:reduce_mul_cols_f64", UNARY.REDUCE_X_OP_MUL, D(), C)
u("no:reduce_f64_in_f32_out", UNARY.REDUCE_X_OP_ADD, D(o=DT.F32), C)
u("no:reduce_f32_in_f64_out", UNARY.REDUCE_X_OP_ADD, D(i=DT.F32), C)
u("no:reduce_f64_comp_bf16", UNARY.REDUCE_X_OP_ADD, D(DT.BF16), C)
u("no:listed_f64_in_f32_out", UNARY.REDUCE_COLS_IDX_OP_ADD, D(n=0, o=DT.F32), C | I4)
# the f32 forms are untouched
u("f32_reduce_cols", UNARY.REDUCE_X_OP_ADD, D(DT.F32, i=DT.F32, o=DT.F32), C)
u("f32_reduce_rows_argop_refused_as_before", UNARY.REDUCE_X_OP_MAX, D(DT.F32, i=DT.F32, o=DT.F32), R | ARG)
print(json.dumps(out))
"""


def test_f64_reductions_accepted_and_the_rest_refused():
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1", LIBXSMM_VERBOSE="0")
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    got["no:f32_reduce_rows_argop_refused_as_before"] = got.pop("f32_reduce_rows_argop_refused_as_before")
    wrong = {k: v for k, v in got.items() if v == k.startswith("no:")}
    assert not wrong, f"accepted / refused against the table: {wrong}"
    assert sum(1 for k in got if not k.startswith("no:")) >= 50
