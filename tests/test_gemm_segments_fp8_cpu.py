"""8-bit float (BF8 = E5M2, HF8 = E4M3) handles in the segments entries (include/libxsmm_hip.h) without a GPU, in dry-run mode: the four plain entries accept
BF8 / HF8 -> f32 and -> own-type handles (-4: accepted, no device, nothing launched); the workspace query counts 4-byte accumulators; an A that is not VNNI-4,
transposed operands in the OFFSET entries and an ext handle with operators are refused with -3 and one error line that names the reason; an ext handle without
operators is accepted by the ext entries; 8-bit integers stay refused with the words they had."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import ctypes as C
sys.path.insert(0, %(root)r)
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG, UNARY
api = capi.load()
def err():
    e = api.hip_get_last_error(); api.hip_clear_last_error(); return e
def sh(m, n, k, t, c):
    return capi.gemm_shape(m, n, k, m, k, m, t, t, c, DT.I32 if t == DT.I8 else DT.F32)
off, adr = capi.br_config(capi.BR_OFFSET, 0, 0, 0), capi.br_config(capi.BR_ADDRESS, 0, 0, 0)
V, B0, TA, TB = GEMM_FLAG.VNNI_A, GEMM_FLAG.BETA_0, GEMM_FLAG.TRANS_A, GEMM_FLAG.TRANS_B
TYPES = dict(bf8_f32=(DT.BF8, DT.F32), bf8_bf8=(DT.BF8, DT.BF8), hf8_f32=(DT.HF8, DT.F32), hf8_hf8=(DT.HF8, DT.HF8))
M, N, K = 40, 24, 20
H = {}
for tag, (t, c) in TYPES.items():
    H["a_" + tag] = api.dispatch_brgemm(sh(M, N, K, t, c), V | B0, 0, adr)
    H["o_" + tag] = api.dispatch_brgemm(sh(M, N, K, t, c), V, 0, off)
H.update(
    a_flat=api.dispatch_brgemm(sh(32, 32, 32, DT.HF8, DT.F32), 0, 0, adr),
    o_flat=api.dispatch_brgemm(sh(32, 32, 32, DT.BF8, DT.F32), B0, 0, off),
    o_tb=api.dispatch_brgemm(sh(32, 32, 32, DT.HF8, DT.F32), V | TB, 0, off),
    o_ta=api.dispatch_brgemm(sh(32, 32, 32, DT.BF8, DT.F32), TA, 0, off),
    e_relu=api.dispatch_brgemm_ext(sh(32, 32, 32, DT.HF8, DT.HF8), V, 0, adr, capi.argops_cp(32, UNARY.RELU), capi.no_postops()),
    oe_bias=api.dispatch_brgemm_ext(sh(32, 32, 32, DT.BF8, DT.BF8), V, 0, off, capi.no_argops(), capi.postops_colbias(32, DT.BF8)),
    e_none=api.dispatch_brgemm_ext(sh(M, N, K, DT.HF8, DT.HF8), V, 0, adr, capi.no_argops(), capi.no_postops()),
    oe_none=api.dispatch_brgemm_ext(sh(M, N, K, DT.BF8, DT.F32), V | B0, 0, off, capi.no_argops(), capi.no_postops()),
    i8=api.dispatch_brgemm(sh(32, 32, 32, DT.I8, DT.I32), V, 0, adr),
    o_i8=api.dispatch_brgemm(sh(32, 32, 32, DT.I8, DT.I32), V, 0, off),
)
print("handles", ",".join(k for k, v in H.items() if not v) or "all")
# never dereferenced on the host: validation reads none of the arrays, none of the bases and not the workspace
BLK, SEG, LA, LB, LC, WS, A, B, CC, DL = (i << 20 for i in range(1, 11))
NS = 5
def call(tag, fn, *args):
    sys.stderr.write("MARK %%s begin\n" %% tag); sys.stderr.flush()
    fn(*args)
    sys.stderr.write("MARK %%s end\n" %% tag); sys.stderr.flush()
    print(tag, err())
def param(offsets, ext=False):
    p = capi.GemmExtParam() if ext else capi.GemmParam()
    if offsets:
        p.a.primary, p.b.primary, p.c.primary = A, B, CC
    if ext:
        p.d.primary = DL
    return p
def plain(tag, h, offsets):
    fn = api.hip_gemm_batch_reduce_segments_offsets if offsets else api.hip_gemm_batch_reduce_segments
    call(tag, fn, h, C.byref(param(offsets)), NS, SEG, LA, LB, LC)
def sliced(tag, h, offsets):
    need = api.hip_gemm_batch_reduce_segments_sliced_workspace(h, NS)
    api.hip_clear_last_error()
    fn = api.hip_gemm_batch_reduce_segments_offsets_sliced if offsets else api.hip_gemm_batch_reduce_segments_sliced
    call(tag, fn, h, C.byref(param(offsets)), 3, BLK, NS, SEG, LA, LB, LC, WS, need)
def ext(tag, h, offsets):
    fn = api.hip_gemm_ext_batch_reduce_segments_offsets if offsets else api.hip_gemm_ext_batch_reduce_segments
    call(tag, fn, h, C.byref(param(offsets, True)), NS, SEG, LA, LB, LC, None, None)
def ext_sliced(tag, h, offsets):
    need = api.hip_gemm_ext_batch_reduce_segments_sliced_workspace(h, NS) or 1 << 19        # (a refused handle: 0 -- the call gets room enough)
    api.hip_clear_last_error()
    fn = api.hip_gemm_ext_batch_reduce_segments_offsets_sliced if offsets else api.hip_gemm_ext_batch_reduce_segments_sliced
    call(tag, fn, h, C.byref(param(offsets, True)), 3, BLK, NS, SEG, LA, LB, LC, None, None, WS, need)
for tag in TYPES:
    plain("ok_address_" + tag, H["a_" + tag], False)
    plain("ok_offset_" + tag, H["o_" + tag], True)
    sliced("ok_sliced_" + tag, H["a_" + tag], False)
    sliced("ok_offset_sliced_" + tag, H["o_" + tag], True)
    print("query_" + tag, ",".join(str(api.hip_gemm_batch_reduce_segments_sliced_workspace(H[p + tag], n)) for p in ("a_", "o_") for n in (0, 1, 5, 1000)), err())
plain("flat", H["a_flat"], False)
plain("o_flat", H["o_flat"], True)
sliced("s_flat", H["a_flat"], False)
plain("o_tb", H["o_tb"], True)
plain("o_ta", H["o_ta"], True)
sliced("os_tb", H["o_tb"], True)
ext("e_relu", H["e_relu"], False)
ext("oe_bias", H["oe_bias"], True)
ext_sliced("es_relu", H["e_relu"], False)
ext("ok_ext", H["e_none"], False)
ext("ok_ext_offset", H["oe_none"], True)
ext_sliced("ok_ext_sliced", H["e_none"], False)
ext_sliced("ok_ext_offset_sliced", H["oe_none"], True)
plain("i8", H["i8"], False)
plain("o_i8", H["o_i8"], True)
sliced("s_i8", H["i8"], False)
print("query_flat", api.hip_gemm_batch_reduce_segments_sliced_workspace(H["a_flat"], 5), err())
print("launches", api.hip_launch_count(0))
"""

KINDS = ("bf8_f32", "bf8_bf8", "hf8_f32", "hf8_hf8")
ENTRIES = ("address", "offset", "sliced", "offset_sliced")
ACCEPTED = ["ok_%s_%s" % (e, k) for e in ENTRIES for k in KINDS] + ["ok_ext", "ok_ext_offset", "ok_ext_sliced", "ok_ext_offset_sliced"]
REFUSED = {"flat": "taken as VNNI-4 only", "o_flat": "taken as VNNI-4 only", "s_flat": "taken as VNNI-4 only",
           "o_tb": "transposed 8-bit float operands are not taken", "o_ta": "transposed 8-bit float operands are not taken",
           "os_tb": "transposed 8-bit float operands are not taken",
           "e_relu": "taken without operators only", "oe_bias": "taken without operators only", "es_relu": "taken without operators only",
           "i8": "operand types", "o_i8": "operand types", "s_i8": "operand types"}
M, N = 40, 24


@pytest.fixture(scope="module")
def child():
    env = dict(os.environ, LIBXSMM_HIP_DRYRUN="1")
    env.pop("LIBXSMM_VERBOSE", None)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _codes(child):
    return dict(ln.split() for ln in child.stdout.splitlines() if len(ln.split()) == 2 and not ln.startswith("query_"))


def test_every_handle_is_dispatched(child):
    assert _codes(child)["handles"] == "all", child.stdout


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_four_plain_entries_accept_8bit_float_handles(child, entry):
    """BF8 -> f32, BF8 -> BF8, HF8 -> f32, HF8 -> HF8 end with -4: accepted, then no device.  (Without the feature: -3, "operand types".)"""
    got = _codes(child)
    for k in KINDS:
        assert got["ok_%s_%s" % (entry, k)] == "-4", (entry, k, child.stdout + child.stderr)
    assert got["launches"] == "0"


def test_an_ext_handle_without_operators_is_accepted_by_the_ext_entries(child):
    got = _codes(child)
    for tag in ("ok_ext", "ok_ext_offset", "ok_ext_sliced", "ok_ext_offset_sliced"):
        assert got[tag] == "-4", (tag, child.stdout + child.stderr)


def test_refusals_are_minus_three_with_one_error_that_names_the_reason(child):
    got = _codes(child)
    for tag, words in REFUSED.items():
        assert got[tag] == "-3", (tag, child.stdout)
        err = child.stderr.split(f"MARK {tag} begin\n")[1].split(f"MARK {tag} end\n")[0]
        lines = [ln for ln in err.splitlines() if "ERROR" in ln]
        assert len(lines) == 1 and words in lines[0] and "no HIP device" not in err, (tag, err)
    # the message that lists what is taken names the new types
    err = child.stderr.split("MARK i8 begin\n")[1].split("MARK i8 end\n")[0]
    assert "bf8 -> f32 / bf8" in err and "hf8 -> f32 / hf8" in err, err
    # accepted calls print the missing device and nothing else
    for tag in ACCEPTED:
        err = child.stderr.split(f"MARK {tag} begin\n")[1].split(f"MARK {tag} end\n")[0]
        lines = [ln for ln in err.splitlines() if "ERROR" in ln]
        assert len(lines) == 1 and "no HIP device" in lines[0], (tag, err)


def test_the_workspace_query_counts_four_byte_accumulators(child):
    out = dict(ln.split(None, 1) for ln in child.stdout.splitlines() if ln.startswith("query_"))
    for k in KINDS:
        sizes, code = out["query_" + k].split()
        assert code == "0"
        sizes = [int(x) for x in sizes.split(",")]
        for ns, got in zip((0, 1, 5, 1000) * 2, sizes):
            assert got % 16 == 0 and got >= ns * M * N * 4 and got <= ns * (M * N * 4 + 15) and (got == 0) == (ns == 0), (k, ns, got)
    assert out["query_flat"].split() == ["0", "-3"]
