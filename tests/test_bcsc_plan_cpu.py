"""plan_bcsc (csrc/bcsc_plan.hpp) on every row of tests/test_bcsc_parity_gpu.py: BCSC, without a GPU: tests/bcsc_plan_main.cpp -- the plan header and a main, compiled
with g++ alone -- must name the kernel the row expects (the GPU test asserts the same name on what launch_bcsc launched), and its grid arithmetic must keep what
the kernels rely on.

A row becomes BcscArgs as the library would fill them: the operands 256 + skew (the skews are bytes behind a 256-byte boundary), a table; a host or bound pattern has
the table ready, its block count, and the k-blocks of the first 64 columns as kmask0 when K / bk <= 64; a device pattern has none of the three."""
import os
import shutil
import subprocess

import pytest

from bcsc_parity_helpers import BcscCase
from test_bcsc_parity_gpu import BCSC, _id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMING = (2, 3)                # BcscForm: kBcscStream, kBcscFull


def args_line(kw):
    case = BcscCase(**dict(kw, mb=1, data="zeros"))              # the pattern and the types; the M-block count goes over as the row has it
    mb = kw.get("mb", 3)
    known = case.pattern_on in ("host", "bound")
    kmask0 = 0
    if known and case.K // case.bk <= 64:
        for nb, col in enumerate(case.cols):
            if nb * case.bn < 64:
                for kb in col:
                    kmask0 |= 1 << kb
    ptrs = [256 + case.skew[x] for x in "ABC"]
    vals = ptrs + [case.M, case.N, case.K, mb, case.bk, case.bn, int(case.a_type), int(case.b_type), int(case.c_type), int(case.vnni), int(case.beta == 0),
                   4096, case.hint, int(case.hint == 2), int(known), kmask0, case.nnzb if known else 0]
    return " ".join(str(v) for v in vals), case, mb


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("bcsc_plan") / "bcsc_plan_main"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "bcsc_plan_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [args_line(kw) for _, kw in BCSC]
    r = subprocess.run([str(exe)], input="\n".join(line for line, _, _ in rows) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = [dict(f.split("=", 1) for f in line.split()) for line in r.stdout.splitlines()]
    assert len(out) == len(BCSC)
    return [(kernel, kw, case, mb, {k: (v if k == "name" else int(v)) for k, v in p.items()}) for (kernel, kw), (_, case, mb), p in zip(BCSC, rows, out)]


def test_the_plan_names_the_kernel_every_row_expects(plans):
    assert len(plans) == 69
    wrong = [(_id((kernel, kw)), p["name"]) for kernel, kw, _, _, p in plans if p["name"] != kernel]
    assert not wrong, wrong


def test_the_plan_keeps_what_the_kernels_rely_on(plans):
    streamed = 0
    for kernel, kw, case, mb, p in plans:
        rid = _id((kernel, kw))
        tiles = -(-case.M // 64) * -(-case.N // 64)
        assert p["invert"] == (case.pattern_on == "device" and p["form"] != 0), rid              # only the kernels that read the table, and only when nobody filled it
        if p["form"] in STREAMING:
            streamed += 1
            slots = 3072 if p["three"] else 2048
            assert p["waves"] == p["mbg"] * tiles and p["waves"] <= slots, rid
            assert 1 <= p["mbg"] <= mb, rid
            fit = min(mb, max(1, slots // tiles))                                    # the M-blocks that fit at a time, before rounding
            assert -(-mb // p["mbg"]) == -(-mb // fit) and p["mbg"] <= fit, rid     # rounding mbg down never costs a wave another M-block
        else:
            assert p["total"] == (-(-case.M // 64) * case.N * mb if kernel == "bcsc_generic_kernel" else tiles * mb), rid
        if "full" in kernel:
            assert case.M % 64 == 0 and case.N % 64 == 0 and p["early"] == (case.N == 64), rid
    assert streamed > 0
