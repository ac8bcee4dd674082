"""The lean f32 streaming kernel (gemm_lean_kernels.hip), read from the code objects inside libxsmm_amd.so (no GPU needed).

Its arguments are separate parameters that the dispatch preloads into SGPRs (the translation unit is compiled with -amdgpu-kernarg-preload-count):
every instance's kernel descriptor must carry a kernarg-preload length, and the 32-bit-stride instances must preload everything the single-chunk form
reads before its first load (a, b, c, three batch strides, nbatch, lda, ldb, ldc: 13 dwords).  The streaming instance (POL 3) stores C with `sc1`
(measured faster than `nt` on the headline launch), the cacheable one (POL 0) keeps `nt`."""
import os
import re
import struct
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr   # noqa: E402

LIB = os.path.join(ROOT, "libxsmm_amd", "lib", "libxsmm_amd.so")
pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(kr.LLVM, "llvm-readelf"))),
                                reason="needs the built library and the ROCm LLVM tools")
FAMILY = "_ZN4xamd27gemm_f32_stream_kernel_lean"
NARROW_DWORDS = 13                    # 3 pointers (6) + 3 u32 batch strides + nbatch + lda + ldb + ldc


def _sections(path):
    out = subprocess.check_output([f"{kr.LLVM}/llvm-readelf", "-S", "--wide", path], text=True)
    secs = []
    for line in out.splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            secs.append((m.group(1), int(m.group(2), 16), int(m.group(3), 16), int(m.group(4), 16)))
    return secs


@pytest.fixture(scope="module")
def lean():
    """{mangled kernel name: (kernarg preload length in dwords, disassembly)} of every lean instance"""
    found = {}
    for image in kr.code_objects(LIB):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(image)
            f.flush()
            syms = subprocess.check_output([f"{kr.LLVM}/llvm-readelf", "-s", "--wide", f.name], text=True)
            kds = {}
            for line in syms.splitlines():
                parts = line.split()
                if len(parts) >= 8 and parts[-1].startswith(FAMILY) and parts[-1].endswith(".kd"):
                    kds[parts[-1][:-3]] = int(parts[1], 16)
            if not kds:
                continue
            secs = _sections(f.name)
            text = subprocess.check_output([f"{kr.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", f.name], text=True)
            bodies = dict(re.findall(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, re.S | re.M))
            for name, addr in kds.items():
                sec = [s for s in secs if s[1] <= addr < s[1] + s[3]][0]
                off = addr - sec[1] + sec[2]
                (preload,) = struct.unpack_from("<H", image, off + 58)     # amdhsa kernel descriptor: kernarg_preload, bits 0-6 = length in dwords
                found[name] = (preload & 0x7F, bodies.get(name, ""))
    assert found, "no gemm_f32_stream_kernel_lean instance in the library"
    return found


def _demangled(name):
    return kr.demangle([name])[0]


def test_every_instance_preloads_its_arguments(lean):
    short = {}
    for name, (length, _) in lean.items():
        pretty = _demangled(name)
        want = NARROW_DWORDS if ", unsigned int>" in pretty else 1
        if length < want:
            short[pretty] = length
    assert not short, f"kernarg preload length too short: {short}"
    assert any(", long long>" in _demangled(n) for n in lean), "the 64-bit batch-stride instances are missing"


def _stores(body):
    return [line for line in body.splitlines() if "buffer_store_dwordx4" in line]


def test_streaming_instance_stores_c_sc1(lean):
    for name, (_, body) in lean.items():
        pretty = _demangled(name)
        m = re.search(r"gemm_f32_stream_kernel_lean<(true|false), (true|false), (true|false), (\d)", pretty)
        pol = int(m.group(4))
        if pol not in (0, 3):
            continue
        stores = _stores(body)
        assert len(stores) == 4, (pretty, stores)
        for s in stores:
            bits = set(s.split("//", 1)[0].split("offen", 1)[1].split())
            if pol == 3:
                assert "sc1" in bits and "nt" not in bits and "sc0" not in bits, (pretty, s)
            else:
                assert bits == {"nt"}, (pretty, s)


def test_first_load_does_not_wait_for_the_argument_block(lean):
    """The headline instance: no scalar load of the kernarg block between the preloaded entry point and the first operand load."""
    name = [n for n in lean if _demangled(n).startswith("void xamd::gemm_f32_stream_kernel_lean<false, false, true, 3, unsigned int>")]
    assert len(name) == 1
    body = lean[name[0]][1].splitlines()
    # the compatibility prologue for firmware without preloading ends in s_branch to the real entry point 256 bytes in
    entry = next(i for i, line in enumerate(body) if "s_branch" in line)
    first = next(i for i, line in enumerate(body) if "buffer_load_dwordx4" in line)
    assert entry < first
    assert not [line for line in body[entry + 1:first] if "s_load" in line or "s_waitcnt" in line]
