"""examples/segments_conv_driver.c: a plain C99 caller of libxsmm_hip_gemm_ext_batch_reduce_segments_offsets -- a 3 x 3 convolution forward with bias + ReLU +
bitmask as one call per image, one set of offset lists for two images -- compiles against the public headers alone and matches its host convolution."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_c_example_runs_a_convolution_with_bias_relu_and_bitmask(tmp_path):
    libdir = os.path.join(ROOT, "libxsmm_amd", "lib")
    exe = str(tmp_path / "segments_conv_driver")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "segments_conv_driver.c"),
           "-L" + libdir, "-lxsmm_amd", "-lm", "-Wl,-rpath," + libdir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("normf_rel") == 2 and r.stdout.count(" 0 mask bits differ") == 2, r.stdout
    assert "gemm_segments_offs_f32_fused_kernel<0,0>" in r.stdout and "with 18 of 27" in r.stdout, r.stdout
