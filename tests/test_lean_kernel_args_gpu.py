"""The lean f32 streaming kernel's argument layout (gemm_lean_kernels.hip: separate preloaded parameters, 32-bit batch strides where they fit and a 64-bit
instance for the rest) against the k-ordered fmaf chain of the oracle, bit for bit: ragged batch counts, the chunked form (br > 1, k > 32), every transpose
combination, both cache policies of 16-byte aligned C (streaming and cacheable) and the dword-store forms, and batch strides past 4 GiB."""
import ctypes as C

import numpy as np
import pytest

from helpers import GemmCase
from libxsmm_amd import capi
from libxsmm_amd.capi import GEMM_FLAG

pytestmark = pytest.mark.gpu

TRANS = [0, GEMM_FLAG.TRANS_A, GEMM_FLAG.TRANS_B, GEMM_FLAG.TRANS_A | GEMM_FLAG.TRANS_B]


def _run(case, hint):
    api = capi.load()
    api.hip_set_streaming_hint(hint)
    try:
        got, _, handle = case.run_gpu(batched=True)
    finally:
        api.hip_set_streaming_hint(0)
    assert api.hip_kernel_name(handle, 1).decode() == "gemm_f32_stream_kernel_lean"
    ref, _ = case.run_oracle(fma=True)
    assert np.array_equal(case.valid_region(ref), case.valid_region(got))


@pytest.mark.parametrize("flags", TRANS)
@pytest.mark.parametrize("hint", [1, 2])                 # 1: cacheable operands (POL 0), 2: streamed from HBM (POL 3)
@pytest.mark.parametrize("batch", [2, 5, 4097])
def test_single_chunk_ragged_batches(flags, hint, batch):
    _run(GemmCase(32, 32, 32, flags=flags, br_type=capi.BR_STRIDE, br_count=1, batch=batch, seed=700 + batch), hint)


@pytest.mark.parametrize("flags", TRANS)
@pytest.mark.parametrize("hint", [1, 2])
def test_chunked_batch_reduce(flags, hint):
    _run(GemmCase(32, 32, 64, flags=flags, br_type=capi.BR_STRIDE, br_count=3, batch=131, seed=710), hint)


@pytest.mark.parametrize("hint", [1, 2])
def test_dword_stores_padded_c(hint):
    """ldc = 33: C rows are not 16-byte aligned, the dword-store policies (POL 2 / 1) with padded leading dimensions of A and B"""
    _run(GemmCase(32, 32, 32, lda=36, ldb=40, ldc=33, br_type=capi.BR_STRIDE, br_count=2, batch=67, seed=720), hint)


@pytest.mark.parametrize("hint", [1, 2])
def test_batch_stride_past_4_gib(hint):
    """B's batch stride is 4 GiB + 4 KiB: the launcher takes the 64-bit-stride instance; both problems land where they belong"""
    import torch
    api = capi.load()
    dev = torch.device("cuda:0")
    case = GemmCase(32, 32, 32, br_type=capi.BR_STRIDE, br_count=1, batch=3, seed=730)
    big = (1 << 32) + 4096
    n = case.b_elems
    Bbig = torch.empty((2 * big) // 4 + n, dtype=torch.float32, device=dev)
    Bh = torch.from_numpy(case.B)
    for b in range(case.batch):
        Bbig[b * big // 4:b * big // 4 + n] = Bh[b * n:(b + 1) * n].to(dev)
    A = torch.from_numpy(case.A).to(dev)
    Cbuf = torch.from_numpy(case.C0.copy()).to(dev)
    handle = case.dispatch(api)
    assert handle
    p, keep = case.make_param(A, Bbig, Cbuf)
    api.hip_set_streaming_hint(hint)
    try:
        api.hip_gemm_batch_strided(handle, C.byref(p), case.batch, case.bs_a, big, case.bs_c)
        api.hip_sync()
        api.check()
    finally:
        api.hip_set_streaming_hint(0)
    assert api.hip_kernel_name(handle, 1).decode() == "gemm_f32_stream_kernel_lean"
    got = Cbuf.cpu().numpy()
    del Bbig
    ref, _ = case.run_oracle(fma=True)
    assert np.array_equal(case.valid_region(ref), case.valid_region(got))
