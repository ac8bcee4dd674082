"""GPU parity of the dense GEMM / BRGEMM kernels at PADDED leading dimensions (lda > m, ldb > k, ldc > m; transposed operands: lda > k, ldb > n).

Every row of DENSE is a GemmCase whose gaps are poisoned (tests/gemm_ld_helpers.py: input gaps hold the type's NaN, gaps of C a sentinel), run through the
batched launcher and held to assert_dense: no non-finite result, every byte outside m x n equal to the oracle's buffer, and a per-element float64 bound
(types the float64 restatement does not cover: the oracle's bar per problem).  The row names the kernel the dispatcher is expected to pick for THAT padding,
asserted through libxsmm_hip_kernel_name: padding that keeps every row / column on 16 bytes keeps a family's fast kernel, padding that breaks it (an odd
leading dimension) forces the family's fallback, and the row of the fallback says so.

Dense kernel names the table cannot reach are listed in UNREACHABLE with the reason (each keeps its own test); tests/test_gemm_ld_cpu.py holds DENSE and UNREACHABLE
against every kernel name string of the dense sources.
"""
import numpy as np
import pytest

from gemm_ld_helpers import assert_dense, block_masks, gap_values, poison
from helpers import GemmCase
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG as F

pytestmark = pytest.mark.gpu
# dense kernel names a 1-D strided batch of a padded GemmCase cannot reach, with the reason (tests/test_gemm_ld_cpu.py holds this and DENSE against the name strings of csrc/)
UNREACHABLE = {
    "gemm_f32_blocked_kernel<1>": "2-D batches only (libxsmm_hip_gemm_batch_strided_2d), packed square tiles by design: tests/test_batch2d_gpu.py",
    "gemm_f32_blocked_kernel<2>": "2-D batches only, packed square tiles by design: tests/test_batch2d_gpu.py",
    "gemm_f32_blocked16_kernel": "2-D batches only, packed 16^3 tiles by design: tests/test_batch2d_gpu.py",
    "gemm_f64_blocked_kernel<1>": "2-D batches only, packed square tiles by design: test_f64_2d_batch_is_the_callers_two_loops",
    "gemm_f64_blocked_kernel<2>": "2-D batches only, packed square tiles by design: test_f64_2d_batch_is_the_callers_two_loops",
    "gemm_bf16_macro_kernel": "2-D batches only, 16-byte aligned rows: tests/test_batch2d_gpu.py",
    "gemm_f16_macro_kernel": "2-D batches only, 16-byte aligned rows: tests/test_batch2d_gpu.py",
    "gemm_f32_dma_kernel<1,1>": "behind a compile-time switch that is off (f32_dma_mode() < 2 in csrc/gemm_kernels.hip): no descriptor reaches it",
    "gemm_bitmask16_kernel": "A is a compressed stream without a leading dimension, GemmCase does not build it: test_gemm_with_bitmask_compressed_a (padded ldb / ldc)",
    "gemm_bitmask_reg_kernel": "A is a compressed stream without a leading dimension: test_gemm_with_bitmask_compressed_a (padded ldb / ldc)",
    "gemm_mx6_stream_kernel<1,1>": "6-bit triples, GemmCase does not build them: test_mx6_gemm_bit_exact (padded rows of its own)",
    "gemm_mx6_stream_kernel<2,2>": "6-bit triples: test_mx6_gemm_bit_exact",
    "gemm_mx4i8_stream_kernel<1,1>": "interleaved nibbles with block scales: test_interleaved_4bit_weight_gemm_bit_exact",
    "gemm_mx4i8_stream_kernel<2,2>": "interleaved nibbles with block scales; the plan never picks 2 x 2 (csrc/gemm_kernels.hip: plan_gemm)",
    "gemm_mx4i8_pipe_kernel": "interleaved nibbles with block scales: test_interleaved_4bit_weight_gemm_bit_exact",
    "gemm_i1_stream_kernel<1,1>": "bit-packed weights: test_low_bit_weight_gemm_bit_exact", "gemm_i1_stream_kernel<2,2>": "bit-packed weights: test_low_bit_weight_gemm_bit_exact",
    "gemm_i2_stream_kernel<1,1>": "bit-packed weights: test_low_bit_weight_gemm_bit_exact", "gemm_i2_stream_kernel<2,2>": "bit-packed weights: test_low_bit_weight_gemm_bit_exact",
    "gemm_i4_stream_kernel<1,1>": "nibble weights with zero points: test_interleaved_4bit_weight_gemm_bit_exact",
    "gemm_i4_stream_kernel<2,2>": "nibble weights with zero points: test_interleaved_4bit_weight_gemm_bit_exact",
}
S, O, A = capi.BR_STRIDE, capi.BR_OFFSET, capi.BR_ADDRESS
MXMX = F.VNNI_A | F.VNNI_B | F.TRANS_B


def f32(**kw):
    return dict(**kw)


def b16(c=DT.BF16, **kw):
    return dict(dict(a_type=DT.BF16, c_type=c, flags=F.VNNI_A), **kw)


def h16(c=DT.F16, **kw):
    return dict(dict(a_type=DT.F16, c_type=c, flags=F.VNNI_A), **kw)


def f64(**kw):
    return dict(a_type=DT.F64, **kw)


def q8(a, b=None, c=DT.I32, **kw):
    return dict(dict(a_type=a, b_type=a if b is None else b, c_type=c, flags=F.VNNI_A), **kw)


# (kernel expected for this padding, case) -- "aligned": every leading dimension keeps rows / columns on 16 bytes; "odd": it does not
DENSE = [
    # ---- f32 ------------------------------------------------------------------------------------------------------------------------------------------
    # the lean streaming kernel: 32 x 32 tiles, beta = 0; aligned padding keeps it, an odd lda / ldb falls back to the direct-load tile kernel <1,1>
    ("gemm_f32_stream_kernel_lean", f32(m=32, n=32, k=32, lda=36, ldb=40, ldc=48, br_type=S, br_count=3, batch=67)),
    ("gemm_f32_stream_kernel_lean", f32(m=32, n=32, k=64, lda=36, ldb=68, ldc=33, batch=67)),                         # odd ldc alone keeps it (element stores of C)
    ("gemm_f32_stream_kernel", f32(m=32, n=32, k=32, lda=36, ldb=40, ldc=48, beta=1, br_type=S, br_count=3, batch=67)),   # beta = 1 / epilogues: the general streaming kernel
    ("gemm_f32_stream_kernel", f32(m=32, n=32, k=32, lda=40, ldb=36, ldc=35, colbias=True, act=2, batch=9)),
    ("gemm_mfma_f32_kernel<1,1>", f32(m=32, n=32, k=32, lda=33, ldb=35, ldc=37, br_type=S, br_count=2, batch=67)),
    ("gemm_mfma_f32_kernel<1,1>", f32(m=32, n=32, k=32, lda=33, ldb=36, ldc=40, beta=1, br_type=O, br_count=3, batch=5)),
    ("gemm_mfma_f32_kernel<1,1>", f32(m=13, n=7, k=5, lda=8, ldb=6, ldc=15, flags=F.TRANS_A, beta=1, batch=5)),
    ("gemm_mfma_f32_kernel<1,1>", f32(m=32, n=32, k=32, lda=33, ldb=35, ldc=37, colbias=True, act=2, batch=9)),       # whole tile, odd lda: the exact instantiation, fused
    ("gemm_mfma_f32_kernel<1,1>", f32(m=32, n=32, k=32, lda=36, ldb=40, ldc=44, flags=F.TRANS_B, br_type=A, br_count=2, batch=5)),
    # several whole tiles per problem: LDS-DMA kernel when aligned, direct-load <2,2> when odd
    ("gemm_f32_dma_kernel<2,2>", f32(m=128, n=64, k=64, lda=132, ldb=68, ldc=136, batch=9)),
    ("gemm_f32_dma_kernel<2,2>", f32(m=128, n=64, k=32, lda=132, ldb=36, ldc=129, beta=1, br_type=S, br_count=2, colbias=True, act=2, batch=5)),
    ("gemm_mfma_f32_kernel<2,2>", f32(m=64, n=64, k=64, lda=65, ldb=67, ldc=69, beta=1, batch=9)),
    ("gemm_mfma_f32_kernel<2,2>", f32(m=64, n=64, k=32, lda=65, ldb=33, ldc=67, beta=1, br_type=S, br_count=2, colbias=True, act=2, batch=5)),
    ("gemm_mfma_f32_kernel<2,2>", f32(m=64, n=64, k=32, lda=68, ldb=36, ldc=72, br_type=O, br_count=3, batch=3)),     # offsets live on the device: direct loads
    ("gemm_mfma_f32_kernel<2,2>", f32(m=128, n=64, k=32, lda=33, ldb=67, ldc=131, flags=F.TRANS_A | F.TRANS_B, batch=3)),
    # 64^3: one problem per workgroup; B shared by a large batch: persistent workgroups
    ("gemm_f32_wg64_kernel", f32(m=64, n=64, k=64, lda=68, ldb=72, ldc=80, batch=9)),
    ("gemm_f32_wg64_kernel", f32(m=64, n=64, k=96, lda=68, ldb=100, ldc=65, beta=1, br_type=S, br_count=3, batch=5)),
    ("gemm_f32_wg64_kernel", f32(m=64, n=64, k=32, lda=72, ldb=36, ldc=68, colbias=True, act=2, batch=3)),
    ("gemm_f32_wg64_sharedb_kernel", f32(m=64, n=64, k=64, lda=68, ldb=72, ldc=80, shared_b=True, batch=2051)),
    # 16^3: a problem per wave (p16w: A by 16-byte LDS-DMA; p16: dword loads of A when lda is not a multiple of 4; p16s from 2048 steps on); beta = 1: t16
    ("gemm_f32_p16w_kernel", f32(m=16, n=16, k=16, lda=20, ldb=20, ldc=24, batch=67)),
    ("gemm_f32_p16w_kernel", f32(m=16, n=16, k=32, lda=20, ldb=36, ldc=20, br_type=S, br_count=3, batch=67)),
    ("gemm_f32_p16_kernel", f32(m=16, n=16, k=16, lda=18, ldb=20, ldc=24, batch=67)),
    ("gemm_mfma_f32_t16_kernel", f32(m=16, n=16, k=16, lda=18, ldb=19, ldc=21, batch=67)),                           # odd ldb / ldc take 16^3 off the problem-per-wave kernels
    ("gemm_f32_p16s_kernel", f32(m=16, n=16, k=16, lda=20, ldb=20, ldc=24, batch=16387)),
    ("gemm_f32_p16s_kernel", f32(m=16, n=16, k=16, lda=20, ldb=24, ldc=20, shared_b=True, batch=3001)),
    ("gemm_mfma_f32_t16_kernel", f32(m=16, n=16, k=16, lda=20, ldb=20, ldc=24, beta=1, batch=67)),
    ("gemm_mfma_f32_t16_kernel", f32(m=48, n=16, k=32, lda=49, ldb=33, ldc=51, beta=1, br_type=S, br_count=2, colbias=True, act=2, batch=5)),
    # one masked tile out of a blob of at most 1024 dwords (fused epilogues of small ragged shapes)
    ("gemm_f32_blob_kernel", f32(m=20, n=12, k=16, lda=24, ldb=17, ldc=21, colbias=True, act=2, beta=1, batch=37)),
    ("gemm_f32_blob_kernel", f32(m=23, n=23, k=23, lda=24, ldb=25, ldc=28, colbias=True, act=1, batch=5)),
    # ragged shapes: one problem per workgroup, register-staged (gemm_f32_ragged_kernel) or by LDS-DMA in K chunks (gemm_f32_wgp_kernel)
    ("gemm_f32_ragged_kernel", f32(m=17, n=9, k=31, lda=20, ldb=33, ldc=19, beta=1, batch=37)),
    ("gemm_f32_ragged_kernel", f32(m=23, n=23, k=23, lda=24, ldb=40, ldc=29, batch=37)),
    ("gemm_f32_ragged_kernel", f32(m=29, n=31, k=30, lda=31, ldb=32, ldc=33, br_type=A, br_count=3, beta=1, batch=5)),
    ("gemm_f32_ragged_kernel", f32(m=29, n=31, k=30, lda=32, ldb=31, ldc=30, br_type=O, br_count=4, batch=5)),
    ("gemm_f32_ragged_kernel", f32(m=29, n=31, k=30, lda=30, ldb=34, ldc=36, br_type=S, br_count=5, batch=5)),
    ("gemm_f32_wgp_kernel", f32(m=128, n=120, k=200, lda=132, ldb=204, ldc=131, beta=1, br_type=S, br_count=2, batch=5)),
    ("gemm_f32_wgp_kernel", f32(m=112, n=112, k=112, lda=116, ldb=120, ldc=116, batch=5)),
    # a long chain in ONE call is split over the chip (a batch of one)
    ("gemm_f32_brchain_kernel", f32(m=32, n=32, k=32, lda=36, ldb=40, ldc=44, beta=1, br_type=S, br_count=1000, batch=1)),
    # ---- bf16 / f16 -----------------------------------------------------------------------------------------------------------------------------------
    ("gemm_bf16_stream_kernel<1,1>", b16(m=32, n=32, k=32, lda=36, ldb=40, ldc=40, br_type=S, br_count=3, batch=37)),
    ("gemm_bf16_stream_kernel<1,1>", b16(DT.F32, m=32, n=32, k=64, lda=40, ldb=72, ldc=33, beta=1, batch=37)),
    ("gemm_bf16_stream_kernel<2,2>", b16(m=128, n=64, k=64, lda=132, ldb=72, ldc=136, colbias=True, act=2, batch=9)),
    ("gemm_f16_stream_kernel<1,1>", h16(m=32, n=32, k=32, lda=36, ldb=40, ldc=33, br_type=S, br_count=3, batch=37)),
    ("gemm_f16_stream_kernel<2,2>", h16(m=128, n=64, k=64, lda=132, ldb=72, ldc=136, batch=9)),
    # 64 x 64 x 64 j: one problem per wave (odd batch: the last workgroup has a wave without a problem); other k: one per workgroup
    ("gemm_bf16_w64_kernel", b16(m=64, n=64, k=64, lda=80, ldb=96, ldc=72, batch=37)),
    ("gemm_bf16_w64_kernel", b16(m=64, n=64, k=128, lda=68, ldb=136, ldc=65, beta=1, br_type=S, br_count=2, colbias=True, act=2, batch=37)),
    ("gemm_f16_w64_kernel", h16(m=64, n=64, k=64, lda=80, ldb=96, ldc=65, batch=37)),
    ("gemm_f16_w64_kernel", h16(DT.F32, m=64, n=64, k=64, lda=68, ldb=72, ldc=68, beta=1, batch=37)),
    ("gemm_bf16_wg64_kernel", b16(m=64, n=64, k=96, lda=68, ldb=104, ldc=66, batch=9)),
    ("gemm_f16_wg64_kernel", h16(m=64, n=64, k=96, lda=68, ldb=104, ldc=65, batch=9)),
    # 16^3 bf16: two problems per wave
    ("gemm_bf16_p16w_kernel", b16(m=16, n=16, k=16, lda=20, ldb=24, ldc=24, batch=5)),
    ("gemm_bf16_p16_kernel", b16(m=16, n=16, k=16, lda=18, ldb=24, ldc=24, batch=9)),
    ("gemm_mfma_bf16_kernel<1,1>", b16(m=16, n=16, k=16, lda=18, ldb=18, ldc=17, batch=9)),                          # B columns / C columns off 16 bytes: the masked tile kernel
    ("gemm_bf16_p16s_kernel", b16(DT.F32, m=16, n=16, k=16, lda=20, ldb=24, ldc=20, batch=32771)),
    # ragged 16-bit: one problem per workgroup out of LDS when every 16-byte piece lies inside its block (lda % 4, ldb % 8), else a wave per tile with clamped loads
    ("gemm_bf16_wgp_kernel", b16(m=40, n=40, k=40, lda=44, ldb=48, ldc=41, batch=37)),
    ("gemm_bf16_wgp_kernel", b16(DT.F32, m=72, n=40, k=48, lda=76, ldb=56, ldc=74, beta=1, br_type=S, br_count=4, batch=37)),
    ("gemm_bf16_wgp_kernel", b16(m=72, n=72, k=72, lda=76, ldb=80, ldc=73, colbias=True, act=2, beta=1, batch=5)),
    ("gemm_f16_wgp_kernel", h16(m=40, n=40, k=40, lda=44, ldb=48, ldc=42, batch=37)),
    ("gemm_mfma_bf16_kernel<2,2>", b16(m=40, n=40, k=40, lda=41, ldb=41, ldc=43, batch=37)),
    ("gemm_mfma_bf16_kernel<2,2>", b16(m=40, n=33, k=200, lda=44, ldb=202, ldc=42, beta=1, batch=37)),
    ("gemm_mfma_bf16_kernel<2,2>", b16(m=40, n=40, k=38, lda=42, ldb=40, ldc=44, br_type=A, br_count=2, batch=5)),
    ("gemm_mfma_bf16_kernel<2,2>", b16(m=40, n=40, k=38, lda=42, ldb=40, ldc=44, br_type=O, br_count=2, beta=1, batch=5)),
    ("gemm_mfma_bf16_kernel<2,2>", b16(m=40, n=40, k=40, lda=41, ldb=43, ldc=45, br_type=S, br_count=3, batch=37)),
    # whole 32 / 64 tiles with B columns off 16 bytes (odd ldb): the exact-tile instantiation of the same kernel
    ("gemm_mfma_bf16_kernel<1,1>", b16(m=32, n=32, k=32, lda=33, ldb=35, ldc=37, br_type=S, br_count=2, batch=37)),
    ("gemm_mfma_bf16_kernel<2,2>", b16(DT.F32, m=64, n=64, k=64, lda=65, ldb=67, ldc=69, beta=1, colbias=True, act=2, batch=9)),
    ("gemm_mfma_f16_kernel<1,1>", h16(m=32, n=32, k=32, lda=33, ldb=35, ldc=37, batch=37)),
    ("gemm_mfma_bf16_kernel<1,1>", b16(m=24, n=24, k=24, lda=25, ldb=27, ldc=29, beta=1, colbias=True, act=2, batch=37)),
    ("gemm_mfma_bf16_kernel<1,1>", b16(m=7, n=5, k=2, lda=9, ldb=4, ldc=8, batch=37)),
    ("gemm_mfma_f16_kernel<2,2>", h16(m=40, n=40, k=40, lda=41, ldb=41, ldc=43, beta=1, batch=37)),
    ("gemm_mfma_f16_kernel<2,2>", h16(m=40, n=40, k=40, lda=41, ldb=43, ldc=45, br_type=S, br_count=2, batch=37)),
    ("gemm_mfma_f16_kernel<1,1>", h16(m=24, n=24, k=24, lda=26, ldb=28, ldc=25, br_type=A, br_count=2, batch=5)),
    ("gemm_mfma_f16_kernel<1,1>", h16(DT.F32, m=24, n=24, k=24, lda=26, ldb=28, ldc=25, br_type=O, br_count=3, batch=5)),
    ("gemm_mfma_f16_kernel<1,1>", h16(DT.F32, m=17, n=7, k=16, lda=20, ldb=24, ldc=24, colbias=True, act=2, beta=1, batch=37)),
    # the other operand forms on the matrix cores: whole 32-tiles, rows on 16 bytes; anything else: the exact kernel
    ("gemm_bf16_forms_kernel", dict(a_type=DT.BF16, c_type=DT.BF16, flags=F.TRANS_A | F.TRANS_B, m=96, n=32, k=64, lda=72, ldb=40, ldc=98, beta=1, batch=5)),
    ("gemm_bf16_forms_kernel", dict(a_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A | F.TRANS_B | F.VNNI_B, m=96, n=32, k=64, lda=104, ldb=40, ldc=98, batch=5)),
    ("gemm_bf16_forms_kernel", dict(a_type=DT.BF16, c_type=DT.F32, flags=F.TRANS_B, m=64, n=32, k=96, lda=72, ldb=40, ldc=65, br_type=S, br_count=3, colbias=True, act=2, batch=5)),
    ("gemm_bf16_forms_kernel", dict(a_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A | F.VNNI_C, m=64, n=32, k=64, lda=72, ldb=72, ldc=72, br_type=S, br_count=2, batch=5)),
    ("gemm_generic_kernel", dict(a_type=DT.BF16, c_type=DT.BF16, flags=F.TRANS_A, m=32, n=32, k=32, lda=33, ldb=34, ldc=35, batch=3)),
    # the forms kernel takes plain and STRIDE batch-reduce only (the alignment of listed blocks is not decidable on the host): OFFSET / ADDRESS run on the exact kernel
    ("gemm_generic_kernel", dict(a_type=DT.BF16, c_type=DT.BF16, flags=F.TRANS_B, m=32, n=32, k=32, lda=40, ldb=40, ldc=36, br_type=O, br_count=2, batch=3)),
    ("gemm_generic_kernel", dict(a_type=DT.BF16, c_type=DT.F32, flags=F.TRANS_A | F.TRANS_B, m=32, n=32, k=32, lda=40, ldb=40, ldc=36, beta=1, br_type=A, br_count=2, batch=3)),
    ("gemm_generic_kernel", dict(a_type=DT.BF16, c_type=DT.BF16, m=12, n=10, k=9, lda=13, ldb=11, ldc=14, beta=1, batch=3)),
    ("gemm_generic_kernel", dict(a_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A | F.VNNI_C, m=16, n=5, k=8, lda=18, ldb=10, ldc=20, batch=3)),
    ("gemm_generic_kernel", dict(a_type=DT.F16, c_type=DT.F16, flags=F.VNNI_A | F.VNNI_C, m=17, n=7, k=16, lda=20, ldb=24, ldc=24, batch=3)),
    ("gemm_generic_kernel", dict(a_type=DT.HF8, c_type=DT.HF8, flags=F.VNNI_C, m=17, n=7, k=16, lda=20, ldb=24, ldc=24, batch=3)),
    # ---- 8-bit ----------------------------------------------------------------------------------------------------------------------------------------
    # whole tiles with B columns on 16 bytes: streaming kernels; the workgroup-per-problem kernel takes packed A / B only (padded ldc keeps it)
    ("gemm_i8_stream_kernel<1,1>", q8(DT.I8, m=32, n=32, k=64, lda=36, ldb=80, ldc=33, beta=1, br_type=S, br_count=3, batch=5)),
    ("gemm_i8_stream_kernel<1,1>", q8(DT.U8, DT.I8, DT.F32, m=64, n=32, k=160, lda=72, ldb=176, ldc=80, scf=0.25, beta=1, batch=3)),
    ("gemm_i8_stream_kernel<2,2>", q8(DT.I8, DT.U8, m=64, n=64, k=64, lda=68, ldb=80, ldc=72, batch=5)),
    ("gemm_i8_stream_kernel<2,2>", q8(DT.U8, m=64, n=64, k=96, lda=80, ldb=112, ldc=65, beta=1, br_type=S, br_count=2, batch=3)),
    ("gemm_fp8_stream_kernel<1,1>", q8(DT.BF8, c=DT.F32, m=32, n=32, k=64, lda=36, ldb=80, ldc=33, br_type=S, br_count=3, batch=5)),
    ("gemm_fp8_stream_kernel<2,2>", q8(DT.HF8, c=DT.F32, m=64, n=64, k=96, lda=72, ldb=112, ldc=80, beta=1, colbias=True, act=2, batch=3)),
    ("gemm_fp8c8_stream_kernel<1,1>", q8(DT.HF8, c=DT.HF8, m=32, n=32, k=64, lda=36, ldb=80, ldc=40, br_type=S, br_count=2, batch=5)),
    ("gemm_fp8c8_stream_kernel<2,2>", q8(DT.BF8, c=DT.BF8, m=64, n=64, k=64, lda=68, ldb=80, ldc=65, beta=1, colbias=True, act=2, batch=3)),
    ("gemm_8bit_wgp_kernel", q8(DT.I8, m=72, n=72, k=72, ldc=76, beta=1, br_type=S, br_count=2, batch=9)),
    ("gemm_8bit_wgp_kernel", q8(DT.BF8, c=DT.F32, m=72, n=40, k=48, ldc=73, batch=9)),
    ("gemm_8bit_wgp_kernel", q8(DT.HF8, c=DT.F32, m=72, n=72, k=72, ldc=76, colbias=True, act=2, beta=1, batch=5)),   # the 8-bit floats fuse (the integers do not)
    # every other shape or alignment with whole k-quads: the masked matrix-core kernel (clamped loads)
    ("gemm_mfma_8bit_kernel<2,2>", q8(DT.I8, m=72, n=72, k=72, lda=76, ldb=80, ldc=76, batch=9)),                   # padded A / B take the packed shape off the wgp kernel
    ("gemm_mfma_8bit_kernel<2,2>", q8(DT.U8, DT.I8, m=40, n=40, k=40, lda=41, ldb=43, ldc=45, beta=1, br_type=S, br_count=3, batch=7)),
    ("gemm_mfma_8bit_kernel<2,2>", q8(DT.HF8, c=DT.F32, m=70, n=33, k=100, lda=72, ldb=102, ldc=75, beta=1, batch=3)),
    ("gemm_mfma_8bit_kernel<1,1>", q8(DT.U8, m=23, n=37, k=20, lda=25, ldb=21, ldc=29, beta=1, batch=3)),
    ("gemm_mfma_8bit_kernel<1,1>", q8(DT.I8, DT.U8, m=32, n=32, k=64, lda=36, ldb=68, ldc=40, br_type=A, br_count=3, batch=3)),
    ("gemm_mfma_8bit_kernel<1,1>", q8(DT.BF8, c=DT.BF8, m=17, n=9, k=12, lda=18, ldb=13, ldc=20, colbias=True, act=2, beta=1, batch=3)),
    ("gemm_mfma_8bit_kernel<1,1>", q8(DT.BF8, c=DT.F32, m=32, n=32, k=64, lda=33, ldb=66, ldc=35, br_type=O, br_count=2, batch=3)),
    ("gemm_generic_kernel", dict(a_type=DT.U8, b_type=DT.I8, c_type=DT.I32, m=12, n=10, k=7, lda=13, ldb=9, ldc=14, batch=3)),
    # 8-bit float weights x bf16 activations
    ("gemm_w8_bf16_kernel<1,1>", dict(a_type=DT.BF8, b_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A, m=32, n=32, k=32, lda=36, ldb=40, ldc=33, beta=1, batch=5)),
    ("gemm_w8_bf16_kernel<2,2>", dict(a_type=DT.HF8, b_type=DT.BF16, c_type=DT.F32, flags=F.VNNI_A, m=96, n=64, k=32, lda=100, ldb=40, ldc=100, batch=3)),
    ("gemm_w8_wgp_kernel", dict(a_type=DT.HF8, b_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A, m=72, n=40, k=48, ldc=76, beta=1, batch=3)),
    ("gemm_w8_wgp_kernel", dict(a_type=DT.BF8, b_type=DT.BF16, c_type=DT.F32, flags=F.VNNI_A, m=72, n=40, k=48, ldc=73, br_type=S, br_count=2, batch=3)),
    ("gemm_w8_bf16_kernel<1,1>", dict(a_type=DT.HF8, b_type=DT.BF16, c_type=DT.F32, flags=F.VNNI_A, m=32, n=32, k=32, lda=36, ldb=40, ldc=40, br_type=S, br_count=3, batch=5)),
    ("gemm_w8_bf16_kernel<1,1>", dict(a_type=DT.BF8, b_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A, m=32, n=32, k=32, lda=33, ldb=34, ldc=35, br_type=A, br_count=2, batch=3)),
    ("gemm_w8_bf16_kernel<2,2>", dict(a_type=DT.BF8, b_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A, m=64, n=64, k=32, lda=68, ldb=40, ldc=66, beta=1, br_type=O, br_count=2, batch=3)),
    ("gemm_w8_bf16_kernel<2,2>", dict(a_type=DT.HF8, b_type=DT.BF16, c_type=DT.F32, flags=F.VNNI_A, m=40, n=40, k=40, lda=41, ldb=43, ldc=45, br_type=S, br_count=2, batch=7)),
    # ---- MX, BF32 -------------------------------------------------------------------------------------------------------------------------------------
    ("gemm_mxfp4_stream_kernel<1,1>", dict(a_type=DT.MXFP4X2, b_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A, m=96, n=32, k=32, lda=100, ldb=40, ldc=98, beta=1, br_type=S, br_count=2, batch=3)),
    ("gemm_mxfp4_stream_kernel<2,2>", dict(a_type=DT.MXFP4X2, b_type=DT.BF16, c_type=DT.F32, flags=F.VNNI_A, m=64, n=64, k=64, lda=72, ldb=72, ldc=68, batch=5)),
    ("gemm_generic_kernel", dict(a_type=DT.MXFP4X2, b_type=DT.BF16, c_type=DT.F32, flags=F.VNNI_A, m=64, n=64, k=64, lda=66, ldb=65, ldc=67, batch=5)),     # odd ldb: the exact kernel
    ("gemm_generic_kernel", dict(a_type=DT.MXFP4X2, b_type=DT.F32, c_type=DT.F32, flags=F.VNNI_A, m=17, n=9, k=64, lda=20, ldb=65, ldc=24, beta=1, batch=3)),
    ("gemm_mx_stream_kernel<1,1>", dict(a_type=DT.MXBF8, b_type=DT.MXBF8, c_type=DT.F32, flags=MXMX, m=32, n=96, k=64, lda=40, ldb=100, ldc=36, batch=5)),
    ("gemm_mx_stream_kernel<2,2>", dict(a_type=DT.MXFP4X2, b_type=DT.MXFP4X2, c_type=DT.F32, flags=MXMX, m=64, n=64, k=128, lda=68, ldb=65, ldc=67, beta=1, br_type=S, br_count=2, batch=3)),
    ("gemm_generic_kernel", dict(a_type=DT.MXHF8, b_type=DT.MXHF8, c_type=DT.F32, flags=MXMX, m=33, n=5, k=32, lda=34, ldb=7, ldc=37, batch=3)),
    ("gemm_bf32_stream_kernel", dict(a_type=DT.BF32, m=32, n=32, k=32, lda=36, ldb=40, ldc=33, colbias=True, act=2, beta=1, br_type=S, br_count=3, batch=5)),
    ("gemm_bf32_stream_kernel", dict(a_type=DT.BF32, m=64, n=32, k=64, lda=68, ldb=72, ldc=72, batch=5)),
    ("gemm_generic_kernel", dict(a_type=DT.BF32, m=32, n=32, k=32, lda=33, ldb=35, ldc=37, br_type=O, br_count=2, batch=3)),      # odd ld or listed blocks: the exact kernel
    ("gemm_generic_kernel", dict(a_type=DT.BF32, m=17, n=9, k=31, lda=20, ldb=33, ldc=19, colbias=True, act=2, beta=1, batch=3)),
    # ---- f64 ------------------------------------------------------------------------------------------------------------------------------------------
    ("gemm_f64_stream_kernel", f64(m=96, n=64, k=32, lda=98, ldb=34, ldc=100, batch=7)),
    ("gemm_f64_stream_kernel", f64(m=64, n=32, k=64, lda=66, ldb=34, ldc=65, flags=F.TRANS_A | F.TRANS_B, beta=1, br_type=S, br_count=2, batch=7)),
    ("gemm_f64_stream64_kernel", f64(m=128, n=64, k=96, lda=130, ldb=98, ldc=132, beta=1, batch=7)),
    ("gemm_f64_stream64_kernel", f64(m=64, n=64, k=64, lda=66, ldb=66, ldc=65, batch=7)),
    ("gemm_f64_ragged_kernel", f64(m=72, n=72, k=72, lda=75, ldb=73, ldc=77, batch=5)),
    ("gemm_f64_ragged_kernel", f64(m=32, n=32, k=32, lda=33, ldb=35, ldc=37, beta=1, br_type=O, br_count=4, batch=5)),
    ("gemm_f64_ragged_kernel", f64(m=23, n=17, k=9, lda=24, ldb=11, ldc=25, br_type=A, br_count=3, batch=5)),
    ("gemm_f64_ragged_kernel", f64(m=40, n=50, k=17, lda=19, ldb=18, ldc=41, flags=F.TRANS_A, beta=1, batch=5)),
    ("gemm_f64_p16_kernel", f64(m=16, n=16, k=16, lda=18, ldb=18, ldc=17, beta=1, batch=37)),
    ("gemm_f64_p16_kernel", f64(m=16, n=16, k=48, lda=18, ldb=50, ldc=20, br_type=S, br_count=3, batch=37)),
]


def _id(v):
    if isinstance(v, str):
        return v
    names = {F.TRANS_A: "ta", F.TRANS_B: "tb", F.VNNI_A: "va", F.VNNI_B: "vb", F.VNNI_C: "vc"}
    parts = []
    for k, x in v.items():
        if k == "flags":
            x = "".join(s for f, s in names.items() if x & f)
        elif k in ("a_type", "b_type", "c_type"):
            x = int(x)
        parts.append(f"{k}{x}")
    return "-".join(parts)


def run_row(kernel, kw, seed=8128):
    """poison -> batched launch -> assert_dense; returns (kernel name, stats)."""
    api = capi.load()
    case = GemmCase(seed=seed, **kw)
    mk = poison(case)
    assert (~mk["C0"]).any(), "the row does not pad C"
    got, gmask, handle = case.run_gpu(batched=True)
    name = api.hip_kernel_name(handle, 1 if case.batch > 1 else 0).decode()
    ref, _ = case.run_oracle()
    stats = {}
    assert_dense(case, got, ref, got_mask=gmask, stats=stats)
    return name, stats


@pytest.mark.parametrize("kernel,kw", DENSE, ids=_id)
def test_dense_kernels_at_padded_leading_dimensions(kernel, kw):
    name, stats = run_row(kernel, kw)
    print(f"LD_STAT {name} {stats}")
    assert name == kernel, f"expected {kernel}, library picked {name}"


# ---- grouped batches and segments: one poisoned, padded case per precision class through the same assert_dense ------------------------------------------------
GROUPED = [
    dict(m=20, n=24, k=18, lda=23, ldb=21, ldc=29, batch=3, seed=5),                                                                  # f32 class
    dict(m=32, n=32, k=32, lda=36, ldb=40, ldc=33, beta=1, batch=7, seed=6),
    dict(m=24, n=48, k=32, lda=28, ldb=36, ldc=25, br_type=S, br_count=3, batch=4, seed=7),
    dict(m=24, n=40, k=34, a_type=DT.BF16, c_type=DT.F32, flags=F.VNNI_A, br_type=S, br_count=2, lda=27, ldb=37, ldc=30, batch=2, seed=25),      # bf16 class
    dict(m=48, n=48, k=48, a_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A, beta=1, lda=52, ldb=56, ldc=50, batch=3, seed=24),
    dict(m=13, n=17, k=29, a_type=DT.BF16, c_type=DT.BF16, lda=14, ldb=31, ldc=15, batch=3, seed=23),
    dict(m=23, n=17, k=9, a_type=DT.F64, lda=24, ldb=11, ldc=25, beta=1, batch=3, seed=8),                                            # groups that fall back to their own launches
    dict(m=23, n=37, k=20, a_type=DT.U8, b_type=DT.I8, c_type=DT.I32, flags=F.VNNI_A, lda=25, ldb=21, ldc=29, beta=1, batch=3, seed=9),
]


def test_grouped_batches_at_padded_leading_dimensions():
    from test_gemm_grouped_gpu import Group, _grouped
    api = capi.load()
    cases = [GemmCase(**kw) for kw in GROUPED]
    for case in cases:
        poison(case)
    groups = [Group(api, case) for case in cases]
    api.hip_launch_count(1)
    _grouped(api, [g.entry() for g in groups])
    # one launch of gemm_grouped_f32_kernel for the three f32 groups, one of gemm_grouped_bf16_kernel for the three bf16 groups, the f64 and the 8-bit group their own:
    # a list that fell back to one launch per group would count eight
    assert api.hip_launch_count(1) == 4
    for kw, g in zip(GROUPED, groups):
        ref, _ = g.case.run_oracle()
        stats = {}
        assert_dense(g.case, g.result(), ref, stats=stats)
        print(f"LD_STAT grouped {_id(kw)} {stats}")


SEGMENTS = [
    dict(m=23, n=17, k=9, lda=24, ldb=11, ldc=25, beta=1),
    dict(m=32, n=32, k=32, lda=36, ldb=40, ldc=33),
    dict(m=23, n=17, k=9, a_type=DT.F64, lda=25, ldb=10, ldc=24),
    dict(m=40, n=24, k=34, a_type=DT.BF16, c_type=DT.BF16, flags=F.VNNI_A, lda=42, ldb=37, ldc=44, beta=1),
    dict(m=32, n=32, k=32, a_type=DT.BF16, c_type=DT.F32, flags=F.VNNI_A, lda=36, ldb=40, ldc=36),
]


@pytest.mark.parametrize("kw", SEGMENTS, ids=_id)
def test_segments_at_padded_leading_dimensions(kw):
    """Every block of the pools poisoned; each segment is then one STRIDE batch-reduce problem over its own blocks for assert_dense."""
    from test_gemm_segments_gpu import Segments
    api = capi.load()

    def poison_pools(seg):
        ma, mb, mc = block_masks(seg.case)
        va, vb, vc = gap_values(seg.case)
        for pool, mask, val in ((seg.A, ma, va), (seg.B, mb, vb), (seg.C0, mc, vc)):
            for b in range(pool.nblocks):
                pool.block(pool.host, b)[~mask] = val
    seg = Segments(api, seed=77, prepare=poison_pools, **kw)
    mc = block_masks(seg.case)[2]
    got = seg.run_checked()
    want = {DT.F32: "gemm_segments_f32_kernel", DT.F64: "gemm_segments_f64_kernel", DT.BF16: "gemm_segments_bf16_kernel"}[seg.case.a_type]
    assert api.hip_kernel_name(seg.handle, 1).decode() == want
    worst = {}
    for s, cnt in enumerate(int(c) for c in seg.counts):
        c0, g = seg.C0.block(seg.C0.host, s), seg.C0.block(got, s)
        if cnt == 0:                                      # an empty segment follows beta: zeros or C0 inside m x n, the sentinel outside
            want = c0.copy()
            if not kw.get("beta"):
                want[mc] = 0
            assert np.array_equal(g.view(np.uint8), want.view(np.uint8)), s
            continue
        lo = int(seg.seg_ptr[s])
        case = GemmCase(seed=0, batch=1, br_type=S, br_count=cnt, **kw)
        case.A = np.concatenate([seg.A.block(seg.A.host, int(b)) for b in seg.ai[lo:lo + cnt]])
        case.B = np.concatenate([seg.B.block(seg.B.host, int(b)) for b in seg.bi[lo:lo + cnt]])
        case.C0 = c0.copy()
        ref, _ = case.run_oracle()
        stats = {}
        assert_dense(case, g, ref, stats=stats)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in stats.items()}
    print(f"LD_STAT segments {_id(kw)} {worst}")


def test_host_resident_vnni4_c_with_pad_columns():
    """C of an 8-bit float type as VNNI-4 with n % 4 = 1 in plain HOST memory (a synchronous call stages it): the staged image spans the pad columns up to a multiple of
    four, so the zeros of columns 5 .. 7 and of rows m .. ldc - 1 come back to the caller's buffer and nothing is written behind the device copy."""
    api = capi.load()
    case = GemmCase(8, 5, 16, a_type=DT.HF8, c_type=DT.HF8, flags=F.VNNI_C, lda=12, ldb=20, ldc=24, seed=5)
    poison(case)
    ref, _ = case.run_oracle()
    Cbuf = case.C0.copy()
    handle = case.dispatch(api)
    assert handle
    p, keep = case.make_param(case.A, case.B, Cbuf)          # numpy memory: not visible to the GPU
    capi.Api.call(handle, p)
    api.check()
    assert api.hip_kernel_name(handle, 0).decode() == "gemm_generic_kernel"
    assert_dense(case, Cbuf, ref)
