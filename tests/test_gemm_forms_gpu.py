"""bf16 GEMM in the operand forms other than VNNI-A / flat-B [ref: src/generator_gemm_reference_impl.c:2127-2170, :2149-2161, :2803-2815]: flat or transposed A,
transposed or transposed-VNNI B, C in VNNI-2 -- on the matrix cores since round 4 (`gemm_bf16_forms_kernel`: whole 32-tiles, 16-byte aligned rows), against the
oracle's restatement of the reference loop within the reference driver's own bf16 bound; everything else stays on the exact kernel (bit-identical, checked elsewhere)."""
import numpy as np
import pytest

from gemm_ld_helpers import assert_dense
from helpers import GemmCase, TOL_BF16, TOL_F32, normf_rel
from libxsmm_amd import capi
from libxsmm_amd.capi import DT, GEMM_FLAG as F

pytestmark = pytest.mark.gpu

A_FORMS = {"vnni": F.VNNI_A, "flat": 0, "trans": F.TRANS_A}
B_FORMS = {"flat": 0, "trans": F.TRANS_B, "tvnni": F.TRANS_B | F.VNNI_B}


@pytest.mark.parametrize("af", list(A_FORMS))
@pytest.mark.parametrize("bf", list(B_FORMS))
@pytest.mark.parametrize("kw", [dict(m=32, n=32, k=32), dict(m=64, n=64, k=64, c_type=DT.F32, beta=1), dict(m=64, n=32, k=96, br_type=capi.BR_STRIDE, br_count=3),
                                dict(m=32, n=64, k=32, colbias=True, act=2), dict(m=96, n=32, k=64, lda=104, ldb=136, ldc=98, beta=1)],
                         ids=["32", "64_f32_beta1", "strdbr3", "bias_relumask", "padded_ld"])
def test_every_operand_form_on_the_matrix_cores(af, bf, kw):
    if af == "vnni" and bf == "flat":
        pytest.skip("the fast form has its own kernels and tests")
    api = capi.load()
    kw = dict(kw)
    flags = A_FORMS[af] | B_FORMS[bf]
    if "lda" in kw:            # the padded leading dimensions above are for (A: m-major, B: k-major); transposed operands lead with the other extent
        if af == "trans":
            kw["lda"] = 72     # >= k
        if bf != "flat":
            kw["ldb"] = 40     # >= n
    case = GemmCase(seed=4242, batch=5, a_type=DT.BF16, c_type=kw.pop("c_type", DT.BF16), flags=flags, **kw)
    got, gmask, handle = case.run_gpu(batched=True)
    ref, rmask = case.run_oracle()
    assert api.hip_kernel_name(handle, 1).decode() == "gemm_bf16_forms_kernel"
    err = normf_rel(case.valid_region(ref), case.valid_region(got), case.c_type)
    assert err < (TOL_BF16 if case.c_type == DT.BF16 else TOL_F32), err
    assert_dense(case, got, ref, got_mask=gmask)


@pytest.mark.parametrize("af,bf", [("vnni", "flat"), ("flat", "trans"), ("trans", "tvnni")])
def test_c_in_vnni2(af, bf):
    api = capi.load()
    case = GemmCase(64, 32, 64, seed=17, batch=4, a_type=DT.BF16, c_type=DT.BF16, flags=A_FORMS[af] | B_FORMS[bf] | F.VNNI_C, br_type=capi.BR_STRIDE, br_count=2)
    got, _, handle = case.run_gpu(batched=True)
    ref, _ = case.run_oracle()
    assert api.hip_kernel_name(handle, 1).decode() == "gemm_bf16_forms_kernel"
    # the VNNI-2 image is a permutation of C: compare it as it lies (bf16 -> f64), norm-wise
    err = normf_rel(ref, got, DT.BF16)
    assert err < TOL_BF16, err
    assert_dense(case, got, ref)


def test_shapes_and_alignments_outside_the_plan_stay_exact():
    api = capi.load()
    for kw in (dict(m=12, n=10, k=8, flags=F.TRANS_B), dict(m=32, n=32, k=32, flags=F.TRANS_A, lda=33), dict(m=32, n=32, k=32, flags=F.VNNI_A | F.TRANS_B, br_type=capi.BR_OFFSET, br_count=2)):
        case = GemmCase(seed=5, batch=3, a_type=DT.BF16, c_type=DT.BF16, **kw)
        got, _, handle = case.run_gpu(batched=True)
        ref, _ = case.run_oracle()
        assert api.hip_kernel_name(handle, 1).decode() == "gemm_generic_kernel"
        assert np.array_equal(case.valid_region(ref), case.valid_region(got))
        assert_dense(case, got, ref)
