"""The LPIPS training loss without a device: the autograd reference of tests/lpips_bwd_ref.py in fp32 against
fp64 on the cases the GPU test uses. A case whose fp32 CPU gradient is off by more than 1e-4 has a ReLU /
max-pool decision that flips between the precisions and cannot pin a kernel; such a seed is not used."""
import pytest

from tests import lpips_bwd_ref as B


@pytest.mark.parametrize("name", sorted(B.CASES))
def test_cases_have_no_precision_flip(name):
    pred, target, l64, g64, l32, g32 = B.case(name)
    assert pred.shape == target.shape and float(pred.abs().max()) <= 1.0 and float(target.abs().max()) <= 1.0
    rel_v = abs(float(l32) - float(l64)) / float(l64)
    rel_g = B.rel_l2(g32, g64)
    print(f"{name}: loss {float(l64):.6e}, fp32 CPU value error {rel_v:.2e}, gradient error {rel_g:.2e}")
    assert float(l64) > 0 and float(g64.norm()) > 0
    assert rel_v <= 1e-4
    assert rel_g <= B.CPU_FP32_GRAD_BOUND
