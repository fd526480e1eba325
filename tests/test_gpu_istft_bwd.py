"""istft_bwd_kernel (csrc/istft_bwd.inc) on the device: the checks of tests/test_emu_istft_bwd.py (tests/wa_checks.py) with the
same shapes and the same bounds, through the C ABI of the product library."""
import pytest
import torch

from tests import istft_grad_ref as R
from tests import wa_checks as K

pytestmark = pytest.mark.gpu

MODES = [R.MASK, R.PHASE, R.MAG]
CASES = [(mode, shape) for mode in MODES for shape in R.shapes_of(mode)]


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    return K.DeviceBackend(get_lib())


@pytest.mark.parametrize("mode,shape", CASES)
def test_gradient_matches_fp64_adjoint(be, mode, shape):
    K.check_gradient(be, mode, shape)


@pytest.mark.parametrize("mode,shape", CASES)
def test_dot_product_identity(be, mode, shape):
    K.check_dot_product(be, mode, shape)


@pytest.mark.parametrize("mode", MODES)
def test_ragged_rows_are_their_batch1_bytes(be, mode):
    K.check_ragged(be, mode)


def test_strided_masks(be):
    shape = (256, 100, 16, 3)
    K.check_gradient(be, R.PHASE, shape, op_view=K.strided_view(R.case(*shape), R.PHASE))


def test_refusals(be):
    K.check_istft_bwd_refusals(be)


@pytest.mark.parametrize("mode", MODES)
def test_two_calls_give_the_same_bits(be, mode):
    K.check_repeatable(be, mode, (256, 100, 16, 3))
