"""istft_bwd_kernel (csrc/istft_bwd.inc) in the host-side build: the gradient of the three inverse transforms against the float64
adjoint of tests/istft_grad_ref.py, the dot-product identity through the C ABI alone, ragged batches, refusals, repeatability.
The check bodies are tests/wa_checks.py's; tests/test_gpu_istft_bwd.py runs the same ones on the device."""
import pytest

from tests import istft_grad_ref as R
from tests import wa_checks as K
from tests.emu_build import load_emu

MODES = [R.MASK, R.PHASE, R.MAG]
CASES = [(mode, shape) for mode in MODES for shape in R.shapes_of(mode)]


@pytest.fixture(scope="module")
def be():
    return K.HostBackend(load_emu())


def test_reference_adjoints_match_torch_autograd():
    """The helper checks itself: explicit adjoints against torch float64 autograd of the same restatement, on the CPU."""
    worst = R.self_check()
    print(f"largest relative difference adjoint / autograd: {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("mode,shape", CASES)
def test_gradient_matches_fp64_adjoint(be, mode, shape):
    """Bound: 4 x the largest max |got - ref| this build gives over all shapes, per gradient kind (R.GRAD_MEASURED_MAX; per-shape
    values in DESIGN section 23); ceiling 1e-5 max |ref| per case."""
    K.check_gradient(be, mode, shape)


@pytest.mark.parametrize("mode,shape", CASES)
def test_dot_product_identity(be, mode, shape):
    K.check_dot_product(be, mode, shape)


@pytest.mark.parametrize("mode", MODES)
def test_ragged_rows_are_their_batch1_bytes(be, mode):
    K.check_ragged(be, mode)


def test_strided_masks(be):
    """The phase mode reads the masks (for g_phase): here as a view of a larger buffer, NaN around it."""
    shape = (256, 100, 16, 3)
    K.check_gradient(be, R.PHASE, shape, op_view=K.strided_view(R.case(*shape), R.PHASE))


def test_refusals(be):
    K.check_istft_bwd_refusals(be)


@pytest.mark.parametrize("mode", MODES)
def test_two_calls_give_the_same_bits(be, mode):
    K.check_repeatable(be, mode, (256, 100, 16, 3))
