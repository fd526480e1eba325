"""misi_bwd_frames_kernel / misi_bwd_gather_kernel (csrc/misi_bwd.inc) in the host-side build: onssen_misi_phase_backward_f32
against the float64 adjoint of tests/misi_grad_ref.py; ragged batches, strided estimates, a silent speaker, repeatability,
refusals; the whole unfolded chain through the C ABI.  The check bodies are tests/misi_bwd_checks.py's, shared with the GPU."""
import pytest

from tests import misi_bwd_checks as K
from tests import misi_grad_ref as G
from tests.emu_build import load_emu


@pytest.fixture(scope="module")
def be():
    return K.HostBackend(load_emu())


@pytest.mark.parametrize("shape", G.SHAPES)
def test_gradient_matches_the_fp64_adjoint(be, shape):
    """Measured on this build, max |got - ref| / max |ref| per shape: the table in DESIGN section 25; the largest is
    G.GRAD_MEASURED_REL and the asserted bound 4 x that, under the 1e-5 ceiling."""
    K.check_gradient(be, shape)


@pytest.mark.parametrize("shape", G.RAGGED_SHAPES)
def test_ragged_rows_are_their_batch1_bytes(be, shape):
    K.check_ragged(be, shape)


def test_strided_estimates(be):
    K.check_strided(be, (256, 64, 777, 5))


@pytest.mark.parametrize("shape", [(256, 64, 768, 2), (256, 100, 1500, 3)])
def test_a_silent_speaker_contributes_nothing(be, shape):
    K.check_zero_speaker(be, shape)


def test_two_calls_give_the_same_bits(be):
    K.check_repeatable(be, (256, 64, 2000, 4))


def test_refusals_leave_the_output_untouched(be):
    K.check_refusals(be)


@pytest.mark.parametrize("iters", [1, 2])
def test_the_whole_chain_through_the_abi(be, iters):
    """d loss / d masks through K unfolded iterations, every launch of the C ABI, against torch float64 autograd of the whole chain.
    Measured on this build, max |got - ref| / max |ref|: K = 1 and K = 2 in DESIGN section 25; the larger is
    G.CHAIN_MEASURED_REL, the bound of this and of the device's test (tests/test_gpu_misi_train_e2e.py) 4 x that."""
    c = G.chain_case()
    mix, _, gy, got = K.chain_through_abi(be, c, iters)
    err, top = K.chain_error(got, c, iters, mix, gy)
    print(f"unfolded MISI K = {iters}: max |got - ref| {err:.3e}, max |ref| {top:.3e} ({err / top:.3e} relative; bound "
          f"{G.CHAIN_REL_BOUND:.3e}, ceiling 1e-4)")
    assert top > 0 and err <= 1e-4 * top and err <= G.CHAIN_REL_BOUND * top
