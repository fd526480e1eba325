"""misi_bwd_frames_kernel / misi_bwd_gather_kernel (csrc/misi_bwd.inc) on the device: the checks of tests/test_emu_misi_bwd.py
(bodies in tests/misi_bwd_checks.py) through the product library, and the autograd node of ``features.misi_phase``."""
import numpy as np
import pytest
import torch

from tests import misi_bwd_checks as K
from tests import misi_cases as MC
from tests import misi_grad_ref as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    return K.DeviceBackend(get_lib())


@pytest.mark.parametrize("shape", G.SHAPES)
def test_gradient_matches_the_fp64_adjoint(be, shape):
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


def test_misi_phase_with_grad_has_the_bits_of_the_plain_call_and_the_abi_gradient(be):
    """``features.misi_phase`` on an ``est`` that requires a gradient: the plain call's bits, a grad_fn, and a backward that is the
    C ABI call's result bit for bit -- uniform and ragged."""
    from onssen_amd import features
    shape = (256, 100, 1500, 3)
    n_fft, hop, n, C = shape
    k, g = MC.case(n_fft, hop, n, C, B=3), G.g_phase(n_fft, hop, n, C, 3)
    mix, g_dev = be.dev(k.mix), be.dev(g)
    for lengths in (None, G.ragged_lengths(n_fft, hop, n)):
        est = be.dev(k.est).requires_grad_(True)
        plain = features.misi_phase(mix, est.detach(), n_fft, hop, lengths=lengths)
        tracked = features.misi_phase(mix, est, n_fft, hop, lengths=lengths)
        assert tracked.grad_fn is not None and not plain.requires_grad and torch.equal(tracked.detach(), plain)
        tracked.backward(g_dev)
        want = K.run_backward(be, k.mix, k.est, n_fft, hop, g, lengths=lengths)
        assert est.grad.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(RuntimeError, match="the mixture is data"):
        features.misi_phase(mix.clone().requires_grad_(True), est, n_fft, hop)
    with pytest.raises(ValueError, match="out= cannot be combined"):
        features.misi_phase(mix, est, n_fft, hop, out=torch.empty_like(plain))
    with torch.no_grad():           # nothing changes without autograd: the plain path, out= included
        out = torch.empty_like(plain)
        assert features.misi_phase(mix, est, n_fft, hop, out=out) is out and not out.requires_grad
