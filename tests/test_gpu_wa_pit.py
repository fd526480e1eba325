"""The waveform-approximation loss (csrc/loss_wa.inc) on the device: the checks of tests/test_emu_wa_pit.py (tests/wa_checks.py)
through the C ABI of the product library, and ``loss.wa_pit`` over them."""
import numpy as np
import pytest
import torch

from tests import wa_checks as K
from tests import wa_pit_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    return K.DeviceBackend(get_lib())


@pytest.mark.parametrize("n", [777, 4096])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_value_permutation_and_gradient(be, C, n):
    K.check_wa(be, C, n)


def test_ragged_rows(be):
    K.check_wa(be, 3, 4096, ragged=True)


@pytest.mark.parametrize("C,n", [(2, 777), (4, 4096)])
def test_strided_references(be, C, n):
    K.check_wa(be, C, n, strided=True)


def test_exact_tie_takes_the_first_permutation(be):
    K.check_wa(be, 2, 777, tie=True)


def test_refusals(be):
    K.check_wa_refusals(be)


def test_wa_pit_autograd(be):
    """``loss.wa_pit``: value, permutation index and the gradient autograd hands back, ragged, references read in place."""
    from onssen_amd.loss import wa_pit
    k = W.case(3, 4096, ragged=True)
    est = be.dev(k.est).requires_grad_(True)
    ref = W.strided_ref(k)(be)
    V, perm = wa_pit(est, ref, lengths=k.lengths, return_perm=True)
    assert perm.dtype == torch.int64 and perm.tolist() == k.perm_index
    (V * be.dev(k.g_value)).sum().backward()
    assert (np.abs(V.detach().cpu().numpy() - k.V) <= 1e-6 * np.abs(k.V)).all()
    assert est.grad.cpu().numpy().tobytes() == k.grad.astype(np.float32).tobytes()
    with torch.no_grad():
        assert torch.equal(wa_pit(est, ref, lengths=k.lengths), V.detach())
