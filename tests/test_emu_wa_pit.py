"""The waveform-approximation loss (csrc/loss_wa.inc) in the host-side build: value, permutation and gradient against the float64
reference of tests/wa_pit_cases.py, ragged rows, strided references, an exact tie, repeatability (inside every check), refusals.
tests/test_gpu_wa_pit.py runs the same checks on the device."""
import pytest

from tests import wa_checks as K
from tests.emu_build import load_emu


@pytest.fixture(scope="module")
def be():
    return K.HostBackend(load_emu())


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
