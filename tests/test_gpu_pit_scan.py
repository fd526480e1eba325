"""Every speaker assignment can win each of the three permutation scans (csrc/pit.inc's enumerator), on the device: the check of
tests/test_emu_pit_scan.py (tests/pit_scan_checks.py) through the C ABI of the product library."""
import pytest
import torch

from tests import pit_scan_checks as P
from tests import wa_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    return K.DeviceBackend(get_lib())


@pytest.mark.parametrize("entry,k", P.CASES)
def test_every_assignment_wins(be, entry, k):
    P.check_every_assignment_wins(be, entry, k)
