"""Every speaker assignment can win each of the three permutation scans (csrc/pit.inc's enumerator), in the host-side build:
tests/pit_scan_checks.py.  tests/test_gpu_pit_scan.py runs the same check on the device."""
import pytest

from tests import pit_scan_checks as P
from tests import wa_checks as K
from tests.emu_build import load_emu


@pytest.fixture(scope="module")
def be():
    return K.HostBackend(load_emu())


@pytest.mark.parametrize("entry,k", P.CASES)
def test_every_assignment_wins(be, entry, k):
    P.check_every_assignment_wins(be, entry, k)
