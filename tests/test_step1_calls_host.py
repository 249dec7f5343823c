"""The part of the Step-1 call contract (csrc/bfd_call.h) that a machine without a device can show: a valid call of each of the eight entries gets
as far as the device question and is refused there with -3, the shared message under the entry's own name, and nothing written."""
import os

import pytest

from babelbrain_amd import _engine
from tests.step1_calls import ENTRIES, Case


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _engine.load_library()
    if lib.bfd_device_count() > 0:
        pytest.skip('a device is visible: the refusal for want of one cannot be shown here')
    return lib


@pytest.mark.parametrize('entry', ENTRIES)
def test_no_device_is_refused_and_nothing_written(lib, entry):
    case = Case(entry)
    assert case.run(lib, 0) == -3
    assert lib.bfd_last_error().decode() == entry + ': no HIP device available (no CPU fallback)'
    assert case.untouched()
