"""The Step-1 call contract (csrc/bfd_call.h) on the device, for each of the eight entries with its smallest valid arguments: a device ordinal out
of range is refused with nothing written, an empty problem returns 0 with kernelMs zeroed, and a call can be repeated in one process with the same
result (scratch and events of the first have been released)."""
import numpy as np
import pytest

from babelbrain_amd import _engine
from tests.step1_calls import ADMIT_EMPTY, ENTRIES, MS_SENTINEL, Case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    return _engine.load_library()


@pytest.mark.parametrize('entry', ENTRIES)
def test_ordinal_out_of_range(lib, entry):
    case = Case(entry)
    assert case.run(lib, lib.bfd_device_count()) == -3
    assert lib.bfd_last_error().decode() == entry + ': device ordinal out of range'
    assert case.untouched()


@pytest.mark.parametrize('entry', ADMIT_EMPTY)
def test_empty_problem(lib, entry):
    case = Case(entry, empty=True)
    assert case.run(lib, 0) == 0
    assert case.ms[0] == 0 and (case.ms[1] == 0 or entry != 'bfd_affine_transform3d')


@pytest.mark.parametrize('entry', ENTRIES)
def test_valid_call_twice(lib, entry):
    case = Case(entry)
    assert case.run(lib, 0) == 0, lib.bfd_last_error().decode()
    assert case.ms[0] > 0 and (case.ms[1] > 0 or entry != 'bfd_affine_transform3d')
    first = case.snapshot()
    assert any(not np.array_equal(first[k], case.pristine[k]) for k in first)        # the call wrote its result
    for k, v in case.outputs.items():                 # sentinels again: the second call has to write everything itself
        v[...] = case.pristine[k]
    case.ms[:] = MS_SENTINEL
    assert case.run(lib, 0) == 0, lib.bfd_last_error().decode()
    assert case.ms[0] > 0
    for k, v in case.outputs.items():
        assert np.array_equal(v, first[k]), k
