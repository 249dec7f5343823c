"""The call contract of the three domain entries (csrc/bfd_call.h) on the device: a bad ordinal, every refusal with the outputs untouched, the empty
problem, and a call repeated in one process."""
import os

import numpy as np
import pytest

from babelbrain_amd import _engine
from tests import domain_calls as DC, domain_oracle as DO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


@pytest.mark.parametrize('entry', DC.ENTRIES)
def test_ordinal_out_of_range(lib, entry):
    for device in (-1, lib.bfd_device_count()):
        c = DC.Case(entry)
        assert c.run(lib, device) == -3 and 'ordinal' in lib.bfd_last_error().decode() and c.untouched()


@pytest.mark.parametrize('entry', DC.ENTRIES)
def test_refusals_in_order_leave_everything_untouched(lib, entry):
    words = {n: w for n, w, _ in DC.faults(entry)}
    for names, first in DC.ordered_plants(entry):
        c = DC.planted(entry, names)
        assert c.run(lib) == -1 and words[first] in lib.bfd_last_error().decode() and c.untouched(), names


@pytest.mark.parametrize('entry', DC.ENTRIES)
def test_empty_problem(lib, entry):
    """An empty volume with an empty box: 0 after the device pick, kernelMs zeroed; the survey and the assembly report their empty results, the rays
    write nothing"""
    zero = DC.i64([0, 0, 0])
    kw = dict(M=(0, 4, 9), lo=zero, hi=zero.copy()) if entry == 'bfd_label_survey3d' else dict(M=(0, 4, 9), lo=zero, size=zero.copy())
    if entry == 'bfd_assemble_material_map3d':
        kw.update(padLo=DC.i64([0, 2, 1]), padHi=DC.i64([0, 1, 1]))
    c = DC.Case(entry, **kw)
    assert c.run(lib) == 0 and c.ms[0] == 0, lib.bfd_last_error().decode()
    if entry == 'bfd_label_survey3d':
        assert not c.outputs['hist'].any() and list(c.outputs['bounds']) == [-1] * 6 and list(c.outputs['focal']) == [0, -1]
    elif entry == 'bfd_assemble_material_map3d':
        assert list(c.outputs['stats']) == [0, -1, -1, 0, 0, -1, -1, 0] and np.array_equal(c.outputs['map'], c.pristine['map'])
    else:
        assert c.untouched(but_ms=True)


@pytest.mark.parametrize('entry', DC.ENTRIES)
def test_valid_call_twice(lib, entry):
    a, b = DC.Case(entry), DC.Case(entry)
    assert a.run(lib) == 0 and b.run(lib) == 0, lib.bfd_last_error().decode()
    assert a.ms[0] > 0 and b.ms[0] > 0
    for k in a.outputs:
        assert a.outputs[k].tobytes() == b.outputs[k].tobytes(), k
    if entry == 'bfd_label_survey3d':
        want = DO.survey(a.labels, (a.lo, a.hi), a.flipK)
        names = ('hist', 'bounds', 'focal')
    elif entry == 'bfd_assemble_material_map3d':
        want = DO.assemble_entry(a.labels, a.ct, a.air, a.lo, a.size, a.padLo, a.padHi, a.flipK, a.lut, a.ctOffset, a.zWater, a.nMaterials, a.focalIJ)
        names = ('map', 'mapNoCT', 'airOut', 'stats')
    else:
        want = DO.sdr_rays(a.ct, a.hu, (a.lo, a.lo + a.size), a.stepI, a.stepJ, a.minSkull, a.centerRegion, a.flipK)
        names = ('value', 'count', 'state')
    for name, w in zip(names, want):
        assert np.array_equal(a.outputs[name], w), name
    assert a.entry != 'bfd_sdr_rays3d' or (a.outputs['state'] == 1).any()
