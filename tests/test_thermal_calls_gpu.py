"""The call contract of the two exposure-analysis entries (csrc/bfd_call.h) on the device: a bad ordinal, every refusal with the outputs untouched,
the data refusals after the device pick with kernelMs zeroed and nothing else written, the empty problem, and a call repeated in one process."""
import os

import numpy as np
import pytest

from babelbrain_amd import ThermalAnalysis as TA, _engine
from tests import thermal_calls as TC, thermal_oracle as TO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


@pytest.mark.parametrize('entry', TC.ENTRIES)
def test_ordinal_out_of_range(lib, entry):
    for device in (-1, lib.bfd_device_count()):
        c = TC.Case(entry)
        assert c.run(lib, device) == -3 and 'ordinal' in lib.bfd_last_error().decode() and c.untouched()


@pytest.mark.parametrize('entry', TC.ENTRIES)
def test_refusals_in_order_leave_everything_untouched(lib, entry):
    words = {n: w for n, w, _ in TC.faults(entry)}
    for names, first in TC.ordered_plants(entry):
        c = TC.planted(entry, names)
        assert c.run(lib) == -1 and words[first] in lib.bfd_last_error().decode() and c.untouched(), names


@pytest.mark.parametrize('entry', TC.ENTRIES)
def test_data_refusals_zero_kernel_ms_and_write_nothing_else(lib, entry):
    """An id beyond the table, then a value that is not finite; both together: the id is named, as the header orders them"""
    def spoil(c, what):
        if 'id' in what:
            c.map[2, 3, 8] = c.nMat
        if 'value' in what:
            (c.vols[1] if entry == 'bfd_class_extrema3d' else c.pw)[-1, -1, -1] = np.inf
    for what, word in (('id', 'nMat'), ('value', 'finite'), ('id value', 'nMat')):
        c = TC.Case(entry)
        spoil(c, what)
        if entry == 'bfd_loss_survey3d':
            c.pristine = c.snapshot()
        assert c.run(lib) == -1, what
        text = lib.bfd_last_error().decode()
        assert text.startswith(entry + ': ' + TA.DATA_REFUSED) and word in text, text
        assert c.untouched(but_ms=True) and c.ms[0] == 0, what
    if entry == 'bfd_loss_survey3d':                                # in place: the water field keeps its bytes on a refusal
        c = TC.Case(entry)
        c.p[1, 0, 0, 0] = np.nan
        c.outputs['waterOut'] = c.pw
        c.pristine = c.snapshot()
        assert c.run(lib) == -1 and c.untouched(but_ms=True) and c.ms[0] == 0


@pytest.mark.parametrize('entry', TC.ENTRIES)
def test_empty_problem(lib, entry):
    """An empty volume: 0 after the device pick, kernelMs zeroed, counts and sums 0, maxima 0, indices -1"""
    c = TC.Case(entry, N=(0, 4, 9))
    assert c.run(lib) == 0 and c.ms[0] == 0, lib.bfd_last_error().decode()
    o = c.outputs
    if entry == 'bfd_class_extrema3d':
        assert not o['count'].any() and not o['maxIn'].any() and not o['maxKey'].any() and (o['argIn'] == -1).all() and (o['argKey'] == -1).all()
    else:
        assert not o['maxTissue'].any() and not o['maxWater'].any() and (o['argTissue'] == -1).all() and (o['argWater'] == -1).all()
        assert not o['eWaterRaw'].any() and not o['eWater'].any() and not o['eTissue'].any()
        assert np.array_equal(o['waterOut'], c.pristine['waterOut'])


@pytest.mark.parametrize('entry', TC.ENTRIES)
def test_valid_call_twice(lib, entry):
    a, b = TC.Case(entry), TC.Case(entry)
    assert a.run(lib) == 0 and b.run(lib) == 0, lib.bfd_last_error().decode()
    assert a.ms[0] > 0 and b.ms[0] > 0
    for k in a.outputs:
        assert a.outputs[k].tobytes() == b.outputs[k].tobytes(), k
    if entry == 'bfd_class_extrema3d':
        want = TO.class_extrema(a.vols, a.map, a.classOf)
        for name, w in zip(('count', 'maxIn', 'argIn', 'maxKey', 'argKey'), want):
            assert np.array_equal(a.outputs[name], w), name
    else:
        for f in range(2):
            w = TO.loss_survey(a.p[f], a.pw[f], a.map, a.classOf, a.rho, a.c, a.rhoWater, a.cWater, a.dx2)
            assert np.array_equal(a.outputs['waterOut'][f], w['water'])
            for k in ('maxTissue', 'argTissue', 'maxWater', 'argWater'):
                assert a.outputs[k][f] == w[k], k
            for k in ('eWaterRaw', 'eWater', 'eTissue'):
                assert np.allclose(a.outputs[k][f], w[k], rtol=1e-14, atol=0), k          # 12 terms: within 11 u of the exact sum each
    # NULL for the optional arguments
    c = TC.Case(entry, **({} if entry == 'bfd_class_extrema3d' else dict(want_waterOut=False)))
    args = list(c.args(0))
    args[-1] = None
    assert getattr(lib, entry)(*args) == 0
