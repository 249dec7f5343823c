"""The call contract of bfd_class_extrema3d and bfd_loss_survey3d without a device: every argument error of include/babelfdtd.h in the header's order,
with nothing written, and -3 where no device is visible (where one is, tests/test_thermal_calls_gpu.py holds a bad ordinal to -3 and the data
refusals to their texts)."""
import os

import numpy as np
import pytest

from babelbrain_amd import ThermalAnalysis as TA, _engine
from tests import thermal_calls as TC


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


def test_abi_symbols_and_version(lib):
    assert lib.bfd_abi_version() == _engine.ABI_VERSION
    for entry in TC.ENTRIES:
        assert entry in _engine.ABI_SYMBOLS and hasattr(lib, entry)


@pytest.mark.parametrize('entry', TC.ENTRIES)
def test_abi_refuses_before_a_device_in_the_header_s_order(lib, entry):
    """-1 with the text of the first fault the header lists, whether or not a device exists, with every output and kernelMs untouched."""
    words = {n: w for n, w, _ in TC.faults(entry)}
    for names, first in TC.ordered_plants(entry):
        c = TC.planted(entry, names)
        assert c.run(lib) == -1, names
        text = lib.bfd_last_error().decode()
        assert text.startswith(entry) and words[first] in text and TA.DATA_REFUSED not in text, (names, first, text)
        assert c.untouched(), names
    for name in TC.required(entry):
        c = TC.Case(entry, **{'want_' + name: False})
        assert c.run(lib) == -1 and 'null' in lib.bfd_last_error().decode() and c.untouched(), name
    for kw in (dict(table_given=False), dict(nMat=0), dict(idBytes=0), dict(idBytes=8)):
        c = TC.Case(entry, **kw)
        assert c.run(lib) == -1 and c.untouched(), (kw, lib.bfd_last_error().decode())


def test_survey_overlaps(lib):
    """waterOut may be pw itself and nothing else: a shifted waterOut, waterOut on p, a sum on the map, two outputs on the same bytes"""
    entry = 'bfd_loss_survey3d'
    c = TC.Case(entry)
    both = np.zeros(c.pw.size + 4, np.float32)
    both[:c.pw.size] = c.pw.ravel()
    c.pw = both[:c.pw.size].reshape(c.pw.shape)
    c.outputs['waterOut'] = both[4:].reshape(c.pw.shape)
    c.pristine = c.snapshot()
    assert c.run(lib) == -1 and 'alias' in lib.bfd_last_error().decode() and c.untouched()
    c = TC.Case(entry)
    c.outputs['waterOut'] = c.p
    c.pristine = c.snapshot()
    assert c.run(lib) == -1 and 'alias' in lib.bfd_last_error().decode() and c.untouched()
    c = TC.Case(entry)
    c.outputs['eTissue'] = np.frombuffer(c.map, np.float64, 18).reshape(2, 9)
    c.pristine = c.snapshot()
    assert c.run(lib) == -1 and 'alias' in lib.bfd_last_error().decode() and c.untouched()
    c = TC.Case(entry)
    c.outputs['eWater'] = c.outputs['eWaterRaw']
    c.pristine = c.snapshot()
    assert c.run(lib) == -1 and 'alias' in lib.bfd_last_error().decode() and c.untouched()
    c = TC.Case(entry)
    c.outputs['waterOut'] = np.frombuffer(np.zeros(c.pw.size * 4, np.uint8), np.float32).reshape(c.pw.shape)
    c.mask = c.outputs['waterOut'].view(np.uint8).reshape(-1)[:c.map.size].reshape(c.N)
    c.pristine = c.snapshot()
    assert c.run(lib) == -1 and 'alias' in lib.bfd_last_error().decode() and c.untouched()


def test_without_a_device_the_call_returns_minus_3(lib):
    if lib.bfd_device_count() > 0:
        for entry in TC.ENTRIES:
            c = TC.Case(entry)
            assert c.run(lib, device=lib.bfd_device_count()) == -3 and c.untouched()
        return
    for entry in TC.ENTRIES:
        for kw in ({}, dict(N=(0, 4, 9)), dict(idBytes=4), dict(nMat=5)):
            c = TC.Case(entry, **kw)
            assert c.run(lib) == -3 and c.untouched(), (entry, kw)
    c = TC.Case('bfd_loss_survey3d')
    c.outputs['waterOut'] = c.pw                                    # in place: no overlap
    c.pristine = c.snapshot()
    assert c.run(lib) == -3 and c.untouched()
    c = TC.Case('bfd_loss_survey3d', want_waterOut=False, mask=np.ones((3, 4, 9), np.uint8))
    assert c.run(lib) == -3 and c.untouched()
