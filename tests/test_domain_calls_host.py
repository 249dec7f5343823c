"""The call contract of the three domain entries (csrc/bfd_call.h) without a GPU: the C ABI refuses bad arguments before it looks for a device, in
the header's order, and writes nothing; without a device a good call returns -3 and writes nothing."""
import os

import pytest

from babelbrain_amd import _engine
from tests import domain_calls as DC


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


@pytest.mark.parametrize('entry', DC.ENTRIES)
def test_abi_refuses_before_a_device_in_the_header_s_order(lib, entry):
    """-1 with the text of the first fault the header lists, whether or not a device exists, with every output and kernelMs untouched."""
    assert entry in _engine.ABI_SYMBOLS and hasattr(lib, entry) and lib.bfd_abi_version() == _engine.ABI_VERSION
    words = {n: w for n, w, _ in DC.faults(entry)}
    for names, first in DC.ordered_plants(entry):
        c = DC.planted(entry, names)
        assert c.run(lib) == -1, names
        text = lib.bfd_last_error().decode()
        assert text.startswith(entry + ': ') and words[first] in text, (names, text)
        assert c.untouched(), names
    nulls = {'bfd_label_survey3d': ('labels', 'lo', 'hi'), 'bfd_assemble_material_map3d': ('labels', 'lo', 'size', 'padLo', 'padHi', 'focalIJ'),
             'bfd_sdr_rays3d': ('hu', 'lo', 'size')}[entry]
    for name in nulls:
        c = DC.Case(entry, **{name: None})
        assert c.run(lib) == -1 and 'null' in lib.bfd_last_error().decode() and c.untouched(), name
    required = {'bfd_label_survey3d': ('hist', 'bounds', 'focal'), 'bfd_assemble_material_map3d': ('map', 'stats'),
                'bfd_sdr_rays3d': ('value', 'count', 'state')}[entry]
    for name in required:
        c = DC.Case(entry, **{'want_' + name: False})
        assert c.run(lib) == -1 and 'null' in lib.bfd_last_error().decode() and c.untouched(), name
    more = {'bfd_label_survey3d': (dict(lo=DC.i64([0, 2, 9])), dict(lo=DC.i64([-1, 0, 0])), dict(flipK=-1)),
            'bfd_assemble_material_map3d': (dict(ctBytes=0), dict(ct=None), dict(size=DC.i64([3, -1, 6])), dict(padLo=DC.i64([2 ** 31, 0, 0])),
                                            dict(nMaterials=-1), dict(focalIJ=DC.i64([0, -1])), dict(focalIJ=DC.i64([0, 5]))),
            'bfd_sdr_rays3d': (dict(ctBytes=0), dict(lo=DC.i64([0, 0, 10])), dict(huBytes=16), dict(nHU=2 ** 31), dict(stepI=0), dict(stepI=2 ** 31),
                               dict(minSkull=2 ** 31), dict(centerRegion=float('nan')), dict(centerRegion=float('inf')))}[entry]
    for kw in more:
        c = DC.Case(entry, **kw)
        assert c.run(lib) == -1 and c.untouched(), kw
    if lib.bfd_device_count() == 0:
        c = DC.Case(entry)
        assert c.run(lib) == -3 and c.untouched()
        if entry == 'bfd_assemble_material_map3d':              # the nullable inputs and outputs are no argument error
            no_bone = DC.Case(entry).lut & 0x7FFFFFFF
            c = DC.Case(entry, ct=None, ctBytes=0, air=None, lut=no_bone, want_mapNoCT=False, want_airOut=False)
            assert c.run(lib) == -3 and c.untouched()
