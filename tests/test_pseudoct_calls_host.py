"""The call contract of the six pseudo-CT entries without a device: every argument error of include/babelfdtd.h in the header's order, with
nothing written, and -3 where no device is visible (where one is, tests/test_pseudoct_calls_gpu.py holds a bad ordinal to -3)."""
import os

import numpy as np
import pytest

from babelbrain_amd import PseudoCT as PC, _engine
from tests import pseudoct_calls as TC


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


def test_abi_symbols_and_version(lib):
    assert lib.bfd_abi_version() == _engine.ABI_VERSION
    for entry in TC.ENTRIES:
        assert entry in _engine.ABI_SYMBOLS and hasattr(lib, entry), entry


@pytest.mark.parametrize('entry', TC.ENTRIES)
def test_abi_refuses_before_a_device_in_the_header_s_order(lib, entry):
    """-1 with the text of the first fault the header lists, whether or not a device exists, with every output and kernelMs untouched."""
    words = {n: w for n, w, _ in TC.faults(entry)}
    for names, first in TC.ordered_plants(entry):
        c = TC.planted(entry, names)
        assert c.run(lib) == -1, names
        text = lib.bfd_last_error().decode()
        assert text.startswith(entry) and words[first] in text and PC.DATA_REFUSED not in text, (names, text)
        assert c.untouched(), names
    for name in TC.REQUIRED[entry]:
        c = TC.Case(entry, **{'want_' + name: False})
        assert c.run(lib) == -1 and 'null' in lib.bfd_last_error().decode() and c.untouched(), name
    nan, inf = float('nan'), float('inf')
    more = {'bfd_integer_histogram3d': (dict(dtype=0), dict(dtype=4)),
            'bfd_order_statistics3d': (dict(R=0), dict(inclusive=-1), dict(ranks=None, quantile=100.5), dict(ranks=None, quantile=-1.0),
                                       dict(ranks=None, quantile=nan)),
            'bfd_uniform_histogram3d': (dict(bins=0), dict(edges=np.full(16, 5.0)), dict(edges=np.r_[np.linspace(0, 1, 15), inf]),
                                        dict(edges=None, want_range=False), dict(edges=None, want_count=False)),
            'bfd_pseudo_ct_candidates3d': (dict(divisor=nan), dict(divisor=inf), dict(lo=nan), dict(eroded=None)),
            'bfd_pseudo_ct_convert3d': (dict(outDtype=0), dict(divisor=0.0), dict(offset=nan), dict(bone=None), dict(skin=None), dict(cavities=None)),
            'bfd_select_component3d': (dict(connectivity=0), dict(tie=-1))}[entry]
    for kw in more:
        c = TC.Case(entry, **kw)
        assert c.run(lib) == -1 and c.untouched(), (kw, lib.bfd_last_error().decode())
    if lib.bfd_device_count() == 0:
        c = TC.Case(entry)
        assert c.run(lib) == -3 and c.untouched()
        # what may be NULL is no argument error
        kw = {'bfd_order_statistics3d': dict(want_ranksUsed=False), 'bfd_uniform_histogram3d': dict(edges=None, want_counts=False),
              'bfd_pseudo_ct_candidates3d': dict(head=None), 'bfd_pseudo_ct_convert3d': dict(head=None)}.get(entry)
        if kw:
            c = TC.Case(entry, **kw)
            assert c.run(lib) == -3 and c.untouched(), kw
