"""Material lists of more than 256 rows in the bio-heat solver, host side: the limit, the C ABI and the map RayleighAndBHTE._bhte_inputs
builds. A CT-derived plan indexes up to 1030 rows (3 or 6 soft tissues + 2^10 bone bins); the id width must follow from the length of
the list (uint8 up to 256 rows, uint16 above), never from a cast that could wrap an id. No device is needed."""
import ctypes as C

import numpy as np
import pytest


def _list(n):
    r = np.arange(n, dtype=np.float64)
    return {'Density': 1000.0 + r, 'SoS': 1500.0 + r, 'Attenuation': 1.0 + 0.1 * r, 'SpecificHeat': 3000.0 + r, 'Conductivity': np.full(n, 0.5),
            'Perfusion': 10.0 + r, 'Absorption': np.full(n, 0.5), 'InitTemperature': np.full(n, 37.0)}


def _inputs(n, mm):
    from babelbrain_amd import RayleighAndBHTE as R
    p = np.ones((1,) + mm.shape, np.float32)
    return R._bhte_inputs(p, mm, _list(n), 4e-4, 0.02, 1050, 3617, 1.0, None, None, None)


def _lib():
    from babelbrain_amd import _engine
    return _engine.load_library()


def test_limit_and_exports():
    from babelbrain_amd import _engine
    lib = _lib()
    assert lib.bfd_bhte_max_materials() >= 1030
    assert lib.bfd_abi_version() == _engine.ABI_VERSION
    for name in ('bfd_bhte_max_materials', 'bfd_bhte_run_volumes16', 'bfd_bhte_run_protocol16'):
        assert hasattr(lib, name), name
    assert {'bfd_bhte_max_materials', 'bfd_bhte_run_volumes16', 'bfd_bhte_run_protocol16'} <= set(_engine.ABI_SYMBOLS)


@pytest.mark.parametrize('n,dtype', [(5, np.uint8), (256, np.uint8), (257, np.uint16), (1030, np.uint16)])
def test_id_width_follows_the_list_length(n, dtype):
    mm = (np.arange(4 * 5 * 6, dtype=np.int64).reshape(4, 5, 6) * 37) % n
    mm[0, 0, 0] = n - 1                                   # the highest id survives whatever the width
    v = _inputs(n, mm)
    assert v['mat'].dtype == dtype and v['mat'].flags['C_CONTIGUOUS'] and v['nMat'] == n
    assert v['wide'] == (n > 256)
    assert np.array_equal(v['mat'].astype(np.int64), mm)  # nothing wrapped
    assert len(v['cd']) == len(v['cp']) == len(v['qf']) == len(v['initT']) == n


def test_a_wider_input_map_does_not_widen_the_ids():
    """the dtype the caller's map happens to have decides nothing: five materials in an int64 or uint16 map are 8-bit ids"""
    for dt in (np.int64, np.uint16, np.uint8, np.float64):
        v = _inputs(5, np.full((3, 3, 3), 4, dt))
        assert v['mat'].dtype == np.uint8 and not v['wide']


def test_more_materials_than_the_limit_are_refused():
    limit = _lib().bfd_bhte_max_materials()
    with pytest.raises(ValueError, match=str(limit)):
        _inputs(limit + 1, np.zeros((3, 3, 3), np.int64))
    v = _inputs(limit, np.full((3, 3, 3), limit - 1, np.int64))
    assert v['mat'].dtype == np.uint16 and int(v['mat'].max()) == limit - 1


@pytest.mark.parametrize('n', [5, 256, 257, 1030])
def test_an_id_equal_to_the_list_length_is_refused(n):
    limit = _lib().bfd_bhte_max_materials()
    mm = np.zeros((3, 3, 3), np.int64)
    mm[1, 2, 0] = n
    with pytest.raises(ValueError, match=str(limit)):
        _inputs(n, mm)
    mm[1, 2, 0] = -1
    with pytest.raises(ValueError):
        _inputs(n, mm)
