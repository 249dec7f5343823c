"""The new engine entries without a GPU (include/babelfdtd.h: bfd_set_material_map_device, bfd_set_reflector_device, bfd_set_sensor_box,
bfd_pack_results) and the entries of the acoustic study (bfd_acoustic_*). The four engine entries work on a sim, and a sim exists only where a
device does, so what can be held here is the first refusal each header comment lists: a null sim (or spec) is -1 with a text, before anything is
looked at, and nothing the caller passed is written. bfd_acoustic_create checks all its arguments before it looks for a device, so its refusals
are held in the header's order; the other study entries need a handle, and refuse a null one. The refusals that need a live sim or study are in
tests/test_engine_device_inputs_gpu.py, tests/test_pack_results_gpu.py and tests/test_acoustic_study_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

from babelbrain_amd import _engine

ENTRIES = ('bfd_set_material_map_device', 'bfd_set_reflector_device', 'bfd_set_sensor_box', 'bfd_pack_results', 'bfd_acoustic_create',
           'bfd_acoustic_destroy', 'bfd_acoustic_set_volumes', 'bfd_acoustic_survey', 'bfd_acoustic_assemble', 'bfd_acoustic_attach', 'bfd_acoustic_pack',
           'bfd_acoustic_get', 'bfd_acoustic_traffic')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


def test_entries_are_exported_and_bound(lib):
    for entry in ENTRIES:
        assert entry in _engine.ABI_SYMBOLS and hasattr(lib, entry) and getattr(lib, entry).argtypes
    assert lib.bfd_abi_version() == _engine.ABI_VERSION
    assert C.sizeof(_engine.PackSpec) == 4 * 15 + 4 + 16 and _engine.PackSpec.ampScale.offset == 64       # int32 x 15, padding, two doubles


def test_a_null_sim_is_refused_and_nothing_is_written(lib):
    vol = np.full(24, 3, np.uint32)
    keep = vol.copy()
    p = vol.ctypes.data_as(C.c_void_p)
    assert lib.bfd_set_material_map_device(None, p, 6, 3, 1, 0, 0) == -1 and 'null' in lib.bfd_last_error().decode()
    assert lib.bfd_set_reflector_device(None, p, 6, 3, 1) == -1 and 'null' in lib.bfd_last_error().decode()
    lo, size, n = np.zeros(3, np.int32), np.ones(3, np.int32), C.c_int64(-7)
    assert lib.bfd_set_sensor_box(None, lo.ctypes.data_as(C.c_void_p), size.ctypes.data_as(C.c_void_p), C.byref(n)) == -1
    assert 'null' in lib.bfd_last_error().decode() and n.value == -7
    sp = _engine.PackSpec((C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(0, 0, 0), 0, (C.c_int32 * 3)(2, 3, 4), (C.c_int32 * 3)(0, 0, 0), 1, 0, 0.0, 0.0)
    out = [np.full(24 * c, 7.0, np.float32) for c in (1, 2, 1)]
    ms = C.c_float(-5.0)
    assert lib.bfd_pack_results(None, C.byref(sp), *[o.ctypes.data_as(C.c_void_p) for o in out], C.byref(ms)) == -1
    assert 'null' in lib.bfd_last_error().decode() and ms.value == -5.0 and all((o == 7.0).all() for o in out)
    assert np.array_equal(vol, keep)


def test_study_creation_refuses_in_the_header_s_order_before_a_device(lib):
    """bfd_acoustic_create: handle, dimensions, 2^31 voxels, ctBytes, hasAir, air without a ct; then -3 where there is no device"""
    h = C.c_void_p()
    good = dict(M=(8, 9, 10), ctBytes=2, hasAir=1)
    faults = [('M', (8, 0, 10), 'at least 1'), ('M', (2048, 1024, 1024), '2^31'), ('ctBytes', 3, 'ctBytes'), ('hasAir', 2, 'hasAir'), ('ctBytes', 0, 'with a ct')]

    def create(kw, handle=True):
        return lib.bfd_acoustic_create(0, *kw['M'], kw['ctBytes'], kw['hasAir'], C.byref(h) if handle else None), lib.bfd_last_error().decode()

    assert create(good, handle=False)[0] == -1
    for q, (name, value, word) in enumerate(faults):
        kw = dict(good)
        for later, v, _ in faults[q + 1:][::-1]:
            if later != name:
                kw[later] = v
        kw[name] = value
        rc, text = create(kw)
        assert rc == -1 and text.startswith('bfd_acoustic_create: ') and word in text and not h, (name, text)
    if lib.bfd_device_count() == 0:
        assert create(good)[0] == -3 and not h
    # every other entry refuses a null handle first; destroy accepts it
    lib.bfd_acoustic_destroy(None)
    vol = np.zeros(8, np.int64)
    p = vol.ctypes.data_as(C.c_void_p)
    assert lib.bfd_acoustic_set_volumes(None, p, None, None) == -1
    assert lib.bfd_acoustic_survey(None, p, p, 1, p, p, p) == -1
    assert lib.bfd_acoustic_assemble(None, p, p, p, p, 1, p, 0, 0, 1, p, 0, p) == -1
    assert lib.bfd_acoustic_attach(None, None) == -1 and lib.bfd_acoustic_pack(None, None, None, 0) == -1
    assert lib.bfd_acoustic_get(None, 0, 0, p) == -1
    up, down = C.c_int64(-7), C.c_int64(-7)
    assert lib.bfd_acoustic_traffic(None, C.byref(up), C.byref(down)) == -1 and (up.value, down.value) == (-7, -7)
    assert not vol.any()
