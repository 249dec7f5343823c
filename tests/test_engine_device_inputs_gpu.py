"""The engine setters that take what is on the device already (include/babelfdtd.h: bfd_set_material_map_device, bfd_set_reflector_device,
bfd_set_sensor_box) against the host forms they stand in for, on one small two-medium problem (water and cortical bone, 56 x 52 x 80, 60 steps,
a reflector pocket). The same inputs through either form must give the same run: all 15 fields, the RMS map, the sensor outputs and the tile
counts, element by element (tests/util.py::assert_same)."""
import ctypes as C

import numpy as np
import pytest
import torch

from babelbrain_amd import _engine, harness as H
from babelbrain_amd._engine import FIELD_NAMES, KIND_RMS
from babelbrain_amd.PropagationModel import compact_sources
from tests.util import assert_same, oracle_dt

pytestmark = pytest.mark.gpu

N = (56, 52, 80)
STEPS = 60
ONE = np.array([1.0])


@pytest.fixture(scope='module')
def problem():
    a, k, info = H.make_problem('C2', N=N, steps=STEPS, stable_dt_fn=oracle_dt)
    mm, ml, f, smap, pulse, h, T, sensor = a
    mm = np.ascontiguousarray(np.minimum(mm, 1), np.uint32)              # water and cortical bone
    assert set(np.unique(mm).tolist()) == {0, 1}
    refl = np.zeros(N, np.uint32)
    refl[30:37, 20:29, 40:46] = 1                                        # the pocket
    lin, row = compact_sources(smap, ONE, ONE, ONE)[:2]
    rho_c = ml[0, 0] * ml[0, 1]
    return dict(mm=mm, ml=np.array(ml, np.float64), qc=np.array(k['QCorrection'], np.float64), f=f, h=h, DT=k['DT'], ND=k['NDelta'],
                sub=k['SensorSubSampling'], start=k['SensorStart'], refl=refl, lin=lin, row=row, pulse=np.ascontiguousarray(pulse),
                wz=np.full(len(lin), 1.0 / rho_c, np.float32), sensor=np.ascontiguousarray(sensor), zsrc=info['zsrc'])


def _engine_for(p, sensor_mode=0):
    e = _engine.Engine(*N, len(p['ml']), p['h'], p['DT'], p['f'], STEPS, NDelta=p['ND'], sensorSub=p['sub'], sensorStart=p['start'],
                       selRMSorPeak=1, selMapsRMS=['Pressure'], selMapsSensors=['Pressure'], sensorMode=sensor_mode)
    e.set_materials(p['ml'], p['qc'])
    return e


def _finish(e, p, sensors=True):
    e.set_sources(p['lin'], p['row'], None, None, p['wz'], p['pulse'])
    if sensors:
        e.set_sensor_map(p['sensor'])
    e.run(STEPS)
    e.sync()
    out = {n: e.get_field(n) for n in FIELD_NAMES}
    out['rms'] = e.get_map(KIND_RMS, 'Pressure')
    return out, e.tile_counts()


def _same_run(got, ref, what, p):
    (fg, tg), (fr, tr) = got, ref
    for n in fr:
        assert_same(fg[n], fr[n], '%s: %s' % (what, n), (N, p['ND'], p['mm']))
    assert tg == tr, (what, tg, tr)


def _dev(a):
    """a uint32 numpy array as an int32 tensor on the device (same bits)"""
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to('cuda:0')


@pytest.fixture(scope='module')
def reference(problem):
    """host setters: the map, then the pocket"""
    p = problem
    e = _engine_for(p)
    try:
        e.set_material_map(p['mm'], 0, 0)
        e.set_reflector(p['refl'])
        ref = _finish(e, p)
    finally:
        e.close()
    assert ref[0]['rms'].max() > 0 and ref[1]['solid'] > 0
    return ref


def test_map_and_reflector_from_a_dense_device_tensor(problem, reference):
    p = problem
    e = _engine_for(p)
    try:
        e.set_material_map_device(_dev(p['mm']))
        e.set_reflector_device(_dev(p['refl']))
        got = _finish(e, p)
    finally:
        e.close()
    _same_run(got, reference, 'device setters, C order', p)


def test_a_new_device_map_clears_the_reflector_and_none_clears_it_too(problem):
    p = problem
    runs = []
    for how in ('host', 'remap', 'none'):
        e = _engine_for(p)
        try:
            if how == 'host':
                e.set_material_map(p['mm'], 0, 0)
            else:
                e.set_material_map_device(_dev(p['mm']))
                e.set_reflector_device(_dev(p['refl']))
                if how == 'remap':
                    e.set_material_map_device(_dev(p['mm']))
                else:
                    e.set_reflector_device(None)
            runs.append(_finish(e, p))
        finally:
            e.close()
    _same_run(runs[1], runs[0], 'map set again on the device', p)
    _same_run(runs[2], runs[0], 'reflector cleared through the device form', p)


@pytest.mark.parametrize('ghost', [0, 1, 2])
def test_map_from_a_view_that_is_not_dense_with_ghost_planes(problem, ghost):
    """the same strided view with ghost planes through the host form and through the device form"""
    p = problem
    rng = np.random.default_rng(ghost)
    big = rng.integers(0, 2, (N[0] + 1, 2 * N[1], N[2] + 2 * ghost + 3), dtype=np.uint32)
    view = big[:-1, ::2, 2:2 + N[2] + 2 * ghost]
    view[:, :, ghost:ghost + N[2]] = p['mm']
    assert not view.flags['C_CONTIGUOUS'] and view.shape == (N[0], N[1], N[2] + 2 * ghost)
    dbig = _dev(big)
    dview = dbig[:-1, ::2, 2:2 + N[2] + 2 * ghost]
    assert tuple(dview.stride()) == tuple(s // 4 for s in view.strides)
    runs = []
    for dev in (False, True):
        e = _engine_for(p)
        try:
            if dev:
                e.set_material_map_device(dview, ghost, ghost)
                e.set_reflector_device(_dev(np.broadcast_to(p['refl'][:, :, :, None], N + (2,)).copy())[..., 1])
            else:
                e.set_material_map(view, ghost, ghost)
                e.set_reflector(p['refl'])
            runs.append(_finish(e, p))
        finally:
            e.close()
    _same_run(runs[1], runs[0], 'strided device view, %d ghost plane(s)' % ghost, p)


def test_refusals_leave_the_engine_as_it_was(problem, reference):
    p = problem
    e = _engine_for(p)
    try:
        e.set_material_map_device(_dev(p['mm']))
        e.set_reflector_device(_dev(p['refl']))
        lib, s = e.lib, [N[1] * N[2], N[2], 1]
        bad = p['mm'].copy()
        bad[5, 6, 7] = len(p['ml'])                                     # an id beyond the material list
        with pytest.raises(_engine.EngineError, match=r'rc=-5'):
            e.set_material_map(bad, 0, 0)
        # -5 is found by the kernel that writes the ids, in either form: the map has to be set again after it (and the pocket with it)
        with pytest.raises(_engine.EngineError, match=r'rc=-5'):
            e.set_material_map_device(_dev(bad))
        e.set_material_map_device(_dev(p['mm']))
        e.set_reflector_device(_dev(p['refl']))
        # a host pointer is not read: -1, nothing written
        host = np.ones(N, np.uint32)
        assert lib.bfd_set_material_map_device(e.h, host.ctypes.data_as(C.c_void_p), *s, 0, 0) == -1
        assert 'device memory' in lib.bfd_last_error().decode()
        assert lib.bfd_set_reflector_device(e.h, host.ctypes.data_as(C.c_void_p), *s) == -1
        assert 'device memory' in lib.bfd_last_error().decode()
        # a view that runs past the end of its allocation
        small = torch.zeros(4096, dtype=torch.int32, device='cuda:0')
        assert lib.bfd_set_material_map_device(e.h, C.c_void_p(small.data_ptr()), 2 ** 40, 2 ** 20, 1, 0, 0) == -1
        assert 'device memory' in lib.bfd_last_error().decode()
        assert lib.bfd_set_material_map_device(e.h, None, *s, 0, 0) == -1
        assert lib.bfd_set_material_map_device(e.h, C.c_void_p(_dev(p['mm']).data_ptr()), *s, 3, 0) == -2
        assert lib.bfd_set_material_map_device(e.h, C.c_void_p(_dev(p['mm']).data_ptr()), -s[0], s[1], s[2], 0, 0) == -2
        got = _finish(e, p)
    finally:
        e.close()
    _same_run(got, reference, 'after the refusals', p)


# ---------------------------------------------------------------- sensor boxes ----------------------------------------------------------------

def _boxes(p):
    nd, z = p['ND'], p['zsrc']
    return {'production': ((nd, nd, z + 1), (N[0] - 2 * nd, N[1] - 2 * nd, N[2] - nd - z - 1)),
            'one voxel': ((20, 21, 30), (1, 1, 1)),
            'one plane': ((13, 14, 33), (17, 19, 1)),
            'whole interior': ((nd, nd, nd), (N[0] - 2 * nd, N[1] - 2 * nd, N[2] - 2 * nd))}


def _sensor_outputs(p, mode, box, by_box):
    lo, size = box
    e = _engine_for(p, sensor_mode=mode)
    try:
        e.set_material_map(p['mm'], 0, 0)
        if by_box:
            n = e.set_sensor_box(lo, size)
        else:
            m = np.zeros(N, np.uint32)
            m[lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = 1
            n = e.set_sensor_map(m)
        e.set_sources(p['lin'], p['row'], None, None, p['wz'], p['pulse'])
        e.run(STEPS)
        e.sync()
        out = dict(n=n, num=e.num_sensors, index=e.sensor_index(), steps=e.num_sensor_steps)
        if mode == 0:
            out['series'] = e.sensors()
        F, pk = e.sensor_dft(p['f'])
        out['re'], out['im'], out['peak'] = np.ascontiguousarray(F.real), np.ascontiguousarray(F.imag), pk
    finally:
        e.close()
    return out


@pytest.mark.parametrize('name', ['production', 'one voxel', 'one plane', 'whole interior'])
@pytest.mark.parametrize('mode', [0, 1])
def test_sensor_box_equals_the_sensor_map_of_the_box(problem, name, mode):
    p = problem
    box = _boxes(p)[name]
    if name == 'production':
        m = np.zeros(N, np.uint32)
        m[box[0][0]:box[0][0] + box[1][0], box[0][1]:box[0][1] + box[1][1], box[0][2]:box[0][2] + box[1][2]] = 1
        assert np.array_equal(m, p['sensor'])                           # the box of harness.sensor_maps
    a, b = _sensor_outputs(p, mode, box, True), _sensor_outputs(p, mode, box, False)
    assert a['n'] == b['n'] == a['num'] == b['num'] == int(np.prod(box[1])) and a['steps'] == b['steps'] > 0
    assert a['index'].dtype == b['index'].dtype and np.array_equal(a['index'], b['index'])
    for k in ('series', 're', 'im', 'peak'):
        if k in b:
            assert_same(a[k], b[k], '%s, sensorMode %d: %s' % (name, mode, k))
    assert np.abs(b['peak']).max() > 0 or name == 'one voxel'


def test_sensor_box_refusals(problem):
    p = problem
    e = _engine_for(p)
    try:
        e.set_material_map(p['mm'], 0, 0)
        assert e.set_sensor_box((12, 12, 20), (3, 4, 5)) == 60
        for lo, size in (((12, 12, 20), (3, 0, 5)), ((12, 12, 20), (3, -1, 5)), ((-1, 12, 20), (3, 4, 5)), ((12, 12, 76), (3, 4, 5)),
                         ((56, 0, 0), (1, 1, 1)), ((0, 0, 0), (57, 1, 1))):
            with pytest.raises(_engine.EngineError, match=r'rc=-1'):
                e.set_sensor_box(lo, size)
            assert e.num_sensors == 60
        n = C.c_int64(-7)
        three = np.zeros(3, np.int32)
        assert e.lib.bfd_set_sensor_box(e.h, None, three.ctypes.data_as(C.c_void_p), C.byref(n)) == -1 and n.value == -7
        assert e.lib.bfd_set_sensor_box(e.h, three.ctypes.data_as(C.c_void_p), None, C.byref(n)) == -1 and n.value == -7
        assert e.num_sensors == 60
    finally:
        e.close()
