"""The result side of the engine (bfd_outputs.hip) on the paths no other test reaches: a caller's `out=` array that is not dense
(bfd_get_map / bfd_get_field through download_volume) and the piece-by-piece readback of the sensor series of a single engine, for a
box of sensor voxels and for an index list. One small grid with two tiles in x and a solid layer, so that the compact solid state
and the single copy of the fluid cells' normal stresses are both in use."""
import numpy as np
import pytest

from babelbrain_amd import _engine, harness as H
from babelbrain_amd.PropagationModel import compact_sources
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

N = (80, 24, 40)            # 64 + 16 columns: two tiles in x; 24 = three tile rows; five sub-tiles of 8 planes
ND = 4
FREQ = 500e3
STEPS = 90                  # about three periods of the source at this grid's time step
SUB, START = 2, 10          # 35 sensor samples, the maps accumulate from step 20
SENTINEL = np.float32(-7.5)


def _medium():
    M = H.MATERIALS[FREQ]
    ml = np.array([M['Water'], M['Cortical']], float)
    mm = np.zeros(N, np.uint32)
    mm[:, :, 12:20] = 1                                     # a skull-like slab across the beam
    return mm, ml


def _engine_with(sensor, sensorMode=0):
    mm, ml = _medium()
    h = H.spatial_step(FREQ, 6)
    dt = _engine.stable_dt(ml, FREQ, True, h, 0.9)
    eng = _engine.Engine(*N, len(ml), h, dt, FREQ, STEPS, NDelta=ND, sensorSub=SUB, sensorStart=START, selRMSorPeak=3,
                         selMapsRMS=['Pressure', 'Sigmaxx'], selMapsSensors=['Pressure', 'Sigmaxy'], sensorMode=sensorMode)
    eng.set_materials(ml)
    eng.set_material_map(mm, 0, 0)
    smap = np.zeros(N, np.uint32)
    smap[24:56, 8:16, 7] = 1                                # a patch, not the whole plane: the slab is hit obliquely too (shear)
    pulse = np.sin(2 * np.pi * FREQ * dt * np.arange(STEPS + 1))[None, :]
    eng.set_sources(*compact_sources(smap, np.array([0.0]), np.array([0.0]), np.array([1.0 / 1.5e6])), pulse)
    assert eng.set_sensor_map(sensor) == int(sensor.sum())
    assert 1.0 / (FREQ * dt) < STEPS                        # the run is longer than one period of the source
    return eng


def _box():
    s = np.zeros(N, np.uint32)
    s[ND:N[0] - ND, ND:N[1] - ND, 9:N[2] - ND] = 1
    return s


def _box_minus_one_voxel():
    s = _box()
    s[40, 12, 15] = 0
    return s


@pytest.fixture(scope='module')
def run():
    """One engine after its run, shared by the tests of this file: they only read from it."""
    eng = _engine_with(_box())
    tc = eng.tile_counts()
    assert tc['solid'] > 0 and tc['lean_fluid'] > 0, tc     # solid runs beside fluid ones
    eng.run(STEPS)
    yield eng
    eng.close()


MAPS = [(_engine.KIND_RMS, 'Pressure'), (_engine.KIND_PEAK, 'Pressure'), (_engine.KIND_LAST, 'Pressure'), (_engine.KIND_LAST, 'Sigmaxx')]
FIELDS = ['Vz', 'Sxx', 'Sxy', 'Rxx', 'Rxy']


def _three_views(fetch):
    """fetch(out) into a C-ordered, a Fortran-ordered and a strided array; the three results and the strided one's parent"""
    c = fetch(np.zeros(N, np.float32))
    f = fetch(np.zeros(N, np.float32, order='F'))
    big = np.full((2 * N[0], N[1], 3 * N[2] + 1), SENTINEL, np.float32)
    view = big[::2, :, 1::3]
    assert view.shape == N and not view.flags['C_CONTIGUOUS'] and not view.flags['F_CONTIGUOUS']
    s = fetch(view)
    return c, f, s, big


def _check_views(c, f, s, big, what):
    print('%s: max |value| %.6g, non-zero cells %d' % (what, np.abs(c).max(), np.count_nonzero(c)))
    assert np.abs(c).max() > 0, what
    assert np.array_equal(c, f), what
    assert np.array_equal(c, s), what
    outside = np.ones(big.shape, bool)
    outside[::2, :, 1::3] = False
    assert np.all(big[outside] == SENTINEL), what           # the gaps of the caller's array are as they were


@pytest.mark.parametrize('kind,name', MAPS)
def test_get_map_into_strided_arrays(run, kind, name):
    c, f, s, big = _three_views(lambda out: run.get_map(kind, name, out=out))
    _check_views(c, f, s, big, 'get_map(%d, %s)' % (kind, name))


@pytest.mark.parametrize('name', FIELDS)
def test_get_field_into_strided_arrays(run, name):
    c, f, s, big = _three_views(lambda out: run.get_field(name, out=out))
    _check_views(c, f, s, big, 'get_field(%s)' % name)


def test_get_map_refuses_before_any_device_work(run):
    """Unselected map, bad kind, bad map id: error -2 and its message; the engine goes on working."""
    lib = run.lib
    out = np.zeros(N, np.float32)

    def call(kind, mapid):
        rc = lib.bfd_get_map(run.h, kind, mapid, _engine._ptr(out), *_engine._estrides(out))
        return rc, lib.bfd_last_error().decode()
    assert call(_engine.KIND_RMS, _engine.MAP_BITS['Vz']) == (-2, 'bfd_get_map: map was not selected in selMapsRMS')
    assert call(_engine.KIND_PEAK, _engine.MAP_BITS['Vz']) == (-2, 'bfd_get_map: map was not selected in selMapsRMS')
    assert call(7, _engine.MAP_BITS['Pressure']) == (-2, 'bfd_get_map: bad kind')
    assert call(_engine.KIND_LAST, 11) == (-2, 'bfd_get_map: bad map id')
    assert call(_engine.KIND_LAST, -1) == (-2, 'bfd_get_map: bad map id')
    assert not out.any()
    assert np.abs(run.get_map(_engine.KIND_RMS, 'Pressure')).max() > 0


def _pieces(monkeypatch, threads):
    monkeypatch.setenv('BFD_D2H_MIN_MB', '1')
    monkeypatch.setenv('BFD_D2H_PIECE_KB', '256')
    monkeypatch.setenv('BFD_D2H_THREADS', threads)


@pytest.mark.parametrize('sensor', [_box, _box_minus_one_voxel])
def test_sensor_series_piece_by_piece_equal_the_one_copy(run, monkeypatch, sensor):
    """sensors() through four host threads and 256 KB pieces (the producer path: no scratch block) against BFD_D2H_THREADS=0 (declined:
    one transposed scratch block, one copy); a box of voxels needs no index list on the device, the box minus one voxel does."""
    eng = run if sensor is _box else _engine_with(sensor())
    if eng is not run:
        eng.run(STEPS)
    _pieces(monkeypatch, '4')
    got = eng.sensors()
    assert got.nbytes > 4 * (1 << 20) and got.shape[0] == 2          # several pieces for each of the four threads
    _pieces(monkeypatch, '0')
    want = eng.sensors()
    if eng is not run:
        eng.close()
    for q, name in enumerate(('Pressure', 'Sigmaxy')):
        print('%s, %s: max |value| %.6g' % (sensor.__name__, name, np.abs(want[q]).max()))
        assert np.abs(want[q]).max() > 0, name
    assert np.array_equal(got, want)


def test_sensor_dft_of_stored_series_equals_the_in_loop_sums(run, monkeypatch):
    """sensor_dft() from the stored series (sensorMode 0) against the sums kept while the samples are taken (sensorMode 1): equal, as in
    test_dft_gpu.py (the arithmetic is the same sample for sample), here on a grid with a solid layer. The readback settings are those of the
    test above; bfd_get_sensor_dft moves two small blocks with plain copies and does not go through the piece-by-piece path."""
    _pieces(monkeypatch, '4')
    F0, pk0 = run.sensor_dft(FREQ)
    lean = _engine_with(_box(), sensorMode=1)
    lean.run(STEPS)
    F1, pk1 = lean.sensor_dft(FREQ)
    lean.close()
    for q, name in enumerate(('Pressure', 'Sigmaxy')):
        er, ei = rel_l2(F0[q].real, F1[q].real), rel_l2(F0[q].imag, F1[q].imag)
        print('%s: max |F| %.6g, rel L2 re %.3g im %.3g' % (name, np.abs(F1[q]).max(), er, ei))
        assert np.abs(F1[q]).max() > 0
        assert np.array_equal(F0[q].real, F1[q].real) and np.array_equal(F0[q].imag, F1[q].imag)
        assert np.array_equal(pk0[q], pk1[q])
