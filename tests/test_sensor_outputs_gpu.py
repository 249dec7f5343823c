"""The sensor side of the engine (bfd_outputs.hip) against the oracle and against itself, on the paths a production call takes:
every one of the eleven sensor quantities as a series, a peak map, an RMS map and a last map, for a box of sensor voxels, the box minus one
voxel (the index list) and a scattered list, with the compact solid state (variant 0) and the full-volume arrays (variant 1); sampling plans
other than the harness's own; more sensors than one launch has threads (grid_for caps a launch at 8192 x 256: the grid-stride loops of
record_sensors, accumulate_sensor_dft, sensor_entries and dft_series run a second time); the in-loop DFT (sensorMode 1) against the DFT of the
stored series -- equal bit for bit, staged, after a reset, after a second sensor map, with quiet runs skipped, in Z-slabs that hold no sensor --
and the stored DFT against tests/dft_reference.py, sensor by sensor."""
import functools

import numpy as np
import pytest

from babelbrain_amd import _engine, harness as H
from babelbrain_amd.PropagationModel import compact_sources
from oracle import oracle as O
from tests.dft_reference import assert_dft
from tests.util import ALL_MAPS, assert_same, compare_runs, geometry_of, oracle_dt

pytestmark = pytest.mark.gpu

QUANTITIES = ALL_MAPS + ['ALLV']            # in the order of their map ids: the order of the sensor block
FREQ = 500e3
ND = 4
RHO_C = 1.5e6
ONE_LAUNCH = 8192 * 256


class Case:
    """One medium with its source, in the form the engine's setters and the oracle's call both take."""

    def __init__(self, N, slab, pocket, patch, nt, sub, start, rows=1):
        M = H.MATERIALS[FREQ]
        self.N, self.nt, self.sub, self.start = N, nt, sub, start
        self.ml = np.array([M['Water'], M['Cortical']], float)
        self.mm = np.zeros(N, np.uint32)
        self.mm[:, :, slab[0]:slab[1]] = 1                      # a skull-like slab across the beam
        self.refl = None
        if pocket is not None:
            self.refl = np.zeros(N, np.uint32)
            self.refl[pocket] = 1
        self.h = H.spatial_step(FREQ, 6)
        self.dt = oracle_dt(self.ml, FREQ, self.h, 0.9)
        self.smap = np.zeros(N, np.uint32)
        for (si, sj, sk) in patch:                              # patches off the centre of the grid: no quantity is zero by symmetry
            ii, jj = np.meshgrid(np.arange(si.start, si.stop), np.arange(sj.start, sj.stop), indexing='ij')
            self.smap[ii, jj, sk] = 1 + (ii // 5 + jj // 3) % rows
        t = 2 * np.pi * FREQ * self.dt * np.arange(nt + 1)
        self.pulse = np.stack([(1.0 + 0.5 * r) * np.sin(t + 0.9 * r) for r in range(rows)])
        self.weights = (np.array([0.0]), np.array([0.0]), np.array([1.0 / RHO_C]))
        self.geometry = (N, ND, self.mm)

    def engine(self, sensor, variant=0, mode=0, maps=('Pressure',), quantities=QUANTITIES, rms_or_peak=1):
        eng = _engine.Engine(*self.N, len(self.ml), self.h, self.dt, FREQ, self.nt, NDelta=ND, sensorSub=self.sub, sensorStart=self.start,
                             selRMSorPeak=rms_or_peak, selMapsRMS=list(maps), selMapsSensors=list(quantities), kernelVariant=variant, sensorMode=mode)
        eng.set_materials(self.ml)
        eng.set_material_map(self.mm, 0, 0)
        if self.refl is not None:
            eng.set_reflector(self.refl)
        eng.set_sources(*compact_sources(self.smap, *self.weights), self.pulse)
        assert eng.set_sensor_map(sensor) == int(sensor.sum())
        return eng

    def oracle(self, sensor, maps=('Pressure',), quantities=QUANTITIES, rms_or_peak=1):
        Ox, Oy, Oz = self.weights
        return O.StaggeredFDTD_3D_with_relaxation(self.mm, self.ml, FREQ, self.smap, self.pulse, self.h, self.nt * self.dt, sensor, Ox=Ox, Oy=Oy, Oz=Oz,
                                                  NDelta=ND, DT=self.dt, SelMapsRMSPeakList=list(maps), SelMapsSensorsList=list(quantities),
                                                  SelRMSorPeak=rms_or_peak, SensorSubSampling=self.sub, SensorStart=self.start, ReflectorMask=self.refl)


# ---- the medium of test_outputs_gpu.py (two tiles in x, a cortical slab at k = 12..19, about three periods of the source) with a reflector pocket
# that holds water cells (k = 10, 11) and bone cells (k = 12, 13), and the source patch moved off the centre
N = (80, 24, 40)
SMALL = Case(N, (12, 20), (slice(30, 36), slice(10, 14), slice(10, 14)), [(slice(20, 50), slice(6, 13), 7)], nt=90, sub=2, start=10)
KINDS = [('rms', _engine.KIND_RMS, 2), ('peak', _engine.KIND_PEAK, 3), ('last', _engine.KIND_LAST, 1)]        # name, kind, slot of the oracle's tuple


def _box():
    s = np.zeros(N, np.uint32)
    s[ND:N[0] - ND, ND:N[1] - ND, 9:N[2] - ND] = 1
    return s


def _box_minus_one_voxel():
    s = _box()
    s[40, 12, 15] = 0
    return s


def _scattered():
    cells = [(1, 2, 3), (78, 22, 38), (2, 12, 20), (40, 1, 15),                      # inside the absorbing layer
             (31, 11, 10), (35, 13, 11), (30, 10, 12), (33, 12, 13),                # reflector cells in water and in bone
             (20, 12, 11), (49, 6, 11), (20, 12, 20),                               # water cells resting on bone, and the one under it
             (20, 12, 12), (20, 12, 19), (49, 6, 12), (49, 6, 19), (36, 9, 12), (36, 9, 19),      # first and last bone cell of a column
             (0, 12, 15), (63, 12, 15), (64, 12, 15), (N[0] - 1, 12, 15), (63, 9, 25), (64, 9, 25), (0, 0, 0),
             (40, 12, 0), (10, 3, 0), (40, 12, N[2] - 1), (70, 20, N[2] - 1), (N[0] - 1, N[1] - 1, N[2] - 1)]      # first and last plane
    s = np.zeros(N, np.uint32)
    for c in cells:
        s[c] = 1
    rng = np.random.default_rng(7)
    s[ND:-ND, ND:-ND, ND:-ND][rng.random((N[0] - 2 * ND, N[1] - 2 * ND, N[2] - 2 * ND)) < 0.004] = 1
    return s


SETS = {'box': _box, 'box minus one voxel': _box_minus_one_voxel, 'scattered list': _scattered}


@functools.lru_cache(maxsize=None)
def _oracle_run(setname):
    return SMALL.oracle(SETS[setname](), maps=QUANTITIES, rms_or_peak=3)


@functools.lru_cache(maxsize=None)
def _device_run(variant, setname, mode):
    """One engine after its run: what it returns, as host arrays the tests only read from."""
    eng = SMALL.engine(SETS[setname](), variant, mode, maps=QUANTITIES, rms_or_peak=3)
    tc = eng.tile_counts()
    if variant == 0:
        assert tc['solid'] > 0, tc
    eng.run(SMALL.nt)
    r = {'index': eng.sensor_index(), 'dft': eng.sensor_dft(FREQ)}
    if mode == 0:
        r['series'] = eng.sensors()
        r['maps'] = {(kn, name): eng.get_map(kind, name) for kn, kind, _ in KINDS for name in QUANTITIES}
    eng.close()
    return r


def _same_dft(got, want, what):
    (F, pk), (F0, pk0) = got, want
    assert F.shape == F0.shape and pk.shape == pk0.shape, what
    for q in range(F.shape[0]):
        for part, x, y in (('re', F[q].real, F0[q].real), ('im', F[q].imag, F0[q].imag), ('peak', pk[q], pk0[q])):
            if not np.array_equal(x, y):
                s = int(np.flatnonzero(x != y)[0])
                raise AssertionError('%s, selected quantity %d: %s differs at %d of %d sensors, first %.9g against %.9g at sensor %d' % (
                    what, q, part, int((x != y).sum()), x.size, float(x[s]), float(y[s]), s))


@pytest.mark.parametrize('setname', list(SETS))
@pytest.mark.parametrize('variant', [0, 1])
def test_every_sensor_quantity_against_the_oracle(variant, setname):
    dev, ora = _device_run(variant, setname, 0), _oracle_run(setname)
    index = ora[-1]['IndexSensorMap']
    assert np.array_equal(dev['index'], index)
    if setname == 'scattered list':
        i, j, k = H.decode_sensor_index(index, N[0], N[1])
        assert {0, 63, 64, N[0] - 1} <= set(i.tolist()) and {0, N[2] - 1} <= set(k.tolist())
        assert SMALL.refl[i, j, k].any() and (SMALL.mm[i, j, k] == 1).any()
    assert dev['series'].shape == (len(QUANTITIES), index.size, 35)
    for q, name in enumerate(QUANTITIES):
        print('variant %d, %s, %s: max |value| %.6g over %d sensors' % (variant, setname, name, np.abs(ora[0][name]).max(), index.size))
        assert np.abs(ora[0][name]).max() > 0, name                     # otherwise the case does not cover this quantity
        assert_same(dev['series'][q], ora[0][name], 'sensor[%s]' % name, SMALL.geometry, (index, N))


@pytest.mark.parametrize('variant', [0, 1])
def test_rms_peak_and_last_map_of_every_quantity_against_the_oracle(variant):
    dev, ora = _device_run(variant, 'box', 0), _oracle_run('box')
    for kn, kind, slot in KINDS:
        for name in QUANTITIES:
            assert np.abs(ora[slot][name]).max() > 0, (kn, name)
            assert_same(dev['maps'][(kn, name)], ora[slot][name], '%s[%s]' % (kn, name), SMALL.geometry)


@pytest.mark.parametrize('setname', list(SETS))
@pytest.mark.parametrize('variant', [0, 1])
def test_stored_dft_within_the_bound_and_the_in_loop_sums_equal_to_it(variant, setname):
    """sensor_dft of the stored engine against the series the same engine returns, sensor by sensor; the sensorMode 1 engine equal to it in re,
    im and peak: the arithmetic is the same sample for sample and the library is built without contraction."""
    stored, lean = _device_run(variant, setname, 0), _device_run(variant, setname, 1)
    F, pk = stored['dft']
    d = SMALL.dt * SMALL.sub
    worst = 0.0
    for q, name in enumerate(QUANTITIES):
        assert np.abs(F[q]).max() > 0, name
        worst = max(worst, assert_dft(F[q], pk[q], stored['series'][q], d, FREQ, 'sensor_dft[%s]' % name, (stored['index'], N)))
    print('variant %d, %s: largest ratio to the bound %.4f' % (variant, setname, worst))
    assert np.array_equal(lean['index'], stored['index'])
    _same_dft(lean['dft'], stored['dft'], 'in-loop against stored')


@pytest.mark.parametrize('variant', [0, 1])
def test_in_loop_mode_staged_reset_and_given_a_new_sensor_map(variant):
    whole, listed = _device_run(variant, 'box', 1), _device_run(variant, 'scattered list', 1)
    eng = SMALL.engine(_box(), variant, 1)
    eng.run(30)
    eng.run(60)
    _same_dft(eng.sensor_dft(FREQ), whole['dft'], 'run(30); run(60) against run(90)')
    eng.reset()
    eng.run(SMALL.nt)
    _same_dft(eng.sensor_dft(FREQ), whole['dft'], 'reset(); run(90)')
    # the series are not there to be had, and the sums belong to one bin
    lib = eng.lib
    out = np.zeros((len(QUANTITIES), eng.num_sensors, eng.num_sensor_steps), np.float32)
    assert lib.bfd_get_sensors(eng.h, _engine._ptr(out)) == -6
    assert lib.bfd_last_error().decode() == 'bfd_get_sensors: the series are not stored with sensorMode 1 (use bfd_get_sensor_dft)'
    assert not out.any()
    F = np.zeros((len(QUANTITIES), eng.num_sensors), np.complex64)
    pk = np.zeros((len(QUANTITIES), eng.num_sensors), np.float32)
    assert lib.bfd_get_sensor_dft(eng.h, 2 * FREQ, _engine._ptr(F.view(np.float32)), _engine._ptr(pk)) == -2
    assert lib.bfd_last_error().decode() == "bfd_get_sensor_dft: with sensorMode 1 the bin is the one of the sim's own frequency"
    assert not F.any() and not pk.any()
    _same_dft(eng.sensor_dft(FREQ), whole['dft'], 'after the refused calls')
    # a second sensor map: sums, peaks and list entries are released and built again
    assert eng.set_sensor_map(_scattered()) == listed['index'].size
    eng.reset()
    eng.run(SMALL.nt)
    assert np.array_equal(eng.sensor_index(), listed['index'])
    _same_dft(eng.sensor_dft(FREQ), listed['dft'], 'set_sensor_map(list) after set_sensor_map(box)')
    eng.close()


# ---- sampling plans other than the harness's own, through the drop-in call (it returns `time`): the smallest grid with a solid layer
PLANS = [(1, 0, 40), (2, 10, 90), (3, 4, 41), (7, 5, 36)]             # (sensorSub, sensorStart, nt); the last one takes exactly one sample


@pytest.mark.parametrize('sub,start,nt', PLANS)
def test_sampling_plans(sub, start, nt):
    from babelbrain_amd import PropagationModel
    Ns = (24, 18, 26)
    c = Case(Ns, (12, 15), None, [(slice(7, 15), slice(6, 11), 6)], nt=nt, sub=sub, start=start)
    sensor = np.zeros(Ns, np.uint32)
    sensor[ND:-ND, ND:-ND, 7:-ND] = 1
    a = (c.mm, c.ml, FREQ, c.smap, c.pulse, c.h, nt * c.dt, sensor)
    k = dict(Ox=c.weights[0], Oy=c.weights[1], Oz=c.weights[2], NDelta=ND, DT=c.dt, SelMapsRMSPeakList=['Pressure', 'Vz'],
             SelMapsSensorsList=['Vy', 'Sigmaxz', 'Pressure', 'ALLV'], SelRMSorPeak=3, SensorSubSampling=sub, SensorStart=start)
    ora = O.StaggeredFDTD_3D_with_relaxation(*a, **k)
    steps = [n for n in range(nt) if n % sub == 0 and n // sub >= start]
    assert len(steps) == {(1, 0, 40): 40, (2, 10, 90): 35, (3, 4, 41): 10, (7, 5, 36): 1}[(sub, start, nt)]
    pm = PropagationModel()
    full = pm.StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, ReturnSensorDFT=True, **k)
    assert np.array_equal(full[0]['time'], np.array(steps) * c.dt)
    compare_runs(full, ora, both=True, geometry=geometry_of(a, k))
    lean = pm.StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, ReturnSensorDFT=True, ReturnSensorSeries=False, **k)
    assert set(lean[0]) == {'time'} and np.array_equal(lean[0]['time'], full[0]['time'])
    index = full[-1]['IndexSensorMap']
    for name in k['SelMapsSensorsList']:
        S = full[0][name]
        assert S.shape == (int(sensor.sum()), len(steps)) and np.abs(S).max() > 0, name
        assert_dft(full[-1]['SensorDFT'][name], full[-1]['SensorPeak'][name], S, c.dt * sub, FREQ, 'SensorDFT[%s]' % name, (index, Ns))
        for key in ('SensorDFT', 'SensorPeak'):
            assert np.array_equal(lean[-1][key][name], full[-1][key][name]), (key, name)


# ---- past one launch: every voxel of 192 x 96 x 128 is a sensor (2 359 296 of them). Sensors are in the order of their x-fastest index, so those
# past the 2 097 152 threads of one launch are the planes from k = 113 on: the bone slab and one source patch lie there, another patch at the near end
BIG_N = (192, 96, 128)
BIG_Q = _engine.ordered(['Pressure', 'Sigmaxy', 'ALLV'])      # the order of the sensor block: by map id
HOLE = (100, 50, 115)                       # a bone voxel past the cap


@functools.lru_cache(maxsize=None)
def _big():
    c = Case(BIG_N, (108, 117), None, [(slice(30, 150), slice(20, 70), 119), (slice(40, 100), slice(30, 60), 7)], nt=24, sub=2, start=2, rows=3)
    sensor = np.ones(BIG_N, np.uint32)
    ora = c.oracle(sensor, quantities=BIG_Q)
    return c, ora


@pytest.mark.parametrize('hole', [False, True])
def test_more_sensors_than_one_launch_has_threads(hole):
    """The box path (every voxel) and the list path (every voxel but one). The oracle ran once, with every voxel: a sensor's series does not
    depend on which other voxels are sensors, so the reference of the list is the same block without the row of the missing voxel."""
    c, ora = _big()
    sensor = np.ones(BIG_N, np.uint32)
    index = ora[-1]['IndexSensorMap']
    want = {name: ora[0][name] for name in BIG_Q}
    if hole:
        sensor[HOLE] = 0
        row = HOLE[0] + BIG_N[0] * (HOLE[1] + BIG_N[1] * HOLE[2])
        assert index[row] == row + 1 and row > ONE_LAUNCH and c.mm[HOLE] == 1
        index = np.delete(index, row)
        want = {name: np.delete(v, row, axis=0) for name, v in want.items()}
    eng = c.engine(sensor, quantities=BIG_Q)
    assert eng.num_sensors == index.size > ONE_LAUNCH                  # the point of the case
    assert eng.tile_counts()['solid'] > 0
    eng.run(c.nt)
    series, dft = eng.sensors(), eng.sensor_dft(FREQ)
    assert np.array_equal(eng.sensor_index(), index)
    eng.close()
    assert series.shape == (3, index.size, 10)
    worst = 0.0
    for q, name in enumerate(BIG_Q):
        assert np.abs(want[name][ONE_LAUNCH:]).max() > 0 and np.abs(want[name][:ONE_LAUNCH]).max() > 0, name
        assert_same(series[q], want[name], 'sensor[%s]' % name, c.geometry, (index, BIG_N))
        worst = max(worst, assert_dft(dft[0][q], dft[1][q], series[q], c.dt * c.sub, FREQ, 'sensor_dft[%s]' % name, (index, BIG_N)))
    print('%d sensors: largest ratio to the bound %.4f' % (index.size, worst))
    lean = c.engine(sensor, mode=1, quantities=BIG_Q)
    lean.run(c.nt)
    got = lean.sensor_dft(FREQ)
    lean.close()
    _same_dft(got, dft, 'in-loop against stored')


# ---- quiet runs: the in-loop sums while runs ahead of the front return at entry (on the grid the front has not crossed when the run ends)
@pytest.mark.parametrize('config', ['C2', 'C3'])
def test_in_loop_dft_with_quiet_runs(config, monkeypatch):
    from tests.test_quiet_runs_gpu import _engine_for, _hip_dt
    Nq, nt = (192, 96, 160), 300
    a, k, info = H.make_problem(config, N=Nq, steps=nt, stable_dt_fn=_hip_dt)
    res = {}
    for skip in ('1', '0'):
        for mode in (0, 1):
            monkeypatch.setenv('BFD_SKIP_ZERO', skip)
            eng = _engine_for(a, k, nt, sensorMode=mode)
            eng.run(nt)
            res[skip, mode] = eng.sensor_dft(info['freq']) + (eng.activity_counts(),)
            if (skip, mode) == ('1', 0):
                series, index = eng.sensors()[0], eng.sensor_index()
            eng.close()
    active, total = res['1', 0][2]
    assert 0 < active < total and res['1', 1][2] == (active, total), (active, total)        # runs really were skipped
    assert res['0', 0][2] == (0, 0) and res['0', 1][2] == (0, 0)
    F, pk = res['1', 0][:2]
    for key in (('1', 1), ('0', 0), ('0', 1)):
        _same_dft(res[key][:2], (F, pk), 'BFD_SKIP_ZERO=%s, sensorMode %d against quiet runs with the stored series' % key)
    assert np.abs(F).max() > 0
    worst = assert_dft(F[0], pk[0], series, k['DT'] * k['SensorSubSampling'], info['freq'], 'sensor_dft[Pressure]', (index, Nq))
    print('%s: %d of %d sub-tiles active, largest ratio to the bound %.4f' % (config, active, total, worst))
    never = ~series.any(axis=1)
    print('%s: %d of %d sensors never reached' % (config, int(never.sum()), never.size))
    assert never.any()
    for key in res:
        assert not res[key][0][0][never].any() and not res[key][1][0][never].any(), key        # F == 0 and peak == 0 exactly


# ---- Z-slabs of which only the middle one holds sensors
@pytest.mark.parametrize('hole', [False, True])
def test_sensor_dft_in_z_slabs_without_sensors(hole):
    from babelbrain_amd import PropagationModel
    Nz = (64, 56, 96)
    a, k, info = H.make_problem('C2', N=Nz, steps=420, stable_dt_fn=oracle_dt)
    k['SelMapsSensorsList'] = ['Pressure', 'Vx', 'Sigmaxz']
    sensor = np.zeros(Nz, np.uint32)
    sensor[12:52, 12:44, 40:56] = 1
    if hole:
        sensor[30, 20, 47] = 0
    a = a[:7] + (sensor,)
    for series in (True, False):
        ref = PropagationModel(device=0).StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, ReturnSensorDFT=True, ReturnSensorSeries=series, **k)
        out = PropagationModel(devices=[0, 0, 0]).StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, ReturnSensorDFT=True, ReturnSensorSeries=series, **k)
        (k0, nk, _), = out[-1]['slabs'][1:2]
        assert len(out[-1]['slabs']) == 3 and k0 <= 40 and 56 <= k0 + nk              # slabs 0 and 2 hold no sensor
        assert np.array_equal(out[-1]['IndexSensorMap'], ref[-1]['IndexSensorMap']) and np.array_equal(out[0]['time'], ref[0]['time'])
        assert set(out[0]) == set(ref[0]) == ({'time'} | set(k['SelMapsSensorsList']) if series else {'time'})
        for name in k['SelMapsSensorsList']:
            if series:
                assert np.array_equal(out[0][name], ref[0][name]), name
            assert np.abs(ref[-1]['SensorDFT'][name]).max() > 0, name
            for key in ('SensorDFT', 'SensorPeak'):
                assert np.array_equal(out[-1][key][name], ref[-1][key][name]), (key, name)
        for q in range(1, len(ref) - 1):
            for name in ref[q]:
                assert np.array_equal(out[q][name], ref[q][name]), (q, name)
        if series:
            first = ref
    for name in k['SelMapsSensorsList']:                                                # and without the series the same numbers
        assert np.array_equal(ref[-1]['SensorDFT'][name], first[-1]['SensorDFT'][name]), name
        assert np.array_equal(ref[-1]['SensorPeak'][name], first[-1]['SensorPeak'][name]), name
