"""The thermal study on the device (babelbrain_amd.ThermalStudy, bfd_thermal_* in csrc/bfd_thermal_study.hip) against today's separate public calls
on the same inputs, element by element (tests.util.assert_same): every stage, the arithmetic the study adds against numpy, the whole flow against
tests/thermal_study_flow.flow_by_calls, residency as byte counts, and the lifetime of a handle. Shapes are the smallest at which the kernels can go
wrong: (3, 3, 3) is the solver's minimum and no multiple of 4; (5, 30, 67) crosses a 64-lane tile on the fastest axis and the 20-row interior of
the four-step kernel's regions on the middle one; (24, 22, 40) is the oracle's default; (9, 7, 130); (109, 130, 148) is 8 voxels more than one sweep
of a 2048 x 256 grid of quads."""
import functools

import numpy as np
import pytest

from babelbrain_amd import _engine
from tests import thermal_study_flow as F
from tests.util import assert_same

pytestmark = pytest.mark.gpu

SHAPES = [(3, 3, 3), (5, 30, 67), (24, 22, 40), (9, 7, 130)]
SWEEP_SHAPE = (109, 130, 148)
assert np.prod(SWEEP_SHAPE) == 2048 * 256 * 4 + 8


@functools.lru_cache(maxsize=None)
def case_of(shape, wide=False, fields=1, **kw):
    """a case (shared, never written) with 5 materials, or 300 behind a CT map"""
    build = dict(ct=True, n_ct=297) if wide else {}
    build.update(kw)
    c = F.make_case(shape, seed=sum(shape), fields=fields, **build)
    assert c['nMat'] == (300 if wide else c['nMat'])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def tables_of(c):
    from babelbrain_amd import ThermalAnalysis as TA
    bench = c['benchmark']
    if bench is not None and bench['TestType'] == 3:
        bench = dict(bench, maxMaterial=int(c['MaterialMap'].max()))
    return TA.region_tables(c['nMat'], 'MaterialMapCT' in c['Input'], c['bSegmentedBrain'], c['bForceHomogenousMedium'], bench)


def study_of(c):
    from babelbrain_amd.ThermalStudy import ThermalStudy
    return ThermalStudy(c['pAmp'], c['pAmpWater'], c['MaterialMap'], c['MaterialList'], c['Input']['x_vec'][1] - c['Input']['x_vec'][0])


def points_map(c):
    shape = c['MaterialMap'].shape
    mpm = np.zeros(shape, np.uint32)
    mpm[shape[0] // 2, shape[1] // 2, shape[2] // 2] = 2
    mpm[0, 0, 0] = 3
    mpm[shape[0] - 1, shape[1] - 1, shape[2] - 1] = 1
    mpm[1, 1, 1] = 4
    return mpm


def equal_dicts(got, ref, what):
    assert set(got) == set(ref)
    for k in ref:
        F.same(got[k], ref[k], '%s[%s]' % (what, k))


# ---------------------------------------------------------------- per stage ----------------------------------------------------------------

@pytest.mark.parametrize('wide', [False, True], ids=['nMat5', 'nMat300'])
@pytest.mark.parametrize('shape', SHAPES + [SWEEP_SHAPE], ids=lambda s: 'x'.join(map(str, s)))
def test_every_stage_equals_the_public_call_one_field(shape, wide):
    from babelbrain_amd import MedianFilter as MF, RayleighAndBHTE as R, ThermalAnalysis as TA
    c = case_of(shape, wide)
    big = shape == SWEEP_SHAPE
    tab = tables_of(c)
    classOf, BrainID = tab['classOf'], tab['BrainID']
    mm, ML = c['MaterialMap'], c['MaterialList']
    dx, dt = c['Input']['x_vec'][1] - c['Input']['x_vec'][0], c['dt']
    SelSkull = ((classOf[mm] >> TA.BIT_SKULL) & 1).astype(bool)
    mpm = points_map(c)
    with study_of(c) as st:
        assert st._lib.bfd_bhte_max_materials() >= 300
        # the median merged under the skull
        st.median_in_region(classOf)
        p = MF.median_in_region(c['pAmp'], SelSkull, 3)
        assert_same(st.fetch('p'), p, 'median in region')
        if SelSkull.any() and not big:
            assert not np.array_equal(p, c['pAmp'])
        # the survey: every output and the cleared water field
        water = c['pAmpWater'].copy()
        ref = TA.loss_survey(p, water, mm, classOf, ML['Density'], ML['SoS'], ML['Density'][0], ML['SoS'][0], dx ** 2, waterOut=water)
        got = st.loss_survey(classOf, ML['Density'][0], ML['SoS'][0], dx ** 2)
        for k in ref:
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
        assert_same(st.fetch('pw'), water, 'cleared water field')
        # the first bio-heat call on the scaled pressure
        ratio = np.float64(1.5596243) * np.float64(2.5e5) / max(np.float64(p.max()), 1.0)
        scaled = p * ratio
        assert scaled.dtype == np.float64
        st.scale(ratio)
        nSteps, nOn = (9, 6) if big else (23, 15)
        T, D, _, Q, pts = R.BHTE(scaled, mm, ML, dx, nSteps, nOn, -1, dt=dt, DutyCycle=0.3, MonitoringPointsMap=mpm, stableTemp=37.0)
        gpts = st.bhte(nSteps, nOn, dt=dt, DutyCycle=0.3, MonitoringPointsMap=mpm, stableTemp=37.0)
        assert_same(st.fetch('q'), Q, 'Qarr')
        assert_same(st.fetch('T'), T, 'ResTemp')
        assert_same(st.fetch('Tmax'), T, 'Tmax without captures')
        assert_same(st.fetch('dose'), D, 'ResDose')
        assert_same(gpts, pts, 'point series of BHTE')
        assert float(T.max()) > 37.0 or shape == (3, 3, 3)          # one interior voxel there, in water
        # the new arithmetic against numpy
        assert_same(st.fetch('p_map'), scaled.astype(np.float32), 'p_map float32')
        wide64 = st.fetch('p_map', np.float64)
        assert wide64.dtype == np.float64 and np.array_equal(wide64, scaled)
        cy = shape[1] // 2
        assert_same(st.fetch_plane('p_map', cy), (p[:, cy, :] * ratio).astype(np.float32), 'p_map_central')
        assert_same(st.fetch_plane('p', cy), p[:, cy, :], 'central plane of p')
        plane = st.fetch_plane('MaterialMap', cy)
        assert plane.dtype == mm.dtype and np.array_equal(plane, mm[:, cy, :])
        # extrema and the hottest points
        p32 = scaled.astype(np.float32)
        ref = TA.tissue_extrema([T, D, p32, p], mm, classOf)
        got = st.tissue_extrema(['T', 'dose', 'p_map', 'p'], classOf)
        for k in ref:
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
        for a, b in zip(st.hottest_points(classOf), TA.hottest_points(T, mm, classOf)):
            assert np.array_equal(a, b)
        # the protocol: two groups of two repetitions, an off period and a pause
        plan = (2, 2, 1, 2, 100) if big else (2, 4, 3, 5, 100)
        rep, total, pause, off, limit = plan
        nOnSteps, nHeat = (4, 3) if big else (9, 6)
        ref = R.RunBHTECycles(0, rep, total, pause, off, limit, 'file', scaled, mm, ML, dx, nOnSteps, nHeat, -1, 1, dt, 0.3, 'HIP', mpm, 37.0, None, None, None, None)
        gpts, nNext = st.run_cycles(0, rep, total, pause, off, limit, nOnSteps, nHeat, 1, dt, 0.3, mpm, 37.0)
        assert nNext == ref[5]
        for name, r in zip(('Tmax', 'doseAtCapture', 'T', 'dose'), ref[:4]):
            assert_same(st.fetch(name), r, 'RunBHTECycles ' + name)
        assert_same(gpts, ref[4], 'point series of RunBHTECycles')
        # the metrics
        args = (ML, BrainID, 500e3, 0.3, 5.0)
        try:
            want = TA.exposure_metrics(ref[0], ref[3], (p, ratio), mm, classOf, *args)
        except ValueError as e:
            with pytest.raises(ValueError, match='class is empty'):
                st.exposure_metrics(classOf, BrainID, *args[2:])
            assert 'class is empty' in str(e) and shape == (3, 3, 3)
        else:
            equal_dicts(st.exposure_metrics(classOf, BrainID, *args[2:]), want, 'exposure_metrics')


@pytest.mark.parametrize('wide', [False, True], ids=['nMat5', 'nMat300'])
@pytest.mark.parametrize('shape', [(3, 3, 3), (5, 30, 67), (9, 7, 130)], ids=lambda s: 'x'.join(map(str, s)))
def test_every_stage_equals_the_public_call_three_fields(shape, wide):
    from babelbrain_amd import MedianFilter as MF, RayleighAndBHTE as R, ThermalAnalysis as TA
    c = case_of(shape, wide, fields=3)
    classOf = tables_of(c)['classOf']
    mm, ML = c['MaterialMap'], c['MaterialList']
    dx, dt = c['Input']['x_vec'][1] - c['Input']['x_vec'][0], c['dt']
    SelSkull = ((classOf[mm] >> TA.BIT_SKULL) & 1).astype(bool)
    mpm = points_map(c)
    with study_of(c) as st:
        st.median_in_region(classOf)                      # the reference filters the WATER fields here (:915-918)
        water = MF.median_in_region(c['pAmpWater'], SelSkull, 3)
        assert_same(st.fetch('pw'), water, 'median in region, water fields')
        assert_same(st.fetch('p'), c['pAmp'], 'tissue fields untouched')
        water = water.copy()
        ref = TA.loss_survey(c['pAmp'], water, mm, classOf, ML['Density'], ML['SoS'], ML['Density'][0], ML['SoS'][0], dx ** 2, waterOut=water)
        got = st.loss_survey(classOf, ML['Density'][0], ML['SoS'][0], dx ** 2)
        for k in ref:
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
        assert_same(st.fetch('pw'), water, 'cleared water fields')
        ratio = np.array([1.1, 0.9, 1.3], np.float32) * np.float32(2.5e5 / max(float(c['pAmp'].max()), 1.0))
        scaled = c['pAmp'].copy()
        for n in range(3):
            scaled[n, :, :, :] *= ratio[n]
        st.scale(ratio)
        oo = np.array([[3, 1], [2, 2], [4, 0]])
        T, D, _, Q, pts = R.BHTEMultiplePressureFields(scaled, mm, ML, dx, 25, oo, -1, dt=dt, MonitoringPointsMap=mpm, stableTemp=37.0)
        gpts = st.bhte(25, oo, dt=dt, MonitoringPointsMap=mpm, stableTemp=37.0)
        assert_same(st.fetch('q'), Q, 'Qarr')
        assert_same(st.fetch('T'), T, 'ResTemp')
        assert_same(st.fetch('dose'), D, 'ResDose')
        assert_same(gpts, pts, 'point series')
        pmap = scaled.max(axis=0)
        assert_same(st.fetch('p_map'), pmap, 'p_map of three fields')
        cy = shape[1] - 1
        assert_same(st.fetch_plane('p_map', cy), pmap[:, cy, :], 'p_map_central')
        ref = TA.tissue_extrema([pmap, T], mm, classOf)
        got = st.tissue_extrema(['p_map', 'T'], classOf)
        for k in ref:
            assert np.array_equal(got[k], ref[k]), k
        ref = R.RunBHTECycles(0, 2, 4, 3, 2, 100, ['a', 'b', 'c'], scaled, mm, ML, dx, 8, oo, -1, 1, dt, 1.0, 'HIP', mpm, 37.0, None, None, None, None)
        gpts, nNext = st.run_cycles(0, 2, 4, 3, 2, 100, 8, oo, 1, dt, 1.0, mpm, 37.0)
        for name, r in zip(('Tmax', 'doseAtCapture', 'T', 'dose'), ref[:4]):
            assert_same(st.fetch(name), r, 'RunBHTECycles ' + name)
        assert_same(gpts, ref[4], 'point series of RunBHTECycles')


def test_merge_with_a_previous_temperature():
    c = case_of((5, 30, 67))
    rng = np.random.default_rng(8)
    prev = (37.0 + rng.uniform(0, 0.02, c['MaterialMap'].shape)).astype(np.float32)
    with study_of(c) as st:
        st.scale(1.25)
        st.bhte(6, 4, dt=c['dt'], DutyCycle=0.3)
        T = st.fetch('Tmax')
        st.merge_previous(prev)
        assert_same(st.fetch('Tmax'), np.maximum(T, prev), 'np.maximum with TempEndFUS')
        assert (prev > T).any() and (prev < T).any()
        assert_same(st.fetch('T'), T, 'T is left alone')
        # the same from volumes held on the device: uploaded once, used by both runs and both merges
        with pytest.raises(_engine.EngineError, match='rc=-6'):
            st.merge_previous(None, 'dose')
        previous = dict(FinalTemp=prev, FinalDose=(prev - np.float32(37.0)), TempEndFUS=prev + np.float32(0.01))
        up = st.traffic()[0]
        st.set_previous(previous)
        assert st.traffic()[0] == up + 3 * prev.nbytes
        st.bhte(0, 0, dt=c['dt'], DutyCycle=0.3, PreviousData=previous)
        assert_same(st.fetch('T'), prev, 'start from FinalTemp')
        assert_same(st.fetch('dose'), previous['FinalDose'], 'start from FinalDose')
        st.merge_previous()
        assert_same(st.fetch('Tmax'), previous['TempEndFUS'], 'merged with the TempEndFUS held')
        assert st.traffic()[0] < up + 3 * prev.nbytes + 1024


# ---------------------------------------------------------------- the whole flow ----------------------------------------------------------------

FLOWS = {
    'plain': dict(shape=(24, 22, 40)),
    'plain, previous data': dict(shape=(5, 30, 67), previous=True),
    'three fields': dict(shape=(9, 7, 130), fields=3),
    'three fields, previous data': dict(shape=(24, 22, 40), fields=3, previous=True),
    'ct, 300 materials': dict(shape=(5, 30, 67), ct=True, n_ct=297),
    'segmented': dict(shape=(24, 22, 40), segmented=True),
    'segmented ct': dict(shape=(9, 7, 130), ct=True, segmented=True, n_ct=20),
    'benchmark 3': dict(shape=(24, 22, 40), benchmark=dict(TestType=3, nMaterials=6)),
    'homogeneous': dict(shape=(9, 7, 130), homogeneous=True),
    'resumed in chunks': dict(shape=(5, 30, 67), limit=3),
    'resumed in chunks, three fields, previous data': dict(shape=(9, 7, 130), fields=3, previous=True, limit=2),
}


@pytest.mark.parametrize('name', sorted(FLOWS))
def test_thermal_exposure_equals_the_flow_by_calls(name):
    from babelbrain_amd.ThermalStudy import thermal_exposure
    kw = dict(FLOWS[name])
    c = F.make_case(kw.pop('shape'), seed=len(name), **kw)
    ref = F.flow_by_calls(c)
    args, kwargs = F.exposure_arguments(c)
    got = thermal_exposure(*args, keep=F.VOLUMES, **kwargs)
    for k in F.SMALL + F.VOLUMES:
        F.same(got[k], ref[k], '%s: %s' % (name, k))
    if 'chunks' in name:
        assert c['NumberGroupedSonications'] * c['Repetitions'] > c['LimitBHTEIterationsPerProcess']           # nCurrent > 0 was resumed in a second call
    assert float(np.max(ref['TempEndFUS'])) > 37.0 and ref['TemperaturePoints'].shape[1] > 20


# ---------------------------------------------------------------- residency ----------------------------------------------------------------

def expected_traffic(c, nPoints, protocolSteps, firstSteps):
    """bytes up and down of thermal_exposure with nothing fetched, from the shapes: what is copied and why"""
    n = int(np.prod(c['MaterialMap'].shape))
    N1, N2, N3 = c['MaterialMap'].shape
    nF, nMat = c['fields'], c['nMat']
    extrema_words = (4 + 1) * 8 * 8 + (8 + 1) * 4            # start values up and results down of one extrema launch (csrc/bfd_thermal.hip)
    up = 2 * nF * n * 4 + n * c['MaterialMap'].dtype.itemsize          # p, pw and the map as passed: once
    down = 4                                                  # the range check of the ids
    bNormal = not c['bForceHomogenousMedium'] and c['benchmark'] is None
    if bNormal:
        up += nMat                                            # class table of the median
    up += nMat + 2 * 8 * nMat                                 # survey: class table, rho, c
    down += nF * (3 * N3 * 8 + 16) + 4                        # survey: three sums per plane and two maxima per field, the flags
    up += 8 * nF                                              # the ratios
    runs = 2
    up += runs * 4 * 4 * nMat                                 # cd, cp, qf, initT per run
    prev = c['PreviousData'] is not None
    if prev:
        up += 3 * n * 4 - runs * 4 * nMat                     # FinalTemp, FinalDose and TempEndFUS, each ONCE (initT is then not needed)
    up += nPoints * 4                                         # the point list of the protocol
    down += nPoints * protocolSteps * 4                       # its point series
    launches = 1 + 1                                          # hottest points; the metrics (three volumes: one launch)
    up += launches * (nMat + extrema_words)
    down += launches * extrema_words
    down += 2 * N1 * N3 * 4                                   # the two central planes
    return up, down


@pytest.mark.parametrize('name', ['plain', 'plain, previous data', 'three fields', 'ct, 300 materials'])
def test_nothing_travels_that_was_not_asked_for(name):
    from babelbrain_amd.ThermalStudy import thermal_exposure
    kw = dict(FLOWS[name])
    c = F.make_case(kw.pop('shape'), seed=len(name), **kw)
    args, kwargs = F.exposure_arguments(c)
    S = thermal_exposure(*args, return_study=True, **kwargs)
    with S['study'] as st:
        pts = S['TemperaturePoints'] if c['PreviousData'] is None else S['TemperaturePoints'][:, 5:]
        up, down = expected_traffic(c, pts.shape[0], pts.shape[1], None)
        assert st.traffic() == (up, down) == S['traffic']
        n = int(np.prod(c['MaterialMap'].shape))
        volumes_up = 2 * c['fields'] * n * 4 + n * c['MaterialMap'].dtype.itemsize + (3 * n * 4 if c['PreviousData'] is not None else 0)
        assert 0 < up - volumes_up < n * 4 and down < n * 4          # the inputs (and PreviousData's volumes) and not one volume more; no volume came down
        for k, (vol, dtype) in enumerate((('Tmax', None), ('doseAtCapture', None), ('T', None), ('dose', None), ('p_map', None), ('q', None))):
            before = st.traffic()
            a = st.fetch(vol, dtype)
            assert st.traffic() == (before[0], before[1] + a.nbytes), vol
        if c['fields'] == 1:
            before = st.traffic()
            a = st.fetch('p_map', np.float64)
            assert a.nbytes == 8 * n and st.traffic() == (before[0], before[1] + a.nbytes)


# ---------------------------------------------------------------- lifetime ----------------------------------------------------------------

def run_once(st, c, ratio):
    st.scale(ratio)
    pts = st.bhte(12, 8, dt=c['dt'], DutyCycle=0.3, MonitoringPointsMap=points_map(c))
    return [st.fetch(k) for k in ('T', 'dose', 'q', 'p_map')] + [pts]


def test_two_studies_at_once_reuse_and_repeats():
    a, b = case_of((5, 30, 67)), case_of((9, 7, 130), True)
    with study_of(a) as sa:
        alone_a = run_once(sa, a, 1.3)
    with study_of(b) as sb:
        alone_b = run_once(sb, b, 0.8)
    with study_of(a) as sa, study_of(b) as sb:              # both alive on one device, their calls interleaved
        sa.scale(1.3)
        sb.scale(0.8)
        both_b = run_once(sb, b, 0.8)
        both_a = run_once(sa, a, 1.3)
        for x, y in zip(both_a + both_b, alone_a + alone_b):
            assert x.tobytes() == y.tobytes()               # the same bytes, also in repeats
        # reuse: a second scale and run on the same handle start over
        again = run_once(sa, a, 0.7)
        assert not np.array_equal(again[0], both_a[0])
        with study_of(a) as fresh:
            for x, y in zip(again, run_once(fresh, a, 0.7)):
                assert x.tobytes() == y.tobytes()
        back = run_once(sa, a, 1.3)
        for x, y in zip(back, alone_a):
            assert x.tobytes() == y.tobytes()


def test_destroy_gives_the_memory_back():
    import ctypes as C
    from babelbrain_amd import _engine
    lib = _engine.load_library()
    # the HIP runtime this process has loaded already, by its path: no second runtime is opened
    paths = sorted({line.split()[-1] for line in open('/proc/self/maps') if 'libamdhip64' in line})
    assert paths, 'the library is loaded, so its runtime is'
    hip = C.CDLL(paths[0])
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]

    def free_bytes():
        f, t = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    def pair(shape, nF=1):
        h = C.c_void_p()
        assert lib.bfd_thermal_create(0, shape[0], shape[1], shape[2], nF, 5, C.byref(h)) == 0
        held = free_bytes()
        lib.bfd_thermal_destroy(h)
        return held
    pair((3, 3, 3))                                         # the runtime's own first allocations
    before = free_bytes()
    pair((3, 3, 3))
    granule = abs(free_bytes() - before)                    # what an empty create / destroy pair leaves: measured, not assumed
    before = free_bytes()
    held = pair((96, 100, 104), 2)
    n = 96 * 100 * 104
    assert before - held >= (6 + 3 * 2) * n * 4 + 2 * n        # the volumes were really there: 12 float32 volumes, the ids, the byte mask
    assert abs(free_bytes() - before) <= granule, (before, free_bytes(), granule)

