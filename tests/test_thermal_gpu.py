"""The Step-3 exposure analysis on the device against the numpy restatement (tests/thermal_oracle.py): counts, maxima, indices and the cleared water
field by equality (-0 == +0, as numpy compares), every plane energy within Higham's bound of the exact sum of the restatement's own terms:

    |got - fsum(terms)| <= ((n - 1) u / (1 - (n - 1) u)) * fsum(terms),   n = N1 N2 non-negative terms, u = 2^-53, any order of summation.

RatioLosses of the golden cases gets four times that bound relative to the golden (each of its two sums is within the bound of the exact sum, and so
is each of numpy's); PressureRatio without fixed power is held by equality. Shapes: N3 on either side of a wave and of a workgroup's width, N1 N2 on
either side of the rows one workgroup of the survey owns (128), volumes on either side of what one launch of the extrema kernel sweeps (2^20)."""
import json
import math
import os

import numpy as np
import pytest

from babelbrain_amd import ThermalAnalysis as TA
from tests import thermal_oracle as TO

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, 'golden', 'thermal_analysis_golden.json')))
GOLD = np.load(os.path.join(HERE, 'golden', 'thermal_analysis_golden.npz'))
CASES = sorted(META['cases'])
U = 2.0 ** -53
N3S = (1, 31, 32, 33, 63, 64, 65, 130)
ID_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def sum_bound(n, exact):
    g = (n - 1) * U
    return g / (1 - g) * exact


def random_problem(shape, idBytes, nMat, nVol, seed):
    rng = np.random.default_rng(seed)
    M = rng.integers(0, min(nMat, 256 ** idBytes), shape).astype(ID_DTYPES[idBytes])
    if nMat > 300 and idBytes > 1:
        M[rng.random(shape) < 0.3] = nMat - 1                       # the last rows of a long table are used
    classOf = rng.integers(0, 256, nMat).astype(np.uint8)
    vols = [rng.normal(0, 50, shape).astype(np.float32) for _ in range(nVol)]
    return M, classOf, vols


def assert_extrema(got, want):
    for name, w in zip(('count', 'maxIn', 'argIn', 'maxKey', 'argKey'), want):
        assert np.array_equal(got[name], w), (name, got[name], w)


def check_extrema(M, classOf, vols):
    got = TA.tissue_extrema(vols, M, classOf)
    assert_extrema(got, TO.class_extrema(vols, M, classOf))
    return got


@pytest.mark.parametrize('q,N3', list(enumerate(N3S)))
def test_extrema_shapes_ids_and_tables(q, N3):
    idBytes, nMat, nVol = (1, 2, 4)[q % 3], (2, 5, 8, 1030)[q % 4], (1, 3)[q % 2]
    check_extrema(*random_problem((3, 5, N3), idBytes, nMat, nVol, q))
    check_extrema(*random_problem((7, 9, N3), (1, 2, 4)[(q + 1) % 3], (2, 5, 8, 1030)[(q + 2) % 4], (1, 3)[(q + 1) % 2], q + 50))


def test_extrema_long_tables_and_many_volumes():
    check_extrema(*random_problem((6, 7, 33), 2, 1030, 3, 1))
    check_extrema(*random_problem((6, 7, 33), 4, 1030, 1, 2))
    check_extrema(*random_problem((6, 7, 33), 4, 4000, 2, 3))       # beyond the rows kept in LDS
    check_extrema(*random_problem((6, 7, 33), 2, 65536, 1, 4))
    check_extrema(*random_problem((5, 4, 9), 1, 5, 6, 5))           # more volumes than one launch reads


@pytest.mark.parametrize('shape', [(128, 64, 127), (128, 64, 128), (128, 64, 129), (2, 1024, 600)])
def test_extrema_either_side_of_one_sweep(shape):
    assert (128 * 64 * 128) == TA.SWEEP_VOXELS
    M, classOf, vols = random_problem(shape, 4, 8, 1, shape[2])
    classOf = np.array([1, 2, 4, 8, 16, 32, 64, 128], np.uint8)
    check_extrema(M, classOf, vols)


def test_extrema_where_the_maximum_lies():
    shape = (2, 1024, 600)                                          # more than one sweep of 2^20 voxels
    n = int(np.prod(shape))
    rng = np.random.default_rng(11)
    base_M = rng.integers(0, 4, shape).astype(np.uint8)
    classOf = np.array([1, 2, 4, 0], np.uint8)                      # id 3 belongs to no class
    base = rng.normal(0, 1, shape).astype(np.float32)
    # (first index, second index): in one wave, in two waves, in two workgroups, in two sweeps; then index 0 and the last index
    for a, b in ((4000, 4001), (4000, 4000 + 4 * 64), (4000, 4000 + 4 * 256 * 3), (4000, 4000 + TA.SWEEP_VOXELS), (0, None), (n - 1, None), (n - 1, 0)):
        x, M = base.copy(), base_M.copy()
        for i in (a, b):
            if i is not None:
                x.reshape(-1)[i] = 77.0
                M.reshape(-1)[i] = 2
        x.reshape(-1)[5000] = 99.0                                  # a larger value outside every class
        M.reshape(-1)[5000] = 3
        got = check_extrema(M, classOf, [x])
        first = min(i for i in (a, b) if i is not None)
        assert got['argIn'][0, 2] == first and got['maxIn'][0, 2] == 77.0 and got['argKey'][0, 2] == first, (a, b)


def test_extrema_degenerate_classes():
    shape = (4, 6, 65)
    rng = np.random.default_rng(12)
    M = rng.integers(0, 3, shape).astype(np.uint16)
    classOf = np.array([1, 2, 2], np.uint8)                         # classes 2 .. 7 are empty
    x = rng.normal(0, 5, shape).astype(np.float32)
    got = check_extrema(M, classOf, [x])
    assert got['count'][2] == 0 and got['argIn'][0, 2] == -1 and got['maxIn'][0, 2] == 0 and got['argKey'][0, 2] == 0
    neg = -np.abs(x) - 1                                            # a class of negative values loses to the first +-0 outside it
    got = check_extrema(M, classOf, [neg])
    first_out = int(np.flatnonzero(M.reshape(-1) != 0)[0])
    assert got['maxIn'][0, 0] < 0 and got['argKey'][0, 0] == first_out and got['maxKey'][0, 0] == 0
    everywhere = np.array([1, 1, 1], np.uint8)                      # no voxel outside: the negative maximum itself
    got = check_extrema(M, everywhere, [neg])
    assert got['argKey'][0, 0] == got['argIn'][0, 0] and got['maxKey'][0, 0] == got['maxIn'][0, 0] < 0
    zero = np.zeros(shape, np.float32)
    zero.reshape(-1)[::3] = -0.0
    got = check_extrema(M, classOf, [zero, x])
    assert list(got['argKey'][0]) == [0] * 8
    tiny = (rng.integers(-3, 4, shape) * 2.0 ** -149).astype(np.float32)          # float32 denormals are values like any other
    check_extrema(M, classOf, [tiny])


# ---------------------------------------------------------------- the survey ----------------------------------------------------------------

def survey_problem(shape, idBytes, nMat, nFields, seed):
    rng = np.random.default_rng(seed)
    M = rng.integers(0, min(nMat, 256 ** idBytes), shape).astype(ID_DTYPES[idBytes])
    classOf = rng.integers(0, 4, nMat).astype(np.uint8)
    classOf[0] = 3                                                  # some id is brain and cleared
    p = rng.uniform(-1e5, 4e5, (nFields,) + shape).astype(np.float32)
    pw = rng.uniform(-1e5, 7e5, (nFields,) + shape).astype(np.float32)
    rho, c = rng.uniform(900, 2300, nMat), rng.uniform(1400, 3200, nMat)
    return dict(M=M, classOf=classOf, p=p, pw=pw, rho=rho, c=c, rhoWater=1000.0, cWater=1482.3, dx2=(0.37e-3) ** 2)


def check_survey(s, brainMask=None, waterOut='separate'):
    pw = s['pw'].copy()
    out = None if waterOut is None else (pw if waterOut == 'inplace' else np.full(pw.shape, -7, np.float32))
    got = TA.loss_survey(s['p'], pw, s['M'], s['classOf'], s['rho'], s['c'], s['rhoWater'], s['cWater'], s['dx2'], brainMask=brainMask, waterOut=out)
    n = s['M'].shape[0] * s['M'].shape[1]
    for f in range(s['p'].shape[0]):
        want = TO.loss_survey(s['p'][f], s['pw'][f], s['M'], s['classOf'], s['rho'], s['c'], s['rhoWater'], s['cWater'], s['dx2'], brainMask=brainMask)
        for k in ('maxTissue', 'argTissue', 'maxWater', 'argWater'):
            assert got[k][f] == want[k], (k, f, got[k][f], want[k])
        if out is not None:
            assert np.array_equal(out[f], want['water']), f
        for which in ('WaterRaw', 'Water', 'Tissue'):
            for k in range(s['M'].shape[2]):
                exact = math.fsum(want['terms' + which][:, :, k].reshape(-1).tolist())
                assert abs(got['e' + which][f, k] - exact) <= sum_bound(n, exact), (which, f, k, got['e' + which][f, k], exact)
    if waterOut != 'inplace':
        assert np.array_equal(pw, s['pw'])                          # the input is not written
    return got


@pytest.mark.parametrize('q,N3', list(enumerate(N3S)))
def test_survey_shapes_ids_and_tables(q, N3):
    idBytes, nMat, nFields = (4, 1, 2)[q % 3], (5, 8, 1030, 2)[q % 4], (1, 3)[q % 2]
    check_survey(survey_problem((3, 5, N3), idBytes, nMat, nFields, q))


@pytest.mark.parametrize('rows', [(127, 1), (128, 1), (43, 3), (16, 17), (3, 128)])
def test_survey_rows_either_side_of_one_workgroup(rows):
    """127, 128, 129, 272 and 384 rows of (i, j): below, at and above the 128 one workgroup owns, and whole multiples of it"""
    assert TA.ROWS == 128
    check_survey(survey_problem(rows + (33,), 4, 1030, 1, rows[0]))


def test_survey_wide_planes_and_long_tables():
    check_survey(survey_problem((5, 30, 300), 2, 1030, 1, 1))       # more than one block of k, more than one chunk of rows
    check_survey(survey_problem((3, 4, 257), 4, 4000, 2, 2))        # beyond the rows kept in LDS


def test_survey_where_the_maximum_lies():
    shape = (6, 50, 130)                                            # 300 rows: three workgroups along the rows
    s = survey_problem(shape, 1, 5, 1, 21)
    s['classOf'] = np.array([1, 1, 0, 2, 2], np.uint8)              # brain: ids 0, 1; cleared: ids 3, 4
    n = int(np.prod(shape))
    base_p, base_w, base_M = s['p'].copy(), s['pw'].copy(), s['M'].copy()
    # in one wave, in two waves, in two workgroups; index 0; the last index
    for a, b in ((1000, 1001), (130 * 7, 130 * 7 + 64), (130 * 7 + 3, 130 * 200 + 3), (0, None), (n - 1, None), (n - 1, 0)):
        s['p'], s['pw'], s['M'] = base_p.copy(), base_w.copy(), base_M.copy()
        for i in (a, b):
            if i is not None:
                s['p'].reshape(-1)[i] = 9e5
                s['pw'].reshape(-1)[i] = 9e5
                s['M'].reshape(-1)[i] = 1
        s['p'].reshape(-1)[500], s['pw'].reshape(-1)[500], s['M'].reshape(-1)[500] = 9.5e5, 9.5e5, 3      # larger, outside the brain and cleared
        got = check_survey(s)
        first = min(i for i in (a, b) if i is not None)
        assert got['argTissue'][0] == first and got['argWater'][0] == first and got['maxTissue'][0] == np.float32(9e5), (a, b)


def test_survey_degenerate_fields():
    shape = (4, 40, 33)
    s = survey_problem(shape, 2, 8, 1, 31)
    s['classOf'][:] = 2                                             # no brain, everything cleared: both fields become zero, index 0
    got = check_survey(s)
    assert got['argTissue'][0] == 0 and got['argWater'][0] == 0 and not got['eTissue'].any() and not got['eWater'].any() and got['eWaterRaw'].all()
    s = survey_problem(shape, 2, 8, 1, 32)
    s['p'] = -np.abs(s['p']) - 1                                    # a negative brain loses to the first voxel outside it
    got = check_survey(s)
    assert got['maxTissue'][0] == 0
    s['p'][:] = 0
    s['pw'][:] = -0.0
    got = check_survey(s)
    assert got['argTissue'][0] == 0 and got['argWater'][0] == 0 and not got['eWaterRaw'].any()
    s = survey_problem(shape, 2, 8, 1, 33)
    s['p'] = (s['p'] * np.float32(1e-24)).astype(np.float32)        # squares and halves that are float32 denormals
    s['pw'] = (s['pw'] * np.float32(1e-25)).astype(np.float32)
    check_survey(s)


def test_survey_brain_mask_against_table_bit_0():
    s = survey_problem((5, 31, 65), 4, 8, 2, 41)
    by_table = check_survey(s)
    mask = (s['classOf'][s['M']] & 1).astype(bool)
    other = dict(s, classOf=s['classOf'] & 2 | (np.arange(8) % 2).astype(np.uint8))        # bit 0 of the table says something else: the mask rules
    by_mask = check_survey(other, brainMask=mask)
    for k in by_table:
        assert by_table[k].tobytes() == by_mask[k].tobytes(), k
    check_survey(other, brainMask=mask.astype(np.float32) * 3)      # any dtype, read as != 0


def test_survey_water_out_absent_separate_and_in_place():
    s = survey_problem((4, 33, 64), 1, 5, 3, 51)
    a = check_survey(s, waterOut=None)
    b = check_survey(s, waterOut='separate')
    c = check_survey(s, waterOut='inplace')
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k


def test_data_refusals():
    M, classOf, vols = random_problem((4, 5, 33), 4, 5, 2, 61)
    bad = M.copy()
    bad[3, 4, 32] = 5
    with pytest.raises(ValueError, match='refused data.*nMat'):
        TA.tissue_extrema(vols, bad, classOf)
    for v in (np.inf, -np.inf, np.nan):
        x = vols[1].copy()
        x[0, 0, 1] = v
        with pytest.raises(ValueError, match='refused data.*finite'):
            TA.tissue_extrema([vols[0], x], M, classOf)
    s = survey_problem((4, 5, 33), 2, 8, 2, 62)
    bad = s['M'].copy()
    bad[0, 0, 0] = 8
    water = s['pw'].copy()
    with pytest.raises(ValueError, match='refused data.*nMat'):
        TA.loss_survey(s['p'], water, bad, s['classOf'], s['rho'], s['c'], 1000.0, 1500.0, 1e-6, waterOut=water)
    assert np.array_equal(water, s['pw'])                           # nothing was cleared
    for name, field in (('p', 0), ('pw', 1)):
        for v in (np.inf, np.nan):
            t = dict(s, **{name: s[name].copy()})
            t[name][field, 3, 4, 32] = v
            with pytest.raises(ValueError, match='refused data.*finite'):
                TA.loss_survey(t['p'], t['pw'], s['M'], s['classOf'], s['rho'], s['c'], 1000.0, 1500.0, 1e-6)
    with pytest.raises(ValueError, match='refused data.*nMat'):     # both: the id is named first
        TA.loss_survey(t['p'], t['pw'], bad, s['classOf'], s['rho'], s['c'], 1000.0, 1500.0, 1e-6)


def test_repeats_are_byte_identical():
    M, classOf, vols = random_problem((9, 140, 300), 2, 1030, 3, 71)
    a, b = TA.tissue_extrema(vols, M, classOf), TA.tissue_extrema(vols, M, classOf)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert TA.last_kernel_ms > 0
    s = survey_problem((9, 140, 300), 4, 1030, 2, 72)
    runs = [TA.loss_survey(s['p'], s['pw'], s['M'], s['classOf'], s['rho'], s['c'], 1000.0, 1500.0, 1e-6) for _ in range(3)]
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes() == runs[2][k].tobytes(), k


# ---------------------------------------------------------------- the golden cases ----------------------------------------------------------------

def flags_of(rec):
    b = rec['build']
    return dict(ct=bool(b.get('ct')), segmented=bool(b.get('segmented')), homogeneous=bool(b.get('homogeneous')), benchmark=b.get('benchmark'))


@pytest.mark.parametrize('name', CASES)
def test_golden_cases(name):
    """AnalyzeLosses, the monitoring points and the exposure metrics on the device against what the reference's own statements gave"""
    import hashlib
    rec = META['cases'][name]
    case = TO.build_case(tuple(META['shape']), **rec['build'])
    f, call, ml, M = flags_of(rec), rec['call'], case['MaterialList'], case['MaterialMap']
    bench = dict(f['benchmark'], maxMaterial=int(M.max())) if f['benchmark'] else None
    t = TA.region_tables(case['nMat'], f['ct'], f['segmented'], f['homogeneous'], bench)
    SelBrain = np.isin(M, t['BrainID'])
    n = M.shape[0] * M.shape[1]
    results = []
    for brain in (SelBrain, t['BrainID']):                          # the volume the reference passes, and the list of ids
        water = case['pAmpWater'].copy()
        d = {}
        PressureRatio, RatioLosses = TA.AnalyzeLosses(case['pAmp'], M, case['LocIJK'], case['Input'], ml, water, call['Isppa'], case['xf'], case['yf'],
                                                      case['zf'], brain, f['homogeneous'], f['segmented'], call['TxSystem'], t['IdRegionBenchmark'],
                                                      FixedAcousticPower=call['FixedAcousticPower'], details=d)
        assert hashlib.sha1(water.tobytes()).hexdigest() == rec['water_sha1']
        want = rec['RatioLosses']
        assert np.asarray(RatioLosses).dtype.name == want['dtype']
        if call['TxSystem'] == 'DomeTx':
            assert float(RatioLosses) == want['value']
        else:
            assert abs(float(RatioLosses) - want['value']) <= 4 * sum_bound(n, 1.0) * want['value']
            assert d['UsedWaterLoc'] == (name == 'switch')
        want = rec['PressureRatio']
        assert np.asarray(PressureRatio).dtype.name == want['dtype']
        if call['FixedAcousticPower'] > 0:
            assert abs(float(PressureRatio) - want['value']) <= 4 * sum_bound(n, 1.0) * want['value']      # the root halves the relative error
        else:
            assert float(PressureRatio) == want['value']
        locs = {r[0]: r[1:4] for r in rec['reports'] if r[0].startswith('Location')}
        assert list(d['LocWater']) == locs['Location Max Pessure Water'] and list(d['LocTissue']) == locs['Location Max Pressure Tissue']
        results.append((PressureRatio, RatioLosses))
    assert results[0] == results[1]
    mSkin, mBrain, mSkull = TA.hottest_points(case['ResTemp'], M, t['classOf'])
    assert list(mSkin) == rec['mSkin'] and list(mBrain) == rec['mBrain'] and list(mSkull) == rec['mSkull']
    mp = TA.monitoring_points(mSkin, mBrain, mSkull, case['LocIJK'], M.shape, f['homogeneous'], f['benchmark'])
    assert np.array_equal(mp.indices, GOLD[name + '_monitor_index']) and np.array_equal(mp.ids, GOLD[name + '_monitor_id'])
    # the metrics with the golden's own PressureRatio, so that they are held by equality whatever the sums above gave
    ratio = np.dtype(rec['PressureRatio']['dtype']).type(rec['PressureRatio']['value'])
    assert rec['p_map_dtype'] == 'float64'
    met = TA.exposure_metrics(case['ResTemp'], case['FinalDose'], (case['pAmp'], ratio), M, t['classOf'], ml, t['BrainID'], call['Frequency'],
                              call['DutyCycle'], call['Isppa'])
    for k, want in rec['metrics'].items():
        assert float(met[k]) == want['value'] and np.asarray(met[k]).dtype.name == want['dtype'], k
    assert np.array_equal(met['MaxIsppa'], GOLD[name + '_MaxIsppa']) and np.array_equal(met['MaxIspta'], GOLD[name + '_MaxIspta'])
    p32 = (case['pAmp'] * np.float32(1.5)).astype(np.float32)       # a float32 p_map, as InputsBHTE.max(axis=0) is
    met = TA.exposure_metrics(case['ResTemp'], case['FinalDose'], p32, M, t['classOf'], ml, t['BrainID'], 5e5, 0.3, 5.0)
    want = TO.exposure_metrics(case['ResTemp'], case['FinalDose'], p32, SelBrain, M == 1, ((t['classOf'][M] >> TA.BIT_SKULL) & 1).astype(bool), ml,
                               t['BrainID'], 5e5, 0.3, 5.0)
    for k in TO.METRICS:
        assert np.array_equal(met[k], want[k]) and np.asarray(met[k]).dtype == np.asarray(want[k]).dtype, k


def test_an_empty_class_raises_as_numpy_does():
    case = TO.build_case((8, 8, 20), seed=1)
    t = TA.region_tables(case['nMat'], False, False)
    M = np.where(case['MaterialMap'] == 1, 0, case['MaterialMap']).astype(np.uint32)          # no skin
    with pytest.raises(ValueError, match='zero-size array'):
        TA.exposure_metrics(case['ResTemp'], case['FinalDose'], case['pAmp'], M, t['classOf'], case['MaterialList'], t['BrainID'], 5e5, 0.3, 5.0)


def test_bhte_takes_the_sparse_monitoring_points():
    from babelbrain_amd import RayleighAndBHTE as R
    rng = np.random.default_rng(81)
    N = (20, 18, 22)
    ml = {'Density': np.array([1000.0, 1116.0, 1850.0, 1700.0, 1041.0]), 'SoS': np.array([1500.0, 1537.0, 2800.0, 2300.0, 1562.0]),
          'Attenuation': np.array([0.0, 9.2, 54.0, 90.0, 3.0]), 'SpecificHeat': np.array([4178.0, 3391.0, 1313.0, 2274.0, 3630.0]),
          'Conductivity': np.array([0.6, 0.37, 0.32, 0.31, 0.51]), 'Perfusion': np.array([0.0, 106.0, 10.0, 30.0, 559.0]),
          'Absorption': np.array([0.0, 0.85, 0.16, 0.15, 0.85]), 'InitTemperature': np.full(5, 37.0)}
    mm = rng.integers(0, 5, N).astype(np.uint8)
    p = (3.0e6 * rng.random(N)).astype(np.float32)
    mp = TA.monitoring_points((3, 4, 5), (10, 9, 11), (2, 2, 20), (10, 9, 12), N)
    sparse = R.BHTE(p, mm, ml, 4e-4, 30, 20, -1, dt=0.02, DutyCycle=0.5, MonitoringPointsMap=mp)
    dense = R.BHTE(p, mm, ml, 4e-4, 30, 20, -1, dt=0.02, DutyCycle=0.5, MonitoringPointsMap=mp.dense())
    assert len(sparse) == len(dense) == 5 and sparse[4].shape == (4, 30)
    for a, b in zip(sparse, dense):
        assert a.tobytes() == b.tobytes()
    assert sparse[4].max() > 37.0
