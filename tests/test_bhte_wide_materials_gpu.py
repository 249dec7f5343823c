"""The bio-heat solver on a CT-derived material list (16-bit ids: bfd_bhte_run_volumes16 / bfd_bhte_run_protocol16). A CT plan quantises bone to
2^10 bins behind the soft tissues, one thermal row per bin (CalculateTemperatureEffects.py:804-841): 6 + 1024 = 1030 rows here, density,
speed of sound and attenuation varying across the bins. Every kernel that reads the ids has a 16-bit instantiation with the same expressions in
the same order, so: every multi-step path has the bits of one step per launch; the temperature has the bits of the numpy oracle and the dose lies,
voxel by voxel, within the derived bound of tests/bhte_reference.py; and a five-material problem whose rows are scattered over the 1030-row list
has the bits of the 8-bit run -- which a dropped high byte or an id queue shifted by one plane cannot give."""
import ctypes as C

import numpy as np
import pytest

from oracle import bhte_oracle as BO
from tests import bhte_reference as BR
from tests.util import rel_l2
from tests.test_bhte_gpu import _ftz, _materials
from tests.test_bhte_protocol_gpu import _against_oracle, _chained, _equal

pytestmark = pytest.mark.gpu

N_SOFT, N_BONE = 6, 1024
DX, DT = 4e-4, 0.02
_ENV = ('BFD_BHTE_FUSE', 'BFD_BHTE_STEPS', 'BFD_BHTE_ZRUN')


def _ct_list(n_bone=N_BONE, init_varies=False):
    """water, skin, brain, white matter, grey matter, CSF, then the bone bins (rows 6..): thermal columns as the caller fills them (:804-841, bSegmentedBrain), acoustic columns rising with the bin's density"""
    n = N_SOFT + n_bone
    b = np.linspace(0.0, 1.0, n_bone)
    ml = {'Density': np.concatenate([[1000.0, 1116.0, 1041.0, 1041.0, 1045.0, 1007.0], 1200.0 + 1100.0 * b]),
          'SoS': np.concatenate([[1500.0, 1537.0, 1562.0, 1552.0, 1500.0, 1504.0], 1600.0 + 1500.0 * b]),
          'Attenuation': np.concatenate([[0.0, 2.3, 3.45, 4.1, 2.9, 0.05], 20.0 + 100.0 * b ** 2]),
          'SpecificHeat': np.concatenate([[4178.0, 3391.0, 3630.0, 3583.0, 3696.0, 4096.0], np.full(n_bone, (1313.0 + 2274.0) / 2)]),
          'Conductivity': np.concatenate([[0.6, 0.37, 0.51, 0.48, 0.55, 0.57], np.full(n_bone, (0.31 + 0.32) / 2)]),
          'Perfusion': np.concatenate([[0.0, 106.0, 559.0, 212.0, 764.0, 0.0], np.full(n_bone, 20.0)]),
          'Absorption': np.concatenate([[0.0, 0.85, 0.85, 0.85, 0.85, 0.0], np.full(n_bone, (0.16 + 0.15) / 2)])}
    ml['InitTemperature'] = 36.0 + 9.0 * ((np.arange(n) * 7919) % n) / n if init_varies else np.full(n, 37.0)      # some rows above 43
    return ml


def _ids(rng, N, n):
    """random ids over the whole list, with the ids around the 8-bit boundary and the last one on faces, at the edges of the y tiles (20 / 22 / 24 rows),
    of the 64-cell x tiles and of short z-runs, and in the interior"""
    mm = rng.integers(0, n, N).astype(np.int64)
    marks = [v for v in (255, 256, 257, n - 1) if v < n]
    spots = [(0, 0, 0), (N[0] - 1, N[1] - 1, N[2] - 1), (0, N[1] // 2, N[2] // 2), (N[0] // 2, 0, N[2] - 1), (N[0] // 2, N[1] // 2, N[2] // 2), (1, 1, 1)]
    spots += [(N[0] // 2, j, min(k, N[2] - 1)) for j in (19, 20, 21, 22, 23, 24) if j < N[1] for k in (N[2] // 3, 63, 64)]
    spots += [(i, N[1] // 2, N[2] // 2) for i in (4, 5, 7, 8, 31, 32) if i < N[0]]
    for s, (i, j, k) in enumerate(spots):
        mm[i, j, k] = marks[s % len(marks)]
    return mm


def _clear(monkeypatch, **env):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# grid, steps, (on, off) per field, z-run, plane sample every, monitored plane
_GRIDS = [((150, 61, 37), 40, [[9, 7], [5, 3]], None, 3, 30), ((65, 23, 9), 13, [[7, 6], [1, 0]], '1', 4, 11),
          ((131, 45, 20), 30, [[6, 4], [0, 5], [8, 2]], None, 5, 22), ((3, 3, 3), 9, [[4, 2], [1, 1]], None, 2, 1),
          ((9, 23, 70), 14, [[5, 2], [2, 1]], '5', 1, 20)]          # the last: two x tiles (the fastest axis is the last one)


@pytest.mark.parametrize('case', _GRIDS, ids=lambda c: 'x'.join(map(str, c[0])))
def test_every_pass_length_has_the_bits_of_one_step_per_launch(case, monkeypatch):
    from babelbrain_amd import RayleighAndBHTE as R
    N, nS, onoff, zrun, fm, sl = case
    rng = np.random.default_rng(31)
    ml = _ct_list()
    n = N_SOFT + N_BONE
    mm = _ids(rng, N, n)
    fields = (3.0e6 * rng.random((len(onoff),) + N)).astype(np.float32)
    mpm = np.zeros(N, np.uint32); mpm[1, 1, 1] = 1; mpm[N[0] // 2, N[1] // 2, N[2] // 2] = 2; mpm[N[0] - 1, N[1] - 2, 0] = 3; mpm[0, N[1] - 1, N[2] - 1] = 4
    T0 = (37.0 + 8.0 * rng.random(N)).astype(np.float32)                 # some cells above 43: both dose bases
    z = dict(BFD_BHTE_ZRUN=zrun) if zrun else {}

    def run(**env):
        _clear(monkeypatch, **env, **z)
        return R.BHTEMultiplePressureFields(fields, mm, ml, DX, nS, onoff, sl, nFactorMonitoring=fm, dt=DT, initT0=T0, MonitoringPointsMap=mpm)
    one = run(BFD_BHTE_FUSE='0')
    assert one[0].max() > 44.0 and one[1].max() > 0 and one[4].shape == (len(np.unique(mpm)) - 1, nS)
    variants = {'S=3': dict(BFD_BHTE_STEPS='3'), 'S=4': dict(BFD_BHTE_STEPS='4'), 'default': {}, 'two-step g': dict(BFD_BHTE_FUSE='1', BFD_BHTE_STEPS='2')}
    for name, env in variants.items():
        got = run(**env)
        for q, (a, b) in enumerate(zip(got, one)):
            assert a.shape == b.shape and np.array_equal(a, b), (name, N, q)


@pytest.mark.parametrize('steps', ['3', '4', 'default', '2'])
def test_against_the_oracle(steps, monkeypatch):
    from babelbrain_amd import RayleighAndBHTE as R
    rng = np.random.default_rng(37)
    N = (70, 30, 35)
    ml = _ct_list(init_varies=True)
    mm = _ids(rng, N, N_SOFT + N_BONE)
    p = (3.0e6 * rng.random(N)).astype(np.float32)
    _clear(monkeypatch, **({} if steps == 'default' else dict(BFD_BHTE_STEPS=steps)))
    T, D, _, Q = R.BHTE(p, mm, ml, DX, 23, 13, -1, dt=DT)                # starts from InitTemperature[material]
    cd, cp, qf = R.bhte_coefficients(ml, DX, DT, 1.0)
    q = (p ** 2) * qf[mm]
    assert np.array_equal(Q, _ftz(q))
    T0 = ml['InitTemperature'].astype(np.float32)[mm]
    To, Do = BO.bhte(T0, np.zeros(N, np.float32), Q, mm, cd, cp, 37.0, DT, 23, 13)
    assert To.max() > 44.0
    assert np.array_equal(T, To) and rel_l2(D, Do) < 1e-6
    h = BR.history(T0, np.zeros(N, np.float32), Q, mm, cd, cp, 37.0, DT, BO.single_field_schedule(23, 13))
    BR.assert_equal(T, h.T, '16-bit ids, steps %s: temperature' % steps, 'ijk', mm)
    worst = BR.assert_dose(D, h.dose64(), 23, '16-bit ids, steps %s: dose' % steps, T=h.T, mat=mm)
    print('16-bit ids, steps per pass %s: dose at %.3f of the bound' % (steps, worst))


def test_relabelled_five_material_problem_has_the_bits_of_the_8_bit_run(monkeypatch):
    """the five rows scattered to ids 3, 255, 256, 517 and 1029 of a 1030-row list whose other rows would give something else entirely"""
    from babelbrain_amd import RayleighAndBHTE as R
    rng = np.random.default_rng(41)
    N = (131, 45, 20)
    ml5 = _materials()
    ml5['InitTemperature'] = np.array([37.0, 36.0, 44.5, 41.0, 38.5])
    mm5 = rng.integers(0, 5, N).astype(np.uint8)
    where = np.array([3, 255, 256, 517, 1029])
    n = 1030
    wide = {'Density': rng.uniform(900.0, 2500.0, n), 'SoS': rng.uniform(1400.0, 3200.0, n), 'Attenuation': rng.uniform(0.0, 200.0, n),
            'SpecificHeat': rng.uniform(1000.0, 4500.0, n), 'Conductivity': rng.uniform(0.1, 1.0, n), 'Perfusion': rng.uniform(0.0, 900.0, n),
            'Absorption': rng.uniform(0.0, 1.0, n), 'InitTemperature': rng.uniform(20.0, 60.0, n)}
    for k in wide:
        wide[k][where] = ml5[k]
    mmw = where[mm5]
    fields = (3.0e6 * rng.random((2,) + N)).astype(np.float32)
    onoff = [[6, 4], [3, 2]]
    mpm = np.zeros(N, np.uint32); mpm[1, 1, 1] = 1; mpm[65, 22, 10] = 2; mpm[130, 43, 0] = 3; mpm[0, 44, 19] = 4
    T0 = (37.0 + 8.0 * rng.random(N)).astype(np.float32)
    for env in ({}, dict(BFD_BHTE_STEPS='3'), dict(BFD_BHTE_STEPS='2'), dict(BFD_BHTE_FUSE='0')):
        _clear(monkeypatch, **env)
        for init in (T0, None):                                           # None: from InitTemperature[material] (table_lookup)
            a = R.BHTEMultiplePressureFields(fields, mm5, ml5, DX, 31, onoff, 22, nFactorMonitoring=3, dt=DT, initT0=init, MonitoringPointsMap=mpm)
            b = R.BHTEMultiplePressureFields(fields, mmw, wide, DX, 31, onoff, 22, nFactorMonitoring=3, dt=DT, initT0=init, MonitoringPointsMap=mpm)
            assert len(a) == len(b) == 5
            for q, (x, y) in enumerate(zip(a, b)):
                assert x.shape == y.shape and np.array_equal(x, y), (env, init is None, q)
            assert a[0].max() > 44.0 and a[1].max() > 0


def test_just_above_the_8_bit_limit(monkeypatch):
    from babelbrain_amd import RayleighAndBHTE as R
    rng = np.random.default_rng(43)
    N = (40, 47, 33)
    p = (3.0e6 * rng.random(N)).astype(np.float32)
    T0 = (37.0 + 8.0 * rng.random(N)).astype(np.float32)
    mpm = np.zeros(N, np.uint32); mpm[20, 20, 16] = 1; mpm[39, 46, 32] = 2
    # 257 rows, every id used: against one step per launch
    ml = _ct_list(257 - N_SOFT)
    mm = rng.permutation(np.arange(N[0] * N[1] * N[2]) % 257).reshape(N)
    assert len(np.unique(mm)) == 257
    _clear(monkeypatch)
    a = R.BHTE(p, mm, ml, DX, 22, 14, 20, nFactorMonitoring=2, dt=DT, initT0=T0, MonitoringPointsMap=mpm)
    _clear(monkeypatch, BFD_BHTE_FUSE='0')
    b = R.BHTE(p, mm, ml, DX, 22, 14, 20, nFactorMonitoring=2, dt=DT, initT0=T0, MonitoringPointsMap=mpm)
    for q, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), q
    # 300 rows of which the map uses the first 256: the 16-bit entry, and the bits of the 8-bit entry on the list cut to 256 rows
    ml = _ct_list(300 - N_SOFT)
    cut = {k: v[:256] for k, v in ml.items()}
    mm = rng.integers(0, 256, N)
    mm[0, 0, 0] = 255
    _clear(monkeypatch)
    a = R.BHTE(p, mm, ml, DX, 22, 14, 20, nFactorMonitoring=2, dt=DT, initT0=T0, MonitoringPointsMap=mpm)
    b = R.BHTE(p, mm, cut, DX, 22, 14, 20, nFactorMonitoring=2, dt=DT, initT0=T0, MonitoringPointsMap=mpm)
    for q, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), q
    assert a[0].max() > 44.0


def test_start_from_the_init_temperature_of_each_material(monkeypatch):
    from babelbrain_amd import RayleighAndBHTE as R
    rng = np.random.default_rng(47)
    N = (33, 50, 41)
    ml = _ct_list(init_varies=True)
    mm = _ids(rng, N, N_SOFT + N_BONE)
    p = (2.0e6 * rng.random(N)).astype(np.float32)
    _clear(monkeypatch)
    a = R.BHTE(p, mm, ml, DX, 17, 9, -1, dt=DT)
    b = R.BHTE(p, mm, ml, DX, 17, 9, -1, dt=DT, initT0=ml['InitTemperature'].astype(np.float32)[mm])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    zero = R.BHTE(p, mm, ml, DX, 0, 0, -1, dt=DT)                        # no step: T is the table itself
    assert np.array_equal(zero[0], ml['InitTemperature'].astype(np.float32)[mm]) and zero[0].max() > 44.0


def test_protocol_on_the_wide_list_equals_chained_calls(monkeypatch):
    from babelbrain_amd import RayleighAndBHTE as R
    rng = np.random.default_rng(53)
    _clear(monkeypatch)
    N = (36, 40, 44)
    ml = _ct_list(init_varies=True)
    mm = _ids(rng, N, N_SOFT + N_BONE)
    x, y, z = np.meshgrid(*[np.arange(n) - n / 2 for n in N], indexing='ij')
    fields = np.stack([4.0e6 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z / 2) ** 2) / 25.0) for cx, cy in ((-6, 0), (5, 4))])
    mpm = np.zeros(N, np.uint32); mpm[18, 20, 22] = 1; mpm[9, 10, 33] = 2; mpm[21, 20, 11] = 3
    # single field (BHTE calls), from InitTemperature[material]
    args = (0, 2, 4, 10, 6, 100)                      # nCurrent, Repetitions, TotalIterations, pause, OFF, limit
    got = R.RunBHTECycles(*args, 'pressure.npz', fields[0], mm, ml, DX, 13, 7, -1, 1, DT, 0.7, 'HIP', mpm, 37.0, None, None, None, None)
    ref = _chained(*args, True, fields[0], mm, ml, DX, 13, 7, DT, 0.7, mpm, 37.0, None, None, None, None)
    _equal(got, ref)
    assert got[4].shape == (3, 4 * (13 + 6) + 2 * 10) and got[0].max() > 44.0
    _against_oracle(got, args, fields[0], mm, ml, DX, 13, 7, DT, 0.7, mpm, ml['InitTemperature'].astype(np.float32)[mm], 'protocol on the 1030-row list 36x40x44')
    # steered fields (BHTEMultiplePressureFields calls)
    onoff = np.array([[5, 3]] * 2, np.int32)
    args = (0, 2, 2, 5, 4, 100)
    got = R.RunBHTECycles(*args, np.zeros(2), fields, mm, ml, DX, 19, onoff, -1, 1, DT, 0.5, 'HIP', mpm, 37.0, None, None, None, None)
    ref = _chained(*args, False, fields, mm, ml, DX, 19, onoff, DT, 0.5, mpm, 37.0, None, None, None, None)
    _equal(got, ref)


def test_the_c_entry_refuses_more_materials_than_the_limit():
    from babelbrain_amd import _engine
    lib = _engine.load_library()
    limit = lib.bfd_bhte_max_materials()
    n, N = limit + 1, (4, 4, 4)
    mat = np.zeros(N, np.uint16)
    tab = np.full(n, 0.01, np.float32)
    p, T, D = np.zeros(N, np.float32), np.full(N, 40.0, np.float32), np.zeros(N, np.float32)
    sched = np.zeros(2, np.int32)
    ms = C.c_double()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(nMat):
        return lib.bfd_bhte_run_volumes16(0, *N, nMat, ptr(mat), ptr(tab), ptr(tab), ptr(tab), ptr(tab), 1, ptr(p), None, ptr(T), ptr(D), 3, 37.0, DT,
                                          2, ptr(sched), -1, 1, None, 0, None, None, C.byref(ms))
    assert call(n) == -1 and str(limit) in lib.bfd_last_error().decode()
    assert np.all(T == 40.0)                                             # refused before anything ran
    assert call(limit) == 0, lib.bfd_last_error().decode()
    assert np.all(T[1:-1, 1:-1, 1:-1] < 40.0) and np.all(T[0] == 40.0)   # perfusion pulls the inner cells towards 37
