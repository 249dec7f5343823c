"""tests/bhte_reference.py held to the oracle, and what its per-voxel dose bound sees that the whole-array norm it replaces does not.

The oracle is on both sides (no GPU). Two cases: A, the 40 x 36 x 44 problem of test_bhte_matches_oracle_and_monitors (uniform 37 degC start, Gaussian
focus, 120 steps: the dose spans 4.5 decades); B, a 70 x 30 x 35 problem from a random 37-45 degC field (23 steps), as the later tests of
tests/test_bhte_gpu.py use.
(1) BO.bhte, rebuilt on the step generator, has the bits of the plain loop it replaced.
(2) The oracle's own float32 dose (numpy's float32 power) lies inside the bound of the float64 reference.
(3) Faults planted in that float32 dose: assert_dose reports every one and names the voxel; the former bound, rel L2 < 1e-5 over the array,
    passes those listed in OLD_METRIC_PASSES.
(4) history refuses a temperature outside [21.5, 86]; assert_equal finds a point series shifted by one step and a plane sampled one step late."""
import numpy as np
import pytest

from oracle import bhte_oracle as BO
from tests import bhte_reference as BR
from tests.util import rel_l2

OLD_TOL = 1e-5


def _materials():
    return {'Density': np.array([1000.0, 1116.0, 1896.5, 1738.0, 1041.0]), 'SoS': np.array([1500.0, 1537.0, 2476.0, 2205.0, 1562.0]),
            'Attenuation': np.array([0.0, 2.3, 81.0, 81.0, 3.45]), 'SpecificHeat': np.array([4178.0, 3391.0, 1313.0, 2274.0, 3630.0]),
            'Conductivity': np.array([0.6, 0.37, 0.32, 0.31, 0.51]), 'Perfusion': np.array([0.0, 106.0, 10.0, 30.0, 559.0]),
            'Absorption': np.array([0.0, 0.85, 0.16, 0.15, 0.85]), 'InitTemperature': np.full(5, 37.0)}


def _ftz(a):
    a = np.array(a, np.float32)
    a[np.abs(a) < np.finfo(np.float32).tiny] = 0
    return a


def _plain_loop(T0, dose0, q, mat, cd, cp, Tcore, dt, sched):
    """BO.bhte as it stood before the step generator: one loop, temperature and dose together"""
    T = np.array(T0, np.float32)
    dose = np.array(dose0, np.float32)
    cdv = np.asarray(cd, np.float32)[mat][1:-1, 1:-1, 1:-1]
    cpv = np.asarray(cp, np.float32)[mat][1:-1, 1:-1, 1:-1]
    Tc = np.float32(Tcore)
    dtm = np.float32(dt / 60.0)
    for f in sched:
        c = T[1:-1, 1:-1, 1:-1]
        sm = ((((T[:-2, 1:-1, 1:-1] + T[2:, 1:-1, 1:-1]) + T[1:-1, :-2, 1:-1]) + T[1:-1, 2:, 1:-1]) + T[1:-1, 1:-1, :-2]) + T[1:-1, 1:-1, 2:]
        tn = c + cdv * (sm - np.float32(6.0) * c)
        tn = tn + cpv * (Tc - c)
        if f >= 0:
            tn = tn + q[f][1:-1, 1:-1, 1:-1]
        Tn = T.copy()
        Tn[1:-1, 1:-1, 1:-1] = tn
        T = Tn
        R = np.where(T >= np.float32(43.0), np.float32(0.5), np.float32(0.25))
        dose = dose + dtm * np.power(R, np.float32(43.0) - T, dtype=np.float32)
    return T, dose


class Case:
    def __init__(self, name, N, T0, q, mm, dt, nS, nOn, sl, fm, pts):
        from babelbrain_amd import RayleighAndBHTE as R
        self.name, self.N, self.T0, self.mm, self.dt, self.nS, self.nOn, self.sl, self.fm, self.pts = name, N, T0, mm, dt, nS, nOn, sl, fm, pts
        self.cd, self.cp, qf = R.bhte_coefficients(_materials(), 4e-4, dt, 1.0 if name == 'B' else 0.5)
        self.q = _ftz(q(qf))
        self.sched = BO.single_field_schedule(nS, nOn)
        self.zero = np.zeros(N, np.float32)
        self.To, self.Do = BO.bhte(T0, self.zero, self.q, mm, self.cd, self.cp, 37.0, dt, nS, nOn)
        self.h = BR.history(T0, self.zero, self.q, mm, self.cd, self.cp, 37.0, dt, self.sched)
        self.D64 = self.h.dose64()


@pytest.fixture(scope='module')
def A():
    rng = np.random.default_rng(5)
    N = (40, 36, 44)
    mm = rng.integers(0, 5, N).astype(np.uint8)
    x, y, z = np.meshgrid(*[np.arange(n) - n / 2 for n in N], indexing='ij')
    p = 5.0e6 * np.exp(-(x ** 2 + y ** 2 + (z / 2) ** 2) / 30.0)
    return Case('A', N, np.full(N, 37.0, np.float32), lambda qf: (p.astype(np.float32) ** 2) * qf[mm], mm, 0.02, 120, 80, 18, 10,
                [(20, 18, 22), (10, 10, 30), (25, 20, 12)])


@pytest.fixture(scope='module')
def B():
    rng = np.random.default_rng(23)
    N = (70, 30, 35)
    mm = rng.integers(0, 5, N).astype(np.uint8)
    p = (3.0e6 * rng.random(N)).astype(np.float32)
    T0 = (37.0 + 8.0 * rng.random(N)).astype(np.float32)
    return Case('B', N, T0, lambda qf: (p ** 2) * qf[mm], mm, 0.02, 23, 13, 15, 3, [(1, 1, 1), (35, 15, 17), (69, 28, 0)])


def test_the_oracle_rebuilt_on_the_step_generator_keeps_its_bits(A, B):
    for c in (A, B):
        T, D = _plain_loop(c.T0, c.zero, c.q[None], c.mm, c.cd, c.cp, 37.0, c.dt, c.sched)
        assert T.dtype == c.To.dtype == np.float32 and D.dtype == c.Do.dtype == np.float32
        assert np.array_equal(T.view(np.uint32), c.To.view(np.uint32)) and np.array_equal(D.view(np.uint32), c.Do.view(np.uint32)), c.name
        assert np.array_equal(c.h.T, c.To) and c.h.steps.shape == (c.nS,) + c.N
    # and the multi-field form, continuing from a dose
    rng = np.random.default_rng(2)
    sched = [0, 0, -1, 1, 1, 1, -1, 0]
    q2 = np.stack([B.q, B.q[::-1].copy()])
    D0 = (1e-3 * rng.random(B.N)).astype(np.float32)
    T, D = _plain_loop(B.T0, D0, q2, B.mm, B.cd, B.cp, 37.0, B.dt, sched)
    T2, D2 = BO.bhte(B.T0, D0, q2, B.mm, B.cd, B.cp, 37.0, B.dt, len(sched), 0, field_of_step=sched)
    assert np.array_equal(T.view(np.uint32), T2.view(np.uint32)) and np.array_equal(D.view(np.uint32), D2.view(np.uint32))


def test_the_oracle_float32_dose_lies_inside_the_bound(A, B):
    for c in (A, B):
        worst = BR.assert_dose(c.Do, c.D64, c.nS, 'oracle float32 dose, case ' + c.name, T=c.To, mat=c.mm)
        print('case %s: dose %.3g .. %.3g, oracle float32 dose at %.3f of the bound, rel L2 %.2e' % (c.name, c.D64.min(), c.D64.max(), worst, rel_l2(c.Do, c.D64)))
        assert 0 < worst < 0.5                                  # far inside: numpy's power is good to an ulp and sums round both ways
    assert A.D64.max() / A.D64.min() > 1e4                      # the decades the old norm could not see across


def _f32(x):
    return np.float32(x)


def _faults(c):
    """name -> (faulty float32 dose, the voxel the message must name -- or, of a fault in many cells, their number)"""
    D, h = c.Do, c.h
    flat = np.argsort(D, axis=None)
    median = np.unravel_index(int(flat[D.size // 2]), D.shape)
    coldest = np.unravel_index(int(flat[0]), D.shape)
    step = c.nS // 2
    inc = BR.term64(h.steps[step], c.dt)
    out = {}
    a = D.copy(); a[median] = _f32(float(D[median]) - inc[median]); out['one increment dropped in a median cell'] = (a, median)
    a = D.copy(); a[median] = _f32(float(D[median]) + inc[median]); out['one increment doubled in a median cell'] = (a, median)
    a = D.copy(); a[coldest] = 0; out['the coldest cell zeroed'] = (a, coldest)
    for share in (10, 30):
        a = D.copy(); cut = flat[:D.size * share // 100]
        a.reshape(-1)[cut] = (D.astype(np.float64) - inc).astype(np.float32).reshape(-1)[cut]
        out["one step's increments dropped in the coldest %d %%" % share] = (a, len(cut))
    below = np.argwhere(h.steps.max(axis=0) < 43.0)
    cell = tuple(int(v) for v in below[len(below) // 2])
    a = D.copy(); a[cell] = _f32(np.sum(float(_f32(c.dt / 60.0)) * 0.5 ** (43.0 - h.steps[(slice(None),) + cell].astype(np.float64))))
    out['base 0.5 in place of 0.25 in one cell below 43'] = (a, cell)
    a = D.copy(); a[:, :, -1] = 0; out['the face cells of one side left without dose'] = (a, (0, 0, D.shape[2] - 1))
    a = D.copy(); a[median] = np.nan; out['a NaN'] = (a, median)
    a = D.copy(); a[median] = -a[median]; out['a negative value'] = (a, median)
    return out


# which faults the former assertion, rel_l2(D, Do) < 1e-5, lets through (measured here, asserted below), per case
OLD_METRIC_PASSES = {
    'A': {'one increment dropped in a median cell', 'one increment doubled in a median cell', "one step's increments dropped in the coldest 10 %"},
    'B': {'the coldest cell zeroed'},             # 1.5e-6: what case A catches by a hair (1.05e-5) is invisible from a random start
}


@pytest.mark.parametrize('name', ['A', 'B'])
def test_planted_faults_are_found_and_named_and_what_the_old_metric_made_of_them(name, A, B):
    c = A if name == 'A' else B
    passed = set()
    for what, (bad, voxel) in _faults(c).items():
        old = rel_l2(bad, c.Do)
        with pytest.raises(AssertionError) as e:
            BR.assert_dose(bad, c.D64, c.nS, what, T=c.To, mat=c.mm)
        msg = str(e.value)
        assert what in msg and '(i, j, k) = (' in msg and ', T ' in msg and ', material ' in msg, msg
        if isinstance(voxel, tuple):
            assert '(i, j, k) = (%d, %d, %d), T %.9g, material %d' % (voxel + (c.To[voxel], c.mm[voxel])) in msg, msg
        else:
            assert '%d of %d voxels' % (voxel, c.Do.size) in msg, msg
        ratio = msg.split(' x the bound')[0].split()[-1] if ' x the bound' in msg else '-'
        print('case %s, %s: old rel L2 %.3e (%s), first voxel at %s x the bound' % (name, what, old, 'passes' if old < OLD_TOL else 'caught', ratio))
        if old < OLD_TOL:
            passed.add(what)
    assert passed == OLD_METRIC_PASSES[name]


def test_dose_form_is_part_of_the_comparison(A):
    with pytest.raises(AssertionError, match='float32'):
        BR.assert_dose(A.Do.astype(np.float64), A.D64, A.nS, 'float64 result')
    with pytest.raises(AssertionError, match='shape'):
        BR.assert_dose(A.Do[:-1], A.D64, A.nS, 'a plane short')
    with pytest.raises(AssertionError, match='steps'):
        BR.assert_dose(A.Do, A.D64, BR.N_MAX + 1, 'too many steps')
    # continuation: the initial dose is part of the reference and costs nothing
    D0 = A.Do
    h = BR.history(A.To, D0, A.q, A.mm, A.cd, A.cp, 37.0, A.dt, [-1] * 7)
    _, D1 = BO.bhte(A.To, D0, A.q, A.mm, A.cd, A.cp, 37.0, A.dt, 7, 0)
    assert BR.assert_dose(D1, h.dose64(), 7, 'continued') < 0.5
    assert BR.assert_dose(D0, h.dose64(0), 0, 'no step') == 0.0


def test_history_refuses_temperatures_outside_the_exact_range(B):
    for T, word in ((21.4, '21.4'), (86.5, '86.5')):
        T0 = B.T0.copy(); T0[0, 3, 4] = T                        # a face cell keeps its temperature
        with pytest.raises(AssertionError, match='outside'):
            BR.history(T0, B.zero, B.q, B.mm, B.cd, B.cp, 37.0, B.dt, [-1, -1])
    T0 = B.T0.copy(); T0[0, 3, 4] = 21.5; T0[0, 3, 5] = 86.0
    assert BR.history(T0, B.zero, B.q, B.mm, B.cd, B.cp, 37.0, B.dt, [-1, -1]).n == 2
    # the reason: inside, float32 43 - T is exact
    rng = np.random.default_rng(1)
    T = rng.uniform(BR.T_LO, BR.T_HI, 100000).astype(np.float32)
    assert np.array_equal((np.float32(43.0) - T).astype(np.float64), 43.0 - T.astype(np.float64))


def test_monitor_equality_finds_a_shifted_series_and_a_late_plane(A, B):
    for c in (A, B):
        pts, mon = c.h.points(c.pts), c.h.plane(c.sl, c.fm)
        assert pts.shape == (len(c.pts), c.nS) and mon.shape == (c.N[0], c.N[2], (c.nS + c.fm - 1) // c.fm)
        assert np.array_equal(pts[:, -1], [c.To[p] for p in c.pts]) and np.array_equal(mon[:, :, 0], c.h.steps[0][:, c.sl, :])
        BR.assert_equal(pts.copy(), pts, 'points', 'ps')
        BR.assert_equal(mon.copy(), mon, 'plane', 'ikm')
        shifted = np.concatenate([pts[:, :1], pts[:, :-1]], axis=1)          # every sample one step late
        with pytest.raises(AssertionError) as e:
            BR.assert_equal(shifted, pts, 'points shifted', 'ps')
        assert '(point, step) = (' in str(e.value) and 'points shifted' in str(e.value)
        late = mon.copy()
        m = mon.shape[2] // 2
        late[:, :, m] = c.h.steps[m * c.fm + 1][:, c.sl, :]                    # one sample taken a step late
        with pytest.raises(AssertionError) as e:
            BR.assert_equal(late, mon, 'plane late', 'ikm')
        assert ', %d)' % m in str(e.value) and '(i, k, sample) = (' in str(e.value)
    # point order follows the ids of the map
    mpm = np.zeros(A.N, np.uint32); mpm[5, 6, 7] = 2; mpm[20, 30, 3] = 1
    assert BR.points_of(mpm) == [(20, 30, 3), (5, 6, 7)]
    N = A.N
    rm = A.h.running_max([0, 80, 120])
    assert np.array_equal(rm, np.maximum(np.maximum(A.T0, A.h.steps[79]), A.To))
