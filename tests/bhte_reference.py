"""The bio-heat solver's outputs against the numpy oracle, element by element: the step history of the oracle, the CEM43 dose in float64 from
that history, and the bound a float32 dose of the device is held to, voxel by voxel.

The device (bhte_dose_rate of csrc/bfd_bhte_kernels.hip) adds, after every step and in step order, fl(dtMin * v_exp_f32(-b (43 - T'))) to the float32
dose, dtMin = float32(dt/60), b = 1 where T' >= 43 and 2 otherwise. The temperature has the oracle's bits (the roundings of bhte_update are
pinned), so the reference sums the same terms exactly:

    D64 = dose0 + sum_s float64(dtMin) 2^(-b_s (43 - T_s))          (43 - T_s in float64)

For T_s in [21.5, 86] the device's float32 43.0f - T' is exact (Sterbenz) and so is its doubling: both sides exponentiate the same argument;
`history` refuses a temperature outside that range. The bound, per voxel, faces included:

    |got - D64| <= (n + K + 1) 2^-24 D64 + n 2^-126

n additions of positive terms, every partial sum <= the total, so each costs at most u = 2^-24 of D64; K u is the relative error of one term
(one rounding of the product plus the error of the hardware exp2); + 1 covers second order for n <= 4000; the last term the flush of
subnormal terms. K is not an estimate: tests/test_bhte_dose_term_gpu.py measures one term against float64 at EVERY float32 temperature of
[21.5, 86] and holds the maximum to the constant below. Derived, not fitted to a result: a dose beyond the bound is a finding about the kernel.
tests/test_bhte_dose_bound_host.py shows which faults the bound finds and which of them the former whole-array relative L2 let pass."""
import numpy as np

from oracle import bhte_oracle as BO
from tests.util import rel_l2

U = 2.0 ** -24                  # half a float32 ulp, relative
FLUSH = 2.0 ** -126             # the smallest normal float32
# Relative error of one dose term fl(dtMin * v_exp_f32(x)) in units of U, against float64. Measured over all 16 777 217 float32 temperatures of
# [T_LO, T_HI] on gfx950 (test_bhte_dose_term_gpu.py prints it and holds it to K): 2.0144 u with dt = 0.02 (at T = 21.5311947), 2.1689 u with
# dt = 0.1 (at T = 21.6241207), mean 0.49 u: one rounding of the product (1 u) and 1 ulp of v_exp_f32. K is the smallest integer not below the
# maximum; no margin, the measurement is exhaustive and the instruction deterministic.
K = 3
N_MAX = 4000                    # (1 + u)^(n + K) - 1 <= (n + K + 1) u up to here
T_LO, T_HI = 21.5, 86.0         # one binade below and above 43: 43 - T is exact in float32


def term64(T, dt):
    """One step's dose increment in float64 from a float32 temperature: float64(float32(dt/60)) 2^(-b (43 - T))."""
    T = np.asarray(T)
    assert T.dtype == np.float32
    e = 43.0 - T.astype(np.float64)
    return float(np.float32(dt / 60.0)) * np.exp2(np.where(T >= np.float32(43.0), -e, -2.0 * e))


class History:
    """steps[s] = float32 temperature after step s (n, N1, N2, N3); T0, dose0, dt as given; mat for the messages."""

    def __init__(self, steps, T0, dose0, dt, mat):
        self.steps, self.T0, self.dose0, self.dt, self.mat = steps, T0, dose0, dt, mat
        self.n = len(steps)

    @property
    def T(self):
        return self.steps[-1] if self.n else self.T0

    def at_boundary(self, b):
        """the state after b steps (b = 0: the start)"""
        return self.T0 if b == 0 else self.steps[b - 1]

    def dose64(self, upto=None):
        """D64 after `upto` steps (default: all of them)"""
        D = self.dose0.astype(np.float64)
        for s in range(self.n if upto is None else int(upto)):
            D = D + term64(self.steps[s], self.dt)
        return D

    def plane(self, sl, fm):
        """the monitored plane as the solver returns it: (N1, N3, samples), sample m = T[:, sl, :] after step m fm"""
        return np.ascontiguousarray(self.steps[::fm, :, sl, :].transpose(1, 2, 0))

    def points(self, where):
        """(points, steps): the temperature after every step at the voxels `where` = [(i, j, k), ...]"""
        return np.ascontiguousarray(np.stack([self.steps[:, i, j, k] for i, j, k in where]))

    def running_max(self, boundaries):
        """max over the states at the step boundaries (the Tmax of a protocol run)"""
        out = self.at_boundary(int(boundaries[0])).copy()
        for b in boundaries[1:]:
            out = np.maximum(out, self.at_boundary(int(b)))
        return out


def history(T0, dose0, q, mat, cd, cp, Tcore, dt, field_of_step):
    """The oracle's temperature after every step of field_of_step (BO.bhte_steps; q (nFields, N1, N2, N3), or (N1, N2, N3) for one field),
    kept whole: the grids of the suite are small. Refuses a temperature outside [T_LO, T_HI], where the dose reference would no longer
    exponentiate the device's argument."""
    T0 = np.array(T0, np.float32)
    q = np.asarray(q, np.float32)
    if q.ndim == 3:
        q = q[None]
    sched = [int(f) for f in field_of_step]
    assert len(sched) <= N_MAX, 'history: %d steps, the dose bound holds up to %d' % (len(sched), N_MAX)
    steps = np.empty((len(sched),) + T0.shape, np.float32)
    for s, T in enumerate(BO.bhte_steps(T0, q, mat, cd, cp, Tcore, sched)):
        lo, hi = float(T.min()), float(T.max())
        if not (lo >= T_LO and hi <= T_HI):           # a NaN fails too
            raise AssertionError('history: temperature %.9g .. %.9g after step %d lies outside [%g, %g]: choose inputs that stay inside' % (lo, hi, s, T_LO, T_HI))
        steps[s] = T
    return History(steps, T0, np.array(dose0, np.float32), dt, np.asarray(mat))


def points_of(mpm):
    """[(i, j, k)] of a MonitoringPointsMap in the order of the rows of the point series (ascending point id)"""
    mpm = np.asarray(mpm)
    idx = np.argwhere(mpm)
    return [tuple(int(v) for v in idx[r]) for r in np.argsort(mpm[mpm != 0], kind='stable')]


def dose_bound(D64, n):
    return (n + K + 1) * U * D64 + n * FLUSH


def assert_dose(got, D64, n, what, T=None, mat=None):
    """got (float32 dose of the device) against D64 after n steps: every voxel finite, >= 0 and within dose_bound. T (the final temperature) and
    mat (material ids) only serve the message. Returns the largest |got - D64| / bound, for the record."""
    got, D64 = np.asarray(got), np.asarray(D64)
    n = int(n)
    assert 0 <= n <= N_MAX, '%s: %d steps, the bound holds up to %d' % (what, n, N_MAX)
    assert got.shape == D64.shape, '%s: shape %s against %s' % (what, got.shape, D64.shape)
    assert got.dtype == np.float32 and D64.dtype == np.float64, '%s: dtypes %s / %s, expected float32 / float64' % (what, got.dtype, D64.dtype)
    assert np.isfinite(D64).all() and (D64 >= 0).all(), '%s: the reference itself is not a dose' % what

    def where(idx):
        idx = tuple(int(v) for v in idx)
        s = '(i, j, k) = (%d, %d, %d)' % idx if len(idx) == 3 else 'index %s' % (idx,)
        if T is not None:
            s += ', T %.9g' % float(np.asarray(T)[idx])
        if mat is not None:
            s += ', material %d' % int(np.asarray(mat)[idx])
        return s
    bad = ~np.isfinite(got) | (got < 0)
    if bad.any():
        first = np.unravel_index(int(np.flatnonzero(bad)[0]), got.shape)
        raise AssertionError('%s: %d of %d voxels (%.4g %%) hold no dose (non-finite or negative), first %r (reference %.17g) at %s' % (
            what, int(bad.sum()), got.size, 100.0 * bad.sum() / got.size, float(got[first]), float(D64[first]), where(first)))
    bound = dose_bound(D64, n)
    err = np.abs(got.astype(np.float64) - D64)
    ratio = np.divide(err, bound, out=np.where(err > 0, np.inf, 0.0), where=bound > 0)
    out = ratio > 1.0
    if out.any():
        def one(name, idx):
            return '%s: got %.9g, reference %.17g, %.4g x the bound at %s' % (name, float(got[idx]), float(D64[idx]), float(ratio[idx]), where(idx))
        first = np.unravel_index(int(np.flatnonzero(out)[0]), got.shape)
        worst = np.unravel_index(int(np.argmax(ratio)), got.shape)
        raise AssertionError('%s: %d of %d voxels outside the dose bound (%.4g %%) after %d steps; %s; %s; whole-array rel L2 %.3e' % (
            what, int(out.sum()), got.size, 100.0 * out.sum() / got.size, n, one('first', first), one('worst', worst), rel_l2(got, D64)))
    return float(ratio.max()) if ratio.size else 0.0


def assert_equal(got, ref, what, axes=None, mat=None):
    """got == ref in value, element by element (float32 both, finite both; +0 == -0), like tests.util.assert_same, with the index named by
    `axes`: 'ijk' a volume, 'ikm' a monitored plane (i, k, sample), 'ps' a point series (point, step)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, '%s: shape %s against %s' % (what, got.shape, ref.shape)
    assert got.dtype == np.float32 and ref.dtype == np.float32, '%s: dtypes %s / %s, expected float32' % (what, got.dtype, ref.dtype)
    names = {'ijk': '(i, j, k)', 'ikm': '(i, k, sample)', 'ps': '(point, step)'}.get(axes, 'index')

    def where(idx):
        idx = tuple(int(v) for v in idx)
        s = '%s = %s' % (names, idx)
        if mat is not None and axes == 'ijk':
            s += ', material %d' % int(np.asarray(mat)[idx])
        return s
    for side, a in (('result', got), ('reference', ref)):
        bad = ~np.isfinite(a)
        if bad.any():
            first = np.unravel_index(int(np.flatnonzero(bad)[0]), a.shape)
            raise AssertionError('%s: %d non-finite element(s) in the %s, first %r at %s' % (what, int(bad.sum()), side, float(a[first]), where(first)))
    diff = got != ref
    if not diff.any():
        return
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    first = np.unravel_index(int(np.flatnonzero(diff)[0]), got.shape)
    worst = np.unravel_index(int(np.argmax(err)), got.shape)

    def one(name, idx):
        return '%s: got %.9g, expected %.9g at %s' % (name, float(got[idx]), float(ref[idx]), where(idx))
    raise AssertionError('%s: %d of %d elements differ (%.4g %%); %s; %s; whole-array rel L2 %.3e' % (
        what, int(diff.sum()), got.size, 100.0 * diff.sum() / got.size, one('first', first), one('worst', worst), rel_l2(got, ref)))
