"""One dose term of the device at EVERY float32 temperature of [21.5, 86] against float64: the measurement behind the constant K of
tests/bhte_reference.py, and the exp2 inside every fused kernel against the one-step kernel.

A 256 x 256 x 257 volume holds the 16 777 217 float32 values of [21.5, 86] as the start temperature (the rest: 37.0), one material without
conduction or perfusion, no pressure: T' = T in every cell, faces included, and the dose after one step is the single term
fl(float32(dt/60) * v_exp_f32(-b (43 - T))). Nothing is thinned: the instruction is deterministic, so the maximum found here IS the constant."""
import numpy as np
import pytest

from tests import bhte_reference as BR

pytestmark = pytest.mark.gpu

N = (256, 256, 257)
_ENV = ('BFD_BHTE_FUSE', 'BFD_BHTE_STEPS', 'BFD_BHTE_ZRUN')


@pytest.fixture(scope='module')
def every_temperature():
    lo, hi = np.float32(BR.T_LO).view(np.uint32), np.float32(BR.T_HI).view(np.uint32)
    vals = np.arange(int(lo), int(hi) + 1, dtype=np.uint32).view(np.float32)
    assert vals.size == 16777217 and vals[0] == 21.5 and vals[-1] == 86.0 and np.all(np.diff(vals) > 0)
    T0 = np.full(N[0] * N[1] * N[2], 37.0, np.float32)
    T0[:vals.size] = vals
    T0 = T0.reshape(N)
    T0.setflags(write=False)
    return T0


def _still():
    return {'Density': np.array([1041.0]), 'SoS': np.array([1562.0]), 'Attenuation': np.array([3.45]), 'SpecificHeat': np.array([3630.0]),
            'Conductivity': np.array([0.0]), 'Perfusion': np.array([0.0]), 'Absorption': np.array([0.85]), 'InitTemperature': np.array([37.0])}


@pytest.mark.parametrize('dt', [0.02, 0.1])
def test_one_term_at_every_temperature_and_the_fused_kernels_sum_it(dt, every_temperature, monkeypatch):
    from babelbrain_amd import RayleighAndBHTE as R
    T0 = every_temperature
    ml, mm, p = _still(), np.zeros(N, np.uint8), np.zeros(N, np.float32)

    def run(nSteps, nOn, **env):
        for k in _ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        T, D, _, Q = R.BHTE(p, mm, ml, 1e-3, nSteps, nOn, -1, dt=dt, initT0=T0)
        assert not Q.any()
        assert np.array_equal(T.view(np.uint32), T0.view(np.uint32)), 'the temperature moved without conduction, perfusion or heat'
        return D
    r = run(1, 0)
    assert r.dtype == np.float32 and np.isfinite(r).all() and (r > 0).all()
    ref = BR.term64(T0, dt)
    k = np.abs(r.astype(np.float64) - ref) / (BR.U * ref)
    w = np.unravel_index(int(np.argmax(k)), N)
    print('dt %g: one term against float64 at every float32 of [21.5, 86]: largest relative error %.4f u (u = 2^-24) at T = %.9g; mean %.4f u' % (
        dt, k[w], T0[w], k.mean()))
    assert k[w] <= BR.K, 'a dose term is %.4f u from float64 at T = %.9g: tests/bhte_reference.py assumes K = %d' % (k[w], T0[w], BR.K)
    # the two-branch function: the base changes at 43 and nowhere else. 2^-(43 - T) and 4^-(43 - T) are 2.6e-6 apart one float32 below 43 (44 u:
    # the bound above tells them apart there), and further apart everywhere else below; at 43 itself the term is dtMin exactly
    dtMin = np.float32(dt / 60.0)
    flat, tf = r.reshape(-1), T0.reshape(-1)
    i43 = int(np.flatnonzero(tf == np.float32(43.0))[0])
    assert flat[i43] == dtMin and flat[i43 - 1] < dtMin < flat[i43 + 1]
    wrong = float(dtMin) * np.exp2(np.where(tf >= np.float32(43.0), -2.0, -1.0) * (43.0 - tf.astype(np.float64)))       # the bases swapped
    off = tf != np.float32(43.0)
    assert np.all(np.abs(flat[off].astype(np.float64) - wrong[off]) > (BR.K + 1) * BR.U * wrong[off])
    # the exp2 of every fused kernel against the exhaustive one: four steps at constant T add the same term four times, in float32, in step order
    want = ((r + r) + r) + r
    for name, nOn, env in (('four steps per pass, nothing heats', 0, {}), ('four steps per pass, a (zero) field heats', 4, {}),
                           ('three steps per pass and one', 0, dict(BFD_BHTE_STEPS='3')), ('three per pass, heating', 4, dict(BFD_BHTE_STEPS='3')),
                           ('two steps per launch', 0, dict(BFD_BHTE_STEPS='2'))):
        D = run(4, nOn, **env)
        diff = D.view(np.uint32) != want.view(np.uint32)
        if diff.any():
            f = np.unravel_index(int(np.flatnonzero(diff)[0]), N)
            raise AssertionError('%s: %d of %d voxels differ from ((r + r) + r) + r of the one-step kernel; first: got %.9g, expected %.9g at (i, j, k) = %s, T %.9g' % (
                name, int(diff.sum()), diff.size, D[f], want[f], f, T0[f]))
