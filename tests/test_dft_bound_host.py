"""tests/dft_reference.py held to itself, and what its per-sensor bound sees that the whole-array norm it replaces does not.

(1) The float64 direct sum, numpy's float64 FFT and an emulation of the device's arithmetic (sequential double sum, one rounding to float32)
against a long-double direct sum, over series lengths from 1 to 3380 and sensors scaled from 1e-30 to 1e30 in one block: the two float64
references stay within the accumulation term alone, the emulation within the whole bound.
(2) Faults planted at the quietest of 64 sensors whose amplitudes span 1e-6 ... 1: assert_dft reports every one of them; rel L2 < 1e-6 on re and
on im over the block -- what test_dft_gpu.py and test_outputs_gpu.py asserted -- passes for the wrong bin, the dropped sample and the shifted
series. No GPU."""
import numpy as np
import pytest

from tests.dft_reference import accumulation_term, assert_dft, dft_bin, dft_float64, dft_tolerance
from tests.util import rel_l2

LENGTHS = [1, 2, 3, 7, 8, 35, 64, 333, 1000, 3380]
D = 1e-7
TINY = np.finfo(np.float32).tiny


def normal_or_zero(x):
    """float32 with no denormal left (the contract of a build that flushes them)"""
    x = np.asarray(x, np.float32).copy()
    x[np.abs(x) < TINY] = 0
    return x


def scaled_block(nTs, seed):
    """61 sensors, sensor s scaled by 10^(s - 30): random samples in [-1, 1) x scale"""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** np.arange(-30, 31)
    return normal_or_zero(rng.uniform(-1, 1, (scale.size, nTs)) * scale[:, None])


def dft_long_double(series, bin):
    x = np.asarray(series).astype(np.longdouble)
    nTs = x.shape[1]
    pi = 4 * np.arctan(np.longdouble(1))
    r = ((int(bin) * np.arange(nTs, dtype=np.int64)) % nTs).astype(np.longdouble)
    a = 2 * pi * r / nTs
    sc = np.longdouble(2) / nTs
    return sc * (x * np.cos(a)).sum(axis=1), -sc * (x * np.sin(a)).sum(axis=1)


def device_emulation(series, bin):
    """What dft_series does: float32 sample -> double, times cos / sin of the reduced phase, summed one after the other in double,
    times 2/nTs, rounded to float32 once. Returns (F complex64, peak float32)."""
    x = np.asarray(series, np.float32)
    nS, nTs = x.shape
    re, im = np.zeros(nS), np.zeros(nS)
    pk = np.full(nS, -np.inf, np.float32)
    for n in range(nTs):
        a = 2.0 * ((bin * n) % nTs) / nTs
        re += x[:, n].astype(np.float64) * np.cos(np.pi * a)
        im -= x[:, n].astype(np.float64) * np.sin(np.pi * a)
        pk = np.maximum(pk, x[:, n])
    F = np.empty(nS, np.complex64)
    F.real = (re * (2.0 / nTs)).astype(np.float32)
    F.imag = (im * (2.0 / nTs)).astype(np.float32)
    return F, pk


@pytest.mark.parametrize('nTs', LENGTHS)
def test_the_reference_stays_inside_its_own_bound(nTs):
    x = scaled_block(nTs, nTs)
    for freq in (0.0, 1.0 / (7 * D), 0.37 / D):
        b = dft_bin(nTs, D, freq)
        lre, lim = dft_long_double(x, b)
        third = accumulation_term(x)
        ref = dft_float64(x, b)
        fft = np.fft.fft(x.astype(np.float64), axis=1)[:, b] * 2 / nTs
        for name, got in (('direct float64 sum', ref), ('float64 FFT', fft)):
            r = max(float(np.max(np.abs(got.real - lre) / third)), float(np.max(np.abs(got.imag - lim) / third)))
            print('nTs %d bin %d, %s: %.3g of the accumulation term' % (nTs, b, name, r))
            assert r <= 1.0, (name, nTs, b, r)
        F, pk = device_emulation(x, b)
        tre, tim = dft_tolerance(x, ref)
        r = max(float(np.max(np.abs(F.real - lre) / tre)), float(np.max(np.abs(F.imag - lim) / tim)))
        print('nTs %d bin %d, device emulation against long double: %.3g of the bound' % (nTs, b, r))
        assert r <= 1.0, (nTs, b, r)
        assert assert_dft(F, pk, x, D, freq, 'device emulation, nTs %d' % nTs) <= 1.0


def test_bin_rule():
    assert dft_bin(1, D, 5e5) == 0 and dft_bin(2, D, 0.0) == 0 and dft_bin(2, D, 4.9e6) == 0 and dft_bin(3, D, 3e6) == 1
    assert dft_bin(35, D, 5 / (35 * D)) == 5
    assert dft_bin(8, D, 1.7 * 0.5 / D) == 3                  # beyond Nyquist: the last positive frequency, not the bin at -Nyquist
    assert dft_bin(64, D, 0.9 * 0.5 / D) == 29


# ---- planted faults ----
NS, NTS, BIN, Q = 64, 35, 5, 0          # the quietest sensor is sensor 0
FREQ = BIN / (NTS * D)


def _block(offset=0.0, negative=False):
    """64 sensors, amplitude 1e-6 ... 1: a tone on bin 5 at 45 degrees plus a little noise of the sensor's own, so that every bin carries signal"""
    rng = np.random.default_rng(5)
    amp = np.logspace(-6, 0, NS)
    n = np.arange(NTS)
    w = np.cos(2 * np.pi * BIN * n / NTS + np.pi / 4)[None, :] + 0.05 * rng.uniform(-1, 1, (NS, NTS)) + offset
    if negative:
        w = -np.abs(w) - 0.1
    return normal_or_zero(w * amp[:, None])


def _good(x):
    F, pk = device_emulation(x, dft_bin(NTS, D, FREQ))
    assert assert_dft(F, pk, x, D, FREQ, 'no fault') <= 1.0
    return F, pk


def _old_check_passes(F, x):
    ref = dft_float64(x, dft_bin(NTS, D, FREQ))
    er, ei = rel_l2(F.real, ref.real), rel_l2(F.imag, ref.imag)
    print('the old assertion: rel L2 re %.3g im %.3g' % (er, ei))
    return er < 1e-6 and ei < 1e-6


def _reported(F, pk, x, needle='sensor %d' % Q):
    with pytest.raises(AssertionError) as e:
        assert_dft(F, pk, x, D, FREQ, 'planted')
    msg = str(e.value)
    assert needle in msg, msg
    return msg


def _wrong_bin(x):
    return device_emulation(x[Q:Q + 1], BIN + 1)[0][0]


def _sample_dropped(x):
    y = x[Q:Q + 1].copy()
    y[0, 17] = 0
    assert x[Q, 17] != 0
    return device_emulation(y, BIN)[0][0]


def _shifted(x):
    return device_emulation(np.roll(x[Q:Q + 1], 1, axis=1), BIN)[0][0]


@pytest.mark.parametrize('fault', [_wrong_bin, _sample_dropped, _shifted])
def test_faults_at_the_quietest_sensor_that_the_norm_does_not_see(fault):
    x = _block()
    F, pk = _good(x)
    assert _old_check_passes(F, x)
    F[Q] = fault(x)
    assert _old_check_passes(F, x)                  # what the old assertion could not see
    msg = _reported(F, pk, x)
    assert '1 of %d sensors outside the bound' % NS in msg and 'x the bound' in msg


def test_im_with_the_other_sign():
    x = _block()
    F, pk = _good(x)
    F[Q] = np.conj(F[Q])
    assert ': im got' in _reported(F, pk, x)


def test_factor_two_over_n_plus_one():
    x = _block()
    F, pk = _good(x)
    F[Q] = np.complex64(F[Q] * (NTS / (NTS + 1.0)))
    _reported(F, pk, x)
    F, pk = _good(x)
    F = (F * np.float32(NTS / (NTS + 1.0))).astype(np.complex64)              # and at every sensor
    assert '%d of %d sensors' % (NS, NS) in _reported(F, pk, x, 'sensor')


def test_peak_of_the_magnitude():
    x = _block(offset=-0.5)
    F, pk = _good(x)
    assert np.abs(x[Q]).max() != x[Q].max()
    pk[Q] = np.abs(x[Q]).max()
    assert 'peak differs' in _reported(F, pk, x)


def test_peak_that_starts_at_zero_on_a_negative_series():
    x = _block(negative=True)
    assert (x < 0).all()
    F, pk = _good(x)
    assert pk[Q] < 0
    pk[Q] = max(np.float32(0), pk[Q])
    msg = _reported(F, pk, x)
    assert 'peak differs' in msg and 'got 0,' in msg


def test_message_names_the_voxel_and_non_finite_values_are_refused():
    x = _block()
    F, pk = _good(x)
    N = (8, 4, 2)
    index = np.arange(1, NS + 1, dtype=np.uint32)
    F[13] = np.complex64(F[13] * 1.001)
    with pytest.raises(AssertionError, match=r'sensor 13, sensor voxel \(i, j, k\) = \(5, 1, 0\)'):
        assert_dft(F, pk, x, D, FREQ, 'planted', sensors=(index, N))
    F, pk = _good(x)
    F[3] = np.nan
    with pytest.raises(AssertionError, match='non-finite'):
        assert_dft(F, pk, x, D, FREQ, 'planted')
    with pytest.raises(AssertionError, match='shapes'):
        assert_dft(F[:-1], pk, x, D, FREQ, 'planted')
    with pytest.raises(AssertionError, match='dtypes'):
        assert_dft(F.astype(np.complex128), pk, x, D, FREQ, 'planted')
