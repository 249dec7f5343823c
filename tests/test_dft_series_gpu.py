"""bfd_dft_series alone (the dft_series kernel and the library's bin rule) on synthetic host series, every sensor held to the bound of
tests/dft_reference.py: series of 1 to 3380 samples, frequencies at 0, on a bin, just to either side of the middle between two bins and beyond
Nyquist, sensors scaled over sixty decades in one block, constant, all-negative and zero series, and more sensors than one launch has threads
(grid_for caps a launch at 8192 x 256: the grid-stride loop runs a second time). Inputs are zero or normal float32: a build that flushes
denormals promises nothing about them."""
import numpy as np
import pytest

from babelbrain_amd import _engine
from tests.dft_reference import ROUNDING, assert_dft, dft_bin, dft_tolerance

pytestmark = pytest.mark.gpu

D = 1e-7
LENGTHS = [1, 2, 3, 7, 8, 35, 64, 333, 3380]
TINY = np.finfo(np.float32).tiny
ONE_LAUNCH = 8192 * 256


def _normal_or_zero(x):
    x = np.asarray(x, np.float32).copy()
    x[np.abs(x) < TINY] = 0
    return x


def _low_bin(nTs):
    """a bin b >= 0 whose upper neighbour b + 1 is still a positive frequency of the table (where the series is long enough to have one)"""
    return max(0, min(nTs // 3, (nTs - 1) // 2 - 1))


# Exact ties are avoided: the library forms kk / (n d), numpy kk (1 / (n d)), and two frequencies one rounding apart may break a tie either way.
# 1e-6 of a bin to either side of the middle is ten decades above that rounding; 0.45 nTs and 0.85 nTs are no half-integers for these lengths.
FREQS = {
    'zero': lambda nTs: 0.0,
    'on a bin': lambda nTs: _low_bin(nTs) / (nTs * D),
    'below the middle': lambda nTs: (_low_bin(nTs) + 0.5 - 1e-6) / (nTs * D),
    'above the middle': lambda nTs: (_low_bin(nTs) + 0.5 + 1e-6) / (nTs * D),
    '0.9 Nyquist': lambda nTs: 0.9 * 0.5 / D,
    '1.7 Nyquist': lambda nTs: 1.7 * 0.5 / D,
}
ROWS = {'constant': 61, 'negative constant': 62, 'all negative': 63, 'zeros': 64}


def _block(nTs):
    """61 random sensors scaled 1e-30 ... 1e30 (every bin carries signal: a wrong bin is a gross miss), then a constant series, a negative
    constant, an all-negative random series and a series of zeros"""
    rng = np.random.default_rng(1000 + nTs)
    scale = 10.0 ** np.arange(-30, 31)
    x = np.zeros((65, nTs), np.float32)
    x[:61] = rng.uniform(-1, 1, (61, nTs)) * scale[:, None]
    x[61] = 3.25
    x[62] = -1.0e-3
    x[63] = -rng.uniform(0.5, 2.0, nTs)
    return _normal_or_zero(x)


@pytest.mark.parametrize('kind', list(FREQS))
@pytest.mark.parametrize('nTs', LENGTHS)
def test_every_sensor_within_the_bound(nTs, kind):
    freq = FREQS[kind](nTs)
    x = _block(nTs)
    F, pk = _engine.dft_series(x, D, freq)
    worst = assert_dft(F, pk, x, D, freq, 'nTs %d, %s' % (nTs, kind))
    print('nTs %d, %s (bin %d): largest ratio to the bound %.4f' % (nTs, kind, dft_bin(nTs, D, freq), worst))
    z = ROWS['zeros']
    assert F[z] == 0 and pk[z] == 0                                        # exactly
    assert pk[ROWS['all negative']] < 0 and pk[ROWS['negative constant']] == np.float32(-1.0e-3)
    assert np.abs(F[:61]).min() > 0
    if kind == 'below the middle' and nTs >= 7:                            # the two sides of the middle are two bins
        assert dft_bin(nTs, D, FREQS['above the middle'](nTs)) == dft_bin(nTs, D, freq) + 1


@pytest.mark.parametrize('nTs', [7, 8, 35, 64, 333, 3380])
def test_a_tone_on_the_bin_gives_its_amplitude_and_phase(nTs):
    """x[n] = A cos(2 pi b n / nTs + phi) with 0 < b < nTs / 2: F = A exp(i phi). The samples reach the device rounded to float32 once, which
    moves F by at most (2/nTs) sum |x[n]| 2^-24; that is added to the bound of the DFT itself."""
    b = nTs // 5 + 1
    assert 0 < b < nTs / 2
    freq = b / (nTs * D)
    A = np.array([1.0, 1e-20, 3e20, 7.5, 0.125, 2.0])
    phi = np.array([0.0, 0.3, -2.0, np.pi / 2, 3.0, -np.pi / 4])
    exact = A[:, None] * np.cos(2 * np.pi * b * np.arange(nTs)[None, :] / nTs + phi[:, None])
    x = _normal_or_zero(exact)
    F, pk = _engine.dft_series(x, D, freq)
    assert_dft(F, pk, x, D, freq, 'tone, nTs %d' % nTs)
    want = A * np.exp(1j * phi)
    tre, tim = dft_tolerance(x, want)
    inputs = ROUNDING * (2.0 / nTs) * np.abs(x.astype(np.float64)).sum(axis=1)
    assert np.all(np.abs(F.real - want.real) <= tre + inputs), (F, want)
    assert np.all(np.abs(F.imag - want.imag) <= tim + inputs), (F, want)


@pytest.mark.parametrize('nSensors,nTs,freq', [(1, 35, 5 / (35 * D)), (255, 35, 5 / (35 * D)), (257, 35, 5 / (35 * D)),
                                                (ONE_LAUNCH + 257, 2, -0.4 / D)])
def test_sensor_counts_around_a_workgroup_and_past_one_launch(nSensors, nTs, freq):
    """1, 255 and 257 sensors; 2 097 152 + 257 sensors of two samples (16 MB in) are more than one launch has threads. With two samples the
    only bin with a phase is the one at -Nyquist, reached with a negative frequency."""
    rng = np.random.default_rng(nSensors)
    x = _normal_or_zero(rng.uniform(-1, 1, (nSensors, nTs)) * 10.0 ** rng.integers(-6, 7, (nSensors, 1)))
    if nTs == 2:
        assert dft_bin(nTs, D, freq) == 1
    F, pk = _engine.dft_series(x, D, freq)
    worst = assert_dft(F, pk, x, D, freq, '%d sensors' % nSensors)
    print('%d sensors of %d samples: largest ratio to the bound %.4f' % (nSensors, nTs, worst))


def test_refused_and_empty_calls():
    lib = _engine.load_library()
    x = np.ones((4, 8), np.float32)
    F = np.full(4, -7.5 - 7.5j, np.complex64)
    pk = np.full(4, -7.5, np.float32)

    def call(nSensors, nTs):
        return lib.bfd_dft_series(0, nSensors, nTs, _engine._ptr(x), D, 1e6, _engine._ptr(F.view(np.float32)), _engine._ptr(pk))
    assert call(4, 0) == -1 and lib.bfd_last_error().decode() == 'bfd_dft_series: bad argument'
    assert call(0, 8) == 0
    assert np.all(F == np.complex64(-7.5 - 7.5j)) and np.all(pk == np.float32(-7.5))       # the outputs are as they were
    assert call(4, 8) == 0
    assert_dft(F, pk, x, D, 1e6, 'after the refused calls')
