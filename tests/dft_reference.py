"""The single-bin DFT of a sensor block in plain numpy float64, and the bound a float32 result of the device is held to, sensor by sensor.

The device (dft_series, accumulate_sensor_dft and finalize_sensor_dft of bfd_outputs.hip) multiplies every float32 sample by sincospi of an
exactly reduced phase, sums the nTs products in double and converts (2/nTs) x sum to float32 once. Against the exact sum that leaves, for re and
for im of every sensor,

    2^-24 |ref|  +  2^-126  +  4 nTs 2^-53 S,        S = (2/nTs) sum_n |x[s, n]|

one float32 rounding of the result; the threshold below which that conversion may flush to zero; nTs terms accumulated in double with sin / cos
good to a few ulp. Derived, not measured: what the device reaches of it is recorded in DESIGN.md section 4, and a result beyond it is a finding
about the kernel. tests/test_dft_bound_host.py holds this file to a long-double sum and shows which faults the bound finds."""
import numpy as np

from babelbrain_amd import harness as H

ROUNDING = 2.0 ** -24           # half a float32 ulp, relative
FLUSH = 2.0 ** -126             # the smallest normal float32
ACCUMULATION = 4 * 2.0 ** -53   # per term of the double sum, relative to S


def dft_bin(nTs, d, freq):
    """The caller's rule (BASE:2498-2499): the bin of numpy's frequency table closest to freq, the first one of equals."""
    return int(np.argmin(np.abs(np.fft.fftfreq(nTs, d) - freq)))


def dft_float64(series, bin):
    """(2/nTs) sum_n x[s, n] exp(-2 pi i ((bin n) mod nTs) / nTs) as a direct sum in float64, the phase index reduced in integers.
    (Not np.fft.fft of the float32 block: numpy transforms float32 in single precision.)"""
    x = np.asarray(series).astype(np.float64)
    nTs = x.shape[1]
    r = (int(bin) * np.arange(nTs, dtype=np.int64)) % nTs
    w = np.exp(-2j * np.pi * r.astype(np.float64) / nTs)
    return (2.0 / nTs) * (x @ w)


def accumulation_term(series):
    """Third term of the bound, per sensor: 4 nTs 2^-53 S."""
    x = np.abs(np.asarray(series).astype(np.float64))
    nTs = x.shape[1]
    return ACCUMULATION * nTs * (2.0 / nTs) * x.sum(axis=1)


def dft_tolerance(series, ref):
    """(bound on re, bound on im), one value per sensor."""
    third = accumulation_term(series)
    ref = np.asarray(ref, np.complex128)
    return ROUNDING * np.abs(ref.real) + FLUSH + third, ROUNDING * np.abs(ref.imag) + FLUSH + third


def _voxel(s, sensors):
    if sensors is None:
        return ''
    index, N = sensors
    i, j, k = H.decode_sensor_index(np.asarray(index)[s:s + 1], N[0], N[1])
    return ', sensor voxel (i, j, k) = (%d, %d, %d)' % (i[0], j[0], k[0])


def assert_dft(F, peak, series, d, freq, what, sensors=None):
    """F (complex64, one value per sensor) against dft_float64 of `series` (nSensors, nTs) at dft_bin(nTs, d, freq): every sensor, re and im
    each within dft_tolerance; peak == series.max(axis=1) exactly; every value finite. sensors = (IndexSensorMap, N) lets the message name the
    voxel. Returns the largest |got - expected| / bound, for the record."""
    series = np.asarray(series)
    F, peak = np.asarray(F), np.asarray(peak)
    nS, nTs = series.shape
    assert F.shape == (nS,) and peak.shape == (nS,), '%s: shapes %s / %s for %d sensors' % (what, F.shape, peak.shape, nS)
    assert F.dtype == np.complex64 and peak.dtype == np.float32, '%s: dtypes %s / %s' % (what, F.dtype, peak.dtype)
    for name, a in (('re', F.real), ('im', F.imag), ('peak', peak)):
        bad = ~np.isfinite(a)
        if bad.any():
            s = int(np.flatnonzero(bad)[0])
            raise AssertionError('%s: %d non-finite value(s) in %s, first %r at sensor %d%s' % (what, int(bad.sum()), name, float(a[s]), s, _voxel(s, sensors)))
    want = series.max(axis=1)
    if not np.array_equal(peak, want):
        diff = peak != want
        s = int(np.flatnonzero(diff)[0])
        raise AssertionError('%s: peak differs from the largest sample at %d of %d sensors (%.4g %%); first: got %.9g, expected %.9g at sensor %d%s' % (
            what, int(diff.sum()), nS, 100.0 * diff.sum() / nS, float(peak[s]), float(want[s]), s, _voxel(s, sensors)))
    ref = dft_float64(series, dft_bin(nTs, d, freq))
    tre, tim = dft_tolerance(series, ref)
    rre = np.abs(F.real.astype(np.float64) - ref.real) / tre
    rim = np.abs(F.imag.astype(np.float64) - ref.imag) / tim
    ratio = np.maximum(rre, rim)
    worst = float(ratio.max()) if nS else 0.0
    out = ratio > 1.0
    if out.any():
        def one(name, s):
            part = 're' if rre[s] >= rim[s] else 'im'
            got = float(F.real[s] if part == 're' else F.imag[s])
            exp = float(ref.real[s] if part == 're' else ref.imag[s])
            return '%s: %s got %.9g, expected %.17g, %.4g x the bound at sensor %d%s' % (name, part, got, exp, float(ratio[s]), s, _voxel(s, sensors))
        raise AssertionError('%s: %d of %d sensors outside the bound (%.4g %%), bin %d of %d; %s; %s' % (
            what, int(out.sum()), nS, 100.0 * out.sum() / nS, dft_bin(nTs, d, freq), nTs, one('first', int(np.flatnonzero(out)[0])),
            one('worst', int(np.argmax(ratio)))))
    return worst
