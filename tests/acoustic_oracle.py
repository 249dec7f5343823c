"""Result packing restated in numpy, statement by statement as the caller of the reference writes it: CalculatePhaseData's FFT, bin pick and
scatter (BASE:2498-2520; harness.phase_maps), the dispersion scaling of RUN_SIMULATION (BASE:2433-2456), and ReturnResults' zero / crop / paste /
flip (BASE:2729-2885; results.zero_up_to_source, Crop.inner, paste_and_flip). What bfd_pack_results computes on the device is held to pack()
here; pack() itself is held to the reference's own vectors by tests/test_acoustic_host.py. NumPy >= 2 semantics (a Python float or a float64
scalar does not widen a float32 array; the product with a float64 SCALAR is still formed in float64 and rounded once)."""
import numpy as np

from babelbrain_amd import harness as H, results as R


def series_dft(series, dt_sensor, freq):
    """(F, peak) per sensor of a (nSensors, nTs) series, BASE:2498-2520: the FFT bin closest to freq times 2 / nTs, and the largest sample."""
    series = np.asarray(series)
    nTs = series.shape[1]
    freqs = np.fft.fftfreq(nTs, dt_sensor)
    ind = int(np.argmin(np.abs(freqs - freq)))
    F = (np.fft.fft(series, axis=1)[:, ind] * 2 / nTs).astype(np.complex64)
    return F, series.max(axis=1)


def scale_amp(a, correction):
    """BASE:2440 on the float32 map: in place, the factor is a float64 scalar."""
    a *= correction * np.sqrt(2)
    return a


def scale_sensor(a, correction):
    """BASE:2517-2520 with the factor folded in: complex64 or float32 array times a Python float, in place."""
    a *= float(correction)
    return a


def pack(F, peak, index, rms, N, lo, hi, zsrc, O=None, at=(0, 0, 0), flipK=True, correction=None, scale_amp=scale_amp):
    """-> (p_amp float32, p_complex complex64, peak float32), each of shape O in C order.
    F, peak: per-sensor values in the order of index (1-based x-fastest IndexSensorMap); rms: the Pressure RMS map (N1, N2, N3), not modified;
    lo / hi: the Crop offsets (hi >= 1, as the reference slices with -offset); O / at: shape of the zero volume the kept region is pasted into and
    where (default: the kept size at 0, which is DataForSim; the mask's shape at the shrinks is paste_and_flip); correction None: no scaling."""
    N1, N2, N3 = N
    four, _, pk = H.phase_maps(np.asarray(F, np.complex64), np.asarray(peak, np.float32), index, N1, N2, N3)
    amp = np.array(rms, np.float32)
    assert amp.shape == (N1, N2, N3)
    if correction is not None:
        scale_amp(amp, correction)
        scale_sensor(four, correction)
        scale_sensor(pk, correction)
    crop = R.Crop(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], *at)
    if O is None:
        O = crop.inner(amp).shape
    out = []
    for a, dt in ((amp, np.float32), (four, np.complex64), (pk, np.float32)):
        R.zero_up_to_source(a, zsrc)
        o = R.paste_and_flip(a, crop, tuple(O), dt)
        out.append(np.ascontiguousarray(o if flipK else np.flip(o, axis=2)))
    return tuple(out)
