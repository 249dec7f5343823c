"""Drop-in for the reference's `GPUFunctions.GPUMedianFilter.MedianFilter` (BabelBrain/CalculateMaskProcess.py:42-70 imports it, calls
InitMedianFilter and hands MedianFilter to BabelDatasetPreps.InitMedianGPUCallback), and for the scipy.ndimage.median_filter call of
Step 3 (ThermalModeling/CalculateTemperatureEffects.py:908-918):

    InitMedianFilter(DeviceName, GPUBackend)                      CalculateMaskProcess.py:64
    MedianFilter(data, size, GPUBackend=...)                      BabelDatasetPreps.py:876, 1053, 1072 (uint8, sizes 7 and 3)
    median_in_region(volume, region, size=3)                      CalculateTemperatureEffects.py:911-913 and :915-918 in one call

The filter runs on the MI355X through the C ABI (bfd_median_filter3d, csrc/bfd_median.hip); there is no CPU fallback. The output is the
element of rank n // 2 of each window, one of the window's values with its bits unchanged (float32 denormals included; where a window
holds both -0.0 and +0.0 either may come out). Behaviour on NaN is undefined. Argument errors are raised before the library is loaded.
"""
import ctypes as C
import operator

import numpy as np

from . import _engine, _step1

_device = 0
last_kernel_ms = None
_MODES = {'reflect': 0, 'constant': 1}
MAX_SIZE = 7               # per axis, the reference's limit


def InitMedianFilter(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as RayleighAndBHTE's Init* functions do. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


def _sizes(size):
    """(s1, s2, s3) from an int or a 3-sequence: odd, 1..7."""
    try:
        s = (operator.index(size),) * 3
    except TypeError:
        try:
            s = tuple(operator.index(v) for v in size)
        except TypeError:
            raise ValueError('size must be an int or a sequence of three ints, not %r' % (size,))
        if len(s) != 3:
            raise ValueError('size must be an int or a sequence of three ints, not %r' % (size,))
    for v in s:
        if v < 1 or v > MAX_SIZE or v % 2 == 0:
            raise ValueError('every size must be odd and between 1 and %d, not %r' % (MAX_SIZE, size))
    return s


def _checked(data, size, mode, cval, mask):
    """Everything that can be refused without the library: returns (contiguous array of uint8 or float32, sizes, mode code, cval, mask or None)."""
    a = _step1.bool_as_uint8(np.asarray(data))
    if a.dtype != np.uint8 and a.dtype != np.float32:
        raise TypeError('MedianFilter takes uint8 (or bool) and float32 volumes, not %s' % a.dtype)
    if a.ndim != 3:
        raise ValueError('MedianFilter takes a 3-D volume, not %d-D' % a.ndim)
    s = _sizes(size)
    for ax in range(3):
        if a.shape[ax] < s[ax] // 2:
            raise ValueError('axis %d has %d elements, fewer than size // 2 = %d' % (ax, a.shape[ax], s[ax] // 2))
    if mode not in _MODES:
        raise ValueError("mode must be 'reflect' or 'constant', not %r" % (mode,))
    if a.dtype == np.uint8:
        if not (0 <= cval <= 255) or cval != int(cval):
            raise ValueError('cval %r is not a uint8 value' % (cval,))
    cval = float(cval)
    m = None
    if mask is not None:
        m = np.asarray(mask)
        if m.shape != a.shape:
            raise ValueError('mask has shape %s, the volume %s' % (m.shape, a.shape))
        m = np.ascontiguousarray(m != 0).view(np.uint8)
    return np.ascontiguousarray(a), s, _MODES[mode], cval, m


def _run(a, s, mode, cval, m):
    global last_kernel_ms
    out = np.empty_like(a)
    ms = C.c_float()
    _step1.call('bfd_median_filter3d', _device, 0 if a.dtype == np.uint8 else 1, _engine._ptr(a), _engine._ptr(out), _engine._ptr(m),
                a.shape[0], a.shape[1], a.shape[2], s[0], s[1], s[2], mode, cval, C.byref(ms))
    last_kernel_ms = ms.value
    return out


def MedianFilter(data, size, GPUBackend=None, mode='reflect', cval=0, mask=None):
    """3-D median filter of a uint8 (or bool, taken and returned as uint8) or float32 volume; returns a fresh array of data's dtype and
    shape and leaves data as it was. size: an int or three ints, each 1, 3, 5 or 7. mode 'reflect' (scipy's default, the reference
    kernel's boundary) or 'constant' with cval (what the scipy fallback at BabelDatasetPreps.py:874 uses). mask: optional array of data's
    shape; the result is where(mask != 0, median, data). Every axis must have at least size // 2 elements. GPUBackend is ignored.
    TypeError for another dtype; ValueError for a bad size, mode, cval, mask shape or a volume that is not 3-D."""
    return _run(*_checked(data, size, mode, cval, mask))


def median_in_region(volume, region, size=3):
    """Step 3's smoothing of the pressure amplitude inside the skull (CalculateTemperatureEffects.py:911-913)
        pAmpSk = median_filter(pAmp.copy(), 3); pAmp[SelSkull] = pAmpSk[SelSkull]
    as one device call that returns the new volume: `volume` filtered where `region` is true, untouched elsewhere. A stack
    (nFields, N1, N2, N3) has every field filtered with the same region (:915-918)."""
    v = np.asarray(volume)
    if v.ndim == 4:
        checked = [_checked(f, size, 'reflect', 0, region) for f in v]      # all argument errors before the first device call
        out = np.empty(v.shape, checked[0][0].dtype) if checked else np.array(v, copy=True)
        for n, c in enumerate(checked):
            out[n] = _run(*c)
        return out
    return _run(*_checked(v, size, 'reflect', 0, region))
