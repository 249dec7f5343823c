"""Gaussian filter on the device: the drop-in for the `scipy.ndimage.gaussian_filter` calls of the bone-rim partial-volume correction
(BabelBrain/BabelDatasetPreps.py:984 and :986, bMaximizeBoneRim), float32 CT values and a float32 mask at sigma_local:

    InitGaussianFilter(DeviceName)
    gaussian_filter(interior_f, sigma=sigma_local)                :984
    gaussian_filter(interior_mask_val.astype(np.float32), sigma=sigma_local)      :986

The filter runs on the MI355X through the C ABI (bfd_gaussian_filter3d, csrc/bfd_distance.hip); there is no CPU fallback. scipy's weights, edge
rules, order of the axes and of every sum, float64 sums rounded to the volume's dtype once per axis. Argument errors are raised before the library is
loaded.
"""
import ctypes as C
import math
import operator

import numpy as np

from . import _engine, _step1

_device = 0
last_kernel_ms = None
_MODES = {'reflect': 0, 'constant': 1, 'nearest': 2, 'mirror': 3}
MAX_RADIUS = 127           # per axis


def InitGaussianFilter(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as RayleighAndBHTE's Init* functions do. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


def gaussian_filter(input, sigma, order=0, mode='reflect', cval=0.0, truncate=4.0, GPUBackend=None):
    """scipy.ndimage.gaussian_filter(input, sigma, order=0, mode=mode, cval=cval, truncate=truncate) of a float32 or float64 3-D volume; returns a
    fresh array of input's dtype and shape. sigma: a scalar or three values; an axis with sigma <= 1e-15 is not filtered. mode 'reflect' (scipy's
    default), 'constant' with cval, 'nearest' or 'mirror', for any ratio of radius to axis length. The radius int(truncate * sigma + 0.5) is at most
    127 per axis. GPUBackend is ignored. NotImplementedError for a non-zero order, for 'wrap' and the other modes and for one mode per axis; TypeError
    for another dtype (scipy would convert; here the caller says what precision it wants); ValueError for a volume that is not 3-D, a sigma or
    truncate that is negative or not finite, or a radius above 127."""
    global last_kernel_ms
    try:
        zero_order = operator.index(order) == 0
    except TypeError:
        zero_order = all(operator.index(o) == 0 for o in order)
    if not zero_order:
        raise NotImplementedError('gaussian_filter takes order 0 only, not %r' % (order,))
    if not isinstance(mode, str) or mode not in _MODES:
        raise NotImplementedError("mode must be 'reflect', 'constant', 'nearest' or 'mirror', not %r" % (mode,))
    a = np.asarray(input)
    if a.dtype != np.float32 and a.dtype != np.float64:
        raise TypeError('gaussian_filter takes float32 and float64 volumes, not %s' % a.dtype)
    if a.ndim != 3:
        raise ValueError('gaussian_filter takes a 3-D volume, not %d-D' % a.ndim)
    s = np.asarray(sigma, np.float64)
    if s.ndim > 1 or (s.ndim == 1 and s.size != 3):
        raise ValueError('sigma must be a scalar or three values, not %r' % (sigma,))
    s = np.ascontiguousarray(np.broadcast_to(s, (3,)))
    if not (np.isfinite(s).all() and (s >= 0).all()):
        raise ValueError('every sigma must be finite and not negative, not %r' % (sigma,))
    truncate = float(truncate)
    if not (math.isfinite(truncate) and truncate >= 0):
        raise ValueError('truncate must be finite and not negative, not %r' % (truncate,))
    for v in s:
        if v > 1e-15 and not truncate * v + 0.5 < MAX_RADIUS + 1:
            raise ValueError('the radius int(truncate * sigma + 0.5) must be at most %d; sigma %r, truncate %r' % (MAX_RADIUS, sigma, truncate))
    a = np.ascontiguousarray(a)
    out = np.empty_like(a)
    ms = C.c_float()
    _step1.call('bfd_gaussian_filter3d', _device, 1 if a.dtype == np.float32 else 3, _engine._ptr(a), _engine._ptr(out), a.shape[0], a.shape[1],
                a.shape[2], s.ctypes.data_as(C.POINTER(C.c_double)), truncate, _MODES[mode], float(cval), C.byref(ms))
    last_kernel_ms = ms.value
    return out
