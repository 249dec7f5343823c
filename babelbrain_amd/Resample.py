"""Drop-in for the reference's `GPUFunctions.GPUResample.Resample` (BabelBrain/CalculateMaskProcess.py:65-74 imports it, calls InitResample
and hands ResampleFromTo to BabelDatasetPreps / CTZTEProcessing), and for the scipy.ndimage calls underneath it:

    InitResample(DeviceName, GPUBackend)                                     CalculateMaskProcess.py:66
    ResampleFromTo(from_img, to_vox_map, order, mode, cval, out_class, GPUBackend)
                                                                             BabelDatasetPreps.py:859 (CT, order 3, cval = min), :1168 (T1, order 0),
                                                                             CTZTEProcessing.py:258
    affine_transform(input, matrix, offset, output_shape, order, mode, cval, prefilter)      scipy.ndimage's, 3-D
    spline_filter(input, order, mode)                                        scipy.ndimage's, 3-D, float64 result

The work runs on the MI355X through the C ABI (bfd_affine_transform3d, bfd_spline_filter3d; csrc/bfd_resample.hip); there is no CPU
fallback. All arithmetic is float64 and the result is rounded once, as scipy does: a float32 input gives what scipy gives for the same input
as float64, cast to float32. Argument errors are raised before the library is loaded. nibabel is not needed: an image is any object with
`shape`, `affine`, `dataobj` and `header`.
"""
import ctypes as C
import operator

import numpy as np

from . import _engine, _step1
from .nifti import SpatialImage

_device = 0
last_kernel_ms = None            # device time of the last call's kernels
last_prefilter_ms = None         # ... of the prefilter alone (affine_transform)
last_interpolation_ms = None     # ... of the interpolation alone
_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.float32): 1, np.dtype(np.int16): 2, np.dtype(np.float64): 3}
_MODES = {'constant': 0, 'nearest': 1, 'mirror': 2}
_OTHER_MODES = ('reflect', 'wrap', 'grid-constant', 'grid-wrap', 'grid-mirror')
_LIMIT = 1 << 31


def InitResample(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as InitMedianFilter does. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


def _order(order):
    try:
        o = operator.index(order)
    except TypeError:
        raise ValueError('order must be an integer from 0 to 3, not %r' % (order,))
    if o in (4, 5):
        raise NotImplementedError('spline orders 4 and 5 are not implemented on the device')
    if o < 0 or o > 5:
        raise ValueError('order must be an integer from 0 to 3, not %r' % (order,))
    return o


def _mode(mode):
    if mode in _MODES:
        return _MODES[mode]
    if mode in _OTHER_MODES:
        raise NotImplementedError("mode %r is not implemented on the device (only 'constant', 'nearest' and 'mirror')" % (mode,))
    raise ValueError("mode must be 'constant', 'nearest' or 'mirror', not %r" % (mode,))


def _volume(input, what):
    a = np.asarray(input)
    if a.dtype not in _DTYPES:
        raise TypeError('%s takes float32, float64, int16 and uint8 volumes, not %s' % (what, a.dtype))
    if a.ndim != 3:
        raise ValueError('%s takes a 3-D volume, not %d-D' % (what, a.ndim))
    if a.size >= _LIMIT:
        raise ValueError('the input has 2^31 voxels or more')
    return np.ascontiguousarray(a)


def normalize_matrix(matrix, offset=0.0):
    """scipy's four forms of the map -> the twelve doubles of the C ABI, a (3, 4) array whose row a is (m_a0, m_a1, m_a2, offset_a):
    (3, 3) with `offset`; (3,) as a diagonal with `offset`; (3, 4) and (4, 4) homogeneous, whose last column is the offset (`offset` is
    ignored, as in scipy; the last row of a (4, 4) must be 0 0 0 1)."""
    m = np.asarray(matrix, np.float64)
    out = np.zeros((3, 4), np.float64)
    if m.shape in ((3, 4), (4, 4)):
        if m.shape == (4, 4) and not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError('the last row of a homogeneous (4, 4) matrix must be (0, 0, 0, 1)')
        out[:] = m[:3]
    else:
        if m.shape == (3, 3):
            out[:, :3] = m
        elif m.shape == (3,):
            out[:, :3] = np.diag(m)
        else:
            raise ValueError('matrix must have shape (3, 3), (3,), (3, 4) or (4, 4), not %s' % (m.shape,))
        off = np.asarray(offset, np.float64)
        if off.ndim == 0:
            off = np.full(3, float(off))
        if off.shape != (3,):
            raise ValueError('offset must be a scalar or have three elements, not shape %s' % (off.shape,))
        out[:, 3] = off
    if not np.all(np.isfinite(out)):
        raise ValueError('matrix and offset must be finite')
    return out


def _shape3(output_shape, default):
    if output_shape is None:
        return tuple(default)
    try:
        s = tuple(operator.index(v) for v in output_shape)
    except TypeError:
        raise ValueError('output_shape must be three integers, not %r' % (output_shape,))
    if len(s) != 3 or min(s) < 0:
        raise ValueError('output_shape must be three integers that are not negative, not %r' % (output_shape,))
    if s[0] * s[1] * s[2] >= _LIMIT:
        raise ValueError('the output has 2^31 voxels or more')
    return s


def _checked(input, matrix, offset, output_shape, order, mode, cval):
    """Everything that can be refused without the library."""
    a = _volume(input, 'affine_transform')
    o, mc = _order(order), _mode(mode)
    m = normalize_matrix(matrix, offset)
    shape = _shape3(output_shape, a.shape)
    cval = float(cval)
    if a.dtype.kind in 'iu' and not np.isfinite(cval):
        raise NotImplementedError('a cval that is not finite cannot be stored in %s' % a.dtype)
    if a.size == 0 and shape[0] * shape[1] * shape[2]:
        raise ValueError('the input is empty')
    return a, m, shape, o, mc, cval


def affine_transform(input, matrix, offset=0.0, output_shape=None, order=3, mode='constant', cval=0.0, prefilter=True, *, _gathered=False):
    """scipy.ndimage.affine_transform for 3-D volumes on the device: output voxel o takes the input at `matrix @ o + offset`.
    input: float32, float64, int16 or uint8, any strides; it is left as it was. matrix: (3, 3), (3,) as a diagonal, (3, 4), or (4, 4) whose
    last column is the offset. order 0-3 (4 and 5: NotImplementedError); mode 'constant' (cval where a coordinate is below 0 or above
    dim - 1), 'nearest' or 'mirror' (every other scipy mode: NotImplementedError); prefilter as in scipy.
    Returns a fresh C-order array of the input's dtype and of output_shape (default: the input's). Values are computed in float64 and
    converted once. Integer dtypes take scipy's conversion: trunc(t + 0.5) for t > 0, trunc(t - 0.5) otherwise -- half-way cases go away
    from zero, 2.5 -> 3, -2.5 -> -3 -- then saturation to the dtype's range; uint8 gives 0 for every t <= 0 (so cval = -1000 is stored
    as 0). A cval that is not finite raises NotImplementedError for integer dtypes. There is no `output=` argument.
    A (3,) matrix is taken as its diagonal: scipy evaluates that form as (o + offset / m) * m, which can differ from m * o + offset in the
    last bit of a coordinate. _gathered=True (checks and timing) keeps order 3 off the LDS-staged path; the result has the same bits."""
    global last_kernel_ms, last_prefilter_ms, last_interpolation_ms
    a, m, shape, o, mc, cval = _checked(input, matrix, offset, output_shape, order, mode, cval)
    out = np.empty(shape, a.dtype)
    ms = (C.c_float * 2)()
    _step1.call('bfd_affine_transform3d', _device, _DTYPES[a.dtype], _engine._ptr(a), _engine._ptr(out), a.shape[0], a.shape[1], a.shape[2],
                shape[0], shape[1], shape[2], _engine._ptr(m), o, mc, cval, (1 if prefilter else 0) | (2 if _gathered else 0), ms)
    last_prefilter_ms, last_interpolation_ms = ms[0], ms[1]
    last_kernel_ms = ms[0] + ms[1]
    return out


def spline_filter(input, order=3, mode='mirror'):
    """scipy.ndimage.spline_filter(input, order, output=numpy.float64, mode) for a 3-D volume: the B-spline coefficients that
    affine_transform(..., prefilter=False) interpolates. Orders 0 and 1 return the input as float64."""
    global last_kernel_ms
    a = _volume(input, 'spline_filter')
    o, mc = _order(order), _mode(mode)
    out = np.empty(a.shape, np.float64)
    ms = C.c_float()
    _step1.call('bfd_spline_filter3d', _device, _DTYPES[a.dtype], _engine._ptr(a), _engine._ptr(out), a.shape[0], a.shape[1], a.shape[2], o, mc, C.byref(ms))
    last_kernel_ms = ms.value
    return out


def vox2vox(from_affine, to_affine):
    """The map from output voxels to input voxels, inv(from_affine) @ to_affine, split into (matrix (3, 3), offset (3,)) as
    GPUResample/Resample.py:307-309 does."""
    A, B = np.asarray(from_affine, np.float64), np.asarray(to_affine, np.float64)
    if A.shape != (4, 4) or B.shape != (4, 4):
        raise ValueError('affines must be 4 x 4, not %s and %s' % (A.shape, B.shape))
    T = np.linalg.inv(A) @ B
    return T[:3, :3].copy(), T[:3, 3].copy()


def _target(to_vox_map):
    """(shape, affine) of a target given as an image or as a (shape, affine) pair."""
    if hasattr(to_vox_map, 'shape') and hasattr(to_vox_map, 'affine'):
        shape, affine = to_vox_map.shape, to_vox_map.affine
    else:
        try:
            shape, affine = to_vox_map
        except (TypeError, ValueError):
            raise ValueError('to_vox_map must be an image or a (shape, affine) pair')
    shape = tuple(operator.index(v) for v in shape)
    affine = np.array(affine, np.float64)
    if affine.shape != (4, 4):
        raise ValueError('the target affine must be 4 x 4, not %s' % (affine.shape,))
    return shape, affine


def ResampleFromTo(from_img, to_vox_map, order=3, mode='constant', cval=0.0, out_class=None, GPUBackend=None):
    """nibabel.processing.resample_from_to on the device: `from_img` (any object with shape, affine, dataobj and header) resampled onto the
    grid of `to_vox_map`, an image or a (shape, affine) pair. Returns out_class(data, to_affine, from_img.header); with out_class=None a
    babelbrain_amd.nifti.SpatialImage. data has the dtype of from_img.dataobj. 3-D only (4-D: NotImplementedError). GPUBackend is ignored."""
    shape, to_affine = _target(to_vox_map)
    if len(from_img.shape) == 4 or len(shape) == 4:
        raise NotImplementedError('4-D images are not implemented on the device')
    if len(from_img.shape) != 3 or len(shape) != 3:
        raise ValueError('ResampleFromTo takes 3-D images, not %d-D onto %d-D' % (len(from_img.shape), len(shape)))
    matrix, offset = vox2vox(from_img.affine, to_affine)
    data = affine_transform(np.asarray(from_img.dataobj), matrix, offset, shape, order, mode, cval)
    return (SpatialImage if out_class is None else out_class)(data, to_affine, from_img.header)
