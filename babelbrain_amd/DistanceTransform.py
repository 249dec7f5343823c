"""Exact Euclidean distance transform on the device: the drop-in for the `scipy.ndimage.distance_transform_edt` call of the bone-rim partial-volume
correction (BabelBrain/BabelDatasetPreps.py:964-967, bMaximizeBoneRim):

    InitDistanceTransform(DeviceName)
    distance_transform_edt(interior_mask, invert=True)            :964-967, without the `1 - mask` pass on the host

The transform runs on the MI355X through the C ABI (bfd_distance_transform_edt3d, csrc/bfd_distance.hip); there is no CPU fallback. It works in
integers throughout, so the squared distances are exact and the float64 result equals scipy's element for element. Argument errors are raised before
the library is loaded.
"""
import ctypes as C

import numpy as np

from . import _engine, _step1

_device = 0
last_kernel_ms = None
MAX_DIM = 16384            # per axis: 3 (N - 1)^2 stays within int32


def InitDistanceTransform(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as RayleighAndBHTE's Init* functions do. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


def distance_transform_edt(input, sampling=None, return_distances=True, return_indices=False, invert=False, squared=False, GPUBackend=None):
    """For every voxel of a 3-D volume the Euclidean distance, in voxels, to the nearest BACKGROUND voxel: input == 0, or input != 0 with invert=True
    (what scipy gives for `input == 0`). Any bool, integer or float array is read as input != 0. Returns float64, equal to
    scipy.ndimage.distance_transform_edt element for element, or with squared=True the exact int32 squared distances. GPUBackend is ignored.
    NotImplementedError for a sampling other than None or all ones and for return_indices; ValueError for a volume that is not 3-D, has an axis above
    16384, has no background voxel (scipy's result there is not a distance), or for return_distances=False; TypeError for another dtype."""
    global last_kernel_ms
    if sampling is not None and not np.all(np.asarray(sampling, np.float64) == 1.0):
        raise NotImplementedError('distance_transform_edt takes unit sampling only, not %r' % (sampling,))
    if return_indices:
        raise NotImplementedError('distance_transform_edt does not return indices')
    if not return_distances:
        raise ValueError('return_distances=False leaves nothing to return')
    a = _step1.bool_as_uint8(np.asarray(input))
    if a.dtype.kind not in 'uif':
        raise TypeError('distance_transform_edt takes bool, integer and float volumes, not %s' % a.dtype)
    if a.ndim != 3:
        raise ValueError('distance_transform_edt takes a 3-D volume, not %d-D' % a.ndim)
    if max(a.shape) > MAX_DIM:
        raise ValueError('every axis must have at most 16384 elements, not %s' % (a.shape,))
    if a.dtype != np.uint8:
        a = (a != 0).view(np.uint8)
    a = np.ascontiguousarray(a)
    if a.size and not (a.any() if invert else not a.all()):
        raise ValueError('the volume has no background voxel: there is no distance to take')
    out = np.empty(a.shape, np.int32 if squared else np.float64)
    ms = C.c_float()
    _step1.call('bfd_distance_transform_edt3d', _device, _engine._ptr(a), 1 if invert else 0, _engine._ptr(out) if squared else None,
                None if squared else _engine._ptr(out), a.shape[0], a.shape[1], a.shape[2], C.byref(ms))
    last_kernel_ms = ms.value
    return out
