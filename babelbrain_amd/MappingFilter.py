"""Drop-in for the reference's `GPUFunctions.GPUMapping.MappingFilter` (BabelBrain/CalculateMaskProcess.py imports it, calls InitMapFilter and hands
MapFilter to BabelDatasetPreps.InitMappingGPUCallback):

    InitMapFilter(DeviceName, GPUBackend)
    MapFilter(HUMap, SelBone, UniqueHU, GPUBackend=...)         BabelDatasetPreps.py:1039: the row of every bone voxel's quantised CT value in the
                                                                table of unique values (host fallback :1034-1037: one full-volume pass per value)

    out[v] = m with UniqueHU[m] == HUMap[v] where SelBone[v] != 0 and such a row exists, 0 everywhere else (uint32, HUMap's shape)

One pass on the MI355X through the C ABI (bfd_map_values3d, csrc/bfd_voxelize.hip), bisection in the table; there is no CPU fallback. UniqueHU must
be strictly increasing, which np.unique output is. Argument errors are raised before the library is loaded."""
import ctypes as C

import numpy as np

from . import _engine, _step1

_device = 0
last_kernel_ms = None
MAX_ROWS = 65536


def InitMapFilter(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as InitLabel does. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


def _checked(HUMap, SelBone, UniqueHU):
    """The reference's asserts as TypeError / ValueError, and the ordering of the table."""
    for name, a in (('HUMap', HUMap), ('SelBone', SelBone), ('UniqueHU', UniqueHU)):
        if not isinstance(a, np.ndarray):
            raise TypeError('%s must be a numpy array' % name)
    if HUMap.dtype != np.float32:
        raise TypeError('HUMap must be float32, not %s' % HUMap.dtype)
    if UniqueHU.dtype != np.float32:
        raise TypeError('UniqueHU must be float32, not %s' % UniqueHU.dtype)
    if SelBone.dtype != np.uint8:
        raise TypeError('SelBone must be uint8, not %s' % SelBone.dtype)
    if HUMap.shape != SelBone.shape:
        raise ValueError('HUMap %r and SelBone %r differ in shape' % (HUMap.shape, SelBone.shape))
    if HUMap.ndim >= 2 and np.isfortran(HUMap):
        raise ValueError('HUMap must not be in Fortran order')
    if UniqueHU.ndim != 1 or not 1 <= UniqueHU.size <= MAX_ROWS:
        raise ValueError('UniqueHU must be one-dimensional with 1 .. %d rows' % MAX_ROWS)
    if np.any(np.isnan(UniqueHU)) or not np.all(UniqueHU[1:] > UniqueHU[:-1]):
        raise ValueError('UniqueHU must be strictly increasing (np.unique output is)')
    return np.ascontiguousarray(HUMap), np.ascontiguousarray(SelBone), np.ascontiguousarray(UniqueHU)


def MapFilter(HUMap, SelBone, UniqueHU, GPUBackend=None):
    """uint32 array of HUMap's shape: the row of HUMap's value in UniqueHU where SelBone is not 0 and the value is in the table, else 0. The ==
    is float32's: -0.0 matches +0.0, NaN matches nothing. TypeError for a wrong dtype, ValueError for a wrong shape, order or table. GPUBackend is
    ignored."""
    global last_kernel_ms
    hu, sel, uni = _checked(HUMap, SelBone, UniqueHU)
    out = np.empty(hu.shape, np.uint32)
    ms = C.c_float()
    _step1.call('bfd_map_values3d', _device, _engine._ptr(hu), _engine._ptr(sel), _engine._ptr(uni), uni.size, _engine._ptr(out), hu.size, C.byref(ms))
    last_kernel_ms = ms.value
    return out
