"""The bone-rim partial-volume correction of the CT (BabelBrain/BabelDatasetPreps.py:935-1017, bMaximizeBoneRim) as one device call:

    InitBoneRim(DeviceName)
    odd_box(RatioCTVoxels)                                        :942-946: every size odd and at least 3
    maximize_bone_rim(ndataCT, nfct, RatioCTVoxels, ...)          :948-1010 (and, with floor, the clamp of :931-933)

The CT and the bone mask go up once, the erosion, the distance transform, the two Gaussian filters and the blend run on the MI355X without the host
in between (bfd_bone_rim_correct3d, csrc/bfd_bonerim.hip; definition in include/babelfdtd.h) and the corrected CT comes down once; there is no CPU
fallback. With global_mean = numpy's own `ndataCT[ndataCT >= 800].mean()` the result equals the reference's flow (tests/bonerim_oracle.py) wherever
the float32 filters equal scipy's; without it the mean is the exact one, formed on the device, which may differ from numpy's pairwise float32 sum by
an ulp or so and reaches only the edge voxels that `last_stats['global_mean_voxels']` counts. Argument errors are raised before the library is
loaded."""
import ctypes as C
import math
import operator

import numpy as np

from . import _engine, _step1

_device = 0
last_kernel_ms = None
last_stats = None                  # dict of STAT_NAMES after a call
last_global_mean = None            # the float32 mean the call used
STAT_NAMES = ('bone', 'interior', 'dense', 'edge', 'global_mean_voxels', 'clipped', 'changed', 'max_d2')
MIN_THRESHOLD = 512.0              # every float32 from here up is a multiple of 2^-14: the exact sum of the dense values rests on it
MAX_BOX = 31
MAX_DIM = 16384
DATA_REFUSED = 'refused data'      # what every data refusal of the entry carries after its name: they become ValueError
SWEEP_VOXELS = 2048 * 4 * 64       # voxels one sweep of the new kernels covers before their grid-stride loops turn (RIM_BLOCKS x waves x 64)


def InitBoneRim(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as InitMedianFilter does. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


def odd_box(RatioCTVoxels):
    """:942-946 on a copy: even sizes go up by one, then 1 becomes 3. Three ints."""
    box = [operator.index(r) for r in RatioCTVoxels]
    if len(box) != 3:
        raise ValueError('RatioCTVoxels must have three values, not %r' % (RatioCTVoxels,))
    for a in range(3):
        if box[a] % 2 == 0:
            box[a] += 1
        if box[a] == 1:
            box[a] = 3
    return box


def maximize_bone_rim(ndataCT, nfct, RatioCTVoxels, interior_high_th=800.0, max_boost=1000.0, floor=None, global_mean=None, inplace=False,
                      return_fields=False):
    """The corrected CT of :948-1010. ndataCT: float32 3-D volume; nfct: the bone mask of its shape, any dtype, read as != 0; RatioCTVoxels: three
    ints, made odd here (odd_box; the caller's list is left as it was). floor: TypeThresold of :931-933, applied to the bone voxels first (None:
    the caller has done it). global_mean: the float32 mean to use where the blurred mask is at most 1e-6, or None for the exact mean of the dense
    voxels formed on the device. inplace: the result is written into ndataCT (which must then be a writable C-contiguous float32 array) and returned.
    return_fields: also a dict of interior (bool), d2 (int32), bi, bm (float32) and global_mean.
    TypeError for a CT that is not float32; ValueError for shapes, a box size outside 3 .. 31, a threshold below 512, values that are not finite,
    and for the data the entry refuses (a CT value that is not finite, a dense value at or above 2^17, no dense voxel, no interior voxel)."""
    global last_kernel_ms, last_stats, last_global_mean
    ct = ndataCT if inplace else np.asarray(ndataCT)
    if not isinstance(ct, np.ndarray) or ct.dtype != np.float32:
        raise TypeError('ndataCT must be a float32 array, not %s' % (getattr(ct, 'dtype', type(ct)),))
    if ct.ndim != 3:
        raise ValueError('ndataCT must be a 3-D volume, not %d-D' % ct.ndim)
    if max(ct.shape) > MAX_DIM or ct.size >= 2 ** 31:
        raise ValueError('every axis must have at most 16384 elements and the volume fewer than 2^31, not %s' % (ct.shape,))
    if inplace and not (ct.flags.c_contiguous and ct.flags.writeable):
        raise ValueError('inplace needs a writable C-contiguous ndataCT')
    mask = np.asarray(nfct)
    if mask.shape != ct.shape:
        raise ValueError('nfct has shape %r, ndataCT %r' % (mask.shape, ct.shape))
    box = odd_box(RatioCTVoxels)
    if min(box) < 3 or max(box) > MAX_BOX:
        raise ValueError('every box size must be 3 .. %d after the adjustment, not %r' % (MAX_BOX, box))
    th = np.float32(interior_high_th)
    if not (np.isfinite(th) and th >= MIN_THRESHOLD):
        raise ValueError('interior_high_th must be finite and at least %g, not %r' % (MIN_THRESHOLD, interior_high_th))
    max_boost = float(max_boost)
    if math.isnan(max_boost):
        raise ValueError('max_boost is not a number')
    if floor is not None and not np.isfinite(np.float32(floor)):
        raise ValueError('floor must be finite, not %r' % (floor,))
    if global_mean is not None and not np.isfinite(np.float32(global_mean)):
        raise ValueError('global_mean must be finite, not %r' % (global_mean,))
    ct = np.ascontiguousarray(ct)
    mask = np.ascontiguousarray(_step1.bool_as_uint8(mask) if mask.dtype in (np.bool_, np.uint8) else (mask != 0).view(np.uint8))
    out = ct if inplace else np.empty_like(ct)
    cbox = np.array(box, np.int32)
    cfloor = None if floor is None else np.array([floor], np.float32)
    gmean = np.array([0.0 if global_mean is None else global_mean], np.float32)
    stats = np.zeros(8, np.int64)
    fields = {}
    if return_fields:
        fields = dict(interior=np.empty(ct.shape, np.uint8), d2=np.empty(ct.shape, np.int32), bi=np.empty_like(ct), bm=np.empty_like(ct))
    ms = C.c_float()
    try:
        _step1.call('bfd_bone_rim_correct3d', _device, _engine._ptr(ct), _engine._ptr(mask), _engine._ptr(out), ct.shape[0], ct.shape[1], ct.shape[2],
                    _engine._ptr(cbox), float(th), max_boost, float(box[0]) / 2.0, float(box[0]), _engine._ptr(cfloor), _engine._ptr(gmean),
                    0 if global_mean is None else 1, _engine._ptr(stats), _engine._ptr(fields.get('interior')), _engine._ptr(fields.get('d2')),
                    _engine._ptr(fields.get('bi')), _engine._ptr(fields.get('bm')), C.byref(ms))
    except _engine.EngineError as e:
        if '(rc=-1)' in str(e) and DATA_REFUSED in str(e):
            raise ValueError(str(e)) from None
        raise
    last_kernel_ms = ms.value
    last_stats = {name: int(v) for name, v in zip(STAT_NAMES, stats)}
    last_global_mean = np.float32(gmean[0])
    if return_fields:
        fields['interior'] = fields['interior'].view(np.bool_)
        fields['global_mean'] = last_global_mean
        return out, fields
    return out
