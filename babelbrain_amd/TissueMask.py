"""The whole-volume stages that assemble FinalMask and the CT index map in the reference's BabelBrain/BabelDatasetPreps.py, on the device:

    InitTissueMask(DeviceName, GPUBackend)
    paint_components(volume, value, fill, select)         label, regionprops, sort by area, np.isin, masked store in one call; the labels stay on the device
    merge_islands(FinalMask, box_fov)                     :909-929, :1077-1097: every skin island but the largest becomes 4 (box_fov: the small ones only)
    drop_largest(mask)                                    :1055-1061: the air around the head
    quantize_values(ndataCT, nfct, CT_quantification)     :1019-1027, :1039: min, max, quantisation, np.unique and MapFilter in one call
    prefocal_cleanup(FinalMask, kFocal)                   :1121-1133: the Python double loop
    finish_mask(FinalMask, LocFocalPoint, ...)            :1066-1133, the flow around these and MedianFilter / BinaryErode

The work runs on the MI355X through the C ABI (bfd_paint_components3d in csrc/bfd_morphology.hip, bfd_quantize_values3d and bfd_clear_beyond_bone3d
in csrc/bfd_tissue.hip; definitions in include/babelfdtd.h); there is no CPU fallback. Every result equals its numpy restatement
(tests/tissue_oracle.py) element for element. Argument errors are raised before the library is loaded."""
import contextlib
import ctypes as C
import operator

import numpy as np

from . import BinaryClosing, MedianFilter, _engine, _step1

_device = 0
last_kernel_ms = None
last_counts = None                 # prefocal_cleanup's [lines with bone beyond kFocal, voxels changed]
SELECT_ALL_BUT_LARGEST, SELECT_SMALL, SELECT_LARGEST = 0, 1, 2
MAX_BITS = 16
# every data refusal of bfd_quantize_values3d (rc -1 after the device pick) carries these words after the entry's name (csrc/bfd_tissue.hip,
# DATA_REFUSED; include/babelfdtd.h): they become ValueError with the library's text
DATA_REFUSED = 'refused data'


def InitTissueMask(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as InitMedianFilter does. finish_mask runs its MedianFilter and BinaryErode calls on this device
    too, without changing what InitMedianFilter and InitBinaryClosing selected for those modules' other callers. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


@contextlib.contextmanager
def _on_my_device(module):
    """A call of another drop-in on this module's device: its own selection is put back afterwards"""
    theirs = module._device
    module._device = _device
    try:
        yield
    finally:
        module._device = theirs


def _volume(a, name):
    """uint8 (or bool), 3-D, fewer than 2^31 voxels, C-contiguous"""
    a = _step1.bool_as_uint8(np.asarray(a))
    if a.dtype != np.uint8:
        raise TypeError('%s must be uint8 or bool, not %s' % (name, a.dtype))
    if a.ndim != 3:
        raise ValueError('%s must be a 3-D volume, not %d-D' % (name, a.ndim))
    if a.size >= 2 ** 31:
        raise ValueError('the volume has 2^31 voxels or more')
    return np.ascontiguousarray(a)


def _byte(v, name):
    try:
        b = operator.index(v)
    except TypeError:
        raise ValueError('%s must be an int in 0 .. 255, not %r' % (name, v))
    if not 0 <= b <= 255:
        raise ValueError('%s must be an int in 0 .. 255, not %r' % (name, v))
    return b


def paint_components(volume, value, fill, select, connectivity=3):
    """(out, counts): `volume` (uint8 or bool, left as it was) with the components of volume == value that `select` chooses set to `fill`.
    select 0: every component but the largest; 1: those of them whose size a has a < 0.1 * the size of the largest; 2: the largest alone. The
    largest is the one with the most voxels, among equals the highest label (sorted(regionprops, key=area)[-1]). counts: int64
    [components, size of the largest, components painted, voxels painted]. Without foreground out equals volume and the counts are 0."""
    global last_kernel_ms
    a = _volume(volume, 'volume')
    value, fill = _byte(value, 'value'), _byte(fill, 'fill')
    if select not in (0, 1, 2):
        raise ValueError('select must be 0, 1 or 2, not %r' % (select,))
    if connectivity not in (1, 2, 3):
        raise ValueError('connectivity must be 1, 2 or 3, not %r' % (connectivity,))
    out = np.empty_like(a)
    counts = np.zeros(4, np.int64)
    ms = C.c_float()
    _step1.call('bfd_paint_components3d', _device, _engine._ptr(a), _engine._ptr(out), a.shape[0], a.shape[1], a.shape[2], value, int(connectivity),
                int(select), fill, _engine._ptr(counts), C.byref(ms))
    last_kernel_ms = ms.value
    return out, counts


def merge_islands(FinalMask, box_fov=False):
    """FinalMask with every island of skin (1) but the largest turned into brain (4); with box_fov only the islands below a tenth of the largest
    (BabelDatasetPreps.py:909-929, :1077-1097)."""
    return paint_components(FinalMask, 1, 4, SELECT_SMALL if box_fov else SELECT_ALL_BUT_LARGEST)[0]


def drop_largest(mask):
    """mask (0 / 1) without its largest component: the air regions without the air around the head (:1055-1061)."""
    return paint_components(mask, 1, 0, SELECT_LARGEST)[0]


def quantize_values(ndataCT, nfct, CT_quantification=10, return_quantized=False):
    """(UniqueHU, ndataCTMap, (mn, mx)), with return_quantized also the quantised volume: BabelDatasetPreps.py:1019-1027 and :1039.
    ndataCT: float32 volume (left as it was); nfct: bool or uint8 of its shape, the bone. UniqueHU: float32, the distinct quantised values under
    the mask, ascending; ndataCTMap: uint32, the row of each bone voxel's quantised value, 0 elsewhere; mn, mx: the range under the mask.
    TypeError for anything but float32 values; ValueError for a bad shape or CT_quantification, and, with the library's text, for an empty mask,
    a value under the mask that is not finite, a range of zero and a step below 2^-126."""
    global last_kernel_ms
    v = np.asarray(ndataCT)
    if v.dtype != np.float32:
        raise TypeError('ndataCT must be float32, not %s' % v.dtype)
    m = _step1.bool_as_uint8(np.asarray(nfct))
    if m.dtype != np.uint8:
        raise TypeError('nfct must be bool or uint8, not %s' % m.dtype)
    if v.ndim != 3 or v.shape != m.shape:
        raise ValueError('ndataCT %r and nfct %r must be 3-D volumes of one shape' % (v.shape, m.shape))
    if v.size >= 2 ** 31:
        raise ValueError('the volume has 2^31 voxels or more')
    try:
        bits = operator.index(CT_quantification)
    except TypeError:
        raise ValueError('CT_quantification must be an int in 1 .. %d, not %r' % (MAX_BITS, CT_quantification))
    if not 1 <= bits <= MAX_BITS:
        raise ValueError('CT_quantification must be an int in 1 .. %d, not %r' % (MAX_BITS, CT_quantification))
    v, m = np.ascontiguousarray(v), np.ascontiguousarray(m)
    quantized = np.empty_like(v) if return_quantized else None
    cmap = np.empty(v.shape, np.uint32)
    table = np.empty(1 << bits, np.float32)
    n = C.c_int64()
    rng = np.zeros(2, np.float32)
    ms = C.c_float()
    try:
        _step1.call('bfd_quantize_values3d', _device, _engine._ptr(v), _engine._ptr(m), v.shape[0], v.shape[1], v.shape[2], bits, _engine._ptr(quantized),
                    _engine._ptr(cmap), _engine._ptr(table), C.byref(n), _engine._ptr(rng), C.byref(ms))
    except _engine.EngineError as e:
        if '(rc=-1)' in str(e) and DATA_REFUSED in str(e):
            raise ValueError(str(e)) from None
        raise
    last_kernel_ms = ms.value
    res = (table[:n.value].copy(), cmap, (rng[0], rng[1]))
    return res + (quantized,) if return_quantized else res


def prefocal_cleanup(FinalMask, kFocal, bone=(2, 3), from_value=4, to_value=1):
    """FinalMask with, on every line (i, j) that has bone beyond kFocal, the voxels equal to from_value beyond the last such bone set to to_value
    (BabelDatasetPreps.py:1121-1133). bone: the two bone values."""
    global last_kernel_ms, last_counts
    a = _volume(FinalMask, 'FinalMask')
    try:
        kf = operator.index(kFocal)
    except TypeError:
        raise ValueError('kFocal must be an index of the last axis, not %r' % (kFocal,))
    if not 0 <= kf < a.shape[2]:
        raise ValueError('kFocal must be an index of the last axis (0 .. %d), not %r' % (a.shape[2] - 1, kFocal))
    if len(bone) != 2:
        raise ValueError('bone must be two values, not %r' % (bone,))
    bA, bB, fv, tv = _byte(bone[0], 'bone'), _byte(bone[1], 'bone'), _byte(from_value, 'from_value'), _byte(to_value, 'to_value')
    out = np.empty_like(a)
    counts = np.zeros(2, np.int64)
    ms = C.c_float()
    _step1.call('bfd_clear_beyond_bone3d', _device, _engine._ptr(a), _engine._ptr(out), a.shape[0], a.shape[1], a.shape[2], kf, bA, bB, fv, tv,
                _engine._ptr(counts), C.byref(ms))
    last_kernel_ms = ms.value
    last_counts = counts
    return out


def finish_mask(FinalMask, LocFocalPoint, TrabecularProportion=0.8, nfct=None, box_fov=False):
    """BabelDatasetPreps.py:1066-1133: the final median filter, the second labelling, the trabecular erosion, the focal voxel and the pre-focal
    cleanup. FinalMask: uint8 volume (left as it was); LocFocalPoint: three indices; nfct: the bone mask of the CT branch (bool), or None for the
    branch without CT. Returns the new uint8 FinalMask. The device calls are MedianFilter, merge_islands, BinaryErode and prefocal_cleanup; the glue
    between them is masked numpy stores on the host."""
    m = _volume(FinalMask, 'FinalMask').copy()
    loc = tuple(operator.index(x) for x in LocFocalPoint)
    if len(loc) != 3 or any(not 0 <= x < s for x, s in zip(loc, m.shape)):
        raise ValueError('LocFocalPoint %r is not a voxel of a volume of shape %r' % (LocFocalPoint, m.shape))
    if nfct is not None:
        nfct = np.asarray(nfct)
        if nfct.shape != m.shape:
            raise ValueError('nfct has shape %r, FinalMask %r' % (nfct.shape, m.shape))
        nfct = nfct != 0
        m[m == 2] = 1
    with _on_my_device(MedianFilter):
        m = MedianFilter.MedianFilter(m, 7)
    if nfct is not None:
        m[nfct] = 2
        m = merge_islands(m, box_fov)
    bone = m == 2
    degree = int(np.round(bone[loc[0], loc[1], loc[2]:].sum() * (1 - TrabecularProportion)))
    if degree != 0:
        with _on_my_device(BinaryClosing):
            m[BinaryClosing.BinaryErode(bone, iterations=degree)] = 3
    else:
        m[bone] = 3                                  # the whole bone counts as trabecular
    m[loc] = 5
    if nfct is not None:
        m = prefocal_cleanup(m, loc[2])
    return m
