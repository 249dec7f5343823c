"""Drop-in for the reference's `GPUFunctions.GPULabel.LabelImage` (BabelBrain/CalculateMaskProcess.py:41, :49 import it, :79-80 call InitLabel and
hand LabelImage to BabelDatasetPreps.InitLabelImageGPUCallback):

    InitLabel(DeviceName, GPUBackend)                                 CalculateMaskProcess.py:79
    LabelImage(nfct, GPUBackend=...)                                  BabelDatasetPreps.py:891, :913, :1058, :1081 (skimage.measure.label of a bool volume)
    largest_component(nfct)                                           :888-894 in one call: label, regionprops, sort by area, == the last label
    largest_component(arr, ties='first')                              CTZTEProcessing.py:599-606: sorted(..., reverse=True)[0] (bfd_select_component3d)
    component_sizes(mask)                                             the areas regionprops would report, labels 1..n

The labelling runs on the MI355X through the C ABI (bfd_label3d, csrc/bfd_morphology.hip); there is no CPU fallback. Labels equal
scipy.ndimage.label(image, generate_binary_structure(3, connectivity))[0] element for element (and skimage.measure.label): background 0,
components numbered in the order of their first voxel in C-order raster scan. Argument errors are raised before the library is loaded."""
import ctypes as C
import operator

import numpy as np

from . import _engine, _step1

_device = 0
last_kernel_ms = None
last_component = None              # largest_component(ties='first'): (components, voxels of the chosen one)


def InitLabel(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as InitMedianFilter does. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


def _checked(image, background, connectivity):
    """Everything that can be refused without the library: returns (contiguous uint8 view of the foreground, connectivity)."""
    a = np.asarray(image)
    if a.dtype != np.bool_:
        raise RuntimeError('Image datatype must be boolean. For other datatypes, use Skimage.measure.label function')
    if a.ndim != 3:
        raise ValueError('LabelImage takes a 3-D volume, not %d-D' % a.ndim)
    if a.size >= 2 ** 31:
        raise ValueError('the volume has 2^31 voxels or more')
    if connectivity is None:
        connectivity = 3
    try:
        c = operator.index(connectivity)
    except TypeError:
        raise ValueError('Connectivity for 3D image should be in [1, ..., 3]. Got %r.' % (connectivity,))
    if not 1 <= c <= 3:
        raise ValueError('Connectivity for 3D image should be in [1, ..., 3]. Got %r.' % (connectivity,))
    if background == 1:
        a = ~a                                      # a fresh array: the caller's stays as it was
    return np.ascontiguousarray(a).view(np.uint8), c


def _run(a, c, want_labels=False, want_sizes=False, want_largest=False):
    """(labels or None, n, sizes or None, largest or None)"""
    global last_kernel_ms
    labels = np.empty(a.shape, np.int32) if want_labels else None
    largest = np.empty(a.shape, np.uint8) if want_largest else None
    # a component has at least one voxel: the foreground count bounds n, so one call suffices
    sizes = np.zeros(int(np.count_nonzero(a)), np.int64) if want_sizes else None
    n = C.c_int64()
    ms = C.c_float()
    _step1.call('bfd_label3d', _device, _engine._ptr(a), _engine._ptr(labels), a.shape[0], a.shape[1], a.shape[2], c, C.byref(n),
                _engine._ptr(sizes), 0 if sizes is None else sizes.size, _engine._ptr(largest), C.byref(ms))
    last_kernel_ms = ms.value
    return (labels, int(n.value), None if sizes is None else sizes[:n.value].copy(), None if largest is None else largest.view(np.bool_))


def LabelImage(image, background=None, return_num=False, connectivity=None, GPUBackend=None):
    """Connected components of a bool volume: int32 labels of image's shape (0 = background), or (labels, n) with return_num. background == 1
    labels the false voxels instead. connectivity 1, 2, 3 (None: 3) = 6, 18, 26 neighbours. RuntimeError for an image that is not bool (the
    reference's), ValueError for a connectivity outside 1..3 or a volume that is not 3-D. The image is left as it was. GPUBackend is ignored."""
    labels, n, _, _ = _run(*_checked(image, background, connectivity), want_labels=True)
    return (labels, n) if return_num else labels


def component_sizes(image, connectivity=None):
    """int64 [n]: the voxel counts of labels 1..n of LabelImage(image, connectivity=connectivity), without bringing the labels to the host."""
    return _run(*_checked(image, None, connectivity), want_sizes=True)[2]


def largest_component(image, connectivity=None, ties='last'):
    """bool mask of the component with the most voxels; among equals the one with the highest label, which is what
        label_img = label(image); regions = sorted(regionprops(label_img), key=lambda d: d.area); mask = label_img == regions[-1].label
    selects (BabelDatasetPreps.py:888-894). All false for an image without foreground. The int32 labels never leave the device.
    ties='first' keeps the lowest label among equals instead (bfd_select_component3d): what
        props = sorted(regionprops(label_img, ...), key=itemgetter('pixelcount'), reverse=True); mask = label_img == props[0].label
    selects (CTZTEProcessing.py:599-606), Python's sort being stable under reverse too."""
    global last_kernel_ms, last_component
    if ties not in ('last', 'first'):
        raise ValueError("ties must be 'last' or 'first', not %r" % (ties,))
    if ties == 'last':
        return _run(*_checked(image, None, connectivity), want_largest=True)[3]
    a, c = _checked(image, None, connectivity)
    out = np.empty(a.shape, np.uint8)
    info = np.zeros(2, np.int64)
    ms = C.c_float()
    _step1.call('bfd_select_component3d', _device, _engine._ptr(a), _engine._ptr(out), a.shape[0], a.shape[1], a.shape[2], c, 1, _engine._ptr(info),
                C.byref(ms))
    last_kernel_ms = ms.value
    last_component = (int(info[0]), int(info[1]))
    return out.view(np.bool_)
