"""Drop-in for the reference's `GPUFunctions.GPUBinaryClosing.BinaryClosing` (BabelBrain/CalculateMaskProcess.py:40, :48 import it, :68 calls
InitBinaryClosing and :75 hands BinaryClose to BabelDatasetPreps.InitBinaryClosingGPUCallback), and for the scipy.ndimage morphology calls around it:

    InitBinaryClosing(DeviceName, GPUBackend)                         CalculateMaskProcess.py:68
    BinaryClose(fct, structure=np.ones(sf2, int), GPUBackend=...)     BabelDatasetPreps.py:881-883 (sf2 = round(5 mm / voxel size) per axis)
    BinaryDilate(mask, iterations=6)                                  :901   (scipy's default cross)
    BinaryErode(mask, iterations=n)                                   :953, :1106

The work runs on the MI355X through the C ABI (bfd_binary_morphology3d, csrc/bfd_morphology.hip); there is no CPU fallback. Results equal
scipy.ndimage.binary_closing / binary_dilation / binary_erosion / binary_opening voxel for voxel, scipy's window for even sizes included. An
all-ones structure of up to 31 per axis is applied as three 1-D passes over the bit-packed mask; any other structure may have up to 7 per axis.
Argument errors are raised before the library is loaded."""
import ctypes as C
import operator

import numpy as np

from . import _engine, _step1

_device = 0
last_kernel_ms = None
MAX_BOX = 31               # per axis, all-ones structures (three 1-D passes)
MAX_GENERAL = 7            # per axis, every other structure (tap list)
_OPS = {'erosion': 0, 'dilation': 1, 'closing': 2, 'opening': 3}


def InitBinaryClosing(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as InitMedianFilter does. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


def structure_path(structure):
    """'box' for an all-ones 3-D structure of 1..31 per axis, 'general' for any other of at most 7 per axis with a true element (None: the
    cross); ValueError for everything else. Returns (path, uint8 C-order structure or None)."""
    if structure is None:
        return 'general', None
    s = np.asarray(structure)
    if s.ndim != 3:
        raise ValueError('the structure must be 3-D, not %d-D' % s.ndim)
    if s.size == 0:
        raise ValueError('the structure must not be empty')
    s = np.ascontiguousarray(s != 0).view(np.uint8)
    if s.all():
        if max(s.shape) > MAX_BOX:
            raise ValueError('an all-ones structure may have at most %d elements per axis, not %s' % (MAX_BOX, s.shape))
        return 'box', s
    if max(s.shape) > MAX_GENERAL:
        raise ValueError('a structure that is not all ones may have at most %d elements per axis, not %s' % (MAX_GENERAL, s.shape))
    if not s.any():
        raise ValueError('the structure has no true element')
    return 'general', s


def _checked(op, input, structure, iterations, output, origin, mask, border_value):
    """Everything that can be refused without the library: returns (contiguous uint8 volume, structure or None, iterations, border value)."""
    if output is not None:
        raise NotImplementedError('an output array is not supported: the result is returned')
    if mask is not None:
        raise NotImplementedError('a mask is not supported')
    try:
        zero_origin = not np.any(np.asarray(origin) != 0)
    except Exception:
        zero_origin = False
    if not zero_origin:
        raise NotImplementedError('only origin 0 is supported, not %r' % (origin,))
    a = _step1.bool_as_uint8(np.asarray(input))
    if a.dtype != np.uint8:
        raise TypeError('binary morphology takes bool or uint8 masks, not %s' % a.dtype)
    if a.ndim != 3:
        raise ValueError('binary morphology takes a 3-D volume, not %d-D' % a.ndim)
    if a.size >= 2 ** 31:
        raise ValueError('the volume has 2^31 voxels or more')
    _, s = structure_path(structure)
    try:
        it = operator.index(iterations)
    except TypeError:
        raise ValueError('iterations must be an int, not %r' % (iterations,))
    if it < 1:
        raise ValueError('iterations must be at least 1 (repeating until nothing changes is not supported), not %d' % it)
    if border_value not in (0, 1):          # True and False included
        raise ValueError('border_value must be 0 or 1, not %r' % (border_value,))
    if op in ('closing', 'opening') and border_value != 0:
        raise ValueError('border_value is 0 for closing and opening, as in scipy')
    return np.ascontiguousarray(a), s, it, int(border_value)


def _run(op, a, s, it, border):
    global last_kernel_ms
    out = np.empty_like(a)
    ms = C.c_float()
    sh = s.shape if s is not None else (3, 3, 3)
    _step1.call('bfd_binary_morphology3d', _device, _OPS[op], _engine._ptr(a), _engine._ptr(out), a.shape[0], a.shape[1], a.shape[2],
                _engine._ptr(s), sh[0], sh[1], sh[2], it, border, C.byref(ms))
    last_kernel_ms = ms.value
    return out.view(np.bool_)


def BinaryClose(input, structure, iterations=1, output=None, origin=0, mask=None, border_value=0, brute_force=False, GPUBackend=None):
    """scipy.ndimage.binary_closing(input, structure, iterations) on the device: a fresh bool array; input (bool or uint8, any strides; non-zero
    is true) is left as it was. structure: 3-D, all ones with up to 31 per axis, or anything up to 7 per axis; None gives the cross.
    NotImplementedError for an output array, a mask or an origin other than 0; ValueError for a bad structure, iterations < 1, a border_value
    other than 0 or a volume that is not 3-D; TypeError for another dtype. brute_force and GPUBackend are ignored."""
    return _run('closing', *_checked('closing', input, structure, iterations, output, origin, mask, border_value))


def BinaryOpen(input, structure=None, iterations=1, output=None, origin=0, mask=None, border_value=0, brute_force=False, GPUBackend=None):
    """scipy.ndimage.binary_opening on the device; arguments as BinaryClose."""
    return _run('opening', *_checked('opening', input, structure, iterations, output, origin, mask, border_value))


def BinaryDilate(input, structure=None, iterations=1, output=None, origin=0, mask=None, border_value=0, brute_force=False, GPUBackend=None):
    """scipy.ndimage.binary_dilation on the device; arguments as BinaryClose, border_value 0 or 1."""
    return _run('dilation', *_checked('dilation', input, structure, iterations, output, origin, mask, border_value))


def BinaryErode(input, structure=None, iterations=1, output=None, origin=0, mask=None, border_value=0, brute_force=False, GPUBackend=None):
    """scipy.ndimage.binary_erosion on the device; arguments as BinaryClose, border_value 0 or 1."""
    return _run('erosion', *_checked('erosion', input, structure, iterations, output, origin, mask, border_value))
