"""What the eleven Step-1 drop-ins (MedianFilter, BinaryClosing, LabelImage, Resample, Voxelize, MappingFilter, DistanceTransform, GaussianFilter, ConformalMask,
TissueMask, PseudoCT), Domain, the domain setup of Step 2, and ThermalAnalysis, the exposure analysis of Step 3, share on the way to the C ABI: the
device pick of their Init* functions, the bool -> uint8 normalisation and the call itself. Each module keeps its own `_device` and `last_kernel_ms`."""
import numpy as np

from . import _engine


def pick_device(DeviceName, current):
    """(the visible devices as list_devices gives them, the ordinal of the first whose name contains DeviceName). `current` where DeviceName is
    empty or matches none; EngineError where no device is visible."""
    devs = _engine.list_devices()
    if not devs:
        raise _engine.EngineError('no HIP device visible')
    if DeviceName:
        for d, name in devs:
            if DeviceName.lower() in name.lower():
                return devs, d
    return devs, current


def bool_as_uint8(a):
    """A bool array as uint8 (a view where it is C-contiguous, else a copy); any other array as it is."""
    if a.dtype == np.bool_:
        return a.view(np.uint8) if a.flags.c_contiguous else a.astype(np.uint8)
    return a


def call(entry, *args):
    """lib.<entry>(*args). The library is loaded here, after every check of the caller's; a non-zero rc raises EngineError with the library's message."""
    lib = _engine.load_library()
    rc = getattr(lib, entry)(*args)
    if rc != 0:
        raise _engine.EngineError('%s failed (rc=%d): %s' % (entry, rc, lib.bfd_last_error().decode()))
