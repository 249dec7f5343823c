"""What the resampling tests share: the volumes, the transforms, the float64 scipy reference, the voxels a comparison may leave out and the
comparison itself. The reference of every value is scipy.ndimage on the input as float64 with output=float64; a device result is compared
with that reference converted ONCE to the result's dtype (integers: scipy's rule, half away from zero, saturating)."""
import functools

import numpy as np

DTYPES = {'float32': np.float32, 'float64': np.float64, 'int16': np.int16, 'uint8': np.uint8}
MAX_EXCLUDED = 8


@functools.lru_cache(maxsize=None)
def volume(shape, dtype_name, seed=0):
    """Normal-distributed, amplitude about 600 (4 sigma of 150); uint8: the same field squeezed into 0..255. Read-only."""
    v = np.random.default_rng(seed).standard_normal(shape) * 150.0
    dt = DTYPES[dtype_name]
    a = np.clip(v / 5.0 + 128.0, 0, 255).astype(dt) if dt == np.uint8 else v.astype(dt)
    a.setflags(write=False)
    return a


def generic_matrix():
    """Rotation by 0.3 rad about axis 2, a shear that couples every axis, scales 0.8 / 1.1 / 0.93 -> (3, 4) with offset (3.2, -4.1, 1.7)."""
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    S = np.array([[1.0, 0.1, 0.013], [0.0, 1.0, 0.05], [0.0213, 0.0371, 1.0]])
    return np.hstack([R @ S @ np.diag([0.8, 1.1, 0.93]), np.array([[3.2], [-4.1], [1.7]])])


def scale_matrix(s, ishape, oshape):
    """Scale s per axis about the centres of the two grids, moved by a fraction of a sample so that no coordinate is a half-integer."""
    m = np.zeros((3, 4))
    m[:, :3] = np.eye(3) * s
    m[:, 3] = [(ishape[a] - 1) / 2.0 - s * (oshape[a] - 1) / 2.0 + 0.0137 * (a + 1) for a in range(3)]
    return m


def reference(a, m34, oshape, order, mode, cval, prefilter=True):
    import scipy.ndimage as ndi
    return ndi.affine_transform(np.asarray(a, np.float64), m34[:, :3], m34[:, 3], oshape, output=np.float64, order=order, mode=mode, cval=cval,
                                prefilter=prefilter)


def convert(ref, dtype):
    """The one conversion of float64 values to dtype, as scipy does it."""
    dtype = np.dtype(dtype)
    if dtype.kind == 'f':
        return ref.astype(dtype)
    info = np.iinfo(dtype)
    if dtype.kind == 'u':
        t = np.where(ref > 0, np.trunc(ref + 0.5), 0.0)
    else:
        t = np.where(ref > 0, np.trunc(ref + 0.5), np.trunc(ref - 0.5))
    return np.clip(t, info.min, info.max).astype(dtype)


def coordinates(m34, oshape):
    I, J, K = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in oshape], indexing='ij')
    return [m34[a, 3] + m34[a, 0] * I + m34[a, 1] * J + m34[a, 2] * K for a in range(3)]


def excluded(m34, ishape, oshape, order, mode, ref, dtype):
    """The voxels a comparison may leave out, from float64 coordinates computed here: a coordinate within 1e-9 dim of 0 or dim - 1 (the cval
    decision, mode constant); for order 0 a coordinate within 1e-9 of a half-integer; for integer outputs a reference within 1e-6 of a
    half-integer."""
    ex = np.zeros(oshape, bool)
    for a, c in enumerate(coordinates(m34, oshape)):
        if mode == 'constant':
            tol = 1e-9 * ishape[a]
            ex |= (np.abs(c) <= tol) | (np.abs(c - (ishape[a] - 1)) <= tol)
        if order == 0:
            ex |= np.abs(c - np.floor(c) - 0.5) <= 1e-9
    if np.dtype(dtype).kind in 'iu':
        ex |= np.abs(ref - np.floor(ref) - 0.5) <= 1e-6
    return ex


def violations(dev, ref, amplitude, exact=False, skip=None):
    """Number of voxels at which dev (the device's array, of its dtype) misses the float64 reference.
    float32: |dev - ref| <= 2^-24 |ref| + 2^-32 A; float64: <= 2^-32 A; integer dtypes and exact=True (order 0): dev == convert(ref)."""
    dev = np.asarray(dev)
    assert dev.shape == ref.shape, (dev.shape, ref.shape)
    keep = np.ones(ref.shape, bool) if skip is None else ~skip
    if exact or dev.dtype.kind in 'iu':
        bad = dev != convert(ref, dev.dtype)
    else:
        bound = 2.0 ** -32 * amplitude + (2.0 ** -24 * np.abs(ref) if dev.dtype == np.float32 else 0.0)
        bad = ~(np.abs(dev.astype(np.float64) - ref) <= bound)
    return int(np.count_nonzero(bad & keep))


def margin(dev, ref, amplitude):
    """max |dev - ref| / A of a float64 result (what DESIGN.md records)."""
    return float(np.abs(np.asarray(dev, np.float64) - ref).max() / amplitude) if ref.size else 0.0


def check(dev, a, m34, oshape, order, mode, cval, max_excluded=MAX_EXCLUDED, prefilter=True, ref=None):
    """Asserts one case; returns (excluded, max |dev - ref| / A). max_excluded=None: no voxel may be left out, whatever its coordinates."""
    if ref is None:
        ref = reference(a, m34, oshape, order, mode, cval, prefilter)
    amplitude = float(np.abs(np.asarray(a, np.float64)).max()) if a.size else 0.0
    assert dev.dtype == a.dtype and dev.shape == tuple(oshape) and dev.flags.c_contiguous
    ex = excluded(m34, a.shape, oshape, order, mode, ref, dev.dtype) if max_excluded is not None else np.zeros(oshape, bool)
    nex = int(np.count_nonzero(ex))
    assert nex <= (max_excluded or 0), '%d voxels excluded, the cap is %d' % (nex, max_excluded or 0)
    nbad = violations(dev, ref, amplitude, exact=(order == 0), skip=ex)
    mg = margin(dev, ref, amplitude) if dev.dtype.kind == 'f' and amplitude else 0.0
    print('order %d %s %s: excluded %d, violations %d, max|dev-ref|/A %.3e' % (order, mode, dev.dtype, nex, nbad, mg))
    assert nbad == 0, '%d voxels miss the bound (max |dev - ref| / A = %.3e)' % (nbad, mg)
    return nex, mg
