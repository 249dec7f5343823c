"""The conformal masks of Step 1 on the device: drop-in for BabelDatasetPreps.py:696-759, where the reference takes the points `Voxelize` returned,
multiplies them by the rotated affine on the host (hstack, float32 np.dot, np.round, int64 cast, filter of the upper side, fancy-index store) once per
mesh. Here the points never exist on the host: a mesh is voxelised and scattered on the device in one call, and only the mask comes back.

    InitConformal(DeviceName, GPUBackend)
    rotated_bounds(source, matrix, ...)                         (lo, hi, count): the index bounds of the points under a float32 [3][4] matrix
    scatter_mask(source, matrix, shape, ...)                    uint8 [M1][M2][M3]; IndexError where a point lies below -M, as numpy raises it
    conformal_masks(skin, skull, csf, SpatialStep, RMat, Location, targetResolution=0.75 * SpatialStep)
                                                                (baseaffineRot, LocFocalPoint, skin int8, skull int8, csf uint8)

`source` is a mesh (anything with `.triangles` of shape (n, 3, 3), or such an array) with `targetResolution` (the reference's grid of the mesh's own
bounds, as Voxelize takes it) or with `bounds` and `grid`; or a packed table (uint32, one dimension, voxelize_table's) with `grid`, `origin`, `unit`.
The definition is in include/babelfdtd.h (bfd_voxel_scatter3d): float32, one operation per rounding, ((m0 x + m1 y) + m2 z) + m3, half to even;
tests/conformal_oracle.py restates it in numpy and the device equals it voxel for voxel. There is no CPU fallback. Argument errors are raised before
the library is loaded."""
import ctypes as C
import operator

import numpy as np

from . import Voxelize as VX, _engine, _step1

_device = 0
last_kernel_ms = None
last_counts = None         # int64 [4] of the last call: points, above, wrapped, below


def InitConformal(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as InitVoxelize does. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


def _matrix(matrix):
    """float32 C-contiguous [3][4]: the first three rows of a [3][4] or [4][4] matrix, refused when not finite as float32."""
    m = np.asarray(matrix)
    if m.dtype.kind not in 'fiu':
        raise TypeError('the matrix must hold numbers, not %s' % m.dtype)
    if m.shape not in ((3, 4), (4, 4)):
        raise ValueError('the matrix must have shape (3, 4) or (4, 4), not %r' % (m.shape,))
    with np.errstate(over='ignore'):
        m32 = np.ascontiguousarray(m[:3], np.float32)
    if not np.all(np.isfinite(m32)):
        raise ValueError('the matrix is not finite (as float32)')
    return m32


def _shape(shape):
    try:
        s = tuple(operator.index(x) for x in shape)
    except TypeError:
        raise ValueError('shape must be three integers, not %r' % (shape,))
    if len(s) != 3 or min(s) < 1:
        raise ValueError('shape must be three integers of at least 1, not %r' % (shape,))
    if s[0] * s[1] * s[2] >= 2 ** 31:
        raise ValueError('the mask %r has 2^31 voxels or more' % (s,))
    return s


def _source(source, targetResolution, bounds, grid, origin, unit):
    """('table', table, grid, origin, unit) or ('mesh', triangles, grid, min, max), every argument checked."""
    if isinstance(source, np.ndarray) and source.dtype == np.uint32 and source.ndim == 1:
        if grid is None or origin is None or unit is None:
            raise ValueError('a table comes with grid, origin and unit')
        g = VX._grid(grid)
        nt = (g[0] * g[1] * g[2] + 31) // 32
        if source.size != nt:
            raise ValueError('the table of a %r grid is uint32 [%d]' % (g, nt))
        o, u = np.ascontiguousarray(origin, np.float64), np.ascontiguousarray(unit, np.float64)
        if o.shape != (3,) or u.shape != (3,) or not (np.all(np.isfinite(o)) and np.all(np.isfinite(u))):
            raise ValueError('origin and unit are three finite numbers each')
        return 'table', np.ascontiguousarray(source), g, o, u
    if origin is not None or unit is not None:
        raise ValueError('origin and unit belong to a table; a mesh takes targetResolution, or bounds and grid')
    t = VX._triangles(source)
    if (bounds is None) != (grid is None):
        raise ValueError('bounds and grid come together')
    if bounds is not None:
        if targetResolution is not None:
            raise ValueError('either targetResolution or bounds and grid, not both')
        r, g = VX._bounds(bounds), VX._grid(grid)
    else:
        if targetResolution is None:
            raise ValueError('a mesh takes targetResolution, or bounds and grid')
        r = VX._bounds(VX.mesh_bounds(source))
        g, _ = VX.grid_rule(r, targetResolution)
    return 'mesh', t, g, np.ascontiguousarray(r[0]), np.ascontiguousarray(r[1])


def _run(src, m, shape, want_bounds):
    """(out or None, lo or None, hi or None, counts) of one call; lo and hi are None where there is no point."""
    global last_kernel_ms, last_counts
    kind, data, g, a, b = src
    out = np.empty(shape, np.uint8) if shape is not None else None
    lo, hi, counts = np.zeros(3, np.int64), np.zeros(3, np.int64), np.zeros(4, np.int64)
    ms = C.c_float()
    M = shape if shape is not None else (0, 0, 0)
    P = _engine._ptr
    tail = (P(m), M[0], M[1], M[2], P(out), P(lo) if want_bounds else None, P(hi) if want_bounds else None, P(counts), C.byref(ms))
    if kind == 'table':
        _step1.call('bfd_voxel_scatter3d', _device, P(data), g[0], g[1], g[2], P(a), P(b), *tail)
    else:
        _step1.call('bfd_voxelize_scatter3d', _device, P(data), data.shape[0], P(a), P(b), g[0], g[1], g[2], *tail)
    last_kernel_ms, last_counts = ms.value, counts
    if not want_bounds or counts[0] == 0:
        lo = hi = None
    return out, lo, hi, counts


def rotated_bounds(source, matrix, targetResolution=None, bounds=None, grid=None, origin=None, unit=None):
    """(lo, hi, count): int64 [3] minimum and maximum of the indices rint(matrix . point) over the points of the source, before anything is dropped
    (None, None, 0 where it has no point)."""
    src, m = _source(source, targetResolution, bounds, grid, origin, unit), _matrix(matrix)
    _, lo, hi, counts = _run(src, m, None, True)
    return lo, hi, int(counts[0])


def scatter_mask(source, matrix, shape, targetResolution=None, bounds=None, grid=None, origin=None, unit=None, with_bounds=False):
    """uint8 [M1][M2][M3]: 1 where a point of the source lands, numpy's index rules behind the reference's filter: points at or above M on an axis are
    dropped, indices in [-M, 0) wrap; IndexError where a point lies below -M, as the reference's fancy-index store raises it. last_counts holds
    (points, above, wrapped, below). with_bounds: (mask, lo, hi) of the same call."""
    src, m, s = _source(source, targetResolution, bounds, grid, origin, unit), _matrix(matrix), _shape(shape)
    out, lo, hi, counts = _run(src, m, s, with_bounds)
    if counts[3]:
        raise IndexError('%d of %d points have an index below -M on some axis of the %r mask' % (counts[3], counts[0], s))
    return (out, lo, hi) if with_bounds else out


def focal_index(matrix, Location):
    """int64 [3]: one point under the device's float32 rule, on the host: every product and sum rounded on its own, in the order of the definition."""
    m = _matrix(matrix)
    with np.errstate(over='ignore'):
        p = np.asarray(Location, np.float32)
    if p.shape != (3,) or not np.all(np.isfinite(p)):
        raise ValueError('Location is three finite numbers (as float32)')
    t = np.array([((m[a, 0] * p[0] + m[a, 1] * p[1]) + m[a, 2] * p[2]) + m[a, 3] for a in range(3)], np.float32)
    if not np.all(np.abs(t) < np.float32(2.0 ** 31)):
        raise ValueError('the focal point lies outside the int32 range of indices')
    return np.round(t).astype(np.int64)


def conformal_masks(skin, skull, csf, SpatialStep, RMat, Location, targetResolution=None):
    """BabelDatasetPreps.py:696-759 from the three meshes: (baseaffineRot float64 [4][4], LocFocalPoint int64 [3], BinMaskConformalSkinRot int8,
    BinMaskConformalSkullRot int8, BinMaskConformalCSFRot uint8). The skin's points are bounded under inv(RMat * SpatialStep) cast to float32, the
    minima give the new origin, the inverse of the moved affine, cast to float32, is the matrix of all three scatters, and the mask's shape comes
    from the maxima of the skin's indices with the focal point's among them. The reference stores the focal point into the skin mask with the points
    (it is the last column of XYZ at line 728); so does this. last_kernel_ms is the sum over the five device calls."""
    global last_kernel_ms
    step = float(SpatialStep)
    if not (np.isfinite(step) and step > 0):
        raise ValueError('SpatialStep must be a positive finite number')
    R = np.asarray(RMat, np.float64)
    if R.shape != (3, 3) or not np.all(np.isfinite(R)):
        raise ValueError('RMat must be a finite (3, 3) matrix')
    res = 0.75 * step if targetResolution is None else float(targetResolution)
    srcs = [_source(mesh, res, None, None, None, None) for mesh in (skin, skull, csf)]
    affine = np.eye(4)
    affine[:3, :3] = R * step
    m = _matrix(np.linalg.inv(affine))                       # LinAlgError where RMat is singular
    focal_index(m, Location)                                 # refuses a bad Location before the library is loaded
    total = 0.0
    _, lo, _, counts = _run(srcs[0], m, None, True)
    total += last_kernel_ms
    if counts[0] == 0:
        raise ValueError('the skin mesh encloses no voxel centre at this resolution')
    affine[:, 3] = affine @ np.array([lo[0], lo[1], lo[2], 1.0])
    m = _matrix(np.linalg.inv(affine))
    _, _, hi, _ = _run(srcs[0], m, None, True)
    total += last_kernel_ms
    focal = focal_index(m, Location)
    shape = _shape(tuple(int(v) for v in np.maximum(hi, focal) + 1))
    masks = []
    for src in srcs:
        out, _, _, counts = _run(src, m, shape, False)
        total += last_kernel_ms
        if counts[3]:
            raise IndexError('%d points have an index below -M on some axis of the %r mask' % (counts[3], shape))
        masks.append(out)
    masks[0][tuple(focal)] = 1
    last_kernel_ms = total
    return affine, focal, masks[0].view(np.int8), masks[1].view(np.int8), masks[2]
