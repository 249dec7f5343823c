"""Drop-in for the reference's `GPUFunctions.GPUVoxelize.Voxelize` (BabelBrain/CalculateMaskProcess.py imports it, calls InitVoxelize and hands
Voxelize to BabelDatasetPreps.InitVoxelizeGPUCallback):

    InitVoxelize(DeviceName, GPUBackend)
    Voxelize(inputMesh, targetResolution, GPUBackend=...)       BabelDatasetPreps.py:570, :667, :670, :673: float32 [N, 3] centres of the voxels inside
                                                                the skin, skull and CSF surfaces (host fallback: trimesh.voxelized(...).fill())
    voxelize_table(triangles, bounds, grid)                     the packed table (1 bit per voxel, the reference's packing)
    voxelize_mask(triangles, bounds, grid)                      bool [gx][gy][gz]
    voxelize_count(triangles, bounds, grid)                     the number of set voxels
    voxel_points(table, grid, origin, unit)                     the centres of a table's set voxels

The voxelisation runs on the MI355X through the C ABI (bfd_voxelize_mesh, bfd_voxel_points; csrc/bfd_voxelize.hip); there is no CPU fallback. Its
definition is in include/babelfdtd.h: float64, parity along x, top-left rule on shared edges; tests/voxelize_oracle.py restates it in numpy and the
device equals it voxel for voxel. The points come in ascending i + gx (j + gy k), the same in every run (the reference's order changes from run to
run). trimesh is not needed: a mesh is anything with `.triangles` of shape (n, 3, 3), or such an array. Argument errors are raised before the
library is loaded."""
import ctypes as C
import operator

import numpy as np

from . import _engine, _step1

_device = 0
last_kernel_ms = None
DEFAULT_RESOLUTION = 1333 / 500e3 / 6 * 0.75 * 1e3


def InitVoxelize(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as InitLabel does. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


def _triangles(inputMesh):
    """float32 C-contiguous [n][3][3] of a mesh object or an array, refused when not that shape or not finite."""
    t = getattr(inputMesh, 'triangles', inputMesh)
    t = np.asarray(t)
    if t.dtype.kind not in 'fiu':
        raise TypeError('triangles must be numbers, not %s' % t.dtype)
    if t.ndim != 3 or t.shape[1:] != (3, 3):
        raise ValueError('triangles must have shape (n, 3, 3), not %r' % (t.shape,))
    if t.shape[0] < 1:
        raise ValueError('the mesh has no triangle')
    with np.errstate(over='ignore'):
        t32 = np.ascontiguousarray(t, np.float32)
    if not np.all(np.isfinite(t32)):
        raise ValueError('a vertex coordinate is not finite (as float32)')
    return t32


def _bounds(bounds):
    r = np.asarray(bounds, np.float64)
    if r.shape != (2, 3):
        raise ValueError('bounds must have shape (2, 3): min and max')
    if not np.all(np.isfinite(r)):
        raise ValueError('the bounds are not finite')
    if not np.all(r[1] > r[0]):
        raise ValueError('the bounding box has no thickness on axis %d' % int(np.argmin(r[1] > r[0])))
    return np.ascontiguousarray(r)


def _grid(grid):
    try:
        g = tuple(operator.index(x) for x in grid)
    except TypeError:
        raise ValueError('grid must be three integers, not %r' % (grid,))
    if len(g) != 3 or min(g) < 1:
        raise ValueError('grid must be three integers of at least 1, not %r' % (grid,))
    if max(g) >= 2 ** 31 or g[0] * g[1] * g[2] > 2 ** 40:
        raise ValueError('the grid %r is too large (an extent of 2^31 or more, or more than 2^40 voxels)' % (g,))
    return g


def mesh_bounds(inputMesh):
    """float64 [2][3]: `.bounding_box.bounds` of a mesh object that has it (trimesh), otherwise min and max of the vertices as given."""
    bb = getattr(getattr(inputMesh, 'bounding_box', None), 'bounds', None)
    if bb is not None:
        return np.asarray(bb, np.float64)
    t = np.asarray(getattr(inputMesh, 'triangles', inputMesh), np.float64).reshape(-1, 3)
    return np.stack([t.min(axis=0), t.max(axis=0)])


def grid_rule(bounds, targetResolution):
    """The reference's grid (Voxelize.py:101-106): dims = max - min, g = ceil(dims / targetResolution), unit = dims / g. Returns (g, unit)."""
    r = _bounds(bounds)
    res = float(targetResolution)
    if not (np.isfinite(res) and res > 0):
        raise ValueError('targetResolution must be a positive finite number')
    dims = np.diff(r, axis=0).flatten()
    g = tuple(int(np.ceil(d / res)) for d in dims)
    return _grid(g), dims / np.array(g)


def _run(triangles, bounds, grid, want_table=False, want_mask=False):
    """(table or None, mask [gz][gy][gx] uint8 or None, count)"""
    global last_kernel_ms
    t, r, g = _triangles(triangles), _bounds(bounds), _grid(grid)
    n = g[0] * g[1] * g[2]
    if want_mask and n >= 2 ** 31:
        raise ValueError('a mask is written only below 2^31 voxels; ask for the table')
    table = np.empty((n + 31) // 32, np.uint32) if want_table else None
    mask = np.empty((g[2], g[1], g[0]), np.uint8) if want_mask else None
    count = C.c_int64()
    ms = C.c_float()
    lo, hi = np.ascontiguousarray(r[0]), np.ascontiguousarray(r[1])
    _step1.call('bfd_voxelize_mesh', _device, _engine._ptr(t), t.shape[0], _engine._ptr(lo), _engine._ptr(hi), g[0], g[1], g[2], _engine._ptr(table),
                _engine._ptr(mask), C.byref(count), C.byref(ms))
    last_kernel_ms = ms.value
    return table, mask, int(count.value)


def voxelize_table(triangles, bounds, grid):
    """uint32 [ceil(gx gy gz / 32)]: bit 31 - (index % 32) of word index / 32 is voxel index = i + gx (j + gy k)."""
    return _run(triangles, bounds, grid, want_table=True)[0]


def voxelize_mask(triangles, bounds, grid):
    """bool [gx][gy][gz] (a transposed view of the [gz][gy][gx] volume the device writes)."""
    return _run(triangles, bounds, grid, want_mask=True)[1].view(np.bool_).transpose(2, 1, 0)


def voxelize_count(triangles, bounds, grid):
    return _run(triangles, bounds, grid)[2]


def voxel_points(table, grid, origin, unit):
    """float32 [count][3]: (float32)(origin + (index + 0.5) unit) of every set voxel of the table, ascending in i + gx (j + gy k)."""
    global last_kernel_ms
    g = _grid(grid)
    tb = np.asarray(table)
    nt = (g[0] * g[1] * g[2] + 31) // 32
    if tb.dtype != np.uint32 or tb.ndim != 1 or tb.size != nt:
        raise ValueError('the table of a %r grid is uint32 [%d]' % (g, nt))
    tb = np.ascontiguousarray(tb)
    o, u = np.ascontiguousarray(origin, np.float64), np.ascontiguousarray(unit, np.float64)
    if o.shape != (3,) or u.shape != (3,) or not (np.all(np.isfinite(o)) and np.all(np.isfinite(u))):
        raise ValueError('origin and unit are three finite numbers each')
    count = C.c_int64()
    ms = C.c_float()
    args = (_device, _engine._ptr(tb), g[0], g[1], g[2], _engine._ptr(o), _engine._ptr(u))
    # the population is taken on the host, before a device is looked for: the refusal of capacity 0 sizes the array
    try:
        _step1.call('bfd_voxel_points', *args, None, 0, C.byref(count), None)
    except _engine.EngineError:
        if count.value == 0:            # an empty table is not refused for its capacity: this is another failure
            raise
    pts = np.empty((int(count.value), 3), np.float32)
    if pts.shape[0] > 0:
        _step1.call('bfd_voxel_points', *args, _engine._ptr(pts), pts.shape[0], C.byref(count), C.byref(ms))
    last_kernel_ms = ms.value
    return pts


def Voxelize(inputMesh, targetResolution=DEFAULT_RESOLUTION, GPUBackend=None):
    """float32 [N, 3]: the centres of the voxels inside the closed surface inputMesh, on the reference's grid (grid_rule of the mesh's bounds).
    inputMesh: anything with `.triangles` (n, 3, 3), or such an array; bounds from `.bounding_box.bounds` when present. GPUBackend is ignored."""
    global last_kernel_ms
    t = _triangles(inputMesh)
    r = _bounds(mesh_bounds(inputMesh))
    g, unit = grid_rule(r, targetResolution)
    table, _, _ = _run(t, r, g, want_table=True)
    ms = last_kernel_ms
    pts = voxel_points(table, g, r[0], unit)
    last_kernel_ms += ms
    return pts
