"""The definition of the conformal-mask scatter (include/babelfdtd.h, bfd_voxel_scatter3d) restated in numpy: the points of a table, the float32
transform with one operation per rounding in the header's order (elementwise operations only, never np.dot, whose BLAS may fuse or reorder), the
half-to-even rounding, numpy's index rules behind the reference's filter of the upper side, the bounds and the four counts. The device, which performs
the same IEEE operations, is held to equality. Shared by test_conformal_host.py and test_conformal_gpu.py; also the flow of BabelDatasetPreps.py:696-759
over lists of points, in this project's own words."""
import numpy as np

from tests import voxelize_oracle as VO

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def table_mask(table, grid):
    """bool [gz][gy][gx] of a table in bfd_voxelize_mesh's packing; padding bits are ignored."""
    gx, gy, gz = (int(g) for g in grid)
    bits = np.unpackbits(np.asarray(table, np.uint32).astype('>u4').view(np.uint8))
    return bits[:gx * gy * gz].reshape(gz, gy, gx).astype(bool)


def table_points(table, grid, origin, unit):
    """float32 [count][3]: the points of bfd_voxel_points, ascending in i + gx (j + gy k)."""
    k, j, i = np.nonzero(table_mask(table, grid))
    idx = np.stack([i, j, k], axis=1).astype(np.float64)
    return (np.asarray(origin, np.float64) + (idx + 0.5) * np.asarray(unit, np.float64)).astype(np.float32)


def transform(points, matrix):
    """float32 [n][3]: t_a = ((m_a0 x + m_a1 y) + m_a2 z) + m_a3, every product and sum a float32 operation of its own."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    m = np.asarray(matrix, np.float32).reshape(-1)[:12].reshape(3, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(over='ignore', invalid='ignore'):
        t = [((m[a, 0] * x + m[a, 1] * y) + m[a, 2] * z) + m[a, 3] for a in range(3)]
    assert all(c.dtype == np.float32 for c in t)
    return np.stack(t, axis=1)


def indices(t):
    """int64 [n][3]: rint half to even, saturated to the int32 range; NaN and -inf count as below, +inf as above."""
    t = np.asarray(t, np.float32)
    with np.errstate(invalid='ignore'):
        n = np.where(t >= np.float32(2.0 ** 31), I32_MAX, 0).astype(np.int64)
        low = ~(t > np.float32(-2.0 ** 31))
        mid = ~low & ~(t >= np.float32(2.0 ** 31))
    n[low] = I32_MIN
    n[mid] = np.round(t[mid]).astype(np.int64)
    return n


def scatter(points, matrix, shape=None):
    """(out uint8 [M1][M2][M3] or None, lo int64 [3] or None, hi, counts int64 [4] = points, above, wrapped, below). shape None: the bounds pass."""
    n = indices(transform(points, matrix))
    counts = np.zeros(4, np.int64)
    counts[0] = n.shape[0]
    lo, hi = (n.min(axis=0), n.max(axis=0)) if n.shape[0] else (None, None)
    if shape is None:
        return None, lo, hi, counts
    M = np.asarray(shape, np.int64)
    out = np.zeros(tuple(int(v) for v in M), np.uint8)
    above = (n >= M).any(axis=1)
    below = ~above & (n < -M).any(axis=1)
    keep = ~above & ~below
    wrapped = keep & (n < 0).any(axis=1)
    counts[1:] = above.sum(), wrapped.sum(), below.sum()
    k = n[keep]
    out[k[:, 0], k[:, 1], k[:, 2]] = 1                      # numpy's own rule wraps the negative indices
    return out, lo, hi, counts


def focal_index(matrix, location):
    """int64 [3]: the index of one point under the same float32 rule."""
    return indices(transform(np.asarray(location, np.float32).reshape(1, 3), matrix))[0]


def conformal_flow(skin_pts, skull_pts, csf_pts, SpatialStep, RMat, Location):
    """BabelDatasetPreps.py:696-759 over three lists of float32 points, with `transform` in the place of np.dot:
    (baseaffineRot float64 [4][4], LocFocalPoint int64 [3], skin int8, skull int8, csf uint8)."""
    affine = np.eye(4)
    affine[:3, :3] = np.asarray(RMat, np.float64) * SpatialStep
    inv = np.linalg.inv(affine).astype(np.float32)
    first = indices(transform(skin_pts, inv[:3]))
    affine[:, 3] = affine @ np.array([first[:, 0].min(), first[:, 1].min(), first[:, 2].min(), 1.0])
    inv = np.linalg.inv(affine).astype(np.float32)
    ijk = np.vstack([indices(transform(skin_pts, inv[:3])), focal_index(inv[:3], Location)])
    focal = ijk[-1].copy()
    shape = tuple(int(v) for v in ijk.max(axis=0) + 1)
    skin = np.zeros(shape, np.int8)
    skin[ijk[:, 0], ijk[:, 1], ijk[:, 2]] = 1               # the focal point is stored too (line 728 indexes with it)
    masks = []
    for pts, dtype in ((skull_pts, np.int8), (csf_pts, np.uint8)):
        n = indices(transform(pts, inv[:3]))
        n = n[(n[:, 0] < shape[0]) & (n[:, 1] < shape[1]) & (n[:, 2] < shape[2])]
        m = np.zeros(shape, dtype)
        m[n[:, 0], n[:, 1], n[:, 2]] = 1
        masks.append(m)
    return affine, focal, skin, masks[0], masks[1]


# ---------------------------------------------------------------- what the tests of both files share ----------------------------------------------------------------

def random_table(grid, seed, fill=0.5):
    """A random table with garbage in the padding bits of its last word."""
    n = grid[0] * grid[1] * grid[2]
    rng = np.random.default_rng(seed)
    bits = (rng.random(((n + 31) // 32) * 32) < fill).astype(np.uint8)
    bits[n:] = 1
    return np.packbits(bits).view('>u4').astype(np.uint32)


def agree(got, want, what=''):
    """out, lo, hi and all four counts, by equality; lo and hi only where there is a point"""
    out, lo, hi, counts = got
    wout, wlo, whi, wcounts = want
    assert np.array_equal(counts, wcounts), (what, counts, wcounts)
    if wcounts[0]:
        assert np.array_equal(lo, wlo) and np.array_equal(hi, whi), (what, lo, wlo, hi, whi)
    assert (out is None) == (wout is None), what
    if wout is not None:
        assert out.shape == wout.shape and np.count_nonzero(out != wout) == 0, what


def rotated_matrix(seed, step, offset):
    """The first three rows of inv(affine), affine = rotation * step with an origin, cast to float32 as the reference casts InVAffineRot."""
    a = np.eye(4)
    a[:3, :3] = VO.rotation(seed) * step
    a[:3, 3] = offset
    return np.linalg.inv(a).astype(np.float32)[:3]


def rotated_about(seed, step, centre, index):
    """As rotated_matrix, with the origin placed so that the point `centre` gets the index `index` (before rounding)."""
    r = VO.rotation(seed) * step
    return rotated_matrix(seed, step, np.asarray(centre, np.float64) - r @ np.asarray(index, np.float64))
