"""The definition of the mesh voxelisation (include/babelfdtd.h, bfd_voxelize_mesh) restated in numpy: float64, one operation per rounding, in the
order the header gives, so that the device, which performs the same IEEE operations, is held to equality. Shared by test_voxelize_host.py (where it
is itself checked against analytic solids) and test_voxelize_gpu.py. Also the mesh builders of both and the host loop of the CT value mapping."""
import numpy as np


def unit_of(bmin, bmax, grid):
    return (np.asarray(bmax, np.float64) - np.asarray(bmin, np.float64)) / np.asarray(grid, np.float64)


def voxelize(triangles, bmin, bmax, grid, want_passes=False):
    """bool [gx][gy][gz] (the mask's transpose in memory order [gz][gy][gx] is what the library writes). With want_passes also
    (passes [gy][gz]: how many triangles passed test (a) per column; atomics: crossings issued; ref_atomics: the sum of xmax + 1 over the same pairs,
    clamped to gx, which the per-voxel formulation would issue)."""
    tri = np.asarray(triangles, np.float32).astype(np.float64)
    bmin = np.asarray(bmin, np.float64)
    gx, gy, gz = (int(g) for g in grid)
    u = unit_of(bmin, bmax, grid)
    cross = np.zeros((gx + 1, gy, gz), np.int64)              # crossings at position c = min(floor(q), gx - 1) + 1
    passes = np.zeros((gy, gz), np.int64)
    atomics = ref_atomics = 0
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for t in tri:
            v0, v1, v2 = t[0] - bmin, t[1] - bmin, t[2] - bmin
            ay, az, by, bz, cy, cz = v0[1], v0[2], v1[1], v1[2], v2[1], v2[2]
            area = (by - ay) * (cz - az) - (cy - ay) * (bz - az)
            if area == 0:
                continue
            if area < 0:
                by, bz, cy, cz = cy, cz, by, bz
            jl = max(np.ceil(min(ay, by, cy) / u[1] - 0.5), 0.0)
            jh = min(np.floor(max(ay, by, cy) / u[1] - 0.5), gy - 1.0)
            kl = max(np.ceil(min(az, bz, cz) / u[2] - 0.5), 0.0)
            kh = min(np.floor(max(az, bz, cz) / u[2] - 0.5), gz - 1.0)
            if not (jl <= jh and kl <= kh):
                continue
            j = np.arange(int(jl), int(jh) + 1)[:, None]
            k = np.arange(int(kl), int(kh) + 1)[None, :]
            py = np.broadcast_to((j + 0.5) * u[1], (j.size, k.size))
            pz = np.broadcast_to((k + 0.5) * u[2], (j.size, k.size))
            inside = np.ones(py.shape, bool)
            for (a0, a1), (b0, b1) in (((ay, az), (by, bz)), ((by, bz), (cy, cz)), ((cy, cz), (ay, az))):
                e = (py - a0) * (pz - b1) - (pz - a1) * (py - b0)
                topleft = b1 < a1 or (b1 == a1 and a0 > b0)
                inside &= (e > 0) | ((e == 0) & topleft)
            if not inside.any():
                continue
            e0, e1 = v1 - v0, v2 - v1
            nx = e0[1] * e1[2] - e0[2] * e1[1]
            ny = e0[2] * e1[0] - e0[0] * e1[2]
            nz = e0[0] * e1[1] - e0[1] * e1[0]
            xs = v0[0] - (ny * (py - v0[1]) + nz * (pz - v0[2])) / nx
            q = np.floor(xs / u[0] - 0.5)
            hit = inside & (q >= 0)                           # NaN compares false
            jj, kk = np.nonzero(hit)
            c = np.minimum(q[jj, kk], gx - 1.0).astype(np.int64) + 1
            cross[c, jj + int(jl), kk + int(kl)] += 1         # a triangle meets a column once: no repeated index
            passes[int(jl):int(jh) + 1, int(kl):int(kh) + 1] += inside
            atomics += jj.size
            ref_atomics += int(c.sum())
    above = np.cumsum(cross[::-1], axis=0)[::-1]              # above[c] = crossings at positions >= c
    mask = (above[1:] & 1).astype(bool)                       # voxel i: positions > i
    return (mask, passes, atomics, ref_atomics) if want_passes else mask


def pack_table(mask):
    """uint32 [ceil(n / 32)]: bit 31 - (index % 32) of word index / 32, index = i + gx (j + gy k)."""
    flat = np.ascontiguousarray(mask.transpose(2, 1, 0)).ravel()
    pad = (-flat.size) % 32
    bits = np.concatenate([flat, np.zeros(pad, bool)]).astype(np.uint8)
    return np.packbits(bits).view('>u4').astype(np.uint32)


def points_of(mask, bmin, unit):
    """float32 [count][3]: the centres of the set voxels in ascending i + gx (j + gy k), each coordinate formed in float64 and rounded once."""
    k, j, i = np.nonzero(mask.transpose(2, 1, 0))
    idx = np.stack([i, j, k], axis=1).astype(np.float64)
    return (np.asarray(bmin, np.float64) + (idx + 0.5) * np.asarray(unit, np.float64)).astype(np.float32)


def inside_polyhedron(triangles, pts):
    """Analytic yardstick for CONVEX closed meshes with outward normals: a point is inside iff it is on the inner side of every face plane.
    Returns (inside, margin): margin = the smallest |signed distance numerator| relative to its scale, to tell centres that sit on a face."""
    tri = np.asarray(triangles, np.float32).astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 1])
    d = np.einsum('pa,ta->pt', pts, n) - np.einsum('ta,ta->t', tri[:, 0], n)[None, :]
    return (d < 0).all(axis=1), np.abs(d).min(axis=1)


# ---------------------------------------------------------------- meshes ----------------------------------------------------------------

def box_triangles(lo, hi):
    """12 triangles of an axis-aligned box, outward normals."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = np.array([[lo[0] if not (m & 1) else hi[0], lo[1] if not (m & 2) else hi[1], lo[2] if not (m & 4) else hi[2]] for m in range(8)])
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]
    f = []
    for a, b, cc, d in quads:
        f += [(a, b, cc), (a, cc, d)]
    return c[np.array(f)].astype(np.float32)


def icosphere(level):
    """Unit icosphere: 20 * 4^level triangles, outward normals, float64 vertices and int faces."""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f)


def rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def ellipsoid_triangles(level, radii, seed, centre=(0.0, 0.0, 0.0)):
    """A randomly rotated ellipsoidal icosphere (convex, outward normals), float32 [n][3][3]."""
    v, f = icosphere(level)
    v = (v * np.asarray(radii, np.float64)) @ rotation(seed).T + np.asarray(centre, np.float64)
    return v[f].astype(np.float32)


def bounds_of(triangles):
    t = np.asarray(triangles, np.float32).astype(np.float64).reshape(-1, 3)
    return t.min(axis=0), t.max(axis=0)


# ---------------------------------------------------------------- CT value mapping ----------------------------------------------------------------

def map_values_host_loop(hu, sel, unique):
    """The host fallback of the reference's Step 1, literally: one full-volume comparison per unique value."""
    out = np.zeros(hu.shape, np.uint32)
    for n, d in enumerate(unique):
        out[hu == d] = n
    out[sel == 0] = 0
    return out


def map_values(hu, sel, unique):
    m = np.minimum(np.searchsorted(unique, hu), unique.size - 1)
    with np.errstate(invalid='ignore'):
        hit = (unique[m] == hu) & (sel != 0)
    return np.where(hit, m, 0).astype(np.uint32)
