"""python scripts/voxelize_timing.py [counts]   Head-sized measurement of the Step-1 voxelisation and CT value mapping: a closed ellipsoid of about 5e5 triangles
on about 900 x 900 x 700 voxels; the same surface inside a clipping box together with the box's 12 faces (a few triangles that cover every column); MapFilter
on 448 x 448 x 384 with 1024 unique values. Device events through the ABI, median of three after a warm-up, wall time of the whole call around it.
`counts` (no device needed, minutes of numpy) prints the atomics issued against the sum of xmax + 1 the per-voxel formulation would issue."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from babelbrain_amd import MappingFilter as MF, Voxelize as VX

def ellipsoid(nlat=500, nlon=500, radii=(90.0, 95.0, 70.0)):
    """A latitude-longitude ellipsoid, slightly rotated: 2 nlon nlat triangles, float32 [n][3][3]"""
    th = np.linspace(0.0, np.pi, nlat + 1)[:, None]
    ph = np.linspace(0.0, 2 * np.pi, nlon, endpoint=False)[None, :]
    v = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th) * np.ones_like(ph)], -1) * np.array(radii)
    a, b = v[:-1], v[1:]
    a2, b2 = np.roll(a, -1, axis=1), np.roll(b, -1, axis=1)
    tri = np.concatenate([np.stack([a, b, b2], -2).reshape(-1, 3, 3), np.stack([a, b2, a2], -2).reshape(-1, 3, 3)])     # 2 nlon of them, at the poles, have no area
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, np.cos(0.2), -np.sin(0.2)], [0.0, np.sin(0.2), np.cos(0.2)]])
    return (tri @ R.T).astype(np.float32)

def box_faces(lo, hi):
    c = np.array([[lo[0] if not (m & 1) else hi[0], lo[1] if not (m & 2) else hi[1], lo[2] if not (m & 4) else hi[2]] for m in range(8)])
    f = []
    for p, q, r, s in [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]:
        f += [(p, q, r), (p, r, s)]
    return c[np.array(f)].astype(np.float32)

def cases():
    tri = ellipsoid()
    lo, hi = tri.reshape(-1, 3).min(axis=0).astype(np.float64), tri.reshape(-1, 3).max(axis=0).astype(np.float64)
    res = float(np.max((hi - lo) / np.array([900, 900, 700])))
    full = ('closed ellipsoid', tri, np.stack([lo, hi]), VX.grid_rule(np.stack([lo, hi]), res)[0])
    blo, bhi = lo * np.array([0.55, 0.9, 0.6]), hi * np.array([0.7, 0.5, 0.9])
    inside = np.all((tri.mean(axis=1) >= blo) & (tri.mean(axis=1) <= bhi), axis=1)
    cut = np.concatenate([tri[inside], box_faces(blo, bhi) * np.float32(0.999)])
    clipped = ('clipped by a box, with the box faces', cut, np.stack([blo, bhi]), VX.grid_rule(np.stack([blo, bhi]), res)[0])
    return [full, clipped]

def median3(fn):
    rows = []
    for rep in range(4):                                           # rep 0 warms up
        t0 = time.perf_counter(); ms = fn(); rows.append((ms, (time.perf_counter() - t0) * 1e3))
    k = sorted(r[0] for r in rows[1:]); w = sorted(r[1] for r in rows[1:])
    return {'kernel_ms_min_median_max': [k[0], k[1], k[2]], 'wall_ms_median': w[1], 'wall_ms_min_max': [w[0], w[2]]}

if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'counts':
        from tests import voxelize_oracle as VO
        for name, tri, b, g in cases():
            m, _, issued, ref = VO.voxelize(tri, b[0], b[1], g, want_passes=True)
            print(json.dumps({'case': name, 'triangles': len(tri), 'grid': g, 'set_voxels': int(m.sum()), 'atomics_issued': issued,
                              'per_voxel_formulation_atomics': ref, 'ratio': ref / max(issued, 1)}), flush=True)
        sys.exit(0)
    VX.InitVoxelize()
    for name, tri, b, g in cases():
        out = {}
        def vox():
            out['table'] = VX.voxelize_table(tri, b, g)
            return VX.last_kernel_ms
        r = median3(vox)
        unit = (b[1] - b[0]) / np.array(g)
        def pts():
            out['n'] = VX.voxel_points(out['table'], g, b[0], unit).shape[0]
            return VX.last_kernel_ms
        p = median3(pts)
        print(json.dumps({'case': name, 'triangles': len(tri), 'grid': g, 'voxels': int(np.prod(g)), 'set_voxels': out['n'], 'voxelize': r, 'points': p}), flush=True)
    rng = np.random.default_rng(0)
    uni = np.unique(rng.uniform(-1000.0, 3000.0, 4096).astype(np.float32))[:1024]
    hu = uni[rng.integers(0, uni.size, (448, 448, 384))]
    sel = (rng.random(hu.shape) < 0.5).astype(np.uint8)
    def mp():
        MF.MapFilter(hu, sel, uni)
        return MF.last_kernel_ms
    r = median3(mp)
    alg = hu.size * 9
    r.update({'case': 'MapFilter 448x448x384, 1024 unique values', 'algorithmic_bytes': alg, 'fraction_of_8TBps': alg / (r['kernel_ms_min_median_max'][1] * 1e-3) / 8e12})
    print(json.dumps(r), flush=True)
