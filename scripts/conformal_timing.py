"""Timing record of the conformal masks on the device (bfd_voxel_scatter3d, bfd_voxelize_scatter3d; babelbrain_amd/ConformalMask.py), on the two
head-sized cases of scripts/voxelize_timing.py (a closed ellipsoid of 500,000 triangles on 868 x 900 x 683, and the same surface clipped by a box) under
a rotated matrix at ratio 0.75 (targetResolution = 0.75 SpatialStep), the origin and the mask's shape found as BabelDatasetPreps.py:710-727 finds them:
  - kernelMs (HIP events) of the bounds pass and of the scatter alone, from the mesh's table (memset of the mask and one kernel);
  - kernelMs and wall time of the fused call, mesh to mask (voxelisation, memset, scatter; the triangles up, the mask down);
  - the whole conformal_masks call on three nested copies of the surface (five device calls), wall time;
  - the path before this entry existed, on the same box: Voxelize (the points copied to the host) and the reference's host lines restated in
    numpy (hstack, float32 np.dot, np.round, int64 cast, filter of the upper side, fancy-index store), per mesh, for cases of at most
    --host-max-points points (it needs about 90 B of host memory per point: 25 GB at 277 M points; 0 leaves it out).
Median of --reps after one warm-up. Prints one JSON line last.

    python scripts/conformal_timing.py [--reps 3] [--host-max-points 300000000] [--case 0|1]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from babelbrain_amd import ConformalMask as CM, Voxelize as VX
from voxelize_timing import cases


def rotation():
    c, s = np.cos(0.4), np.sin(0.4)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]) @ np.array([[1.0, 0.0, 0.0], [0.0, np.cos(0.25), -np.sin(0.25)], [0.0, np.sin(0.25), np.cos(0.25)]])


def timed(fn, reps):
    fn()
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(CM.last_kernel_ms)
    return float(np.median(ms)), float(np.median(wall))


def host_lines(pts, inv32, shape):
    """BabelDatasetPreps.py:736-744 in numpy, as the reference's host does them"""
    xyz = np.hstack((pts, np.ones((pts.shape[0], 1), dtype=pts.dtype))).T
    ijk = np.round(np.dot(inv32, xyz)).astype(np.int64).T
    mask = np.zeros(shape, np.int8)
    inds = (ijk[:, 0] < shape[0]) & (ijk[:, 1] < shape[1]) & (ijk[:, 2] < shape[2])
    ijk = ijk[inds, :]
    mask[ijk[:, 0], ijk[:, 1], ijk[:, 2]] = 1
    return mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-max-points', type=int, default=300000000)
    ap.add_argument('--case', type=int, default=None)
    a = ap.parse_args()
    devs = CM.InitConformal()
    VX.InitVoxelize()
    res = {'device': devs[CM._device][1], 'cases': []}
    for q, (name, tri, b, g) in enumerate(cases()):
        if a.case is not None and q != a.case:
            continue
        unit = (b[1] - b[0]) / np.array(g)
        step = float(unit.max()) / 0.75
        affine = np.eye(4)
        affine[:3, :3] = rotation() * step
        lo, _, n = CM.rotated_bounds(tri, np.linalg.inv(affine), bounds=b, grid=g)
        affine[:, 3] = affine @ np.array([lo[0], lo[1], lo[2], 1.0])
        inv32 = np.linalg.inv(affine).astype(np.float32)
        _, hi, _ = CM.rotated_bounds(tri, inv32, bounds=b, grid=g)
        shape = tuple(int(v) + 1 for v in hi)
        row = {'case': name, 'triangles': len(tri), 'grid': g, 'points': n, 'mask_shape': shape, 'mask_bytes': int(np.prod(shape))}
        print('%s: %d triangles, grid %r, %d points -> mask %r' % (name, len(tri), g, n, shape), flush=True)
        table = VX.voxelize_table(tri, b, g)
        tk = dict(grid=g, origin=b[0], unit=unit)
        row['bounds_kernel_ms'], row['bounds_from_table_call_ms'] = timed(lambda: CM.rotated_bounds(table, inv32, **tk), a.reps)
        out = {}

        def scatter_table():
            out['mask'] = CM.scatter_mask(table, inv32, shape, **tk)
        row['scatter_kernel_ms'], row['scatter_from_table_call_ms'] = timed(scatter_table, a.reps)
        row['set_voxels'] = int(out['mask'].sum())
        row['counts'] = [int(v) for v in CM.last_counts]
        row['fused_kernel_ms'], row['fused_call_ms'] = timed(lambda: CM.scatter_mask(tri, inv32, shape, bounds=b, grid=g), a.reps)
        print('  bounds %.3f ms, scatter (memset + kernel) %.3f ms; fused mesh -> mask: kernels %.3f ms, call %.1f ms' %
              (row['bounds_kernel_ms'], row['scatter_kernel_ms'], row['fused_kernel_ms'], row['fused_call_ms']), flush=True)
        if q == 0:
            meshes = [tri, tri * np.float32(0.93), tri * np.float32(0.86)]
            res_mm = float(unit.max())
            row['conformal_masks_kernel_ms'], row['conformal_masks_call_ms'] = timed(
                lambda: CM.conformal_masks(meshes[0], meshes[1], meshes[2], step, rotation(), (1.0, 2.0, 3.0), targetResolution=res_mm), a.reps)
            print('  conformal_masks, three meshes: kernels %.3f ms, call %.1f ms' % (row['conformal_masks_kernel_ms'], row['conformal_masks_call_ms']), flush=True)
        if n <= a.host_max_points:
            t0 = time.perf_counter()
            pts = VX.voxel_points(table, g, b[0], unit)
            t1 = time.perf_counter()
            ref = host_lines(pts, inv32, shape)
            t2 = time.perf_counter()
            row['points_to_host_ms'], row['host_lines_ms'] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
            row['voxels_differing_from_host_lines'] = int(np.count_nonzero(ref != out['mask'].view(np.int8)))
            print('  before: the points to the host %.0f ms, the host lines %.0f ms per mesh; voxels that differ from the device mask: %d' %
                  (row['points_to_host_ms'], row['host_lines_ms'], row['voxels_differing_from_host_lines']), flush=True)
            del pts, ref
        res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
