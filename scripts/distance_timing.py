"""Timing record of the device distance transform (bfd_distance_transform_edt3d) and Gaussian filter (bfd_gaussian_filter3d): kernelMs (HIP events
around the kernels) and the wall time of the whole call (allocation, both copies, kernels), median of --reps after one warm-up, at 448 x 448 x 384:
  - the transform of a shell mask (a skull-like ellipsoidal shell, invert=True: the distance to the shell), float64 out, and the squared int32 alone;
  - the filter of a float32 volume at sigma 3 (three axes, radius 12).
With each: the bytes the passes must move at the least and the fraction of 8 TB/s that the kernel time makes of them.
  transform   pack 1 B read; rows 4 B written; two line passes, each 4 B read + 4 B written (the stacks come on top: up to 8 B written and 8 B read per
              voxel and pass, as deep as the envelope gets); root 4 B read + 8 B written: 33 B per voxel with the root, 21 B without
  filter      4 B read + 4 B written per voxel and filtered axis: 24 B per voxel
scipy.ndimage runs the same two calls on the same host at --scipy-shape (default: the same size), once each: context, not a criterion.
Prints one JSON line last.

    python scripts/distance_timing.py [--reps 5] [--shape 448 448 384] [--scipy-shape 448 448 384]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from babelbrain_amd import DistanceTransform as DT, GaussianFilter as GF

PEAK = 8e12


def shell_mask(shape):
    g = np.meshgrid(*[((np.arange(n, dtype=np.float32) - (n - 1) / 2) / (n / 2)) for n in shape], indexing='ij', sparse=True)
    rad = np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2)
    return ((rad < 0.85) & (rad >= 0.75)).astype(np.uint8)


def timed(fn, module, reps):
    fn()
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(module.last_kernel_ms)
    return float(np.median(ms)), float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shape', type=int, nargs=3, default=[448, 448, 384])
    ap.add_argument('--scipy-shape', type=int, nargs=3, default=None, help='0 0 0: no scipy run')
    a = ap.parse_args()
    shape = tuple(a.shape)
    sshape = tuple(a.scipy_shape) if a.scipy_shape else shape
    devs = DT.InitDistanceTransform()
    GF.InitGaussianFilter()
    n = int(np.prod(shape))
    print('device: %s; %d x %d x %d = %d voxels; reps %d' % ((devs[DT._device][1],) + shape + (n, a.reps)))
    res = {'device': devs[DT._device][1], 'shape': shape, 'cases': []}

    def case(name, fn, module, bytes_per_voxel):
        ms, wall = timed(fn, module, a.reps)
        gbs = bytes_per_voxel * n / (ms * 1e-3) / 1e9
        print('%-44s kernel %8.3f ms, call %8.1f ms; %2d B/voxel at the least = %.2f GB -> %6.0f GB/s = %.1f %% of 8 TB/s' %
              (name, ms, wall, bytes_per_voxel, bytes_per_voxel * n / 1e9, gbs, 100 * gbs * 1e9 / PEAK), flush=True)
        res['cases'].append({'name': name, 'kernel_ms': ms, 'call_ms': wall, 'min_bytes': bytes_per_voxel * n, 'fraction_of_8TBs': gbs * 1e9 / PEAK})

    mask = shell_mask(shape)
    case('distance transform, float64 out', lambda: DT.distance_transform_edt(mask, invert=True), DT, 33)
    case('distance transform, squared int32 out', lambda: DT.distance_transform_edt(mask, invert=True, squared=True), DT, 21)
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(shape, dtype=np.float32) * 700 + 300) * mask
    case('gaussian filter, float32, sigma 3', lambda: GF.gaussian_filter(x, 3.0), GF, 24)
    for s, nm in (((3.0, 0, 0), 'axis 0'), ((0, 3.0, 0), 'axis 1'), ((0, 0, 3.0), 'axis 2')):
        case('gaussian filter, float32, sigma 3, %s alone' % nm, lambda s=s: GF.gaussian_filter(x, s), GF, 8)

    if all(sshape):
        from scipy import ndimage
        sm = shell_mask(sshape)
        t0 = time.perf_counter()
        ndimage.distance_transform_edt(1 - sm)
        t_edt = time.perf_counter() - t0
        sx = np.ascontiguousarray(x[:sshape[0], :sshape[1], :sshape[2]])
        t0 = time.perf_counter()
        ndimage.gaussian_filter(sx, 3.0)
        t_g = time.perf_counter() - t0
        print('scipy on this host at %d x %d x %d: distance_transform_edt %.2f s, gaussian_filter(sigma 3) %.2f s' % (sshape + (t_edt, t_g)))
        res['scipy'] = {'shape': sshape, 'edt_s': t_edt, 'gaussian_s': t_g}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
