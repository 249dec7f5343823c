"""Timing record of the device median filter (bfd_median_filter3d): kernelMs (HIP events around the kernel) and the wall time of the whole
MedianFilter call (allocation, both copies, kernel), median of --reps after one warm-up, for
  - uint8 7x7x7 and 3x3x3 at 512 x 512 x 400 (a CT-resolution mask) on a 0/1 volume, a 0-5 label volume and a full-range volume
    (1, 3 and 8 radix rounds per voxel);
  - float32 3x3x3 at 320^3 unmasked and with a region of 10 % of the voxels (median_in_region).
The uint8 volumes are noise: every tile holds every value and takes every round, the upper bound. One more case is a 0/1 volume of blobs
(coarse noise thresholded) as a head mask is: tiles that hold one value with their halo take no round at all.
With scipy importable, scipy.ndimage.median_filter runs on the same host on a --scipy-edge^3 corner of the same volume and is printed as
microseconds per voxel with the whole-volume time that rate gives -- context, not a criterion, and an extrapolation, not a measurement.
Prints one JSON line last.

    python scripts/median_timing.py [--reps 3] [--scipy-edge 96] [--commit NAME]
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from babelbrain_amd import MedianFilter as MF


def smooth_field(shape, rng):
    """a cheap smooth random field in [0, 1): coarse noise repeated to the full grid, so that values form blobs of about 16 voxels"""
    c = rng.random(tuple(-(-n // 16) for n in shape), dtype=np.float32)
    return np.repeat(np.repeat(np.repeat(c, 16, 0), 16, 1), 16, 2)[:shape[0], :shape[1], :shape[2]]


def timed(fn, reps):
    fn()
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(MF.last_kernel_ms)
    return float(np.median(ms)), float(np.median(wall)), wall


def scipy_rate(a, size, edge):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    sub = np.ascontiguousarray(a[:edge, :edge, :edge])
    t0 = time.perf_counter()
    ndimage.median_filter(sub, size)
    return (time.perf_counter() - t0) / sub.size * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--scipy-edge', type=int, default=96)
    ap.add_argument('--mask-shape', type=int, nargs=3, default=[512, 512, 400])
    ap.add_argument('--field-edge', type=int, default=320)
    ap.add_argument('--commit', default='', help='what to name as the source state (default: git rev-parse of this checkout)')
    a = ap.parse_args()
    commit = a.commit
    if not commit:
        try:
            commit = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=os.path.dirname(os.path.abspath(__file__)),
                                             stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = 'unknown'
    rng = np.random.default_rng(0)
    devs = MF.InitMedianFilter()
    print('device: %s; commit %s; reps %d' % (devs[MF._device][1], commit, a.reps))
    res = {'commit': commit, 'device': devs[MF._device][1], 'cases': []}

    def case(name, vol, size, region=None):
        fn = (lambda: MF.MedianFilter(vol, size)) if region is None else (lambda: MF.median_in_region(vol, region, size))
        ms, wall, walls = timed(fn, a.reps)
        rate = scipy_rate(vol, size, a.scipy_edge) if a.scipy_edge > 0 else None
        line = '%-50s kernel %9.3f ms (%6.3f ns/voxel), call %8.1f ms' % (name, ms, ms * 1e6 / vol.size, wall)
        if rate is not None:
            line += '; scipy on this host, %d^3 corner: %.2f us/voxel = %.0f s for the whole volume (extrapolated)' % (a.scipy_edge, rate, rate * vol.size * 1e-6)
        print(line, flush=True)
        res['cases'].append({'name': name, 'voxels': int(vol.size), 'kernel_ms': ms, 'call_ms': wall, 'call_ms_repetitions': walls,
                             'scipy_us_per_voxel_extrapolated': rate})

    shape = tuple(a.mask_shape)
    for name, top in (('uint8 0/1', 2), ('uint8 labels 0-5', 6), ('uint8 full range', 256)):
        v = rng.integers(0, top, shape, dtype=np.uint8)
        for size in (7, 3):
            case('%s, %d^3, %d x %d x %d' % ((name, size) + shape), v, size)
    v = (smooth_field(shape, rng) > 0.5).astype(np.uint8)
    for size in (7, 3):
        case('uint8 0/1 blobs, %d^3, %d x %d x %d' % ((size,) + shape), v, size)
    del v
    e = a.field_edge
    p = (smooth_field((e, e, e), rng) * 1e5 + rng.standard_normal((e, e, e), dtype=np.float32) * 1e3).astype(np.float32)
    case('float32, 3^3, %d^3' % e, p, 3)
    region = smooth_field((e, e, e), rng) < 0.1
    case('float32, 3^3, %d^3, region %.1f %%' % (e, 100.0 * region.mean()), p, 3, region)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
