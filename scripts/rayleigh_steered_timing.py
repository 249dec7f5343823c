"""Device time of the element-resolved Rayleigh integral against the single-field call, same process, same inputs.

A phased array of 128 elements x 1100 sub-sources (the size INTEGRATION.md section 3 quotes for the 750 kHz array) against 2^22
field points (about 1/22 of that grid, so that a call takes under a second). Reports kernelMs, median of 5 after one warm-up, of
  - one bfd_rayleigh_forward call (ForwardSimple): the yardstick, unchanged by this feature;
  - ForwardSteered at S = 1, 8 and 16 columns;
and, in wall time, ForwardElements at one field point against the loop of 128 ForwardSimple calls it replaces
(BabelIntegrationH246.py:333-339). Prints one JSON line last.

    python scripts/rayleigh_steered_timing.py [--points 4194304] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from babelbrain_amd import harness as H, RayleighAndBHTE as R


def median_ms(fn, reps):
    fn()                                      # warm-up
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(R.last_kernel_ms)
    return float(np.median(ms)), float(np.median(wall)), [round(v, 3) for v in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=1 << 22)
    ap.add_argument('--elements', type=int, default=128)
    ap.add_argument('--records', type=int, default=1100)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    nE, per, N = a.elements, a.records, a.points
    M = nE * per
    pts, ds = H._bowl_points(150e-3, 160e-3, 220, 0.0)
    assert len(ds) >= M
    cen, ds = pts[:M].astype(np.float32), ds[:M].astype(np.float32)
    rng = np.random.default_rng(0)
    rf = np.stack([rng.uniform(-50e-3, 50e-3, N), rng.uniform(-50e-3, 50e-3, N), rng.uniform(60e-3, 200e-3, N)], 1).astype(np.float32)
    k = 2 * np.pi * 750e3 / 1500.0
    ec = cen.reshape(nE, per, 3).mean(axis=1)
    foci = np.stack([rng.uniform(-10e-3, 10e-3, 16), rng.uniform(-10e-3, 10e-3, 16), rng.uniform(130e-3, 170e-3, 16)], 1)
    W = H.steering_weights(k, ec, foci)
    u0 = np.repeat(W[:, 0], per)
    res = {'elements': nE, 'records_per_element': per, 'points': N, 'reps': a.reps}
    pairs = M * N

    ms, wall, all_ms = median_ms(lambda: R.ForwardSimple(k, cen, ds, u0, rf), a.reps)
    res['forward_simple_ms'] = ms
    print('bfd_rayleigh_forward          : kernel %9.2f ms  %s  (%.0f Gpairs/s), call %.0f ms' % (ms, all_ms, pairs / ms / 1e6, wall))
    base = ms
    for S in (1, 8, 16):
        ms, wall, all_ms = median_ms(lambda: R.ForwardSteered(k, cen, ds, per, W[:, :S], rf), a.reps)
        res['steered_S%d_ms' % S] = ms
        res['steered_S%d_over_single' % S] = ms / base
        print('ForwardSteered S = %2d         : kernel %9.2f ms  %s  = %.2f x one single-field call, %.2f x per field; call %.0f ms' % (
            S, ms, all_ms, ms / base, ms / base / S, wall))
    ms, wall, all_ms = median_ms(lambda: R.ForwardElements(k, cen, ds, per, rf[:1 << 18]), a.reps)
    res['elements_2p18_points_ms'] = ms
    print('ForwardElements, 2^18 points  : kernel %9.2f ms  %s  (%.0f Gpairs/s)' % (ms, all_ms, M * (1 << 18) / ms / 1e6))

    point = rf[:1]
    ones = np.ones(per, np.complex64)

    def loop():
        return np.array([R.ForwardSimple(k, cen[e * per:(e + 1) * per], ds[e * per:(e + 1) * per], ones, point)[0] for e in range(nE)])
    ms, wall_one, _ = median_ms(lambda: R.ForwardElements(k, cen, ds, per, point), a.reps)
    _, wall_loop, _ = median_ms(loop, a.reps)
    res.update(elements_one_point_kernel_ms=ms, elements_one_point_wall_ms=wall_one, loop_of_calls_wall_ms=wall_loop)
    print('ForwardElements, one point    : kernel %9.3f ms, call %.2f ms; loop of %d ForwardSimple calls %.2f ms' % (ms, wall_one, nE, wall_loop))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
