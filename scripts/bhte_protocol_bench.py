#!/usr/bin/env python3
"""A repeated-sonication thermal protocol (CalculateTemperatureEffects.py:259-460) two ways, on the same seeded inputs:
one RunBHTECycles call (bfd_bhte_run_protocol: one upload, one download, captures on the device) against the reference's
loop restated over the existing BHTE drop-in (one call per ON period, OFF period and group pause; T and dose through the
host in between). Prints one JSON line: wall seconds and kernel ms of both, host<->device bytes of both computed from the
shapes (what the calls copy, not a measurement), and whether all six returns are array_equal.

  python scripts/bhte_protocol_bench.py [--grid 280 276 272] [--out FILE]

Default protocol: ~21 M voxels, dt = 0.01 s, 1 s ON, 4 s OFF, 10 repetitions per group, 3 groups, 20 s between groups."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from babelbrain_amd import RayleighAndBHTE as R  # noqa: E402


def materials():
    # water, skin, cortical, trabecular, brain (CalculateTemperatureEffects.py:780-791, acoustic columns at 500 kHz)
    return {'Density': np.array([1000.0, 1116.0, 1896.5, 1738.0, 1041.0]), 'SoS': np.array([1500.0, 1537.0, 2476.0, 2205.0, 1562.0]),
            'Attenuation': np.array([0.0, 2.3, 81.0, 81.0, 3.45]), 'SpecificHeat': np.array([4178.0, 3391.0, 1313.0, 2274.0, 3630.0]),
            'Conductivity': np.array([0.6, 0.37, 0.32, 0.31, 0.51]), 'Perfusion': np.array([0.0, 106.0, 10.0, 30.0, 559.0]),
            'Absorption': np.array([0.0, 0.85, 0.16, 0.15, 0.85]), 'InitTemperature': np.full(5, 37.0)}


def chained(rep, total, pause, off, P, mm, ml, dx, nOn, nStepsOn, dt, duty, mpm, stable):
    """The reference loop (nCurrent = 0, no previous data) over R.BHTE; returns the six results and the summed kernel ms."""
    cool = P * 0
    kms = 0.0
    kw = dict(dt=dt, DutyCycle=duty, MonitoringPointsMap=mpm, stableTemp=stable)
    FT = FD = TP = Tmax = None
    for n in range(total):
        T0, D0 = (FT, FD) if n > 0 else (None, None)
        Ton, Don, _, _, Pon = R.BHTE(P, mm, ml, dx, nOn, nStepsOn, -1, initT0=T0, initDose=D0, **kw); kms += R.last_kernel_ms
        Tmax = Ton if n == 0 else np.maximum(Tmax, Ton)
        if off > 0:
            FT, FD, _, _, Poff = R.BHTE(cool, mm, ml, dx, off, 0, -1, initT0=Ton, initDose=Don, **kw); kms += R.last_kernel_ms
            TP = np.hstack((Pon, Poff)) if n == 0 else np.hstack((TP, Pon, Poff))
        else:
            FT, FD = Ton, Don
            TP = Pon if n == 0 else np.hstack((TP, Pon))
        if (n + 1) % rep == 0 and pause > 0:
            FT, FD, _, _, Pp = R.BHTE(cool, mm, ml, dx, pause, 0, -1, initT0=FT, initDose=FD, **kw); kms += R.last_kernel_ms
            TP = np.hstack((TP, Pp))
    return (Tmax, Don, FT, FD, TP, total), kms


def bytes_protocol(n, nPoints, nSteps):
    # up: ids (1 B) + pressure (4 B); T and dose start on the device (initial temperature by material, zero dose)
    # down: T, dose, Tmax, dose at the last ON end (4 B each) + the point samples
    return {'h2d': n * 5, 'd2h': n * 16 + nPoints * nSteps * 4}


def bytes_chained(n, nPoints, calls):
    h2d = d2h = 0
    for i, (kind, _, _, steps) in enumerate(calls):
        h2d += n * 5 + (n * 8 if i > 0 else 0)          # ids + pressure (zeros in an OFF call) + T and dose after the first call
        d2h += n * 12 + nPoints * steps * 4             # T, dose, heat source + the point samples
    return {'h2d': h2d, 'd2h': d2h}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, nargs=3, default=[280, 276, 272])
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not R._engine.list_devices():
        raise SystemExit('no HIP device visible: this benchmark measures the GPU only')
    N = tuple(a.grid)
    dt, dx, duty = 0.01, 5e-4, 0.3
    nOn, nStepsOn, off, rep, groups, pause = 100, 100, 400, 10, 3, 2000
    total = rep * groups
    rng = np.random.default_rng(2026)
    mm = rng.integers(0, 5, N).astype(np.uint8)
    x, y, z = np.meshgrid(*[np.arange(k, dtype=np.float32) - k / 2 for k in N], indexing='ij', sparse=True)
    P = (1.5e6 * np.exp(-(x ** 2 + y ** 2 + (z / 3) ** 2) / 60.0)).astype(np.float32)
    mpm = np.zeros(N, np.uint32)
    for i, (u, v, w) in enumerate([(0.5, 0.5, 0.5), (0.3, 0.5, 0.6), (0.5, 0.7, 0.4), (0.6, 0.4, 0.5)]):
        mpm[int(u * N[0]), int(v * N[1]), int(w * N[2])] = i + 1
    ml = materials()
    # warm-up: code objects and the device context, on a small grid
    wm = np.zeros((24, 24, 24), np.uint32); wm[12, 12, 12] = 1
    R.RunBHTECycles(0, 2, 2, 3, 3, 100, 'p', P[:24, :24, :24], mm[:24, :24, :24], ml, dx, 5, 3, -1, 1, dt, duty, 'HIP', wm, 37.0,
                    None, None, None, None)
    chained(1, 1, 3, 3, P[:24, :24, :24], mm[:24, :24, :24], ml, dx, 5, 3, dt, duty, wm, 37.0)

    t0 = time.perf_counter()
    prot = R.RunBHTECycles(0, rep, total, pause, off, 100, 'p', P, mm, ml, dx, nOn, nStepsOn, -1, 1, dt, duty, 'HIP', mpm, 37.0,
                           None, None, None, None)
    wall_p = time.perf_counter() - t0
    kms_p = R.last_kernel_ms
    t0 = time.perf_counter()
    ref, kms_c = chained(rep, total, pause, off, P, mm, ml, dx, nOn, nStepsOn, dt, duty, mpm, 37.0)
    wall_c = time.perf_counter() - t0

    equal = all(np.array_equal(u, v) for u, v in zip(prot[:5], ref[:5])) and prot[5] == ref[5]
    sched, caps, calls, _ = R.protocol_schedule(0, rep, total, pause, off, 100, nOn, nStepsOn)
    n = int(np.prod(N)); nPts = int(np.count_nonzero(mpm))
    line = {'bench': 'bhte_protocol', 'grid': list(N), 'voxels': n, 'dt': dt, 'steps': len(sched), 'calls_chained': len(calls),
            'protocol': {'on_s': nOn * dt, 'off_s': off * dt, 'repetitions': rep, 'groups': groups, 'pause_s': pause * dt, 'duty': duty},
            'protocol_wall_s': round(wall_p, 4), 'chained_wall_s': round(wall_c, 4), 'wall_ratio': round(wall_c / wall_p, 3),
            'protocol_kernel_ms': round(kms_p, 2), 'chained_kernel_ms': round(kms_c, 2),
            'protocol_gvoxel_steps_per_s': round(n * len(sched) / (kms_p * 1e-3) / 1e9, 1),
            'bytes_protocol': bytes_protocol(n, nPts, len(sched)), 'bytes_chained': bytes_chained(n, nPts, calls),
            'bytes_note': 'computed from the shapes: what the calls copy between host and device',
            'outputs_equal': bool(equal), 'peak_T': float(prot[0].max())}
    out = json.dumps(line)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')
    if not equal:
        raise SystemExit('outputs differ')


if __name__ == '__main__':
    main()
