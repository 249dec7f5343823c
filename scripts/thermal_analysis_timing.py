"""Timing record of the Step-3 exposure analysis on the device (bfd_loss_survey3d and bfd_class_extrema3d behind babelbrain_amd.ThermalAnalysis) on
448 x 448 x 384 with a uint32 map of 1030 materials and a skull-like shell (harness.skull_shell_map), median of --reps after one warm-up:
  - kernelMs of each entry (HIP events around its kernels) and the wall time of the call (allocation, copies, kernels);
  - the bytes each must move, every volume and the map once (survey: p, pw and the map, 12 B per voxel, and 4 B per cleared voxel where the water
    field is written back; extrema: three volumes and the map, 16 B per voxel), and the rate that gives;
  - as the yardstick of the same session, one of the project's own one-pass kernels: bfd_pseudo_ct_convert3d (float32 in, float64 out: three masks
    3 B, the output 8 B per voxel, 4 B per bone voxel);
  - the time of the literal numpy flow on the same host (tests/thermal_oracle.py: AnalyzeLosses, the monitoring points, the metrics), once, and of
    the drop-ins around the two entries (ThermalAnalysis.AnalyzeLosses, hottest_points, exposure_metrics), with the results of the two compared.
Prints one JSON line last.

    python scripts/thermal_analysis_timing.py [--reps 5] [--shape 448 448 384] [--no-host]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from babelbrain_amd import PseudoCT as PC, ThermalAnalysis as TA, harness as H
from tests import thermal_oracle as TO


def median_of(fn, reps, module):
    fn()
    wall, kms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        kms.append(module.last_kernel_ms)
    return r, float(np.median(kms)), float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shape', type=int, nargs=3, default=[448, 448, 384])
    ap.add_argument('--no-host', action='store_true', help='without the numpy flow (for a kernel trace)')
    a = ap.parse_args()
    shape = tuple(a.shape)
    n = int(np.prod(shape))
    devs = TA.InitThermalAnalysis()
    PC.InitPseudoCT()
    rng = np.random.default_rng(0)
    h = 0.4e-3
    nMat = 1030
    M = H.skull_shell_map(shape[0], shape[1], shape[2], h, 12, n_ct_bins=nMat - 3)
    M[(M == 0) & np.roll(M >= 3, -3, axis=2)] = 1               # three voxels of skin above the shell
    assert M.dtype == np.uint32 and M.max() < nMat
    t = TA.region_tables(nMat, True, False)
    ml = dict(SoS=np.concatenate(([1500.0], rng.uniform(1450.0, 3100.0, nMat - 1))), Density=np.concatenate(([1000.0], rng.uniform(950.0, 2200.0, nMat - 1))))
    x = np.arange(shape[0]) * h
    grids = dict(xf=x, yf=np.arange(shape[1]) * h, zf=np.arange(shape[2]) * h)
    Input = dict(x_vec=grids['xf'], y_vec=grids['yf'], z_vec=grids['zf'], MaterialMapCT=True)
    pAmp = (rng.random(shape, np.float32) * np.float32(3e5)).astype(np.float32)
    pAmpWater = (rng.random(shape, np.float32) * np.float32(6e5)).astype(np.float32)
    ResTemp = (np.float32(37) + rng.random(shape, np.float32) * np.float32(6)).astype(np.float32)
    FinalDose = rng.random(shape, np.float32)
    LocIJK = np.array([shape[0] // 2, shape[1] // 2, int(shape[2] * 0.6)])
    cleared = int(np.count_nonzero((t['classOf'][M] >> TA.BIT_SELREGION) & 1))
    brain = int(np.count_nonzero(t['classOf'][M] & 1))
    print('device: %s; %d x %d x %d = %d voxels; %d materials; brain %d, cleared %d voxels; reps %d'
          % ((devs[TA._device][1],) + shape + (n, nMat, brain, cleared, a.reps)), flush=True)
    res = {'device': devs[TA._device][1], 'shape': shape, 'materials': nMat, 'brain': brain, 'cleared': cleared}
    dx2 = (x[1] - x[0]) ** 2

    def rate(nbytes, ms):
        return nbytes / (ms * 1e-3) / 1e12

    for name, out in (('survey', None), ('survey, water written back', 'out')):
        buf = None if out is None else np.empty((1,) + shape, np.float32)
        _, k, w = median_of(lambda: TA.loss_survey(pAmp, pAmpWater, M, t['classOf'], ml['Density'], ml['SoS'], 1000.0, 1500.0, dx2, waterOut=buf), a.reps, TA)
        nbytes = 12 * n + (4 * cleared if out else 0)
        print('%-32s kernels %7.3f ms, %.3f GB: %.2f TB/s; the call %7.1f ms' % (name, k, nbytes / 1e9, rate(nbytes, k), w), flush=True)
        res[name] = dict(kernel_ms=k, call_ms=w, bytes=nbytes, TBps=rate(nbytes, k))
    vols = [ResTemp, FinalDose, pAmp]
    _, k, w = median_of(lambda: TA.tissue_extrema(vols, M, t['classOf']), a.reps, TA)
    print('%-32s kernels %7.3f ms, %.3f GB: %.2f TB/s; the call %7.1f ms' % ('extrema, three volumes', k, 16 * n / 1e9, rate(16 * n, k), w), flush=True)
    res['extrema'] = dict(kernel_ms=k, call_ms=w, bytes=16 * n, TBps=rate(16 * n, k))
    _, k, w = median_of(lambda: TA.tissue_extrema(vols[:1], M, t['classOf']), a.reps, TA)
    print('%-32s kernels %7.3f ms, %.3f GB: %.2f TB/s; the call %7.1f ms' % ('extrema, one volume', k, 8 * n / 1e9, rate(8 * n, k), w), flush=True)
    res['extrema1'] = dict(kernel_ms=k, call_ms=w, bytes=8 * n, TBps=rate(8 * n, k))

    bone = M >= 3
    nb = 11 * n + 4 * int(np.count_nonzero(bone))
    _, k, w = median_of(lambda: PC.hounsfield(pAmp, 3e5, None, bone, M > 0, M == 1, PC.PETRA_SLOPE, PC.PETRA_OFFSET), a.reps, PC)
    print('%-32s kernels %7.3f ms, %.3f GB: %.2f TB/s; the call %7.1f ms' % ('yardstick: pseudo-CT conversion', k, nb / 1e9, rate(nb, k), w), flush=True)
    res['yardstick_convert'] = dict(kernel_ms=k, call_ms=w, bytes=nb, TBps=rate(nb, k))

    def device_flow():
        water = pAmpWater.copy()
        ratio, losses = TA.AnalyzeLosses(pAmp, M, LocIJK, Input, ml, water, 5.0, grids['xf'], grids['yf'], grids['zf'], t['BrainID'], False, False, 'CTX_500')
        pts = TA.hottest_points(ResTemp, M, t['classOf'])
        met = TA.exposure_metrics(ResTemp, FinalDose, (pAmp, ratio), M, t['classOf'], ml, t['BrainID'], 5e5, 0.3, 5.0)
        return ratio, losses, pts, met, water

    dev, _, w = median_of(device_flow, max(1, a.reps // 2), TA)
    print('the drop-ins (AnalyzeLosses, hottest_points, exposure_metrics; with the copy of the water field): %.1f ms' % w, flush=True)
    res['device_flow_ms'] = w
    if not a.no_host:
        t0 = time.perf_counter()
        SelBrain, SelSkin, SelSkull, BrainID, _ = TO.selections(M, True, False)
        t1 = time.perf_counter()
        water = pAmpWater.copy()
        ratio, losses = TO.AnalyzeLosses(pAmp, M, LocIJK, Input, ml, water, 5.0, grids['xf'], grids['yf'], grids['zf'], SelBrain, False, False, 'CTX_500')
        t2 = time.perf_counter()
        _, mSkin, mBrain, mSkull = TO.monitoring_points_map(ResTemp, SelSkin, SelBrain, SelSkull, LocIJK)
        met = TO.exposure_metrics(ResTemp, FinalDose, pAmp * ratio, SelBrain, SelSkin, SelSkull, ml, BrainID, 5e5, 0.3, 5.0)
        t3 = time.perf_counter()
        print('the numpy flow on this host: selections %.2f s, AnalyzeLosses %.2f s, the extrema lines %.2f s (with pAmp * PressureRatio)'
              % (t1 - t0, t2 - t1, t3 - t2), flush=True)
        same = (np.array_equal(water, dev[4]) and float(ratio) == float(dev[0]) and all(np.array_equal(p, q) for p, q in zip((mSkin, mBrain, mSkull), dev[2]))
                and all(np.array_equal(met[k], dev[3][k]) for k in TO.METRICS))
        rel = abs(float(losses) - float(dev[1])) / float(losses)
        print('the two flows: water field, PressureRatio, hottest points and metrics equal: %s; RatioLosses differs by %.2e relative (bound %.2e)'
              % (same, rel, 4 * (shape[0] * shape[1] - 1) * 2.0 ** -53), flush=True)
        print('AnalyzeLosses and the extrema lines: %.2f s in numpy against %.1f ms: %.0f x' % (t3 - t1, w, (t3 - t1) * 1e3 / w), flush=True)
        res.update(host_selections_s=t1 - t0, host_analyze_losses_s=t2 - t1, host_extrema_s=t3 - t2, flows_equal=bool(same), ratio_losses_rel=rel)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
