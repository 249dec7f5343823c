"""The Step-3 flow at the size of a treatment plan, once per process: `--path calls` runs it with the separate public calls
(tests/thermal_study_flow.flow_by_calls, the path of the commits before the thermal study), `--path study` with
babelbrain_amd.ThermalStudy.thermal_exposure fetching the four volumes the reference saves. One field, a CT-derived list of 1030 rows, the time
plan of a 40 s sonication at dt = 0.01 (the first bio-heat call, then one ON and one OFF period of the protocol). Prints one JSON line: kernel
milliseconds, the wall time of the flow alone, the study's traffic counters and the device memory it held. The case is built once and kept under
--cache, so that a series of runs measures the same inputs; profiles/README.md, "Thermal study", holds the numbers.

    for path in calls study; do for run in 1 2 3; do timeout 600 python scripts/thermal_study_flow.py --path $path --cache /tmp/thermal_case; done; done"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import thermal_study_flow as F  # noqa: E402

ARRAYS = ('pAmp', 'pAmpWater', 'MaterialMap')


def case_of(shape, cache):
    """the case of `shape`, built from its seed or read back from `cache` (the three volumes and the tables): the same inputs either way"""
    plan = dict(seed=1, ct=True, n_ct=1027, Repetitions=1, NumberGroupedSonications=1, DurationUS=40.0, DurationOff=40.0, Pause=0.0)
    held = cache and all(os.path.exists(os.path.join(cache, k + '.npy')) for k in ARRAYS) and os.path.exists(os.path.join(cache, 'tables.npz'))
    if not held:
        c = F.make_case(shape, **plan)
        if cache:
            os.makedirs(cache, exist_ok=True)
            for k in ARRAYS:
                np.save(os.path.join(cache, k + '.npy'), c[k])
            np.savez(os.path.join(cache, 'tables.npz'), **c['MaterialList'])
        c.pop('ResTemp'), c.pop('FinalDose')              # build_case's own analysis volumes: the flow computes its own
        return c
    c = F.make_case((12, 12, 24), **plan)                  # the scalars of the plan; volumes, tables and grids are replaced below
    c.pop('ResTemp'), c.pop('FinalDose')
    for k in ARRAYS:
        c[k] = np.load(os.path.join(cache, k + '.npy'))
    c['MaterialList'] = dict(np.load(os.path.join(cache, 'tables.npz')))
    N1, N2, N3 = c['MaterialMap'].shape
    h = 0.5e-3                                             # the grids and the target as tests/thermal_oracle.build_case lays them out
    xf, yf, zf = (np.arange(N1) - N1 // 2) * h, (np.arange(N2) - N2 // 2) * h, np.arange(N3) * h + 1.25e-3
    c['xf'], c['yf'], c['zf'] = xf, yf, zf
    c['LocIJK'] = np.array([N1 // 2 + 1, N2 // 2 - 1, int(N3 * 0.7)])
    c['Input'] = dict(x_vec=xf.copy(), y_vec=yf.copy(), z_vec=zf.copy(), MaterialMapCT=True, TargetLocation=c['LocIJK'])
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--path', choices=('calls', 'study'), required=True)
    ap.add_argument('--shape', type=int, nargs=3, default=(448, 448, 384))
    ap.add_argument('--cache', default='')
    a = ap.parse_args()
    c = case_of(tuple(a.shape), a.cache)
    assert c['nMat'] == 1030
    from babelbrain_amd import _engine
    from babelbrain_amd.ThermalStudy import thermal_exposure
    _engine.load_library().bfd_device_count()
    out = dict(path=a.path, shape=list(c['MaterialMap'].shape), steps=None)
    t0 = time.perf_counter()
    if a.path == 'calls':
        S = F.flow_by_calls(c)
        out.update(wall_s=time.perf_counter() - t0, kernel_ms=S['kernel_ms'])
    else:
        args, kw = F.exposure_arguments(c)
        S = thermal_exposure(*args, keep=('TempEndFUS', 'DoseEndFUS', 'FinalTemp', 'FinalDose'), **kw)
        n = int(np.prod(c['MaterialMap'].shape))
        out.update(wall_s=time.perf_counter() - t0, kernel_ms=S['kernel_ms'], bytes_up=S['traffic'][0], bytes_down=S['traffic'][1],
                   device_bytes_volumes=9 * n * 4 + 2 * n + n)
    out['steps'] = int(S['TemperaturePoints'].shape[1])
    out['TI'], out['CEMBrain'] = float(S['TI']), float(S['CEMBrain'])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
