"""python scripts/resample_timing.py [scipy]   CT-size measurement: 512 x 512 x 400 int16 -> 448 x 448 x 384 under a small rotation, orders 3 and 0. Device events through the ABI
(prefilter and interpolation separately), wall time of the whole call around it (the call ends in a device-to-host copy)."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from babelbrain_amd import Resample as R

def case():
    ishape, oshape = (512, 512, 400), (448, 448, 384)
    rng = np.random.default_rng(0)
    ct = (rng.standard_normal(ishape, dtype=np.float32) * 400.0).astype(np.int16)
    th = 0.05
    c, s = np.cos(th), np.sin(th)
    M = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.diag([512 / 448.0, 512 / 448.0, 400 / 384.0])
    ci, co = (np.array(ishape) - 1) / 2.0, (np.array(oshape) - 1) / 2.0
    return ct, M, ci - M @ co, oshape

if __name__ == '__main__':
    ct, M, off, oshape = case()
    if len(sys.argv) > 1 and sys.argv[1] == 'scipy':            # the CPU comparison
        import scipy.ndimage as ndi
        for order in (3, 0):
            t0 = time.perf_counter(); ndi.affine_transform(ct, M, off, oshape, order=order, cval=float(ct.min())); t1 = time.perf_counter()
            print(json.dumps({'scipy_order': order, 'wall_s': t1 - t0}), flush=True)
        sys.exit(0)
    R.InitResample()
    n_in, n_out = ct.size, int(np.prod(oshape))
    cval = float(ct.min())
    rows = []

    def call(order, gathered, rep):
        t0 = time.perf_counter()
        out = R.affine_transform(ct, M, off, oshape, order=order, cval=cval, _gathered=gathered)
        wall = time.perf_counter() - t0
        rows.append({'order': order, 'interpolation': 'gathered' if gathered or order != 3 else 'staged', 'rep': rep, 'prefilter_ms': R.last_prefilter_ms,
                     'interpolation_ms': R.last_interpolation_ms, 'wall_ms': wall * 1e3})
        print(json.dumps(rows[-1]), flush=True)
        return out
    # order 3: the LDS-staged and the gathered interpolation alternating in one process; rep 0 of each is the warm-up
    for rep in range(6):
        a = call(3, False, rep)
        b = call(3, True, rep)
        if rep == 0:
            print(json.dumps({'staged_equals_gathered': bool(np.array_equal(a, b))}), flush=True)
    for rep in range(4):
        call(0, False, rep)
    for name in ('staged', 'gathered'):
        t = sorted(r['interpolation_ms'] for r in rows if r['order'] == 3 and r['interpolation'] == name and r['rep'] > 0)
        print(json.dumps({'order': 3, 'interpolation': name, 'interpolation_ms_min_median_max': [t[0], t[len(t) // 2], t[-1]]}), flush=True)
    # the prefilter's algorithmic bytes: the int16 read and the float64 write of the conversion, one float64 read and write per axis
    alg = n_in * (2 + 8 + 3 * 16)
    best = min(r['prefilter_ms'] for r in rows if r['order'] == 3 and r['rep'] > 0)
    print(json.dumps({'prefilter_algorithmic_bytes': alg, 'best_prefilter_ms': best, 'fraction_of_8TBps': alg / (best * 1e-3) / 8e12}), flush=True)
    for rep in range(2):                                        # the prefilter alone, through spline_filter (840 MB come back)
        t0 = time.perf_counter(); R.spline_filter(ct, 3, 'mirror'); wall = time.perf_counter() - t0
        print(json.dumps({'spline_filter_rep': rep, 'kernel_ms': R.last_kernel_ms, 'wall_ms': wall * 1e3}), flush=True)
