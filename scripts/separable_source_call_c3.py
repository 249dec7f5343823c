"""One production-shaped drop-in call at C3 (512^3, nt from the caller's time plan, full sensor volume) in two legs: the
dense float64 PulseSource table (harness.pulse_sources) and the SeparableSource of harness.cw_pulse_sources. Each leg runs
in a fresh child process, so that ru_maxrss separates them. Per leg: input build time (all inputs, and the source table
alone), host peak RSS, table bytes, call wall, device step loop, device bytes; then the rel-L2 between the two legs'
Pressure RMS maps.

    python scripts/separable_source_call_c3.py [--timeout SECONDS_PER_LEG] [--label TEXT]
"""
import argparse
import json
import os
import resource
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rss_gb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6      # kB -> GB


def leg(kind, outdir):
    import numpy as np
    from babelbrain_amd import harness as H, PropagationModel, _engine, RayleighAndBHTE
    separable = kind == 'separable'
    table_s = []
    builder = 'cw_pulse_sources' if separable else 'pulse_sources'
    inner = getattr(H, builder)

    def timed(*a, **k):             # make_problem looks the builder up in the module: time the table alone
        t = time.time()
        r = inner(*a, **k)
        table_s.append(time.time() - t)
        return r
    setattr(H, builder, timed)
    t0 = time.time()
    a, k, info = H.make_problem('C3', stable_dt_fn=lambda ml, f, h, c: _engine.stable_dt(ml, f, True, h, c),
                                forward=RayleighAndBHTE.ForwardSimple, separable=separable)
    t1 = time.time()
    rss_inputs = rss_gb()
    pm = PropagationModel()
    t2 = time.time()
    out = pm.StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, ReturnSensorDFT=True, **k)
    t3 = time.time()
    tm = pm.last_timing
    rms = out[2]['Pressure']
    np.save(os.path.join(outdir, 'rms_%s.npy' % kind), rms)
    n = 512 ** 3
    res = dict(leg=kind, nt=info['nt'], n_sources=info['n_sources'], table_bytes=int(a[4].nbytes),
               inputs_s=t1 - t0, table_s=table_s[0], rss_after_inputs_gb=rss_inputs, call_wall_s=t3 - t2,
               step_loop_s=tm['total_ms'] / 1e3, device_gvoxel_steps_per_s=n * info['nt'] / tm['total_ms'] / 1e6,
               call_gvoxel_steps_per_s=n * info['nt'] / (t3 - t2) / 1e9, device_bytes=int(out[-1]['device_bytes']),
               rss_peak_gb=rss_gb(), rms_max=float(rms.max()), sensor_block=list(out[0]['Pressure'].shape))
    print('LEG ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=['dense', 'separable'])
    ap.add_argument('--outdir')
    ap.add_argument('--timeout', type=int, default=400)
    ap.add_argument('--label', default='')
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg, args.outdir)
    import numpy as np
    res = {}
    with tempfile.TemporaryDirectory() as d:
        for kind in ('dense', 'separable'):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', kind, '--outdir', d],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.timeout)
            lines = [x for x in p.stdout.splitlines() if x.startswith('LEG ')]
            if p.returncode != 0 or not lines:
                print(p.stdout[-4000:])
                print('leg %s failed (exit %d): stopping' % (kind, p.returncode))
                return 1
            res[kind] = json.loads(lines[-1][4:])
        a = np.load(os.path.join(d, 'rms_dense.npy')).astype(np.float64)
        b = np.load(os.path.join(d, 'rms_separable.npy')).astype(np.float64)
        rel = float(np.sqrt(np.sum((b - a) ** 2) / np.sum(a ** 2)))
    print('scripts/separable_source_call_c3.py: one production-shaped C3 call (512^3, ctx500, CT medium, ReturnSensorDFT=True, '
          'sensor series returned) per leg, each leg in a fresh process%s' % (' -- ' + args.label if args.label else ''))
    print('nt=%d, %d source voxels' % (res['dense']['nt'], res['dense']['n_sources']))
    fmt = '%-40s %16s %16s'
    print(fmt % ('', 'dense float64', 'SeparableSource'))
    rows = [('PulseSource bytes on the host', 'table_bytes', lambda v: '%.3g MB' % (v / 1e6)),
            ('source table build (s)', 'table_s', lambda v: '%.3f' % v),
            ('all inputs built (s)', 'inputs_s', lambda v: '%.2f' % v),
            ('host peak RSS after inputs (GB)', 'rss_after_inputs_gb', lambda v: '%.2f' % v),
            ('host peak RSS of the leg (GB)', 'rss_peak_gb', lambda v: '%.2f' % v),
            ('call wall (s)', 'call_wall_s', lambda v: '%.2f' % v),
            ('device step loop (s)', 'step_loop_s', lambda v: '%.2f' % v),
            ('device-only Gvoxel-steps/s', 'device_gvoxel_steps_per_s', lambda v: '%.1f' % v),
            ('whole call Gvoxel-steps/s', 'call_gvoxel_steps_per_s', lambda v: '%.1f' % v),
            ('device bytes (GB)', 'device_bytes', lambda v: '%.3f' % (v / 1e9)),
            ('Pressure RMS max', 'rms_max', lambda v: '%.6g' % v)]
    for name, key, f in rows:
        print(fmt % (name, f(res['dense'][key]), f(res['separable'][key])))
    print('Pressure RMS map, rel-L2 separable vs dense: %.3e' % rel)
    print('raw: ' + json.dumps(res))
    return 0


if __name__ == '__main__':
    sys.exit(main())
