"""Timing record of Step 2 as a device-resident study (babelbrain_amd/AcousticStudy.py) against the same flow by the separate public calls, the path
before the study: Domain.plan_domain / assemble, Engine with the host setters, sensor_dft, sensor_index, get_map, harness.phase_maps, the scaling
statements and results.data_for_sim. The head phantom of scripts/domain_timing.py at 448 x 448 x 384 gives the two domains profiles/README.md
"Domain" uses: 215 x 215 x 198 (tight) and 472 x 472 x 408 (not tight). Both paths run the tissue case and then the water case on the same live
engine, with a CT list and the air mask. Wall time under a host clock, split by stage; the step loop is the same launches in both paths and is
reported beside the rest. Also the result packing alone (bfd_pack_results: the kernel time its events give, and the bytes it must move from the
shapes). Prints one JSON line last.

    python scripts/acoustic_study_timing.py [--steps 200] [--reps 2] [--only tight|not_tight]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from babelbrain_amd import AcousticStudy as AS, Domain as DM, _engine, harness as H, results as R
from babelbrain_amd._engine import KIND_RMS
from babelbrain_amd.PropagationModel import compact_sources
from domain_timing import N_HU, phantom

FREQ = 500e3


class Clock:
    def __init__(self):
        self.ms = {}
        self._t = time.perf_counter()

    def lap(self, name):
        t = time.perf_counter()
        self.ms[name] = self.ms.get(name, 0.0) + (t - self._t) * 1e3
        self._t = t


def materials():
    t = H.MATERIALS[FREQ]
    ml = np.tile(np.array(t['Cortical'], np.float64), (N_HU + 3, 1))
    ml[0], ml[1], ml[2] = t['Water'], t['Skin'], t['Brain']
    ml[3:, 1] += 0.5 * np.arange(N_HU)
    return ml


def time_plan(plan, ml, h, steps):
    dt_ideal = _engine.stable_dt(ml, FREQ, True, h, H.ALPHA_CFL, 1.0)
    dt_water = _engine.stable_dt(ml[:1], FREQ, True, h, 1.0)
    ppp, dt = H.ppp_rule(dt_ideal, FREQ)
    _, _, sub, _ = plan.time_plan(dt, ppp, ml[0, 1])
    start = max(int((steps - H.CYCLES_TO_TRACK * ppp) / sub), 0)
    return dt, sub, start, H.dispersion_correction(dt, dt_water)


def plane_of(plan):
    return H.source_plane(H.CONFIGS['C2']['tx'], plan.N1, plan.N2, plan.SpatialStep, FREQ)


def by_calls(labels, ct, air, ml, h, kw, steps):
    c = Clock()
    plan = DM.plan_domain(labels, h, **kw)
    c.lap('plan')
    m, noct, sub_air, _ = DM.assemble(labels, plan, ct, air, len(ml))
    c.lap('assemble')
    dt, sub, start, corr = time_plan(plan, ml, h, steps)
    N1, N2, N3 = plan.shape
    zsrc, pml = int(plan.ZSourceLocation), plan.PMLThickness
    plane = plane_of(plan)
    c.lap('source plane (host, both paths)')
    e = _engine.Engine(N1, N2, N3, len(ml), h, dt, FREQ, steps, NDelta=pml, sensorSub=sub, sensorStart=start, selRMSorPeak=1, selMapsRMS=['Pressure'],
                       selMapsSensors=['Pressure'], sensorMode=1)
    out = {}
    try:
        e.set_materials(ml, 1.0)
        e.set_material_map(m, 0, 0)
        e.set_reflector(sub_air)
        smap, src = H.cw_pulse_sources(plane, FREQ, dt, steps * dt, N3, zsrc)
        e.set_sources(*compact_sources(smap, np.array([0.0]), np.array([0.0]), np.array([1.0 / (ml[0, 0] * ml[0, 1])]))[:5], src)
        e.set_sensor_map(H.sensor_maps(N1, N2, N3, zsrc, pml)[0])
        e.prepare()
        c.lap('engine inputs')
        for which in ('tissue', 'water'):
            if which == 'water':
                e.set_material_map(np.zeros(plan.shape, np.uint32), 0, 0)
                e.reset()
                e.prepare()
                c.lap('engine inputs')
            e.run(steps)
            e.sync()
            c.lap('step loop')
            F, pk = e.sensor_dft(FREQ)
            four, _, _ = H.phase_maps(F[0], pk[0], e.sensor_index(), N1, N2, N3)
            rms = e.get_map(KIND_RMS, 'Pressure')
            rms *= corr * np.sqrt(2)
            four *= float(corr)
            tissue = which == 'tissue'
            d = R.data_for_sim(plan.crop(), zsrc, rms, four, noct if tissue else np.zeros(plan.shape, np.uint32), plan.FocalSpotLocation, ml, plan.XDim,
                               plan.YDim, plan.ZDim, h, 4e-2, MaterialMapCT=m if tissue else None, AirMask=sub_air if tissue else None)
            out[which] = {k: np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v for k, v in d.items()}
            c.lap('results')
    finally:
        e.close()
    c.lap('close')
    return out, c.ms, plan


def by_study(labels, ct, air, ml, h, kw, steps):
    c = Clock()
    out = {}
    with AS.AcousticStudy(labels, ct, air) as st:
        c.lap('upload')
        plan = st.plan(h, **kw)
        c.lap('plan')
        st.assemble(plan, len(ml))
        c.lap('assemble')
        dt, sub, start, corr = time_plan(plan, ml, h, steps)
        plane = plane_of(plan)
        c.lap('source plane (host, both paths)')
        st.engine(ml, FREQ, h, dt, steps, 1.0, sensorSub=sub, sensorStart=start)
        st.set_source_plane(plane, steps * dt)
        st.sim.prepare()
        c.lap('engine inputs')
        for which in ('tissue', 'water'):
            if which == 'water':
                st.assemble(plan, len(ml), water_only=True)
                st.attach()
                st.reset()
                st.sim.prepare()
                c.lap('engine inputs')
            st.run()
            c.lap('step loop')
            st.pack(corr, which)
            out[which] = st.data_for_sim(ml, 4e-2, which)
            c.lap('results')
        traffic = st.traffic()
    c.lap('close')
    return out, c.ms, traffic


def pack_alone(labels, ct, air, ml, h, kw, steps, reps):
    """bfd_pack_results on a live engine: kernel time from its events, bytes from the shapes"""
    with AS.AcousticStudy(labels, ct, air) as st:
        plan = st.plan(h, **kw)
        st.assemble(plan, len(ml))
        dt, sub, start, corr = time_plan(plan, ml, h, steps)
        st.engine(ml, FREQ, h, dt, steps, 1.0, sensorSub=sub, sensorStart=start)
        st.set_source_plane(plane_of(plan), steps * dt)
        st.run()
        crop = plan.crop()
        ms, wall = [], []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            r = st.sim.pack_results(crop.lo, crop.hi, int(plan.ZSourceLocation), correction=corr)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(r['kernel_ms'])
        kept = r['p_amp'].size
        t0 = time.perf_counter()
        st.sim.get_map(KIND_RMS, 'Pressure')
        get_map_ms = (time.perf_counter() - t0) * 1e3
        # per kept voxel: 4 B of the accumulator, 16 B of the DFT sums and 4 B of the peaks read, 4 + 8 + 4 B written
        nbytes = kept * (24 + 16)
        k = float(np.median(ms[1:]))
        return {'kept_voxels': kept, 'kernel_ms': k, 'call_ms': float(np.median(wall[1:])), 'bytes': nbytes, 'gb_per_s': nbytes / k / 1e6,
                'get_map_rms_call_ms': get_map_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--only', choices=['tight', 'not_tight'])
    a = ap.parse_args()
    devs = DM.InitDomain()
    labels, ct, air = phantom((448, 448, 384))
    h = 1102.515 / 500e3 / 6
    ml = materials()
    res = {'device': devs[DM._device][1], 'steps': a.steps, 'reps': a.reps, 'paths': {}}
    for tight in (True, False):
        name = 'tight' if tight else 'not_tight'
        if a.only and a.only != name:
            continue
        kw = dict(FocalLength=63.2e-3, Aperture=64e-3, bTightNarrowBeamDomain=tight, zLengthBeyonFocalPointWhenNarrow=8e-3)
        rows = {'calls': [], 'study': []}
        equal = None
        for rep in range(a.reps):
            ref, ms_c, plan = by_calls(labels, ct, air, ml, h, kw, a.steps)
            got, ms_s, traffic = by_study(labels, ct, air, ml, h, kw, a.steps)
            rows['calls'].append(ms_c)
            rows['study'].append(ms_s)
            equal = all(np.array_equal(got[w][k], ref[w][k]) for w in ref for k in ref[w])
            for w in ref:
                for k in ref[w]:
                    if not np.array_equal(got[w][k], ref[w][k]):
                        x, y = np.asarray(got[w][k]).reshape(-1), np.asarray(ref[w][k]).reshape(-1)
                        bad = np.flatnonzero(x != y)
                        print('  %s %s: %d of %d differ; first got %r, expected %r; largest |expected| among them %.3e' % (
                            w, k, bad.size, x.size, x[bad[0]], y[bad[0]], float(np.abs(y[bad]).max())), flush=True)
            print('%s rep %d: domain %r; calls %.0f ms %s; study %.0f ms %s; equal %s' % (
                name, rep, plan.shape, sum(ms_c.values()), {k: round(v) for k, v in ms_c.items()}, sum(ms_s.values()), {k: round(v) for k, v in ms_s.items()},
                equal), flush=True)
            del ref, got
        res['paths'][name] = {'domain': plan.shape, 'calls_ms': rows['calls'], 'study_ms': rows['study'], 'equal': bool(equal), 'traffic': traffic,
                              'pack': pack_alone(labels, ct, air, ml, h, kw, a.steps, 3)}
        print('%s: pack alone %r' % (name, res['paths'][name]['pack']), flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
