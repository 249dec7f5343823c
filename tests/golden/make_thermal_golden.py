#!/usr/bin/env python3
"""Generates tests/golden/thermal_analysis_golden.npz + thermal_analysis_golden.json by running the reference's own statements of
ThermalModeling/CalculateTemperatureEffects.py on seeded cases (tests/thermal_oracle.py, build_case). The module cannot be imported by every Python
(an f-string near its end nests its own quotes), so the text of AnalyzeLosses (from its `def` to the next top-level `def`) and of three blocks of
CalculateTemperatureEffects (the selections :864-906, the monitoring points :996-1023, the metrics :1126-1151) is sliced from the file and executed
in place, never stored, as make_golden.block_between does. Only parameters, seeds and results are stored; no reference source.

Everything the reference prints in AnalyzeLosses is recorded, label and numbers, so the intermediates are held too.

Run:  python tests/golden/make_thermal_golden.py
"""
import hashlib
import json
import os
import sys
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import make_golden as MG                  # noqa: E402
from tests import thermal_oracle as TO    # noqa: E402

SOURCE = os.path.join(MG.REF, 'ThermalModeling', 'CalculateTemperatureEffects.py')
SHAPE = (24, 22, 40)
# name: (build_case parameters, call parameters)
CASES = {
    'plain': (dict(seed=1), {}),
    'plain_ct': (dict(seed=2, ct=True, n_ct=20), {}),
    'segmented': (dict(seed=3, segmented=True), {}),
    'segmented_ct': (dict(seed=4, ct=True, segmented=True, n_ct=20), {}),
    'homogeneous': (dict(seed=5, homogeneous=True), {}),
    'benchmark1': (dict(seed=6, benchmark=dict(TestType=1, nMaterials=3)), {}),
    'benchmark2': (dict(seed=7, benchmark=dict(TestType=2, nMaterials=4)), {}),
    'benchmark3': (dict(seed=8, benchmark=dict(TestType=3, nMaterials=6)), {}),
    'dome': (dict(seed=9), dict(TxSystem='DomeTx')),
    'fixed_power': (dict(seed=10), dict(FixedAcousticPower=2.5)),
    'switch': (dict(seed=11, split=True), {}),
    'target_at_max': (dict(seed=12, target_at_max=True), {}),
}
CALL = dict(Isppa=5.0, TxSystem='CTX_500', FixedAcousticPower=0.0, Frequency=500e3, DutyCycle=0.3)
SWITCH_LABEL = 'Warning: RatioLossesLoc'


def lines_between(lines, start_marker, end_marker):
    a = next(i for i, l in enumerate(lines) if start_marker in l)
    b = next(i for i in range(a, len(lines)) if end_marker in lines[i])
    return textwrap.dedent('\n'.join(lines[a:b + 1]))


def reference_blocks():
    lines = open(SOURCE).read().splitlines()
    a = next(i for i, l in enumerate(lines) if l.startswith('def AnalyzeLosses('))
    b = next(i for i in range(a + 1, len(lines)) if lines[i].startswith('def '))
    return dict(analyze='\n'.join(lines[a:b]),
                select=lines_between(lines, 'bNormalOperation=True', 'SelSkin=MaterialMap==1'),
                monitor=lines_between(lines, 'ResTempSkin=ResTemp * SelSkin.astype(np.float32)', 'MonitoringPointsMap[cx,cy,cz]=4'),
                metrics=lines_between(lines, 'TI=ResTemp[SelBrain].max()', 'Ispta =DutyCycle*Isppa'))


def numbers(args):
    return [float(a) for a in args if not isinstance(a, str)]


def scalar(v):
    return dict(value=float(v), dtype=np.asarray(v).dtype.name)


def main():
    blocks = reference_blocks()
    out, meta = {}, {'generated_from': 'ThermalModeling/CalculateTemperatureEffects.py: AnalyzeLosses, :864-906, :996-1023, :1126-1151',
                     'numpy': np.__version__, 'shape': list(SHAPE), 'call': CALL, 'cases': {}}
    for name, (build, delta) in CASES.items():
        call = dict(CALL, **delta)
        case = TO.build_case(SHAPE, **build)
        benchmark = build.get('benchmark')
        reports = []
        ns = dict(np=np, print=lambda *a: reports.append([a[0].split('\n')[0]] + numbers(a[1:])))
        ns.update(IdRegionBenchmark=[], MaterialMap=case['MaterialMap'], Input=case['Input'], LocIJK=case['LocIJK'], bForceHomogenousMedium=bool(build.get('homogeneous')),
                  bSegmentedBrain=bool(build.get('segmented')), BenchmarkTestFile='benchmark.h5' if benchmark else '',
                  BenchmarkInput=dict(Materials=[None] * benchmark['nMaterials'], TestType=benchmark['TestType']) if benchmark else None)
        exec(blocks['select'], ns)
        exec(blocks['analyze'], ns)
        water = case['pAmpWater'].copy()
        PressureRatio, RatioLosses = ns['AnalyzeLosses'](case['pAmp'], case['MaterialMap'], case['LocIJK'], case['Input'], case['MaterialList'], water,
                                                         call['Isppa'], case['xf'], case['yf'], case['zf'], ns['SelBrain'], ns['bForceHomogenousMedium'],
                                                         ns['bSegmentedBrain'], call['TxSystem'], ns['IdRegionBenchmark'],
                                                         FixedAcousticPower=call['FixedAcousticPower'])
        analyze_reports = list(reports)
        ns.update(ResTemp=case['ResTemp'], FinalDose=case['FinalDose'], Frequency=call['Frequency'], DutyCycle=call['DutyCycle'], Isppa=call['Isppa'],
                  SaveDict=dict(p_map=case['pAmp'] * PressureRatio, MaterialList=case['MaterialList']))          # p_map: :1115
        exec(blocks['monitor'], ns)
        exec(blocks['metrics'], ns)
        where = np.flatnonzero(ns['MonitoringPointsMap'])
        rec = dict(build=build, call=call, reports=analyze_reports, PressureRatio=scalar(PressureRatio), RatioLosses=scalar(RatioLosses),
                   water_sha1=hashlib.sha1(water.tobytes()).hexdigest(), water_zeroed=int(np.count_nonzero(water != case['pAmpWater'])),
                   BrainID=[int(v) for v in ns['BrainID']], IdRegionBenchmark=[int(v) for v in ns['IdRegionBenchmark']],
                   selected=[int(np.count_nonzero(ns[k])) for k in ('SelBrain', 'SelSkin', 'SelSkull')],
                   mSkin=[int(ns[k]) for k in ('mxSkin', 'mySkin', 'mzSkin')], mBrain=[int(ns[k]) for k in ('mxBrain', 'myBrain', 'mzBrain')],
                   mSkull=[int(ns[k]) for k in ('mxSkull', 'mySkull', 'mzSkull')], p_map_dtype=ns['SaveDict']['p_map'].dtype.name,
                   metrics={k: scalar(ns[k]) for k in TO.METRICS if np.ndim(ns[k]) == 0})
        out[name + '_monitor_index'] = where.astype(np.int64)
        out[name + '_monitor_id'] = ns['MonitoringPointsMap'].reshape(-1)[where]
        out[name + '_MaxIsppa'] = np.asarray(ns['MaxIsppa'])
        out[name + '_MaxIspta'] = np.asarray(ns['MaxIspta'])
        for k, sel in (('SelBrain', ns['SelBrain']), ('SelSkin', ns['SelSkin']), ('SelSkull', ns['SelSkull'])):
            out[name + '_' + k] = np.packbits(sel)
        meta['cases'][name] = rec
        took = any(r[0].startswith(SWITCH_LABEL) for r in analyze_reports)
        assert took == (name == 'switch'), (name, took)
        if not benchmark and not build.get('homogeneous'):
            assert (rec['mBrain'] == [int(v) for v in case['LocIJK']]) == (name == 'target_at_max'), name
        assert all(rec['selected']) or benchmark or build.get('homogeneous'), (name, rec['selected'])
        print(name, rec['PressureRatio'], rec['RatioLosses'], rec['selected'], rec['mBrain'], list(out[name + '_monitor_id']))

    np.savez_compressed(os.path.join(HERE, 'thermal_analysis_golden.npz'), **out)
    with open(os.path.join(HERE, 'thermal_analysis_golden.json'), 'w') as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
    print('wrote', len(out), 'arrays,', os.path.getsize(os.path.join(HERE, 'thermal_analysis_golden.npz')), 'bytes')


if __name__ == '__main__':
    main()
