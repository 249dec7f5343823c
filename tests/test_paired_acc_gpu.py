"""Paired Pressure accumulation (bfd_api.hip, "paired accumulation"): in the all-fluid runs the accumulating steps go in pairs -- the first
leaves the RMS / peak maps alone, the stress half-step of the second adds the Pressure of both -- and whatever reads or clears the maps
settles an open pair first. Every result must equal, bit for bit, what accumulating in every step gives (BFD_PAIR_ACC=0, the path of
the parent commit), in a fresh engine each: RMS, peak and last maps, the sensor series and every state array.

Quiet runs switch pairing off and a default call has them on, so the engines are built as bench.py builds them (rmsFirstStep >= 1), and
every case asserts through Engine.paired_launches() that the pairing stress flavour really ran on the default leg (and never on the other)."""
import numpy as np
import pytest

from babelbrain_amd import _engine, harness as H, slab
from babelbrain_amd._engine import KIND_RMS, KIND_PEAK, KIND_LAST, FIELD_NAMES
from tests.util import oracle_dt

pytestmark = pytest.mark.gpu

# three tiles in x (64 cells each), five in y (8 rows), and z-runs of at most 32 planes: at least three runs deep, ragged in x and z
N = (136, 40, 100)
# maps read after an odd and after an even number of accumulating steps, more steps and a second read, a reset while a pair is open
PLAN = (('run', 39), ('maps',), ('run', 26), ('maps',), ('run', 13), ('reset',), ('run', 41), ('maps',), ('run', 1), ('maps',))
STEPS = 160        # a few periods of the source: the pulse table covers whole periods only


def _problem(config, steps, reflector=False, stress_source=False, maps=('Pressure',), sel=1):
    a, k, info = H.make_problem(config, N=N, steps=steps, stable_dt_fn=oracle_dt, full_sensors=False)
    k['SelMapsRMSPeakList'] = list(maps)
    k['SelMapsSensorsList'] = ['Pressure', 'Vz']
    k['SelRMSorPeak'] = sel
    if reflector:
        refl = np.zeros(a[0].shape, np.uint32)
        refl[60:70, 14:22, 40:46] = 1          # across a tile border in x and y, inside one z-run
        refl[20:23, 30:33, 62:66] = 1          # across a z-run border of every run length
        k['ReflectorMask'] = refl
    if stress_source:
        k.update(TypeSource=2, Ox=np.array([1.0]), Oy=np.array([1.0]), Oz=np.array([1.0]))
    return a, k


def _outputs(eng, sel, maps):
    out = {}
    for n in maps:
        if sel & 1:
            out['rms_' + n] = eng.get_map(KIND_RMS, n)
        if sel & 2:
            out['peak_' + n] = eng.get_map(KIND_PEAK, n)
        out['last_' + n] = eng.get_map(KIND_LAST, n)
    return out


def _leg(a, k, plan, rms_first_step, sel, maps):
    s, info = slab.create_hip_slab(a, k, 0, 1, 0, rmsFirstStep=rms_first_step)
    eng = s.eng
    try:
        got = []
        for op in plan:
            if op[0] == 'run':
                eng.run(op[1])
            elif op[0] == 'reset':
                eng.reset()
            elif op[0] == 'set':        # inputs set again in the middle of a run: the setters settle an open pair first
                eng.set_materials(np.ascontiguousarray(a[1], np.float64).reshape(-1, 5), k.get('QCorrection', 1.0))
                eng.set_sensor_map(np.ascontiguousarray(a[7]))
            elif op[0] == 'split':      # one step by its half-steps, the maps read and a setter called between them (the values read there are not compared:
                eng.half_step_stress()  # the second step of a pair has them one step ahead of the unpaired path; nothing may be added twice)
                if sel & 1:
                    eng.get_map(KIND_RMS, 'Pressure')
                if sel & 2:
                    eng.get_map(KIND_PEAK, 'Pressure')
                eng.set_sensor_map(np.ascontiguousarray(a[7]))
                eng.half_step_velocity()
            else:
                got.append(_outputs(eng, sel, maps))
        eng.sync()
        final = _outputs(eng, sel, maps)
        final['sensors'] = eng.sensors()
        for f in FIELD_NAMES:
            final['field_' + f] = eng.get_field(f)
        got.append(final)
        return got, eng.paired_launches(), eng.tile_counts(), eng.algorithmic_bytes(True)
    finally:
        s.close()


def _both(monkeypatch, a, k, plan, rms_first_step, sel, maps=('Pressure',), maps_filled=True):
    monkeypatch.setenv('BFD_PAIR_ACC', '0')
    ref, nref, _, bytes_ref = _leg(a, k, plan, rms_first_step, sel, maps)
    monkeypatch.delenv('BFD_PAIR_ACC')
    out, nout, tiles, bytes_out = _leg(a, k, plan, rms_first_step, sel, maps)
    assert nref == 0
    assert len(out) == len(ref)
    for q, (o, r) in enumerate(zip(out, ref)):
        assert set(o) == set(r)
        for name in r:
            assert o[name].shape == r[name].shape and np.array_equal(o[name], r[name]), (q, name)
    # the run did something: the wave is there and the maps are not empty
    assert np.abs(ref[-1]['field_Szz']).max() > 0
    if maps_filled:
        assert max(np.abs(v).max() for n, v in ref[0].items() if n[:4] in ('rms_', 'peak')) > 0
    return nout, tiles, bytes_ref, bytes_out


@pytest.mark.parametrize('config,reflector,sel,rms_first_step,maps', [
    ('C1', False, 1, 1, ('Pressure',)),
    ('C1', False, 3, 2, ('Pressure',)),
    ('C3', True, 1, 1, ('Pressure',)),
    ('C3', True, 2, 4, ('Pressure',)),
    ('C3', True, 3, 7, ('Pressure', 'Vz')),
])
def test_fluid_media_equal_unpaired_accumulation(monkeypatch, config, reflector, sel, rms_first_step, maps):
    """water and the multi-material CT fluid with reflector voxels; RMS, peak, both; even and odd first accumulating step"""
    a, k = _problem(config, STEPS, reflector=reflector, maps=maps, sel=sel)
    paired, tiles, bytes_ref, bytes_out = _both(monkeypatch, a, k, PLAN, rms_first_step, sel, maps)
    assert paired > 0
    # the byte tables follow the kernels: the velocity kernel no longer moves the sum, the stress kernel half of it per launch
    assert bytes_out['velocity_fluid'] < bytes_ref['velocity_fluid'] and bytes_out['stress_fluid'] > bytes_ref['stress_fluid']
    moved = bytes_ref['velocity_fluid'] - bytes_out['velocity_fluid']
    assert bytes_out['stress_fluid'] - bytes_ref['stress_fluid'] == pytest.approx(moved / 2)


@pytest.mark.parametrize('sel,rms_first_step', [(3, 1), (1, 2)])
def test_solid_runs_beside_fluid_runs(monkeypatch, sel, rms_first_step):
    """the skull medium: the fluid runs pair, the solid runs accumulate in every step in velocity_solid"""
    a, k = _problem('C2', STEPS, sel=sel)
    paired, tiles, _, _ = _both(monkeypatch, a, k, PLAN, rms_first_step, sel)
    assert tiles['solid'] > 0 and tiles['lossless_fluid'] + tiles['lossy_fluid'] > 0
    assert paired > 0


@pytest.mark.parametrize('config,sel', [('C3', 3), ('C2', 2)])
def test_setters_and_reads_between_steps_and_half_steps(monkeypatch, config, sel):
    """setters with a pair open (after an odd number of accumulating steps) and with none; both steps of a pair taken by their half-steps with
    a map read and a setter between them; peak-only accumulation beside solid runs"""
    a, k = _problem(config, STEPS, reflector=config == 'C3', sel=sel)
    plan = (('run', 21), ('set',), ('run', 8), ('set',), ('run', 4), ('split',), ('split',), ('split',), ('run', 5), ('maps',), ('run', 2), ('maps',))
    paired, _, _, _ = _both(monkeypatch, a, k, plan, 1, sel)
    assert paired > 0


def test_stress_source_keeps_the_unpaired_path(monkeypatch):
    """a stress-type source changes Szz between the two kernels of a step: no pairing, same results"""
    a, k = _problem('C3', STEPS, reflector=True, stress_source=True, sel=3)
    paired, _, bytes_ref, bytes_out = _both(monkeypatch, a, k, PLAN, 1, 3)
    assert paired == 0 and bytes_out == bytes_ref


def test_quiet_runs_keep_the_unpaired_path(monkeypatch):
    """rmsFirstStep = 0 (a production call: the maps start with the sensor window, beyond this plan): the quiet flavours accumulate themselves"""
    a, k = _problem('C1', STEPS, sel=1)
    paired, _, _, _ = _both(monkeypatch, a, k, PLAN, 0, 1, maps_filled=False)
    assert paired == 0


def test_field_fills_the_domain(monkeypatch):
    """an odd number of steps, long enough for the wave to cross the whole grid and die in the absorbing layer on every side"""
    a, k = _problem('C3', 901, reflector=True, sel=3)
    paired, _, _, _ = _both(monkeypatch, a, k, (('run', 901),), 1, 3)
    assert paired == 450


def test_two_slabs_of_one_volume_equal_one_engine(monkeypatch):
    """the Z-slab split inside the library, built the way bench.py's group_run builds it, against one unpaired engine"""
    from babelbrain_amd.PropagationModel import compact_sources
    steps = 241
    a, k, info = H.make_problem('C3', N=N, steps=steps, stable_dt_fn=oracle_dt, zslab=(0, N[2]), full_sensors=False)
    MaterialMap, ml, f, SourceMap, Pulse, h, T, SensorMap = a
    lin, row, wx, wy, wz = compact_sources(np.asarray(SourceMap), k['Ox'], k['Oy'], k['Oz'])

    def build(devices):
        g = _engine.Group(devices, *N, len(ml), h, k['DT'], f, steps, sensorSub=k['SensorSubSampling'], sensorStart=k['SensorStart'],
                          selRMSorPeak=3, selMapsRMS=['Pressure'], selMapsSensors=['Pressure'], rmsFirstStep=1)
        g.set_materials(ml, k.get('QCorrection', 1.0))
        g.set_material_map(MaterialMap)
        g.set_sources(lin, row, wx, wy, wz, Pulse)
        g.set_sensor_map(SensorMap)
        g.prepare()
        return g

    def leg(devices):
        g = build(devices)
        try:
            g.run(120)
            g.sync()
            first = g.get_map(KIND_RMS, 'Pressure')
            g.run(121)
            g.sync()
            res = (first, g.get_map(KIND_RMS, 'Pressure'), g.get_map(KIND_PEAK, 'Pressure'), g.get_map(KIND_LAST, 'Pressure'), g.sensors())
            return res, [g.slab(r)[3].paired_launches() for r in range(g.size)]
        finally:
            g.close()

    monkeypatch.setenv('BFD_PAIR_ACC', '0')
    ref, nref = leg([0])
    monkeypatch.delenv('BFD_PAIR_ACC')
    out, nout = leg([0, 0])
    assert nref == [0] and len(nout) == 2 and all(n > 0 for n in nout)
    for o, r in zip(out, ref):
        assert np.array_equal(o, r)
    assert ref[1].max() > 0 and ref[1][:, :, N[2] // 2:].max() > 0        # the wave reached the second slab
