"""Advanced Vz (bfd_lists.hip, "advanced Vz"): in the plain fluid runs outside the absorbing layer stress_fluid stores the new Vz of a run's inner
planes (kbeg+1 .. kend-3) and velocity_fluid leaves Vz alone there. Every result must equal, bit for bit, what updating Vz of every plane in
velocity_fluid gives (BFD_ADV_VZ=0, the path of the parent commit), in a fresh engine each: every state array, the RMS / peak / last maps of
Pressure and Vz and the sensor series of both.

Quiet runs keep the old path and a default call has them on, so the engines are built as bench.py builds them (rmsFirstStep >= 1). Every
qualifying case asserts on the byte tables of the default leg that the advance really ran: velocity_fluid moves less, by exactly twice what
stress_fluid moves more. The grid is 264 wide: at 136 every x-tile touches the absorbing layer and nothing would advance; here two x-tiles and
three y-tiles lie inside, with z-runs next to layer runs on every side."""
import numpy as np
import pytest

from babelbrain_amd import _engine, harness as H, slab
from babelbrain_amd._engine import KIND_RMS, KIND_PEAK, KIND_LAST, FIELD_NAMES
from tests.util import oracle_dt

pytestmark = pytest.mark.gpu

N = (264, 56, 100)
STEPS = 160        # a few periods of the source: the pulse table covers whole periods only
# a reset, maps read between steps, the inputs set again between steps; the long stretch last, so that the state arrays compared at the end hold the
# wave well inside the advancing runs (it travels about a plane in three steps from the source plane at z = 12)
PLAN = (('run', 13), ('maps',), ('reset',), ('run', 39), ('maps',), ('run', 26), ('set',), ('run', 54), ('maps',), ('run', 1), ('maps',))
INNER = (slice(64, 192), slice(16, 40))        # the x- and y-tiles outside the absorbing layer; in z the planes 16 .. 87
MAPS = ('Pressure', 'Vz')
SEL = 3


def _problem(config, reflector=False, stress_source=False):
    a, k, info = H.make_problem(config, N=N, steps=STEPS, stable_dt_fn=oracle_dt, full_sensors=False)
    k['SelMapsRMSPeakList'] = list(MAPS)
    k['SelMapsSensorsList'] = ['Pressure', 'Vz']
    k['SelRMSorPeak'] = SEL
    if reflector:
        refl = np.zeros(a[0].shape, np.uint32)
        refl[100:110, 20:28, 25:29] = 1        # inside the inner planes of a run of every length (8: planes 24 .. 31), across a tile border in y
        refl[126:130, 30:33, 30:34] = 1        # across a z-run border of every run length and a tile border in x and y
        k['ReflectorMask'] = refl
    if stress_source:
        k.update(TypeSource=2, Ox=np.array([1.0]), Oy=np.array([1.0]), Oz=np.array([1.0]))
    return a, k


def _outputs(eng):
    out = {}
    for n in MAPS:
        out['rms_' + n] = eng.get_map(KIND_RMS, n)
        out['peak_' + n] = eng.get_map(KIND_PEAK, n)
        out['last_' + n] = eng.get_map(KIND_LAST, n)
    return out


def _leg(a, k, plan, rms_first_step):
    s, info = slab.create_hip_slab(a, k, 0, 1, 0, rmsFirstStep=rms_first_step)
    eng = s.eng
    ml = np.ascontiguousarray(a[1], np.float64).reshape(-1, 5)
    refused = 0
    try:
        got = []
        for op in plan:
            if op[0] == 'run':
                eng.run(op[1])
            elif op[0] == 'reset':
                eng.reset()
            elif op[0] == 'set':        # between steps: allowed, the lists are rebuilt
                eng.set_materials(ml, k.get('QCorrection', 1.0))
                eng.set_sensor_map(np.ascontiguousarray(a[7]))
            elif op[0] == 'split':      # one step by its half-steps; the sensor map set and a map read between them (the values read there are not compared)
                eng.half_step_stress()
                eng.set_sensor_map(np.ascontiguousarray(a[7]))
                eng.get_map(KIND_RMS, 'Pressure')
                eng.get_map(KIND_LAST, 'Vz')
                eng.half_step_velocity()
            elif op[0] == 'refuse':     # set_materials between the half-steps: refused where the lists carry the bit (nothing changes), then the step finishes
                eng.half_step_stress()
                try:
                    eng.set_materials(ml, k.get('QCorrection', 1.0))
                except _engine.EngineError as e:
                    assert 'finish the time step first' in str(e)
                    refused += 1
                eng.half_step_velocity()
            else:
                got.append(_outputs(eng))
        eng.sync()
        final = _outputs(eng)
        final['sensors'] = eng.sensors()
        for f in FIELD_NAMES:
            final['field_' + f] = eng.get_field(f)
        got.append(final)
        return got, eng.algorithmic_bytes(True), eng.algorithmic_bytes(False), eng.tile_counts(), refused
    finally:
        s.close()


def _compare(out, ref):
    assert len(out) == len(ref)
    for q, (o, r) in enumerate(zip(out, ref)):
        assert set(o) == set(r)
        for name in r:
            assert o[name].shape == r[name].shape and np.array_equal(o[name], r[name]), (q, name)
    # the run did something: at the end the wave fills the first advancing runs, past both reflector boxes
    vz = np.abs(ref[-1]['field_Vz'][INNER])
    print('planes with Vz != 0 inside:', np.flatnonzero(vz.max(axis=(0, 1)))[[0, -1]])
    assert np.abs(ref[-1]['field_Szz']).max() > 0 and vz[:, :, 17:30].min(axis=(0, 1)).max() > 0 and vz[:, :, 34:40].max() > 0


def _advance_ran(bytes_ref, bytes_out):
    """velocity_fluid bytes fall by exactly twice what stress_fluid gains, and by more than nothing"""
    for bo, br in zip(bytes_out, bytes_ref):
        less = br['velocity_fluid'] - bo['velocity_fluid']
        more = bo['stress_fluid'] - br['stress_fluid']
        assert less > 0 and less == 2 * more
        assert all(bo[c] == br[c] for c in br if c not in ('velocity_fluid', 'stress_fluid'))


def _both(monkeypatch, a, k, plan, rms_first_step, qualifies=True):
    monkeypatch.setenv('BFD_ADV_VZ', '0')
    ref, acc_ref, plain_ref, _, refused_ref = _leg(a, k, plan, rms_first_step)
    monkeypatch.delenv('BFD_ADV_VZ')
    out, acc_out, plain_out, tiles, refused_out = _leg(a, k, plan, rms_first_step)
    _compare(out, ref)
    if qualifies:
        _advance_ran((acc_ref, plain_ref), (acc_out, plain_out))
    else:
        assert acc_out == acc_ref and plain_out == plain_ref
    assert refused_ref == 0
    return tiles, refused_out, ref


@pytest.mark.parametrize('config,reflector,rms_first_step', [
    ('C1', False, 1),           # pairing
    ('C1', False, 2),           # pairing from an even step: the reads of PLAN fall on an open pair
    ('C3', True, 1),
    ('C3', True, 2),
    ('C3', True, 10 ** 6),      # beyond nt: the plain flavours only
])
def test_fluid_media_equal_the_two_pass_update(monkeypatch, config, reflector, rms_first_step):
    """water (UNI bodies) and the multi-material CT fluid with reflector voxels inside a run's inner planes and across run and tile borders"""
    a, k = _problem(config, reflector=reflector)
    tiles, _, ref = _both(monkeypatch, a, k, PLAN, rms_first_step)
    assert tiles['solid'] == 0
    if rms_first_step < STEPS:
        assert max(np.abs(v).max() for n, v in ref[0].items() if n[:4] in ('rms_', 'peak')) > 0


@pytest.mark.parametrize('zrun', [8, 16, 32])
def test_run_lengths(monkeypatch, zrun):
    """runs of at most 8, 16 and 32 planes: 5, 13 and 29 advanced planes in a full run"""
    monkeypatch.setenv('BFD_ZRUN', str(zrun))
    a, k = _problem('C3', reflector=True)
    _both(monkeypatch, a, k, PLAN, 1)


def test_split_half_steps_and_a_refused_setter(monkeypatch):
    """steps taken by their half-steps: the sensor map set and maps read in between; set_materials is refused there and changes nothing"""
    a, k = _problem('C3', reflector=True)
    plan = (('run', 21), ('split',), ('split',), ('refuse',), ('run', 8), ('maps',), ('refuse',), ('split',), ('set',), ('run', 5), ('maps',))
    _, refused, _ = _both(monkeypatch, a, k, plan, 1)
    assert refused == 2


def test_stress_source_keeps_the_two_pass_update(monkeypatch):
    """a stress-type source changes Szz between the two kernels of a step: no advance, same byte tables, same results"""
    a, k = _problem('C3', reflector=True, stress_source=True)
    _both(monkeypatch, a, k, PLAN, 1, qualifies=False)


def test_medium_with_solid_runs_keeps_the_two_pass_update(monkeypatch):
    """the skull medium: velocity_solid and the sparse kernel read their fluid neighbours' Vz, so the whole engine stays on the two-pass update"""
    a, k = _problem('C2')
    tiles, refused, _ = _both(monkeypatch, a, k, PLAN + (('refuse',),), 1, qualifies=False)
    assert tiles['solid'] > 0 and refused == 0


@pytest.mark.parametrize('steps', [STEPS, 241])
def test_two_slabs_of_one_volume_equal_one_engine(monkeypatch, steps):
    """the Z-slab split inside the library against one engine on the two-pass update: a slab's first and last runs advance too. In 160 steps the
    wave only just comes to the cut at z = 50; in 241 it is well inside the second slab"""
    from babelbrain_amd.PropagationModel import compact_sources
    a, k, info = H.make_problem('C3', N=N, steps=steps, stable_dt_fn=oracle_dt, zslab=(0, N[2]), full_sensors=False)
    MaterialMap, ml, f, SourceMap, Pulse, h, T, SensorMap = a
    lin, row, wx, wy, wz = compact_sources(np.asarray(SourceMap), k['Ox'], k['Oy'], k['Oz'])

    def leg(devices):
        g = _engine.Group(devices, *N, len(ml), h, k['DT'], f, steps, sensorSub=k['SensorSubSampling'], sensorStart=k['SensorStart'],
                          selRMSorPeak=3, selMapsRMS=list(MAPS), selMapsSensors=['Pressure', 'Vz'], rmsFirstStep=1)
        try:
            g.set_materials(ml, k.get('QCorrection', 1.0))
            g.set_material_map(MaterialMap)
            g.set_sources(lin, row, wx, wy, wz, Pulse)
            g.set_sensor_map(SensorMap)
            g.prepare()
            g.run(79)
            g.sync()
            first = [g.get_map(KIND_RMS, n) for n in MAPS]
            g.run(steps - 79)
            g.sync()
            res = first + [g.get_map(kind, n) for n in MAPS for kind in (KIND_RMS, KIND_PEAK, KIND_LAST)] + [g.sensors()]
            return res, [g.slab(r)[3].algorithmic_bytes(False) for r in range(g.size)]
        finally:
            g.close()

    monkeypatch.setenv('BFD_ADV_VZ', '0')
    ref, _ = leg([0])
    _, bytes_ref = leg([0, 0])
    monkeypatch.delenv('BFD_ADV_VZ')
    out, bytes_out = leg([0, 0])
    assert len(bytes_out) == 2
    for bo, br in zip(bytes_out, bytes_ref):
        less = br['velocity_fluid'] - bo['velocity_fluid']
        assert less > 0 and less == 2 * (bo['stress_fluid'] - br['stress_fluid'])
    for o, r in zip(out, ref):
        assert np.array_equal(o, r)
    vz_rms = ref[len(MAPS) + 3]
    print('planes with RMS(Vz) != 0:', np.flatnonzero(vz_rms.max(axis=(0, 1)))[[0, -1]])
    assert vz_rms[:, :, 40:48].max() > 0
    if steps > STEPS:
        assert vz_rms[:, :, N[2] // 2 + 8:].max() > 0        # the wave is in the second slab, past its first run
