"""Inputs replaced on a live engine (include/babelfdtd.h: bfd_reset keeps the inputs, every setter may be called again, either form of source
releases the other, bfd_set_reflector(NULL) clears the mask). Behind those promises sit the class bytes and run lists, the fused runs, the compact
solid state and its row table, the sparse shear list with its memory variables, the activity map, the BFD_RUN_ADV_VZ bit, the open accumulation
pair, srcLowEnd / srcHighBeg, the streamed / resident / separable source tables and, in a group, the halo plan. A stale one of them gives plausible,
finite, wrong fields, so every run here is held, element by element, to the CPU oracle given the inputs in force (tests/util.py::assert_same) and,
bit for bit, to a fresh engine that only ever saw those inputs. The engine under test is never its own reference.

Part A replaces inputs after bfd_reset, in chains of short runs on 64 x 56 x 72 (and 192 x 40 x 72 where a run must lie outside the absorbing
layer for Vz to advance), through one Engine and through Group([0, 0, 0]) in both step orders. Part B replaces them in the middle of a run where the
oracle still defines the answer: a cell whose 15 fields and whose neighbours within the stencil are exactly zero does not know its material, so a
map changed only in such cells at step n must give what the new map gives from step 0 (B1; each case asserts the zero zone itself, on the engine's
fields, before it calls the setter); and adding 0.0 changes nothing, so sources A before step n and B from step n on equal the oracle given both
with the complementary columns of their tables zeroed (B2, additive source types only)."""
import numpy as np
import pytest

from babelbrain_amd import _engine, harness as H
from babelbrain_amd._engine import FIELD_NAMES, KIND_RMS
from babelbrain_amd.PropagationModel import compact_sources
from babelbrain_amd.sources import SeparableSource
from oracle import oracle as O
from tests.util import ALL_MAPS, assert_same, oracle_dt

pytestmark = pytest.mark.gpu

# the nine state arrays the oracle's last maps cover; the six memory variables are held to the fresh engine only
FIELD_TO_MAP = (('Vx', 'Vx'), ('Vy', 'Vy'), ('Vz', 'Vz'), ('Sxx', 'Sigmaxx'), ('Syy', 'Sigmayy'), ('Szz', 'Sigmazz'),
                ('Sxy', 'Sigmaxy'), ('Sxz', 'Sigmaxz'), ('Syz', 'Sigmayz'))
RMS_MAPS = ('Pressure', 'Vz')
ONE = np.array([1.0])


# ------------------------------------------------------------------------------------------------------------------------------------------
# problems and inputs
# ------------------------------------------------------------------------------------------------------------------------------------------
def _base(N, nt, all_steps=False):
    """The skull medium (water, cortical bone with shear, brain) at size N with the caller's own plane source: everything a run needs but the
    inputs that the tests replace."""
    a, k, info = H.make_problem('C2', N=N, steps=nt, stable_dt_fn=oracle_dt, full_sensors=False, accumulate_all_steps=all_steps)
    mm, ml, f, smap, pulse, h, T, sensor = a
    rho_c = ml[0, 0] * ml[0, 1]
    lin, row = compact_sources(smap, ONE, ONE, ONE)[:2]
    return dict(N=tuple(N), nt=nt, f=f, h=h, DT=k['DT'], ND=k['NDelta'], sub=k['SensorSubSampling'], start=k['SensorStart'], ml=np.array(ml, np.float64),
                qc=np.array(k['QCorrection'], np.float64), mm=np.ascontiguousarray(mm), sensor=np.ascontiguousarray(sensor), lin=lin, row=row,
                pulse=np.ascontiguousarray(pulse), rho_c=rho_c,
                # Ox, Oy, Oz: a velocity source pushes along all three axes; a stress source has weight 1 (the back-propagation call)
                weights={0: (0.25 / rho_c, 0.5 / rho_c, 1.0 / rho_c), 2: (1.0, 1.0, 1.0)})


def _inputs(p, **kw):
    inp = dict(ml=p['ml'], qc=p['qc'], mm=p['mm'], refl=None, lin=p['lin'], row=p['row'], pulse=p['pulse'], sensor=p['sensor'])
    inp.update(kw)
    return inp


def _voxels(p, ijk):
    """(lin, row) of a list of voxels, row r = position in the list; linear index x fastest"""
    N1, N2, N3 = p['N']
    ijk = np.asarray(ijk, np.int64)
    assert (ijk >= 0).all() and (ijk < np.array(p['N'])).all()
    lin = ijk[:, 0] + N1 * (ijk[:, 1] + N2 * ijk[:, 2])
    assert len(set(lin.tolist())) == len(lin)
    return lin, np.arange(len(lin), dtype=np.uint32)


def _tones(p, rows, nt, seed, scale=1.0):
    """rows CW signals of different amplitude and phase with the caller's half-cosine ramp, nt columns, as a K = 2 separable table; dense() is the
    float64 table of the same float32 values"""
    rng = np.random.default_rng(seed)
    t = np.arange(nt) * p['DT']
    ramp = np.ones(nt)
    rp = min(int(round(4 / p['f'] / p['DT'])), nt)
    ramp[:rp] = (1 - np.cos(np.pi * np.arange(rp) / rp)) * 0.5
    amp, ph = scale * rng.uniform(0.5, 1.0, rows), rng.uniform(0, 2 * np.pi, rows)
    wt = 2 * np.pi * p['f'] * t
    return SeparableSource(np.stack([amp * np.cos(ph), amp * np.sin(ph)], axis=1), np.stack([np.sin(wt) * ramp, np.cos(wt) * ramp], axis=0))


def _dense(pulse):
    return pulse.dense() if isinstance(pulse, SeparableSource) else np.ascontiguousarray(np.atleast_2d(pulse), np.float64)


def _source_map(p, lin, row):
    N1, N2, N3 = p['N']
    smap = np.zeros(p['N'], np.uint32)
    lin = np.asarray(lin, np.int64)
    smap[lin % N1, (lin // N1) % N2, lin // (N1 * N2)] = np.asarray(row, np.uint32) + 1
    return smap


def _oracle(p, inp, type_source, nt=None):
    """the CPU oracle on these inputs from step 0: every last map, the RMS maps and the Pressure series"""
    nt = p['nt'] if nt is None else nt
    wx, wy, wz = p['weights'][type_source]
    pulse = _dense(inp['pulse']) if len(inp['lin']) else np.zeros((1, nt))
    out = O.StaggeredFDTD_3D_with_relaxation(
        inp['mm'], inp['ml'], p['f'], _source_map(p, inp['lin'], inp['row']), pulse, p['h'], nt * p['DT'], inp['sensor'],
        Ox=np.array([wx]), Oy=np.array([wy]), Oz=np.array([wz]), NDelta=p['ND'], DT=p['DT'], SelMapsRMSPeakList=ALL_MAPS,
        SelMapsSensorsList=['Pressure'], SelRMSorPeak=1, TypeSource=type_source, QfactorCorrection=True, QCorrection=inp['qc'],
        SensorSubSampling=p['sub'], SensorStart=p['start'], ReflectorMask=inp['refl'])
    assert out[-1]['nt'] == nt
    return out


def _dilate(mask, r):
    """box dilation by r cells along every axis"""
    out = np.array(mask, bool)
    for ax in range(3):
        acc = out.copy()
        for s in range(1, r + 1):
            to, fr = [slice(None)] * 3, [slice(None)] * 3
            to[ax], fr[ax] = slice(s, None), slice(None, -s)
            acc[tuple(to)] |= out[tuple(fr)]
            acc[tuple(fr)] |= out[tuple(to)]
        out = acc
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# the engine or group under test
# ------------------------------------------------------------------------------------------------------------------------------------------
class _Rig:
    """One Engine, or one Group of Z-slabs on device 0, behind the same few calls; `inp` follows what the setters were given, under the ABI's own
    rules (a new material map clears the reflector, a mask replaces the one before), so that it always names the inputs in force."""

    def __init__(self, p, inp, type_source=0, devices=None, rms_first_step=0):
        self.p, self.type, self.group = p, type_source, devices is not None
        kw = dict(NDelta=p['ND'], typeSource=type_source, sensorSub=p['sub'], sensorStart=p['start'], selRMSorPeak=1, selMapsRMS=list(RMS_MAPS),
                  selMapsSensors=['Pressure'], rmsFirstStep=rms_first_step)
        nMat = len(inp['ml'])
        if self.group:
            self.e = _engine.Group(devices, *p['N'], nMat, p['h'], p['DT'], p['f'], p['nt'], **kw)
        else:
            self.e = _engine.Engine(*p['N'], nMat, p['h'], p['DT'], p['f'], p['nt'], **kw)
        self.inp = {}
        try:
            self.set_materials(inp['ml'], inp['qc'])
            self.set_map(inp['mm'])
            if inp['refl'] is not None:
                self.set_reflector(inp['refl'])
            self.set_sources(inp['lin'], inp['row'], inp['pulse'])
            self.set_sensors(inp['sensor'])
        except Exception:
            self.close()
            raise

    def close(self):
        self.e.close()

    def views(self):
        return [self.e.slab(r)[3] for r in range(self.e.size)] if self.group else [self.e]

    def sync(self):
        self.e.sync()

    def set_materials(self, ml, qc):
        self.e.set_materials(ml, qc)
        self.inp.update(ml=np.array(ml, np.float64), qc=np.array(qc, np.float64))

    def set_map(self, mm):
        if self.group:
            self.e.set_material_map(mm)
        else:
            self.e.set_material_map(mm, 0, 0)
        self.inp.update(mm=np.ascontiguousarray(mm, np.uint32), refl=None)          # the ids are rewritten: the reflector bit goes with them

    def set_reflector(self, mask):
        self.e.set_reflector(mask)
        self.inp.update(refl=None if mask is None else np.ascontiguousarray(mask, np.uint32))

    def set_sources(self, lin, row, pulse):
        n = len(lin)
        w = [None if v == 1.0 else np.full(n, v, np.float32) for v in self.p['weights'][self.type]]
        if not n and not isinstance(pulse, SeparableSource):
            pulse = np.zeros((1, 1))
        self.e.set_sources(np.asarray(lin, np.int64), np.asarray(row, np.uint32), w[0], w[1], w[2], pulse)
        self.inp.update(lin=np.asarray(lin, np.int64), row=np.asarray(row, np.uint32), pulse=pulse)

    def set_sensors(self, sensor):
        self.e.set_sensor_map(sensor)
        self.inp.update(sensor=np.ascontiguousarray(sensor, np.uint32))

    def run(self, n):
        self.e.run(n)

    def reset(self):
        self.e.reset()

    def fields(self):
        self.sync()
        vs = self.views()
        return {n: np.concatenate([v.get_field(n) for v in vs], axis=2) for n in FIELD_NAMES}

    def outputs(self):
        out = self.fields()
        for m in RMS_MAPS:
            out['rms_' + m] = self.e.get_map(KIND_RMS, m)
        out['sensors'] = self.e.sensors()
        out['sensor_index'] = self.e.sensor_index()
        return out

    def solid_tiles(self):
        return sum(v.tile_counts()['solid'] for v in self.views())


def _fresh(p, inp, type_source, legs, rms_first_step=0):
    """a fresh single engine that only ever sees these inputs: its outputs and, after the first leg, its activity counts"""
    rig = _Rig(p, inp, type_source, rms_first_step=rms_first_step)
    try:
        rig.run(legs[0])
        act = rig.e.activity_counts()
        for n in legs[1:]:
            rig.run(n)
        out = rig.outputs()
        out['activity'] = act
        return out
    finally:
        rig.close()


_REFS = {}


def _references(key, p, inp, type_source, legs, rms_first_step=0):
    """(oracle, fresh engine) of a stage: computed once, shared by every rig that runs the stage, never written to"""
    if key not in _REFS:
        assert sum(legs) == p['nt']
        _REFS[key] = (_oracle(p, inp, type_source), _fresh(p, dict(inp), type_source, legs, rms_first_step))
    return _REFS[key]


def _hold(out, ref, fresh, p, inp, what):
    """every output of the rig against the oracle (element by element) and against the fresh engine (bit for bit)"""
    geo = (p['N'], p['ND'], inp['mm'])
    for fld, key in FIELD_TO_MAP:
        assert_same(out[fld], ref[1][key], '%s: get_field(%s)' % (what, fld), geo)
    for m in RMS_MAPS:
        assert_same(out['rms_' + m], ref[2][m], '%s: RMS map of %s' % (what, m), geo)
    assert np.array_equal(out['sensor_index'], ref[-1]['IndexSensorMap']), what
    assert out['sensors'].shape[0] == 1
    assert_same(out['sensors'][0], ref[0]['Pressure'], '%s: sensor block' % what, geo, (ref[-1]['IndexSensorMap'], p['N']))
    for n in fresh:
        if n != 'activity':
            assert out[n].shape == fresh[n].shape and np.array_equal(out[n], fresh[n]), '%s: %s differs from the fresh engine' % (what, n)


RIGS = [('engine', 0), ('engine', 2), ('group-serial', 0), ('group-overlap', 0)]      # TypeSource is fixed per engine: the chains run with 0 and with 2


def _make_rig(monkeypatch, rig, p, inp, type_source, **kw):
    devices = None
    if rig != 'engine':
        monkeypatch.setenv('BFD_GROUP_OVERLAP', '1' if rig == 'group-overlap' else '0')
        devices = [0, 0, 0]
    return _Rig(p, inp, type_source, devices=devices, **kw)


N_A, NT_A, LEG_A = (64, 56, 72), 200, 60
POINT_A = [(32, 28, 30), (30, 26, 33), (35, 30, 28)]                       # mid-grid, above the shell
# first and last z-chunk of the domain and of every 24-plane slab, and sub-tiles far from the plane source and from POINT_A
POINT_B = [(13, 13, 3), (50, 42, 69), (40, 30, 40), (20, 20, 24), (30, 40, 47), (33, 17, 25), (47, 15, 48), (16, 41, 23)]


def _chain_problem(type_source):
    p = _base(N_A, NT_A)
    inp = _inputs(p)
    if type_source == 2:
        lin, row = _voxels(p, POINT_A)
        inp.update(lin=lin, row=row, pulse=_tones(p, len(lin), NT_A, 5).dense())
    return p, inp


def _stage(rig, change, order, p, key, what, legs=(LEG_A, NT_A - LEG_A)):
    """one link of a chain: the inputs replaced before or after bfd_reset, the run, and the comparison with the oracle and the fresh engine on the
    inputs now in force. Returns (outputs, oracle, fresh, activity after the first leg)."""
    rig.sync()
    if order == 'set-reset':
        change(rig)
        rig.reset()
    else:
        rig.reset()
        change(rig)
    ref, fresh = _references(key, p, dict(rig.inp), rig.type, legs)
    rig.run(legs[0])
    rig.sync()
    act = [v.activity_counts() for v in rig.views()]
    for n in legs[1:]:
        rig.run(n)
    out = rig.outputs()
    _hold(out, ref, fresh, p, rig.inp, what)
    return out, ref, fresh, act


# ------------------------------------------------------------------------------------------------------------------------------------------
# A. replaced after a reset
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rig_kind,type_source', RIGS)
def test_media_replaced_after_a_reset(rig_kind, type_source, monkeypatch):
    """all-fluid -> bone in the middle slab only -> all-fluid -> the skull shell (the solid region moved and changed size: another shear list) ->
    another material table of the same length with another cmax (other CPML profiles) under the engine's fixed DT. In the group the middle slab's
    bfd_halo_fields goes 4 -> 7 -> 4 and the halo plan follows."""
    p, inp = _chain_problem(type_source)
    fluid = np.where(p['mm'] == 1, 2, p['mm']).astype(np.uint32)
    block = fluid.copy()
    block[18:46, 14:40, 28:44] = 1                                          # inside planes 24 .. 47, two planes and more away from either cut
    M = H.MATERIALS[500e3]
    ml2 = np.array([M['Water'], M['Trabecular'], M['Skin']], np.float64)
    cmax1, cmax2 = O.tables(p['ml'], p['f'], p['h'], p['DT'])[2], O.tables(ml2, p['f'], p['h'], p['DT'])[2]
    assert cmax2 < cmax1 and (p['mm'] == 1).any() and not (fluid == 1).any()
    rig = _make_rig(monkeypatch, rig_kind, p, _inputs(p, **dict(inp, mm=fluid)), type_source)
    try:
        solid, masks = [], []
        plan = [('fluid', lambda r: None, 'set-reset'), ('block', lambda r: r.set_map(block), 'set-reset'), ('fluid again', lambda r: r.set_map(fluid), 'reset-set'),
                ('shell', lambda r: r.set_map(p['mm']), 'reset-set'), ('other table', lambda r: r.set_materials(ml2, p['qc']), 'set-reset')]
        for name, change, order in plan:
            out, ref, _, _ = _stage(rig, change, order, p, ('media', type_source, name), '%s, %s' % (rig_kind, name))
            solid.append(rig.solid_tiles())
            masks.append([[v.halo_fields()[g] for g in (0, 1)] for v in rig.views()])
            assert ref[2]['Pressure'].max() > 0
        assert solid[0] == 0 and solid[2] == 0 and solid[1] > 0 and solid[3] > 0 and solid[1] != solid[3], solid
        assert np.abs(_REFS[('media', type_source, 'block')][0][1]['Sigmaxy']).max() > 0
        if rig.group:
            assert [rig.e.slab(r)[:2] for r in range(3)] == [(0, 24), (24, 24), (48, 24)]
            lean, full = [[2], [2]], [[0, 1, 2], [0, 1, 2]]
            assert masks[0] == [lean] * 3 and masks[1] == [lean, full, lean] and masks[2] == [lean] * 3 and masks[3][1] == full, masks
    finally:
        rig.close()


@pytest.mark.parametrize('rig_kind,type_source', RIGS)
def test_reflector_replaced_after_a_reset(rig_kind, type_source, monkeypatch):
    """mask A, then mask B (B alone must hold: or_reflector takes the old bit off first), then none, then mask A followed by a new material map,
    which rewrites the ids and with them the reflector: the run equals the oracle without one."""
    p, inp = _chain_problem(type_source)
    A = np.zeros(p['N'], np.uint32); A[24:34, 20:30, 20:26] = 1
    B = np.zeros(p['N'], np.uint32); B[30:44, 26:36, 44:50] = 1            # across the cut between planes 47 and 48
    moved = np.where(p['mm'] == 1, 2, p['mm']).astype(np.uint32)
    moved[20:40, 30:44, 36:52] = 1

    def mask_then_map(r):
        r.set_reflector(A)
        r.set_map(moved)
    rig = _make_rig(monkeypatch, rig_kind, p, inp, type_source)
    try:
        rms = {}
        plan = [('mask A', lambda r: r.set_reflector(A), 'set-reset'), ('mask B', lambda r: r.set_reflector(B), 'reset-set'),
                ('no mask', lambda r: r.set_reflector(None), 'set-reset'), ('mask A then a new map', mask_then_map, 'reset-set')]
        for name, change, order in plan:
            out, ref, _, _ = _stage(rig, change, order, p, ('reflector', type_source, name), '%s, %s' % (rig_kind, name))
            rms[name] = ref[2]['Pressure']
        assert rig.inp['refl'] is None
        # the masks matter: each of the three runs on the first map has a Pressure map of its own
        assert not np.array_equal(rms['mask A'], rms['mask B']) and not np.array_equal(rms['mask B'], rms['no mask']) and not np.array_equal(rms['mask A'], rms['no mask'])
    finally:
        rig.close()


@pytest.mark.parametrize('rig_kind,type_source', RIGS)
def test_sources_and_sensors_replaced_after_a_reset(rig_kind, type_source, monkeypatch):
    """Another voxel set (first and last z-chunk, sub-tiles the sources before never marked) and the forms in turn: dense resident -> streamed in
    tiles of 7 steps -> separable -> dense resident -> no source at all, which must leave every field exactly zero; a second sensor map with sensors in
    the planes next to the cuts. Quiet runs are on: set_sources then reset and reset then set_sources both start the activity map over, and after the
    first 60 steps it counts what a fresh engine's counts."""
    p, inp = _chain_problem(type_source)
    monkeypatch.setenv('BFD_SKIP_ZERO', '1')
    linA, rowA, pulseA = inp['lin'], inp['row'], inp['pulse']
    linB, rowB = _voxels(p, POINT_B)
    sepB = _tones(p, len(linB), NT_A, 9, scale=40.0 if type_source == 0 else 1.0)
    box = np.zeros(p['N'], np.uint32); box[20:30, 20:28, 20:50] = 1
    assert box[:, :, [23, 24, 47, 48]].any(axis=(0, 1)).all()

    def streamed(r):
        with monkeypatch.context() as m:
            m.setenv('BFD_SOURCE_TILE', '7')
            r.set_sources(linA, rowA, pulseA)
    rig = _make_rig(monkeypatch, rig_kind, p, inp, type_source)
    try:
        plan = [('first set', lambda r: None, 'set-reset'),
                ('moved voxels, dense', lambda r: r.set_sources(linB, rowB, sepB.dense()), 'set-reset'),
                ('first set, streamed', streamed, 'reset-set'),
                ('moved voxels, separable', lambda r: r.set_sources(linB, rowB, sepB), 'set-reset'),
                ('first set, dense', lambda r: r.set_sources(linA, rowA, pulseA), 'reset-set'),
                ('second sensor map', lambda r: r.set_sensors(box), 'set-reset'),
                ('no source', lambda r: r.set_sources(linA[:0], rowA[:0], np.zeros((1, 1))), 'reset-set')]
        for name, change, order in plan:
            out, ref, fresh, act = _stage(rig, change, order, p, ('sources', type_source, name), '%s, %s' % (rig_kind, name))
            assert all(t > 0 for _, t in act), act                         # quiet runs are on, in the engine and in every slab
            if not rig.group:
                assert act == [fresh['activity']] and (name == 'no source' or 0 < act[0][0] <= act[0][1]), (name, act, fresh['activity'])
            if name == 'no source':
                for n, v in out.items():
                    assert n == 'sensor_index' or not v.any(), n
                assert not any(np.asarray(v).any() for q in (1, 2) for v in ref[q].values())
            else:
                assert ref[2]['Pressure'].max() > 0 and np.abs(ref[0]['Pressure']).max() > 0
        assert out['sensors'].shape[1] == int(box.sum())
    finally:
        rig.close()


N_W, NT_W = (192, 40, 72), 160       # one x-tile (64 .. 127) and one y-tile (16 .. 23) outside the absorbing layer: runs that advance Vz exist


def _advance_bytes(monkeypatch, p, inp, rms_first_step):
    """velocity_fluid's bytes per launch in an engine that never advances Vz (BFD_ADV_VZ=0) on these inputs"""
    with monkeypatch.context() as m:
        m.setenv('BFD_ADV_VZ', '0')
        rig = _Rig(p, inp, 0, rms_first_step=rms_first_step)
    try:
        rig.e.prepare()
        return rig.e.algorithmic_bytes(False)['velocity_fluid']
    finally:
        rig.close()


def test_fluid_solid_fluid_switches_the_vz_advance_and_the_pairing(monkeypatch):
    """An engine built as bench.py builds its own (rmsFirstStep = 1: no quiet runs) qualifies for the advanced Vz and the paired accumulation
    while its medium is all fluid: all-fluid -> skull -> all-fluid switches the BFD_RUN_ADV_VZ bit on, off and on, and every run equals the oracle."""
    p = _base(N_W, NT_W, all_steps=True)                                    # the oracle accumulates from SensorStart: 0, as rmsFirstStep = 1 does
    assert p['start'] == 0
    fluid = np.where(p['mm'] == 1, 2, p['mm']).astype(np.uint32)
    rig = _Rig(p, _inputs(p, mm=fluid), 0, rms_first_step=1)
    try:
        seen = []
        for name, mm in (('fluid', fluid), ('skull', p['mm']), ('fluid again', fluid)):
            rig.reset()
            rig.set_map(mm)
            before = rig.e.paired_launches()
            ref, fresh = _references(('wide', name), p, dict(rig.inp), 0, (NT_W,), rms_first_step=1)
            rig.run(NT_W)
            _hold(rig.outputs(), ref, fresh, p, rig.inp, name)
            plain = _advance_bytes(monkeypatch, p, dict(rig.inp), 1)
            seen.append((rig.solid_tiles(), rig.e.paired_launches() - before, plain - rig.e.algorithmic_bytes(False)['velocity_fluid']))
            assert rig.e.activity_counts() == (0, 0) and ref[2]['Pressure'].max() > 0
        (s0, p0, a0), (s1, p1, a1), (s2, p2, a2) = seen
        assert s0 == 0 and s2 == 0 and s1 > 0, seen
        assert p0 > 0 and p2 > 0, seen                                      # the fluid runs paired their accumulating steps
        assert a0 > 0 and a2 == a0 and a1 == 0, seen                        # Vz advanced in the first and third run, not beside solid runs
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
# B1. the material map (or the reflector) changed in the zero zone in the middle of a run
# ------------------------------------------------------------------------------------------------------------------------------------------
N_B, NT_B = (64, 56, 160), 640


def _flipped(p):
    """the same problem upside down: the source plane near the high-z end, so that the bone the wave excites first has the HIGHER linear indices"""
    q = dict(p)
    q['mm'] = np.ascontiguousarray(p['mm'][:, :, ::-1])
    q['sensor'] = np.ascontiguousarray(p['sensor'][:, :, ::-1])
    smap = np.ascontiguousarray(_source_map(p, p['lin'], p['row'])[:, :, ::-1])
    lin, row = compact_sources(smap, ONE, ONE, ONE)[:2]
    q['lin'], q['row'] = lin, row
    return q


def _zero_zone(fields, changed):
    """the precondition of B1: all 15 fields exactly zero in the changed cells and 4 cells around them"""
    zone = _dilate(changed, 4)
    assert changed.any() and zone.sum() > changed.sum()
    for n in FIELD_NAMES:
        assert not fields[n][zone].any(), 'precondition: %s is not zero around the changed cells' % n


def _excited_solid(fields, mm):
    shear = (fields['Sxy'] != 0) | (fields['Sxz'] != 0) | (fields['Syz'] != 0)
    return int((shear & (mm == 1)).sum())


def _changed_mid_run(rig, p, steps, key, what, legs=None):
    """steps = [(n, change, changed cells)] in ascending n: runs to step n, asserts the zero zone on the rig's own fields, calls the setter, checks
    that a field read before the next step is still the same field, and goes on. At the end the rig equals the oracle and a fresh engine, both
    given the final inputs from step 0. Returns (outputs, oracle, the fields read at each change)."""
    at, seen = 0, []
    for n, change, changed in steps:
        rig.run(n - at)
        at = n
        before = rig.fields()
        _zero_zone(before, changed)
        change(rig)
        after = rig.fields()
        for f in FIELD_NAMES:
            assert np.array_equal(after[f], before[f]), '%s: get_field(%s) between the setter at step %d and the next step' % (what, f, n)
        seen.append(before)
    rig.run(p['nt'] - at)
    ref, fresh = _references(key, p, dict(rig.inp), rig.type, legs or (p['nt'],), rms_first_step=rig.e.cfg.rmsFirstStep)
    out = rig.outputs()
    _hold(out, ref, fresh, p, rig.inp, what)
    return out, ref, seen


ISLAND = (slice(24, 40), slice(20, 36), slice(40, 52))                      # in the flipped problem: lower linear indices than all of the shell


def _compact_env(monkeypatch, form):
    monkeypatch.setenv('BFD_COMPACT_SOLID', '0' if form == 'full-volume' else '1')
    monkeypatch.setenv('BFD_COMPACT_HOSTED', '0' if form == 'own-block' else '1')


@pytest.mark.parametrize('form', ['hosted', 'own-block', 'full-volume'])
@pytest.mark.parametrize('direction', ['inserted', 'removed'])
def test_island_before_the_excited_bone_renumbers_the_rows(direction, form, monkeypatch):
    """At step 80 more than 1000 cells of the shell hold a shear stress. A still-zero bone island of lower linear indices is inserted (or taken
    out): every excited cell gets another row of the compact solid state (hosted in the full-volume buffers or in a block of its own), or -- with
    BFD_COMPACT_SOLID=0 -- another slot of the sparse shear memory. The values must travel with their cells."""
    _compact_env(monkeypatch, form)
    p = _flipped(_base(N_B, NT_B))
    shell = p['mm']
    both = shell.copy(); both[ISLAND] = 1
    assert not (shell[ISLAND] == 1).any() and np.flatnonzero(both.transpose(2, 1, 0) == 1)[0] < np.flatnonzero(shell.transpose(2, 1, 0) == 1)[0]
    first, last = (shell, both) if direction == 'inserted' else (both, shell)
    rig = _Rig(p, _inputs(p, mm=first), 0)
    try:
        n_solid = rig.solid_tiles()
        out, ref, seen = _changed_mid_run(rig, p, [(80, lambda r: r.set_map(last), first != last)], ('island', direction), '%s, %s' % (direction, form))
        assert _excited_solid(seen[0], first) >= 1000
        assert rig.solid_tiles() != n_solid
        if direction == 'inserted':
            assert np.abs(ref[1]['Sigmaxy'][ISLAND]).max() > 0           # the wave did reach the island
        assert max(np.abs(out[n]).max() for n in ('Rxy', 'Rxz', 'Ryz')) > 0
    finally:
        rig.close()


FAR_ISLAND = (slice(22, 42), slice(18, 38), slice(100, 112))


@pytest.mark.parametrize('form', ['hosted', 'own-block', 'full-volume'])
def test_the_only_island_removed_and_put_back(form, monkeypatch):
    """A medium whose only bone is a still-zero island: taken out at step 80 (no solid run is left, the compact state goes) and put back at step
    160 (it comes back, still ahead of the wave). Equal to the oracle with the island from step 0."""
    _compact_env(monkeypatch, form)
    p = _base(N_B, NT_B)
    fluid = np.where(p['mm'] == 1, 2, p['mm']).astype(np.uint32)
    island = fluid.copy(); island[FAR_ISLAND] = 1
    rig = _Rig(p, _inputs(p, mm=island), 0)
    try:
        counts = [rig.solid_tiles()]

        def take_out(r):
            r.set_map(fluid)
            counts.append(r.solid_tiles())

        def put_back(r):
            r.set_map(island)
            counts.append(r.solid_tiles())
        out, ref, _ = _changed_mid_run(rig, p, [(80, take_out, island != fluid), (160, put_back, island != fluid)], ('only island',), form)
        assert counts[0] > 0 and counts[1] == 0 and counts[2] == counts[0], counts
        assert np.abs(ref[1]['Sigmaxy'][FAR_ISLAND]).max() > 0
    finally:
        rig.close()


def test_first_island_in_an_engine_that_advances_vz_with_a_pair_open(monkeypatch):
    """An all-fluid engine with advanced Vz and paired accumulation (rmsFirstStep = 1) gets its first bone island after an odd number of steps: the
    open pair is settled, the bit goes, the solid kernels come in, inside the x- and y-tile whose runs advanced."""
    p = _base(N_W, 320, all_steps=True)
    fluid = np.where(p['mm'] == 1, 2, p['mm']).astype(np.uint32)
    where = (slice(80, 104), slice(14, 26), slice(46, 56))
    island = fluid.copy(); island[where] = 1
    rig = _Rig(p, _inputs(p, mm=fluid), 0, rms_first_step=1)
    try:
        rig.e.prepare()
        plain = _advance_bytes(monkeypatch, p, dict(rig.inp), 1)
        assert rig.solid_tiles() == 0 and rig.e.algorithmic_bytes(False)['velocity_fluid'] < plain
        out, ref, seen = _changed_mid_run(rig, p, [(7, lambda r: r.set_map(island), island != fluid)], ('first island',), 'first island')
        assert rig.e.paired_launches() > 0 and rig.solid_tiles() > 0
        assert np.abs(seen[0]['Vz']).max() > 0 and np.abs(ref[1]['Sigmaxy'][where]).max() > 0
    finally:
        rig.close()


@pytest.mark.parametrize('overlap', ['0', '1'])
def test_island_lands_in_an_all_fluid_slab_of_a_group(overlap, monkeypatch):
    """Three Z-slabs; the shell lies in the first two, the third reads Vz / Szz only from its neighbour (bfd_halo_fields 4) until the island
    lands in it at step 80: its mask becomes 7 and the halo plan must follow."""
    monkeypatch.setenv('BFD_GROUP_OVERLAP', overlap)
    p = _base(N_B, NT_B)
    where = (FAR_ISLAND[0], FAR_ISLAND[1], slice(110, 122))
    island = p['mm'].copy(); island[where] = 1
    rig = _Rig(p, _inputs(p), 0, devices=[0, 0, 0])
    try:
        k0 = rig.e.slab(2)[0]
        assert k0 <= 110 and not (p['mm'][:, :, k0 - 2:] == 1).any() and (p['mm'][:, :, :k0 - 2] == 1).any()
        masks = [[v.halo_fields()[0] for v in rig.views()]]
        out, ref, seen = _changed_mid_run(rig, p, [(80, lambda r: r.set_map(island), island != p['mm'])], ('group island',), 'overlap ' + overlap)
        masks.append([v.halo_fields()[0] for v in rig.views()])
        assert masks[0][2] == [2] and masks[1] == [[0, 1, 2]] * 3 and masks[0][0] == [0, 1, 2], masks
        assert _excited_solid(seen[0], p['mm']) >= 1000 and np.abs(ref[1]['Sigmaxy'][where]).max() > 0
    finally:
        rig.close()


def test_reflector_set_in_the_zero_zone():
    """a reflector mask set at step 80 ahead of the wave equals the oracle with the mask from step 0"""
    p = _base(N_B, NT_B)
    mask = np.zeros(p['N'], np.uint32); mask[24:40, 22:34, 90:96] = 1
    rig = _Rig(p, _inputs(p), 0)
    try:
        out, ref, seen = _changed_mid_run(rig, p, [(80, lambda r: r.set_reflector(mask), mask != 0)], ('reflector mid-run',), 'reflector')
        assert _excited_solid(seen[0], p['mm']) >= 1000
        assert not out['Vz'][mask != 0].any() and np.abs(ref[1]['Vz'][24:40, 22:34, 84:90]).max() > 0
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
# B2. sources replaced in the middle of a run (additive types)
# ------------------------------------------------------------------------------------------------------------------------------------------
NT_S, CUT = 260, 45                                                         # 45 is no multiple of the 7-step tile
SET_A = [(32, 28, 40), (20, 30, 60), (40, 20, 80)]
SET_B = [(13, 13, 3), (50, 42, 156), (30, 30, 100), (33, 17, 25), (22, 40, 12)]


@pytest.mark.parametrize('quiet', ['1', '0'])
@pytest.mark.parametrize('forms', ['resident-resident', 'resident-streamed', 'separable-dense'])
@pytest.mark.parametrize('type_source', [0, 2])
def test_sources_replaced_in_the_middle_of_a_run(type_source, forms, quiet, monkeypatch):
    """Voxel set A with table P_A for steps < 45, the disjoint set B with P_B from step 45 on, both tables of full length and indexed by the
    absolute step. The oracle injects column n of the table at step n (oracle/fdtd_oracle.c: pulse[row * lengthSource + n] with n = its step
    counter, for both source types), so it is given A and B together, P_A zeroed from column 45 on and P_B before it: adding 0.0 changes no value."""
    monkeypatch.setenv('BFD_SKIP_ZERO', quiet)
    p = _base(N_B, NT_S)
    scale = 40.0 if type_source == 0 else 1.0
    linA, rowA = _voxels(p, SET_A)
    linB, rowB = _voxels(p, SET_B)
    assert not set(linA.tolist()) & set(linB.tolist())
    sepA, sepB = _tones(p, len(linA), NT_S, 21, scale), _tones(p, len(linB), NT_S, 22, scale)
    PA, PB = sepA.dense(), sepB.dense()
    assert PA.shape[1] == NT_S and np.abs(PA[:, CUT:]).max() > 0 and np.abs(PB[:, :CUT]).max() > 0      # what the engine must not inject is not zero
    first, second = forms.split('-')
    rig = _Rig(p, _inputs(p, lin=linA, row=rowA, pulse=sepA if first == 'separable' else PA), type_source)
    try:
        rig.run(CUT)
        assert rig.e.step == CUT
        with monkeypatch.context() as m:
            if second == 'streamed':
                m.setenv('BFD_SOURCE_TILE', '7')
            rig.set_sources(linB, rowB, PB)
        rig.run(NT_S - CUT)
        act = rig.e.activity_counts()
        assert (act[1] > 0) == (quiet == '1'), act
        PA0, PB0 = PA.copy(), PB.copy()
        PA0[:, CUT:] = 0.0
        PB0[:, :CUT] = 0.0
        union = _inputs(p, lin=np.concatenate([linA, linB]), row=np.concatenate([rowA, rowB + len(linA)]), pulse=np.vstack([PA0, PB0]))
        ref, fresh = _references(('sources mid-run', type_source), p, union, type_source, (NT_S,))
        _hold(rig.outputs(), ref, fresh, p, union, '%s, type %d, quiet runs %s' % (forms, type_source, quiet))
        assert ref[2]['Pressure'].max() > 0 and np.abs(ref[1]['Sigmaxy']).max() > 0
    finally:
        rig.close()
