"""What a live acoustic study refuses (include/babelfdtd.h, "Acoustic study"; csrc/bfd_acoustic.hip): every argument error of the bfd_acoustic_*
entries in the header's order -- the checks of the entry a stage names, then waterOnly / slot / which, then -6 -- with the first planted fault
reported while every later one is planted too, the outputs keeping their sentinel and bfd_acoustic_traffic unchanged. A handle exists only where
a device does, so this is a GPU test; the refusals of a NULL handle are in tests/test_acoustic_calls_host.py. Also here: the -2 and -6 of
bfd_set_reflector_device, -6 before bfd_acoustic_set_volumes at the C level, and two studies alive at the same time."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from babelbrain_amd import AcousticStudy as AS, Domain as DM, _engine, harness as H
from tests import domain_oracle as DO

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PLAN_KEYS = list(DO.DEFAULTS) + ['FocalLength', 'Aperture']
FREQ = 500e3
P = _engine._ptr


def i64(v):
    return np.array(v, np.int64)


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(GOLDEN, 'domain_golden.json')) as fh:
        meta = json.load(fh)
    return np.load(os.path.join(GOLDEN, 'domain_golden.npz')), meta


def _inputs(golden, name):
    g, meta = golden
    rec = meta['cases'][name]
    return (g[name + '_labels'], g[name + '_ct'] if rec['ct'] else None, g[name + '_air'] if rec['air'] else None, rec,
            {k: rec[k] for k in PLAN_KEYS})


def _materials(n):
    t = H.MATERIALS[FREQ]
    ml = np.tile(np.array(t['Cortical'], np.float64), (n, 1))
    ml[0], ml[1], ml[2] = t['Water'], t['Skin'], t['Brain']
    return ml


class Live:
    """a study with CT and air, planned and assembled, with its engine at step 0"""

    def __init__(self, golden):
        labels, ct, air, rec, kw = _inputs(golden, 'segmented_ct_air')
        self.labels, self.ct, self.air, self.rec = labels, ct, air, rec
        self.st = AS.AcousticStudy(labels, ct, air)
        self.plan = self.st.plan(rec['SpatialStep'], **kw)
        self.ml = _materials(rec['n_materials'])
        self.stats = self.st.assemble(self.plan, len(self.ml))
        self.dt = _engine.stable_dt(self.ml, FREQ, True, rec['SpatialStep'], H.ALPHA_CFL, 1.0)
        self.st.engine(self.ml, FREQ, rec['SpatialStep'], self.dt, 20)
        self.lib, self.h = self.st._lib, self.st._handle()

    def refused(self, rc, want, entry, word, what):
        text = self.lib.bfd_last_error().decode()
        assert rc == want and text.startswith(entry + ': ') and word in text, (what, rc, text)

    def assemble_args(self):
        plan = self.plan
        lo, hi = i64(plan.box_lo), i64(plan.box_hi)
        return dict(lo=lo, size=hi - lo, padLo=i64(plan.pad_lo), padHi=i64(plan.pad_hi), flipK=int(plan.flip_k), lut=DM.relabel_lut(True, True), off=6,
                    zWater=int(plan.ZSourceLocation), nMat=len(self.ml), focalIJ=i64(plan.FocalSpotLocation[:2]), waterOnly=0)


@pytest.fixture(scope='module')
def live(golden):
    v = Live(golden)
    yield v
    v.st.close()


def _ordered(good, faults, call):
    """every fault with all the later ones planted too: the first is the one reported"""
    for q, (name, value, word) in enumerate(faults):
        kw = dict(good)
        for later, v, _ in faults[q + 1:][::-1]:
            kw[later] = v
        kw[name] = value
        call(kw, word, (name, value))


def test_set_volumes_and_survey(live):
    lib, h, before = live.lib, live.h, live.st.traffic()
    for ct, air, word in ((None, live.air, 'a ct is passed'), (live.ct, None, 'an air mask is passed'), (None, None, 'a ct is passed')):
        live.refused(lib.bfd_acoustic_set_volumes(h, P(live.labels), P(ct), P(air)), -1, 'bfd_acoustic_set_volumes', word, word)
    live.refused(lib.bfd_acoustic_set_volumes(h, None, P(live.ct), P(live.air)), -1, 'bfd_acoustic_set_volumes', 'null', 'labels')
    M = live.labels.shape

    def survey(kw, word, what):
        out = [np.full(256, -7, np.int64), np.full(6, -7, np.int64), np.full(2, -7, np.int64)]
        rc = lib.bfd_acoustic_survey(h, P(kw['lo']), P(kw['hi']), kw['flipK'], *[P(o) for o in out])
        live.refused(rc, -1, 'bfd_acoustic_survey', word, what)
        assert all((o == -7).all() for o in out), what
    good = dict(lo=i64([0, 0, 0]), hi=i64(M), flipK=1)
    _ordered(good, [('lo', i64([-1, 0, 0]), 'box'), ('flipK', 2, 'flipK')], survey)
    _ordered(good, [('hi', i64([M[0] + 1, M[1], M[2]]), 'box'), ('flipK', -1, 'flipK')], survey)
    survey(dict(good, lo=i64([2, 0, 0]), hi=i64([1, M[1], M[2]])), 'box', 'lo > hi')
    three = i64([0, 0, 0])
    assert lib.bfd_acoustic_survey(h, None, P(three), 1, P(three), P(three), P(three)) == -1 and 'null' in lib.bfd_last_error().decode()
    assert live.st.traffic() == before
    # the refusals changed nothing: the resident volumes still answer
    assert np.array_equal(live.st.survey(None, None, True)[0], DM.survey(live.labels)[0])


def test_assemble(live, golden):
    lib, h, before = live.lib, live.h, live.st.traffic()
    entry = 'bfd_acoustic_assemble'

    def assemble(kw, word, what, handle=h):
        stats = np.full(8, -7, np.int64)
        rc = lib.bfd_acoustic_assemble(handle, P(kw['lo']), P(kw['size']), P(kw['padLo']), P(kw['padHi']), kw['flipK'], P(kw['lut']), kw['off'], kw['zWater'],
                                       kw['nMat'], P(kw['focalIJ']), kw['waterOnly'], P(stats))
        live.refused(rc, -1, entry, word, what)
        assert (stats == -7).all(), what
    good = live.assemble_args()
    faults = [('lo', i64([-1, 0, 0]), 'the box'), ('padLo', i64([-1, 0, 0]), 'padding'), ('padHi', i64([2 ** 30, 2 ** 30, 2 ** 30]), 'the map has 2^31'),
              ('flipK', 2, 'flipK'), ('zWater', -2, 'zWater'), ('nMat', -1, 'nMaterials'), ('focalIJ', i64([0, -1]), 'focalIJ'), ('waterOnly', 2, 'waterOnly')]
    _ordered(good, faults, assemble)
    assemble(dict(good, size=i64([0, 0, 0]) + 10 ** 6), 'the box', 'size beyond the volume')
    assemble(dict(good, nMat=2 ** 32), 'nMaterials', 'nMaterials beyond 32 bits')
    empty = dict(good, size=i64([0, 0, 0]), padLo=i64([0, 0, 0]), padHi=i64([0, 0, 0]))
    assemble(dict(empty, waterOnly=2), 'waterOnly', 'waterOnly before the empty map')
    assemble(empty, 'no voxel', 'empty map')
    for name in ('lo', 'size', 'padLo', 'padHi', 'lut', 'focalIJ'):
        assemble(dict(good, **{name: None}), 'null', name)
    assert lib.bfd_acoustic_assemble(h, P(good['lo']), P(good['size']), P(good['padLo']), P(good['padHi']), 1, P(good['lut']), 6, 0, 5, P(good['focalIJ']), 0,
                                     None) == -1
    assert live.st.traffic() == before
    # a table that marks bone is an argument error only for a study without a CT, in its place after flipK
    labels, _, _, rec, kw = _inputs(golden, 'tight_small')
    with AS.AcousticStudy(labels) as other:
        plan = other.plan(rec['SpatialStep'], **kw)
        lo, hi = i64(plan.box_lo), i64(plan.box_hi)
        g2 = dict(lo=lo, size=hi - lo, padLo=i64(plan.pad_lo), padHi=i64(plan.pad_hi), flipK=1, lut=DM.relabel_lut(False, False), off=0,
                  zWater=int(plan.ZSourceLocation), nMat=5, focalIJ=i64(plan.FocalSpotLocation[:2]), waterOnly=0)
        t0 = other.traffic()
        _ordered(g2, [('flipK', 2, 'flipK'), ('lut', DM.relabel_lut(True, False), 'no ct'), ('zWater', -2, 'zWater')],
                 lambda kw_, word, what: assemble(kw_, word, what, other._handle()))
        live.refused(lib.bfd_acoustic_set_volumes(other._handle(), P(labels), P(live.ct), None), -1, 'bfd_acoustic_set_volumes', 'a ct is passed', 'ct for a study without')
        assert other.traffic() == t0
    # the live study's map is what it was
    assert np.array_equal(live.st.fetch('map'), DM.assemble(live.labels, live.plan, live.ct, live.air, len(live.ml))[0])


def test_pack_get_traffic_and_attach(live):
    lib, h, sim = live.lib, live.h, live.st.sim
    before = live.st.traffic()
    crop, plan = live.plan.crop(), live.plan
    kept = [n - a - b for n, a, b in zip(plan.shape, crop.lo, crop.hi)]
    good = dict(slot=0, lo=crop.lo, hi=crop.hi, O=kept, at=(0, 0, 0), flipK=1, correction=1.0)

    def pack(kw, word, what, want=-1, sim_h=None, null_spec=False):
        sp = _engine.pack_spec(kw['lo'], kw['hi'], plan.ZSourceLocation, kw['O'], kw['at'], True, kw['correction'])
        sp.flipK = kw['flipK']
        rc = lib.bfd_acoustic_pack(h, sim.h if sim_h is None else sim_h, None if null_spec else C.byref(sp), kw['slot'])
        live.refused(rc, want, 'bfd_acoustic_pack', word, what)
    faults = [('slot', 3, 'slot'), ('flipK', 2, 'flipK'), ('correction', float('nan'), 'finite'), ('lo', (-1, 0, 0), 'lo / hi'),
              ('O', (kept[0], 0, kept[2]), 'output shape'), ('at', (1, 0, 0), 'offset')]
    _ordered(good, faults, pack)
    pack(dict(good, slot=-1), 'slot', 'slot -1')
    pack(good, 'null', 'null spec', null_spec=True)
    pack(dict(good, at=(0, -1, 0)), 'offset', 'an argument error before the missing run')
    pack(good, 'the run comes first', 'step 0', want=-6)
    other = _engine.Engine(plan.N1 + 1, plan.N2, plan.N3, len(live.ml), live.rec['SpatialStep'], live.dt, FREQ, 20, sensorMode=1)
    try:
        sp = _engine.pack_spec(crop.lo, crop.hi, plan.ZSourceLocation, [kept[0] + 1, kept[1], kept[2]])          # a good spec for THAT sim
        assert lib.bfd_acoustic_pack(h, other.h, C.byref(sp), 0) == -1 and 'shape' in lib.bfd_last_error().decode()
        assert lib.bfd_acoustic_attach(h, other.h) == -1 and 'shape' in lib.bfd_last_error().decode()
    finally:
        other.close()
    assert lib.bfd_acoustic_attach(h, None) == -1 and 'null' in lib.bfd_last_error().decode()

    out = np.full(int(np.prod(plan.shape)), 7, np.uint32)

    def get(which, slot, word, want=-1, ptr=True):
        rc = lib.bfd_acoustic_get(h, which, slot, P(out) if ptr else None)
        live.refused(rc, want, 'bfd_acoustic_get', word, (which, slot))
        assert (out == 7).all()
    get(9, 3, 'null', ptr=False)
    get(9, 3, 'which')
    get(-1, 0, 'which')
    get(0, 3, 'slot')
    get(5, -1, 'slot')
    get(0, 0, 'bfd_acoustic_pack of this slot comes first', want=-6)
    up, down = C.c_int64(-7), C.c_int64(-7)
    assert lib.bfd_acoustic_traffic(h, None, C.byref(down)) == -1 and lib.bfd_acoustic_traffic(h, C.byref(up), None) == -1
    assert (up.value, down.value) == (-7, -7)
    assert live.st.traffic() == before


def test_reflector_device_refusals_and_stages_before_the_volumes(live):
    lib = live.lib
    e = _engine.Engine(32, 32, 40, 1, 1e-3, 1e-7, FREQ, 10)
    try:
        e.set_materials(np.array([H.MATERIALS[FREQ]['Water']], np.float64))
        host = np.zeros(8, np.uint32)
        assert lib.bfd_set_reflector_device(e.h, P(host), -1, 1, 1) == -2 and 'negative strides' in lib.bfd_last_error().decode()
        assert lib.bfd_set_reflector_device(e.h, None, 0, 0, 0) == -6 and 'set the material map first' in lib.bfd_last_error().decode()
        assert lib.bfd_set_reflector_device(e.h, P(host), 1280, 40, 1) == -6                      # no map yet: before the pointer is looked at
    finally:
        e.close()
    # a handle whose volumes were never set: -6 with the stage named, after the argument errors
    h = C.c_void_p()
    assert lib.bfd_acoustic_create(0, 8, 9, 10, 0, 0, C.byref(h)) == 0
    try:
        lo, hi = i64([0, 0, 0]), i64([8, 9, 10])
        outs = [np.full(256, -7, np.int64), np.full(6, -7, np.int64), np.full(2, -7, np.int64)]
        assert lib.bfd_acoustic_survey(h, P(lo), P(hi), 2, *[P(o) for o in outs]) == -1
        assert lib.bfd_acoustic_survey(h, P(lo), P(hi), 1, *[P(o) for o in outs]) == -6
        assert 'bfd_acoustic_set_volumes comes first' in lib.bfd_last_error().decode() and all((o == -7).all() for o in outs)
        zero, stats, lut = i64([0, 0, 0]), np.full(8, -7, np.int64), DM.relabel_lut(False, False)
        args = (P(lo), P(hi), P(zero), P(zero), 1, P(lut), 0, 0, 5, P(i64([1, 1])))
        assert lib.bfd_acoustic_assemble(h, *args, 2, P(stats)) == -1
        assert lib.bfd_acoustic_assemble(h, *args, 0, P(stats)) == -6 and 'bfd_acoustic_set_volumes comes first' in lib.bfd_last_error().decode()
        assert (stats == -7).all()
        assert lib.bfd_acoustic_attach(h, live.st.sim.h) == -6 and 'bfd_acoustic_assemble comes first' in lib.bfd_last_error().decode()
        up, down = C.c_int64(), C.c_int64()
        assert lib.bfd_acoustic_traffic(h, C.byref(up), C.byref(down)) == 0 and (up.value, down.value) == (0, 0)
    finally:
        lib.bfd_acoustic_destroy(h)


def test_two_studies_alive_at_once_and_one_after_a_close(golden):
    a_in, b_in = _inputs(golden, 'segmented_ct_air'), _inputs(golden, 'tight_small')
    want = {}
    for key, (labels, ct, air, rec, kw) in (('a', a_in), ('b', b_in)):
        plan = DM.plan_domain(labels, rec['SpatialStep'], **kw)
        want[key] = (plan, DM.assemble(labels, plan, ct, air, rec['n_materials'] if ct is not None else None))
    a = AS.AcousticStudy(*a_in[:3])
    b = AS.AcousticStudy(*b_in[:3])
    try:
        pa, pb = a.plan(a_in[3]['SpatialStep'], **a_in[4]), b.plan(b_in[3]['SpatialStep'], **b_in[4])       # interleaved: neither disturbs the other
        sb = b.assemble(pb, None)
        sa = a.assemble(pa, a_in[3]['n_materials'])
        assert sa == want['a'][1][3] and sb == want['b'][1][3]
        assert np.array_equal(b.fetch('map'), want['b'][1][0])
        assert np.array_equal(a.fetch('map'), want['a'][1][0]) and np.array_equal(a.fetch('airOut'), want['a'][1][2])
        a.close()
        assert np.array_equal(b.fetch('map'), want['b'][1][0])                                   # the other handle's release took nothing of this one
        with AS.AcousticStudy(*a_in[:3]) as c:                                                      # and a new one after a close
            assert c.assemble(c.plan(a_in[3]['SpatialStep'], **a_in[4]), a_in[3]['n_materials']) == sa
            assert np.array_equal(c.fetch('mapNoCT'), want['a'][1][1])
    finally:
        a.close()
        b.close()
