"""bfd_pack_results (Engine.pack_results) against the numpy restatement of tests/acoustic_oracle.py, applied to what the SAME engine gives
through the separate public calls: sensor_dft(), sensor_index() and get_map(RMS). One engine of 97 x 61 x 155 (no axis a multiple of the 64-wide
tile) runs 80 steps of the skull problem with a sampling plan that captures, once per sensor set, and is then packed many times. Every output
must equal the restatement element by element (tests/util.py::assert_same; complex maps by their real and imaginary parts).

Kept lengths: 1, 2, 63, 64, 65 and 127 .. 130 where the axis has room for them beside the one plane the reference's slicing drops at the high end
(x: up to 96, y: up to 60, z: all of them); each axis also takes its longest, n - 1; the output extents 127 .. 130 are reached on every axis through O larger than the kept region."""
import ctypes as C

import numpy as np
import pytest

from babelbrain_amd import _engine, harness as H
from babelbrain_amd._engine import KIND_RMS
from babelbrain_amd.PropagationModel import compact_sources
from tests import acoustic_oracle as AO
from tests.util import assert_same, oracle_dt

pytestmark = pytest.mark.gpu

N = (97, 61, 155)
STEPS = 80
ONE = np.array([1.0])
CORRECTION = 1.0173
NAMES = ('p_amp', 'p_complex', 'peak')


class Rig:
    def __init__(self):
        a, k, info = H.make_problem('C2', N=N, steps=STEPS, stable_dt_fn=oracle_dt)
        mm, ml, f, smap, pulse, h, T, sensor = a
        self.f, self.zsrc, self.nd, self.sensor = f, info['zsrc'], k['NDelta'], np.ascontiguousarray(sensor)
        e = _engine.Engine(*N, len(ml), h, k['DT'], f, STEPS, NDelta=k['NDelta'], sensorSub=k['SensorSubSampling'], sensorStart=k['SensorStart'],
                           selRMSorPeak=1, selMapsRMS=['Pressure'], selMapsSensors=['Pressure'], sensorMode=1)
        self.e = e
        e.set_materials(ml, k['QCorrection'])
        e.set_material_map(mm, 0, 0)
        lin, row = compact_sources(smap, ONE, ONE, ONE)[:2]
        e.set_sources(lin, row, None, None, np.full(len(lin), 1.0 / (ml[0, 0] * ml[0, 1]), np.float32), np.ascontiguousarray(pulse))
        self.kind = None

    def sensors(self, kind, monkeypatch=None):
        """the run with this sensor set (again only when the set changes)"""
        if kind == self.kind:
            return
        e, nd, z = self.e, self.nd, self.zsrc
        m = self.sensor.copy()
        if kind == 'box call':
            n = e.set_sensor_box((nd, nd, z + 1), (N[0] - 2 * nd, N[1] - 2 * nd, N[2] - nd - z - 1))
        else:
            if kind == 'minus one':
                m[40, 30, 70] = 0
            elif kind == 'scattered':
                rng = np.random.default_rng(3)
                m[:] = 0
                pick = rng.choice(N[0] * N[1] * N[2], 1000, replace=False)
                m.reshape(-1)[pick] = 1
            elif kind == 'half':
                m[:, :, 80:] = 0
            elif kind == 'box as list':
                monkeypatch.setenv('BFD_SENSOR_BOX', '0')
            n = e.set_sensor_map(m)
        assert n == (int(m.sum()) if kind != 'box call' else int(self.sensor.sum()))
        e.reset()
        e.run(STEPS)
        e.sync()
        self.kind = kind
        F, pk = e.sensor_dft(self.f)
        self.F, self.pk, self.index, self.rms = F[0], pk[0], e.sensor_index(), e.get_map(KIND_RMS, 'Pressure')
        assert np.isfinite(self.pk).all() and np.abs(self.F).max() > 0 and self.rms.max() > 0        # the plan captured

    def oracle(self, lo, hi, zsrc, O=None, at=(0, 0, 0), flipK=True, correction=None):
        return dict(zip(NAMES, AO.pack(self.F, self.pk, self.index, self.rms, N, lo, hi, zsrc, O, at, flipK, correction)))

    def close(self):
        self.e.close()


@pytest.fixture(scope='module')
def rig():
    r = Rig()
    yield r
    r.close()


def same(got, ref, what):
    for n in NAMES:
        if n not in ref or n not in got:
            continue
        assert got[n].dtype == ref[n].dtype and got[n].flags['C_CONTIGUOUS'], (what, n)
        if n == 'p_complex':
            assert_same(np.ascontiguousarray(got[n].real), np.ascontiguousarray(ref[n].real), '%s: %s real' % (what, n))
            assert_same(np.ascontiguousarray(got[n].imag), np.ascontiguousarray(ref[n].imag), '%s: %s imag' % (what, n))
        else:
            assert_same(got[n], ref[n], '%s: %s' % (what, n))


def _lengths(n):
    return sorted({L for L in (1, 2, 63, 64, 65, 127, 128, 129, 130) if L <= n - 1} | {n - 1})


def _geometries():
    """(lo, hi) with the wanted kept length on one axis, the others kept short so that a case costs little"""
    base_lo, base_hi = [20, 14, 30], [N[0] - 20 - 9, N[1] - 14 - 5, N[2] - 30 - 40]
    out = []
    for ax in range(3):
        for q, L in enumerate(_lengths(N[ax])):
            lo, hi = list(base_lo), list(base_hi)
            lo[ax] = min(3 + 5 * q, N[ax] - L - 1)
            hi[ax] = N[ax] - lo[ax] - L
            assert hi[ax] >= 1 and N[ax] - lo[ax] - hi[ax] == L
            out.append((ax, L, tuple(lo), tuple(hi)))
    return out


@pytest.mark.parametrize('kind', ['box call', 'production'])
def test_kept_lengths_flips_and_the_source_plane(rig, kind):
    rig.sensors(kind)
    seen = set()
    for ax, L, lo, hi in _geometries():
        kept2 = N[2] - lo[2] - hi[2]
        for flip in (True, False) if kind == 'box call' else (True,):
            zs = (lo[2] - 1, lo[2] + kept2 // 2, lo[2] + kept2 - 1, -1)[(L + ax + flip) % 4]      # below, inside, at the last kept plane (all zero), none
            seen.add((zs < lo[2], zs >= lo[2] + kept2 - 1))
            corr = CORRECTION if (L + flip) % 2 else None
            got = rig.e.pack_results(lo, hi, zs, flipK=flip, correction=corr)
            assert got['p_amp'].shape == tuple(N[a] - lo[a] - hi[a] for a in range(3))
            same(got, rig.oracle(lo, hi, zs, flipK=flip, correction=corr), 'axis %d kept %d flip %d zSource %d scale %s' % (ax, L, flip, zs, corr))
    assert {(True, False), (False, False), (False, True)} <= seen


def test_the_whole_production_region_scaled_and_not(rig):
    rig.sensors('production')
    nd = rig.nd
    lo, hi = (nd, nd, nd), (nd, nd, nd)
    for corr in (CORRECTION, None):
        got = rig.e.pack_results(lo, hi, rig.zsrc, correction=corr)
        ref = rig.oracle(lo, hi, rig.zsrc, correction=corr)
        same(got, ref, 'DataForSim region, correction %s' % corr)
        assert np.count_nonzero(got['p_complex']) > 0 and got['kernel_ms'] > 0
    # without the flag there is no scaling at all, not even the sqrt(2)
    raw = np.flip(rig.rms[nd:-nd, nd:-nd, nd:-nd], axis=2).copy()
    raw[:, :, raw.shape[2] - (rig.zsrc + 1 - nd):] = 0
    assert_same(got['p_amp'], raw, 'unscaled amplitude is the RMS map itself')


@pytest.mark.parametrize('O3', [127, 128, 129, 130])
def test_output_larger_than_the_kept_region(rig, O3):
    """paste_and_flip: O beyond the kept size with at > 0, the output extents around two tiles on every axis"""
    rig.sensors('production')
    lo, hi = (15, 13, 40), (N[0] - 15 - 70, N[1] - 13 - 33, N[2] - 40 - 100)
    for O, at in (((O3, 40, 101), (O3 - 71, 3, 1)), ((71, O3, 130), (1, O3 - 33, 17)), ((80, 35, O3), (5, 0, O3 - 100))):
        for flip in (True, False):
            got = rig.e.pack_results(lo, hi, 55, O=O, at=at, flipK=flip, correction=CORRECTION)
            assert got['peak'].shape == O
            same(got, rig.oracle(lo, hi, 55, O=O, at=at, flipK=flip, correction=CORRECTION), 'O %s at %s flip %d' % (O, at, flip))


def test_every_output_null_in_turn_and_repeats_give_the_same_bytes(rig):
    rig.sensors('production')
    lo, hi = (12, 12, 12), (20, 13, 14)
    full = rig.e.pack_results(lo, hi, rig.zsrc, correction=CORRECTION)
    again = rig.e.pack_results(lo, hi, rig.zsrc, correction=CORRECTION)
    for n in NAMES:
        assert full[n].tobytes() == again[n].tobytes(), n
    for drop in NAMES:
        want = tuple(n for n in NAMES if n != drop)
        got = rig.e.pack_results(lo, hi, rig.zsrc, correction=CORRECTION, want=want)
        assert drop not in got
        for n in want:
            assert got[n].tobytes() == full[n].tobytes(), (drop, n)
    none = rig.e.pack_results(lo, hi, rig.zsrc, correction=CORRECTION, want=())
    assert none == {'kernel_ms': 0.0}


@pytest.mark.parametrize('kind', ['minus one', 'scattered', 'half'])
def test_other_sensor_sets(rig, kind):
    """the box minus one voxel and 1000 scattered sensors take the list path; a box over half the kept region is a box again"""
    rig.sensors(kind)
    nd = rig.nd
    for lo, hi, O, at, flip in (((nd, nd, nd), (nd, nd, nd), None, (0, 0, 0), True), ((30, 20, 60), (25, 15, 31), (50, 30, 70), (4, 2, 3), False)):
        for corr in (CORRECTION, None):
            got = rig.e.pack_results(lo, hi, rig.zsrc, O=O, at=at, flipK=flip, correction=corr)
            same(got, rig.oracle(lo, hi, rig.zsrc, O=O, at=at, flipK=flip, correction=corr), '%s, lo %s' % (kind, lo))
    n = np.count_nonzero(rig.e.pack_results((0, 0, 0), (1, 1, 1), -1)['peak'])
    assert n <= rig.e.num_sensors and (kind == 'scattered' or n > 0)


def test_box_path_and_list_path_give_identical_bytes_on_the_box(rig, monkeypatch):
    lo, hi = (12, 12, 12), (12, 12, 12)
    packs = {}
    for kind in ('production', 'box call', 'box as list'):
        rig.sensors(kind, monkeypatch)
        packs[kind] = [rig.e.pack_results(lo, hi, rig.zsrc, correction=CORRECTION),
                       rig.e.pack_results((30, 20, 60), (25, 15, 31), 70, O=(50, 30, 70), at=(4, 2, 3), flipK=False)]
    monkeypatch.delenv('BFD_SENSOR_BOX')
    rig.kind = None                                                     # the next test sets its sensors again, as a box
    for kind in ('box as list', 'box call'):
        for a, b in zip(packs[kind], packs['production']):
            for n in NAMES:
                assert a[n].tobytes() == b[n].tobytes(), (kind, n)


def test_refusals_in_the_header_s_order_write_nothing(rig):
    rig.sensors('production')
    e = rig.e
    good = dict(lo=(12, 12, 12), hi=(12, 12, 12), zSource=12, O=(73, 37, 131), at=(0, 0, 0), flipK=1, applyScale=1, ampScale=1.4, correction=1.0)
    faults = [('flipK', 2, 'flipK'), ('applyScale', -1, 'flipK'), ('ampScale', float('nan'), 'finite'), ('correction', float('inf'), 'finite'),
              ('lo', (-1, 12, 12), 'lo / hi'), ('hi', (12, 49, 12), 'lo / hi'), ('O', (73, 0, 131), 'output shape'), ('O', (2 ** 11, 2 ** 10, 2 ** 10), 'output shape'),
              ('at', (0, -1, 0), 'offset'), ('at', (1, 0, 0), 'offset')]

    def call(kw, null_spec=False):
        sp = _engine.PackSpec((C.c_int32 * 3)(*kw['lo']), (C.c_int32 * 3)(*kw['hi']), kw['zSource'], (C.c_int32 * 3)(*kw['O']), (C.c_int32 * 3)(*kw['at']),
                              kw['flipK'], kw['applyScale'], kw['ampScale'], kw['correction'])
        n = int(np.prod(good['O']))
        out = [np.full(c * n, 7.0, np.float32) for c in (1, 2, 1)]
        ms = C.c_float(-5.0)
        rc = e.lib.bfd_pack_results(e.h, None if null_spec else C.byref(sp), *[o.ctypes.data_as(C.c_void_p) for o in out], C.byref(ms))
        assert all((o == 7.0).all() for o in out) and ms.value == -5.0
        return rc, e.lib.bfd_last_error().decode()

    assert call(good, null_spec=True)[0] == -1
    for q, (name, value, word) in enumerate(faults):
        kw = dict(good)
        for later, v, _ in faults[q:][::-1]:                            # this fault and every later one planted: the first is reported
            kw[later] = v
        kw[name] = value
        rc, text = call(kw)
        assert rc == -1 and word in text, (name, text)
    # the engine is as it was
    got = e.pack_results((12, 12, 12), (12, 12, 12), rig.zsrc, correction=CORRECTION)
    same(got, rig.oracle((12, 12, 12), (12, 12, 12), rig.zsrc, correction=CORRECTION), 'after the refusals')


def test_denormal_values_are_scaled_as_numpy_scales_them(rig):
    """Factors so small that the float32 factor itself (1e-41) or the products (1e-43) are denormal: numpy on a CPU keeps denormal operands and
    results of the float32 scaling; the device would flush both in a float32 instruction, so the product is formed another way (bfd_pack_core.h)."""
    rig.sensors('production')
    lo, hi = (12, 12, 12), (12, 12, 12)
    tiny = np.float32(1.1754944e-38)
    for corr in (1e-41, 1e-43):
        assert 0 < np.float32(corr) < tiny
        ref = rig.oracle(lo, hi, rig.zsrc, correction=corr)
        parts = np.concatenate([ref['p_complex'].real.reshape(-1), ref['p_complex'].imag.reshape(-1), ref['peak'].reshape(-1), ref['p_amp'].reshape(-1)])
        n_denormal = int(np.count_nonzero((parts != 0) & (np.abs(parts) < tiny)))
        assert n_denormal > 1000 and np.count_nonzero(ref['p_complex']) > 1000, (corr, n_denormal)
        same(rig.e.pack_results(lo, hi, rig.zsrc, correction=corr), ref, 'correction %g' % corr)
