"""The domain setup without a GPU: the literal numpy restatement (tests/domain_oracle.py) against what the reference's own UpdateConditions and
compute_sdr_from_rays produced (tests/golden/domain_golden.npz); Domain.plan_domain's separable cone against the restatement's 3-D cone, with survey
replaced by numpy; the table of relabels against the sequential statements; bfd_domain_core.h, compiled for the host, against numpy's rounding;
planted faults the restatement must see; Domain raises what it says it raises before the library is loaded."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from babelbrain_amd import Domain as DM, _engine
from tests import domain_oracle as DO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PLAN_KEYS = list(DO.DEFAULTS) + ['FocalLength', 'Aperture']
with open(os.path.join(GOLDEN, 'domain_golden.json')) as _fh:
    META = json.load(_fh)
CASES = sorted(META['cases'])


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'domain_golden.npz'))


@pytest.fixture
def numpy_survey(monkeypatch):
    """Domain.survey answered by the restatement: no device"""
    calls = []

    def survey(labels, box=None, flip_k=True):
        calls.append(box)
        return DO.survey(labels, box, flip_k)
    monkeypatch.setattr(DM, 'survey', survey)
    return calls


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """The library is out of reach: its path names a missing file and loading it is an error. The refusals below must come first."""
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_engine, 'LIB_PATH', str(tmp_path / 'no_such_library.so'))
    monkeypatch.setattr(_engine, '_lib', None)
    monkeypatch.setattr(_engine, 'load_library', boom)


def params(rec):
    return {k: rec[k] for k in PLAN_KEYS}


# ---------------------------------------------------------------- the restatement against the reference's results ----------------------------------------------------------------

def test_the_cases_cover_what_they_should():
    c = META['cases']
    assert {c[n]['bTightNarrowBeamDomain'] for n in c} == {True, False}
    assert any(len(c[n]['ExtraAdjustX']) == 2 for n in c) and any(c[n]['TxMechanicalAdjustmentX'] != 0 for n in c)
    assert any(c[n]['FocalLength'] == 0 for n in c) and any(c[n]['ZIntoSkin'] > 0 for n in c)
    assert any(c[n]['XLOffset'] > 12 for n in c) and any(c[n]['XShrink_L'] > 0 for n in c)
    assert {(c[n]['segmented'], c[n]['ct'] is not None) for n in c} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(c[n]['air'] for n in c) and any(c[n]['ct'] and not c[n]['air'] for n in c)
    t = c['tight_small']
    assert [t[f] for f in ('N1', 'N2', 'N3')] == [73, 73, 72] and [t[f] for f in ('XShrink_L', 'YShrink_L', 'ZShrink_L')] == [6, 4, 11]
    assert [t[f] for f in ('XShrink_R', 'YShrink_R', 'ZShrink_R')] == [5, 3, 11]
    assert os.path.getsize(os.path.join(GOLDEN, 'domain_golden.npz')) < os.path.getsize(os.path.join(GOLDEN, 'harness_golden.npz'))


@pytest.mark.parametrize('name', CASES)
def test_restatement_equals_the_golden(golden, name):
    rec = META['cases'][name]
    labels = golden[name + '_labels']
    assert np.array_equal(labels, DO.head(rec['shape'], rec['segmented']))
    o = DO.plan(labels, rec['SpatialStep'], **params(rec))
    for f in DO.PLAN_FIELDS[:-1]:
        assert getattr(o, f) == rec[f], f
    for f in ('XDim', 'YDim', 'ZDim', 'FocalSpotLocation'):
        assert np.array_equal(getattr(o, f), golden[name + '_' + f]), f
    assert list(o.box_hi) == [u if u > 0 else s + u for u, s in zip(rec['upper'], rec['shape'])]
    ct = golden[name + '_ct'] if rec['ct'] else None
    air = golden[name + '_air'] if rec['air'] else None
    m, noct, sub_air, stats = DO.assemble(labels, o, ct, air, rec['n_materials'])
    assert np.array_equal(m, golden[name + '_MaterialMap'])
    zoom = rec['SpatialStep'] * 1e3
    assert stats['first_k'] * zoom / 1e3 - stats['first_k_focal'] * zoom / 1e3 == rec['DomainZReference']
    if ct is not None:
        assert np.array_equal(noct, golden[name + '_MaterialMapNoCT'])
        assert air is None or np.array_equal(sub_air, golden[name + '_SubAirRegions'])
        assert stats['ct_min'] >= 3 and stats['ct_max'] <= rec['n_materials'] and stats['bone_voxels'] > 1000
        hu = golden['UniqueHU']
        assert DO.sdr(ct, hu, o, zoom) == golden[name + '_sdr'][0]
        assert DO.sdr(ct, hu, o, zoom, 0.8, 2, 0.75) == golden[name + '_sdr'][1]


def test_restatement_sees_planted_faults(golden):
    name = 'segmented_ct_air'
    rec = META['cases'][name]
    labels, ct, air = golden[name + '_labels'], golden[name + '_ct'], golden[name + '_air']
    o = DO.plan(labels, rec['SpatialStep'], **params(rec))
    for fault, key in (('water_short', '_MaterialMap'), ('offset3', '_MaterialMap'), ('noct_late', '_MaterialMapNoCT')):
        m, noct, _, _ = DO.assemble(labels, o, ct, air, rec['n_materials'], fault=fault)
        got = m if key == '_MaterialMap' else noct
        assert not np.array_equal(got, golden[name + key]), fault
    # half away from zero in the segment: the counts 2 mod 4 are the exact halves at centre region 0.5
    assert DO.segment(6, 0.5) == (2, 5) and DO.segment(6, 0.5, away=True) == (2, 6 - 1)
    assert DO.segment(10, 0.5) == (2, 9) and DO.segment(10, 0.5, away=True) == (3, 9)
    box = (o.box_lo, o.box_hi)
    good = DO.sdr_rays(ct, golden['UniqueHU'], box, 2, 2, 2, 0.5, True)
    bad = DO.sdr_rays(ct, golden['UniqueHU'], box, 2, 2, 2, 0.5, True, away=True)
    assert np.array_equal(good[2], bad[2]) and not np.array_equal(good[0], bad[0])


# ---------------------------------------------------------------- the separable plan ----------------------------------------------------------------

def same_plan(p, o):
    for f in DO.PLAN_FIELDS:
        assert getattr(p, f) == getattr(o, f), (f, getattr(p, f), getattr(o, f))
    for f in ('XDim', 'YDim', 'ZDim', 'FocalSpotLocation'):
        assert np.array_equal(getattr(p, f), getattr(o, f)), f
    A, Z = p.region_sets()
    assert A.shape == p.shape[:2] and Z.shape == p.shape[2:]
    assert np.array_equal(A[:, :, None] & Z[None, None, :], o.RegionMap)
    assert tuple(p.box_lo) == tuple(o.box_lo) and tuple(p.box_hi) == tuple(o.box_hi)


@pytest.mark.parametrize('name', CASES)
def test_plan_equals_the_literal_cone_on_the_golden_cases(golden, numpy_survey, name):
    rec = META['cases'][name]
    labels = golden[name + '_labels']
    p = DM.plan_domain(labels, rec['SpatialStep'], **params(rec))
    same_plan(p, DO.plan(labels, rec['SpatialStep'], **params(rec)))
    assert len(numpy_survey) == 2                                            # one survey per pass, on the crop in force
    assert numpy_survey[0] == ([0, 0, 0], list(labels.shape)) and numpy_survey[1] == (list(p.box_lo), list(p.box_hi))
    crop = p.crop()
    assert crop.lo == p.pad_lo and crop.hi == p.pad_hi and crop.shrink == tuple(p.box_lo)
    T, nt, sub, start = p.time_plan(rec['TemporalStep'], int(rec['PPP']), 1500.0)
    assert (T, sub, start) == (rec['TimeSimulation'], rec['SensorSubSampling'], rec['SensorStart'])
    q = DM.plan_domain(labels.astype(np.float64), rec['SpatialStep'], **params(rec))        # get_fdata hands float64
    assert q.shape == p.shape and q.box_lo == p.box_lo


def test_plan_equals_the_literal_cone_on_random_parameters(numpy_survey):
    rng = np.random.default_rng(11)
    h = 1102.515 / 500e3 / 6
    done = raised = 0
    for n in range(40):
        shape = (int(rng.integers(24, 40)), int(rng.integers(24, 40)), int(rng.integers(36, 52)))
        flip = bool(n % 2)
        labels = DO.head(shape, segmented=bool(n % 3 == 0), flipped=flip)
        kw = dict(FocalLength=float(rng.choice([0.0, 20e-3, 35e-3, 63.2e-3])), Aperture=float(rng.uniform(8e-3, 40e-3)),
                  PMLThickness=int(rng.integers(4, 13)), ZIntoSkin=float(rng.uniform(0, 2e-3)), TxMechanicalAdjustmentX=float(rng.normal(0, 1e-3)),
                  TxMechanicalAdjustmentY=float(rng.normal(0, 1e-3)), TxMechanicalAdjustmentZ=float(rng.normal(0, 2e-3)),
                  ExtraDepthAdjust=float(rng.uniform(0, 2e-3)), ExtraAdjustX=[0.0] + [float(x) for x in rng.normal(0, 3e-3, n % 3)],
                  ExtraAdjustY=[0.0] + [float(x) for x in rng.normal(0, 3e-3, n % 3)], PaddingForRayleigh=int(rng.integers(0, 3)),
                  PaddingForKArray=int(rng.integers(0, 3)), ZTxCorrecton=float(rng.uniform(0, 1e-3)), bTightNarrowBeamDomain=bool(rng.integers(0, 2)),
                  zLengthBeyonFocalPointWhenNarrow=float(rng.uniform(2e-3, 12e-3)))
        try:
            o = DO.plan(labels, h, flip_k=flip, **kw)
        except (ValueError, IndexError) as e:
            with pytest.raises(type(e)):
                DM.plan_domain(labels, h, flip_k=flip, **kw)
            raised += 1
            continue
        same_plan(DM.plan_domain(labels, h, flip_k=flip, **kw), o)
        done += 1
    assert done >= 25, (done, raised)


def test_plan_raises_where_the_reference_does(numpy_survey):
    h = 1102.515 / 500e3 / 6
    labels = DO.head((30, 28, 40))
    kw = dict(FocalLength=35e-3, Aperture=30e-3)
    two = labels.copy()
    two[0, 0, 0] = 5
    for bad in (two, np.where(labels == 5, 4, labels).astype(np.uint8)):
        with pytest.raises(ValueError, match='exactly one'):
            DM.plan_domain(bad, h, **kw)
        with pytest.raises(ValueError):
            DO.plan(bad, h, **kw)
    with pytest.raises(ValueError, match='no tissue'):
        DM.plan_domain(np.zeros_like(labels), h, **kw)
    with pytest.raises(ValueError, match='ExtraAdjust'):
        DM.plan_domain(labels, h, ExtraAdjustX=[], ExtraAdjustY=[], **kw)
    with pytest.raises(NotImplementedError):
        DM.plan_domain(labels, h, DomeType=True, **kw)
    # an empty cone: a bound is read only on the tight path, as in the reference
    empty = dict(FocalLength=35e-3, Aperture=80e-3)                     # arcsin of more than 1: no radius, no cone
    assert DM.plan_domain(labels, h, **empty).region_count == 0 and DO.plan(labels, h, **empty).region_count == 0
    with pytest.raises(ValueError, match='cone'):
        DM.plan_domain(labels, h, bTightNarrowBeamDomain=True, **empty)
    with pytest.raises(ValueError):
        DO.plan(labels, h, bTightNarrowBeamDomain=True, **empty)


# ---------------------------------------------------------------- the table of relabels ----------------------------------------------------------------

@pytest.mark.parametrize('ct', [True, False])
@pytest.mark.parametrize('seg', [True, False])
def test_lut_equals_the_sequential_statements(ct, seg):
    raw = np.arange(256, dtype=np.uint32).reshape(4, 8, 8)
    want = DO.relabel(raw.copy(), ct, seg)
    lut = DM.relabel_lut(ct, seg)
    assert lut.dtype == np.uint32 and lut.shape == (256,)
    bone = (lut >> 31).astype(bool)
    assert np.array_equal(np.flatnonzero(bone), [2, 3] if ct else [])
    assert np.array_equal((lut & np.uint32(0x7FFFFFFF))[raw], want)
    assert lut[0] == 0 and lut[1] == 1


# ---------------------------------------------------------------- bfd_domain_core.h on the host ----------------------------------------------------------------

CORE_PROGRAM = r"""
#include "bfd_domain_core.h"
#include <stdio.h>
#include <stdlib.h>
// argv: counts up to n, centre region  ->  beg end per count 1 .. n, as text
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const int n = atoi(argv[1]);
    const double cr = atof(argv[2]);
    for (int c = 1; c <= n; c++) {
        int b, e;
        dm_segment(c, cr, &b, &e);
        printf("%d %d\n", b, e);
    }
    for (int64_t k = 0; k < 5; k++)
        if (dm_source_k(k, 5, 1) != 4 - k || dm_source_k(k, 5, 0) != k) return 3;
    return 0;
}
"""


@pytest.fixture(scope='module')
def core(tmp_path_factory):
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx, 'no C++ compiler found'
    d = tmp_path_factory.mktemp('domaincore')
    src = d / 'domaincore.cpp'
    src.write_text(CORE_PROGRAM)
    exe = str(d / 'domaincore')
    subprocess.run([cxx, '-O1', '-ffp-contract=off', '-I', os.path.join(os.path.dirname(_engine.LIB_PATH), 'csrc'), str(src), '-o', exe, '-lm'], check=True)

    def segments(n, cr):
        out = subprocess.run([exe, str(n), repr(float(cr))], check=True, capture_output=True, text=True).stdout
        return np.array(out.split(), np.int64).reshape(n, 2)
    return segments


@pytest.mark.parametrize('cr', [0.25, 0.5, 0.75, 1.0, 0.0, 0.3, 2.5])
def test_core_segment_equals_numpy_for_every_count(core, cr):
    got = core(2000, cr)
    want = np.array([DO.segment(c, cr) for c in range(1, 2001)])
    assert np.array_equal(got, want)
    if cr == 0.5:                                                            # counts 2 mod 4: mid - count / 4 ends in .5, resolved to even
        away = np.array([DO.segment(c, cr, away=True) for c in range(1, 2001)])
        differ = np.flatnonzero(np.any(away != want, axis=1)) + 1
        assert differ.size > 400 and np.all(differ % 4 == 2)


# ---------------------------------------------------------------- refusals ----------------------------------------------------------------

def test_python_refuses_before_the_library(no_library):
    vol = np.zeros((3, 4, 5), np.uint8)
    vol[1, 1, 1] = 5
    with pytest.raises(ValueError, match='3-D'):
        DM.survey(vol[0])
    for bad in (vol.astype(np.float32) + 0.5, vol.astype(np.int32) - 1, vol.astype(np.int32) + 300, np.full((3, 4, 5), np.nan), vol.astype(complex)):
        with pytest.raises(ValueError):
            DM.survey(bad)
    for box in (([0, 0, 0], [3, 4, 6]), ([2, 0, 0], [1, 4, 5]), ([-1, 0, 0], [3, 4, 5]), ([0, 0], [3, 4]), 'box'):
        with pytest.raises(ValueError, match='box'):
            DM.survey(vol, box)
    with pytest.raises(NotImplementedError):
        DM.plan_domain(vol, 1e-3, FocalLength=0.05, Aperture=0.05, DomeType=True)
    for kw in (dict(PMLThickness=0), dict(ExtraAdjustX=[]), dict(ExtraAdjustY=())):
        with pytest.raises(ValueError):
            DM.plan_domain(vol, 1e-3, FocalLength=0.05, Aperture=0.05, **kw)
    with pytest.raises(ValueError, match='SpatialStep'):
        DM.plan_domain(vol, 0.0, FocalLength=0.05, Aperture=0.05)
    plan = DM.DomainPlan(N1=5, N2=6, N3=7, XLOffset=1, YLOffset=1, ZLOffset=1, XROffset=1, YROffset=1, ZROffset=1, box_lo=(0, 0, 0), box_hi=(3, 4, 5),
                         mask_shape=(3, 4, 5), flip_k=True, FocalSpotLocation=np.array([2, 2, 2]), ZSourceLocation=1)
    with pytest.raises(ValueError, match='plan was made'):
        DM.assemble(np.zeros((3, 4, 6), np.uint8), plan)
    with pytest.raises(ValueError, match='ct_index'):
        DM.assemble(vol, plan, ct_index=np.zeros((3, 4, 6), np.uint32))
    with pytest.raises(ValueError, match='ct_index'):
        DM.assemble(vol, plan, ct_index=vol.astype(np.float64) - 1)
    with pytest.raises(ValueError, match='air'):
        DM.assemble(vol, plan, ct_index=vol.astype(np.uint16), air=np.zeros((3, 4, 6), bool))
    with pytest.raises(ValueError, match='n_materials'):
        DM.assemble(vol, plan, n_materials=-1)
    w = DM.assemble(vol, plan, water_only=True)
    assert w[0].shape == (5, 6, 7) and w[0].dtype == np.uint32 and not w[0].any() and w[1:] == (None, None, None)
    ct, hu = vol.astype(np.uint32), np.linspace(0, 100, 8).astype(np.float32)
    for kw in (dict(step_i=0), dict(step_j=1.5), dict(min_skull_voxels=0), dict(center_region=-1), dict(center_region=np.nan)):
        with pytest.raises(ValueError):
            DM.sdr_rays(ct, hu, None, **dict(dict(step_i=1, step_j=1), **kw))
    for bad in (hu.reshape(2, 4), hu[:0], np.array([1, np.inf], np.float32)):
        with pytest.raises(ValueError, match='UniqueHU'):
            DM.sdr_rays(ct, bad, None, 1, 1)
    with pytest.raises(ValueError, match='spacing_mm'):
        DM.skull_density_ratio(ct, hu, plan, 0.0)
    for call in (lambda: DM.survey(vol), lambda: DM.survey(vol.astype(np.float64), ([0, 1, 2], [3, 4, 5]), False), lambda: DM.assemble(vol, plan),
                 lambda: DM.sdr_rays(ct, hu, None, 1, 2), lambda: DM.skull_density_ratio(ct.astype(np.int64), hu.astype(np.float64), plan, (0.4, 0.4)),
                 lambda: DM.plan_domain(vol, 1e-3, FocalLength=0.05, Aperture=0.05)):
        with pytest.raises(AssertionError, match='library was loaded'):        # a good call gets as far as the library
            call()


def test_init_domain_picks_its_own_device(monkeypatch):
    from babelbrain_amd import TissueMask as TM
    monkeypatch.setattr(DM, '_device', 0)
    monkeypatch.setattr(DM._step1, 'pick_device', lambda name, current: ([(0, 'a'), (5, 'b')], 5))
    assert DM.InitDomain('b') == [(0, 'a'), (5, 'b')] and DM._device == 5 and TM._device == 0
