"""The acoustic study (babelbrain_amd/AcousticStudy.py, csrc/bfd_acoustic.hip) against the same work by separate public calls. On the ten cases of
tests/golden/domain_golden.npz the study's plan equals Domain.plan_domain and its resident maps, air mask and stats equal Domain.assemble. One
phantom, without and with CT and air, goes through acoustic_field and through Domain.* / Engine with host setters / sensor_dft / phase_maps / the
reference's scaling statements / results.data_for_sim: every entry of both DataForSim dicts (tissue and water) must be equal, dtypes included. The
bytes that crossed the host boundary are derived here from the shapes and asserted exactly."""
import json
import os

import numpy as np
import pytest

from babelbrain_amd import AcousticStudy as AS, Domain as DM, _engine, harness as H, results as R, sources
from babelbrain_amd._engine import KIND_RMS
from babelbrain_amd.PropagationModel import compact_sources
from tests import acoustic_oracle as AO, domain_oracle as DO

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PLAN_KEYS = list(DO.DEFAULTS) + ['FocalLength', 'Aperture']
CASES = ['tight_small', 'tight_large', 'loose', 'two_adjusts', 'flat', 'grows', 'segmented', 'ct', 'segmented_ct_air', 'loose_ct_air']
FREQ = 500e3
STEPS = 100
SURVEY_UP, SURVEY_DOWN = 24 + 4, 257 * 8 + 24 + 4                    # the bounds and focal words out; histogram, bounds and focal word back
ASSEMBLE_UP, ASSEMBLE_DOWN = 256 * 4 + 24 + 20, 24 + 20               # the table and the two blocks of counters out; the counters back


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(GOLDEN, 'domain_golden.json')) as fh:
        meta = json.load(fh)
    return np.load(os.path.join(GOLDEN, 'domain_golden.npz')), meta


def _inputs(golden, name):
    g, meta = golden
    rec = meta['cases'][name]
    labels = g[name + '_labels']
    ct = g[name + '_ct'] if rec['ct'] else None
    air = g[name + '_air'] if rec['air'] else None
    return labels, ct, air, rec, {k: rec[k] for k in PLAN_KEYS}


def _same_plan(a, b):
    assert sorted(a.__dict__) == sorted(b.__dict__)
    for k, v in b.__dict__.items():
        w = a.__dict__[k]
        if isinstance(v, np.ndarray):
            assert w.dtype == v.dtype and np.array_equal(w, v), k
        else:
            assert type(w) is type(v) and w == v, k


@pytest.mark.parametrize('name', CASES)
def test_plan_and_assemble_equal_the_separate_calls(golden, name):
    labels, ct, air, rec, kw = _inputs(golden, name)
    plan = DM.plan_domain(labels, rec['SpatialStep'], **kw)
    nMat = rec['n_materials'] if ct is not None else None
    m, noct, sub_air, stats = DM.assemble(labels, plan, ct, air, nMat)
    with AS.AcousticStudy(labels, ct, air) as st:
        with pytest.raises(_engine.EngineError, match=r'rc=-6.*bfd_acoustic_assemble comes first'):
            st.plan_ = plan
            st.fetch('map')
        st.plan_ = None
        got = st.plan(rec['SpatialStep'], **kw)
        _same_plan(got, plan)
        assert st.assemble(got, nMat) == stats
        fm = st.fetch('map')
        assert fm.dtype == np.uint32 and fm.shape == plan.shape and np.array_equal(fm, m)
        if ct is not None:
            assert np.array_equal(st.fetch('mapNoCT'), noct)
        else:
            with pytest.raises(_engine.EngineError, match=r'rc=-6'):
                st.fetch('mapNoCT')
        if air is not None:
            assert np.array_equal(st.fetch('airOut'), sub_air)
        else:
            with pytest.raises(_engine.EngineError, match=r'rc=-6'):
                st.fetch('airOut')
        n = labels.size
        surveys = 2 + 1 + (ct is not None)
        fetched = 4 * m.size * (1 + (ct is not None) + (air is not None))
        up = n + (ct.nbytes if ct is not None else 0) + (n if air is not None else 0) + surveys * SURVEY_UP + ASSEMBLE_UP
        assert st.traffic() == (up, surveys * SURVEY_DOWN + ASSEMBLE_DOWN + fetched)
        assert st.assemble(got, nMat, water_only=True) is None                      # formed on the device: nothing crosses
        assert not st.fetch('map').any()
        assert st.traffic() == (up, surveys * SURVEY_DOWN + ASSEMBLE_DOWN + fetched + 4 * m.size)


# ---------------------------------------------------------------- the whole flow ----------------------------------------------------------------

def _materials(n):
    """n rows: water, skin, brain, then bone of rising speed (a CT's rows)"""
    t = H.MATERIALS[FREQ]
    ml = np.tile(np.array(t['Cortical'], np.float64), (n, 1))
    ml[0], ml[1], ml[2] = t['Water'], t['Skin'], t['Brain']
    ml[3:, 1] += 1.0 * np.arange(n - 3)
    return ml


def _plane(plan):
    return H.source_plane(H.CONFIGS['C2']['tx'], plan.N1, plan.N2, plan.SpatialStep, FREQ)


def _separate_calls(labels, ct, air, rec, kw, ml):
    """the flow of acoustic_field through the public calls that exist without it"""
    h = rec['SpatialStep']
    plan = DM.plan_domain(labels, h, **kw)
    m, noct, sub_air, stats = DM.assemble(labels, plan, ct, air, len(ml))
    dt_ideal = _engine.stable_dt(ml, FREQ, True, h, H.ALPHA_CFL, 1.0)
    dt_water = _engine.stable_dt(ml[:1], FREQ, True, h, 1.0)
    ppp, dt = H.ppp_rule(dt_ideal, FREQ)
    _, _, sub, _ = plan.time_plan(dt, ppp, ml[0, 1])
    nt, T = STEPS, STEPS * dt
    start = max(int((nt - H.CYCLES_TO_TRACK * ppp) / sub), 0)
    correction = H.dispersion_correction(dt, dt_water)
    N1, N2, N3 = plan.shape
    zsrc, pml = int(plan.ZSourceLocation), plan.PMLThickness
    e = _engine.Engine(N1, N2, N3, len(ml), h, dt, FREQ, nt, NDelta=pml, sensorSub=sub, sensorStart=start, selRMSorPeak=1, selMapsRMS=['Pressure'],
                       selMapsSensors=['Pressure'], sensorMode=1)
    out = {}
    try:
        e.set_materials(ml, 1.0)
        e.set_material_map(m, 0, 0)
        if sub_air is not None:
            e.set_reflector(sub_air)
        plane = _plane(plan)
        smap, src = H.cw_pulse_sources(plane, FREQ, dt, T, N3, zsrc)
        lin, row, wx, wy, wz = compact_sources(smap, np.array([0.0]), np.array([0.0]), np.array([1.0 / (ml[0, 0] * ml[0, 1])]))[:5]
        e.set_sources(lin, row, wx, wy, wz, src)
        assert e.set_sensor_map(H.sensor_maps(N1, N2, N3, zsrc, pml)[0]) > 0
        for which in ('tissue', 'water'):
            if which == 'water':
                e.set_material_map(np.zeros(plan.shape, np.uint32), 0, 0)
                e.reset()
            e.run(nt)
            e.sync()
            F, pk = e.sensor_dft(FREQ)
            four, _, _ = H.phase_maps(F[0], pk[0], e.sensor_index(), N1, N2, N3)
            rms = e.get_map(KIND_RMS, 'Pressure')
            AO.scale_amp(rms, correction)                                        # BASE:2440: the factor a float64 scalar
            AO.scale_sensor(four, correction)                                    # BASE:2517-2520 with the factor folded in: c64 *= python float
            if which == 'tissue':
                d = R.data_for_sim(plan.crop(), zsrc, rms, four, noct if ct is not None else m, plan.FocalSpotLocation, ml, plan.XDim, plan.YDim, plan.ZDim,
                                   h, 4e-2, MaterialMapCT=m if ct is not None else None, AirMask=sub_air)
            else:
                d = R.data_for_sim(plan.crop(), zsrc, rms, four, np.zeros(plan.shape, np.uint32), plan.FocalSpotLocation, ml, plan.XDim, plan.YDim, plan.ZDim,
                                   h, 4e-2)
            out[which] = d
    finally:
        e.close()
    n_src = int(np.count_nonzero(np.abs(plane) > 0))
    return out, plan, stats, correction, n_src, len(sources.cw_time(FREQ, dt, T))


def _same_dict(got, ref, what):
    assert sorted(got) == sorted(ref), (what, sorted(got), sorted(ref))
    for k, v in ref.items():
        w = got[k]
        if isinstance(v, np.ndarray):
            assert isinstance(w, np.ndarray) and w.dtype == v.dtype and w.shape == v.shape, (what, k, getattr(w, 'dtype', None), v.dtype)
            assert np.isfinite(v).all() if v.dtype.kind in 'fc' else True, (what, k)
            assert np.array_equal(w, v), (what, k, int(np.count_nonzero(w != v)))
        else:
            assert type(w) is type(v) and w == v, (what, k)


@pytest.mark.parametrize('name', ['tight_small', 'segmented_ct_air'])
def test_acoustic_field_equals_the_flow_by_separate_calls(golden, name):
    labels, ct, air, rec, kw = _inputs(golden, name)
    ml = _materials(rec['n_materials'] if ct is not None else 5)
    ref, plan, stats, correction, n_src, nT = _separate_calls(labels, ct, air, rec, kw, ml)
    got = AS.acoustic_field(labels, ml, FREQ, rec['SpatialStep'], _plane, kw, ct_index=ct, air=air, QCorrection=1.0, steps=STEPS)
    _same_plan(got['plan'], plan)
    assert got['stats'] == stats and got['correction'] == correction and got['nt'] == STEPS
    assert np.abs(ref['tissue']['p_complex']).max() > 0 and ref['tissue']['p_amp'].max() > 0 and ref['water']['p_amp'].max() > 0
    assert not np.array_equal(ref['tissue']['p_amp'], ref['water']['p_amp'])
    assert ('MaterialMapCT' in ref['tissue']) == (ct is not None) and ('AirMask' in ref['tissue']) == (air is not None)
    _same_dict(got['tissue'], ref['tissue'], name + ' tissue')
    _same_dict(got['water'], ref['water'], name + ' water')
    # traffic, from the shapes: the volumes once, the words of four (five with a CT) surveys and one assembly, the table and lists handed to the engine
    n = labels.size
    surveys = 2 + 1 + (ct is not None)
    handed = ml.nbytes + 8 * len(ml) + 20 * n_src + 4 * 2 * n_src + 4 * 2 * nT
    up = n + (ct.nbytes if ct is not None else 0) + (n if air is not None else 0) + surveys * SURVEY_UP + ASSEMBLE_UP + handed
    kept = got['tissue']['p_amp'].size
    tissue = kept * (4 + 8 + 4 + (4 if ct is not None else 0) + (1 if air is not None else 0))
    water = kept * (4 + 8 + 4)
    assert got['traffic'] == (up, surveys * SURVEY_DOWN + ASSEMBLE_DOWN + tissue + water)


def test_stages_out_of_order_name_the_stage_they_need(golden):
    labels, ct, air, rec, kw = _inputs(golden, 'tight_small')
    ml = _materials(5)
    with AS.AcousticStudy(labels) as st:
        plan = st.plan(rec['SpatialStep'], **kw)
        with pytest.raises(_engine.EngineError, match='assemble comes first'):
            st.engine(ml, FREQ, rec['SpatialStep'], 1e-7, 10)
        st.assemble(plan, 5)
        dt = _engine.stable_dt(ml, FREQ, True, rec['SpatialStep'], H.ALPHA_CFL, 1.0)
        st.engine(ml, FREQ, rec['SpatialStep'], dt, 20)
        with pytest.raises(_engine.EngineError, match=r'rc=-6.*the run comes first'):
            st.pack(1.0, 'tissue')
        with pytest.raises(_engine.EngineError, match=r'rc=-6.*bfd_acoustic_pack of this slot comes first'):
            st.fetch('p_amp', 'tissue')
        st.set_source_plane(_plane(plan))
        st.run()
        st.pack(None, 'refocus', full=True)
        assert st.fetch('peak', 'refocus').shape == tuple(plan.mask_shape)
        with pytest.raises(_engine.EngineError, match=r'rc=-6.*bfd_acoustic_pack of this slot comes first'):
            st.fetch('p_amp', 'water')
        # a sim of another shape is not this study's
        other = _engine.Engine(plan.N1 + 1, plan.N2, plan.N3, 5, rec['SpatialStep'], dt, FREQ, 20)
        try:
            assert st._lib.bfd_acoustic_attach(st._handle(), other.h) == -1 and 'shape' in st._lib.bfd_last_error().decode()
        finally:
            other.close()
