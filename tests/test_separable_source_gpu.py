"""SeparableSource on the device (bfd_set_sources_separable): every result equals the dense path fed src.dense() bit for
bit -- drop-in calls with every TypeSource, a streamed dense table, quiet runs on and off, graph replay with the source form
replaced between pieces, reset, the multi-slab group, the K = 1 point source of the back-propagation call -- and the CW form
agrees with the caller's own float64 table to float32 rounding."""
import numpy as np
import pytest

from babelbrain_amd import PropagationModel, SeparableSource, _engine, harness as H
from babelbrain_amd.PropagationModel import compact_sources
from tests.util import oracle_dt, rel_l2

pytestmark = pytest.mark.gpu

N = (48, 40, 56)


def _problem(steps=150, type_source=0, **kw):
    a, k, info = H.make_problem('C2', N=N, steps=steps, stable_dt_fn=oracle_dt, separable=True, **kw)
    assert isinstance(a[4], SeparableSource)
    k.update(TypeSource=type_source, SelMapsRMSPeakList=['Pressure', 'Vz'], SelMapsSensorsList=['Pressure', 'Vz'], SelRMSorPeak=3)
    if type_source >= 2:        # stress sources are weighted by Ox; the caller's velocity weights (Ox = Oy = 0) would silence them
        k.update(Ox=np.array([1.0]), Oy=np.array([1.0]), Oz=np.array([1.0]))
    return a, k, info


def _with(a, pulse):
    a = list(a)
    a[4] = pulse
    return tuple(a)


def _call(a, k, **kw):
    return PropagationModel().StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, **k, **kw)


def _same(out, ref):
    """sensor series, last, RMS and peak maps"""
    assert len(out) == len(ref) == 5
    for q in range(4):
        assert set(out[q]) == set(ref[q])
        for n in ref[q]:
            assert np.array_equal(out[q][n], ref[q][n]), (q, n)
    assert np.array_equal(out[-1]['IndexSensorMap'], ref[-1]['IndexSensorMap'])
    assert np.abs(ref[2]['Pressure']).max() > 0


@pytest.mark.parametrize('type_source', [0, 1, 2, 3])
def test_drop_in_call_equals_dense_table(type_source):
    a, k, info = _problem(type_source=type_source)
    src = a[4]
    out = _call(a, k)
    ref = _call(_with(a, src.dense()), k)
    _same(out, ref)
    # weights and signals instead of the table: fewer device bytes
    assert out[-1]['device_bytes'] < ref[-1]['device_bytes']


def test_streamed_dense_leg_equals_resident_separable(monkeypatch):
    a, k, info = _problem()
    out = _call(a, k)
    monkeypatch.setenv('BFD_SOURCE_TILE', '16')
    ref = _call(_with(a, a[4].dense()), k)
    _same(out, ref)


def test_quiet_runs_on_and_off(monkeypatch):
    a, k, info = _problem()
    ref = _call(_with(a, a[4].dense()), k)
    for mode in ('1', '0'):
        monkeypatch.setenv('BFD_SKIP_ZERO', mode)
        _same(_call(a, k), ref)


def test_graph_replay_with_the_source_form_replaced(monkeypatch):
    """BFD_USE_GRAPH=1, kernelVariant 3: the run is cut into pieces and the source form replaced between them (dense,
    separable, dense); every replacement drops the recorded graph, the next piece records one with the new form"""
    a, k, info = _problem(steps=200)
    mm, ml, f, smap, src, h, T, sensor = a
    assert k['SensorStart'] * k['SensorSubSampling'] > 64
    dense = src.dense()
    srcs = compact_sources(smap, k['Ox'], k['Oy'], k['Oz'])

    def run(pieces, forms):
        eng = _engine.Engine(*mm.shape, len(ml), h, k['DT'], f, info['nt'], sensorSub=k['SensorSubSampling'],
                             sensorStart=k['SensorStart'], selMapsRMS=['Pressure'], selMapsSensors=['Pressure', 'Vz'], kernelVariant=3)
        eng.set_materials(ml, k['QCorrection'])
        eng.set_material_map(mm, 0, 0)
        eng.set_sensor_map(sensor)
        for n, form in zip(pieces, forms):
            if form is not None:
                eng.set_sources(*srcs, form)
            eng.run(n)
        assert eng.step == info['nt']
        out = (eng.sensors().copy(), eng.get_map(_engine.KIND_RMS, 'Pressure'), eng.get_field('Vz'), eng.get_field('Szz'))
        eng.close()
        return out

    monkeypatch.setenv('BFD_USE_GRAPH', '1')
    ref = run([info['nt']], [dense])
    got = run([27, 40, info['nt'] - 67], [dense, src, dense])
    sep = run([info['nt']], [src])
    monkeypatch.delenv('BFD_USE_GRAPH')
    direct = run([27, 40, info['nt'] - 67], [dense, src, dense])
    for x, y, z, d in zip(ref, got, sep, direct):
        assert np.array_equal(x, y) and np.array_equal(x, z) and np.array_equal(x, d)
    assert np.abs(ref[1]).max() > 0


def test_reset_and_group_call():
    a, k, info = _problem(type_source=2)
    mm, ml, f, smap, src, h, T, sensor = a
    ref = _call(_with(a, src.dense()), k)
    eng = _engine.Engine(*mm.shape, len(ml), h, k['DT'], f, info['nt'], typeSource=2, sensorSub=k['SensorSubSampling'],
                         sensorStart=k['SensorStart'], selMapsRMS=['Pressure'], selMapsSensors=['Pressure'])
    eng.set_materials(ml, k['QCorrection'])
    eng.set_material_map(mm, 0, 0)
    eng.set_sources(*compact_sources(smap, k['Ox'], k['Oy'], k['Oz']), src)
    eng.set_sensor_map(sensor)
    eng.run(60)
    eng.reset()
    eng.run(info['nt'])
    assert np.array_equal(eng.get_map(_engine.KIND_RMS, 'Pressure'), ref[2]['Pressure'])
    eng.close()
    one = _call(a, k)
    grp = _call(a, k, DefaultGPUDeviceNumber=[0, 0])
    assert len(grp[-1]['slabs']) == 2
    _same(grp, one)
    _same(one, ref)


def test_punctual_k1_stress_source():
    """the back-propagation call: one stress source (TypeSource 2) at the target, unit sine ramped at both ends"""
    a, k, info = _problem(steps=300, type_source=2)
    mm, ml, f, _, _, h, T, _ = a
    N1, N2, N3 = mm.shape
    _, back = H.sensor_maps(N1, N2, N3, info['zsrc'])
    smap = H.punctual_source_map(N1, N2, N3, (N1 // 2, N2 // 2, N3 // 2))
    src = H.punctual_source_separable(f, k['DT'], T)
    assert src.K == 1
    kw = {q: v for q, v in k.items() if q not in ('Ox', 'Oy', 'Oz')}
    out = PropagationModel().StaggeredFDTD_3D_with_relaxation(mm, ml, f, smap, src, h, T, back, SILENT=True, **kw)
    ref = PropagationModel().StaggeredFDTD_3D_with_relaxation(mm, ml, f, smap, src.dense(), h, T, back, SILENT=True, **kw)
    _same(out, ref)
    assert np.array_equal(src.dense(), H.punctual_source(f, k['DT'], T).astype(np.float32).astype(np.float64))


def test_cw_form_against_the_float64_table():
    """cw_pulse_sources against pulse_sources's float64 table (C2 medium, 48 x 40 x 56, 150 steps): the Pressure RMS map and
    the sensor series agree to rel-L2 <= 1e-5 (observed on the MI355X: RMS 6.6e-8, sensors 1.6e-7)."""
    a, k, info = _problem()
    a64, k64, _ = H.make_problem('C2', N=N, steps=150, stable_dt_fn=oracle_dt)
    assert isinstance(a64[4], np.ndarray) and a64[4].dtype == np.float64
    out = _call(a, k)
    ref = _call(a64, k)
    e_rms = rel_l2(out[2]['Pressure'], ref[2]['Pressure'])
    e_sens = rel_l2(out[0]['Pressure'], ref[0]['Pressure'])
    print('separable vs float64 table: RMS rel-L2 %.3e, sensors %.3e' % (e_rms, e_sens))
    assert e_rms <= 1e-5 and e_sens <= 1e-5
    assert e_rms > 0          # two different float32 tables
