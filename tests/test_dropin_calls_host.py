"""The entries the drop-in call makes, in order, on its three paths: one engine, a group of two slabs, and the DFT-only sensors of one
engine. A recording stub stands in for the loaded library (no library, no GPU). Engine and Group share their calls in one base and
StaggeredFDTD_3D_with_relaxation has one body for both solvers; the lists below were recorded with this stub from the code that
still had the two classes and the two bodies written out side by side, so they hold the merged code to what both copies called."""
import numpy as np
import pytest

from babelbrain_amd import PropagationModel, _engine

VALUES = {'bfd_device_count': 1, 'bfd_group_size': 2, 'bfd_num_sensors': 0, 'bfd_placement_note': b'', 'bfd_last_error': b''}


class Recorder:
    """Every bfd_* entry returns 0, but for the few whose value is read (VALUES); *_create hands out a handle so that close() has one."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('bfd_'):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            if name.endswith('_create'):
                args[-1]._obj.value = 0x1000
            return VALUES.get(name, 0)
        return entry


N = (8, 8, 16)
SETUP = ['set_materials', 'set_material_map', 'set_reflector', 'set_sources', 'set_sensor_map', 'timing_begin', 'run', 'timing_end']

SINGLE = (['bfd_device_count', 'bfd_device_name', 'bfd_device_count', 'bfd_create'] + ['bfd_' + e for e in SETUP] +
          ['bfd_num_sensors', 'bfd_num_sensor_steps', 'bfd_get_sensors', 'bfd_num_sensors', 'bfd_get_sensor_index', 'bfd_device_bytes',
           'bfd_placement_note', 'bfd_get_map', 'bfd_get_map', 'bfd_get_map', 'bfd_destroy', 'bfd_placement_cache_release'])
GROUP = (['bfd_device_count', 'bfd_group_create'] + ['bfd_group_' + e for e in SETUP] +
         ['bfd_group_size', 'bfd_group_size', 'bfd_group_peer_status',
          'bfd_group_num_sensors', 'bfd_group_num_sensor_steps', 'bfd_group_get_sensors', 'bfd_group_num_sensors', 'bfd_group_get_sensor_index',
          'bfd_group_device_bytes', 'bfd_group_size', 'bfd_group_slab', 'bfd_group_slab', 'bfd_group_size', 'bfd_group_slab', 'bfd_placement_note',
          'bfd_group_slab', 'bfd_placement_note', 'bfd_group_get_map', 'bfd_group_get_map', 'bfd_group_get_map', 'bfd_group_destroy',
          'bfd_placement_cache_release'])
DFT_ONLY = (['bfd_device_count', 'bfd_device_name', 'bfd_device_count', 'bfd_create'] + ['bfd_' + e for e in SETUP] +
            ['bfd_num_sensors', 'bfd_get_sensor_index', 'bfd_device_bytes', 'bfd_placement_note', 'bfd_num_sensors', 'bfd_num_sensors',
             'bfd_get_sensor_dft', 'bfd_get_map', 'bfd_get_map', 'bfd_get_map', 'bfd_destroy', 'bfd_placement_cache_release'])


def dropin(monkeypatch, devices=None, **kw):
    rec = Recorder()
    monkeypatch.setattr(_engine, '_lib', rec)
    mm = np.zeros(N, np.uint32)
    src = np.zeros(N, np.uint32); src[4, 4, 3] = 1
    sen = np.zeros(N, np.uint32); sen[4, 4, 10] = 1
    out = PropagationModel(devices=devices).StaggeredFDTD_3D_with_relaxation(
        mm, np.array([[1000.0, 1500.0, 0.0, 0.0, 0.0]]), 5e5, src, np.ones((1, 20)), 1e-3, 20 * 1e-7, sen, DT=1e-7, SelRMSorPeak=3,
        SelMapsRMSPeakList=['Pressure'], SelMapsSensorsList=['Pressure'], ReflectorMask=np.zeros(N, np.uint32), SILENT=True, **kw)
    return rec.calls, out


def test_single_device_path(monkeypatch):
    calls, out = dropin(monkeypatch)
    assert calls == SINGLE
    assert len(out) == 5 and sorted(out[0]) == ['Pressure', 'time'] and all(sorted(m) == ['Pressure'] for m in out[1:4])
    assert list(out[4]) == ['IndexSensorMap', 'DT', 'nt', 'device_bytes', 'timing', 'placement'] and out[4]['placement'] == ''


def test_group_path(monkeypatch):
    calls, out = dropin(monkeypatch, devices=[0, 0])
    assert calls == GROUP
    assert len(out) == 5 and sorted(out[0]) == ['Pressure', 'time'] and all(m['Pressure'].shape == N for m in out[1:4])
    assert list(out[4]) == ['IndexSensorMap', 'DT', 'nt', 'device_bytes', 'timing', 'devices', 'slabs', 'placement']
    assert out[4]['devices'] == [0, 0] and out[4]['placement'] == ['', ''] and len(out[4]['slabs']) == 2


def test_dft_only_path(monkeypatch):
    calls, out = dropin(monkeypatch, ReturnSensorDFT=True, ReturnSensorSeries=False)
    assert calls == DFT_ONLY
    assert list(out[0]) == ['time']
    assert list(out[4]) == ['IndexSensorMap', 'DT', 'nt', 'device_bytes', 'timing', 'placement', 'SensorDFT', 'SensorPeak']


@pytest.mark.parametrize('devices', [None, [0, 0]])
def test_neither_series_nor_dft_is_refused_before_a_solver_exists(monkeypatch, devices):
    with pytest.raises(ValueError, match='ReturnSensorSeries=False needs ReturnSensorDFT=True'):
        dropin(monkeypatch, devices=devices, ReturnSensorSeries=False)
    assert _engine._lib.calls == []
