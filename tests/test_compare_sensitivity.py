"""What tests/util.py's exact comparison sees and the whole-array rel L2 it replaced does not.

The fields of a run span many decades (absorbing layer, ahead of the front, shadow of the skull), so an error confined to
quiet cells does not move an L2 norm taken over the whole array. Here faults are planted in a copy of the oracle's own
output (C2 medium, 64 x 60 x 72, 220 steps, every map, RMS and peak): each one (a) passes the old bound, rel L2 <= 1e-5,
which is why this test exists, and (b) makes compare_runs / assert_same raise with the planted location in the message.
No GPU: the oracle is on both sides."""
import copy

import numpy as np
import pytest

from babelbrain_amd import harness as H
from oracle import oracle as O
from tests.util import ALL_MAPS, assert_same, compare_runs, geometry_of, oracle_dt, rel_l2

OLD_TOL = 1e-5


@pytest.fixture(scope='module')
def run():
    a, k, info = H.make_problem('C2', N=(64, 60, 72), steps=220, stable_dt_fn=oracle_dt)
    k['SelMapsRMSPeakList'] = ALL_MAPS
    k['SelMapsSensorsList'] = ['Pressure', 'Vz', 'Sigmaxy']
    k['SelRMSorPeak'] = 3
    out = O.StaggeredFDTD_3D_with_relaxation(*a, **k)
    return out, geometry_of(a, k)


def _layer(geometry):
    N, nd, _ = geometry
    inner = np.zeros(N, bool)
    inner[nd:N[0] - nd, nd:N[1] - nd, nd:N[2] - nd] = True
    return ~inner


def _planted(out, slot, name, idx, value):
    bad = list(out)
    bad[slot] = dict(out[slot])
    bad[slot][name] = out[slot][name].copy()
    bad[slot][name][idx] = value
    return tuple(bad)


def _raises(out_bad, out, geometry):
    with pytest.raises(AssertionError) as e:
        compare_runs(out_bad, out, OLD_TOL, both=True, geometry=geometry)
    return str(e.value)


def test_identical_runs_and_signed_zeros_pass(run):
    out, geometry = run
    assert compare_runs(copy.deepcopy(out), out, 0.0, both=True, geometry=geometry) == 0.0
    z = np.zeros((4, 5, 6), np.float32)
    assert np.signbit(-z).all()
    assert_same(-z, z, 'minus zero against plus zero')
    assert_same(z, -z, 'plus zero against minus zero')


def test_smallest_last_map_value_in_the_layer_dropped(run):
    out, geometry = run
    ref = out[1]['Pressure']
    cand = _layer(geometry) & (ref != 0)
    assert cand.any()
    mag = np.where(cand, np.abs(ref), np.inf)
    idx = np.unravel_index(int(np.argmin(mag)), ref.shape)
    bad = _planted(out, 1, 'Pressure', idx, 0.0)
    assert rel_l2(bad[1]['Pressure'], ref) <= OLD_TOL
    msg = _raises(bad, out, geometry)
    assert 'last[Pressure]' in msg and '1 of %d elements differ' % ref.size in msg
    assert '(i, j, k) = (%d, %d, %d), inside the absorbing layer' % idx in msg
    assert 'material %d,' % geometry[2][idx] in msg
    assert 'sub-tile (%d, %d, %d)' % (idx[0] // 64, idx[1] // 8, idx[2] // 8) in msg


def test_quietest_sensor_row_dropped(run):
    out, geometry = run
    ref = out[0]['Pressure']
    norms = np.sqrt(np.sum(ref.astype(np.float64) ** 2, axis=1))
    assert (norms > 0).any()
    row = int(np.argmin(np.where(norms > 0, norms, np.inf)))
    bad = _planted(out, 0, 'Pressure', row, 0.0)
    assert rel_l2(bad[0]['Pressure'], ref) <= OLD_TOL
    msg = _raises(bad, out, geometry)
    i, j, k = H.decode_sensor_index(out[-1]['IndexSensorMap'][row:row + 1], geometry[0][0], geometry[0][1])
    assert 'sensor[Pressure]' in msg and '(sensor, sample) = (%d, ' % row in msg
    assert 'sensor voxel (i, j, k) = (%d, %d, %d)' % (i[0], j[0], k[0]) in msg
    assert '%d of %d elements differ' % (np.count_nonzero(ref[row]), ref.size) in msg


@pytest.mark.parametrize('slot,name', [(2, 'Pressure'), (3, 'Pressure'), (2, 'Sigmaxy')])
def test_value_written_into_the_layer_of_a_map(run, slot, name):
    """RMS and peak maps stay at exactly 0 inside the absorbing layer; half of 1e-5 x the map's norm in one such cell is
    below the old bound by construction."""
    out, geometry = run
    ref = out[slot][name]
    assert ref.max() > 0 and np.all(ref[_layer(geometry)] == 0)
    idx = (geometry[1] // 2, ref.shape[1] // 2, ref.shape[2] // 3)
    assert _layer(geometry)[idx]
    value = np.float32(0.5 * OLD_TOL * np.sqrt(np.sum(ref.astype(np.float64) ** 2)))
    assert value > 0
    bad = _planted(out, slot, name, idx, value)
    assert 0 < rel_l2(bad[slot][name], ref) <= OLD_TOL
    msg = _raises(bad, out, geometry)
    assert '[%s]' % name in msg and '(i, j, k) = (%d, %d, %d), inside the absorbing layer' % idx in msg


@pytest.mark.parametrize('slot,name', [(1, 'Pressure'), (2, 'Pressure'), (1, 'Vx')])
def test_largest_element_moved_by_one_ulp(run, slot, name):
    """One ulp is 6e-8 of the value, and the value is at most the norm."""
    out, geometry = run
    ref = out[slot][name]
    idx = np.unravel_index(int(np.argmax(np.abs(ref))), ref.shape)
    bad = _planted(out, slot, name, idx, np.nextafter(ref[idx], np.float32(np.inf)))
    assert 0 < rel_l2(bad[slot][name], ref) <= OLD_TOL
    msg = _raises(bad, out, geometry)
    assert '(i, j, k) = (%d, %d, %d), ' % idx in msg
    assert '(1 ulp)' in msg and 'largest distance 1 ulp' in msg


def test_nan_where_the_reference_is_zero(run):
    out, geometry = run
    ref = out[2]['Pressure']
    idx = (1, 2, 3)
    assert ref[idx] == 0
    bad = _planted(out, 2, 'Pressure', idx, np.nan)
    msg = _raises(bad, out, geometry)
    assert 'non-finite' in msg and '(i, j, k) = (1, 2, 3)' in msg
    with pytest.raises(AssertionError, match='non-finite'):            # on either side
        assert_same(ref, bad[2]['Pressure'], 'NaN in the reference')
    inf = ref.copy(); inf[idx] = np.inf
    with pytest.raises(AssertionError, match='non-finite'):
        assert_same(inf, inf, 'the same infinity on both sides')


def test_shape_and_type_are_part_of_the_comparison(run):
    out, _ = run
    ref = out[2]['Pressure']
    with pytest.raises(AssertionError, match='shape'):
        assert_same(ref[:-1], ref, 'a plane short')
    with pytest.raises(AssertionError, match='float32'):
        assert_same(ref.astype(np.float64), ref, 'float64')


def test_the_old_bound_alone_lets_these_faults_through(run):
    """exact=False is the old behaviour: half of a quiet map gone, still green."""
    out, geometry = run
    ref = out[1]['Pressure']
    order = np.argsort(np.abs(ref), axis=None)
    cut = order[:int(0.4 * ref.size)]                      # the 40 % of smallest magnitude, all at once
    bad = list(out); bad[1] = dict(out[1]); bad[1]['Pressure'] = ref.copy()
    bad[1]['Pressure'].reshape(-1)[cut] = 0
    assert np.count_nonzero(ref.reshape(-1)[cut]) > 0.05 * ref.size
    compare_runs(tuple(bad), out, OLD_TOL, both=True, exact=False)
    _raises(tuple(bad), out, geometry)
