"""The oracle in arbitrary Z-cuts equals the oracle: OracleSlab engines at the cut sets of tests/slab_cuts.py (thin slabs, uneven
cuts, cuts inside the absorbing layer), their halo planes exchanged in-process, against the single-domain oracle on every
output, element by element. This holds merge_slab_outputs, the oracle's ghost handling and the cut sets themselves without a
GPU; tests/test_slab_cuts_gpu.py runs the HIP engines on the same cases."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import slab_cuts as SC
from tests.util import geometry_of


def _check(a, k, cuts, what):
    ref = SC.as_merged(O.StaggeredFDTD_3D_with_relaxation(*a, nthreads=4, **k), k)
    got = SC.run_oracle_cuts(a, k, cuts)
    SC.assert_merged_same(got, ref, geometry_of(a, k), what)
    return ref


@pytest.mark.parametrize('medium,cutset', SC.CASES)
def test_oracle_slabs_at_the_cuts_equal_the_oracle(medium, cutset):
    a, k, cuts = SC.problem(medium, cutset)
    what = '%s cuts %s' % (medium, cutset)
    ref = _check(a, k, cuts, what)
    SC.assert_cuts_are_live(ref, a, cuts, what)
    assert np.abs(ref['LastMap']['Pressure'][:, :, -1]).max() > 0                  # the wave reaches the last plane
    if medium.startswith('C2'):
        assert np.abs(ref['LastMap']['Sigmaxy']).max() > 0
    if (medium, cutset) in (('C2', 'A'), ('C2wide', 'A')):
        assert len(SC.cuts_across_solid(a, cuts)) >= 3                             # shear edges and 1/rho face averages across the cut


def test_the_cut_sets_reach_the_thicknesses_they_are_for():
    """SUB = 8 (see tests/test_slab_cuts_gpu.py): every thickness around a multiple of the sub-tile depth up to 3 SUB + 2"""
    nk = lambda name: sorted(set(n for _, n in SC.bounds_of(SC.CUTS[name])))
    assert nk('A') == [4, 5, 7, 8, 14] and nk('B') == [7, 9, 10, 15, 16] and nk('C') == [17, 23, 24]
    assert nk('D33') == [31, 33] and nk('D31') == [31, 33] and nk('E') == [4, 5] and nk('Q26') == [26]
    for seed, cuts in SC.RANDOM_CUTS.items():
        assert all(4 <= n <= 9 for _, n in SC.bounds_of(cuts))


@pytest.mark.parametrize('seed', sorted(SC.RANDOM_CUTS))
def test_oracle_slabs_in_random_media(seed):
    """solid specks and reflector pockets inside the layer, slabs of 4 to 9 planes"""
    a, k, cuts = SC.problem('random', seed)
    ref = _check(a, k, cuts, 'random medium %d' % seed)
    assert SC.solid_of(a).any() and np.abs(ref['LastMap']['Pressure']).max() > 0


@pytest.mark.parametrize('type_source', [0, 1, 2, 3])
def test_oracle_sources_and_sensors_on_cut_planes(type_source):
    a, k, cuts = SC.cut_plane_problem(type_source)
    ref = _check(a, k, cuts, 'TypeSource %d' % type_source)
    z = (ref['IndexSensorMap'].astype(np.int64) - 1) // (a[0].shape[0] * a[0].shape[1])
    assert set((15, 16, 17, 18)) <= set(z.tolist())
    for p in (15, 16, 17, 18):
        assert np.abs(ref['Sensor']['Pressure'][z == p]).max() > 0


def test_create_hip_slab_refuses_bounds_it_cannot_hold():
    """bounds= is checked before an engine exists: thinner than the splitters allow, outside the domain, not the rank's place"""
    from babelbrain_amd import slab
    a, k, cuts = SC.problem('C2', 'A')
    for rank, world, bounds in ((1, 3, (20, 3)), (2, 3, (60, 8)), (0, 3, (4, 8)), (2, 3, (40, 8)), (1, 3, (0, 8))):
        with pytest.raises(ValueError, match='bounds'):
            slab.create_hip_slab(a, k, rank, world, 0, bounds=bounds)
    with pytest.raises(ValueError, match='bounds'):
        slab.create_hip_slab(a, k, 0, 2, 0, bounds=(0, 32), local=(64, 0, 32, 0, 2))
