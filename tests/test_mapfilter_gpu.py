"""Device CT value mapping (bfd_map_values3d behind babelbrain_amd.MappingFilter.MapFilter) held to EQUALITY against np.searchsorted plus an
equality check, and against the literal host loop of the reference's Step 1 (BabelDatasetPreps.py:1034-1037) on small cases. The kernel stages the
table in LDS up to 4096 rows and reads it from global memory beyond: the table sizes straddle that switch."""
import numpy as np
import pytest

from babelbrain_amd import MappingFilter as MF
from tests import voxelize_oracle as VO

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (7, 9, 65), (33, 64, 130)]
TABLE_SIZES = [1, 2, 1023, 1024, 4096, 4097, 65536]
_tables = {}


def table(nU):
    """nU distinct float32 values, ascending, with 0.0 among them (nU > 1), built once"""
    if nU not in _tables:
        rng = np.random.default_rng(nU)
        u = np.unique(rng.uniform(-1100.0, 3200.0, 2 * nU).astype(np.float32))
        u = u[u != 0][:nU - 1]                                    # float32 leaves far more than nU distinct values of 2 nU draws
        u = np.unique(np.concatenate([[0.0], u]).astype(np.float32)) if nU > 1 else np.array([417.25], np.float32)
        assert u.size == nU and np.all(u[1:] > u[:-1])
        u.setflags(write=False)
        _tables[nU] = u
    return _tables[nU]


def volume(shape, uni, seed):
    """Three quarters table values, one quarter values the table lacks, and the special values where there is room"""
    rng = np.random.default_rng(seed)
    hu = uni[rng.integers(0, uni.size, shape)]
    absent = rng.random(shape) < 0.25
    hu[absent] = np.nextafter(hu[absent], np.float32(np.inf))            # one ulp off a table value (the table may hold that one too: the oracle decides)
    flat = hu.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e30, -1e30, uni[0], uni[-1]], np.float32)
    if flat.size >= special.size:
        flat[rng.permutation(flat.size)[:special.size]] = special
    sel = (rng.random(shape) < 0.6).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)      # any non-zero byte selects
    return hu, sel


def check(hu, sel, uni):
    hu0, sel0 = hu.copy(), sel.copy()
    out = MF.MapFilter(hu, sel, np.array(uni), GPUBackend='OpenCL')
    assert out.dtype == np.uint32 and out.shape == hu.shape
    assert np.array_equal(hu, hu0, equal_nan=True) and np.array_equal(sel, sel0)
    assert np.array_equal(out, VO.map_values(hu, sel, uni))
    assert MF.last_kernel_ms > 0
    return out


@pytest.mark.parametrize('nU', TABLE_SIZES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_against_searchsorted(shape, nU):
    uni = table(nU)
    hu, sel = volume(shape, uni, 7 * nU + shape[2])
    out = check(hu, sel, uni)
    if hu.size > 1000 and nU > 1:
        assert np.count_nonzero(out) > 0 and np.count_nonzero((out == 0) & (sel != 0)) > 0


@pytest.mark.parametrize('nU', [1, 2, 40])
def test_against_the_host_loop(nU):
    uni = table(nU)
    hu, sel = volume((7, 9, 65), uni, nU)
    out = check(hu, sel, uni)
    assert np.array_equal(out, VO.map_values_host_loop(hu, sel, uni))


def test_special_values():
    uni = np.array([-np.inf, -3.5, 0.0, 2.0, np.inf], np.float32)
    hu = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 2.0, 2.0000002, -3.5, 1e-45, -1e-45, 7.0], np.float32).reshape(1, 1, -1)
    one = np.ones(hu.shape, np.uint8)
    out = check(hu, one, uni)
    assert out.ravel().tolist() == [2, 2, 0, 4, 0, 3, 0, 1, 0, 0, 0]       # -inf is row 0: indistinguishable from "absent", as in the reference
    assert np.array_equal(out, VO.map_values_host_loop(hu, one, uni))
    assert not check(hu, np.zeros(hu.shape, np.uint8), uni).any()          # nothing selected
    neg = np.array([-2.0, -0.0, 5.0], np.float32)                          # the table's zero is negative, the volume's positive
    assert check(np.array([[[0.0, -0.0, 5.0]]], np.float32), np.ones((1, 1, 3), np.uint8), neg).ravel().tolist() == [1, 1, 2]


@pytest.mark.parametrize('sel_value', [0, 1])
def test_selection_all_or_nothing(sel_value):
    uni = table(1024)
    hu, _ = volume((7, 9, 65), uni, 3)
    out = check(hu, np.full(hu.shape, sel_value, np.uint8), uni)
    assert out.any() == bool(sel_value)


def test_quantised_ct():
    """The table and the volume as Step 1 builds them (BabelDatasetPreps.py:1022-1027): CT values of the bone voxels quantised to 2^10 levels, np.unique
    of those, bone mask as uint8."""
    rng = np.random.default_rng(11)
    ct = rng.normal(900.0, 450.0, (33, 64, 130)).astype(np.float32)
    bone = ct > 300.0
    lo, hi = ct[bone].min(), ct[bone].max()
    A, M = hi - lo, 2 ** 10 - 1
    ct[bone] = (A / M) * np.round((M / A) * (ct[bone] - lo)) + lo
    uni = np.unique(ct[bone])
    assert ct.dtype == np.float32 and uni.dtype == np.float32 and 512 < uni.size <= 1024
    out = check(ct, bone.astype(np.uint8), uni)
    assert np.array_equal(uni[out[bone]], ct[bone]) and not out[~bone].any()
    assert np.array_equal(np.unique(out[bone]), np.arange(uni.size))
