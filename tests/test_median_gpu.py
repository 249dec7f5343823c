"""The device median filter (bfd_median_filter3d behind babelbrain_amd.MedianFilter) against the numpy oracle of tests/median_oracle.py, element by
element. The kernel's output tile is 4 x 4 x 64 voxels (i, j, k; lanes along k) with a halo of size // 2: the shapes below are the smallest that leave a
tile partly empty, span several tiles on every axis, or are thinner than the halo."""
import numpy as np
import pytest

from babelbrain_amd import MedianFilter as MF
from tests.median_oracle import median_oracle, median_oracle_block
from tests.util import assert_same

pytestmark = pytest.mark.gpu

TILE = (4, 4, 64)
OVER = (10, 9, 133)          # 2 tiles + 2, 2 tiles + 1, 2 tiles + 5: exceeds the 4 x 4 x 64 tile by a non-multiple on every axis
SHAPES = [(20, 17, 23), (7, 7, 7), (3, 4, 70), OVER]
SIZES = [3, 5, 7, (3, 5, 7), (7, 1, 3), (1, 1, 1)]


def same(got, ref, what):
    """assert_same on the values; uint8 goes through float32, which holds every uint8 exactly"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    if got.dtype == np.uint8:
        got, ref = got.astype(np.float32), ref.astype(np.float32)
    assert_same(got, ref, what)


def run(a, size, **kw):
    before = a.copy()
    got = MF.MedianFilter(a, size, **kw)
    assert np.array_equal(a.view(np.uint8), before.view(np.uint8)), 'the input was modified'
    assert got is not a and got.flags.c_contiguous
    return got


@pytest.mark.parametrize('mode,cval', [('reflect', 0), ('constant', 0), ('constant', 1)])
@pytest.mark.parametrize('size', SIZES, ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_uint8_labels(shape, size, mode, cval):
    a = np.random.default_rng(11).integers(0, 6, shape).astype(np.uint8)
    got = run(a, size, mode=mode, cval=cval)
    same(got, median_oracle(a, size, mode, cval), 'labels %s size %s %s cval %d' % (shape, size, mode, cval))
    if size == (1, 1, 1):
        assert np.array_equal(got, a)


RANGE_SHAPE = (14, 13, 150)


def _range_volume(kind):
    rng = np.random.default_rng(5)
    if kind == 'full':
        return rng.integers(0, 256, RANGE_SHAPE).astype(np.uint8)
    a = rng.integers(0, 2, RANGE_SHAPE).astype(np.uint8)
    if kind == 'sparse-high':
        # single voxels of 128..255 at density 1e-3, and two placed by hand: the first voxel of tile (1, 1, 1) lies in the halo of the seven
        # tiles below it and in no other tile; (3, 3, 63) is the last voxel of tile (0, 0, 0)
        hit = rng.random(RANGE_SHAPE) < 1e-3
        a[hit] = rng.integers(128, 256, int(hit.sum())).astype(np.uint8)
        a[4, 4, 64] = 128
        a[3, 3, 63] = 255
        assert 2 <= int((a >= 128).sum()) < 100
    return a


@pytest.mark.parametrize('size', [7, 3])
@pytest.mark.parametrize('kind', ['full', 'binary', 'sparse-high'])
def test_uint8_value_ranges(kind, size):
    a = _range_volume(kind)
    for mode, cval in (('reflect', 0), ('constant', 255)):       # cval 255: the fill alone widens the range of a tile at the boundary
        same(run(a, size, mode=mode, cval=cval), median_oracle(a, size, mode, cval), 'uint8 %s size %d %s' % (kind, size, mode))


def _float_volume(kind):
    rng = np.random.default_rng(3)
    x = rng.standard_normal(OVER)
    if kind == 'normal':
        return x.astype(np.float32)
    if kind == 'four-values':
        return np.array([-1.5, -0.0, 0.25, 3.0], np.float32)[rng.integers(0, 4, OVER)]
    if kind == 'signed-zeros':
        return np.array([-0.0, 0.0, -0.0, 0.0, -1e-3, 1e-3], np.float32)[rng.integers(0, 6, OVER)]
    a = (x * 1e-41).astype(np.float32)                           # float32 denormals, both signs
    assert np.all(np.abs(a) < np.finfo(np.float32).tiny) and np.count_nonzero(a) > 0.99 * a.size
    return a


@pytest.mark.parametrize('size', [3, (3, 5, 7)], ids=str)
@pytest.mark.parametrize('kind', ['normal', 'four-values', 'signed-zeros', 'denormal'])
def test_float32(kind, size):
    a = _float_volume(kind)
    for mode, cval in (('reflect', 0), ('constant', -0.5)):
        ref = median_oracle(a, size, mode, cval)
        got = run(a, size, mode=mode, cval=cval)
        same(got, ref, 'float32 %s size %s %s' % (kind, size, mode))
        if kind in ('normal', 'denormal'):                       # no ties between +0 and -0 here: the bits themselves must agree
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        if kind == 'denormal' and mode == 'reflect':
            assert np.count_nonzero(got) > 0.99 * got.size, 'denormals were flushed'


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_region_mask(dtype):
    rng = np.random.default_rng(8)
    shape = (13, 10, 140)
    a = rng.integers(0, 6, shape).astype(np.uint8) if dtype == np.uint8 else rng.standard_normal(shape).astype(np.float32)
    size = 5
    ref = median_oracle(a, size)
    full = run(a, size)
    same(full, ref, 'unmasked')
    bits = np.uint8 if dtype == np.uint8 else np.uint32

    region = np.zeros(shape, bool)
    region[2:9, 1:7, 30:100] = rng.random((7, 6, 70)) < 0.5        # some tiles whole, some partly, most not at all
    got = run(a, size, mask=region)
    same(got, np.where(region, ref, a), 'region')
    assert np.array_equal(got.view(bits)[~region], a.view(bits)[~region])          # bit for bit outside
    assert np.array_equal(got.view(bits)[region], full.view(bits)[region])         # the unmasked call's bits inside

    same(run(a, size, mask=np.zeros(shape, np.uint8)), a, 'empty region')
    same(run(a, size, mask=np.full(shape, 200, np.uint8)), ref, 'full region, mask values other than 1')
    for corner in ((4, 4, 64), (3, 3, 63), (0, 0, 0), (12, 9, 139), (7, 8, 127)):   # one voxel on a tile corner
        one = np.zeros(shape, np.uint8)
        one[corner] = 1
        want = a.copy()
        want[corner] = ref[corner]
        same(run(a, size, mask=one), want, 'single voxel %s' % (corner,))


def test_many_tiles():
    shape = (192, 160, 176)
    a = np.random.default_rng(21).integers(0, 6, shape).astype(np.uint8)
    got = run(a, 7)
    for lo in ((0, 0, 0), (76, 58, 70), (152, 120, 136)):          # a corner of the volume, the interior, the opposite corner
        hi = tuple(v + 40 for v in lo)
        blk = got[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        same(np.ascontiguousarray(blk), median_oracle_block(a, 7, lo, hi), 'block at %s' % (lo,))
    assert np.array_equal(run(a, 7), got), 'two calls differ'


def test_drop_in_surface():
    rng = np.random.default_rng(2)
    a = np.ascontiguousarray(rng.integers(0, 2, (24, 19, 70)).astype(np.uint8))
    before = a.copy()
    got = MF.MedianFilter(a, 7, GPUBackend='OpenCL')
    assert got.dtype == np.uint8 and got.shape == a.shape and np.array_equal(a, before)
    same(got, median_oracle(a, 7), 'MedianFilter(a, 7, GPUBackend=...)')
    same(MF.MedianFilter(a.astype(bool), 7), got, 'bool input')
    same(MF.MedianFilter(a.transpose(2, 1, 0), (3, 5, 7)), median_oracle(np.ascontiguousarray(a.transpose(2, 1, 0)), (3, 5, 7)), 'strided input')
    assert MF.InitMedianFilter(DeviceName='no such device', GPUBackend='Metal')

    fields = rng.standard_normal((2, 12, 11, 80)).astype(np.float32)
    skull = rng.random((12, 11, 80)) < 0.3
    want = fields.copy()
    for n in range(2):                                           # CalculateTemperatureEffects.py:915-918 with the oracle as median_filter
        sk = median_oracle(want[n].copy(), 3)
        want[n][skull] = sk[skull]
    kept = fields.copy()
    got = MF.median_in_region(fields, skull)
    assert np.array_equal(fields, kept)
    same(got, want, 'median_in_region, two fields')
    same(MF.median_in_region(fields[1], skull, size=3), want[1], 'median_in_region, one field')
