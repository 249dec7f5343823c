"""The median filter without a GPU: the numpy oracle of the device tests equals scipy, and MedianFilter refuses bad arguments before the
library is loaded."""
import os

import numpy as np
import pytest

from babelbrain_amd import MedianFilter as MF, _engine
from tests.median_oracle import median_oracle, median_oracle_block

SHAPES = [(9, 8, 11), (7, 7, 7), (20, 17, 23), (3, 4, 70)]
SIZES = [3, 5, 7, (3, 5, 7), (7, 1, 3)]


def _volume(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape).astype(np.uint8)
    return rng.standard_normal(shape).astype(np.float32)


@pytest.mark.parametrize('mode', ['reflect', 'constant'])
@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
@pytest.mark.parametrize('size', SIZES, ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_oracle_equals_scipy(shape, size, dtype, mode):
    ndi = pytest.importorskip('scipy.ndimage')
    a = _volume(shape, dtype)
    cval = 3 if dtype == np.uint8 else -0.25
    ref = ndi.median_filter(a, size=size, mode=mode, cval=cval)
    got = median_oracle(a, size, mode, cval)
    assert got.dtype == a.dtype and got.shape == a.shape
    assert np.array_equal(got, ref)


def test_block_oracle_equals_whole():
    a = _volume((30, 26, 41), np.uint8, 1) % 6
    whole = median_oracle(a, 7)
    for lo, hi in (((0, 0, 0), (9, 8, 10)), ((11, 9, 13), (20, 19, 30)), ((21, 18, 30), (30, 26, 41))):
        blk = median_oracle_block(a, 7, lo, hi)
        assert np.array_equal(blk, whole[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])


@pytest.fixture
def no_library(monkeypatch):
    """Loading the library is an error here: the refusals below must come first."""
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_engine, 'load_library', boom)


@pytest.mark.parametrize('size', [2, 4, 9, 0, -3, (3, 3), (3, 4, 3), (3, 3, 9), 3.5, 'a', None], ids=str)
def test_bad_size(no_library, size):
    with pytest.raises(ValueError):
        MF.MedianFilter(np.zeros((8, 8, 8), np.uint8), size)


@pytest.mark.parametrize('dtype', [np.float64, np.int16, np.uint16, np.int8, np.int32, np.complex64])
def test_bad_dtype(no_library, dtype):
    with pytest.raises(TypeError):
        MF.MedianFilter(np.zeros((8, 8, 8), dtype), 3)


def test_other_refusals(no_library):
    a = np.zeros((8, 8, 8), np.uint8)
    with pytest.raises(ValueError):
        MF.MedianFilter(np.zeros((8, 8), np.uint8), 3)                       # not 3-D
    with pytest.raises(ValueError):
        MF.MedianFilter(np.zeros((2, 8, 8, 8), np.float32), 3)
    with pytest.raises(ValueError):
        MF.MedianFilter(np.zeros((2, 8, 8), np.uint8), 7)                    # axis 0 shorter than 7 // 2
    with pytest.raises(ValueError):
        MF.MedianFilter(np.zeros((8, 8, 1), np.float32), (1, 1, 5))
    with pytest.raises(ValueError):
        MF.MedianFilter(a, 3, mask=np.ones((8, 8, 7), np.uint8))             # mask of another shape
    with pytest.raises(ValueError):
        MF.MedianFilter(a, 3, mode='nearest')
    with pytest.raises(ValueError):
        MF.MedianFilter(a, 3, mode='constant', cval=256)
    with pytest.raises(ValueError):
        MF.median_in_region(np.zeros((2, 8, 8, 8), np.float32), np.ones((8, 8, 9), bool))
    with pytest.raises(ValueError):
        MF.median_in_region(np.zeros((8, 8), np.float32), np.ones((8, 8), bool))


def test_bool_and_strided_input_pass_the_checks(no_library):
    """bool is taken as uint8 and a non-contiguous view is made contiguous: both get as far as the library (which this fixture forbids)."""
    b = np.zeros((8, 9, 10), bool)
    b[2:5] = True
    a, s, mode, cval, m = MF._checked(b, 7, 'reflect', 0, None)
    assert a.dtype == np.uint8 and a.flags.c_contiguous and np.array_equal(a, b.astype(np.uint8)) and s == (7, 7, 7) and m is None
    v = np.arange(8 * 9 * 10, dtype=np.float32).reshape(8, 9, 10).transpose(2, 1, 0)
    a, s, mode, cval, m = MF._checked(v, (3, 5, 7), 'constant', 1.5, v > 100)
    assert a.flags.c_contiguous and np.array_equal(a, v) and s == (3, 5, 7) and mode == 1 and cval == 1.5
    assert m.dtype == np.uint8 and m.flags.c_contiguous and np.array_equal(m, (v > 100).astype(np.uint8))
    with pytest.raises(AssertionError, match='library was loaded'):
        MF.MedianFilter(b, 7, GPUBackend='OpenCL')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


def test_library_refuses_bad_arguments_before_any_device(lib):
    """bfd_median_filter3d reports argument errors (rc -1) before it looks for a device; nothing is read or written. A volume of 2^31
    voxels is one of them: nothing is truncated."""
    assert 'bfd_median_filter3d' in _engine.ABI_SYMBOLS and hasattr(lib, 'bfd_median_filter3d')
    a, o = np.zeros(64, np.uint8), np.full(64, 7, np.uint8)
    pa, po = _engine._ptr(a), _engine._ptr(o)

    def call(dtype=0, i=pa, out=po, N=(4, 4, 4), s=(3, 3, 3), mode=0, cval=0.0):
        return lib.bfd_median_filter3d(0, dtype, i, out, None, N[0], N[1], N[2], s[0], s[1], s[2], mode, cval, None)
    for kw, word in ((dict(N=(1 << 11, 1 << 10, 1 << 10)), '2^31'), (dict(N=(1 << 40, 1 << 40, 1 << 40)), '2^31'), (dict(dtype=2), 'dtype'),
                     (dict(s=(3, 2, 3)), 'size'), (dict(s=(9, 3, 3)), 'size'), (dict(N=(4, 2, 4), s=(3, 7, 3)), 'axis 1'), (dict(out=pa), 'alias'),
                     (dict(mode=2), 'mode'), (dict(mode=1, cval=300.0), 'cval'), (dict(i=None), 'null')):
        assert call(**kw) == -1, kw
        assert word in lib.bfd_last_error().decode(), (kw, lib.bfd_last_error().decode())
    assert np.all(a == 0) and np.all(o == 7)
