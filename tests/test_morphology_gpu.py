"""Device binary morphology (bfd_binary_morphology3d behind babelbrain_amd.BinaryClosing) against scipy.ndimage, voxel for voxel.
The kernels pack the mask to words of W = 64 voxels along k and work with one thread per word; along i and j they have no tile of their own, so T
is the 8 x 8 x 64 tile of the labelling that follows them in the chain. N3 covers less than a word, exactly one, one plus 6 and two plus 5; i and j
take T + 1 and 2 T + 2."""
import numpy as np
import pytest

from babelbrain_amd import BinaryClosing as BC

ndi = pytest.importorskip('scipy.ndimage')

pytestmark = pytest.mark.gpu

T = 8
W = 64
SHAPES = [(T + 1, 2 * T + 2, 31), (2 * T + 2, T + 1, W), (T + 1, T + 1, W + 6), (2 * T + 2, T + 1, 2 * W + 5)]
BOXES = [14, 13, 2, 31, (14, 13, 10), (5, 4, 3), (1, 1, 1)]
DEVICE = {'erosion': BC.BinaryErode, 'dilation': BC.BinaryDilate, 'closing': BC.BinaryClose, 'opening': BC.BinaryOpen}
SCIPY = {'erosion': ndi.binary_erosion, 'dilation': ndi.binary_dilation, 'closing': ndi.binary_closing, 'opening': ndi.binary_opening}


def ones(s):
    return np.ones((s,) * 3 if isinstance(s, int) else s, int)


def volume(shape, kind):
    rng = np.random.default_rng(17)
    if kind == 'sparse':                   # 2 %: the closing fills
        return rng.random(shape) < 0.02
    if kind == 'dense':
        return rng.random(shape) < 0.6
    if kind == 'zeros':
        return np.zeros(shape, bool)
    if kind == 'ones':
        return np.ones(shape, bool)
    a = np.zeros(shape, bool)              # 'corners': the eight corners and the two voxels on either side of a word boundary
    a[::shape[0] - 1, ::shape[1] - 1, ::shape[2] - 1] = True
    if shape[2] > W:
        a[shape[0] // 2, shape[1] // 2, W - 1] = True
        a[shape[0] // 2 - 1, shape[1] // 2 + 1, W] = True
    return a


KINDS = ['sparse', 'dense', 'zeros', 'ones', 'corners']


def reference(op, a, structure, **kw):
    """scipy.ndimage's binary operation. Its brute force takes about 5 s per call with the 29,791 taps of a 31 x 31 x 31 structure, whatever the
    volume holds; for that one box the closing is taken from scipy's maximum_filter and minimum_filter instead, which say the same for an odd
    all-ones window with false outside and are separable (test_box_31_against_binary_closing holds the two together once)."""
    if op == 'closing' and not kw and np.shape(structure) == (31, 31, 31) and np.all(structure):
        grown = ndi.maximum_filter(a, size=31, mode='constant', cval=0)
        return ndi.minimum_filter(grown, size=31, mode='constant', cval=0)
    return SCIPY[op](a, structure, **kw)


def check(op, a, structure, what, **kw):
    """device == scipy on dtype, shape and values; the input unchanged; a fresh array"""
    before = a.copy()
    got = DEVICE[op](a, structure, **kw)
    assert np.array_equal(a, before), '%s: the input was modified' % what
    ref = reference(op, a != 0, structure, **kw)
    assert got is not a and got.dtype == ref.dtype == np.bool_ and got.shape == ref.shape, (what, got.dtype, got.shape)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError('%s: %d of %d voxels differ, first at %s (got %d)' % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])]))
    return got


@pytest.mark.parametrize('s', BOXES, ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_box_closing(shape, s):
    for kind in KINDS:
        check('closing', volume(shape, kind), ones(s), 'closing %s of %s %s' % (s, kind, shape))


def test_box_31_against_binary_closing():
    a = volume(SHAPES[0], 'sparse')
    ref = ndi.binary_closing(a, ones(31))
    assert np.array_equal(reference('closing', a, ones(31)), ref)
    assert np.array_equal(BC.BinaryClose(a, ones(31)), ref)


def test_box_closing_volume_thinner_than_the_structure():
    for kind in KINDS:
        check('closing', volume((9, 10, 11), kind), ones(14), 'closing 14 of %s (9, 10, 11)' % kind)


def test_box_closing_erodes_the_faces():
    """an all-ones volume closed with 14 loses 14 // 2 = 7 layers at the low end and 14 - 1 - 7 = 6 at the high end of every axis"""
    shape = (2 * T + 2, 2 * T + 3, W + 6)
    got = check('closing', np.ones(shape, bool), ones(14), 'closing 14 of ones')
    want = np.zeros(shape, bool)
    want[7:-6, 7:-6, 7:-6] = True
    assert np.array_equal(got, want)
    for ax in range(3):
        g = np.moveaxis(got, ax, 0)
        assert not g[:7].any() and not g[-6:].any() and g[7:-6].any()


@pytest.mark.parametrize('border', [0, 1])
@pytest.mark.parametrize('s', [4, 5])
@pytest.mark.parametrize('op', ['erosion', 'dilation'])
def test_box_erosion_and_dilation(op, s, border):
    for shape in SHAPES:
        for kind in ('sparse', 'dense', 'corners'):
            check(op, volume(shape, kind), ones(s), '%s %d border %d of %s %s' % (op, s, border, kind, shape), border_value=border)


def general_structures():
    rng = np.random.default_rng(23)
    r = rng.random((5, 3, 7)) < 0.4
    r[2, 1, 3] = False                       # a false centre
    r[0, 0, 0] = r[4, 2, 6] = True
    h = np.ones((3, 3, 3), bool)
    h[0, 2, 0] = False                       # generate_binary_structure(3, 3) less one corner: not a box any more
    return {'c2': ndi.generate_binary_structure(3, 2), 'c3-less-a-corner': h, 'random-5x3x7': r}


@pytest.mark.parametrize('shape', SHAPES[2:], ids=str)
def test_general_path(shape):
    cross = ndi.generate_binary_structure(3, 1)
    st = general_structures()
    for kind in ('sparse', 'dense', 'corners'):
        a = volume(shape, kind)
        what = '%s %s' % (kind, shape)
        for it in (1, 6):
            check('dilation', a, cross, 'dilation cross x %d of %s' % (it, what), iterations=it)
        check('erosion', a, cross, 'erosion cross x 3 of ' + what, iterations=3)
        check('erosion', a, cross, 'erosion cross border 1 of ' + what, border_value=1)
        for name in st:
            for op in ('erosion', 'dilation', 'closing', 'opening'):
                check(op, a, st[name], '%s %s of %s' % (op, name, what))
        # generate_binary_structure(3, 3) is all ones: the box path takes it, so it runs here beside the general structures
        for op in ('erosion', 'dilation'):
            check(op, a, ndi.generate_binary_structure(3, 3), '%s c3 of %s' % (op, what))
        for op in ('opening', 'closing'):
            check(op, a, cross, '%s cross x 2 of %s' % (op, what), iterations=2)


def test_structure_none_is_the_cross():
    a = volume(SHAPES[3], 'dense')
    cross = ndi.generate_binary_structure(3, 1)
    for op in ('erosion', 'dilation', 'opening'):
        got = DEVICE[op](a, iterations=2)
        assert np.array_equal(got, SCIPY[op](a, cross, iterations=2)), op
    assert np.array_equal(BC.BinaryClose(a, None), ndi.binary_closing(a, cross))


def test_same_call_twice_and_input_forms():
    a = volume(SHAPES[3], 'sparse')
    st = ones((14, 13, 10))
    first = check('closing', a, st, 'closing, bool')
    assert np.array_equal(BC.BinaryClose(a, st), first)
    u = a.astype(np.uint8) * np.random.default_rng(1).integers(1, 256, a.shape).astype(np.uint8)      # true = any value of 1..255
    assert np.array_equal((u != 0), a)
    assert np.array_equal(check('closing', u, st, 'closing, uint8 1..255'), first)
    t = np.ascontiguousarray(a.transpose(2, 1, 0)).transpose(2, 1, 0)                                  # the same values, k slowest in memory
    assert not t.flags.c_contiguous
    assert np.array_equal(check('closing', t, st, 'closing, transposed'), first)
    assert BC.last_kernel_ms is not None and BC.last_kernel_ms > 0
    assert BC.InitBinaryClosing(DeviceName='no such device', GPUBackend='Metal')


def test_many_tiles():
    a = volume((96, 80, 200), 'sparse')
    check('closing', a, ones(14), 'closing 14 of sparse (96, 80, 200)')
