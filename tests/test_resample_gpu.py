"""Spline resampling on the device against scipy.ndimage, element by element (tests/resample_cases.py holds the bound and the exclusions).
Largest |dev - ref| / A seen on an MI355X over the float64 results of this file: order 1 7.3e-15, order 2 1.2e-13, order 3 9.8e-14
("Resampling"); the bound's second term is 2^-32 = 2.3e-10."""
import numpy as np
import pytest

from babelbrain_amd import BinaryClosing, MedianFilter, Resample as R
from babelbrain_amd.nifti import SpatialImage
from tests import resample_cases as RC

pytestmark = pytest.mark.gpu
ndi = pytest.importorskip('scipy.ndimage')

GEN_IN, GEN_OUT = (40, 37, 45), (50, 44, 41)
MODES = ['constant', 'nearest', 'mirror']


def run(a, m, oshape, order, mode, cval=0.0, prefilter=True, gathered=False):
    return R.affine_transform(a, m[:, :3], m[:, 3], oshape, order=order, mode=mode, cval=cval, prefilter=prefilter, _gathered=gathered)


@pytest.mark.parametrize('dtype', list(RC.DTYPES))
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('order', [0, 1, 2, 3])
def test_generic_affine(order, mode, dtype):
    """About a third of the output lies outside the input; cval = -1000 (stored as 0 in uint8)."""
    a, m = RC.volume(GEN_IN, dtype), RC.generic_matrix()
    before = a.copy()
    dev = run(a, m, GEN_OUT, order, mode, -1000.0)
    assert np.array_equal(a, before)
    RC.check(dev, a, m, GEN_OUT, order, mode, -1000.0, max_excluded=0 if np.dtype(a.dtype).kind == 'f' and order else RC.MAX_EXCLUDED)
    if mode == 'constant':
        outside = RC.reference(a, m, GEN_OUT, 0, mode, -1000.0) == -1000.0
        assert 0.25 < outside.mean() < 0.45


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('order', [2, 3])
def test_prefilter_off_on_device_coefficients(order, mode):
    """spline_filter's coefficients through affine_transform(prefilter=False) give what the prefiltered call gives, within the bound.
    ('nearest' pads before its prefilter and spline_filter does not, as in scipy: the reference is scipy's for the same two calls.)"""
    a, m = RC.volume(GEN_IN, 'float64'), RC.generic_matrix()
    coef = R.spline_filter(a, order, mode)
    ref_coef = ndi.spline_filter(np.asarray(a), order, output=np.float64, mode=mode)
    amplitude = float(np.abs(a).max())
    assert coef.dtype == np.float64 and RC.violations(coef, ref_coef, amplitude) == 0
    dev = run(ref_coef, m, GEN_OUT, order, mode, -1000.0, prefilter=False)
    ref = RC.reference(ref_coef, m, GEN_OUT, order, mode, -1000.0, prefilter=False)
    assert RC.violations(dev, ref, amplitude) == 0


@pytest.mark.parametrize('dtype', ['float32', 'int16'])
@pytest.mark.parametrize('order', [0, 1, 2, 3])
def test_exactly_representable_transforms(order, dtype):
    """Identity, an integer shift, diag(0.5, 1, 1) onto 2 N - 1 samples (coordinates exactly on 0, on dim - 1 and on half-integers) and an
    axis flip: every coordinate is exact, so nothing may be left out."""
    shape = (21, 18, 23)
    a = RC.volume(shape, dtype)
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    dev = run(a, eye, shape, order, 'constant', -7.0)
    if order < 2:
        assert np.array_equal(dev, a)
    RC.check(dev, a, eye, shape, order, 'constant', -7.0, max_excluded=None)
    shift = eye.copy(); shift[:, 3] = [1, 2, 3]
    half = eye.copy(); half[0, 0] = 0.5
    flip = eye.copy(); flip[1, 1] = -1.0; flip[1, 3] = shape[1] - 1
    for m, oshape in ((shift, shape), (half, (2 * shape[0] - 1, shape[1], shape[2])), (flip, shape)):
        for mode in MODES:
            RC.check(run(a, m, oshape, order, mode, -7.0), a, m, oshape, order, mode, -7.0, max_excluded=None)
    assert np.array_equal(run(a, flip, shape, 0, 'constant'), a[:, ::-1, :])


@pytest.mark.parametrize('ishape,oshape', [((65, 33, 130), (63, 35, 129)), ((4, 4, 700), (4, 5, 701)), ((700, 3, 5), (699, 3, 6)),
                                           ((1, 2, 3), (2, 3, 4)), ((3, 1, 40), (4, 2, 37))], ids=str)
def test_tile_and_line_edges(ishape, oshape):
    """Dimensions that are no multiple of a wave or a tile, lines that cross many LDS tiles with carried state, axes of length 1, 2 and 3:
    the prefilter alone and the whole transform, orders 2 and 3 (and 0), every mode."""
    a = RC.volume(ishape, 'float64')
    amplitude = float(np.abs(a).max())
    m = np.hstack([np.diag([0.973, 1.021, 0.987]) * np.sqrt(1.01), np.array([[0.31], [-0.27], [0.43]]) * np.sqrt(2.0)])
    m[0, 1] = 0.0113; m[2, 0] = -0.0041
    for mode in MODES:
        for order in (2, 3):
            coef = R.spline_filter(a, order, mode)
            assert RC.violations(coef, ndi.spline_filter(np.asarray(a), order, output=np.float64, mode=mode), amplitude) == 0, (order, mode)
        for order in (0, 2, 3):
            RC.check(run(a, m, oshape, order, mode, 5.0), a, m, oshape, order, mode, 5.0)


@pytest.mark.parametrize('scale', [3.0, 1.0 / 3.0], ids=['scale3', 'scale1/3'])
def test_both_scales(scale):
    """Scale 3: neighbouring outputs lie three samples apart and the source box of a 4 x 8 x 32 tile (about 13 x 25 x 97 coefficients)
    exceeds the LDS box, so order 3 gathers; scale 1/3: the box is small and is staged. The same bound holds."""
    ishape = (60, 50, 200) if scale > 1 else (24, 20, 40)
    oshape = (20, 17, 66) if scale > 1 else (70, 58, 118)
    a = RC.volume(ishape, 'float32')
    m = RC.scale_matrix(scale, ishape, oshape)
    for order in (1, 3):
        RC.check(run(a, m, oshape, order, 'constant', -1.0), a, m, oshape, order, 'constant', -1.0)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', ['int16', 'float64'])
def test_staged_equals_gathered(dtype, mode):
    """Order 3 with the source box of each output tile staged in LDS (the default) and gathered from global memory: the same bits. The
    generic map (tiles inside, across the border and outside; partial tiles) and a near-unit scale of a volume with many tiles."""
    a, m = RC.volume(GEN_IN, dtype), RC.generic_matrix()
    assert np.array_equal(run(a, m, GEN_OUT, 3, mode, -1000.0), run(a, m, GEN_OUT, 3, mode, -1000.0, gathered=True))
    ishape, oshape = (65, 33, 130), (63, 35, 129)
    b = RC.volume(ishape, dtype)
    m2 = RC.scale_matrix(1.03, ishape, oshape)
    staged = run(b, m2, oshape, 3, mode, -1000.0)
    assert np.array_equal(staged, run(b, m2, oshape, 3, mode, -1000.0, gathered=True))
    RC.check(staged, b, m2, oshape, 3, mode, -1000.0)
    coef = np.asarray(RC.volume(ishape, 'float32'))                       # prefilter off: the box is staged from the input's own dtype
    assert np.array_equal(run(coef, m2, oshape, 3, mode, 0.0, prefilter=False), run(coef, m2, oshape, 3, mode, 0.0, prefilter=False, gathered=True))


@pytest.mark.parametrize('dtype', list(RC.DTYPES))
def test_all_outside(dtype):
    a = RC.volume(GEN_IN, dtype)
    m = np.hstack([np.eye(3), 10.0 * np.array(GEN_IN, np.float64).reshape(3, 1)])
    dev = run(a, m, GEN_OUT, 3, 'constant', 42.0)
    assert dev.dtype == a.dtype and np.all(dev == 42)


def _ct():
    shape, tshape = (48, 52, 40), (60, 56, 64)
    ct = (RC.volume(shape, 'float64') * 4.0 + 200.0).astype(np.int16)
    r2 = np.sqrt(2.0)                                    # origins that put no coordinate on a half-integer
    A = np.array([[-0.6, 0.0, 0.0, 14.0 + r2 / 7], [0.0, 0.6, 0.0, -15.0 - r2 / 5], [0.0, 0.0, 1.2, -22.0 - r2 / 9], [0.0, 0.0, 0.0, 1.0]])      # axis 0 flipped
    B = np.array([[0.5, 0.0, 0.0, -15.5 + r2 / 11], [0.0, 0.5, 0.0, -14.0 + r2 / 13], [0.0, 0.0, 0.5, -20.0 - r2 / 17], [0.0, 0.0, 0.0, 1.0]])
    return ct, A, B, tshape


@pytest.mark.parametrize('order', [3, 0])
def test_resample_from_to_end_to_end(order):
    """An int16 CT of 0.6 x 0.6 x 1.2 mm with a flip onto a 0.5 mm grid, as BabelDatasetPreps.py:859 (order 3, cval = min) and :1168 (order 0)."""
    ct, A, B, tshape = _ct()
    before = ct.copy()
    cval = float(ct.min()) if order == 3 else 0.0
    header = {'descrip': 'ct'}
    res = R.ResampleFromTo(SpatialImage(ct, A, header), (tshape, B), order=order, mode='constant', cval=cval)
    assert np.array_equal(ct, before)
    assert isinstance(res, SpatialImage) and res.header is header and np.array_equal(res.affine, B) and res.shape == tshape
    T = np.linalg.inv(A) @ B
    RC.check(res.dataobj, ct, T[:3, :], tshape, order, 'constant', cval)
    res2 = R.ResampleFromTo(SpatialImage(ct, A, header), SpatialImage(np.zeros(tshape, np.uint8), B), order=order, cval=cval)
    assert np.array_equal(res2.dataobj, res.dataobj)


def test_chain_with_median_and_closing():
    """The resampled CT thresholded, median-filtered and closed equals the same chain on scipy's resample, voxel for voxel."""
    ct, A, B, tshape = _ct()
    T = np.linalg.inv(A) @ B
    cval = float(ct.min())
    dev = R.ResampleFromTo(SpatialImage(ct, A), (tshape, B), order=3, cval=cval).dataobj
    ref = RC.convert(RC.reference(ct, T[:3, :], tshape, 3, 'constant', cval), np.int16)

    def chain(v):
        return BinaryClosing.BinaryClose(MedianFilter.MedianFilter((v > 300).astype(np.uint8), 3), structure=np.ones((3, 3, 3), bool))
    assert np.array_equal(chain(dev), chain(ref))
