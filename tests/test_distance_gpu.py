"""The device distance transform (bfd_distance_transform_edt3d behind babelbrain_amd.DistanceTransform) held to EQUALITY with
scipy.ndimage.distance_transform_edt, element for element, for the float64 distances and the int32 squared distances; the device Gaussian filter
(bfd_gaussian_filter3d behind babelbrain_amd.GaussianFilter) held to a derived bound against scipy.ndimage.gaussian_filter in float64; and the chain
of the bone-rim correction (erosion, distance transform, two filters) on a synthetic head.

The bound: the weights are non-negative and sum to one, so each axis pass contracts the error already there and adds at most one rounding of a value
no larger than max|x| in magnitude: float32, |got - ref| <= 2^-24 max|x| (1 + 2^-20) per filtered axis; float64, (1 + 2 r + 2) 2^-53 max|x| per
filtered axis, the second term for the float64 sum's own error. No element is left out."""
import numpy as np
import pytest
from scipy import ndimage

from babelbrain_amd import BinaryClosing as BC, DistanceTransform as DT, GaussianFilter as GF

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------- the distance transform ----------------------------------------------------------

def _check_edt(mask, invert=False):
    ref = ndimage.distance_transform_edt((mask == 0) if invert else mask)
    d = DT.distance_transform_edt(mask, invert=invert)
    d2 = DT.distance_transform_edt(mask, invert=invert, squared=True)
    assert d.dtype == np.float64 and d2.dtype == np.int32 and d.shape == mask.shape
    assert np.array_equal(d2, np.rint(ref * ref).astype(np.int32))
    assert np.array_equal(d, ref)
    assert DT.last_kernel_ms > 0


@pytest.mark.parametrize('shape', [(9, 8, 7), (1, 1, 130), (130, 1, 1), (3, 70, 5), (33, 20, 66), (70, 9, 67), (64, 64, 64), (65, 63, 129), (2, 300, 2)])
def test_edt_equals_scipy(shape):
    for background in (0.5, 0.02, 0.98):
        rng = np.random.default_rng(shape[0] * 1000 + int(background * 100))
        mask = (rng.random(shape) >= background).astype(np.uint8)
        mask.flat[rng.integers(mask.size)] = 0
        _check_edt(mask)
    _check_edt(mask.astype(bool))
    _check_edt(mask.astype(np.float32) * 0.5, invert=True)


def test_edt_special_masks():
    corner = np.ones((12, 9, 70), np.uint8)
    corner[-1, 0, -1] = 0
    _check_edt(corner)
    plane = np.ones((10, 11, 13), np.uint8)
    plane[:, 4, :] = 0
    _check_edt(plane)
    rows = np.ones((6, 7, 130), np.uint8)                          # most rows without background, one plane without any
    rows[1, 2, 64:] = 0
    rows[4, 6, 0] = 0
    rows[5, 0, 129] = 0
    _check_edt(rows)
    for shape in ((16384, 1, 2), (1, 16384, 2), (2, 1, 16384)):      # the longest line there is: squared distances up to 16383^2 + 1
        far = np.ones(shape, np.uint8)
        far[0, 0, 0] = 0
        _check_edt(far)
        far[-1, -1, -1] = 0
        _check_edt(far)
    _check_edt(np.zeros((1, 1, 1), np.uint8))
    _check_edt(np.ones((1, 1, 1), np.uint8), invert=True)
    for shape in ((0, 5, 6), (4, 0, 6), (4, 5, 0)):                # the empty problem
        assert DT.distance_transform_edt(np.zeros(shape, np.uint8)).shape == shape
        assert DT.distance_transform_edt(np.zeros(shape, bool), squared=True).dtype == np.int32


def head_phantom(shape=(96, 80, 72)):
    """A ball of soft tissue inside a shell of bone, as ellipsoids in the grid: (radius function, the shell's mask)."""
    g = np.meshgrid(*[(np.arange(n) - (n - 1) / 2) / (n / 2) for n in shape], indexing='ij')
    rad = np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2)
    return rad, (rad < 0.85) & (rad >= 0.6)


def test_edt_ball_and_shell_inverted_and_repeatable():
    rad, shell = head_phantom()
    mask = (shell | (rad < 0.3)).astype(np.uint8)
    ref = ndimage.distance_transform_edt(1 - mask)
    a = DT.distance_transform_edt(mask, invert=True)
    b = DT.distance_transform_edt(mask, invert=True)
    assert np.array_equal(a, ref)
    assert a.tobytes() == b.tobytes()
    assert np.array_equal(DT.distance_transform_edt(mask, invert=True, squared=True), np.rint(ref * ref).astype(np.int32))


# ------------------------------------------------------------ the Gaussian filter ------------------------------------------------------------

def bound(x, sigma, truncate=4.0):
    sig = np.broadcast_to(np.asarray(sigma, np.float64), (3,))
    big = float(np.abs(x).max())
    if x.dtype == np.float32:
        return sum(1 for s in sig if s > 1e-15) * 2.0 ** -24 * big * (1 + 2.0 ** -20)
    return sum(1 + 2 * int(truncate * s + 0.5) + 2 for s in sig if s > 1e-15) * 2.0 ** -53 * big


DIFFER = {}        # elements on which the float32 result differs from scipy's float32 result, per case: a report, not a condition


def _check_gauss(x, sigma, mode='reflect', cval=0.0, truncate=4.0):
    assert abs(cval) <= np.abs(x).max()                            # cval is a sample of the extended line: the bound's max|x| covers it
    got = GF.gaussian_filter(x, sigma, mode=mode, cval=cval, truncate=truncate)
    assert got.dtype == x.dtype and got.shape == x.shape and GF.last_kernel_ms >= 0
    ref = ndimage.gaussian_filter(x.astype(np.float64), sigma, mode=mode, cval=cval, truncate=truncate)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    differ = int(np.count_nonzero(got != ndimage.gaussian_filter(x, sigma, mode=mode, cval=cval, truncate=truncate)))
    DIFFER[(x.shape, str(x.dtype), str(sigma), mode)] = differ
    print('%s %s sigma %s %s: max error %.3g, bound %.3g; %d elements differ from scipy in %s' % (x.shape, x.dtype, sigma, mode, err, bound(x, sigma, truncate),
                                                                                                 differ, x.dtype))
    assert err <= bound(x, sigma, truncate)
    return got


def _volume(shape, dtype, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.normal(300, 700, shape) * (rng.random(shape) < 0.5)).astype(dtype)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('mode', ['reflect', 'constant', 'nearest', 'mirror'])
def test_gaussian_within_the_bound(dtype, mode):
    _check_gauss(_volume((40, 37, 70), dtype), 3.0, mode, cval=-123.4)
    _check_gauss(_volume((5, 3, 130), dtype, 2), 1.0, mode, cval=77.7)
    _check_gauss(_volume((5, 3, 130), dtype, 2), 3.0, mode, cval=77.7)          # radius 12 on axes of 5 and 3: several reflections
    _check_gauss(_volume((33, 20, 66), dtype, 3), (3.0, 5.0, 3.0), mode, cval=1.0)
    _check_gauss(_volume((33, 20, 66), dtype, 3), (0.0, 2.0, 0.0), mode, cval=1.0)
    _check_gauss(_volume((1, 2, 3), dtype, 4), 3.0, mode, cval=-5.5)
    _check_gauss(_volume((7, 1, 65), dtype, 4), 2.0, mode, cval=-5.5)           # an axis of length 1 in the middle
    _check_gauss(_volume((9, 70, 1), dtype, 4), 2.0, mode, cval=-5.5)           # axis 1 is the contiguous one
    _check_gauss(_volume((130, 1, 1), dtype, 4), 2.0, mode, cval=-5.5)          # and axis 0


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_gaussian_large_radius_and_the_kernel_thresholds(dtype):
    """Radius 127; and the radii on either side of the switch between the tiled and the direct kernel on axes 0 and 1 (88 | 89 for float32, 40 | 41
    for float64), reached with truncate 1."""
    x = _volume((16, 16, 300), dtype, 5)
    _check_gauss(x, 31.75, 'reflect')
    lo = 88 if dtype == np.float32 else 40
    y = _volume((70, 6, 9), dtype, 6)
    for r in (lo, lo + 1):
        _check_gauss(y, (float(r), 0.0, 0.0), 'mirror', truncate=1.0)
        _check_gauss(y.transpose(1, 0, 2).copy(), (0.0, float(r), 0.0), 'reflect', truncate=1.0)


def test_gaussian_skips_and_copies():
    x = _volume((6, 7, 8), np.float32, 7)
    assert GF.gaussian_filter(x, 0.0).tobytes() == x.tobytes()
    assert GF.gaussian_filter(x, (0.0, 1e-16, 0.0)).tobytes() == x.tobytes()
    assert GF.gaussian_filter(x, 0.1).tobytes() == x.tobytes()                 # radius 0: one weight, 1.0
    assert GF.gaussian_filter(np.zeros((0, 4, 5), np.float64), 2.0).shape == (0, 4, 5)
    nc = _volume((8, 7, 6), np.float32, 8).transpose(2, 1, 0)                  # not contiguous
    _check_gauss(nc, 1.5)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_gaussian_constant_volume_and_impulse(dtype):
    c = np.full((20, 9, 70), 1234.5678, dtype)
    for mode in ('reflect', 'nearest', 'mirror'):
        got = _check_gauss(c, 3.0, mode)
        assert np.abs(got.astype(np.float64) - float(c[0, 0, 0])).max() <= bound(c, 3.0)
    x = np.zeros((31, 29, 70), dtype)
    x[15, 14, 35] = 1000.0
    got = _check_gauss(x, (2.0, 1.0, 3.0), 'constant')
    from scipy.ndimage._filters import _gaussian_kernel1d
    w = [_gaussian_kernel1d(s, 0, int(4 * s + 0.5)) for s in (2.0, 1.0, 3.0)]
    outer = 1000.0 * w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]
    box = got[15 - 8:15 + 9, 14 - 4:14 + 5, 35 - 12:35 + 13].astype(np.float64)
    assert np.abs(box - outer).max() <= bound(x, (2.0, 1.0, 3.0))
    got[15 - 8:15 + 9, 14 - 4:14 + 5, 35 - 12:35 + 13] = 0
    assert not got.any()                                                      # nothing outside the kernel's support


@pytest.mark.parametrize('sigma,truncate', [(3.0, 4.0), (5.0, 4.0), (2.0, 4.0), (0.7, 4.0), (31.75, 4.0), (16.3, 4.0), (7.123456789, 3.3)])
def test_library_weights_equal_scipy(sigma, truncate):
    """A float64 impulse of 1.0 under 'constant' returns the weights the library formed, untouched: every sum is 1.0 * w[d] plus zeros. Equality with
    scipy.ndimage's own kernel, along each axis."""
    from scipy.ndimage._filters import _gaussian_kernel1d
    radius = int(truncate * sigma + 0.5)
    want = _gaussian_kernel1d(sigma, 0, radius)
    n = 2 * radius + 1
    for axis in range(3):
        shape = [2, 2, 2]
        shape[axis] = n
        x = np.zeros(shape)
        centre = [1, 1, 1]
        centre[axis] = radius
        x[tuple(centre)] = 1.0
        sig = [0.0, 0.0, 0.0]
        sig[axis] = sigma
        got = GF.gaussian_filter(x, sig, mode='constant', truncate=truncate)
        line = [1, 1, 1]
        line[axis] = slice(None)
        assert np.array_equal(got[tuple(line)], want), axis


# ----------------------------------------------------------------- the chain -----------------------------------------------------------------

def _blend(ct, interior, dist, blur_val, blur_mask, sigma):
    """The host part of the correction, restated from its description: inside the rim (distance to the interior at most 2 sigma) the CT value moves
    towards the interior's local mean, blur_val / blur_mask where the blurred mask is above 1e-6, with a weight that falls linearly with the distance;
    the result is clipped to the CT range."""
    rim = (~interior) & (dist <= 2 * sigma) & (ct > 300)
    mean = np.where(blur_mask > 1e-6, blur_val / np.maximum(blur_mask, 1e-6), ct)
    wgt = np.clip(1.0 - dist / (2 * sigma), 0.0, 1.0)
    out = ct.astype(np.float64).copy()
    out[rim] = np.maximum(ct[rim], (wgt * mean + (1 - wgt) * ct)[rim])
    return np.clip(out, ct.min(), ct.max())


def test_bone_rim_chain():
    rad, shell = head_phantom()
    rng = np.random.default_rng(11)
    ct = np.where(rad < 0.6, 40.0, -1000.0) + rng.normal(0, 5, rad.shape)
    ct[shell] = 1200.0 + rng.normal(0, 60, int(shell.sum()))
    rim = ((rad >= 0.85) & (rad < 0.9)) | ((rad < 0.6) & (rad >= 0.55))
    ct[rim] = 600.0 + rng.normal(0, 100, int(rim.sum()))          # partial-volume values on both faces of the shell
    ct = ct.astype(np.float32)
    sigma = 3.0

    eroded = BC.BinaryErode(shell, np.ones((3, 3, 3)))
    want = ndimage.binary_erosion(shell, structure=np.ones((3, 3, 3)))
    assert np.array_equal(eroded.astype(bool), want)
    interior = eroded.astype(bool)
    dist = DT.distance_transform_edt(interior, invert=True)
    dist_ref = ndimage.distance_transform_edt(1 - want)
    assert np.array_equal(dist, dist_ref)

    interior_f = np.where(interior, ct, np.float32(0)).astype(np.float32)
    mask_f = interior.astype(np.float32)
    blur_val = _check_gauss(interior_f, sigma)
    blur_mask = _check_gauss(mask_f, sigma)
    ref_val = ndimage.gaussian_filter(interior_f, sigma=sigma)
    ref_mask = ndimage.gaussian_filter(mask_f, sigma=sigma)
    a = _blend(ct, interior, dist, blur_val, blur_mask, sigma)
    b = _blend(ct, interior, dist_ref, ref_val, ref_mask, sigma)
    print('bone-rim chain: corrected CT on device fields vs scipy fields, max difference %.3g (reported, not bounded); %d voxels changed by the correction'
          % (np.abs(a - b).max(), np.count_nonzero(b != ct)))
    assert np.count_nonzero(b != ct) > 0


def test_report_of_float32_differences():
    """Printed last: the elements on which the float32 results of this module's cases differ from scipy's float32 results (expected 0)."""
    total = sum(v for k, v in DIFFER.items() if k[1] == 'float32')
    print('float32 cases: %d, elements that differ from scipy in float32: %d' % (sum(1 for k in DIFFER if k[1] == 'float32'), total))
