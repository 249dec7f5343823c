"""The resampling without a GPU: argument errors before the library is loaded, the matrix forms, the affine composition of ResampleFromTo,
the two ABI entries' refusals before any device, the B-spline weights of the core header, and the sensitivity of the device tests' comparison."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from babelbrain_amd import Resample as R, _engine
from babelbrain_amd.nifti import SpatialImage
from tests import resample_cases as RC


@pytest.fixture
def no_library(monkeypatch):
    """Loading the library is an error here: the refusals below must come first."""
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_engine, 'load_library', boom)


V = np.zeros((6, 7, 8), np.float32)
EYE = np.eye(3)


@pytest.mark.parametrize('order,exc', [(4, NotImplementedError), (5, NotImplementedError), (6, ValueError), (-1, ValueError), (1.5, ValueError),
                                        ('3', ValueError), (None, ValueError)], ids=str)
def test_bad_order(no_library, order, exc):
    with pytest.raises(exc):
        R.affine_transform(V, EYE, order=order)
    with pytest.raises(exc):
        R.spline_filter(V, order=order)
    with pytest.raises(exc):
        R.ResampleFromTo(SpatialImage(V, np.eye(4)), (V.shape, np.eye(4)), order=order)


@pytest.mark.parametrize('mode,exc', [('reflect', NotImplementedError), ('wrap', NotImplementedError), ('grid-constant', NotImplementedError),
                                       ('grid-wrap', NotImplementedError), ('grid-mirror', NotImplementedError), ('edge', ValueError), (None, ValueError)], ids=str)
def test_bad_mode(no_library, mode, exc):
    with pytest.raises(exc):
        R.affine_transform(V, EYE, mode=mode)
    with pytest.raises(exc):
        R.spline_filter(V, mode=mode)
    with pytest.raises(exc):
        R.ResampleFromTo(SpatialImage(V, np.eye(4)), (V.shape, np.eye(4)), mode=mode)


@pytest.mark.parametrize('dtype', [np.uint16, np.int8, np.int32, np.int64, np.float16, np.complex64, np.bool_])
def test_bad_dtype(no_library, dtype):
    with pytest.raises(TypeError):
        R.affine_transform(np.zeros((4, 4, 4), dtype), EYE)
    with pytest.raises(TypeError):
        R.spline_filter(np.zeros((4, 4, 4), dtype))


def test_other_refusals(no_library):
    with pytest.raises(ValueError):
        R.affine_transform(np.zeros((4, 4), np.float32), EYE)                       # not 3-D
    with pytest.raises(ValueError):
        R.spline_filter(np.zeros((2, 4, 4, 4), np.float32))
    for bad in (np.eye(2), np.zeros((3, 5)), np.zeros(4), np.zeros((4, 3)), 2.0):
        with pytest.raises(ValueError):
            R.affine_transform(V, bad)
    with pytest.raises(ValueError):
        R.affine_transform(V, np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 1.0]]))      # last row of a homogeneous matrix
    with pytest.raises(ValueError):
        R.affine_transform(V, EYE * np.nan)
    with pytest.raises(ValueError):
        R.affine_transform(V, EYE, offset=[1, 2])
    with pytest.raises(ValueError):
        R.affine_transform(V, EYE, offset=np.inf)
    for shape in ((4, 4), (4, 4, -1), (1 << 11, 1 << 10, 1 << 10), 'abc', 5):
        with pytest.raises(ValueError):
            R.affine_transform(V, EYE, output_shape=shape)
    for cval in (np.nan, np.inf, -np.inf):
        for dtype in (np.int16, np.uint8):
            with pytest.raises(NotImplementedError):
                R.affine_transform(np.zeros((4, 4, 4), dtype), EYE, cval=cval)
    with pytest.raises(TypeError):
        R.affine_transform(V, EYE, output=np.zeros_like(V))                         # output= is not taken
    with pytest.raises(NotImplementedError):
        R.ResampleFromTo(SpatialImage(np.zeros((4, 4, 4, 2), np.float32), np.eye(4)), ((4, 4, 4), np.eye(4)))
    with pytest.raises(NotImplementedError):
        R.ResampleFromTo(SpatialImage(V, np.eye(4)), ((4, 4, 4, 2), np.eye(4)))
    with pytest.raises(ValueError):
        R.ResampleFromTo(SpatialImage(V, np.eye(4)), ((4, 4, 4), np.eye(3)))
    with pytest.raises(ValueError):
        R.ResampleFromTo(SpatialImage(V, np.eye(4)), 7)


def test_good_arguments_reach_the_library(no_library):
    """A strided view, every dtype and a finite cval get as far as the library (which this fixture forbids)."""
    v = np.arange(6 * 7 * 8, dtype=np.float64).reshape(6, 7, 8).transpose(2, 0, 1)
    a, m, shape, o, mc, cval = R._checked(v, EYE, 0.0, None, 3, 'mirror', 2)
    assert a.flags.c_contiguous and np.array_equal(a, v) and shape == (8, 6, 7) and (o, mc, cval) == (3, 2, 2.0)
    for dtype in (np.float32, np.float64, np.int16, np.uint8):
        with pytest.raises(AssertionError, match='library was loaded'):
            R.affine_transform(np.zeros((4, 4, 4), dtype), EYE, cval=-1000)
    with pytest.raises(AssertionError, match='library was loaded'):
        R.spline_filter(V)
    with pytest.raises(AssertionError, match='library was loaded'):
        R.affine_transform(V, EYE, cval=np.nan)                                      # float dtypes take any cval


def test_matrix_forms():
    """(3, 3) with an offset, (3, 4) and (4, 4) give the same twelve doubles; (3,) is a diagonal."""
    rng = np.random.default_rng(3)
    M, off = rng.standard_normal((3, 3)), rng.standard_normal(3)
    want = np.hstack([M, off[:, None]])
    h = np.eye(4); h[:3] = want
    for got in (R.normalize_matrix(M, off), R.normalize_matrix(want), R.normalize_matrix(h), R.normalize_matrix(want, offset=99.0),
                R.normalize_matrix(M.tolist(), list(off))):
        assert got.dtype == np.float64 and got.shape == (3, 4) and got.flags.c_contiguous and np.array_equal(got, want)
    d = rng.standard_normal(3)
    assert np.array_equal(R.normalize_matrix(d, off), R.normalize_matrix(np.diag(d), off))
    assert np.array_equal(R.normalize_matrix(d, 2.5)[:, 3], [2.5, 2.5, 2.5])


def _affines():
    A = np.array([[-0.6, 0.05, 0.0, 14.0], [0.02, 0.6, -0.1, -15.0], [0.0, 0.03, -1.2, 22.0], [0.0, 0.0, 0.0, 1.0]])      # two flips and shear
    B = np.array([[0.5, 0.0, 0.04, -15.5], [0.0, -0.5, 0.0, 14.0], [0.01, 0.0, 0.5, -20.0], [0.0, 0.0, 0.0, 1.0]])
    return A, B


def test_affine_composition():
    A, B = _affines()
    M, off = R.vox2vox(A, B)
    T = np.linalg.inv(A) @ B
    assert np.array_equal(M, T[:3, :3]) and np.array_equal(off, T[:3, 3])
    p = np.array([3.0, 4.0, 5.0, 1.0])                    # an output voxel and its input voxel name the same point
    assert np.allclose(A @ np.append(M @ p[:3] + off, 1.0), B @ p, atol=1e-12)
    with pytest.raises(ValueError):
        R.vox2vox(np.eye(3), B)


def test_resample_from_to_forms_and_out_class(monkeypatch):
    """The (shape, affine) pair and the image form give the same call and the same result; out_class receives (data, to_affine, header).
    The device call is replaced by scipy here: this is about the plumbing."""
    ndi = pytest.importorskip('scipy.ndimage')
    calls = []

    def fake(input, matrix, offset=0.0, output_shape=None, order=3, mode='constant', cval=0.0, prefilter=True):
        calls.append((np.array(matrix), np.array(offset), tuple(output_shape), order, mode, cval))
        return ndi.affine_transform(input, matrix, offset, output_shape, order=order, mode=mode, cval=cval)
    monkeypatch.setattr(R, 'affine_transform', fake)
    A, B = _affines()
    data = np.asarray(RC.volume((12, 11, 10), 'int16'))
    header = object()
    img = SpatialImage(data, A, header)
    r1 = R.ResampleFromTo(img, ((9, 8, 7), B), order=1, cval=-3)
    r2 = R.ResampleFromTo(img, SpatialImage(np.zeros((9, 8, 7), np.uint8), B), order=1, cval=-3, GPUBackend='OpenCL')
    assert isinstance(r1, SpatialImage) and r1.header is header and np.array_equal(r1.affine, B) and r1.shape == (9, 8, 7)
    assert r1.dataobj.dtype == np.int16 and np.array_equal(r1.dataobj, r2.dataobj) and np.array_equal(r1.get_fdata(), r1.dataobj.astype(np.float64))
    T = np.linalg.inv(A) @ B
    for c in calls:
        assert np.array_equal(c[0], T[:3, :3]) and np.array_equal(c[1], T[:3, 3]) and c[2:] == ((9, 8, 7), 1, 'constant', -3)
    got = R.ResampleFromTo(img, ((9, 8, 7), B), out_class=lambda *a: a)
    assert len(got) == 3 and got[0].shape == (9, 8, 7) and np.array_equal(got[1], B) and got[2] is header


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


def test_library_refuses_bad_arguments_before_any_device(lib):
    """Both entries report argument errors (rc -1) before they look for a device; nothing is read or written."""
    for name in ('bfd_affine_transform3d', 'bfd_spline_filter3d'):
        assert name in _engine.ABI_SYMBOLS and hasattr(lib, name)
    a, o, co = np.zeros(64, np.float32), np.full(64, 7, np.float32), np.full(64, 7, np.float64)
    m = np.ascontiguousarray(np.hstack([np.eye(3), np.zeros((3, 1))]))
    pa, po, pm, pc = _engine._ptr(a), _engine._ptr(o), _engine._ptr(m), _engine._ptr(co)
    bad_m = m.copy(); bad_m[1, 2] = np.nan

    def affine(dtype=1, i=pa, out=po, N=(4, 4, 4), O=(4, 4, 4), mat=pm, order=3, mode=0, cval=0.0, flags=1):
        return lib.bfd_affine_transform3d(0, dtype, i, out, N[0], N[1], N[2], O[0], O[1], O[2], mat, order, mode, cval, flags, None)

    def filt(dtype=1, i=pa, out=pc, N=(4, 4, 4), order=3, mode=0):
        return lib.bfd_spline_filter3d(0, dtype, i, out, N[0], N[1], N[2], order, mode, None)
    big = (1 << 11, 1 << 10, 1 << 10)
    for kw, word in ((dict(i=None), 'null'), (dict(out=None), 'null'), (dict(mat=None), 'null'), (dict(out=pa), 'alias'), (dict(order=4), 'order'),
                     (dict(order=-1), 'order'), (dict(mode=3), 'mode'), (dict(mode=-1), 'mode'), (dict(dtype=4), 'dtype'), (dict(dtype=-1), 'dtype'),
                     (dict(N=(4, -4, 4)), 'negative'), (dict(O=(4, 4, -1)), 'negative'), (dict(N=big), '2^31'), (dict(O=big), '2^31'),
                     (dict(O=(1 << 40, 1 << 40, 1 << 40)), '2^31'), (dict(mat=_engine._ptr(bad_m)), 'finite'), (dict(dtype=2, cval=float('nan')), 'cval'), (dict(flags=4), 'flags')):
        assert affine(**kw) == -1, kw
        assert word in lib.bfd_last_error().decode(), (kw, lib.bfd_last_error().decode())
    half = _engine._ptr(a[16:])                                                    # partial overlap of the two buffers
    assert lib.bfd_affine_transform3d(0, 1, pa, half, 4, 4, 2, 4, 4, 2, pm, 1, 0, 0.0, 1, None) == -1 and 'alias' in lib.bfd_last_error().decode()
    for kw, word in ((dict(i=None), 'null'), (dict(out=None), 'null'), (dict(i=pc), 'alias'), (dict(order=4), 'order'), (dict(mode=3), 'mode'),
                     (dict(dtype=7), 'dtype'), (dict(N=(-1, 4, 4)), 'negative'), (dict(N=big), '2^31')):
        assert filt(**kw) == -1, kw
        assert word in lib.bfd_last_error().decode(), (kw, lib.bfd_last_error().decode())
    assert np.all(a == 0) and np.all(o == 7) and np.all(co == 7)


def _closed_form(order, x):
    """Centred cardinal B-spline of degree `order` at distance x, float64."""
    x = abs(x)
    if order == 1:
        return max(1.0 - x, 0.0)
    if order == 2:
        return 0.75 - x * x if x <= 0.5 else (0.5 * (1.5 - x) ** 2 if x <= 1.5 else 0.0)
    return (4.0 - 6.0 * x * x + 3.0 * x ** 3) / 6.0 if x <= 1.0 else ((2.0 - x) ** 3 / 6.0 if x <= 2.0 else 0.0)


WEIGHTS_PROGRAM = r"""
#include "bfd_resample_core.h"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char **argv)
{   // argv: order, then coordinates; one line per coordinate: first tap, then the order + 1 weights, as hexadecimal floats
    const int order = atoi(argv[1]);
    for (int a = 2; a < argc; a++) {
        const double c = strtod(argv[a], 0);
        double w[4];
        rs_weights(c, order, w);
        printf("%ld", rs_first_tap(c, order));
        for (int t = 0; t <= order; t++) printf(" %a", w[t]);
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope='module')
def weights_program(tmp_path_factory):
    """bfd_resample_core.h compiled for the host by a plain C++ compiler, as its first lines say it can be."""
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx, 'no C++ compiler found'
    d = tmp_path_factory.mktemp('weights')
    src = d / 'weights.cpp'
    src.write_text(WEIGHTS_PROGRAM)
    exe = str(d / 'weights')
    subprocess.run([cxx, '-O1', '-ffp-contract=off', '-I', os.path.join(os.path.dirname(_engine.LIB_PATH), 'csrc'), str(src), '-o', exe, '-lm'], check=True)
    return exe


@pytest.mark.parametrize('order', [1, 2, 3])
def test_core_weights(weights_program, order):
    """The weights the kernels use (bfd_resample_core.h): they sum to 1, they are the B-spline at the taps' distances, and the first tap is
    floor(c) - order // 2 (odd orders) or floor(c + 0.5) - order // 2 (even)."""
    rng = np.random.default_rng(order)
    cs = [float(c) for c in rng.uniform(-3.0, 50.0, 400)] + [0.0, 0.5, 1.0, 7.5, 7.25, 41.0, -0.5, -2.0]
    r = subprocess.run([weights_program, str(order)] + [c.hex() for c in cs], capture_output=True, text=True, check=True)
    lines = r.stdout.split('\n')[:len(cs)]
    assert len(lines) == len(cs)
    for c, line in zip(cs, lines):
        f = line.split()
        first, w = int(f[0]), np.array([float.fromhex(x) for x in f[1:]])
        assert len(w) == order + 1
        assert first == int(np.floor(c if order & 1 else c + 0.5)) - order // 2
        assert abs(w.sum() - 1.0) <= 4e-16
        want = [_closed_form(order, c - (first + t)) for t in range(order + 1)]
        assert np.allclose(w, want, rtol=0, atol=1e-15), (c, w, want)


def test_comparison_reports_float32_coefficients_and_float32_matrix():
    """The two faults the bound is there to reject, planted into scipy's own pipeline on the CPU: B-spline coefficients rounded to float32,
    and a float32 matrix and offset. The comparison of the device tests reports both, for float64 and for float32 results; and it passes
    scipy's own float32 and integer outputs (the bound is not tighter than one rounding)."""
    ndi = pytest.importorskip('scipy.ndimage')
    a = np.asarray(RC.volume((40, 37, 45), 'float32'), np.float64)
    m, oshape = RC.generic_matrix(), (50, 44, 41)
    amplitude = float(np.abs(a).max())
    ref = RC.reference(a, m, oshape, 3, 'constant', -1000.0)
    coef32 = ndi.spline_filter(a, 3, output=np.float64, mode='mirror').astype(np.float32).astype(np.float64)
    f_coef = ndi.affine_transform(coef32, m[:, :3], m[:, 3], oshape, output=np.float64, order=3, cval=-1000.0, prefilter=False)
    m32 = m.astype(np.float32).astype(np.float64)
    f_mat = ndi.affine_transform(a, m32[:, :3], m32[:, 3], oshape, output=np.float64, order=3, cval=-1000.0)
    inside = ref != -1000.0
    for name, faulty in (('float32 coefficients', f_coef), ('float32 matrix', f_mat)):
        skip = ~inside | (faulty == -1000.0)              # not the voxels where the fault moves the cval decision: the values
        err = np.abs(faulty - ref)[~skip].max() / amplitude
        print('%s: max |fault - ref| / A = %.3e' % (name, err))
        assert err > 2.0 ** -32
        assert RC.violations(faulty, ref, amplitude, skip=skip) > 0, name
        assert RC.violations(faulty.astype(np.float32), ref, amplitude, skip=skip) > 0, name
    assert RC.violations(ref, ref, amplitude) == 0 and RC.violations(ref.astype(np.float32), ref, amplitude) == 0
    for dtype in ('float32', 'int16', 'uint8'):
        v = np.asarray(RC.volume((40, 37, 45), dtype))
        r = RC.reference(v, m, oshape, 3, 'constant', -1000.0)
        own = ndi.affine_transform(v, m[:, :3], m[:, 3], oshape, order=3, cval=-1000.0)
        skip = RC.excluded(m, v.shape, oshape, 3, 'constant', r, v.dtype)
        assert skip.sum() <= RC.MAX_EXCLUDED and RC.violations(own, r, float(np.abs(v.astype(np.float64)).max()), skip=skip) == 0, dtype


def test_generic_cases_exclude_few_voxels():
    """The exclusions of the generic device case, computed on the CPU: at most MAX_EXCLUDED voxels for every order, mode and dtype."""
    pytest.importorskip('scipy.ndimage')
    m, oshape = RC.generic_matrix(), (50, 44, 41)
    for dtype in RC.DTYPES:
        v = RC.volume((40, 37, 45), dtype)
        for mode in ('constant', 'nearest', 'mirror'):
            for order in range(4):
                ref = RC.reference(v, m, oshape, order, mode, -1000.0)
                assert RC.excluded(m, v.shape, oshape, order, mode, ref, v.dtype).sum() <= RC.MAX_EXCLUDED, (dtype, mode, order)
