"""Distance transform and Gaussian filter without a GPU: bfd_distance_core.h, compiled for the host and run serially, equals scipy voxel for voxel
(squared distances, their roots, the Gaussian weights) and stays within the derived bound for the filter; the C ABI refuses bad arguments before it
looks for a device and writes nothing on any refusal; the Python wrappers raise what they say they raise before the library is loaded."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from babelbrain_amd import DistanceTransform as DT, GaussianFilter as GF, _engine

CORE_PROGRAM = r"""
#include "bfd_distance_core.h"
#include <stdio.h>
#include <string.h>
#include <vector>

static bool read_all(const char *path, std::vector<char> &b)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    b.resize((size_t)n);
    const bool ok = fread(b.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}

template <typename T>
static void gauss_axis(const T *in, T *out, int64_t outer, int64_t m, int64_t inner, const double *w, int r, int mode, double cval)
{
    for (int64_t o = 0; o < outer; o++)
        for (int64_t x = 0; x < inner; x++) {
            const T *line = in + o * m * inner + x;
            for (int64_t u = 0; u < m; u++) {
                auto tap = [&](int d) {
                    const int64_t s = gauss_edge_index(u + d, m, mode);
                    return s < 0 ? cval : (double)line[s * inner];
                };
                out[(o * m + u) * inner + x] = (T)gauss_sum(tap, w, r);
            }
        }
}

template <typename T>
static int gauss(const int64_t *N, int mode, const double *sigma, double truncate, double cval, const char *data, FILE *f)
{
    const int64_t n = N[0] * N[1] * N[2];
    std::vector<T> a((size_t)n), b((size_t)n);
    memcpy(a.data(), data, (size_t)n * sizeof(T));
    for (int ax = 0; ax < 3; ax++) {
        if (!(sigma[ax] > 1e-15)) continue;
        const int r = gauss_radius(sigma[ax], truncate);
        if (r < 0) return 20;
        double w[GAUSS_MAX_RADIUS + 1];
        gauss_weights(sigma[ax], r, w);
        const int64_t outer = ax == 0 ? 1 : (ax == 1 ? N[0] : N[0] * N[1]);
        const int64_t inner = ax == 0 ? N[1] * N[2] : (ax == 1 ? N[2] : 1);
        gauss_axis<T>(a.data(), b.data(), outer, N[ax], inner, w, r, mode, cval);
        a.swap(b);
    }
    return fwrite(a.data(), sizeof(T), (size_t)n, f) == (size_t)n ? 0 : 21;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    std::vector<char> b;
    if (!read_all(argv[2], b)) return 3;
    FILE *f = fopen(argv[3], "wb");
    if (!f) return 4;
    int rc = 0;
    if (!strcmp(argv[1], "edt")) {
        int64_t h[4];
        memcpy(h, b.data(), sizeof h);
        const int64_t N1 = h[0], N2 = h[1], N3 = h[2], n = N1 * N2 * N3, W = edt_row_words(N3);
        const bool invert = h[3] & 1;
        const uint8_t *in = (const uint8_t *)b.data() + sizeof h;
        std::vector<uint64_t> bits((size_t)(N1 * N2 * W), 0);
        for (int64_t v = 0; v < n; v++)
            if ((in[v] != 0) == invert) bits[(size_t)(v / N3 * W + (v % N3 >> 6))] |= (uint64_t)1 << (v % N3 & 63);
        std::vector<int32_t> d2((size_t)n);
        for (int64_t v = 0; v < n; v++) d2[(size_t)v] = edt_row_dist2(&bits[(size_t)(v / N3 * W)], W, v % N3);
        std::vector<edt_site> stack((size_t)n);
        for (int64_t L = 0; L < N1 * N3; L++)       // along j, the lines laid out as the kernel has them
            edt_line(d2.data() + L / N3 * N2 * N3 + L % N3, N3, (int)N2, stack.data() + L, N1 * N3);
        for (int64_t L = 0; L < N2 * N3; L++)       // along i
            edt_line(d2.data() + L, N2 * N3, (int)N1, stack.data() + L, N2 * N3);
        std::vector<double> d((size_t)n);
        for (int64_t v = 0; v < n; v++) d[(size_t)v] = sqrt((double)d2[(size_t)v]);
        if (fwrite(d2.data(), 4, (size_t)n, f) != (size_t)n || fwrite(d.data(), 8, (size_t)n, f) != (size_t)n) rc = 10;
    } else if (!strcmp(argv[1], "weights")) {
        double p[2];
        memcpy(p, b.data(), sizeof p);
        const int64_t r = gauss_radius(p[0], p[1]);
        double w[GAUSS_MAX_RADIUS + 1];
        if (r >= 0) gauss_weights(p[0], (int)r, w);
        if (fwrite(&r, 8, 1, f) != 1 || (r >= 0 && fwrite(w, 8, (size_t)r + 1, f) != (size_t)r + 1)) rc = 11;
    } else if (!strcmp(argv[1], "exp")) {
        const size_t n = b.size() / 8;
        std::vector<double> x(n), y(n);
        memcpy(x.data(), b.data(), n * 8);
        const bool vec = gauss_numpy_vector_exp();
        for (size_t i = 0; i < n; i++) y[i] = gauss_exp(x[i], vec);
        if (fwrite(y.data(), 8, n, f) != n) rc = 12;
    } else if (!strcmp(argv[1], "gauss")) {
        int64_t h[5];
        double p[5];
        memcpy(h, b.data(), sizeof h);
        memcpy(p, b.data() + sizeof h, sizeof p);
        const char *data = b.data() + sizeof h + sizeof p;
        rc = h[3] == 1 ? gauss<float>(h, (int)h[4], p, p[3], p[4], data, f) : gauss<double>(h, (int)h[4], p, p[3], p[4], data, f);
    } else rc = 5;
    fclose(f);
    return rc;
}
"""


@pytest.fixture(scope='module')
def core(tmp_path_factory):
    """bfd_distance_core.h compiled for the host by a plain C++ compiler, as its first lines say it can be."""
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx, 'no C++ compiler found'
    d = tmp_path_factory.mktemp('distcore')
    src = d / 'distcore.cpp'
    src.write_text(CORE_PROGRAM)
    exe = str(d / 'distcore')
    subprocess.run([cxx, '-O1', '-std=c++14', '-ffp-contract=off', '-I', os.path.join(os.path.dirname(_engine.LIB_PATH), 'csrc'), str(src), '-o', exe, '-lm'],
                   check=True)

    class Core:
        @staticmethod
        def _run(what, payload):
            inp, out = str(d / 'in.bin'), str(d / 'out.bin')
            with open(inp, 'wb') as f:
                f.write(payload)
            subprocess.run([exe, what, inp, out], check=True)
            return out

        def edt(self, mask, invert=False):
            m = np.ascontiguousarray(mask, np.uint8)
            out = self._run('edt', np.array(list(m.shape) + [int(invert)], np.int64).tobytes() + m.tobytes())
            d2 = np.fromfile(out, np.int32, m.size).reshape(m.shape)
            return d2, np.fromfile(out, np.float64, m.size, offset=4 * m.size).reshape(m.shape)

        def weights(self, sigma, truncate):
            out = self._run('weights', np.array([sigma, truncate], np.float64).tobytes())
            r = int(np.fromfile(out, np.int64, 1)[0])
            return r, (np.fromfile(out, np.float64, r + 1, offset=8) if r >= 0 else None)

        def exp(self, x):
            return np.fromfile(self._run('exp', np.ascontiguousarray(x, np.float64).tobytes()), np.float64)

        def gauss(self, x, sigma, mode, cval=0.0, truncate=4.0):
            x = np.ascontiguousarray(x)
            head = np.array(list(x.shape) + [1 if x.dtype == np.float32 else 3, GF._MODES[mode]], np.int64).tobytes()
            par = np.array(list(np.broadcast_to(np.asarray(sigma, np.float64), (3,))) + [truncate, cval], np.float64).tobytes()
            return np.fromfile(self._run('gauss', head + par + x.tobytes()), x.dtype).reshape(x.shape)
    return Core()


# ---------------------------------------------------------- the distance transform ----------------------------------------------------------

def _brute_force(mask):
    bg = np.argwhere(mask == 0)
    pts = np.argwhere(np.ones(mask.shape, bool))
    return ((pts[:, None, :] - bg[None, :, :]) ** 2).sum(-1).min(1).reshape(mask.shape)


def _check_edt(core, mask, invert=False):
    ref = ndimage.distance_transform_edt((mask == 0) if invert else mask)
    d2, d = core.edt(mask, invert)
    assert np.array_equal(d2, np.rint(ref * ref).astype(np.int32))
    assert np.array_equal(d, ref)
    return ref


def test_core_header_against_brute_force(core):
    mask = (np.random.default_rng(0).random((9, 8, 7)) < 0.8).astype(np.uint8)
    ref = _check_edt(core, mask)
    assert np.array_equal(np.rint(ref * ref).astype(np.int64), _brute_force(mask))        # scipy itself, held to the definition


@pytest.mark.parametrize('shape', [(1, 1, 130), (130, 1, 1), (3, 70, 5), (33, 20, 66)])
@pytest.mark.parametrize('background', [0.5, 0.02, 0.98])
def test_core_header_equals_scipy(core, shape, background):
    rng = np.random.default_rng(shape[0] * 1000 + int(background * 100))
    mask = (rng.random(shape) >= background).astype(np.uint8)
    mask.flat[rng.integers(mask.size)] = 0                         # at least one background voxel
    _check_edt(core, mask)
    _check_edt(core, mask == 0, invert=True)


def test_core_header_special_masks(core):
    corner = np.ones((12, 9, 70), np.uint8)
    corner[-1, 0, -1] = 0
    _check_edt(core, corner)
    plane = np.ones((10, 11, 13), np.uint8)
    plane[:, 4, :] = 0
    _check_edt(core, plane)
    rows = np.ones((6, 7, 130), np.uint8)                          # most rows without background, one plane without any
    rows[1, 2, 64:] = 0
    rows[4, 6, 0] = 0
    rows[5, 0, 129] = 0
    _check_edt(core, rows)
    for shape in ((16384, 1, 2), (1, 16384, 2), (2, 1, 16384)):      # the longest line there is: squared distances up to 16383^2 + 1
        far = np.ones(shape, np.uint8)
        far[0, 0, 0] = 0
        _check_edt(core, far)
        far[-1, -1, -1] = 0
        _check_edt(core, far)
    _check_edt(core, np.zeros((3, 4, 5), np.uint8))


# ------------------------------------------------------------ the Gaussian filter ------------------------------------------------------------

def _kernel1d(sigma, radius):
    try:
        from scipy.ndimage._filters import _gaussian_kernel1d
        return _gaussian_kernel1d(sigma, 0, radius)
    except ImportError:
        x = np.arange(-radius, radius + 1)
        phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
        return phi / phi.sum()


WEIGHT_CASES = [(3.0, 4.0), (1.0, 4.0), (5.0, 4.0), (2.0, 4.0), (0.7, 4.0), (0.1, 4.0), (31.75, 4.0), (16.3, 4.0), (1.6, 2.5), (88.0, 1.0),
                (7.123456789, 3.3), (2.5, 4.0), (4.4, 4.0), (10.0, 4.0), (12.0, 4.0), (3.3, 4.0), (0.35, 30.0)]


def test_exp_equals_numpy(core):
    """The weights' exp is numpy's on the same machine: the C library's, or, where the CPU has the AVX-512 feature set numpy asks for, the vector
    library's routine restated for one element (gauss_exp_svml), which is not correctly rounded. Every argument the weights can produce lies in
    (-707.7, 0] unless truncate is above 37."""
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-707.7, 0, 200000), -rng.uniform(0, 40, 200000), -0.5 / rng.uniform(0.05, 40, 100000) ** 2 * rng.integers(0, 128, 100000) ** 2,
                        [0.0, -0.0, -1e-300, -707.70327]])
    x = x[x > -707.7032713517042]
    got = core.exp(x)
    print('%d arguments, %d differ from np.exp, %d from the correctly rounded value where math.exp gives it' %
          (x.size, np.count_nonzero(got != np.exp(x)), np.count_nonzero(got != np.array([math.exp(v) for v in x]))))
    assert np.array_equal(got, np.exp(x))


def test_gaussian_weights_equal_scipy(core):
    """Equality with scipy.ndimage's own _gaussian_kernel1d, centre outwards and mirrored."""
    for sigma, truncate in WEIGHT_CASES:
        radius = int(truncate * sigma + 0.5)
        r, w = core.weights(sigma, truncate)
        assert r == radius
        k = _kernel1d(sigma, radius)
        assert np.array_equal(w, k[radius:]) and np.array_equal(w, k[radius::-1]), (sigma, truncate)


def test_gaussian_radius_limit(core):
    assert core.weights(31.87, 4.0)[0] == 127
    assert core.weights(31.875, 4.0)[0] == -1 and core.weights(1e300, 1e300)[0] == -1


def gaussian_bound(x, sigma, truncate=4.0, cval=0.0, mode='reflect'):
    """The bound of the issue for the dtype of x: per filtered axis one rounding of a value no larger than max|x| (the weights are non-negative and sum
    to one, so a pass contracts the error already there); for float64 the error of the float64 sum itself, (2 r + 2) units, comes on top."""
    big = max(np.abs(x).max(), abs(cval) if mode == 'constant' else 0.0)
    sig = np.broadcast_to(np.asarray(sigma, np.float64), (3,))
    if x.dtype == np.float32:
        return sum(1 for s in sig if s > 1e-15) * 2.0 ** -24 * big * (1 + 2.0 ** -20)
    return sum(1 + 2 * int(truncate * s + 0.5) + 2 for s in sig if s > 1e-15) * 2.0 ** -53 * big


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('mode', ['reflect', 'constant', 'nearest', 'mirror'])
def test_core_header_gaussian_within_the_bound(core, dtype, mode):
    """The serial restatement of the kernels' arithmetic, on axes shorter than the radius too. Printed: the elements that differ from scipy's result in
    the same dtype (0 where scipy was built without fused multiply-add)."""
    rng = np.random.default_rng(5)
    for shape, sigma in (((5, 3, 40), 3.0), ((1, 2, 33), (2.0, 0.0, 1.0)), ((9, 8, 7), (1.0, 2.0, 0.5))):
        x = (rng.normal(300, 700, shape) * (rng.random(shape) < 0.5)).astype(dtype)
        got = core.gauss(x, sigma, mode, cval=-123.4)
        ref = ndimage.gaussian_filter(x.astype(np.float64), sigma, mode=mode, cval=-123.4)
        err = np.abs(got.astype(np.float64) - ref).max()
        same = ndimage.gaussian_filter(x, sigma, mode=mode, cval=-123.4)
        print('%s %s %s: max error %.3g, bound %.3g, %d elements differ from scipy in %s' % (shape, mode, sigma, err, gaussian_bound(x, sigma, cval=-123.4, mode=mode),
                                                                                           np.count_nonzero(got != same), np.dtype(dtype).name))
        assert err <= gaussian_bound(x, sigma, cval=-123.4, mode=mode)


# ------------------------------------------------------------ the argument contract ------------------------------------------------------------

@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_edt_entry_refuses_before_the_device(lib):
    """Every argument error is -1 whether or not a device is visible, and nothing is written; without a device a good call is -3, with nothing written."""
    for name in ('bfd_distance_transform_edt3d', 'bfd_gaussian_filter3d'):
        assert name in _engine.ABI_SYMBOLS and hasattr(lib, name)
    mask = np.ones((4, 5, 6), np.uint8)
    mask[1, 2, 3] = 0
    d2 = np.full(mask.shape, -7, np.int32)
    d = np.full(mask.shape, -7.0)
    ms = C.c_float(-5.0)

    def call(m=mask, flags=0, o2=d2, o=d, N=None, device=0):
        N = N or m.shape
        return lib.bfd_distance_transform_edt3d(device, P(m), flags, P(o2), P(o), N[0], N[1], N[2], C.byref(ms))

    def untouched():
        return (d2 == -7).all() and (d == -7.0).all() and ms.value == -5.0

    for f, what in ((lambda: call(o2=None, o=None), 'at least one output'), (lambda: call(N=(16385, 1, 1)), '16384'), (lambda: call(N=(1, 1, 16385)), '16384'),
                    (lambda: call(N=(-1, 5, 6)), 'negative'), (lambda: call(m=np.ones((4, 5, 6), np.uint8)), 'background'),
                    (lambda: call(m=np.zeros((4, 5, 6), np.uint8), flags=1), 'background'), (lambda: call(flags=2), 'flags'),
                    (lambda: call(N=(16384, 16384, 8)), '2^31'), (lambda: call(m=None, N=(4, 5, 6)), 'null')):
        assert f() == -1 and what in lib.bfd_last_error().decode(), what
        assert untouched()
    assert lib.bfd_distance_transform_edt3d(0, P(d2), 0, P(d2), None, 4, 5, 6, None) == -1 and 'overlap' in lib.bfd_last_error().decode()
    if lib.bfd_device_count() == 0:
        assert call() == -3 and call(N=(0, 5, 6)) == -3 and untouched()
        assert call(device=-1) == -3
    else:
        assert call(device=lib.bfd_device_count()) == -3 and call(device=-1) == -3 and untouched()


def test_gaussian_entry_refuses_before_the_device(lib):
    x = np.arange(4 * 5 * 6, dtype=np.float32).reshape(4, 5, 6)
    out = np.full(x.shape, -7, np.float32)
    ms = C.c_float(-5.0)

    def call(dtype=1, i=x, o=out, N=x.shape, sigma=(1.0, 1.0, 1.0), truncate=4.0, mode=0, device=0):
        s = None if sigma is None else (C.c_double * 3)(*sigma)
        return lib.bfd_gaussian_filter3d(device, dtype, P(i), P(o), N[0], N[1], N[2], s, truncate, mode, 0.0, C.byref(ms))

    def untouched():
        return (out == -7).all() and ms.value == -5.0

    inf, nan = float('inf'), float('nan')
    for f, what in ((lambda: call(sigma=(1.0, 32.0, 1.0)), 'radius'), (lambda: call(sigma=(1.0, 1.0, 2.0), truncate=64.0), 'radius'), (lambda: call(sigma=(-1.0, 1.0, 1.0)), 'sigma'),
                    (lambda: call(sigma=(1.0, nan, 1.0)), 'sigma'), (lambda: call(sigma=(1.0, 1.0, inf)), 'sigma'), (lambda: call(truncate=-1.0), 'truncate'),
                    (lambda: call(truncate=nan), 'truncate'), (lambda: call(truncate=inf), 'truncate'), (lambda: call(dtype=0), 'dtype'), (lambda: call(dtype=2), 'dtype'),
                    (lambda: call(mode=4), 'mode'), (lambda: call(mode=-1), 'mode'), (lambda: call(sigma=None), 'null'), (lambda: call(i=None), 'null'), (lambda: call(o=None), 'null'),
                    (lambda: call(N=(4, -5, 6)), 'negative'), (lambda: call(N=(1 << 20, 1 << 10, 2)), '2^31'), (lambda: call(o=x), 'overlap')):
        assert f() == -1 and what in lib.bfd_last_error().decode(), what
        assert untouched()
    both = np.zeros(2 * x.size - 1, np.float32)               # the two volumes share one element
    assert lib.bfd_gaussian_filter3d(0, 1, P(both), P(both[x.size - 1:]), 4, 5, 6, (C.c_double * 3)(1, 1, 1), 4.0, 0, 0.0, None) == -1
    assert 'overlap' in lib.bfd_last_error().decode()
    if lib.bfd_device_count() == 0:
        assert call() == -3 and call(N=(0, 5, 6)) == -3 and call(sigma=(0.0, 0.0, 0.0)) == -3 and untouched()
    else:
        assert call(device=lib.bfd_device_count()) == -3 and call(device=-1) == -3 and untouched()


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """The library is out of reach: its path names a missing file and loading it is an error. The refusals below must come first."""
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_engine, 'LIB_PATH', str(tmp_path / 'no_such_library.so'))
    monkeypatch.setattr(_engine, '_lib', None)
    monkeypatch.setattr(_engine, 'load_library', boom)


def test_distance_transform_refuses_before_the_library(no_library):
    mask = np.ones((4, 5, 6), bool)
    mask[0, 0, 0] = False
    with pytest.raises(NotImplementedError):
        DT.distance_transform_edt(mask, sampling=(1.0, 2.0, 1.0))
    with pytest.raises(NotImplementedError):
        DT.distance_transform_edt(mask, sampling=0.5)
    with pytest.raises(NotImplementedError):
        DT.distance_transform_edt(mask, return_indices=True)
    with pytest.raises(ValueError, match='background'):
        DT.distance_transform_edt(np.ones((4, 5, 6), np.float32))
    with pytest.raises(ValueError, match='background'):
        DT.distance_transform_edt(np.zeros((4, 5, 6), np.int16), invert=True)
    with pytest.raises(ValueError, match='3-D'):
        DT.distance_transform_edt(mask[0])
    with pytest.raises(ValueError, match='16384'):
        DT.distance_transform_edt(np.zeros((1, 1, 16385), bool))
    with pytest.raises(ValueError, match='return_distances'):
        DT.distance_transform_edt(mask, return_distances=False)
    with pytest.raises(TypeError):
        DT.distance_transform_edt(np.zeros((2, 2, 2), complex))


def test_gaussian_filter_refuses_before_the_library(no_library):
    x = np.zeros((4, 5, 6), np.float32)
    for bad in (dict(order=1), dict(order=(0, 1, 0)), dict(mode='wrap'), dict(mode='grid-wrap'), dict(mode='grid-constant'), dict(mode='grid-mirror'),
                dict(mode=['reflect', 'mirror', 'reflect'])):
        with pytest.raises(NotImplementedError):
            GF.gaussian_filter(x, 1.0, **bad)
    for dtype in (np.uint8, np.int16, np.float16, bool, complex):
        with pytest.raises(TypeError):
            GF.gaussian_filter(x.astype(dtype), 1.0)
    with pytest.raises(ValueError, match='3-D'):
        GF.gaussian_filter(x[0], 1.0)
    with pytest.raises(ValueError, match='sigma'):
        GF.gaussian_filter(x, (1.0, 2.0))
    with pytest.raises(ValueError, match='sigma'):
        GF.gaussian_filter(x, -1.0)
    with pytest.raises(ValueError, match='sigma'):
        GF.gaussian_filter(x, (1.0, float('nan'), 1.0))
    with pytest.raises(ValueError, match='truncate'):
        GF.gaussian_filter(x, 1.0, truncate=float('inf'))
    with pytest.raises(ValueError, match='radius'):
        GF.gaussian_filter(x, 32.0)


def test_wrappers_without_a_device(lib):
    if lib.bfd_device_count() > 0:
        pytest.skip('a GPU is present')
    with pytest.raises(_engine.EngineError):
        DT.distance_transform_edt(np.zeros((2, 3, 4), bool))
    with pytest.raises(_engine.EngineError):
        GF.gaussian_filter(np.zeros((2, 3, 4), np.float32), 1.0)
    with pytest.raises(_engine.EngineError):
        DT.InitDistanceTransform('MI355X')
    with pytest.raises(_engine.EngineError):
        GF.InitGaussianFilter('MI355X')
