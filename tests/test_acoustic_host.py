"""Result packing without a GPU. (1) tests/acoustic_oracle.py, the numpy restatement the device is held to, against the reference's own vectors
(tests/golden/harness_golden.npz: phase_* from CalculatePhaseData, rr_* from ReturnResults), and five planted faults that must each change its
result. (2) csrc/bfd_pack_core.h, the index arithmetic and the three scale definitions the kernels use, compiled for the host and held to the
restatement: every kept length 1 .. 130 on each axis, and the scales on 10^5 random values, denormals and signed zeros."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from babelbrain_amd import _engine, results as R
from tests import acoustic_oracle as AO


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the restatement against the reference ----------------------------------------------------------------

def _phase_case(g):
    N1, N2, N3, ppp, sub, f, dts = g['phase_args']
    return (int(N1), int(N2), int(N3)), float(f), float(dts)


def test_restatement_gives_calculate_phase_data(golden):
    """series -> FFT bin * 2 / nTs -> scatter, no scaling, nothing cropped away but the last plane of each axis (the reference slices with -offset)"""
    g, _ = golden
    N, f, dts = _phase_case(g)
    F, pk = AO.series_dft(g['phase_series'], dts, f)
    amp, four, peak = AO.pack(F, pk, g['phase_index'], np.zeros(N, np.float32), N, (0, 0, 0), (1, 1, 1), -1, flipK=False)
    # the golden Fourier map is a float32-rounded FFT of whichever numpy wrote it: its own tolerance stays a norm, as in tests/test_dft_gpu.py
    ref = g['phase_fourier'][:-1, :-1, :-1]
    assert four.dtype == np.complex64 and np.array_equal(four != 0, ref != 0)
    assert np.linalg.norm((four - ref).astype(np.complex128)) <= 1e-6 * np.linalg.norm(ref.astype(np.complex128))
    assert np.array_equal(peak, g['phase_peak'][:-1, :-1, :-1]) and peak.dtype == np.float32
    assert np.count_nonzero(four) == len(g['phase_index']) and not amp.any()


def _rr_case(g):
    a = [int(v) for v in g['rr_args']]
    N, zsrc = tuple(a[:3]), a[4]
    lo, hi, shrink = (a[5], a[7], a[9]), (a[6], a[8], a[10]), tuple(a[11:14])
    n = N[0] * N[1] * N[2]
    index = np.arange(1, n + 1, dtype=np.uint32)                       # every voxel a sensor, in IndexSensorMap's order
    F = g['rr_in_PressMapFourier'].reshape(-1, order='F')
    return N, zsrc, lo, hi, shrink, index, F


def test_restatement_gives_return_results(golden):
    g, _ = golden
    N, zsrc, lo, hi, shrink, index, F = _rr_case(g)
    peak = g['rr_in_InPeakValue'].reshape(-1, order='F')
    amp, four, _ = AO.pack(F, peak, index, g['rr_in_InPeakValue'], N, lo, hi, zsrc)
    assert same_bits(amp, g['rr_dfs_p_amp']) and same_bits(four, g['rr_dfs_p_complex'])
    orig = g['rr_in_SkullMaskDataOrig'].shape
    full, _, pk = AO.pack(F, peak, index, g['rr_in_InPeakValue'], N, lo, hi, zsrc, O=orig, at=shrink)
    assert same_bits(full, g['rr_out_FullSolutionPressure']) and same_bits(pk, g['rr_out_FullSolutionPressure'])


def test_scaling_statements_as_numpy_2_evaluates_them():
    """BASE:2440 forms the product in float64 and rounds once (np.sqrt(2) is a float64 scalar); the float32 product differs somewhere"""
    rng = np.random.default_rng(5)
    a = rng.uniform(0.5, 2.0, 4096).astype(np.float32)
    c = 1.0173
    got = AO.scale_amp(a.copy(), c)
    assert got.dtype == np.float32 and np.array_equal(got, (a.astype(np.float64) * (c * np.sqrt(2))).astype(np.float32))
    assert not np.array_equal(got, a * np.float32(c * np.sqrt(2)))
    z = (a[:2048] + 1j * a[2048:]).astype(np.complex64)
    gz = AO.scale_sensor(z.copy(), c)
    assert gz.dtype == np.complex64 and np.array_equal(gz.real, z.real * np.float32(c)) and np.array_equal(gz.imag, z.imag * np.float32(c))


def test_planted_faults_change_the_result(golden):
    g, _ = golden
    N, zsrc, lo, hi, shrink, index, F = _rr_case(g)
    rms = g['rr_in_InPeakValue']
    peak = rms.reshape(-1, order='F')
    orig = g['rr_in_SkullMaskDataOrig'].shape
    c = 1.0173
    kw = dict(O=orig, at=shrink, correction=c)
    good = AO.pack(F, peak, index, rms, N, lo, hi, zsrc, **kw)
    again = AO.pack(F, peak, index, rms, N, lo, hi, zsrc, **kw)
    assert all(same_bits(x, y) for x, y in zip(good, again))

    def differs(other, which=(0, 1, 2)):
        return all(not np.array_equal(good[q], other[q]) for q in which)
    assert differs(AO.pack(F, peak, index, rms, N, lo, hi, zsrc, flipK=False, **kw)), 'flip omitted'
    assert differs(AO.pack(F, peak, index, rms, N, lo, hi, zsrc - 1, **kw)), '< for <= at the source plane'
    f32 = AO.pack(F, peak, index, rms, N, lo, hi, zsrc, scale_amp=lambda a, cc: np.multiply(a, np.float32(cc * np.sqrt(2)), out=a), **kw)
    assert differs(f32, (0,)) and same_bits(f32[1], good[1]), 'float32 amplitude product'
    N_, f, dts = _phase_case(g)
    nTs = g['phase_series'].shape[1]
    F2, pk2 = AO.series_dft(g['phase_series'], dts, f)
    a = AO.pack(F2, pk2, g['phase_index'], np.zeros(N_, np.float32), N_, (0, 0, 0), (1, 1, 1), -1)
    b = AO.pack(F2 * np.float32(nTs / 2), pk2, g['phase_index'], np.zeros(N_, np.float32), N_, (0, 0, 0), (1, 1, 1), -1)
    assert not np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), 'missing 2 / nTs'
    assert any(shrink)
    assert differs(AO.pack(F, peak, index, rms, N, lo, hi, zsrc, O=orig, at=(0, 0, 0), correction=c)), 'shrink offset dropped'


# ---------------------------------------------------------------- the core header ----------------------------------------------------------------

CORE_PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bfd_pack_core.h"
// index: in  int64 nCases; per case int32 dims[3], PackGeom (15 int32), PackBox (6 int32)
//        out per case: int64 source[O voxels] (x-fastest linear index of pack_source_voxel, -1 = none), int64 target[dims voxels, x fastest]
//        (pack_output_index), int64 sensor[dims voxels, x fastest] (pack_box_sensor)
// scale: in  int64 n; double ampScale; float correction; float x[n]      out float amp[n], float prod[n]
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[2], "rb"), *o = fopen(argv[3], "wb");
    int64_t n;
    if (!f || !o || fread(&n, 8, 1, f) != 1) return 2;
    if (!strcmp(argv[1], "index")) {
        for (int64_t q = 0; q < n; q++) {
            int32_t dims[3]; PackGeom g; PackBox B;
            if (fread(dims, 4, 3, f) != 3 || fread(&g, 4, 15, f) != 15 || fread(&B, 4, 6, f) != 6) return 2;
            for (int a = 0; a < g.O[0]; a++) for (int b = 0; b < g.O[1]; b++) for (int c = 0; c < g.O[2]; c++) {
                int i, j, k;
                const int64_t v = pack_source_voxel(g, a, b, c, i, j, k) ? i + (int64_t)dims[0] * (j + (int64_t)dims[1] * k) : -1;
                fwrite(&v, 8, 1, o);
            }
            for (int k = 0; k < dims[2]; k++) for (int j = 0; j < dims[1]; j++) for (int i = 0; i < dims[0]; i++) { const int64_t v = pack_output_index(g, i, j, k); fwrite(&v, 8, 1, o); }
            for (int k = 0; k < dims[2]; k++) for (int j = 0; j < dims[1]; j++) for (int i = 0; i < dims[0]; i++) { const int64_t v = pack_box_sensor(B, i, j, k); fwrite(&v, 8, 1, o); }
        }
    } else {
        double ampScale; float corr;
        if (fread(&ampScale, 8, 1, f) != 1 || fread(&corr, 4, 1, f) != 1) return 2;
        float *x = (float *)malloc(4 * n + 4);
        if (fread(x, 4, n, f) != (size_t)n) return 2;
        for (int64_t i = 0; i < n; i++) { const float v = pack_scale_amp(x[i], ampScale); fwrite(&v, 4, 1, o); }
        for (int64_t i = 0; i < n; i++) { const float v = pack_scale_f32(x[i], corr); fwrite(&v, 4, 1, o); }
    }
    fclose(o);
    return 0;
}
"""


@pytest.fixture(scope='module')
def core(tmp_path_factory):
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx, 'no C++ compiler found'
    d = tmp_path_factory.mktemp('packcore')
    src = d / 'packcore.cpp'
    src.write_text(CORE_PROGRAM)
    exe = str(d / 'packcore')
    subprocess.run([cxx, '-O1', '-ffp-contract=off', '-I', os.path.join(os.path.dirname(_engine.LIB_PATH), 'csrc'), str(src), '-o', exe, '-lm'], check=True)
    inp, outp = str(d / 'in.bin'), str(d / 'out.bin')

    def index(cases):
        with open(inp, 'wb') as f:
            f.write(np.int64(len(cases)).tobytes())
            for c in cases:
                words = list(c['dims']) + list(c['lo']) + list(c['keep']) + list(c['O']) + list(c['at']) + [c['zsrc'], c['k0'], int(c['flip'])] + list(c['box'])
                f.write(np.array(words, np.int32).tobytes())
        subprocess.run([exe, 'index', inp, outp], check=True)
        flat, out, p = np.fromfile(outp, np.int64), [], 0
        for c in cases:
            nO, nV = int(np.prod(c['O'])), int(np.prod(c['dims']))
            out.append((flat[p:p + nO].reshape(c['O']), flat[p + nO:p + nO + nV], flat[p + nO + nV:p + nO + 2 * nV]))
            p += nO + 2 * nV
        assert p == flat.size
        return out

    def scale(x, amp_scale, corr):
        x = np.ascontiguousarray(x, np.float32)
        with open(inp, 'wb') as f:
            f.write(np.int64(x.size).tobytes() + np.float64(amp_scale).tobytes() + np.float32(corr).tobytes() + x.tobytes())
        subprocess.run([exe, 'scale', inp, outp], check=True)
        r = np.fromfile(outp, np.float32)
        return r[:x.size], r[x.size:]
    return index, scale


def _index_cases():
    cases = []
    for ax in range(3):
        for L in range(1, 131):
            lo, hi = [1, 1, 1], [1, 1, 1]
            lo[ax], hi[ax] = 2 + L % 3, 1 + L % 2
            keep = [2, 2, 2]
            keep[ax] = L
            dims = [lo[a] + keep[a] + hi[a] for a in range(3)]
            at = [L % 2, (L // 2) % 2, (L // 4) % 3]
            O = [keep[a] + at[a] + ((L + a) % 2) for a in range(3)]
            k0 = 3 if L % 7 == 0 else 0
            zsrc = k0 + lo[2] - 2 + (L + ax) % (keep[2] + 3)                 # below, inside and above the kept planes
            box = [max(dims[0] - 2, 1), max(dims[1] - 1, 1), max(dims[2] - 2, 1), 1, 0, 1]      # extents, then first voxel
            cases.append(dict(dims=dims, lo=lo, hi=hi, keep=keep, O=O, at=at, k0=k0, zsrc=zsrc, flip=bool((L + ax) % 2), box=box))
    return cases


def test_core_index_arithmetic_equals_the_restatement(core):
    """An id volume goes through the reference's own zero / crop / paste / flip (results.py); the header must name the same voxel for every output
    voxel, the same output voxel for every slab voxel, and the rank a SensorMap of the box gives every voxel."""
    index, _ = core
    cases = _index_cases()
    assert sorted({c['keep'][a] for a in range(3) for c in cases}) == list(range(1, 131))
    got = index(cases)
    seen_zero = set()
    for c, (src, tgt, sens) in zip(cases, got):
        dims = c['dims']
        n = int(np.prod(dims))
        ids = np.arange(1, n + 1, dtype=np.int64).reshape(dims, order='F')
        zs = c['zsrc'] - c['k0']
        assert zs >= -1
        R.zero_up_to_source(ids, zs)
        crop = R.Crop(c['lo'][0], c['hi'][0], c['lo'][1], c['hi'][1], c['lo'][2], c['hi'][2], *c['at'])
        out = R.paste_and_flip(ids, crop, tuple(c['O']), np.int64)
        if not c['flip']:
            out = np.flip(out, axis=2)
        assert np.array_equal(src, out - 1), c
        want = np.full(n, -1, np.int64)
        flat = np.ascontiguousarray(out).reshape(-1)
        want[flat[flat > 0] - 1] = np.flatnonzero(flat > 0)
        assert np.array_equal(tgt, want), c
        seen_zero.add((zs < c['lo'][2], zs >= c['lo'][2] + c['keep'][2] - 1))
        bx, by, bz, i0, j0, k0 = c['box']
        mask = np.zeros(dims, bool)
        mask[i0:i0 + bx, j0:j0 + by, k0:k0 + bz] = True
        rank = np.full(n, -1, np.int64)
        where = np.flatnonzero(mask.reshape(-1, order='F'))
        rank[where] = np.arange(where.size)
        assert np.array_equal(sens, rank), c
    assert {(True, False), (False, False), (False, True)} <= seen_zero        # source plane below, inside, at or above the last kept plane


def test_core_scales_equal_numpy_bit_for_bit(core):
    _, scale = core
    rng = np.random.default_rng(11)
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 5.9e-39, 1.17549435e-38, 3.4028235e38 / 2], np.float32)
    x = np.concatenate([rng.normal(0, 1, 50000).astype(np.float32) * np.float32(1e5), rng.uniform(-1, 1, 50000).astype(np.float32),
                        (rng.uniform(-1, 1, 1000) * 1e-38).astype(np.float32), tiny])
    for c in (1.0173, 0.98, 1.0):
        amp, prod = scale(x, c * np.sqrt(2), c)
        assert same_bits(amp, AO.scale_amp(x.copy(), c))
        assert same_bits(prod, AO.scale_sensor(x.copy(), c))
        z = (x + 1j * x[::-1]).astype(np.complex64)
        gz = AO.scale_sensor(z.copy(), c)
        # value equality: the complex product with c + 0j may turn a -0 into +0, which no output depends on (tests/util.py::assert_same)
        assert np.array_equal(prod, gz.real) and np.array_equal(prod[::-1], gz.imag)
