"""The thermal study without a GPU: the ABI, the per-element arithmetic of csrc/bfd_thermal_study_core.h compiled for the host against numpy, the
flow helper (tests/thermal_study_flow.py) over the numpy oracles with planted faults it must see, and every argument error of every entry in the
header's order with the outputs untouched."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from babelbrain_amd import _engine
from tests import thermal_study_flow as F

ENTRIES = ['bfd_thermal_create', 'bfd_thermal_destroy', 'bfd_thermal_set_inputs', 'bfd_thermal_median_region', 'bfd_thermal_loss_survey',
           'bfd_thermal_set_scale', 'bfd_thermal_run', 'bfd_thermal_set_previous', 'bfd_thermal_merge_max', 'bfd_thermal_extrema', 'bfd_thermal_get', 'bfd_thermal_get_plane',
           'bfd_thermal_traffic']


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


def test_the_abi_exports_the_study_and_keeps_its_version(lib):
    assert lib.bfd_abi_version() == _engine.ABI_VERSION
    for name in ENTRIES:
        assert name in _engine.ABI_SYMBOLS and hasattr(lib, name), name


# ---------------------------------------------------------------- the core header against numpy ----------------------------------------------------------------

CORE_PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "bfd_thermal_study_core.h"
// in: int64 n, int64 nFields, double ratio[nFields], float qf[n], float p[nFields][n]
// out: float mode0[n], float mode1[n], double wide[n] (field 0), float heat0[n], float heat1[n], float max0[n] (fields scaled in mode 1 ... see below)
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb");
    int64_t n, F;
    if (!f || fread(&n, 8, 1, f) != 1 || fread(&F, 8, 1, f) != 1) return 1;
    std::vector<double> ratio(F);
    std::vector<float> qf(n), p(n * F), m0(n), m1(n), h0(n), h1(n), fm(n);
    std::vector<double> wide(n);
    if (fread(ratio.data(), 8, F, f) != (size_t)F || fread(qf.data(), 4, n, f) != (size_t)n || fread(p.data(), 4, n * F, f) != (size_t)(n * F)) return 1;
    fclose(f);
    for (int64_t i = 0; i < n; i++) {
        m0[i] = ts_scaled(p[i], ratio[0], TS_MODE_DOUBLE_RATIO);
        m1[i] = ts_scaled(p[i], ratio[0], TS_MODE_FLOAT_RATIO);
        wide[i] = ts_scaled64(p[i], ratio[0]);
        h0[i] = ts_heat(m0[i], qf[i]);
        h1[i] = ts_heat(m1[i], qf[i]);
        fm[i] = ts_field_max(p.data() + i, n, (int)F, ratio.data(), TS_MODE_FLOAT_RATIO);
    }
    f = fopen(argv[2], "wb");
    fwrite(m0.data(), 4, n, f); fwrite(m1.data(), 4, n, f); fwrite(wide.data(), 8, n, f); fwrite(h0.data(), 4, n, f); fwrite(h1.data(), 4, n, f);
    fwrite(fm.data(), 4, n, f);
    fclose(f);
    uint32_t bad = 0;
    if (ts_narrow_id(4, 5, &bad) != 4 || bad || ts_narrow_id(5, 5, &bad) != 0 || !bad) return 2;
    const uint8_t table[3] = {1, 8, 9};
    if (ts_region(0, table, 3) != 0 || ts_region(1, table, 3) != 1 || ts_region(2, table, 0) != 1) return 3;
    return 0;
}
"""


@pytest.fixture(scope='module')
def core(tmp_path_factory):
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx, 'no C++ compiler found'
    d = tmp_path_factory.mktemp('studycore')
    src = d / 'studycore.cpp'
    src.write_text(CORE_PROGRAM)
    exe = str(d / 'studycore')
    subprocess.run([cxx, '-O1', '-ffp-contract=off', '-I', os.path.join(os.path.dirname(_engine.LIB_PATH), 'csrc'), str(src), '-o', exe, '-lm'], check=True)

    def run(p, ratio, qf):
        p = np.ascontiguousarray(np.atleast_2d(p), np.float32)
        ratio = np.ascontiguousarray(ratio, np.float64).reshape(-1)
        nF, n = p.shape
        inp, outp = str(d / 'in.bin'), str(d / 'out.bin')
        with open(inp, 'wb') as f:
            f.write(np.int64(n).tobytes() + np.int64(nF).tobytes() + ratio.tobytes() + np.ascontiguousarray(qf, np.float32).tobytes() + p.tobytes())
        subprocess.run([exe, inp, outp], check=True)
        raw = open(outp, 'rb').read()
        o, out = 0, {}
        for name, dt in (('mode0', np.float32), ('mode1', np.float32), ('wide', np.float64), ('heat0', np.float32), ('heat1', np.float32), ('fmax', np.float32)):
            out[name] = np.frombuffer(raw, dt, n, o)
            o += n * np.dtype(dt).itemsize
        return out
    return run


def sweep():
    """float32 values of every size: denormals, the smallest normals, ordinary pressures, the largest finite value, both signs, zeros"""
    rng = np.random.default_rng(11)
    tiny = np.finfo(np.float32).tiny
    special = np.array([0.0, -0.0, 1e-45, 3e-45, tiny / 2, tiny, tiny * 1.5, 1.0, 3.0, 2.5e5, 6.0e5, 16777217.0, 3.4028235e38, 1.7e38], np.float32)
    bits = rng.integers(0, 0x7F800000, 6000, dtype=np.int64).astype(np.uint32)          # every exponent, finite
    vals = np.concatenate([special, -special, bits.view(np.float32), -bits.view(np.float32), rng.uniform(1e4, 1e6, 4000).astype(np.float32)])
    return np.ascontiguousarray(vals, np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize('ratio', [0.7310585786300049, 0.9999, 1.0001, 1.5596243, 1.0000001192092896 * 3.3])
def test_core_scaling_equals_numpy_in_both_modes(core, ratio):
    p = sweep()
    qf = np.full(p.size, 3.25e-13, np.float32)
    with np.errstate(over='ignore'):
        want0 = (p * np.float64(ratio)).astype(np.float32)
        want1 = p * np.float32(ratio)
        wide = p * np.float64(ratio)
        assert wide.dtype == np.float64 and want1.dtype == np.float32          # NumPy >= 2 promotion, which the definition restates
        got = core(p, [ratio], qf)
        assert np.array_equal(bits(got['mode0']), bits(want0))
        assert np.array_equal(bits(got['mode1']), bits(want1))
        assert np.array_equal(bits(got['wide']), bits(wide))
        # a swapped mode cannot pass: no ratio here is a float32, so the one rounding of mode 0 and the two of mode 1 differ somewhere on the sweep
        assert float(np.float32(ratio)) != ratio
        assert np.count_nonzero(bits(want0) != bits(want1)) > 0
        for mode, s in (('heat0', want0), ('heat1', want1)):
            assert np.array_equal(bits(got[mode]), bits((s * s) * qf))


def test_core_field_maximum_equals_numpy_nan_included(core):
    rng = np.random.default_rng(3)
    p = rng.uniform(-5e5, 5e5, (3, 4096)).astype(np.float32)
    p[0, 5] = p[1, 5] = p[2, 5]                       # a tie
    p[0, 7], p[1, 8], p[2, 9] = np.nan, np.nan, np.nan          # a NaN in the first, a middle and the last field wins
    p[:, 10] = np.nan
    p[0, 11], p[1, 11] = np.inf, -np.inf
    ratio = np.array([1.25, 0.5, 2.0], np.float32)
    scaled = p * ratio[:, None]
    assert scaled.dtype == np.float32
    want = scaled.max(axis=0)
    got = core(p, ratio.astype(np.float64), np.zeros(p.shape[1], np.float32))['fmax']
    assert np.isnan(want[[7, 8, 9, 10]]).all() and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok])


# ---------------------------------------------------------------- the flow over the oracles ----------------------------------------------------------------

@pytest.fixture(scope='module')
def small_flow():
    c = F.make_case((9, 8, 20), seed=4, previous=True)
    return c, F.flow_by_calls(c, F.oracle_calls())


def test_flow_over_the_oracles_runs_and_repeats(small_flow):
    c, S = small_flow
    again = F.flow_by_calls(c, F.oracle_calls())
    for k in F.SMALL + F.VOLUMES:
        assert np.array_equal(np.asarray(S[k]), np.asarray(again[k])), k
    assert S['p_map'].dtype == np.float64 and S['TempEndFUS'].dtype == np.float32
    assert S['TemperaturePoints'].shape[0] == 4 and S['TempEndFUS'].max() > 37.5
    assert np.all(S['TempEndFUS'] >= c['PreviousData']['TempEndFUS'])


@pytest.mark.parametrize('fault', ['median', 'merge', 'scale'])
def test_a_statement_left_out_changes_a_result(small_flow, fault):
    """the planted faults the comparison with thermal_exposure must see: each leaves a statement of the flow out"""
    c, S = small_flow
    bad = F.flow_by_calls(c, F.oracle_calls(), skip=(fault,))
    changed = [k for k in F.SMALL + F.VOLUMES if not np.array_equal(np.asarray(S[k]), np.asarray(bad[k]))]
    print(fault, changed)
    assert changed, fault


def test_flow_over_the_oracles_with_three_fields():
    c = F.make_case((9, 8, 20), seed=5, fields=3)
    S = F.flow_by_calls(c, F.oracle_calls())
    assert S['PressureRatio'].dtype == np.float32 and S['PressureRatio'].shape == (3,)
    assert S['p_map'].dtype == np.float32 and np.array_equal(S['p_map'], (c['pAmp'] * S['PressureRatio'][:, None, None, None]).max(axis=0))


# ---------------------------------------------------------------- argument errors ----------------------------------------------------------------

def err(lib):
    return lib.bfd_last_error().decode()


def test_create_refuses_in_the_headers_order(lib):
    h = C.c_void_p()
    limit = lib.bfd_bhte_max_materials()
    for args, text in (((0, 8, 8, 8, 1, 5, None), 'null argument'), ((0, 2, 8, 8, 1, 5, C.byref(h)), 'at least 3'), ((0, 8, 8, 2, 1, 5, C.byref(h)), 'at least 3'),
                       ((0, 2048, 2048, 2048, 1, 5, C.byref(h)), '2^31 voxels'), ((0, 8, 8, 8, 0, 5, C.byref(h)), 'nFields'),
                       ((0, 8, 8, 8, 1, 0, C.byref(h)), 'nMat'), ((0, 8, 8, 8, 1, limit + 1, C.byref(h)), 'nMat'),
                       # the first argument error wins over the later ones
                       ((0, 2, 8, 8, 0, 0, C.byref(h)), 'at least 3')):
        assert lib.bfd_thermal_create(*args) == -1 and text in err(lib) and err(lib).startswith('bfd_thermal_create: '), (args[:6], err(lib))
        assert not h
    if lib.bfd_device_count() == 0:
        assert lib.bfd_thermal_create(0, 8, 8, 8, 1, 5, C.byref(h)) == -3 and not h


def test_every_entry_refuses_a_null_handle_before_anything_else(lib):
    """and leaves its outputs as they were"""
    P = _engine._ptr
    f4, i8, f8, u1 = np.full(8, 7.0, np.float32), np.full(8, 7, np.int64), np.full(8, 7.0), np.full(8, 7, np.uint8)
    ms, msd = C.c_float(7.0), C.c_double(7.0)
    up, down = C.c_int64(7), C.c_int64(7)
    calls = [
        ('bfd_thermal_set_inputs', (None, P(f4), P(f4), P(u1), 1)),
        ('bfd_thermal_median_region', (None, P(u1), 3, 7, C.byref(ms))),
        ('bfd_thermal_loss_survey', (None, P(u1), None, P(f8), P(f8), 1000.0, 1500.0, 1e-6, P(f4), P(i8), P(f4), P(i8), P(f8), P(f8), P(f8), C.byref(ms))),
        ('bfd_thermal_set_scale', (None, P(f8), 0)),
        ('bfd_thermal_run', (None, P(f4), P(f4), P(f4), P(f4), 0, None, None, 37.0, 0.01, 0, None, 1, 0, None, None, 0, None, C.byref(msd))),
        ('bfd_thermal_set_previous', (None, P(f4), P(f4), P(f4))),
        ('bfd_thermal_merge_max', (None, 0, P(f4))),
        ('bfd_thermal_extrema', (None, P(np.zeros(1, np.int32)), 1, P(u1), P(i8), P(f4), P(i8), P(f4), P(i8), C.byref(ms))),
        ('bfd_thermal_get', (None, 0, P(f4), 0)),
        ('bfd_thermal_get_plane', (None, 5, 0, P(f4))),
        ('bfd_thermal_traffic', (None, C.byref(up), C.byref(down))),
    ]
    for name, args in calls:
        assert getattr(lib, name)(*args) == -1, name
        assert err(lib) == name + ': null argument', (name, err(lib))
    assert (f4 == 7).all() and (i8 == 7).all() and (f8 == 7).all() and ms.value == 7.0 and msd.value == 7.0 and up.value == 7 and down.value == 7
    lib.bfd_thermal_destroy(None)                      # accepted


def test_python_argument_errors_come_before_the_library(monkeypatch):
    from babelbrain_amd import ThermalStudy as TS

    def boom():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_engine, 'load_library', boom)
    ml = dict(Density=np.ones(5), SoS=np.ones(5))
    p = np.zeros((4, 4, 4), np.float32)
    with pytest.raises(TypeError):
        TS.ThermalStudy(p.astype(np.float64), p, np.zeros((4, 4, 4), np.uint8), ml, 1e-3)
    with pytest.raises(ValueError):
        TS.ThermalStudy(p, p, np.zeros((4, 4, 5), np.uint8), ml, 1e-3)
    with pytest.raises(ValueError):
        TS.ThermalStudy(p[:2], p[:2], np.zeros((2, 4, 4), np.uint8), ml, 1e-3)
    with pytest.raises(ValueError):
        TS.thermal_exposure(p, p, np.zeros((4, 4, 4), np.uint8), ml, {}, [1, 1, 1], 5.0, 0.3, 5e5, 0.01, 0.1, 0.1, keep=('nothing',))
