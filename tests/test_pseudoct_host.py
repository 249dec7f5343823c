"""The host side of the pseudo-CT (babelbrain_amd/PseudoCT.py, csrc/bfd_pseudoct_core.h) without a device: the module's find_peaks against
scipy's, the percentile interpolation, the bin rule, the truncation, the keys and the HU expression (the core header compiled for the host)
against numpy, the refusals that come before the library, and the oracle's flow on the phantom: every step has work there."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import signal

from babelbrain_amd import BinaryClosing as BC, LabelImage as LI, PseudoCT as PC, TissueMask as TM, _engine
from tests import pseudoct_calls as TC, pseudoct_oracle as PO


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """The library is out of reach: its path names a missing file and loading it is an error. The refusals below must come first."""
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_engine, 'LIB_PATH', str(tmp_path / 'no_such_library.so'))
    monkeypatch.setattr(_engine, '_lib', None)
    monkeypatch.setattr(_engine, 'load_library', boom)


# ---------------------------------------------------------------- find_peaks ----------------------------------------------------------------

def same_peaks(x, distance):
    got = PC.find_peaks(x, distance=distance)
    want = signal.find_peaks(x, distance=distance)[0]
    assert got.dtype == want.dtype and np.array_equal(got, want), (distance, x.tolist(), got, want)


def test_find_peaks_equals_scipy_on_random_histograms():
    rng = np.random.default_rng(1)
    for trial in range(300):
        n = int(rng.integers(1, 200))
        levels = int(rng.choice([2, 3, 6, 50, 100000]))           # few levels: plateaus and equal heights within the distance
        x = rng.integers(0, levels, n)
        if trial % 3 == 0:
            x = np.repeat(x, rng.integers(1, 4, n))               # wider plateaus
        for distance in (None, 1, 2, 5, 50, 7.5):
            same_peaks(x, distance)
            same_peaks(x.astype(np.float64), distance)


def test_find_peaks_plateaus_ends_and_ties():
    for x in ([5, 1, 1, 5], [0, 5, 0], [5, 5, 0, 5, 5], [0, 3, 3, 0], [0, 3, 3, 3, 0], [0, 3, 3, 3, 3, 0, 3, 0], [1, 2, 3], [3, 2, 1], [0], [], [1, 1],
              [0, 2, 0, 2, 0, 2, 0, 2, 0], [0, 2, 0, 3, 0, 2, 0, 3, 0, 2, 0], [0, 1, 0, 0, 1, 1, 0, 9, 9, 9, 0, 1, 0], [9, 0, 9], [0, 9, 9]):
        for distance in (None, 1, 2, 3, 4, 100):
            same_peaks(np.array(x, np.int64), distance)
    with pytest.raises(ValueError, match='distance'):
        PC.find_peaks(np.arange(5), distance=0)
    with pytest.raises(ValueError, match='1-D'):
        PC.find_peaks(np.zeros((2, 2)))


def test_normaliser_from_a_histogram_equals_the_oracle():
    rng = np.random.default_rng(2)
    for trial in range(20):
        v = np.round(np.concatenate([np.abs(rng.normal(0, 15, 4000)), rng.normal(700, 30, 1500), rng.normal(1800 + 10 * trial, 40, 3000)])) - trial
        want = PO.petra_normaliser(v)
        hist, edges = PO.integer_histogram(v)
        got = PC._normaliser_from_histogram(hist, int(v.min()), 50, 2)
        assert isinstance(got, float) and got == want, (trial, got, want)
        for distance, peaks in ((5, 3), (200, 1), (1, 4)):
            assert PC._normaliser_from_histogram(hist, int(v.min()), distance, peaks) == PO.petra_normaliser(v, distance, peaks)
    with pytest.raises(ValueError, match='fewer than two bins'):
        PC._normaliser_from_histogram(np.array([5, 3]), 0, 50, 2)
    with pytest.raises(ValueError, match='no peak'):
        PC._normaliser_from_histogram(np.array([5, 1, 2, 3]), 0, 50, 2)


# ---------------------------------------------------------------- the core header ----------------------------------------------------------------

CORE_PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "bfd_pseudoct_core.h"
// <mode> <in> <out>: float64 records in, float64 (keys: uint64) out
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 3;
    std::vector<double> in;
    double x;
    while (fread(&x, 8, 1, f) == 1) in.push_back(x);
    fclose(f);
    std::vector<double> out;
    std::vector<uint64_t> keys;
    const std::string mode = argv[1];
    if (mode == "pct") {                 // records [n, q, sorted values (n)]: the percentile
        for (size_t p = 0; p < in.size();) {
            const int64_t n = (int64_t)in[p];
            const double q = in[p + 1];
            int64_t lo, hi;
            double g;
            pc_quantile_ranks(n, q, &lo, &hi, &g);
            out.push_back((double)lo); out.push_back((double)hi);
            out.push_back(pc_lerp(in[p + 2 + lo], in[p + 2 + hi], g));
            p += 2 + (size_t)n;
        }
    } else if (mode == "bin") {          // [bins, edges (bins + 1), values ...]: the bin of each value
        const int bins = (int)in[0];
        const double *edges = &in[1];
        for (size_t p = 2 + (size_t)bins; p < in.size(); p++) out.push_back((double)pc_uniform_bin(in[p], edges[0], edges[bins], bins, edges));
    } else if (mode == "trunc") {
        for (double v : in) out.push_back((double)pc_trunc(v));
    } else if (mode == "hu") {           // records [q, slope, offset, skin, bone, cavity]
        for (size_t p = 0; p + 5 < in.size(); p += 6) out.push_back(pc_hu(in[p], in[p + 1], in[p + 2], in[p + 3] != 0, in[p + 4] != 0, in[p + 5] != 0));
    } else if (mode == "key64") {        // the key of each float64, then the key unkeyed
        for (double v : in) keys.push_back(pc_key64(pc_bits64(v)));
        for (double v : in) keys.push_back(pc_unkey64(pc_key64(pc_bits64(v))));
    } else if (mode == "key32") {        // float32 bits handed as float64 numbers: key, the key unkeyed, and the bits of the widened value
        for (double v : in) keys.push_back(pc_key32((uint32_t)v));
        for (double v : in) keys.push_back(pc_unkey32(pc_key32((uint32_t)v)));
        for (double v : in) keys.push_back(pc_bits64(pc_value<false>((uint64_t)(uint32_t)v)));
        for (double v : in) keys.push_back(pc_bits64(pc_key_value<false>(pc_key<false>((uint64_t)(uint32_t)v))));
    } else return 4;
    f = fopen(argv[3], "wb");
    if (!f) return 5;
    if (!out.empty()) fwrite(out.data(), 8, out.size(), f);
    if (!keys.empty()) fwrite(keys.data(), 8, keys.size(), f);
    fclose(f);
    return 0;
}
'''


@pytest.fixture(scope='module')
def core(tmp_path_factory):
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx, 'no C++ compiler found'
    d = tmp_path_factory.mktemp('pseudoctcore')
    src = d / 'pseudoctcore.cpp'
    src.write_text(CORE_PROGRAM)
    exe = str(d / 'pseudoctcore')
    subprocess.run([cxx, '-O1', '-ffp-contract=off', '-I', os.path.join(os.path.dirname(_engine.LIB_PATH), 'csrc'), str(src), '-o', exe, '-lm'], check=True)

    def run(mode, data, out_dtype=np.float64):
        inp, outp = str(d / 'in.bin'), str(d / 'out.bin')
        np.ascontiguousarray(data, np.float64).tofile(inp)
        subprocess.run([exe, mode, inp, outp], check=True)
        return np.fromfile(outp, out_dtype)
    return run


def percentile_cases():
    rng = np.random.default_rng(3)
    cases = []
    for n in (1, 2, 21, 20, 1000):
        for trial in range(6):
            x = np.sort(rng.normal(0, 1000, n) if trial % 2 else np.round(rng.normal(0, 3, n)))
            # g either side of 0.5 and on it at n = 21: positions 10.4, 10.5, 10.6
            for q in (0, 50, 95, 100, 52, 52.5, 53, 2.5, 97.5, 99.999, float(rng.uniform(0, 100))):
                cases.append((x, q))
    return cases


def test_core_percentile_equals_numpy(core):
    cases = percentile_cases()
    got = core('pct', np.concatenate([np.r_[x.size, q, x] for x, q in cases])).reshape(-1, 3)
    for (x, q), (lo, hi, value) in zip(cases, got):
        want = np.percentile(x, q)
        assert value == want, (x.size, q, value, want)
        assert lo == np.floor((x.size - 1) * (q / 100)) and hi == min(lo + 1, x.size - 1)
        assert PC.percentile_from_statistics(x.size, q, x[int(lo)], x[int(hi)]) == want


def bin_cases():
    rng = np.random.default_rng(4)
    cases = []
    for bins in (1, 15, 30, 1024):
        for trial in range(5):
            v = rng.normal(500, 300, 400) if trial % 2 else np.round(rng.normal(500, 300, 400))
            if trial == 4:
                v = np.full(7, 123.456)                                  # min and max equal: the interval is +-0.5
            mn, mx = v.min(), v.max()
            if mn == mx:
                mn, mx = mn - 0.5, mx + 0.5
            edges = np.linspace(mn, mx, bins + 1)
            # values exactly on edges and one ulp to either side of them, inside the range
            on = np.concatenate([edges, np.nextafter(edges[:-1], np.inf), np.nextafter(edges[1:], -np.inf)])
            cases.append((bins, edges, np.concatenate([v, on])))
    return cases


def test_core_bin_rule_equals_numpy(core):
    for bins, edges, v in bin_cases():
        got = core('bin', np.r_[bins, edges, v]).astype(np.int64)
        want, wedges = np.histogram(v, bins=bins, range=(edges[0], edges[-1]))
        assert np.array_equal(wedges, edges)
        assert got.min() >= 0 and got.max() < bins and np.array_equal(np.bincount(got, minlength=bins), want), bins


def test_core_truncation_is_toward_zero(core):
    v = np.array([-0.9, -0.0, 0.0, 0.9, -1.0, 1.0, -1.5, 1.5, 65535.0, -65535.0, 65535.9, -65535.9, 0.999999999, -0.999999999, 2.0 ** 40 + 0.5])
    got = core('trunc', v)
    assert np.array_equal(got, v.astype(int).astype(np.float64)) and list(got[:4]) == [0, 0, 0, 0]
    # the histogram these give: the bin of 0 collects (-1, 1)
    x = np.array([-0.9, -0.0, 0.9, -1.0, 1.0, 1.9])
    hist, _ = PO.integer_histogram(x)
    assert list(hist) == [1, 3, 2]


def test_core_keys_preserve_the_order_and_widen_exactly(core):
    rng = np.random.default_rng(5)
    d = np.r_[rng.normal(0, 1e3, 200), -np.inf, np.inf, -0.0, 0.0, 5e-324, -5e-324, 1e308, -1e308]
    d = d[np.lexsort((~np.signbit(d), d))]                             # ascending, -0.0 before +0.0
    keys = core('key64', d, np.uint64)
    assert np.all(np.diff(keys[:d.size].astype(object)) >= 0) and np.array_equal(keys[d.size:], d.view(np.uint64))
    strict = d[1:] > d[:-1]
    assert np.all((keys[1:d.size] > keys[:d.size - 1])[strict])
    f = np.sort(np.r_[rng.normal(0, 1e3, 200), -np.inf, np.inf, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, 3e38].astype(np.float32))
    bits = f.view(np.uint32)
    out = core('key32', bits.astype(np.float64), np.uint64).reshape(4, -1)
    assert np.all(np.diff(out[0].astype(np.int64)) >= 0) and np.all((out[0][1:] > out[0][:-1])[f[1:] > f[:-1]])
    assert np.array_equal(out[1], bits.astype(np.uint64))
    assert np.array_equal(out[2].view(np.float64), f.astype(np.float64)) and np.array_equal(out[3].view(np.float64), f.astype(np.float64))


def test_core_hu_equals_the_reference_s_statements(core):
    rng = np.random.default_rng(6)
    n = 4000
    for slope, offset in ((-2085.0, 2329.0), (-2080.02235771, 2133.22867303), (1.0, 0.0)):
        q = rng.uniform(-1, 2, n) * (1.0 if slope != 1.0 else 3000.0)
        edge = PO.hu_edge_quotients(slope, offset)
        q[100:100 + edge.size] = edge
        skin, bone, cav = rng.random(n) > 0.3, rng.random(n) > 0.3, rng.random(n) > 0.9
        bone[100:100 + edge.size], cav[100:100 + edge.size] = True, False
        rec = np.stack([q, np.full(n, slope), np.full(n, offset), skin, bone, cav], 1)
        got = core('hu', rec.ravel())
        want = PO.hounsfield(q.reshape(1, 1, n), 1.0, None, bone.reshape(1, 1, n), skin.reshape(1, 1, n), cav.reshape(1, 1, n), slope, offset).ravel()
        assert np.array_equal(got, want)
        assert set(np.unique(want[~bone])) <= {-1000.0, 42.0} and (want == 3300.0).any() and (want[bone & ~cav] == -1000.0).any()
        assert want.max() == 3300.0 and want.min() == -1000.0


# ---------------------------------------------------------------- the module before the library ----------------------------------------------------------------

def test_refusals_come_before_the_library(no_library):
    v = np.zeros((3, 4, 5), np.float32)
    m = np.ones((3, 4, 5), bool)
    for bad in (v.astype(np.int16), v.astype(np.float16), v.astype(np.complex64)):
        for call in (lambda: PC.integer_histogram(bad), lambda: PC.petra_normaliser(bad), lambda: PC.masked_percentile(bad, m),
                     lambda: PC.uniform_histogram(bad, 15, 0.0), lambda: PC.convert_pseudo_ct(bad, m, m, m, m)):
            with pytest.raises(TypeError, match='float32 or float64'):
                call()
    with pytest.raises(ValueError, match='3-D'):
        PC.integer_histogram(v[0])
    with pytest.raises(ValueError, match='shape'):
        PC.masked_percentile(v, m[:2])
    with pytest.raises(ValueError, match='Percentiles'):
        PC.masked_percentile(v, m, q=101)
    for bins in (0, 1025, 2.5, None):
        with pytest.raises(ValueError, match='bins'):
            PC.uniform_histogram(v, bins, 0.0)
    with pytest.raises(ValueError, match='not a number'):
        PC.uniform_histogram(v, 15, float('nan'))
    with pytest.raises(ValueError, match='csf'):
        PC.convert_pseudo_ct(v, m, m, m)
    with pytest.raises(TypeError, match='dtype'):
        PC.convert_pseudo_ct(v, m, m, m, m, dtype=np.float16)
    with pytest.raises(ValueError, match='shape'):
        PC.convert_pseudo_ct(v, m, m[:, :3], m, m)
    with pytest.raises(ValueError, match='divisor'):
        PC.candidates(v, 0.0, None, m, 0.1, 0.6)
    with pytest.raises(ValueError, match='divisor'):
        PC.hounsfield(v, float('inf'), None, m, m, m, 1.0, 0.0)
    with pytest.raises(ValueError, match='ties'):
        LI.largest_component(m, ties='middle')
    with pytest.raises(ValueError, match='3-D'):
        PC.charm_masks(np.zeros((3, 4)))


def test_init_and_the_devices_of_the_other_modules(monkeypatch):
    monkeypatch.setattr(PC._step1, 'pick_device', lambda name, current: ([(0, 'a'), (5, 'b')], 5))
    monkeypatch.setattr(PC, '_device', 0)
    monkeypatch.setattr(BC, '_device', 2)
    monkeypatch.setattr(LI, '_device', 3)
    monkeypatch.setattr(TM, '_device', 4)
    assert PC.InitPseudoCT('b') == [(0, 'a'), (5, 'b')] and PC._device == 5
    seen = []
    monkeypatch.setattr(TM, 'drop_largest', lambda mask: seen.append(TM._device) or np.zeros(mask.shape, np.uint8))
    PC.charm_masks(np.zeros((2, 2, 2)))
    assert seen == [5] and (BC._device, LI._device, TM._device) == (2, 3, 4)


def test_abi_symbols_and_version():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _engine.load_library()
    assert lib.bfd_abi_version() == _engine.ABI_VERSION
    for entry in TC.ENTRIES:
        assert entry in _engine.ABI_SYMBOLS and hasattr(lib, entry), entry


# ---------------------------------------------------------------- the oracle's flow on the phantom ----------------------------------------------------------------

@pytest.mark.parametrize('petra', [False, True])
def test_every_step_of_the_flow_has_work_on_the_phantom(petra):
    p = PO.phantom(petra=petra)
    a = (p['zte'], p['head'], p['skin'], p['cavities'], p['csf'])
    ct, parts = PO.convert(*a, bIsPetra=petra)
    assert ct.dtype == np.float64 and ct.shape == p['zte'].shape
    # the two halves of the skull tie for the largest component, and the two islands tie with each other
    sizes = np.sort(np.bincount(PO.label(parts['candidates']).ravel())[1:])
    assert sizes.size == 4 and sizes[0] == sizes[1] == 2 and sizes[2] == sizes[3] == parts['bone_before_closing'].sum()
    assert parts['bone'].sum() > parts['bone_before_closing'].sum()
    assert 0.9 < parts['maximum'] < 1.2 and not (0.1 <= parts['maximum'] <= 0.6)
    bone_hu = ct[parts['bone'] & (p['cavities'] == 0)]
    assert ((bone_hu > 1000) & (bone_hu < 2000)).mean() > 0.8          # 0.35 of the soft-tissue level: about 1600 HU
    for switch in (dict(erode=False), dict(close=False), dict(cavities=False), dict(first_tie=False), dict(hu_from_gauss=True)):
        other, _ = PO.convert(*a, bIsPetra=petra, **switch)
        assert not np.array_equal(other, ct), switch
    if petra:
        assert parts['normaliser'] == 1800.0
    else:
        assert parts['normaliser'] == PO.masked_percentile(p['zte'], p['csf'], 95, -500)


def test_charm_masks_of_the_oracle():
    c = np.zeros((6, 7, 8))
    c[1:5, 1:6, 1:7] = 5
    c[2, 2, 2], c[2, 2, 3], c[3, 4, 5], c[3, 3, 3] = 1, 9, 4, 0          # a one-voxel cavity inside
    skin, csf, cav = PO.charm_masks(c)
    assert skin.sum() == 4 * 5 * 6 - 1 and csf.sum() == 2 and cav.sum() == 1 and cav[3, 3, 3]
