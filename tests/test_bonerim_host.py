"""The host side of the bone-rim correction (babelbrain_amd/BoneRim.py, csrc/bfd_bonerim_core.h) without a device: the phantom gives every branch
of the flow work, each planted fault changes the oracle's result, the global mean reaches the global-mean voxels alone, and the core header compiled
for the host gives numpy's bits: the weight table, the blend operation by operation, the exact mean; numpy's own pairwise mean lies within its
a-priori bound of the exact one. The refusals of BoneRim.py come before the library is loaded."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from babelbrain_amd import BoneRim as BR, _engine
from tests import bonerim_oracle as BO

F32 = np.float32


@pytest.fixture(scope='module')
def head():
    return BO.phantom()


@pytest.fixture(scope='module')
def flows(head):
    ct, bone = head
    return {tuple(r): BO.correct(ct, bone, r) for r in ([3, 3, 3], [2, 2, 4], [5, 5, 3])}


# ---------------------------------------------------------------- the phantom and the oracle ----------------------------------------------------------------

def test_odd_box():
    for ratio, want in (([3, 3, 3], [3, 3, 3]), ([2, 2, 4], [3, 3, 5]), ([1, 1, 1], [3, 3, 3]), ([0, 6, 7], [3, 7, 7]), ([30, 31, 5], [31, 31, 5])):
        given = list(ratio)
        assert BR.odd_box(given) == want == BO.odd_box(ratio) and given == ratio
    with pytest.raises(ValueError):
        BR.odd_box([3, 3])


@pytest.mark.parametrize('ratio', [(3, 3, 3), (2, 2, 4)])
def test_the_phantom_gives_every_branch_work(flows, ratio):
    out, fields, stats = flows[ratio]
    print(ratio, stats, 'lowered', fields['lowered'])
    for name in ('interior', 'edge', 'global_mean_voxels', 'clipped', 'max_d2', 'changed', 'dense', 'bone'):
        assert stats[name] > 0, name
    assert fields['lowered'] > 0
    assert stats['edge'] + stats['interior'] == stats['bone']


def test_a_wide_box_alone_is_not_enough(flows):
    assert flows[(5, 5, 3)][2]['global_mean_voxels'] == 0


@pytest.mark.parametrize('fault', BO.FAULTS)
def test_every_planted_fault_changes_the_result(head, flows, fault):
    ct, bone = head
    got = BO.correct(ct, bone, [2, 2, 4], fault=fault)[0]
    differ = int(np.count_nonzero(got != flows[(2, 2, 4)][0]))
    print(fault, differ)
    assert differ > 0


def test_the_threshold_in_float64_is_the_threshold_in_float32():
    """float32(1e-6) < 1e-6 < the next float32, so for a float32 bm the comparisons bm > float32(1e-6) and float64(bm) > 1e-6 agree on every value:
    on float32(1e-6) itself both are false. The fault that CAN change a result is the local mean taken in float64 (local_mean_float64 above)."""
    t = F32(1e-6)
    assert float(t) < 1e-6 < float(np.nextafter(t, F32(1)))
    bm = np.array([np.nextafter(t, F32(0)), t, np.nextafter(t, F32(1)), 0.0, 1.0], F32)
    assert np.array_equal(bm > 1e-6, bm.astype(np.float64) > 1e-6)
    assert (bm > 1e-6).tolist() == [False, False, True, False, True]


def test_the_global_mean_reaches_the_global_mean_voxels_alone(head, flows):
    ct, bone = head
    ref, fields, stats = flows[(3, 3, 3)]
    took = fields['edge'] & ~(fields['bm'] > F32(1e-6))
    assert int(took.sum()) == stats['global_mean_voxels']
    exact, own = BO.exact_mean(ct), BO.numpy_mean(ct)
    print('numpy mean %r, exact mean %r' % (own, exact))
    assert own.dtype == np.float32 and fields['global_mean'] == own
    other = BO.correct(ct, bone, [3, 3, 3], global_mean=exact)[0]
    assert not np.any((other != ref) & ~took)
    far = BO.correct(ct, bone, [3, 3, 3], global_mean=exact + F32(500))[0]         # a mean that is visibly another
    assert np.any(far != ref) and not np.any((far != ref) & ~took)


# ---------------------------------------------------------------- the core header ----------------------------------------------------------------

CORE_PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "bfd_bonerim_core.h"
// <mode> <in> <out>: float64 records in, 64-bit words out
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
    std::vector<uint64_t> words;
    const std::string mode = argv[1];
    if (mode == "table") {               // [scale, last d2]: the table's length, then the weight of every d2 = 0 .. last as the kernel reads it
        std::vector<double> w;
        rim_weight_table(in[0], (int64_t)in[1], gauss_numpy_vector_exp(), w);
        out.push_back((double)w.size());
        for (int64_t d2 = 0; d2 <= (int64_t)in[1]; d2++) out.push_back(rim_weight(w.data(), (int64_t)w.size(), d2));
    } else if (mode == "blend") {        // records [o, bi, bm, gmean, w, maxBoost]: lm, took the global mean, the stored value, clipped
        for (size_t p = 0; p + 5 < in.size(); p += 6) {
            bool global, clipped;
            const float lm = rim_local_mean((float)in[p + 1], (float)in[p + 2], (float)in[p + 3], &global);
            const float r = rim_blend((float)in[p], lm, in[p + 4], in[p + 5], &clipped);
            out.push_back((double)lm); out.push_back(global ? 1.0 : 0.0); out.push_back((double)r); out.push_back(clipped ? 1.0 : 0.0);
        }
    } else if (mode == "mean") {         // dense values: S, the count, the bits of the mean widened
        uint64_t S = 0;
        for (double v : in) S += rim_fixed((float)v);
        const double m = (double)rim_mean(S, (uint64_t)in.size());
        uint64_t mb;
        memcpy(&mb, &m, 8);
        words.push_back(S); words.push_back((uint64_t)in.size()); words.push_back(mb);
    } else if (mode == "voxel") {        // records [ct, bone, have floor, floor, threshold]: the floored value, dense, the product's bits
        for (size_t p = 0; p + 4 < in.size(); p += 5) {
            const float y = rim_floor((float)in[p], in[p + 1] != 0, in[p + 2] != 0, (float)in[p + 3]);
            const bool dense = rim_dense(y, (float)in[p + 4]);
            const float prod = rim_dense_product(y, dense);
            uint32_t pb;
            memcpy(&pb, &prod, 4);
            out.push_back((double)y); out.push_back(dense ? 1.0 : 0.0); out.push_back((double)pb);
        }
    } else return 4;
    f = fopen(argv[3], "wb");
    if (!f) return 5;
    if (!out.empty()) fwrite(out.data(), 8, out.size(), f);
    if (!words.empty()) fwrite(words.data(), 8, words.size(), f);
    fclose(f);
    return 0;
}
'''


@pytest.fixture(scope='module')
def core(tmp_path_factory):
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx, 'no C++ compiler found'
    d = tmp_path_factory.mktemp('bonerimcore')
    src = d / 'bonerimcore.cpp'
    src.write_text(CORE_PROGRAM)
    exe = str(d / 'bonerimcore')
    subprocess.run([cxx, '-O1', '-std=c++14', '-ffp-contract=off', '-I', os.path.join(os.path.dirname(_engine.LIB_PATH), 'csrc'), str(src), '-o', exe, '-lm'],
                   check=True)

    def run(mode, data, out_dtype=np.float64):
        inp, outp = str(d / 'in.bin'), str(d / 'out.bin')
        np.ascontiguousarray(data, np.float64).tofile(inp)
        subprocess.run([exe, mode, inp, outp], check=True)
        return np.fromfile(outp, out_dtype)
    return run


@pytest.mark.parametrize('scale', [1.5, 2.5, 3.5, 15.5])
def test_core_weight_table_equals_numpy(core, scale):
    last = 20000
    got = core('table', [scale, last])
    want = np.exp(-np.sqrt(np.arange(last + 1, dtype=np.float64)) / scale)
    assert np.array_equal(got[1:], want), int(np.count_nonzero(got[1:] != want))
    assert got[1] == 1.0 and got[0] == last + 1                    # nothing underflows this early


def test_core_weight_table_ends_where_the_weights_are_zero(core):
    scale, last = 0.004, 20                                         # -sqrt(d2) / scale is below -750 from d2 = 10 on
    got = core('table', [scale, last])
    want = np.exp(-np.sqrt(np.arange(last + 1, dtype=np.float64)) / scale)
    assert np.array_equal(got[1:], want)
    assert got[0] == np.flatnonzero(want)[-1] + 1 < last + 1


def numpy_blend(o, bi, bm, gmean, w, max_boost):
    """steps 7-8 on arrays, in the reference's words and types"""
    with np.errstate(invalid='ignore', divide='ignore'):
        lm = np.where(bm > 1e-6, bi / bm, gmean)
    assert lm.dtype == np.float32
    correct_vals = o + w * (lm - o)
    delta = correct_vals - o
    delta_clipped = np.clip(delta, a_min=None, a_max=max_boost)
    correct_vals = o + delta_clipped
    assert correct_vals.dtype == np.float64
    stored = np.empty(o.shape, np.float32)
    stored[...] = correct_vals
    return lm, ~(bm > F32(1e-6)), stored, delta > max_boost


def blend_cases():
    rng = np.random.default_rng(5)
    n = 4000
    o = rng.normal(500, 300, n).astype(F32)
    bm = (rng.random(n) ** 4).astype(F32)
    bm[::7] = (rng.random(bm[::7].size) * 2e-6).astype(F32)
    bi = (bm * rng.normal(1600, 500, n)).astype(F32)
    w = np.exp(-np.sqrt(rng.integers(0, 500, n).astype(np.float64)) / rng.choice([1.5, 2.5, 3.5], n))
    rows = [np.stack([o, bi, bm, np.full(n, F32(1739.0594)), w, np.full(n, 1000.0)], 1).astype(np.float64)]
    t = F32(1e-6)
    one_down, one_up = np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)
    planted = [
        # delta exactly 1000 and the float64 values either side of it (bm = 1: lm = bi)
        (300.0, 1300.0, 1.0, 0.0, 1.0, 1000.0), (300.0, 1300.0, 1.0, 0.0, one_down, 1000.0), (300.0, 1300.0, 1.0, 0.0, one_up, 1000.0),
        (300.0, 1300.0, 1.0, 0.0, 1.0, float(np.nextafter(1000.0, 0.0))), (300.0, 1300.0, 1.0, 0.0, 1.0, float(np.nextafter(1000.0, 2000.0))),
        # bm at float32(1e-6) and its two neighbours
        (450.0, 2e-3, float(np.nextafter(t, F32(0))), 1700.0, 0.5, 1000.0), (450.0, 2e-3, float(t), 1700.0, 0.5, 1000.0),
        (450.0, 2e-3, float(np.nextafter(t, F32(1))), 1700.0, 0.5, 1000.0), (450.0, 0.0, 0.0, 1700.0, 0.5, 1000.0),
        # lm < o: the value is lowered, and the clip has no lower side
        (2700.0, 900.0, 1.0, 0.0, 0.9, 1000.0), (2700.0, -5000.0, 1.0, 0.0, 1.0, 1000.0),
        # w = 1 and w denormal
        (431.25, 1517.375, 1.0, 0.0, 1.0, 1e9), (431.25, 1517.375, 1.0, 0.0, 5e-324, 1000.0), (431.25, 1517.375, 1.0, 0.0, 0.0, 1000.0),
        # results on a float32 rounding tie: o + 2^-14 at o = 1024 (even: down) and at o = 1024 + 2^-13 (odd: up), and three quarters of an ulp
        (1024.0, 1025.0, 1.0, 0.0, 2.0 ** -14, 1000.0), (1024.0 + 2.0 ** -13, 1025.0 + 2.0 ** -13, 1.0, 0.0, 2.0 ** -14, 1000.0),
        (1024.0, 1025.0, 1.0, 0.0, 1.5 * 2.0 ** -14, 1000.0), (1024.0, 1025.0, 1.0, 0.0, float(np.nextafter(2.0 ** -14, 0.0)), 1000.0),
        # a negative value and a maxBoost below zero
        (-200.0, 900.0, 1.0, 0.0, 0.25, 1000.0), (600.0, 900.0, 1.0, 0.0, 0.25, -10.0),
    ]
    planted = np.array(planted, np.float64)
    planted[:, :4] = planted[:, :4].astype(F32)                     # o, bi, bm and gmean are float32 values
    rows.append(planted)
    return np.concatenate(rows)


def test_core_blend_equals_numpy_operation_by_operation(core):
    c = blend_cases()
    assert np.array_equal(c[:, :4], c[:, :4].astype(F32))          # the float32 inputs are float32 values
    got = core('blend', c).reshape(-1, 4)
    lm, took, stored, clipped = numpy_blend(c[:, 0].astype(F32), c[:, 1].astype(F32), c[:, 2].astype(F32), c[:, 3].astype(F32), c[:, 4], c[:, 5])
    assert np.array_equal(got[:, 1] != 0, took) and took.any() and not took.all()
    assert np.array_equal(got[:, 0].astype(F32).view(np.uint32), lm.view(np.uint32))
    assert np.array_equal(got[:, 2].astype(F32).view(np.uint32), stored.view(np.uint32)), np.flatnonzero(got[:, 2].astype(F32) != stored)
    assert np.array_equal(got[:, 3] != 0, clipped) and clipped.any()
    planted = stored[-20:]
    assert np.all(planted[:5] == 1300)                              # a float64 ulp either side of 1000 is far below a float32 ulp of 1300
    assert clipped[-20:][:5].tolist() == [False, False, True, True, False]
    assert took[-20:][5:9].tolist() == [True, True, False, True]
    assert planted[9] < 2700 and planted[10] == -5000
    assert planted[11] == F32(1517.375) and planted[12] == F32(431.25) and planted[13] == F32(431.25)
    assert planted[14] == 1024 and planted[15] == F32(1024 + 2.0 ** -12) and planted[16] == F32(1024 + 2.0 ** -13) and planted[17] == 1024
    assert planted[19] == 590


def test_core_voxel_steps_equal_numpy(core):
    rng = np.random.default_rng(6)
    ct = np.concatenate([rng.normal(600, 400, 500), [800.0, np.nextafter(F32(800), F32(0)), -0.0, 0.0, -3.5, 299.99, 300.0]]).astype(F32)
    bone = (rng.random(ct.size) < 0.6)
    for have, floor in ((0, 0.0), (1, 300.0)):
        got = core('voxel', np.stack([ct, bone, np.full(ct.size, have), np.full(ct.size, floor), np.full(ct.size, 800.0)], 1).astype(np.float64)).reshape(-1, 3)
        y = ct.copy()
        if have:
            b = y[bone]
            b[b < floor] = floor
            y[bone] = b
        dense = y >= 800.0
        prod = y * dense
        assert prod.dtype == np.float32 and np.signbit(prod).any()
        assert np.array_equal(got[:, 0].astype(F32), y) and np.array_equal(got[:, 1] != 0, dense)
        assert np.array_equal(got[:, 2].astype(np.uint32), prod.view(np.uint32))


def test_core_exact_mean_equals_python_integers(core, head):
    rng = np.random.default_rng(8)
    for vals in (head[0][head[0] >= 800], rng.uniform(512, 131071, 5000).astype(F32), np.array([512.0], F32),
                 np.array([np.nextafter(F32(131072), F32(0))] * 3, F32), (512 + rng.integers(0, 2 ** 23, 3000) * 2.0 ** -14).astype(F32)):
        S, count, bits = core('mean', vals, np.uint64)
        want = sum(int(v) for v in (vals.astype(np.float64) * 16384.0))
        assert int(S) == want and int(count) == vals.size
        mean = np.array([bits], np.uint64).view(np.float64)[0]
        assert mean == np.float32(float(want) / (16384.0 * vals.size)) == BO.exact_mean(vals, 512.0)


def test_numpy_mean_within_its_bound_of_the_exact_mean(head):
    """numpy's float32 .mean() of n positive values is its pairwise sum divided by n. The sum: blocks of at most 128 values, eight accumulators of up
    to 16 values each (15 roundings), three levels to join them, up to 7 single additions for the rest: at most 25 roundings on any value's way
    through a block. Above the blocks the halves are joined pairwise; a part of d halvings has at most n / 2^d + 14 values (the first half is rounded
    down to a multiple of 8), so there are at most ceil(log2(n / 64)) levels, one rounding each. With D = 25 + ceil(log2(n / 64)), u = 2^-24 and
    positive values, |sum_np - sum| <= ((1 + u)^D - 1) sum. The division rounds once more, and the exact mean is itself rounded to float32 once
    (after a float64 division and a float64 conversion of S, 2^-52 between them). So
        |numpy mean - exact mean| <= ((1 + u)^(D + 1) - 1 + 1.0001 u) mean."""
    rng = np.random.default_rng(9)
    for vals in (head[0][head[0] >= 800], rng.uniform(512, 4000, 100000).astype(F32), rng.uniform(512, 131071, 1 << 20).astype(F32),
                 rng.uniform(800, 3000, 129).astype(F32), rng.uniform(800, 3000, 7).astype(F32)):
        n = vals.size
        D = 25 + max(0, math.ceil(math.log2(n / 64)))
        u = 2.0 ** -24
        exact, own = BO.exact_mean(vals, 512.0), vals.mean()
        bound = (math.expm1((D + 1) * math.log1p(u)) + 1.0001 * u) * float(exact)
        print('n %d: numpy mean %r, exact mean %r, difference %.3g (%d ulp), bound %.3g' % (
            n, own, exact, abs(float(own) - float(exact)), abs(int(own.view(np.int32)) - int(exact.view(np.int32))), bound))
        assert own.dtype == np.float32 and abs(float(own) - float(exact)) <= bound


# ---------------------------------------------------------------- the module's own refusals ----------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """The library is out of reach: its path names a missing file and loading it is an error. The refusals below must come first."""
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_engine, 'LIB_PATH', str(tmp_path / 'no_such_library.so'))
    monkeypatch.setattr(_engine, '_lib', None)
    monkeypatch.setattr(_engine, 'load_library', boom)


def test_argument_errors_come_before_the_library(no_library, head):
    ct, bone = head
    with pytest.raises(TypeError):
        BR.maximize_bone_rim(ct.astype(np.float64), bone, [3, 3, 3])
    with pytest.raises(TypeError):
        BR.maximize_bone_rim(ct.tolist(), bone, [3, 3, 3], inplace=True)
    for kw in (dict(ndataCT=ct[0]), dict(nfct=bone[1:]), dict(RatioCTVoxels=[3, 3]), dict(RatioCTVoxels=[3, 33, 3]), dict(RatioCTVoxels=[3, -1, 3]),
               dict(interior_high_th=500.0), dict(interior_high_th=float('nan')), dict(max_boost=float('nan')), dict(floor=float('inf')),
               dict(global_mean=float('nan')), dict(ndataCT=ct.transpose(2, 1, 0), nfct=bone.transpose(2, 1, 0), inplace=True)):
        args = dict(ndataCT=ct, nfct=bone, RatioCTVoxels=[3, 3, 3])
        args.update(kw)
        with pytest.raises(ValueError):
            BR.maximize_bone_rim(**args)
    ro = ct.copy()
    ro.flags.writeable = False
    with pytest.raises(ValueError):
        BR.maximize_bone_rim(ro, bone, [3, 3, 3], inplace=True)
