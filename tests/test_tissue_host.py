"""The tissue-mask entries without a GPU: the numpy restatements (tests/tissue_oracle.py) against the reference's own expressions; bfd_tissue_core.h,
compiled for the host, against the restatement (levels, values, exact halves, the merging table builder); the C ABI refuses bad arguments before it
looks for a device, in the header's order, and writes nothing; TissueMask raises what it says it raises before the library is loaded."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from babelbrain_amd import TissueMask as TM, _engine
from tests import tissue_calls as TC, tissue_oracle as TO


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """The library is out of reach: its path names a missing file and loading it is an error. The refusals below must come first."""
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_engine, 'LIB_PATH', str(tmp_path / 'no_such_library.so'))
    monkeypatch.setattr(_engine, '_lib', None)
    monkeypatch.setattr(_engine, 'load_library', boom)


# ---------------------------------------------------------------- the restatements ----------------------------------------------------------------

def _ct_case(seed, narrow=False):
    rng = np.random.default_rng(seed)
    shape = (7, 9, 11)
    if narrow:
        v = (np.float32(3000.0) + rng.random(shape).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    else:
        v = (rng.normal(700, 400, shape) * rng.choice([1.0, -1.0, 0.01], shape)).astype(np.float32)
    return v, rng.random(shape) < 0.6


@pytest.mark.parametrize('bits', [1, 10, 16])
@pytest.mark.parametrize('narrow', [False, True])
def test_quantize_restatement_equals_the_reference_expression(bits, narrow):
    for seed in range(8):
        v, sel = _ct_case(seed, narrow)
        lit_q, lit_u = TO.quantize_literal(v, sel, bits)
        q, table, cmap, (mn, mx) = TO.quantize(v, sel, bits)
        assert q.dtype == np.float32 and lit_q.dtype == np.float32
        assert np.array_equal(q, lit_q) and np.array_equal(table, lit_u)
        assert mn == v[sel].min() and mx == v[sel].max()
        assert np.array_equal(table[cmap[sel]], q[sel]) and not cmap[~sel].any() and np.array_equal(q[~sel], v[~sel])
        assert len(table) <= 2 ** bits and np.all(np.diff(table) > 0)


def test_cleanup_restatement_equals_the_reference_loop():
    rng = np.random.default_rng(5)
    lines = changed = 0
    for n in range(60):
        shape = tuple(int(x) for x in rng.integers(1, 9, 3))
        m = rng.choice(np.array([0, 1, 2, 3, 4], np.uint8), shape, p=[0.1, 0.2, 0.15, 0.15, 0.4])
        loc = tuple(int(rng.integers(0, s)) for s in shape)
        m[loc] = 5
        want = TO.clear_beyond_bone_loop(m)
        got, counts = TO.clear_beyond_bone(m, loc[2])
        assert np.array_equal(got, want), (shape, loc)
        assert counts[1] == (got != m).sum()
        lines += counts[0]
        changed += counts[1]
    assert lines > 100 and changed > 100


def test_paint_tie_and_threshold_rules():
    # ties: the highest label among the largest; the equal ones below it are "every component except the largest"
    assert TO.choose_labels([5, 9, 9, 2], 0) == ([4, 1, 2], 3)
    assert TO.choose_labels([5, 9, 9, 2], 2) == ([3], 3)
    assert TO.choose_labels([9], 0) == ([], 1) and TO.choose_labels([9], 2) == ([1], 1)
    # the threshold is strict and formed in float64: 0.1 * 1000 == 100.0 and 0.1 * 30 == 3.0 (0.1 * 3 is 0.30000000000000004, 0.1 * 30 is not above 3)
    assert 0.1 * 30 == 3.0 and 0.1 * 1000 == 100.0
    assert TO.choose_labels([99, 1000, 100, 101], 1) == ([1], 2)
    assert TO.choose_labels([3, 30, 4], 1) == ([], 2) and TO.choose_labels([2, 30, 3], 1) == ([1], 2)
    assert TO.choose_labels([1000, 1000, 99], 1) == ([3], 2)
    v = np.zeros((3, 3, 9), np.uint8)
    v[0, 0, 0:2] = 1
    v[2, 2, 3:5] = 1
    v[1, 1, 8] = 1
    v[0, 2, :] = 3
    out, counts = TO.paint(v, 1, 3, 0, 4)
    assert list(counts) == [3, 2, 2, 3] and out[0, 0, 0] == 4 and out[2, 2, 3] == 1 and out[1, 1, 8] == 4 and np.all(out[0, 2] == 3)
    out, counts = TO.paint(v, 1, 3, 2, 0)
    assert list(counts) == [3, 2, 1, 2] and out[0, 0, 0] == 1 and out[2, 2, 3] == 0
    out, counts = TO.paint(v, 7, 3, 0, 4)
    assert np.array_equal(out, v) and not counts.any()


def test_phantom_gives_every_step_of_the_flow_work():
    """The phantom of the flow tests (tests/test_tissue_gpu.py compares TissueMask.finish_mask with finish_mask_host on it): the cleanup changes
    voxels, a cleanup left out or given another of the focal voxel's indices gives another mask, box_fov changes which islands are painted, both
    erosion branches occur."""
    m, nfct, loc = TO.head_phantom()
    assert m[loc] == 4 and len(set(loc)) == 3
    want, degree, counts = TO.finish_mask_host(m, loc, 0.8, nfct, False)
    assert degree >= 1 and counts[0] > 100 and counts[1] > 100 and set(np.unique(want)) == {0, 1, 2, 3, 4, 5}
    for k in (-1, loc[0], loc[1], 0):                            # no cleanup; the cleanup at a wrong index
        other = TO.finish_mask_host(m, loc, 0.8, nfct, False, cleanup_k=k)[0]
        assert (other != want).sum() >= 30, k
    kept = TO.finish_mask_host(m, loc, 0.8, nfct, True)[0]
    differ = kept != want
    assert differ.sum() > 2000 and np.all(want[differ] == 4) and np.all(kept[differ] == 1)
    # the painting itself: several islands, one above a tenth of the largest
    f = m.copy()
    f[f == 2] = 1
    f = ndimage.median_filter(f, 7)
    f[nfct] = 2
    c0, c1 = TO.paint(f, 1, 3, 0, 4)[1], TO.paint(f, 1, 3, 1, 4)[1]
    assert c0[0] >= 4 and c0[2] == c0[0] - 1 and 0 < c1[2] < c0[2]
    assert TO.finish_mask_host(m, loc, 1.0, nfct, False)[1] == 0
    no_ct = TO.finish_mask_host(m, loc, 0.5, None, True)
    assert no_ct[1] >= 2 and no_ct[2] is None and (no_ct[0] == 3).any() and (no_ct[0] == 2).any()


# ---------------------------------------------------------------- bfd_tissue_core.h on the host ----------------------------------------------------------------

CORE_PROGRAM = r"""
#include "bfd_tissue_core.h"
#include <stdio.h>
#include <string.h>
#include <vector>
// argv[1] "levels": int64 bits, n; float mn, mx; float x[n]  ->  int32 level[n], float value[n]
// argv[1] "table":  int64 bits, 0; float mn, mx; uint32 presence[tq_presence_words(bits)]  ->  int64 rows, float table[rows], uint16 rank[2^bits]
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 3;
    int64_t h[2];
    float mm[2];
    if (fread(h, 8, 2, f) != 2 || fread(mm, 4, 2, f) != 2) return 4;
    const int bits = (int)h[0];
    const tq_params p = tq_make(mm[0], mm[1], bits);
    FILE *g = fopen(argv[3], "wb");
    if (!g) return 5;
    if (!strcmp(argv[1], "levels")) {
        std::vector<float> x((size_t)h[1]), v((size_t)h[1]);
        std::vector<int32_t> l((size_t)h[1]);
        if (fread(x.data(), 4, x.size(), f) != x.size()) return 6;
        for (size_t q = 0; q < x.size(); q++) { l[q] = tq_level(p, x[q]); v[q] = tq_value(p, l[q]); }
        if (fwrite(l.data(), 4, l.size(), g) != l.size() || fwrite(v.data(), 4, v.size(), g) != v.size()) return 7;
    } else {
        std::vector<uint32_t> pres((size_t)tq_presence_words(bits));
        if (fread(pres.data(), 4, pres.size(), f) != pres.size()) return 8;
        std::vector<float> table((size_t)1 << bits);
        std::vector<uint16_t> rank((size_t)1 << bits, 0xFFFF);
        const int64_t rows = tq_build_table(p, pres.data(), bits, table.data(), rank.data());
        if (fwrite(&rows, 8, 1, g) != 1 || fwrite(table.data(), 4, (size_t)rows, g) != (size_t)rows || fwrite(rank.data(), 2, rank.size(), g) != rank.size()) return 9;
    }
    fclose(f);
    fclose(g);
    return 0;
}
"""


@pytest.fixture(scope='module')
def core(tmp_path_factory):
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx, 'no C++ compiler found'
    d = tmp_path_factory.mktemp('tissuecore')
    src = d / 'tissuecore.cpp'
    src.write_text(CORE_PROGRAM)
    exe = str(d / 'tissuecore')
    subprocess.run([cxx, '-O1', '-ffp-contract=off', '-I', os.path.join(os.path.dirname(_engine.LIB_PATH), 'csrc'), str(src), '-o', exe, '-lm'], check=True)

    def levels(x, mn, mx, bits):
        inp, outp = str(d / 'in.bin'), str(d / 'out.bin')
        x = np.ascontiguousarray(x, np.float32)
        with open(inp, 'wb') as f:
            f.write(np.array([bits, x.size], np.int64).tobytes() + np.array([mn, mx], np.float32).tobytes() + x.tobytes())
        subprocess.run([exe, 'levels', inp, outp], check=True)
        return np.fromfile(outp, np.int32, x.size), np.fromfile(outp, np.float32, x.size, offset=4 * x.size)

    def table(presence_levels, mn, mx, bits):
        inp, outp = str(d / 'in.bin'), str(d / 'out.bin')
        words = np.zeros(max(2, 2 ** bits // 32), np.uint32)
        lv = np.asarray(presence_levels, np.int64)
        np.bitwise_or.at(words, lv >> 5, (np.uint32(1) << (lv & 31).astype(np.uint32)))
        with open(inp, 'wb') as f:
            f.write(np.array([bits, 0], np.int64).tobytes() + np.array([mn, mx], np.float32).tobytes() + words.tobytes())
        subprocess.run([exe, 'table', inp, outp], check=True)
        rows = int(np.fromfile(outp, np.int64, 1)[0])
        return np.fromfile(outp, np.float32, rows, offset=8), np.fromfile(outp, np.uint16, 2 ** bits, offset=8 + 4 * rows)
    return levels, table


@pytest.mark.parametrize('bits', [1, 2, 10, 16])
def test_core_levels_and_values_equal_the_restatement(core, bits):
    for seed, narrow in ((1, False), (2, True), (3, False)):
        v, sel = _ct_case(seed, narrow)
        x = v[sel]
        want_l, want_v, _, _ = TO.quantize_levels(x, x.min(), x.max(), bits)
        got_l, got_v = core[0](x, x.min(), x.max(), bits)
        assert np.array_equal(got_l, want_l) and np.array_equal(got_v, want_v)
        assert got_l.min() == 0 and got_l.max() == 2 ** bits - 1


def test_core_exact_halves_go_to_even(core):
    """mn = 0 and mx = M make s = r = 1: level(k + 0.5) is a tie at every k, resolved to the even neighbour"""
    for bits in (4, 10):
        M = 2 ** bits - 1
        k = np.arange(M, dtype=np.float32)
        x = np.concatenate([k + np.float32(0.5), [np.float32(0), np.float32(M)]]).astype(np.float32)
        got_l, got_v = core[0](x, 0.0, float(M), bits)
        even = (k + (k.astype(np.int64) % 2)).astype(np.int64)            # k even: down to k; k odd: up to k + 1
        assert np.array_equal(got_l[:-2], even) and got_l[-2] == 0 and got_l[-1] == M
        assert np.array_equal(got_l, TO.quantize_levels(x, 0.0, float(M), bits)[0])
        assert np.array_equal(got_v, got_l.astype(np.float32))
        assert np.array_equal(got_l[:4], [0, 2, 2, 4])


def test_core_table_merges_equal_values(core):
    """mn = 3000, A = 0.5, 16 bits: the 65536 levels give 2049 distinct float32 values (the spacing of float32 at 3000 is 2^-12, the step 0.5 / 65535).
    Every level present; the builder must return the merged values and ranks that index them."""
    bits, mn, mx = 16, np.float32(3000.0), np.float32(3000.5)
    lv = np.arange(2 ** bits)
    r = np.float32(np.float32(mx - mn) / np.float32(2 ** bits - 1))
    values = TO.level_values(lv, mn, r)
    assert np.all(np.diff(values) >= 0)
    want = np.unique(values)
    assert len(want) == 2049
    table, rank = core[1](lv, mn, mx, bits)
    assert np.array_equal(table, want)
    assert np.array_equal(table[rank], values) and np.array_equal(rank, np.searchsorted(want, values))
    # a sparse set: absent levels open no row and keep their sentinel, equal neighbours across a chunk boundary still merge
    some = np.array([0, 31, 63, 64, 65, 4096, 4097, 40000, 65535])
    table, rank = core[1](some, mn, mx, bits)
    assert np.array_equal(table, np.unique(values[some])) and np.array_equal(table[rank[some]], values[some])
    assert len(table) < len(some) and rank[1] == 0xFFFF
    # few levels: one chunk, most of it beyond 2^bits
    for b in (1, 2, 5):
        lv = np.arange(2 ** b)
        table, rank = core[1](lv, -5.0, 11.0, b)
        v = TO.level_values(lv, np.float32(-5), np.float32(np.float32(16) / np.float32(2 ** b - 1)))
        assert np.array_equal(table, v) and np.array_equal(rank, lv)


# ---------------------------------------------------------------- refusals ----------------------------------------------------------------

def test_python_refuses_before_the_library(no_library):
    vol = np.zeros((3, 4, 5), np.uint8)
    ct = np.zeros((3, 4, 5), np.float32)
    with pytest.raises(TypeError):
        TM.paint_components(vol.astype(np.int32), 1, 4, 0)
    with pytest.raises(ValueError, match='3-D'):
        TM.paint_components(vol[0], 1, 4, 0)
    for kw in (dict(value=256), dict(fill=-1), dict(select=3), dict(connectivity=0), dict(value=1.5)):
        with pytest.raises(ValueError):
            TM.paint_components(vol, **dict(dict(value=1, fill=4, select=0), **kw))
    with pytest.raises(TypeError, match='float32'):
        TM.quantize_values(ct.astype(np.float64), vol)
    with pytest.raises(TypeError, match='float32'):
        TM.quantize_values(vol, vol)
    with pytest.raises(TypeError, match='nfct'):
        TM.quantize_values(ct, ct)
    with pytest.raises(ValueError, match='shape'):
        TM.quantize_values(ct, vol[:2])
    for bits in (0, 17, 2.5):
        with pytest.raises(ValueError, match='CT_quantification'):
            TM.quantize_values(ct, vol, bits)
    for k in (-1, 5, 1.5):
        with pytest.raises(ValueError, match='kFocal'):
            TM.prefocal_cleanup(vol, k)
    with pytest.raises(ValueError, match='bone'):
        TM.prefocal_cleanup(vol, 1, bone=(2,))
    with pytest.raises(ValueError, match='to_value'):
        TM.prefocal_cleanup(vol, 1, to_value=300)
    with pytest.raises(TypeError):
        TM.prefocal_cleanup(ct, 1)
    with pytest.raises(ValueError, match='LocFocalPoint'):
        TM.finish_mask(vol, (1, 1, 5))
    with pytest.raises(ValueError, match='nfct'):
        TM.finish_mask(vol, (1, 1, 1), nfct=np.zeros((3, 4, 6), bool))
    for call in (lambda: TM.paint_components(vol, 1, 4, 0), lambda: TM.merge_islands(vol == 0), lambda: TM.drop_largest(vol),
                 lambda: TM.quantize_values(ct, vol == 0), lambda: TM.prefocal_cleanup(vol, 4)):
        with pytest.raises(AssertionError, match='library was loaded'):        # a good call gets as far as the library
            call()


def test_finish_mask_borrows_the_other_modules_for_its_device_only(monkeypatch):
    """finish_mask runs MedianFilter and BinaryErode on TissueMask's device and leaves those modules' own selection as it was, also when a call
    raises; InitTissueMask does not touch them."""
    from babelbrain_amd import BinaryClosing as BC, MedianFilter as MD
    seen = []
    monkeypatch.setattr(TM, '_device', 3)
    monkeypatch.setattr(MD, '_device', 1)
    monkeypatch.setattr(BC, '_device', 2)
    monkeypatch.setattr(MD, 'MedianFilter', lambda m, size: (seen.append(('median', MD._device)), m)[1])
    monkeypatch.setattr(BC, 'BinaryErode', lambda b, iterations=1: (seen.append(('erode', BC._device)), b)[1])
    v = np.full((3, 3, 12), 2, np.uint8)
    out = TM.finish_mask(v, (1, 1, 2), 0.8)
    assert seen == [('median', 3), ('erode', 3)] and (MD._device, BC._device) == (1, 2) and out[1, 1, 2] == 5

    def boom(m, size):
        raise RuntimeError('median')
    monkeypatch.setattr(MD, 'MedianFilter', boom)
    with pytest.raises(RuntimeError, match='median'):
        TM.finish_mask(v, (1, 1, 2), 0.8)
    assert MD._device == 1
    monkeypatch.setattr(TM._step1, 'pick_device', lambda name, current: ([(0, 'a'), (5, 'b')], 5))
    TM.InitTissueMask('b')
    assert TM._device == 5 and (MD._device, BC._device) == (1, 2)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


@pytest.mark.parametrize('entry', TC.ENTRIES)
def test_abi_refuses_before_a_device_in_the_header_s_order(lib, entry):
    """-1 with the text of the first fault the header lists, whether or not a device exists, with every output and kernelMs untouched."""
    assert entry in _engine.ABI_SYMBOLS and hasattr(lib, entry) and lib.bfd_abi_version() == _engine.ABI_VERSION
    words = {n: w for n, w, _ in TC.faults(entry)}
    for names, first in TC.ordered_plants(entry):
        c = TC.planted(entry, names)
        assert c.run(lib) == -1, names
        text = lib.bfd_last_error().decode()
        assert text.startswith(entry) and words[first] in text and TM.DATA_REFUSED not in text, (names, text)
        assert c.untouched(), names
    nulls = {'bfd_paint_components3d': ('out', 'counts'), 'bfd_quantize_values3d': ('table', 'numValues', 'range'),
             'bfd_clear_beyond_bone3d': ('out', 'counts')}[entry]
    for name in nulls:
        c = TC.Case(entry, **{'want_' + name: False})
        assert c.run(lib) == -1 and 'null' in lib.bfd_last_error().decode() and c.untouched(), name
    more = {'bfd_paint_components3d': (dict(value=-1), dict(value=256), dict(fill=-1), dict(connectivity=0), dict(select=-1)),
            'bfd_quantize_values3d': (dict(bits=0), dict(values=None)),
            'bfd_clear_beyond_bone3d': (dict(kFocal=-1), dict(boneA=256), dict(from_=-1), dict(to=256))}[entry]
    for kw in more:
        c = TC.Case(entry, **kw)
        assert c.run(lib) == -1 and c.untouched(), kw
    if lib.bfd_device_count() == 0:
        c = TC.Case(entry)
        assert c.run(lib) == -3 and c.untouched()
        if entry == 'bfd_quantize_values3d':                    # the nullable outputs are no argument error
            c = TC.Case(entry, want_quantized=False, want_map=False)
            assert c.run(lib) == -3 and c.untouched()
