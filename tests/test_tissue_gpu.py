"""The tissue-mask entries on the device: bfd_paint_components3d, bfd_quantize_values3d, bfd_clear_beyond_bone3d and TissueMask.finish_mask equal their
numpy restatements (tests/tissue_oracle.py) element for element, outputs and counts alike; the call contract of csrc/bfd_call.h holds."""
import os

import numpy as np
import pytest

from babelbrain_amd import MappingFilter as MF, TissueMask as TM, _engine
from tests import tissue_calls as TC, tissue_oracle as TO

pytestmark = pytest.mark.gpu

N3S = (1, 31, 32, 33, 63, 64, 65, 130)


def same(got, want, what=''):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, int((got != want).sum()))


# ---------------------------------------------------------------- paint ----------------------------------------------------------------

def check_paint(v, value, fill, select, connectivity=3, what=''):
    out, counts = TM.paint_components(v, value, fill, select, connectivity)
    want, wcounts = TO.paint(v, value, connectivity, select, fill)
    same(out, want, what)
    assert list(counts) == list(wcounts), (what, counts, wcounts)
    return out, counts


def speckle(shape, seed, p1=0.2):
    rng = np.random.default_rng(seed)
    rest = (1 - p1) / 5
    return rng.choice(np.arange(6, dtype=np.uint8), shape, p=[rest, p1, rest, rest, rest, rest])


@pytest.mark.parametrize('shape', [(9, 17, 130), (17, 9, 65), (8, 8, 64), (1, 1, 1), (3, 70, 2)])
def test_paint_across_label_tiles(shape):
    """Values 0 to 5 with value = 1: the tiles of 8 x 8 x 64 are crossed on faces, edges and corners; everything that is not painted is copied."""
    v = speckle(shape, sum(shape), 0.22)
    for connectivity in (1, 2, 3):
        for select in (0, 1, 2):
            out, counts = check_paint(v, 1, 4, select, connectivity, (shape, connectivity, select))
            assert np.array_equal(out[v != 1], v[v != 1])
    check_paint(v, 3, 9, 0, 2, 'value 3')
    if max(shape) > 8:
        assert counts[0] > 1 and counts[3] > 0


def test_paint_no_foreground_and_one_component():
    v = speckle((9, 10, 70), 3)
    v[v == 1] = 0
    for select in (0, 1, 2):
        out, counts = check_paint(v, 1, 4, select)
        assert np.array_equal(out, v) and not counts.any()
    v[2:8, 3:9, 60:68] = 1                             # one component across a tile face
    out, counts = check_paint(v, 1, 4, 0)
    assert np.array_equal(out, v) and list(counts) == [1, 6 * 6 * 8, 0, 0]
    out, counts = check_paint(v, 1, 4, 2)
    assert list(counts) == [1, 288, 1, 288] and not (out == 1).any()


def test_paint_equal_sizes_the_higher_label_is_the_largest():
    v = np.zeros((10, 10, 70), np.uint8)
    v[1:3, 1:3, 1:3] = 1                               # label 1
    v[6:8, 6:8, 62:64] = 1                             # label 2, the same 8 voxels
    v[4, 4, 30] = 1                                    # label 2 in raster order: the cube above becomes label 3
    out, counts = check_paint(v, 1, 4, 0)
    assert list(counts) == [3, 8, 2, 9] and out[1, 1, 1] == 4 and out[4, 4, 30] == 4 and out[6, 6, 62] == 1
    out, counts = check_paint(v, 1, 0, 2)
    assert list(counts) == [3, 8, 1, 8] and out[1, 1, 1] == 1 and out[6, 6, 62] == 0
    check_paint(v, 1, 4, 1)                            # 8 < 0.8 is false: the equal one stays, the single voxel too (1 < 0.8 is false)


def test_paint_threshold_of_a_tenth():
    v = np.zeros((14, 50, 14), np.uint8)
    v[1:11, 1:11, 1:11] = 1                            # L = 1000
    v[1:10, 13:24, 12] = 1                             # 99
    v[1:11, 26:36, 12] = 1                             # 100
    v[1:11, 38:48, 12] = 1
    v[1, 38, 11] = 1                                   # 101
    out, counts = check_paint(v, 1, 4, 1)
    assert list(counts) == [4, 1000, 1, 99] and out[1, 13, 12] == 4 and out[1, 26, 12] == 1 and out[1, 38, 12] == 1
    w = np.zeros((8, 8, 8), np.uint8)
    w[0:5, 0:6, 0] = 1                                 # L = 30
    w[7, 0:3, 4] = 1                                   # 3: 3 < 0.1 * 30 == 3.0 is false
    w[7, 6:8, 7] = 1                                   # 2
    out, counts = check_paint(w, 1, 4, 1)
    assert list(counts) == [3, 30, 1, 2] and out[7, 0, 4] == 1 and out[7, 6, 7] == 4


def test_paint_connectivity_by_edge_and_corner():
    v = np.zeros((12, 12, 70), np.uint8)
    v[0, 0, 0] = v[1, 1, 0] = 1                        # an edge
    v[2, 2, 1] = 1                                     # a corner with (1, 1, 0)
    v[7, 7, 63] = v[8, 8, 64] = 1                      # a corner across the corner of a tile
    v[7, 3, 20] = v[8, 4, 20] = 1                      # an edge across a tile face
    n = {}
    for connectivity in (1, 2, 3):
        n[connectivity] = check_paint(v, 1, 4, 0, connectivity)[1][0]
        check_paint(v, 1, 4, 2, connectivity)
    assert n == {1: 7, 2: 5, 3: 3}


def test_paint_thousands_of_single_voxels():
    v = np.zeros((32, 32, 24), np.uint8)
    v[::2, ::2, ::2] = 1
    out, counts = check_paint(v, 1, 4, 0)
    assert list(counts) == [3072, 1, 3071, 3071] and out[30, 30, 22] == 1
    check_paint(v, 1, 4, 1)
    check_paint(v, 1, 0, 2)
    check_paint(v, 1, 4, 0, 1)


def test_paint_repeats_are_byte_identical():
    v = speckle((20, 23, 131), 9, 0.25)
    first = TM.paint_components(v, 1, 4, 1)
    for _ in range(3):
        again = TM.paint_components(v, 1, 4, 1)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    assert np.array_equal(TM.merge_islands(v), TO.paint(v, 1, 3, 0, 4)[0]) and np.array_equal(TM.merge_islands(v, True), first[0])
    m = (v == 1).astype(np.uint8)
    assert np.array_equal(TM.drop_largest(m), TO.paint(m, 1, 3, 2, 0)[0])
    assert np.array_equal(TM.drop_largest(v == 1), TO.paint(m, 1, 3, 2, 0)[0])


# ---------------------------------------------------------------- quantise ----------------------------------------------------------------

def check_quantize(values, mask, bits, what=''):
    table, cmap, (mn, mx), q = TM.quantize_values(values, mask, bits, return_quantized=True)
    wq, wtable, wmap, (wmn, wmx) = TO.quantize(values, mask, bits)
    same(q, wq, what)
    same(table, wtable, what)
    same(cmap, wmap, what)
    assert mn == wmn and mx == wmx, what
    sel = np.asarray(mask) != 0
    assert np.array_equal(cmap[sel], np.searchsorted(table, q[sel])), what
    same(MF.MapFilter(q, sel.astype(np.uint8), table), cmap, what)
    return table, cmap, q


def ct_volume(shape, seed, share=0.4):
    rng = np.random.default_rng(seed)
    v = (rng.normal(300, 900, shape)).astype(np.float32)                      # negative values among them
    return v, rng.random(shape) < share


@pytest.mark.parametrize('bits', [1, 2, 10, 16])
def test_quantize_row_lengths(bits):
    for n3 in N3S:
        v, sel = ct_volume((5, 7, n3), 100 + n3)
        sel[0, 0, 0] = sel[4, 6, n3 - 1] = True
        table, _, _ = check_quantize(v, sel, bits, (bits, n3))
        assert v[sel].min() < 0 < v[sel].max()
        check_quantize(v, np.ones_like(sel), bits, (bits, n3, 'all'))
        check_quantize(v, sel.view(np.uint8) * np.uint8(7), bits, (bits, n3, 'uint8'))
        two = np.zeros_like(sel)
        two[2, 3, n3 // 2] = two[4, 6, n3 - 1] = True
        table, _, _ = check_quantize(v, two, bits, (bits, n3, 'two'))
        assert len(table) == 2


def test_quantize_exact_halves():
    for bits in (4, 10):
        M = 2 ** bits - 1
        x = np.concatenate([np.arange(M, dtype=np.float32) + np.float32(0.5), [0, M]]).astype(np.float32)
        v = np.zeros((3, 5, (len(x) + 14) // 15), np.float32)
        v.ravel()[:len(x)] = x
        sel = np.zeros(v.shape, bool)
        sel.ravel()[:len(x)] = True
        table, cmap, q = check_quantize(v, sel, bits)
        assert np.array_equal(q.ravel()[:6], [0, 2, 2, 4, 4, 6]) and np.all(q.ravel()[:M] % 2 == 0) and q.ravel()[M + 1] == M


def test_quantize_narrow_range_at_large_magnitude():
    """3000 to 3000.5 at 16 bits: float32 has 2049 values there, far fewer than levels. (Such inputs cannot occupy two levels of one value; the
    merging of equal neighbours is held in tests/test_tissue_host.py on a full presence set.)"""
    rng = np.random.default_rng(11)
    v = (np.float32(3000) + rng.random((9, 10, 130)).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    sel = rng.random(v.shape) < 0.7
    table, _, _ = check_quantize(v, sel, 16)
    assert 1500 < len(table) <= 2049


@pytest.mark.parametrize('bits', [10, 16])
def test_quantize_more_voxels_than_one_launch_sweeps(bits):
    """130^3 voxels are 549,250 quads; a launch sweeps at most 2048 x 256 = 524,288 of them at once. 16 bits read the ranks from global memory."""
    v, sel = ct_volume((130, 130, 130), 7, 0.3)
    table, cmap, q = check_quantize(v, sel, bits)
    assert len(table) > 2 ** bits // 4 and cmap.max() == len(table) - 1


def quantize_case(**kw):
    return TC.Case('bfd_quantize_values3d', **kw)


def test_quantize_nullable_outputs(lib):
    full = quantize_case()
    assert full.run(lib) == 0
    want = TO.quantize(full.values, full.vol, full.bits)
    n = int(full.outputs['numValues'][0])
    assert np.array_equal(full.outputs['table'][:n], want[1]) and np.all(full.outputs['table'][n:] == -7)
    assert np.array_equal(full.outputs['quantized'], want[0]) and np.array_equal(full.outputs['map'], want[2])
    for kw in (dict(want_quantized=False), dict(want_map=False), dict(want_quantized=False, want_map=False)):
        c = quantize_case(**kw)
        assert c.run(lib) == 0, lib.bfd_last_error().decode()
        for name in ('quantized', 'map'):
            assert np.array_equal(c.outputs[name], full.outputs[name] if c.want[name] else c.pristine[name])
        for name in ('table', 'numValues', 'range'):
            assert np.array_equal(c.outputs[name], full.outputs[name])


def test_quantize_data_refusals_leave_the_outputs_untouched(lib):
    base = quantize_case()
    under = base.vol != 0

    def planted(value_at_first=None, fill=None, mask=None):
        v = base.values.copy()
        if fill is not None:
            v[under] = fill
        if value_at_first is not None:
            v[tuple(np.argwhere(under)[3])] = value_at_first
        return dict(values=v, vol=base.vol if mask is None else mask)

    tiny = base.values.copy()
    tiny[under] = 0
    tiny[tuple(np.argwhere(under)[0])] = np.float32(2.0 ** -120)                # A = 2^-120 is normal, r = A / 15 is too; at 16 bits r < 2^-126
    cases = [('mask is empty', planted(mask=np.zeros_like(base.vol)), 4), ('not finite', planted(np.inf), 4), ('not finite', planted(-np.inf), 4),
             ('not finite', planted(np.nan), 4), ('is zero', planted(fill=np.float32(-12.5)), 4), ('below 2^-126', dict(values=tiny, vol=base.vol), 16)]
    for word, kw, bits in cases:
        c = quantize_case(bits=bits, **kw)
        if bits == 16:
            c.outputs['table'] = np.full(65536, -7, np.float32)
            c.pristine = c.snapshot()
        assert c.run(lib) == -1, word
        text = lib.bfd_last_error().decode()
        assert text.startswith('bfd_quantize_values3d: ' + TM.DATA_REFUSED) and word in text, (word, text)
        assert c.untouched(but_ms=True) and c.ms[0] == 0, word
        with pytest.raises(ValueError, match=word.replace('^', '\\^')):
            TM.quantize_values(c.values, c.vol, bits)
    # a non-finite value outside the mask is nobody's business
    v = base.values.copy()
    v[~under] = np.nan
    c = quantize_case(values=v)
    assert c.run(lib) == 0 and np.array_equal(c.outputs['map'], TO.quantize(v, base.vol, base.bits)[2])
    assert np.array_equal(c.outputs['quantized'], TO.quantize(v, base.vol, base.bits)[0], equal_nan=True)


# ---------------------------------------------------------------- cleanup ----------------------------------------------------------------

def mask_volume(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.arange(6, dtype=np.uint8), shape, p=[0.2, 0.2, 0.03, 0.03, 0.5, 0.04])


def check_cleanup(v, kFocal, what='', **kw):
    out = TM.prefocal_cleanup(v, kFocal, **kw)
    bone = kw.get('bone', (2, 3))
    want, wcounts = TO.clear_beyond_bone(v, kFocal, bone[0], bone[1], kw.get('from_value', 4), kw.get('to_value', 1))
    same(out, want, what)
    assert list(TM.last_counts) == list(wcounts), (what, TM.last_counts, wcounts)
    return out, wcounts


@pytest.mark.parametrize('n3', N3S)
def test_cleanup_row_lengths(n3):
    """5 x 7 = 35 lines, no multiple of the four a workgroup takes; every alignment of a line's first voxel occurs where n3 is odd"""
    v = mask_volume((5, 7, n3), n3)
    v[0, 0, :] = np.where(np.isin(v[0, 0, :], (2, 3)), 4, v[0, 0, :])           # a line without bone
    v[1, 1, n3 // 2:] = np.where(np.isin(v[1, 1, n3 // 2:], (2, 3)), 4, v[1, 1, n3 // 2:])       # bone in the lower half only
    v[1, 1, 0] = 2
    v[2, 2, n3 - 1] = 3                                                        # bone at the last voxel: nothing beyond it
    v[3, 3, :] = 4
    v[3, 3, n3 // 3] = 3                                                       # from voxels on both sides of the bone
    for kf in sorted({0, n3 // 2, n3 - 1}):
        out, counts = check_cleanup(v, kf, (n3, kf))
        assert np.array_equal(out[0, 0], v[0, 0]) and np.array_equal(out[2, 2], v[2, 2])
        if kf >= n3 // 2:
            assert np.array_equal(out[1, 1], v[1, 1])                           # bone only at k <= kFocal
        if n3 // 3 > kf:
            assert np.all(out[3, 3, :n3 // 3] == 4) and np.all(out[3, 3, n3 // 3 + 1:] == 1)
    assert counts[0] == 0 and counts[1] == 0                                    # kFocal = n3 - 1: nothing lies beyond
    check_cleanup(v, 0, 'boneB alone', bone=(9, 3))
    check_cleanup(v, 0, 'other values', bone=(5, 0), from_value=1, to_value=200)


@pytest.mark.parametrize('n3', [1020, 1021, 1022, 1024, 2500])
def test_cleanup_around_the_register_resident_length(n3):
    """A wave keeps 1024 bytes of a line: 1021 voxels fit at every alignment, 1022 do not"""
    v = mask_volume((3, 5, n3), n3)
    v[0, 1, 2:] = np.where(np.isin(v[0, 1, 2:], (2, 3)), 4, v[0, 1, 2:])
    v[0, 1, 1] = 2                                                             # changes reach the line's very end
    v[2, 4, :] = 4
    v[2, 4, n3 - 2] = 3
    for kf in (n3 - 3, n3 // 2, 0):
        out, counts = check_cleanup(v, kf, (n3, kf))
    assert counts[1] > n3 // 8 and out[2, 4, n3 - 1] == 1


def test_cleanup_repeats_are_byte_identical():
    v = mask_volume((33, 31, 97), 1)
    first = TM.prefocal_cleanup(v, 40)
    assert first.tobytes() == TM.prefocal_cleanup(v, 40).tobytes() and np.array_equal(first, TO.clear_beyond_bone(v, 40)[0])


@pytest.mark.parametrize('loc', [(16, 15, 40), (0, 30, 0), (32, 0, 95), (5, 5, 96)])
def test_cleanup_equals_the_reference_loop(loc):
    """The device against BabelDatasetPreps.py:1122-1133 in the reference's own shape: two flips, the focal voxel found as the one that holds 5"""
    m = mask_volume((33, 31, 97), 2)
    m[m == 5] = 0
    m[loc] = 5
    want = TO.clear_beyond_bone_loop(m)
    same(TM.prefocal_cleanup(m, loc[2]), want, loc)
    assert TM.last_counts[1] == (want != m).sum() and (TM.last_counts[1] > 0) == (loc[2] < 95)


# ---------------------------------------------------------------- flow ----------------------------------------------------------------

@pytest.fixture(scope='module')
def phantom():
    """tests/test_tissue_host.py::test_phantom_gives_every_step_of_the_flow_work holds the phantom to what the cases below rely on"""
    return TO.head_phantom()


@pytest.mark.parametrize('with_ct,box_fov,proportion', [(True, False, 0.8), (True, True, 0.8), (False, False, 0.8), (False, True, 0.5), (True, False, 1.0)])
def test_finish_mask_equals_the_host_flow(phantom, with_ct, box_fov, proportion):
    m, nfct, loc = phantom
    before = m.copy()
    want, degree, wcounts = TO.finish_mask_host(m, loc, proportion, nfct if with_ct else None, box_fov)
    TM.last_counts = None
    got = TM.finish_mask(m, loc, proportion, nfct if with_ct else None, box_fov)
    same(got, want, (with_ct, box_fov, proportion))
    assert np.array_equal(m, before) and got[loc] == 5
    assert (degree == 0) == (proportion == 1.0) and (got == 3).any()
    if proportion < 1.0:
        assert (got == 2).any()
    if with_ct:
        assert list(TM.last_counts) == list(wcounts) and wcounts[1] > 0             # this call's cleanup, and it changed voxels
    else:
        assert TM.last_counts is None and wcounts is None                            # no cleanup without CT


def test_finish_mask_box_fov_keeps_the_large_island(phantom):
    m, nfct, loc = phantom
    all_painted, kept = TM.finish_mask(m, loc, 0.8, nfct, False), TM.finish_mask(m, loc, 0.8, nfct, True)
    differ = all_painted != kept
    assert differ.sum() > 2000 and np.all(all_painted[differ] == 4) and np.all(kept[differ] == 1)


# ---------------------------------------------------------------- contract ----------------------------------------------------------------

@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


@pytest.mark.parametrize('entry', TC.ENTRIES)
def test_ordinal_out_of_range(lib, entry):
    for device in (-1, lib.bfd_device_count()):
        c = TC.Case(entry)
        assert c.run(lib, device) == -3 and 'ordinal' in lib.bfd_last_error().decode() and c.untouched()


@pytest.mark.parametrize('entry', TC.ENTRIES)
def test_refusals_in_order_leave_everything_untouched(lib, entry):
    words = {n: w for n, w, _ in TC.faults(entry)}
    for names, first in TC.ordered_plants(entry):
        c = TC.planted(entry, names)
        assert c.run(lib) == -1 and words[first] in lib.bfd_last_error().decode() and c.untouched(), names


@pytest.mark.parametrize('entry', TC.ENTRIES)
def test_empty_volume(lib, entry):
    c = TC.Case(entry, N=(0, 4, 9))
    rc = c.run(lib)
    if entry == 'bfd_quantize_values3d':                                        # an empty volume has an empty mask
        assert rc == -1 and 'mask is empty' in lib.bfd_last_error().decode() and c.untouched(but_ms=True) and c.ms[0] == 0
    else:
        assert rc == 0 and c.ms[0] == 0 and not c.outputs['counts'].any() and np.array_equal(c.outputs['out'], c.pristine['out'])


@pytest.mark.parametrize('entry', TC.ENTRIES)
def test_valid_call_twice(lib, entry):
    a, b = TC.Case(entry), TC.Case(entry)
    assert a.run(lib) == 0 and b.run(lib) == 0, lib.bfd_last_error().decode()
    assert a.ms[0] > 0 and b.ms[0] > 0
    for k in a.outputs:
        assert a.outputs[k].tobytes() == b.outputs[k].tobytes(), k
    if entry == 'bfd_paint_components3d':
        want = TO.paint(a.vol, a.value, a.connectivity, a.select, a.fill)
    elif entry == 'bfd_clear_beyond_bone3d':
        want = TO.clear_beyond_bone(a.vol, a.kFocal, a.boneA, a.boneB, a.from_, a.to)
    else:
        q, table, cmap, _ = TO.quantize(a.values, a.vol, a.bits)
        assert np.array_equal(a.outputs['quantized'], q) and np.array_equal(a.outputs['map'], cmap)
        assert np.array_equal(a.outputs['table'][:int(a.outputs['numValues'][0])], table)
        return
    assert np.array_equal(a.outputs['out'], want[0]) and list(a.outputs['counts']) == list(want[1])
