"""The domain entries on the device: bfd_label_survey3d, bfd_assemble_material_map3d and bfd_sdr_rays3d equal their numpy restatements
(tests/domain_oracle.py) element for element and number for number, and plan_domain -> assemble -> skull_density_ratio reproduce what the
reference's own UpdateConditions and compute_sdr_from_rays left in tests/golden/domain_golden.npz. Integer work and single float operations: every
comparison is equality."""
import json
import os

import numpy as np
import pytest

from babelbrain_amd import Domain as DM, _engine, harness as H
from tests import domain_calls as DC, domain_oracle as DO

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PLAN_KEYS = list(DO.DEFAULTS) + ['FocalLength', 'Aperture']


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(GOLDEN, 'domain_golden.json')) as fh:
        meta = json.load(fh)
    return np.load(os.path.join(GOLDEN, 'domain_golden.npz')), meta


def runs_of_labels(rng, shape, high=9, zero=0.5):
    """Labels in runs along k, so that words of four equal voxels and mixed words both occur; `zero` of the runs are 0"""
    n = int(np.prod(shape))
    out = np.zeros(n, np.uint8)
    p = 0
    while p < n:
        length = int(rng.integers(1, 12))
        out[p:p + length] = 0 if rng.random() < zero else rng.integers(1, high)
        p += length
    return out.reshape(shape)


def random_box(rng, shape):
    lo = [int(rng.integers(0, s + 1)) for s in shape]
    hi = [int(rng.integers(l, s + 1)) for l, s in zip(lo, shape)]
    return lo, hi


def same_survey(lib, labels, lo, hi, flip):
    hist, bounds, focal, ms = DC.survey(lib, labels, lo, hi, flip)
    want = DO.survey(labels, (lo, hi), flip)
    assert np.array_equal(hist, want[0]) and np.array_equal(bounds, want[1]) and np.array_equal(focal, want[2]), (labels.shape, lo, hi, flip, bounds, want[1],
                                                                                                                     focal, want[2])
    assert ms > 0
    return hist, bounds, focal


# ---------------------------------------------------------------- survey ----------------------------------------------------------------

def test_survey_rows_of_every_length_and_boxes_inside_words(lib):
    """Rows of 1 .. 130 voxels (one wave takes 256 per round, rows begin at every byte of a word), boxes that start and end anywhere, both flips"""
    rng = np.random.default_rng(1)
    for M3 in range(1, 131):
        shape = (int(rng.integers(1, 4)), int(rng.integers(1, 6)), M3)
        labels = runs_of_labels(rng, shape)
        for _ in range(int(rng.integers(0, 3))):
            labels[tuple(int(rng.integers(0, s)) for s in shape)] = 5
        lo, hi = random_box(rng, shape)
        same_survey(lib, labels, lo, hi, M3 % 2)
        same_survey(lib, labels, [0, 0, 0], shape, 1 - M3 % 2)


def test_survey_long_rows_and_single_rows(lib):
    rng = np.random.default_rng(2)
    for shape in ((1, 7, 300), (6, 1, 257), (1, 1, 1030), (2, 3, 777)):
        labels = runs_of_labels(rng, shape, high=256, zero=0.3)
        for flip in (0, 1):
            lo, hi = random_box(rng, shape)
            same_survey(lib, labels, lo, hi, flip)
            hist = same_survey(lib, labels, [0, 0, 0], shape, flip)[0]
        assert hist[200:].sum() > 0 and hist.sum() == labels.size


def test_survey_corner_voxel_no_tissue_and_focal_counts(lib):
    shape = (5, 6, 37)
    for flip in (0, 1):
        for corner in ((0, 0, 0), (4, 5, 36), (4, 0, 36), (0, 5, 0)):
            labels = np.zeros(shape, np.uint8)
            labels[corner] = 3
            _, bounds, focal = same_survey(lib, labels, [0, 0, 0], shape, flip)
            k = shape[2] - 1 - corner[2] if flip else corner[2]
            assert list(bounds) == [corner[0], corner[0], corner[1], corner[1], k, k] and list(focal) == [0, -1]
            _, bounds, _ = same_survey(lib, labels, [1, 1, 1], [4, 5, 36], flip)           # the corner lies outside this box
            assert list(bounds) == [-1] * 6
        labels = np.zeros(shape, np.uint8)
        hist, bounds, focal = same_survey(lib, labels, [0, 0, 0], shape, flip)
        assert hist[0] == labels.size and list(bounds) == [-1] * 6 and list(focal) == [0, -1]
        labels[3, 2, 30] = 5                                                              # one focal voxel, outside the box: still found
        _, bounds, focal = same_survey(lib, labels, [0, 0, 0], [2, 2, 2], flip)
        k = 6 if flip else 30
        assert list(focal) == [1, (3 * 6 + 2) * 37 + k] and list(bounds) == [-1] * 6
        labels[3, 2, 3] = labels[4, 5, 36] = 5                                             # three of them: the first in the driver's raster order
        _, _, focal = same_survey(lib, labels, [0, 0, 0], shape, flip)
        assert list(focal) == [3, (3 * 6 + 2) * 37 + (6 if flip else 3)]
        labels[1, 1, 8:12] = 5                                                            # a word of four of them, and an earlier row
        labels[0, 4, 20] = 5
        _, _, focal = same_survey(lib, labels, [0, 0, 0], shape, flip)
        assert focal[0] == 8 and focal[1] == (0 * 6 + 4) * 37 + (16 if flip else 20)


def test_survey_more_rows_than_one_launch_sweeps(lib):
    """2048 workgroups of four waves take 8192 rows per round"""
    rng = np.random.default_rng(3)
    shape = (101, 97, 9)
    labels = runs_of_labels(rng, shape, high=7)
    labels[100, 96, 8] = 5
    assert shape[0] * shape[1] > 8192
    same_survey(lib, labels, [3, 2, 1], [101, 95, 9], 1)
    same_survey(lib, labels, [0, 0, 0], shape, 0)


# ---------------------------------------------------------------- assembly ----------------------------------------------------------------

def luts():
    rng = np.random.default_rng(4)
    anyl = rng.integers(0, 2 ** 31, 256).astype(np.uint32)
    anyl[rng.random(256) < 0.3] |= np.uint32(DM.LUT_BONE)
    anyl[0] = 0
    return [(True, DM.relabel_lut(True, True)), (True, DM.relabel_lut(True, False)), (False, DM.relabel_lut(False, True)),
            (False, DM.relabel_lut(False, False)), (True, anyl)]


def same_assembly(lib, labels, ct, air, lo, size, padLo, padHi, flip, lut, off, zWater, nMat, focalIJ, **kw):
    got = DC.assemble(lib, labels, ct, air, lo, size, padLo, padHi, flip, lut, off, zWater, nMat, focalIJ, **kw)
    want = DO.assemble_entry(labels, ct, air, lo, size, padLo, padHi, flip, lut, off, zWater, nMat, focalIJ)
    tag = (labels.shape, lo, size, padLo, padHi, flip, zWater)
    assert np.array_equal(got[0], want[0]), tag
    assert got[1] is None or np.array_equal(got[1], want[1]), tag
    assert got[2] is None or np.array_equal(got[2], want[2]), tag
    assert list(got[3]) == list(want[3]), (tag, got[3], want[3])
    assert got[4] > 0
    return got


def test_assembly_rows_of_every_length_every_lut_branch(lib):
    rng = np.random.default_rng(5)
    tables = luts()
    for M3 in list(range(1, 20)) + [63, 64, 65, 127, 128, 129, 130]:
        shape = (int(rng.integers(1, 5)), int(rng.integers(1, 5)), M3)
        labels = runs_of_labels(rng, shape, high=10, zero=0.3)
        with_ct, lut = tables[M3 % len(tables)]
        ct = rng.integers(0, 60000, shape).astype(np.uint16 if M3 % 2 else np.uint32) if with_ct else None
        air = (rng.random(shape) < 0.2).astype(np.uint8) if M3 % 3 else None
        lo, hi = random_box(rng, shape)
        size = [h - l for l, h in zip(lo, hi)]
        padLo, padHi = [int(x) for x in rng.integers(0, 4, 3)], [int(x) for x in rng.integers(0, 4, 3)]
        N = [s + a + b for s, a, b in zip(size, padLo, padHi)]
        if 0 in N:
            padHi = [b + 1 for b in padHi]
            N = [n + 1 for n in N]
        focal = [int(rng.integers(0, N[0])), int(rng.integers(0, N[1]))]
        for zWater in (-1, 0, N[2] - 1, N[2] // 2):
            same_assembly(lib, labels, ct, air, lo, size, padLo, padHi, M3 % 2, lut, 3 + 3 * (M3 % 2), zWater, int(rng.integers(0, 12)), focal,
                          want_noct=bool(M3 % 4), want_air=bool(M3 % 5))


def test_assembly_padding_materials_bone_and_focal_column(lib):
    rng = np.random.default_rng(6)
    shape = (9, 8, 21)
    labels = runs_of_labels(rng, shape, high=6, zero=0.2)
    labels[4, 4, :] = 0                                                      # a column without tissue
    ct = rng.integers(1, 30, shape).astype(np.uint32)
    lut = DM.relabel_lut(True, False)
    for padLo, padHi in (([0, 0, 0], [0, 0, 0]), ([0, 3, 0], [2, 0, 1]), ([5, 0, 2], [0, 4, 0])):
        got = same_assembly(lib, labels, ct, None, [0, 0, 0], shape, padLo, padHi, 1, lut, 3, 1, 33, [4 + padLo[0], 4 + padLo[1]])
        stats = got[3]
        assert stats[6] == -1 and stats[5] >= 2 and stats[0] > 0 and stats[1] >= 4 and stats[2] <= 32 and stats[7] == 0
        assert np.array_equal(got[2], np.zeros_like(got[0]))                 # no air handed: the air output is zero
        top = int(stats[4])
        for nMat, over in ((top + 1, False), (top, True), (1, True)):       # ids equal to and above nMaterials are counted
            s = same_assembly(lib, labels, ct, None, [0, 0, 0], shape, padLo, padHi, 1, lut, 3, 1, nMat, [0, 0])[3]
            assert (s[7] > 0) == over
    nobone = labels.copy()
    nobone[(nobone == 2) | (nobone == 3)] = 1
    stats = same_assembly(lib, nobone, ct, None, [1, 1, 1], [7, 6, 19], [2, 2, 2], [2, 2, 2], 0, lut, 6, -1, 100, [3, 3])[3]
    assert list(stats[:3]) == [0, -1, -1] and stats[3] > 0
    stats = same_assembly(lib, np.zeros(shape, np.uint8), None, None, [0, 0, 0], shape, [1, 1, 1], [1, 1, 1], 1, DM.relabel_lut(False, False), 0, 5, 5,
                          [2, 2])[3]
    assert list(stats) == [0, -1, -1, 0, 0, -1, -1, 0]


def test_assembly_more_voxels_than_one_launch_sweeps(lib):
    rng = np.random.default_rng(7)
    shape = (90, 80, 77)
    labels = runs_of_labels(rng, shape, high=9, zero=0.4)
    ct = rng.integers(1, 500, shape).astype(np.uint16)
    air = (rng.random(shape) < 0.1).astype(np.uint8)
    assert 100 * 91 * 89 > 2048 * 256
    same_assembly(lib, labels, ct, air, [2, 1, 3], [86, 77, 70], [12, 12, 13], [2, 2, 6], 1, DM.relabel_lut(True, True), 6, 14, 400, [50, 40])


# ---------------------------------------------------------------- rays ----------------------------------------------------------------

COUNTS = (0, 1, 2, 3, 4, 6, 10, 63, 64, 65)


def ray_volume(rng, shape, n_hu, dtype, pieces=False):
    """Every ray (i, j) gets one of COUNTS skull voxels (as many as fit), at random places or, with `pieces`, in two blocks with a gap"""
    ct = np.zeros(shape, dtype)
    L = shape[2]
    for i in range(shape[0]):
        for j in range(shape[1]):
            n = min(int(rng.choice(COUNTS)), L)
            if pieces and n >= 2 and L >= n + 3:
                a = int(rng.integers(0, L - n - 2))
                g = int(rng.integers(1, L - n - a))
                where = np.r_[a:a + n // 2, a + n // 2 + g:a + n + g]
            else:
                where = rng.choice(L, n, replace=False)
            ct[i, j, where] = rng.integers(1, n_hu, n)
    return ct


def same_rays(lib, ct, hu, lo, hi, flip, si, sj, mn, cr):
    value, count, state, ms = DC.rays(lib, ct, hu, lo, hi, flip, si, sj, mn, cr)
    want = DO.sdr_rays(ct, hu, (lo, hi), si, sj, mn, cr, flip)
    tag = (ct.shape, lo, hi, flip, si, sj, mn, cr)
    assert np.array_equal(count, want[1]) and np.array_equal(state, want[2]), (tag, state, want[2])
    assert value.dtype == hu.dtype and np.array_equal(value, want[0]), (tag, value, want[0])
    assert (ms > 0) == (value.size > 0)               # a lattice without rays launches nothing
    return value, count, state


def test_rays_of_every_length_count_and_type(lib):
    rng = np.random.default_rng(8)
    seen = set()
    for n, L in enumerate(list(range(1, 12)) + [62, 63, 64, 65, 66, 100, 127, 128, 129, 130]):
        shape = (int(rng.integers(4, 9)), int(rng.integers(4, 12)), L)
        n_hu = 50
        hu = rng.uniform(-300, 2500, n_hu).astype(np.float32 if n % 2 else np.float64)
        ct = ray_volume(rng, shape, n_hu, np.uint16 if n % 3 else np.uint32, pieces=bool(n % 2))
        for flip in (0, 1):
            lo, hi = ([0, 0, 0], list(shape)) if flip == n % 2 else random_box(rng, shape)
            for si, sj, mn, cr in ((1, 1, 3, 0.5), (5, 2, 1, 0.75), (2, 5, 2, 0.25), (1, 3, 3, 1.0)):
                seen |= set(np.unique(same_rays(lib, ct, hu, lo, hi, flip, si, sj, mn, cr)[2]).tolist())
    assert {0, 1, 3} <= seen


def test_rays_gap_decides_the_centre_negative_tables_and_the_table_s_end(lib):
    hu = np.array([-1000.0, 300.0, 900.0, 1500.0, 40.0], np.float32)
    ct = np.zeros((2, 3, 40), np.uint32)
    ct[0, 0, 5:9] = 2
    ct[0, 0, 20:24] = 3                              # eight skull voxels in two pieces: the centre spans the gap, where hu[0] = -1000 decides
    ct[0, 1, 5:13] = 2                               # eight in one piece
    ct[0, 2, 3:6] = 4                                # the table's last row
    ct[1, 0, 7:10] = [1, 5, 1]                       # an index equal to the table's length
    ct[1, 1, 30:34] = 4
    ct[1, 2, 12] = 1                                 # one skull voxel: mid = 0, beg = end = 0 whatever the centre region
    for flip in (0, 1):
        value, count, state = same_rays(lib, ct, hu, [0, 0, 0], [2, 3, 40], flip, 1, 1, 3, 0.5)
        assert value[0, 0] == np.float32(-1000.0) / np.float32(1500.0) and value[0, 1] == 1 and value[0, 2] == 1
        assert state.tolist() == [[1, 1, 1], [4, 1, 0]] and count.tolist() == [[8, 8, 3], [3, 4, 1]]
    for dtype in (np.float32, np.float64):
        negative = -np.abs(hu).astype(dtype)
        _, _, state = same_rays(lib, ct, negative, [0, 0, 0], [2, 3, 40], 1, 1, 1, 3, 0.5)
        assert state.tolist() == [[2, 2, 2], [4, 2, 0]]
    # a ray whose centre slice is empty: one skull voxel gives beg = end = 0; from two on, centre region 0 still keeps the middle voxel
    for cr in (0.0, 0.5):
        _, _, state = same_rays(lib, ct, hu, [0, 0, 0], [2, 3, 40], 0, 1, 1, 1, cr)
        assert state.tolist() == [[1, 1, 1], [4, 1, 3]]


# ---------------------------------------------------------------- the pipeline against the reference's results ----------------------------------------------------------------

def planned(golden, name):
    g, meta = golden
    rec = meta['cases'][name]
    labels = g[name + '_labels']
    return labels, rec, DM.plan_domain(labels, rec['SpatialStep'], **{k: rec[k] for k in PLAN_KEYS})


@pytest.mark.parametrize('name', ['tight_small', 'tight_large', 'loose', 'two_adjusts', 'flat', 'grows', 'segmented', 'ct', 'segmented_ct_air', 'loose_ct_air'])
def test_plan_assemble_sdr_equal_the_golden(golden, name):
    g, _ = golden
    labels, rec, plan = planned(golden, name)
    for f in DO.PLAN_FIELDS[:-1]:
        assert getattr(plan, f) == rec[f], f
    for f in ('XDim', 'YDim', 'ZDim', 'FocalSpotLocation'):
        assert np.array_equal(getattr(plan, f), g[name + '_' + f]), f
    ct = g[name + '_ct'] if rec['ct'] else None
    air = g[name + '_air'] if rec['air'] else None
    m, noct, sub_air, stats = DM.assemble(labels, plan, ct, air, rec['n_materials'] if ct is not None else None)
    assert m.dtype == np.uint32 and np.array_equal(m, g[name + '_MaterialMap'])
    assert (noct is None) == (ct is None) and (sub_air is None) == (air is None)
    zoom = rec['SpatialStep'] * 1e3
    assert stats['first_k'] * zoom / 1e3 - stats['first_k_focal'] * zoom / 1e3 == rec['DomainZReference']
    if ct is not None:
        assert np.array_equal(noct, g[name + '_MaterialMapNoCT'])
        if air is not None:
            assert np.array_equal(sub_air, g[name + '_SubAirRegions'])
        hu = g['UniqueHU']
        sdr = DM.skull_density_ratio(ct, hu, plan, zoom)
        dense, (value, count, state) = DM.skull_density_ratio(ct, hu, plan, (zoom, zoom), 0.8, 2, 0.75, return_rays=True)
        assert type(sdr) is np.float32 and sdr == g[name + '_sdr'][0] and dense == g[name + '_sdr'][1]
        assert (state == 1).sum() > 50 and count.max() >= 5
        again = DM.assemble(labels, plan, ct, air, rec['n_materials'])                     # byte-identical repeats
        assert again[0].tobytes() == m.tobytes() and again[1].tobytes() == noct.tobytes() and again[3] == stats
        assert DM.skull_density_ratio(ct, hu, plan, zoom) == sdr
    assert np.array_equal(DM.assemble(labels, plan, water_only=True)[0], np.zeros(plan.shape, np.uint32))


def test_other_dtypes_and_the_errors_of_the_reference(golden):
    g, _ = golden
    labels, rec, plan = planned(golden, 'ct')
    ct, hu = g['ct_ct'], g['UniqueHU']
    want = DM.assemble(labels, plan, ct, None, rec['n_materials'])
    got = DM.assemble(labels.astype(np.float64), plan, ct.astype(np.int64), None, rec['n_materials'])      # get_fdata hands float64
    assert np.array_equal(got[0], want[0]) and got[3] == want[3]
    with pytest.raises(ValueError, match='max'):
        DM.assemble(labels, plan, ct, None, 20)
    with pytest.raises(ValueError, match='min'):
        DM.assemble(labels, plan, np.where(ct == 5, 0, ct), None, rec['n_materials'], ct_offset=2)
    nobone = np.where((labels == 2) | (labels == 3), 1, labels).astype(np.uint8)
    with pytest.raises(ValueError, match='no bone'):
        DM.assemble(nobone, plan, ct, None, rec['n_materials'])
    with pytest.raises(IndexError):
        DM.skull_density_ratio(ct, hu[:20], plan, 0.3675)
    single = np.zeros_like(ct)
    single[plan.box_lo[0], plan.box_lo[1], labels.shape[2] - 1 - plan.box_lo[2]] = 1       # the first ray of the lattice, one skull voxel
    with pytest.raises(ValueError, match='centre'):
        DM.skull_density_ratio(single, hu, plan, 0.3675, min_skull_voxels=1)
    assert np.isnan(DM.skull_density_ratio(np.zeros_like(ct), hu, plan, 0.3675))
    two = labels.copy()
    two[0, 0, 0] = 5
    with pytest.raises(ValueError, match='exactly one'):
        DM.plan_domain(two, rec['SpatialStep'], **{k: rec[k] for k in PLAN_KEYS})
    with pytest.raises(ValueError, match='no tissue'):
        DM.plan_domain(np.zeros_like(labels), rec['SpatialStep'], **{k: rec[k] for k in PLAN_KEYS})


def test_the_solver_runs_the_assembled_map(golden):
    """A short run of PropagationModel on the assembled map equals the run on the oracle's map"""
    from babelbrain_amd import PropagationModel
    labels, rec, plan = planned(golden, 'tight_small')
    m = DM.assemble(labels, plan)[0]
    want = DO.assemble(labels, DO.plan(labels, rec['SpatialStep'], **{k: rec[k] for k in PLAN_KEYS}))[0]
    a, k, info = H.make_problem('C2', N=plan.shape, steps=120, accumulate_all_steps=True, stable_dt_fn=lambda ml, f, h, c: _engine.stable_dt(ml, f, True, h, c))
    t = H.MATERIALS[info['freq']]
    matlist = np.array([t['Water'], t['Skin'], t['Cortical'], t['Trabecular'], t['Brain']], np.float64)
    k = dict(k, QCorrection=np.ones(5))
    outs = [PropagationModel(device=0).StaggeredFDTD_3D_with_relaxation(mm, matlist, *a[2:], SILENT=True, **k) for mm in (m, want)]
    assert outs[0][2]['Pressure'].max() > 0
    assert outs[0][2]['Pressure'].tobytes() == outs[1][2]['Pressure'].tobytes() and outs[0][0]['Pressure'].tobytes() == outs[1][0]['Pressure'].tobytes()
