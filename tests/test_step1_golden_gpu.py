"""The device flows of Step 1 against what the reference's own statements produced (tests/golden/step1_golden.npz + .json, written by
tests/golden/make_step1_golden.py from the reference's text), not against the restatements: EQUALITY of every array, dtype and recorded count. The
inputs are rebuilt from the recorded seeds (tests/step1_cases.py; tests/test_step1_golden_host.py holds them to their recorded sha1).

Conditions (they are stated, not tuned):
  - conformal: the generator admits only cases in which no transformed coordinate lies within the float32 bound of a half-integer, so the
    reference's np.dot, whatever its BLAS, and the device's element-wise float32 form must give the same index at every point: no voxel is excluded.
  - bone rim: the library forms its weight table on the host with exp as NumPy takes it. The fixture records the weights of each case's distinct
    squared distances; where this host's np.exp reproduces them bit for bit the corrected CT is held by equality (see test_bone_rim).
  - documented deviations stay: the exact integer mean of BoneRim when global_mean is not passed is not a case here."""
import numpy as np
import pytest

from babelbrain_amd import (BinaryClosing as BC, BoneRim as BR, ConformalMask as CM, LabelImage as LI, MappingFilter as MF, MedianFilter as MED,
                            PseudoCT as PCT, TissueMask as TM)
from tests import step1_cases as S1

pytestmark = pytest.mark.gpu


def same(got, want, what=''):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()))


def report(rec, label):
    rows = [r for r in rec['reports'] if r[0] == label]
    assert len(rows) == 1, (label, rec['reports'])
    return rows[0][1:]


# ---------------------------------------------------------------- tissue mask ----------------------------------------------------------------

@pytest.mark.parametrize('name', list(S1.BONE_MASK))
def test_bone_mask_chain(name):
    """:870-898 as Step 1 strings the drop-ins: MedianFilter(mode='constant') -> BinaryClose -> LabelImage.largest_component"""
    rec, gold = S1.case('bone_mask', name)
    ct = S1.inputs('bone_mask', name)['ndataCT']
    fct = MED.MedianFilter(np.ascontiguousarray(ct > S1.TYPE_THRESHOLD).astype(np.uint8), 7, mode='constant')
    same(fct != 0, S1.unpack(gold['median'], ct.shape), 'median')
    sf2 = np.round((np.ones(3) * 5) / rec['case']['zooms']).astype(int)
    assert list(sf2) == rec['structure']
    closed = BC.BinaryClose(fct, structure=np.ones(sf2, dtype=int))
    same(closed, S1.unpack(gold['closed'], ct.shape), 'closed')
    nfct = LI.largest_component(closed != 0)
    same(nfct, S1.unpack(gold['nfct'], ct.shape), 'nfct')
    assert sorted(int(v) for v in LI.component_sizes(closed != 0)) == rec['areas'] and int(nfct.sum()) == rec['counts'][3]


@pytest.mark.parametrize('name', list(S1.ISLANDS))
def test_merge_islands(name):
    rec, gold = S1.case('islands', name)
    inp = S1.inputs('islands', name)
    dilated = BC.BinaryDilate(inp['BinMaskConformalCSFRot'], iterations=6)
    same(dilated, S1.unpack(gold['dilated'], dilated.shape), 'dilated CSF')
    before = S1.before_merge(inp, dilated)
    want = gold['FinalMask'].astype(np.uint8)
    same(TM.merge_islands(before, rec['case']['bApplyBOXFOV']), want, 'FinalMask')
    out, counts = TM.paint_components(before, 1, 4, TM.SELECT_SMALL if rec['case']['bApplyBOXFOV'] else TM.SELECT_ALL_BUT_LARGEST)
    same(out, want, 'FinalMask')
    assert report(rec, 'number of skin region islands') == [counts[0]] and counts[1] == max(rec['areas']) and counts[2] == rec['painted']


def test_drop_largest_air_region():
    rec, gold = S1.case('air', 'two_pockets')
    ct = S1.inputs('air', 'two_pockets')['ndataCTForAir']
    air = MED.MedianFilter(((ct >= S1.REGION_AIR[0]) & (ct <= S1.REGION_AIR[1])).astype(np.uint8), 3)
    out = TM.drop_largest(air)
    same(out, S1.unpack(gold['AirRegions'], ct.shape).astype(np.uint8), 'AirRegions')
    assert out.any() and sorted(int(v) for v in LI.component_sizes(air == 1)) == rec['areas']           # recorded in ascending order


@pytest.mark.parametrize('name', list(S1.QUANTIZE))
def test_quantize_values(name):
    rec, gold = S1.case('quantize', name)
    inp = S1.inputs('quantize', name)
    ct, nfct = inp['ndataCT'], inp['nfct']
    table, cmap, (mn, mx), q = TM.quantize_values(ct, nfct, rec['case']['CT_quantification'], return_quantized=True)
    same(table, gold['UniqueHU'], 'UniqueHU')
    same(cmap[nfct], gold['map_nfct'], 'ndataCTMap under nfct')
    assert not cmap[~nfct].any() and cmap.dtype.name == rec['map_dtype']
    assert q.dtype.name == rec['ndataCT_dtype'] and S1.sha1(q) == rec['ndataCT']
    assert report(rec, 'Unique CT/Density values') == [len(table)]
    assert mn.dtype.name == rec['minData']['dtype'] and float(mn) == rec['minData']['value'] and float(mx) == rec['maxData']['value']
    again = TM.quantize_values(ct, nfct, rec['case']['CT_quantification'])
    assert len(again) == 3
    same(again[0], table)
    same(again[1], cmap)
    same(MF.MapFilter(q, nfct.astype(np.uint8), table), cmap, 'MapFilter of the quantised volume')


@pytest.mark.parametrize('name', list(S1.FINISH))
def test_finish_mask(name):
    rec, gold = S1.case('finish', name)
    inp = S1.inputs('finish', name)
    c = rec['case']
    given = inp['FinalMask'].astype(np.uint8)
    before = given.copy()
    got = TM.finish_mask(given, inp['LocFocalPoint'], c['TrabecularProportion'], inp['nfct'] if c['ct'] else None, c['bApplyBOXFOV'])
    same(got, gold['FinalMask'], 'FinalMask')
    assert np.array_equal(given, before) and got[tuple(inp['LocFocalPoint'])] == 5 and ((got == 2).any()) == (rec['DegreeErosion'] != 0)


# ---------------------------------------------------------------- bone rim ----------------------------------------------------------------

@pytest.mark.parametrize('name', list(S1.BONE_RIM))
def test_bone_rim(name):
    """maximize_bone_rim with floor= and the recorded global mean against :931-1017.

    Masks, edge set, squared distances and the counts bone, interior, dense, edge, global_mean_voxels, max_d2 and clipped are integers: equality,
    in both branches below. The corrected CT: the weight of an edge voxel is exp(-sqrt(d2) / scale) in float64, from the host's exp. Where this
    host's np.exp gives the recorded weights bit for bit, the corrected CT and `changed` are held by equality too. Where it does not, a weight
    differs from the recorded one by at most one float64 ulp, 2^-52 at most since w <= 1; through orig + w * (local - orig), with
    |local - orig| < 2^17 (the entry refuses larger values), the float64 result moves by less than 2^-35, far below half a float32 ulp of a bone
    value (at least 2^-16 at the floor of 300), so the one float32 rounding of the store lands on the same or on the neighbouring float32: the
    edge voxels are then held to one float32 step of the recorded value. `clipped` counts delta > 1000 on the float64 delta, which moves by the
    same 2^-35, so it stays held by equality; `changed` is a count of float32 results and is left to the exact branch. That bound is about the
    rim weight alone: the Gaussian weights behind bi and bm, which give the local mean, also come from the host's exp, so in that branch bi and
    bm are asserted to have the recorded sha1 (scipy's float32 fields); a host on which they differ fails there, it is not given the bound.
    In the exact branch the comparison of bi and bm with scipy's fields is printed for diagnosis only: the device filter is held to scipy within
    one rounding elsewhere (tests/test_distance_gpu.py), and what is asserted here is the equality of the corrected CT itself. The branch taken
    is printed."""
    rec, gold = S1.case('bone_rim', name)
    inp = S1.inputs('bone_rim', name)
    ct, nfct = inp['ndataCT'], inp['nfct']
    host = np.exp(-np.sqrt(gold['distinct_d2'].astype(np.float64)) / rec['distance_scale'])
    exact = np.array_equal(host, gold['weights'])
    print('%s: np.exp of this host %s the %d recorded weights: %s' % (name, 'reproduces' if exact else 'DOES NOT reproduce', host.size,
                                                                      'equality of the corrected CT' if exact else 'one float32 step at the edge voxels'))
    out, f = BR.maximize_bone_rim(ct, nfct, list(rec['case']['ratio']), floor=S1.TYPE_THRESHOLD, global_mean=gold['global_interior_mean'], return_fields=True)
    edge = S1.unpack(gold['edge'], ct.shape)
    same(f['interior'], S1.unpack(gold['interior'], ct.shape), 'interior')
    same(nfct & ~f['interior'], edge, 'edge')
    same(f['d2'][edge].astype(np.uint16), gold['d2_edge'], 'squared distance of the edge voxels')
    same(f['global_mean'], gold['global_interior_mean'], 'global mean')
    assert BR.odd_box(rec['case']['ratio']) == rec['box']
    fields_equal = [S1.sha1(f[k]) == rec[key] for k, key in (('bi', 'blur_interior'), ('bm', 'blur_mask'))]
    print('%s: bi %s, bm %s scipy\'s float32 field (informational where the weights are reproduced)' % (name, *('equals' if e else 'differs from' for e in fields_equal)))
    for key in ('bone', 'interior', 'dense', 'edge', 'global_mean_voxels', 'max_d2', 'clipped'):
        assert BR.last_stats[key] == rec['stats'][key], key
    floored = ct.copy()
    floored[nfct & (floored < S1.TYPE_THRESHOLD)] = S1.TYPE_THRESHOLD
    same(out[~edge], floored[~edge], 'outside the edge: the clamped input')
    assert out.dtype == np.float32
    if exact:
        same(out[edge], gold['ndataCT_edge'], 'corrected CT at the edge')
        assert S1.sha1(out) == rec['ndataCT'] and BR.last_stats == rec['stats']
    else:
        assert all(fields_equal), 'bi or bm differs from the recorded field: the one-step bound covers the rim weight alone'
        want = gold['ndataCT_edge']
        assert np.all(np.abs(out[edge].astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


# ---------------------------------------------------------------- pseudo-CT ----------------------------------------------------------------

@pytest.mark.parametrize('name', list(S1.PSEUDO_CT))
def test_pseudo_ct(name):
    rec, gold = S1.case('pseudo_ct', name)
    inp = S1.inputs('pseudo_ct', name)
    shape = inp['zte'].shape
    if rec['case']['simNIBS_type'] == 'charm':
        skin, csf, cavities = PCT.charm_masks(inp['charm'][:, :, :, 0])
        for got, key in ((skin, 'arrSkin'), (csf, 'arrMask'), (cavities, 'arrCavities')):
            same(got, S1.unpack(gold[key], shape), key)
    else:
        skin, csf, cavities = inp['skin'], inp['csf'], inp['cavities']
    before = inp['zte'].copy()
    arrCT, parts = PCT.convert_pseudo_ct(inp['zte'], inp['head'], skin, cavities, csf, petra=rec['case']['petra'], return_parts=True)
    assert inp['zte'].dtype.name == rec['case']['dtype'] and inp['zte'].tobytes() == before.tobytes()
    for key in ('candidates', 'bone_before_closing', 'bone'):
        same(parts[key], S1.unpack(gold[key], shape), key)
    assert parts['normaliser'] == rec['normaliser'] and parts['maximum'] == rec['maximum']
    same(arrCT[parts['bone']], gold['arrCT_bone'], 'arrCT under the bone')
    same(arrCT == -1000, S1.unpack(gold['air'], shape), 'arrCT == -1000')
    assert arrCT.dtype.name == rec['dtype'] and S1.sha1(arrCT) == rec['arrCT']


# ---------------------------------------------------------------- conformal ----------------------------------------------------------------

@pytest.mark.parametrize('name', list(S1.CONFORMAL))
def test_conformal_masks(name, monkeypatch):
    """conformal_masks over the packed tables the fixture's points came from (its sources are meshes; the tables take their place through _source,
    everything after it is the call's own), then rotated_bounds and scatter_mask under the recorded affine."""
    rec, gold = S1.case('conformal', name)
    inp = S1.inputs('conformal', name)
    c = rec['case']
    shape = tuple(rec['shape'])
    want = [S1.unpack(gold[k], shape) for k in ('skin', 'skull', 'csf')]
    source = CM._source
    monkeypatch.setattr(CM, '_source', lambda n, *a: source(inp['tables'][n], None, None, inp['grids'][n], inp['origins'][n], inp['units'][n]))
    affine, focal, skin, skull, csf = CM.conformal_masks(0, 1, 2, c['step'], inp['RMat'], c['location'])
    monkeypatch.undo()
    same(affine, gold['baseaffineRot'], 'baseaffineRot')
    same(focal, gold['LocFocalPoint'], 'LocFocalPoint')
    for got, w, dt, n in zip((skin, skull, csf), want, rec['dtypes'], rec['counts']):
        assert got.dtype.name == dt and got.shape == shape and int(got.sum()) == n
        same(got != 0, w)
    m = np.linalg.inv(gold['baseaffineRot']).astype(np.float32)
    for n, w in enumerate(want):
        kw = dict(grid=inp['grids'][n], origin=inp['origins'][n], unit=inp['units'][n])
        lo, hi, count = CM.rotated_bounds(inp['tables'][n], m, **kw)
        assert count == rec['points'][n] and lo.min() >= 0 and np.all(hi < shape) and (n > 0 or lo.max() == 0)
        got = CM.scatter_mask(inp['tables'][n], m, shape, **kw)
        if n == 0:
            got[tuple(focal)] = 1                              # the reference stores the focal point with the skin's points
        same(got != 0, w, ('skin', 'skull', 'csf')[n])
        assert list(CM.last_counts) == [rec['points'][n], 0, 0, 0]
