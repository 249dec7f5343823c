"""The restatements of Step 1 that the device tests lean on (tests/tissue_oracle.py, bonerim_oracle.py, pseudoct_oracle.py, conformal_oracle.py) against
what the reference's own statements produced (tests/golden/step1_golden.npz + .json, written by tests/golden/make_step1_golden.py): EQUALITY, of
arrays, dtypes and every recorded intermediate, the printed counts among them. Then: every fault switch of the oracles makes a golden case differ,
the stand-ins for skimage's label and regionprops behave as skimage's, and the inputs rebuilt from the seeds are the recorded ones.

Conditions (no tolerance anywhere):
  - conformal: the reference rounds np.dot in float32, whose order of summation is the BLAS's; the restatement rounds element by element. The
    generator refuses a case in which any transformed coordinate lies within 8 * 2^-24 * S of a half-integer (tests/test_conformal_host.py derives
    the bound), so no voxel is excluded here; test_conformal_condition_holds_for_every_case holds that again on this host.
  - quantize_literal and BO.correct follow NumPy's promotion rules (a float32 scalar times a Python number): they are compared under the major
    version of NumPy the fixture records, and skipped with that reason under another."""
import os

import numpy as np
import pytest
from scipy import ndimage

from tests import bonerim_oracle as BO, conformal_oracle as CO, pseudoct_oracle as PO, step1_cases as S1, tissue_oracle as TO

META = S1.golden()[0]
promotion = pytest.mark.skipif(not S1.same_major(META), reason='the types of this restatement follow NumPy %s.x promotion rules, this is NumPy %s'
                               % (META['numpy'].split('.')[0], np.__version__))


def same(got, want, what=''):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()))


def report(rec, label):
    rows = [r for r in rec['reports'] if r[0] == label]
    assert len(rows) == 1, (label, rec['reports'])
    return rows[0][1:]


def all_cases():
    return [(f, n) for f, cases in S1.FAMILIES.items() for n in cases]


# ---------------------------------------------------------------- the fixture ----------------------------------------------------------------

@pytest.mark.parametrize('family,name', all_cases())
def test_inputs_rebuilt_from_the_seeds_are_the_recorded_ones(family, name):
    rec, _ = S1.case(family, name)
    assert rec['inputs'] == S1.input_hashes(S1.inputs(family, name))
    assert rec['case'] == {k: (list(v) if isinstance(v, tuple) else v) for k, v in S1.FAMILIES[family][name].items()}


def test_fixture_is_complete_and_small():
    meta, arrays = S1.golden()
    assert {f: sorted(c) for f, c in meta['families'].items()} == {f: sorted(c) for f, c in S1.FAMILIES.items()}
    assert os.path.getsize(os.path.join(S1.GOLDEN, 'step1_golden.npz')) < os.path.getsize(os.path.join(S1.GOLDEN, 'domain_golden.npz'))
    assert set(k.split('.')[0] for k in arrays) == set(S1.FAMILIES)


# ---------------------------------------------------------------- the stand-ins for skimage ----------------------------------------------------------------

def test_label_and_regionprops_stand_ins():
    """What the reference relies on: labels in raster order with 26 neighbours, regionprops in label order with .label and .area, a stable
    sort, so that sorted(key=area)[-1] is the highest label among equals and sorted(reverse=True)[0] the lowest."""
    v = np.zeros((6, 7, 9), bool)
    v[0, 0, 0] = v[1, 1, 1] = True                                 # a corner pair: one component of two voxels, label 1
    v[0, 5, 0:3] = True                                            # label 2, three voxels
    v[3, 3, 3] = True                                              # label 3, one voxel
    v[5, 6, 7] = v[4, 5, 8] = True                                 # label 4, a corner pair again: it begins in plane 4
    v[5, 0, 0:3] = True                                            # label 5, three voxels
    lab = S1.label(v)
    assert lab.dtype == np.int32 and lab.max() == 5 and lab[0, 0, 0] == lab[1, 1, 1] == 1 and lab[0, 5, 1] == 2 and lab[3, 3, 3] == 3
    assert lab[5, 0, 2] == 5 and lab[5, 6, 7] == lab[4, 5, 8] == 4 and np.array_equal(lab != 0, v)
    regions = S1.regionprops(lab)
    assert [r.label for r in regions] == [1, 2, 3, 4, 5] and [r.area for r in regions] == [2, 3, 1, 2, 3]
    assert [r.label for r in sorted(regions, key=lambda d: d.area)] == [3, 1, 4, 2, 5]
    assert sorted(regions, key=lambda d: d.area)[-1].label == 5                                    # among equals the highest label
    assert sorted(regions, key=lambda d: d.area, reverse=True)[0].label == 2                       # among equals the lowest

    def pixelcount(regionmask):
        return np.sum(regionmask)

    from operator import itemgetter
    props = S1.regionprops(lab, extra_properties=(pixelcount,))
    assert [p['pixelcount'] for p in props] == [2, 3, 1, 2, 3] and props[1].pixelcount == 3 and props[0]['area'] == 2
    assert sorted(props, key=itemgetter('pixelcount'), reverse=True)[0].label == 2
    # a label that does not occur is no region
    lab2 = lab.copy()
    lab2[lab2 == 3] = 0
    assert [r.label for r in S1.regionprops(lab2)] == [1, 2, 4, 5]
    assert S1.regionprops(np.zeros((2, 2, 2), np.int32)) == []
    # the rules the oracles state in their own words are these
    assert TO.choose_labels([2, 3, 1, 2, 3], 2) == ([5], 5)
    assert np.array_equal(PO.label(v), lab)


# ---------------------------------------------------------------- tissue mask ----------------------------------------------------------------

def bone_mask_chain(ct, zooms, select=2):
    """:870-898 with scipy's filters and TO.paint for the choice of the largest component"""
    median = ndimage.median_filter(ct > S1.TYPE_THRESHOLD, 7, mode='constant', cval=0)
    sf2 = np.round((np.ones(3) * 5) / zooms).astype(int)
    closed = ndimage.binary_closing(median, structure=np.ones(sf2, dtype=int))
    painted, counts = TO.paint(closed, 1, 3, select, 0)
    return median, closed, closed & (painted == 0), counts, sf2


@pytest.mark.parametrize('name', list(S1.BONE_MASK))
def test_bone_mask_chain(name):
    rec, gold = S1.case('bone_mask', name)
    ct = S1.inputs('bone_mask', name)['ndataCT']
    median, closed, nfct, counts, sf2 = bone_mask_chain(ct, rec['case']['zooms'])
    assert list(sf2) == rec['structure'] and report(rec, 'Theshold for bone') == [S1.TYPE_THRESHOLD]
    assert np.ones(sf2, dtype=int).dtype.name == rec['structure_dtype'] and median.dtype.name == rec['median_dtype'] and nfct.dtype.name == rec['nfct_dtype']
    for got, key in ((median, 'median'), (closed, 'closed'), (nfct, 'nfct')):
        same(got, S1.unpack(gold[key], ct.shape), key)
    assert counts[0] == rec['regions'] and counts[1] == max(rec['areas']) == rec['counts'][3]
    masked = ct.copy()
    masked[nfct == False] = 0                                                     # noqa: E712
    assert S1.sha1(masked) == rec['ndataCT'] and S1.sha1(ct) == rec['ndataCTForAir']
    # sensitivity: every component but the largest in its place
    assert not np.array_equal(bone_mask_chain(ct, rec['case']['zooms'], select=0)[2], nfct)


def islands_restated(name, select=None):
    rec, gold = S1.case('islands', name)
    inp = S1.inputs('islands', name)
    dilated = ndimage.binary_dilation(inp['BinMaskConformalCSFRot'], iterations=6)
    if select is None:
        select = 1 if rec['case']['bApplyBOXFOV'] else 0
    return rec, gold, inp, dilated, TO.paint(S1.before_merge(inp, dilated), 1, 3, select, 4)


@pytest.mark.parametrize('name', list(S1.ISLANDS))
def test_islands(name):
    rec, gold, inp, dilated, (out, counts) = islands_restated(name)
    same(dilated, S1.unpack(gold['dilated'], dilated.shape), 'dilated CSF')
    assert dilated.dtype.name == rec['dilated_dtype']
    assert rec['FinalMask_dtype'] == 'int8' and gold['FinalMask'].min() >= 0
    same(out, gold['FinalMask'].astype(np.uint8), 'FinalMask')
    assert report(rec, 'number of skin region islands') == [counts[0]] and counts[1] == max(rec['areas']) and counts[2] == rec['painted']
    # sensitivity: the other rule of selection gives another mask (a swapped select)
    swapped = islands_restated(name, select=0 if rec['case']['bApplyBOXFOV'] else 1)[4][0]
    assert (swapped != out).sum() > 1000


def test_air_regions():
    rec, gold = S1.case('air', 'two_pockets')
    ct = S1.inputs('air', 'two_pockets')['ndataCTForAir']
    air = ndimage.median_filter(((ct >= S1.REGION_AIR[0]) & (ct <= S1.REGION_AIR[1])).astype(np.uint8), 3)
    out, counts = TO.paint(air, 1, 3, 2, 0)
    assert rec['dtype'] == 'uint8'
    same(out, S1.unpack(gold['AirRegions'], ct.shape).astype(np.uint8), 'AirRegions')
    assert counts[0] == len(rec['areas']) and counts[1] == max(rec['areas']) and rec['kept'] >= 3 and out.any()
    assert not np.array_equal(TO.paint(air, 1, 3, 0, 0)[0], out)


@pytest.mark.parametrize('name', list(S1.QUANTIZE))
def test_quantize(name):
    rec, gold = S1.case('quantize', name)
    inp = S1.inputs('quantize', name)
    ct, nfct = inp['ndataCT'], inp['nfct']
    quantized, table, cmap, (mn, mx) = TO.quantize(ct, nfct, rec['case']['CT_quantification'])
    same(table, gold['UniqueHU'], 'UniqueHU')
    assert table.dtype.name == rec['UniqueHU_dtype']
    same(cmap[nfct], gold['map_nfct'], 'ndataCTMap under nfct')
    assert cmap.dtype.name == rec['map_dtype'] and not cmap[~nfct].any()
    assert quantized.dtype.name == rec['ndataCT_dtype'] and S1.sha1(quantized) == rec['ndataCT']
    assert report(rec, 'Unique CT/Density values') == [len(table)] == [rec['levels']]
    for got, key in ((mn, 'minData'), (mx, 'maxData')):
        assert got.dtype.name == rec[key]['dtype'] and float(got) == rec[key]['value']
    levels, qx, _, step = TO.quantize_levels(ct[nfct], mn, mx, rec['case']['CT_quantification'])          # the step and the values before the store
    assert step.dtype.name == rec['ResStep']['dtype'] and float(step) == rec['ResStep']['value'] and qx.dtype.name == rec['qx_dtype']
    same(qx, quantized[nfct], 'qx')
    if rec['case']['CT_quantification'] == 1:
        assert len(table) == 2
    else:
        assert 2 ** rec['case']['CT_quantification'] // 8 < len(table) <= 2 ** rec['case']['CT_quantification']


@promotion
@pytest.mark.parametrize('name', list(S1.QUANTIZE))
def test_quantize_literal(name):
    rec, gold = S1.case('quantize', name)
    inp = S1.inputs('quantize', name)
    quantized, table = TO.quantize_literal(inp['ndataCT'], inp['nfct'], rec['case']['CT_quantification'])
    same(table, gold['UniqueHU'], 'UniqueHU')
    assert quantized.dtype.name == rec['ndataCT_dtype'] and S1.sha1(quantized) == rec['ndataCT']


def finish_restated(name, **kw):
    rec, gold = S1.case('finish', name)
    inp = S1.inputs('finish', name)
    c = rec['case']
    out = TO.finish_mask_host(inp['FinalMask'].astype(np.uint8), inp['LocFocalPoint'], c['TrabecularProportion'], inp['nfct'] if c['ct'] else None,
                              c['bApplyBOXFOV'], **kw)
    return rec, gold, inp, out


@pytest.mark.parametrize('name', list(S1.FINISH))
def test_finish_mask(name):
    rec, gold, inp, (mask, degree, counts) = finish_restated(name)
    assert rec['dtype'] == 'uint8'
    same(mask, gold['FinalMask'], 'FinalMask')
    assert report(rec, 'DegreeErosion') == [degree] == [rec['DegreeErosion']]
    if rec['case']['ct']:
        assert counts[1] > 0 and set(rec['values']) == {0, 1, 2, 3, 4, 5} - ({2} if degree == 0 else set())
        before = TO.finish_mask_host(inp['FinalMask'].astype(np.uint8), inp['LocFocalPoint'], rec['case']['TrabecularProportion'], inp['nfct'],
                                     rec['case']['bApplyBOXFOV'], cleanup_k=-1)[0]
        same(TO.clear_beyond_bone(before, int(inp['LocFocalPoint'][2]))[0], gold['FinalMask'], 'clear_beyond_bone')
        same(TO.clear_beyond_bone_loop(before), gold['FinalMask'], 'clear_beyond_bone_loop')
        # the second labelling, as the flow finds it: the median of the mask with bone as skin, the CT's bone put back
        m = inp['FinalMask'].astype(np.uint8)
        m[m == 2] = 1
        m = ndimage.median_filter(m, 7)
        m[inp['nfct']] = 2
        counts = TO.paint(m, 1, 3, 1 if rec['case']['bApplyBOXFOV'] else 0, 4)[1]
        assert report(rec, 'second number of skin region islands') == [counts[0]] == [len(rec['areas'])] and counts[1] == rec['areas'][-1]
    else:
        assert counts is None


def test_finish_mask_cases_differ_and_notice_cleanup_k():
    g = {name: S1.case('finish', name)[1]['FinalMask'] for name in S1.FINISH}
    assert (g['ct'] != g['ct_degree_0']).sum() > 1000 and g['no_ct'].shape != g['no_ct_degree_0'].shape
    rec, _, inp, _ = finish_restated('ct_box_fov')
    every = TO.finish_mask_host(inp['FinalMask'].astype(np.uint8), inp['LocFocalPoint'], 0.8, inp['nfct'], False)[0]
    assert (every != g['ct_box_fov']).sum() > 2000 and max(rec['areas'][:-1]) > 0.1 * rec['areas'][-1]           # bApplyBOXFOV keeps the large island
    loc = S1.inputs('finish', 'ct')['LocFocalPoint']
    for k in (-1, int(loc[0]), int(loc[1]), 0):                    # no cleanup; the cleanup at a wrong index
        assert (finish_restated('ct', cleanup_k=k)[3][0] != g['ct']).sum() >= 30, k


# ---------------------------------------------------------------- bone rim ----------------------------------------------------------------

_rim = {}


def rim_restated(name, fault=None):
    if (name, fault) not in _rim:
        rec, _ = S1.case('bone_rim', name)
        inp = S1.inputs('bone_rim', name)
        _rim[name, fault] = BO.correct(inp['ndataCT'], inp['nfct'], rec['case']['ratio'], floor=S1.TYPE_THRESHOLD, fault=fault)
    return _rim[name, fault]


@promotion
@pytest.mark.parametrize('name', list(S1.BONE_RIM))
def test_bone_rim(name):
    rec, gold = S1.case('bone_rim', name)
    inp = S1.inputs('bone_rim', name)
    shape = inp['ndataCT'].shape
    out, fields, stats = rim_restated(name)
    edge = S1.unpack(gold['edge'], shape)
    same(fields['interior'], S1.unpack(gold['interior'], shape), 'interior')
    same(fields['edge'], edge, 'edge')
    same(fields['d2'][edge].astype(np.uint16), gold['d2_edge'], 'squared distance of the edge voxels')
    same(fields['global_mean'], gold['global_interior_mean'], 'global mean')
    assert S1.sha1(fields['bi']) == rec['blur_interior'] and S1.sha1(fields['bm']) == rec['blur_mask']
    same(out[edge], gold['ndataCT_edge'], 'corrected CT at the edge')
    assert S1.sha1(out) == rec['ndataCT'] and stats == rec['stats'] and fields['lowered'] == rec['lowered']
    assert BO.odd_box(rec['case']['ratio']) == rec['box'] and report(rec, 'nPixelsErode') == list(rec['case']['ratio'])
    assert report(rec, 'Global interior bone mean HU:') == [float(fields['global_mean'])] == [rec['global_interior_mean']['value']]
    assert rec['correct_vals_dtype'] == 'float64' and rec['local_mean_dtype'] == 'float32' and rec['interior_f_dtype'] == 'float32'
    # the weights: exp of this host against the recorded table (the device test's condition)
    scale = rec['distance_scale']
    assert scale == rec['box'][0] / 2.0 and rec['sigma_local'] == rec['box'][0]
    assert np.array_equal(np.unique(fields['d2'][edge]), gold['distinct_d2'])


@promotion
@pytest.mark.parametrize('fault', BO.FAULTS)
def test_every_bone_rim_fault_is_seen(fault):
    seen = [name for name in S1.BONE_RIM if S1.sha1(rim_restated(name, fault)[0]) != S1.case('bone_rim', name)[0]['ndataCT']]
    print(fault, 'seen by', seen)
    assert seen


def test_bone_rim_cases_cover_the_boxes_and_the_global_mean():
    boxes = {name: S1.case('bone_rim', name)[0]['box'] for name in S1.BONE_RIM}
    assert boxes == {'box_3': [3, 3, 3], 'box_5': [5, 5, 5], 'box_mixed': [3, 3, 5]}
    assert S1.case('bone_rim', 'box_3')[0]['stats']['global_mean_voxels'] > 0 and all(S1.case('bone_rim', n)[0]['stats']['clipped'] > 0 for n in boxes)


# ---------------------------------------------------------------- pseudo-CT ----------------------------------------------------------------

def convert_restated(name, **switch):
    rec, gold = S1.case('pseudo_ct', name)
    inp = S1.inputs('pseudo_ct', name)
    if rec['case']['simNIBS_type'] == 'charm':
        skin, csf, cavities = PO.charm_masks(inp['charm'][:, :, :, 0])
    else:
        skin, csf, cavities = inp['skin'], inp['csf'], inp['cavities']
    return rec, gold, inp, (skin, csf, cavities), PO.convert(inp['zte'], inp['head'], skin, cavities, csf, bIsPetra=rec['case']['petra'], **switch)


@pytest.mark.parametrize('name', list(S1.PSEUDO_CT))
def test_pseudo_ct(name):
    rec, gold, inp, masks, (arrCT, parts) = convert_restated(name)
    shape = inp['zte'].shape
    assert inp['zte'].dtype.name == rec['case']['dtype']
    if rec['case']['simNIBS_type'] == 'charm':
        for got, key, dt in zip(masks, ('arrSkin', 'arrMask', 'arrCavities'), rec['charm_dtypes']):
            assert got.dtype.name == dt
            same(got, S1.unpack(gold[key], shape), key)
        assert [int(m.sum()) for m in masks] == rec['charm_counts']
    for key in ('candidates', 'bone_before_closing', 'bone'):
        same(parts[key], S1.unpack(gold[key], shape), key)
    assert parts['normaliser'] == rec['normaliser'] and parts['maximum'] == rec['maximum']
    bone = parts['bone']
    same(arrCT[bone], gold['arrCT_bone'], 'arrCT under the bone')
    same(arrCT == -1000, S1.unpack(gold['air'], shape), 'arrCT == -1000')
    assert arrCT.dtype.name == rec['dtype'] == 'float64' and S1.sha1(arrCT) == rec['arrCT']
    assert rec['candidate_sizes'][0] == rec['candidate_sizes'][1] and rec['chosen_label'] == 1          # the tie, and the reference's choice
    assert rec['counts'] == [int(parts[k].sum()) for k in ('candidates', 'bone_before_closing', 'bone')]
    labels = dict(zte='ZTE conversion with slope and offset', petra='PETRA conversion with slope and offset')
    k = PO.PETRA if rec['case']['petra'] else PO.ZTE
    assert report(rec, labels['petra' if rec['case']['petra'] else 'zte']) == [k['slope'], k['offset']]
    assert report(rec, 'converting ZTE/PETRA to pCT with range') == [0.1, 0.6]


@pytest.mark.parametrize('switch', [dict(erode=False), dict(close=False), dict(cavities=False), dict(first_tie=False), dict(hu_from_gauss=True)])
def test_every_pseudo_ct_switch_is_seen(switch):
    seen = [name for name in ('zte_float64_headreco', 'petra_float32_charm') if S1.sha1(convert_restated(name, **switch)[4][0]) != S1.case('pseudo_ct', name)[0]['arrCT']]
    print(switch, 'seen by', seen)
    assert seen


def test_charm_masks_differ_from_the_headreco_masks():
    """the charm cases give the conversion other masks than the headreco cases of the same volume, so the two readings are two cases"""
    inp = S1.inputs('pseudo_ct', 'zte_float64_charm')
    skin, csf, cavities = PO.charm_masks(inp['charm'][:, :, :, 0])
    assert (skin != (inp['skin'] != 0)).any() and (csf != inp['csf']).any() and np.array_equal(cavities, inp['cavities'] != 0)
    assert S1.case('pseudo_ct', 'zte_float64_charm')[0]['arrCT'] != S1.case('pseudo_ct', 'zte_float64_headreco')[0]['arrCT']


# ---------------------------------------------------------------- conformal ----------------------------------------------------------------

@pytest.mark.parametrize('name', list(S1.CONFORMAL))
def test_conformal_flow(name):
    rec, gold = S1.case('conformal', name)
    inp = S1.inputs('conformal', name)
    c = rec['case']
    affine, focal, skin, skull, csf = CO.conformal_flow(inp['points'][0], inp['points'][1], inp['points'][2], c['step'], inp['RMat'], c['location'])
    same(affine, gold['baseaffineRot'], 'baseaffineRot')
    same(focal, gold['LocFocalPoint'], 'LocFocalPoint')
    assert affine.dtype.name == rec['affine_dtype'] and focal.dtype.name == rec['focal_dtype']
    assert list(skin.shape) == rec['shape'] and [len(p) for p in inp['points']] == rec['points']
    for got, key, dt, n in zip((skin, skull, csf), ('skin', 'skull', 'csf'), rec['dtypes'], rec['counts']):
        assert got.dtype.name == dt and int(got.sum()) == n
        same(got != 0, S1.unpack(gold[key], skin.shape), key)
    assert rec['focal_outside'] == (name == 'focal_outside') and skin[tuple(focal)] == 1


def test_conformal_condition_holds_for_every_case():
    for name, c in S1.CONFORMAL.items():
        assert S1.conformal_condition(S1.inputs('conformal', name), c), name
    assert not S1.conformal_condition(S1.conformal_inputs(S1.CONFORMAL_REFUSED), S1.CONFORMAL_REFUSED)      # the condition can fail: such a case is refused
