#!/usr/bin/env python3
"""Generates tests/golden/step1_golden.npz + step1_golden.json by running the reference's own statements of Step 1 on seeded phantoms
(tests/step1_cases.py): seven blocks of BabelBrain/BabelDatasetPreps.py (GetSkullMaskFromSimbNIBSSTL) and the whole of
CTZTEProcessing.ConvertZTE_PETRA_pCT. Neither module can be imported here (SimpleITK, skimage, PySide6, trimesh ...), so the text of each block is
sliced from the file between two marker lines, dedented and executed in a namespace filled here, never stored, as make_thermal_golden.py does. Only
parameters, seeds, recorded prints, library versions and results are stored; no reference source.

Stand-ins: skimage's label and regionprops (tests/step1_cases.py, held by tests/test_step1_golden_host.py), CodeTimer as an empty context manager,
print as a recorder, and for the pseudo-CT a file manager over a dict, a nibabel whose Nifti1Image records its arguments and no-op histogram and
soft-tissue functions. The intermediates of ConvertZTE_PETRA_pCT are read from its frame when it returns.

Run:  python tests/golden/make_step1_golden.py
"""
import contextlib
import gc
import io
import json
import os
import sys
import tempfile
import textwrap
import time
import zipfile
from operator import itemgetter
from types import SimpleNamespace

import numpy as np
import scipy
import scipy.ndimage
from scipy import ndimage, signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import make_golden as MG                                   # noqa: E402
from make_thermal_golden import lines_between              # noqa: E402
from tests import step1_cases as S1                        # noqa: E402

PREPS = os.path.join(MG.REF, 'BabelBrain', 'BabelDatasetPreps.py')
CTZTE = os.path.join(MG.REF, 'BabelBrain', 'CTZTEProcessing.py')
FIXED_DATE = (1980, 1, 1, 0, 0, 0)


def reference_blocks():
    lines = open(PREPS).read().splitlines()
    between = lambda a, b: lines_between(lines, a, b)      # noqa: E731
    blocks = dict(
        bone_mask=between('if not bDisableCTMedianFilter:', 'ndataCT[nfct==False]=0'),
        islands=between('with CodeTimer("CTS:L3:S1: CT/Density binary_dilation"', 'FinalMask[np.isin(label_img,np.array(AllLabels))]=4'),
        quantize=between('maxData=ndataCT[nfct].max()', "print('Unique CT/Density values'"),
        quantize_map=between('ndataCTMap=np.zeros(ndataCT.shape,np.uint32)', 'ndataCTMap[nfct==False]=0'),
        air=between('AirRegions=(ndataCTForAir >= RegionAirCT[0])', 'AirRegions[label_img==regions[-1].label]=0'),
        conformal=between('baseaffineRot=baseaffine.copy()', 'BinMaskConformalCSFRot[AffIJK[:,0],AffIJK[:,1],AffIJK[:,2]]=1'))
    # the bone rim: from the clamp to the gc.collect() that ends the `if bMaximizeBoneRim` block, the last line of that indentation before maxData
    a = next(i for i, l in enumerate(lines) if 'CTBone=ndataCT[nfct]' in l)
    b = next(i for i in range(a, len(lines)) if 'maxData=ndataCT[nfct].max()' in lines[i])
    b = max(i for i in range(a, b) if lines[i].strip() == 'gc.collect()')
    blocks['bone_rim'] = textwrap.dedent('\n'.join(lines[a:b + 1]))
    # the finish: up to the second flip of the cleanup
    a = next(i for i, l in enumerate(lines) if 'with CodeTimer("CTS:L3:S1: final median filter "' in l)
    flips = [i for i in range(a, len(lines)) if 'FinalMask=np.flip(FinalMask,axis=2)' in lines[i]]
    blocks['finish'] = textwrap.dedent('\n'.join(lines[a:flips[1] + 1]))
    lines = open(CTZTE).read().splitlines()
    a = next(i for i, l in enumerate(lines) if l.startswith('def ConvertZTE_PETRA_pCT('))
    b = next((i for i in range(a + 1, len(lines)) if lines[i] and not lines[i][0].isspace() and not lines[i].startswith(')')), len(lines))
    blocks['pseudo_ct'] = '\n'.join(lines[a:b])
    return blocks


@contextlib.contextmanager
def CodeTimer(*a, **k):
    yield


def recorder(reports):
    def report(*a):
        numbers = [float(v) for x in a[1:] if not isinstance(x, str) for v in np.asarray(x, np.float64).ravel()]
        reports.append([str(a[0]) if isinstance(a[0], str) else ''] + numbers)
    return report


def namespace(reports, **more):
    ns = dict(np=np, ndimage=ndimage, scipy=scipy, gc=gc, os=os, time=time, CodeTimer=CodeTimer, print=recorder(reports), label=S1.label,
              regionprops=S1.regionprops, MedianFilter=None, LabelImage=None, MapFilter=None)
    ns.update(more)
    return ns


def scalar(v):
    return dict(value=float(v), dtype=np.asarray(v).dtype.name)


def under(volume, mask):
    """a float volume as the fixture keeps it: the values under a mask, whole in their own type"""
    return np.ascontiguousarray(volume[mask])


# ---------------------------------------------------------------- the families ----------------------------------------------------------------

def run_bone_mask(block, case, inp):
    reports, seen = [], {}

    def closing(fct, structure, GPUBackend):
        seen['median'], seen['structure'] = fct.copy(), structure
        return ndimage.binary_closing(fct, structure=structure)

    ns = namespace(reports, bDisableCTMedianFilter=False, TypeThresold=S1.TYPE_THRESHOLD, ndataCT=inp['ndataCT'].copy(), BinaryClosingFilter=closing,
                   BinaryClosingFilterCOMPUTING_BACKEND=None, mask_nifti2=SimpleNamespace(header=SimpleNamespace(get_zooms=lambda: case['zooms'])))
    exec(block, ns)
    raw = inp['ndataCT'] > S1.TYPE_THRESHOLD
    closed = ns['fct'] != 0
    assert seen['median'].dtype == bool and (seen['median'] != raw).sum() > 100 and (closed != seen['median']).sum() > 20
    assert len(ns['regions']) >= 2 and 0 < ns['nfct'].sum() < closed.sum()
    rec = dict(reports=reports, structure=list(seen['structure'].shape), structure_dtype=seen['structure'].dtype.name, regions=len(ns['regions']),
               areas=[int(r.area) for r in ns['regions']], median_dtype=seen['median'].dtype.name, nfct_dtype=ns['nfct'].dtype.name,
               ndataCT=S1.sha1(ns['ndataCT']), ndataCTForAir=S1.sha1(ns['ndataCTForAir']), counts=[int(raw.sum()), int(seen['median'].sum()),
                                                                                                  int(closed.sum()), int(ns['nfct'].sum())])
    return rec, dict(median=S1.pack(seen['median']), closed=S1.pack(closed), nfct=S1.pack(ns['nfct']))


def run_islands(block, case, inp):
    reports = []
    ns = namespace(reports, FinalMask=inp['FinalMask'].copy(), BinMaskConformalSkullRot=inp['BinMaskConformalSkullRot'].copy(),
                   BinMaskConformalCSFRot=inp['BinMaskConformalCSFRot'].copy(), nfct=inp['nfct'].copy(), bApplyBOXFOV=case['bApplyBOXFOV'])
    exec(block, ns)
    areas = [int(r.area) for r in ns['regions']]
    assert len(areas) >= 4 and areas[-2] > 0.1 * areas[-1] and areas[0] < 0.1 * areas[-1]
    assert len(ns['AllLabels']) == (len(areas) - 1 if not case['bApplyBOXFOV'] else sum(a < 0.1 * areas[-1] for a in areas[:-1]))
    rec = dict(reports=reports, areas=areas, painted=len(ns['AllLabels']), FinalMask_dtype=ns['FinalMask'].dtype.name,
               dilated_dtype=ns['BinMaskConformalCSFRot'].dtype.name)
    return rec, dict(dilated=S1.pack(ns['BinMaskConformalCSFRot']), FinalMask=ns['FinalMask'])


def run_bone_rim(block, case, inp):
    reports = []
    ns = namespace(reports, ndataCT=inp['ndataCT'].copy(), nfct=inp['nfct'].copy(), TypeThresold=S1.TYPE_THRESHOLD, bMaximizeBoneRim=True,
                   RatioCTVoxels=np.array(case['ratio'], int), bSaveCTMaximized=False, T1Conformal_nii=os.path.join('subject', 'T1W.nii.gz'))
    exec(block, ns)
    edge = ns['edge_voxels']
    d2 = np.rint(ns['dist_to_interior'] ** 2).astype(np.int64)
    assert np.array_equal(np.sqrt(d2.astype(np.float64)), ns['dist_to_interior'])
    distinct, first = np.unique(d2[edge], return_index=True)
    weights = ns['weights'][first]
    assert np.array_equal(weights[np.searchsorted(distinct, d2[edge])], ns['weights']) and ns['weights'].dtype == np.float64
    blur_mask = ns['blur_mask']
    rec = dict(reports=reports, box=[int(v) for v in ns['RatioCTVoxels']], distance_scale=ns['distance_scale'],
               sigma_local=int(ns['sigma_local']), global_interior_mean=scalar(ns['global_interior_mean']), correct_vals_dtype=ns['correct_vals'].dtype.name,
               local_mean_dtype=ns['local_interior_mean_img'].dtype.name, interior_f_dtype=ns['interior_f'].dtype.name,
               ndataCT=S1.sha1(ns['ndataCT']), blur_interior=S1.sha1(ns['blur_interior']), blur_mask=S1.sha1(blur_mask),
               stats=dict(bone=int(ns['nfct'].sum()), interior=int(np.count_nonzero(ns['interior_mask'])), dense=int(ns['interior_mask_val'].sum()),
                          edge=int(edge.sum()), global_mean_voxels=int(np.count_nonzero(~(blur_mask[edge] > 1e-6))),
                          clipped=int(np.count_nonzero(ns['delta'] > ns['max_boost'])),
                          changed=int(np.count_nonzero(ns['ndataCT'].view(np.uint32) != clamp(inp, S1.TYPE_THRESHOLD).view(np.uint32))),
                          max_d2=int(d2[edge].max())),
               lowered=int(np.count_nonzero(ns['correct_vals'] < ns['orig_vals'])))
    print(rec['stats'], rec['lowered'])
    # the plate lies beyond the reach of a Gaussian of sigma 3 (truncated at 4 sigma) from every dense voxel, within that of sigma 5
    assert (rec['stats']['global_mean_voxels'] > 0) == (rec['box'][0] == 3) and rec['stats']['clipped'] > 0 and rec['lowered'] > 0
    arrays = dict(interior=S1.pack(ns['interior_mask']), edge=S1.pack(edge), d2_edge=d2[edge].astype(np.uint16), distinct_d2=distinct.astype(np.int64),
                  weights=weights, global_interior_mean=np.asarray(ns['global_interior_mean']), ndataCT_edge=under(ns['ndataCT'], edge))
    assert d2[edge].max() < 65536 and arrays['global_interior_mean'].dtype == np.float32
    return rec, arrays


def clamp(inp, floor):
    ct = inp['ndataCT'].copy()
    ct[inp['nfct'] & (ct < floor)] = floor
    return ct


def run_quantize(blocks, case, inp):
    reports = []
    ns = namespace(reports, ndataCT=inp['ndataCT'].copy(), nfct=inp['nfct'].copy(), CT_quantification=case['CT_quantification'])
    exec(blocks[0], ns)
    quantized = ns['ndataCT'].copy()
    exec(blocks[1], ns)
    nfct, table, cmap = inp['nfct'], ns['UniqueHU'], ns['ndataCTMap']
    assert np.array_equal(table[cmap[nfct]], quantized[nfct]) and not cmap[~nfct].any()
    rec = dict(reports=reports, levels=int(table.size), UniqueHU_dtype=table.dtype.name, map_dtype=cmap.dtype.name, ndataCT_dtype=quantized.dtype.name,
               ndataCT=S1.sha1(quantized), qx_dtype=ns['qx'].dtype.name, minData=scalar(ns['minData']), maxData=scalar(ns['maxData']),
               ResStep=scalar(ns['ResStep']))
    return rec, dict(UniqueHU=table, map_nfct=under(cmap, nfct))


def run_air(block, case, inp):
    reports = []
    ns = namespace(reports, ndataCTForAir=inp['ndataCTForAir'].copy(), RegionAirCT=list(S1.REGION_AIR))
    exec(block, ns)
    air = ns['AirRegions']
    kept = S1.regionprops(S1.label(air == 1))
    assert len(ns['regions']) >= 4 and len(kept) == len(ns['regions']) - 1 >= 3 and air[12, 20, 25] == 0 and air[17, 16, 32] == 1 and air[0, 0, 0] == 0
    rec = dict(reports=reports, areas=[int(r.area) for r in ns['regions']], kept=len(kept), dtype=air.dtype.name)
    return rec, dict(AirRegions=S1.pack(air))


def run_finish(block, case, inp):
    reports = []
    ns = namespace(reports, FinalMask=inp['FinalMask'].copy(), LocFocalPoint=inp['LocFocalPoint'].copy(), CT_or_ZTE_input='ct.nii.gz' if case['ct'] else None,
                   bApplyBOXFOV=case['bApplyBOXFOV'], TrabecularProportion=case['TrabecularProportion'])
    if case['ct']:
        ns['nfct'] = inp['nfct'].copy()
    exec(block, ns)
    out = np.ascontiguousarray(ns['FinalMask'])
    assert (ns['DegreeErosion'] == 0) == (case['TrabecularProportion'] == 1.0) and out[tuple(inp['LocFocalPoint'])] == 5
    rec = dict(reports=reports, DegreeErosion=int(ns['DegreeErosion']), dtype=out.dtype.name, values=[int(v) for v in np.unique(out)])
    if case['ct']:
        rec['areas'] = [int(r.area) for r in ns['regions']]
    return rec, dict(FinalMask=out)


def run_conformal(block, case, inp):
    assert S1.conformal_condition(inp, case), 'a transformed coordinate lies within the float32 bound of a half-integer: choose another rotation'
    ns = namespace([], baseaffine=np.eye(4), RMat=inp['RMat'].copy(), SpatialStep=case['step'], skin_grid=inp['points'][0].copy(),
                   skull_grid=inp['points'][1].copy(), csf_grid=inp['points'][2].copy(), Location=list(case['location']))
    exec(block, ns)
    masks = [ns['BinMaskConformalSkinRot'], ns['BinMaskConformalSkullRot'], ns['BinMaskConformalCSFRot']]
    focal = ns['LocFocalPoint']
    assert masks[0].sum() > masks[1].sum() > masks[2].sum() > 200 and focal.min() >= 0
    points_only = masks[0].copy()
    points_only[tuple(focal)] = masks[1][tuple(focal)]                                   # the skull's points lie inside the skin's
    outside = bool(np.any(focal > np.array(np.nonzero(points_only)).max(axis=1)))
    assert outside == (case is S1.CONFORMAL['focal_outside'])
    rec = dict(shape=list(masks[0].shape), dtypes=[m.dtype.name for m in masks], counts=[int(m.sum()) for m in masks], points=[len(p) for p in inp['points']],
               focal_dtype=focal.dtype.name, affine_dtype=ns['baseaffineRot'].dtype.name,
               focal_outside=outside)
    arrays = dict(baseaffineRot=ns['baseaffineRot'], LocFocalPoint=np.asarray(focal), skin=S1.pack(masks[0]), skull=S1.pack(masks[1]), csf=S1.pack(masks[2]))
    return rec, arrays


class Volume:
    """what file_manager.load_file hands out: get_fdata gives a fresh float64 array, as nibabel's does"""

    def __init__(self, data):
        self.data, self.affine = data, np.eye(4)

    def get_fdata(self):
        return np.array(self.data, np.float64)


def run_pseudo_ct(block, case, inp):
    reports, files, images, frames = [], {}, [], {}
    root = 'm2m_subject'
    files['T1.nii.gz'], files['ZTE.nii.gz'] = Volume(inp['head']), Volume(inp['zte'])
    if case['simNIBS_type'] == 'charm':
        files[os.path.join(root, 'final_tissues.nii.gz')] = Volume(inp['charm'])
    else:
        for name, key in (('csf.nii.gz', 'csf'), ('skin.nii.gz', 'skin'), ('cavities.nii.gz', 'cavities')):
            files[os.path.join(root, name)] = Volume(inp[key])

    def image(data, affine=None, header=None):
        images.append(data)
        return SimpleNamespace(data=data, affine=affine)

    fm = SimpleNamespace(pseudo_CT_range=(0.1, 0.6), simNIBS_dir=root, simNIBS_type=case['simNIBS_type'], load_file=lambda name: files[name],
                         save_file=lambda file_data=None, filename=None, **k: files.__setitem__(filename, file_data), sitk_to_nibabel=lambda x: x,
                         output_files=dict(pCTfname='pCT.nii.gz', ZTEInT1W='ZTEInT1W.nii.gz'))
    ns = namespace(reports, tempfile=tempfile, signal=signal, itemgetter=itemgetter, nibabel=SimpleNamespace(Nifti1Image=image),
                   GeneratePseudoCTHistogram=lambda *a, **k: None, soft_tissue_from_label=lambda x: None)
    exec(block, ns)
    code = ns['ConvertZTE_PETRA_pCT'].__code__

    def profile(frame, event, arg):
        if event == 'return' and frame.f_code is code:
            frames.update(frame.f_locals)

    sys.setprofile(profile)
    try:
        pCT = ns['ConvertZTE_PETRA_pCT']('T1.nii.gz', 'ZTE.nii.gz', Volume(inp['head']), fm, bIsPetra=case['petra'])
    finally:
        sys.setprofile(None)
    arrCT = pCT.data
    assert arrCT is images[-1] and arrCT is frames['arrCT']
    label_img, props = frames['label_img'], frames['props']
    sizes = sorted((int(p.area) for p in props), reverse=True)
    assert sizes[0] == sizes[1], 'the two halves of the skull are the largest candidates and equal: the tie rule decides'
    before = label_img == props[0].label
    bone = frames['arr2'] != 0
    normaliser = float(np.max(frames['locs'])) if case['petra'] else float(frames['cutoff'])
    rec = dict(reports=reports, dtype=arrCT.dtype.name, arrCT=S1.sha1(arrCT), normaliser=normaliser, maximum=float(np.max(frames['arrGauss'])),
               candidate_sizes=sizes[:6], chosen_label=int(props[0].label),
               counts=[int(frames['arr'].sum()), int(before.sum()), int(bone.sum())])
    arrays = dict(candidates=S1.pack(frames['arr']), bone_before_closing=S1.pack(before), bone=S1.pack(bone), arrCT_bone=under(arrCT, bone),
                  air=S1.pack(arrCT == -1000))
    if case['simNIBS_type'] == 'charm':
        arrays.update(arrSkin=S1.pack(frames['arrSkin']), arrMask=S1.pack(frames['arrMask']), arrCavities=S1.pack(frames['arrCavities']))
        rec['charm_dtypes'] = [frames[k].dtype.name for k in ('arrSkin', 'arrMask', 'arrCavities')]
        rec['charm_counts'] = [int(frames[k].sum()) for k in ('arrSkin', 'arrMask', 'arrCavities')]
        assert rec['charm_counts'][2] > 0
    return rec, arrays


def save_npz(path, arrays):
    """np.savez_compressed with sorted names and a fixed date in every member, so that a second run writes the same bytes"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name], order='C'), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', FIXED_DATE)
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    blocks = reference_blocks()
    runs = dict(pseudo_ct=run_pseudo_ct, bone_mask=run_bone_mask, islands=run_islands, bone_rim=run_bone_rim, air=run_air, finish=run_finish,
                conformal=run_conformal, quantize=run_quantize)
    out, meta = {}, {'generated_from': 'BabelBrain/BabelDatasetPreps.py :696-759, :870-898, :900-929, :931-1017, :1019-1028, :1034-1037, :1049-1061, '
                                       ':1066-1133; BabelBrain/CTZTEProcessing.py ConvertZTE_PETRA_pCT',
                     'numpy': np.__version__, 'scipy': scipy.__version__, 'TypeThresold': S1.TYPE_THRESHOLD, 'RegionAirCT': list(S1.REGION_AIR),
                     'families': {}}
    for family, cases in S1.FAMILIES.items():
        meta['families'][family] = {}
        for name, case in cases.items():
            inp = S1.inputs(family, name)
            block = (blocks['quantize'], blocks['quantize_map']) if family == 'quantize' else blocks[family]
            rec, arrays = runs[family](block, case, inp)
            rec['case'] = {k: (list(v) if isinstance(v, tuple) else v) for k, v in case.items()}
            rec['inputs'] = S1.input_hashes(inp)
            meta['families'][family][name] = rec
            size = 0
            for k, v in arrays.items():
                out['%s.%s.%s' % (family, name, k)] = v
                size += v.nbytes
            print(family, name, size, 'bytes raw', [r for r in rec.get('reports', []) if len(r) < 6][:6])
    path = os.path.join(HERE, 'step1_golden.npz')
    save_npz(path, out)
    with open(os.path.join(HERE, 'step1_golden.json'), 'w') as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', len(out), 'arrays,', os.path.getsize(path), 'bytes;', os.path.getsize(os.path.join(HERE, 'step1_golden.json')), 'bytes of json')


if __name__ == '__main__':
    main()
