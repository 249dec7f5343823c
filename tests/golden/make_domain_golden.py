#!/usr/bin/env python3
"""Generates tests/golden/domain_golden.npz + domain_golden.json by IMPORTING the reference's caller module and running its own UpdateConditions,
CalculateDomainZReference and compute_sdr_from_rays on a stand-in `self`, in the manner of make_golden.py (whose stubs it uses): a fake PModel that
returns a given dt, an object with get_fdata / header.get_zooms for the mask file. Only inputs, parameters and results are stored; no reference source.

What Step1_InitializeConditions does around the call is restated here in three lines (the flip and astype of :1176-1179, the offset of :1241-1244, the
crop of :1385-1387).

Run:  python tests/golden/make_domain_golden.py
"""
import json
import os
import sys
from types import SimpleNamespace
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import make_golden as MG                 # noqa: E402
from tests import domain_oracle as DO    # noqa: E402

FREQ, PPW, N_HU = 500e3, 6, 40
BASE = dict(PMLThickness=12, FocalLength=63.2e-3, Aperture=64e-3, ZIntoSkin=0.0, TxMechanicalAdjustmentX=0.0, TxMechanicalAdjustmentY=0.0,
            TxMechanicalAdjustmentZ=0.0, ExtraDepthAdjust=0.0, ExtraAdjustX=[0.0], ExtraAdjustY=[0.0], PaddingForRayleigh=0, PaddingForKArray=0,
            ZTxCorrecton=0.0, bTightNarrowBeamDomain=True, zLengthBeyonFocalPointWhenNarrow=8e-3)
# name: (mask shape, segmented, ct dtype or None, air, parameters that differ from BASE)
CASES = {
    'tight_small': ((60, 56, 70), False, None, False, {}),
    'tight_large': ((120, 110, 140), False, None, False, {}),
    'loose': ((60, 56, 70), False, None, False, dict(bTightNarrowBeamDomain=False)),
    'two_adjusts': ((60, 56, 70), False, None, False, dict(ExtraAdjustX=[0.0, 4e-3], ExtraAdjustY=[0.0, -3e-3], TxMechanicalAdjustmentX=1.5e-3,
                                                           TxMechanicalAdjustmentY=-1e-3, TxMechanicalAdjustmentZ=2e-3, ExtraDepthAdjust=1e-3)),
    'flat': ((60, 56, 70), False, None, False, dict(FocalLength=0.0, Aperture=30e-3)),
    'grows': ((40, 36, 70), False, None, False, dict(bTightNarrowBeamDomain=False, PaddingForRayleigh=2, ZTxCorrecton=1e-3)),
    'segmented': ((60, 56, 70), True, None, False, {}),
    'ct': ((60, 56, 70), False, 'uint32', False, dict(ZIntoSkin=1.2e-3)),
    'segmented_ct_air': ((60, 56, 70), True, 'uint16', True, dict(ZIntoSkin=0.8e-3)),
    'loose_ct_air': ((48, 52, 70), False, 'uint32', True, dict(bTightNarrowBeamDomain=False)),
}


def main():
    MG.install_stubs()
    sys.path.insert(0, MG.REF)
    import matplotlib
    matplotlib.use('Agg')
    from TranscranialModeling import BabelIntegrationBASE as B

    out, meta = {}, {'generated_from': 'TranscranialModeling/BabelIntegrationBASE.py: UpdateConditions, CalculateDomainZReference, compute_sdr_from_rays',
                     'frequency': FREQ, 'ppw': PPW, 'cases': {}}
    hu = np.sort(np.random.default_rng(5).uniform(-150.0, 2400.0, N_HU)).astype(np.float32)
    out['UniqueHU'] = hu
    for name, (shape, segmented, ct_dtype, with_air, delta) in CASES.items():
        par = dict(BASE, **delta)
        labels = DO.head(shape, segmented)
        ct = air = None
        if ct_dtype:
            ct, air = DO.ct_for(labels, N_HU, seed=len(name), dtype=np.dtype(ct_dtype))
            if not with_air:
                air = None
        D = np.flip(labels, axis=2)
        rows = 5 if ct is None else N_HU + 6
        mat = np.zeros((rows, 5))
        mat[:, 0], mat[:, 1] = 1000.0, 1500.0
        mat[1:, 2] = 1400.0
        density = airmap = None
        if ct is not None:
            density = np.flip(ct, axis=2).astype(np.uint32)
            orig = density.copy()
            density += 6 if np.any(D > 5) else 3
            if air is not None:
                airmap = np.flip(air, axis=2).astype(np.uint32)
        slf = SimpleNamespace(ReturnArrayMaterial=lambda mat=mat: mat, _Frequency=FREQ, _basePPW=PPW, _QfactorCorrection=True, _SensorSubSampling=0,
                              _NumberCyclesToTrackAtEnd=2, _DensityCTMap=density, _AirRegions=airmap, **{'_' + k: v for k, v in par.items()})
        wavelength = min(np.sort(mat[:, 1:3].flatten())[np.sort(mat[:, 1:3].flatten()) > 0][0], B.GetSmallestSOS(FREQ, bShear=True)) / FREQ
        h = wavelength / PPW
        nii = SimpleNamespace(get_fdata=lambda labels=labels: labels.astype(np.float64), header=SimpleNamespace(get_zooms=lambda h=h: (h * 1e3,) * 3),
                              affine=np.eye(4))
        pmodel = SimpleNamespace(CalculateMatricesForPropagation=lambda *a: (0.9 / FREQ / 30,) + (None,) * 9)
        with mock.patch.object(B, 'PModel', pmodel), mock.patch('builtins.print'):
            B.SimulationConditionsBASE.UpdateConditions(slf, nii, AlphaCFL=1.0, bWaterOnly=False)
            correction = B.SimulationConditionsBASE.CalculateDomainZReference(slf)
        assert slf._SpatialStep == h
        rec = dict(par, shape=list(shape), segmented=segmented, ct=ct_dtype, air=with_air, SpatialStep=h, n_materials=rows)
        for f in DO.PLAN_FIELDS[:-1]:
            rec[f] = int(getattr(slf, '_' + f))
        rec['upper'] = [int(slf._upperXR), int(slf._upperYR), int(slf._upperZR)]
        rec['TemporalStep'], rec['PPP'], rec['TimeSimulation'] = float(slf._TemporalStep), float(slf._PPP), float(slf._TimeSimulation)
        rec['SensorSubSampling'], rec['SensorStart'] = int(slf._SensorSubSampling), int(slf._SensorStart)
        rec['DomainZReference'] = float(correction)
        out[name + '_labels'] = labels
        out[name + '_FocalSpotLocation'] = np.asarray(slf._FocalSpotLocation, np.int64)
        for f in ('XDim', 'YDim', 'ZDim'):
            out[name + '_' + f] = getattr(slf, '_' + f)
        out[name + '_MaterialMap'] = slf._MaterialMap
        if ct is not None:
            out[name + '_ct'] = ct
            out[name + '_MaterialMapNoCT'] = slf._MaterialMapNoCT
            if air is not None:
                out[name + '_air'] = air
                out[name + '_SubAirRegions'] = slf._SubAirRegions
            sub = orig[slf._XShrink_L:slf._upperXR, slf._YShrink_L:slf._upperYR, slf._ZShrink_L:slf._upperZR]
            with mock.patch('builtins.print'):
                sdr = B.compute_sdr_from_rays(hu[sub], sub > 0, spacing_mm=(h * 1e3, h * 1e3))
                sdr_dense = B.compute_sdr_from_rays(hu[sub], sub > 0, spacing_mm=(h * 1e3, h * 1e3), ray_spacing_mm=0.8, min_skull_voxels=2, center_region=0.75)
            out[name + '_sdr'] = np.array([sdr, sdr_dense])
            assert np.isfinite(sdr) and np.isfinite(sdr_dense)
        meta['cases'][name] = rec
        print(name, [rec[f] for f in DO.PLAN_FIELDS[:-1]], list(slf._FocalSpotLocation), rec['DomainZReference'])

    np.savez_compressed(os.path.join(HERE, 'domain_golden.npz'), **out)
    with open(os.path.join(HERE, 'domain_golden.json'), 'w') as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
    print('wrote', len(out), 'arrays,', os.path.getsize(os.path.join(HERE, 'domain_golden.npz')), 'bytes')


if __name__ == '__main__':
    main()
