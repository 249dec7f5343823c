"""Timing record of the domain entries (bfd_label_survey3d, bfd_assemble_material_map3d, bfd_sdr_rays3d; babelbrain_amd/Domain.py) on a head-sized
volume, 448 x 448 x 384 at 0.3675 mm: nested spherical shells of skin, cortical and trabecular bone and brain about a centre below the volume, the
focal voxel on the axis, a CT index under the bone (1000 rows) and scattered air. Tight and not tight, with CT and air. Per path:
  - plan_domain as a whole under a host clock, with the kernel time of its two surveys and the time of one survey call;
  - assemble and skull_density_ratio: kernelMs (HIP events, the kernels alone) and the whole call (copies to and from the device included);
  - the bytes the assembly must move, computed from the shapes, and what that is in GB/s of kernelMs;
  - beside them the literal numpy restatement (tests/domain_oracle.py: the 3-D cone from np.meshgrid, np.nonzero over the padded volume, slices,
    in-place relabels, the Python ray loop) on the same machine's CPU, once, and whether the two agree.
Median of --reps after one warm-up. Prints one JSON line last.

    python scripts/domain_timing.py [--reps 3] [--shape 448 448 384] [--no-oracle]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from babelbrain_amd import Domain as DM
from tests import domain_oracle as DO

N_HU = 1000


def phantom(shape, seed=0):
    """(labels uint8, ct uint32, air uint8), as stored (flipped along axis 2)"""
    rng = np.random.default_rng(seed)
    M1, M2, M3 = shape
    ax = [(np.arange(M1, dtype=np.float32) - M1 / 2) ** 2, (np.arange(M2, dtype=np.float32) - M2 / 2) ** 2, (np.arange(M3, dtype=np.float32) - 0.9 * M3) ** 2]
    d2 = ax[0][:, None, None] + ax[1][None, :, None] + ax[2][None, None, :]
    R = 0.75 * M3
    m = np.zeros(shape, np.uint8)
    for radius, label in ((R, 1), (R - 12, 2), (R - 18, 3), (R - 30, 2), (R - 36, 4)):
        m[d2 <= np.float32(radius * radius)] = label
    m[M1 // 2, M2 // 2, int(0.55 * M3)] = 5
    bone = (m == 2) | (m == 3)
    ct = np.zeros(shape, np.uint32)
    ct[bone] = rng.integers(1, N_HU, int(bone.sum()))
    air = ((m == 4) & (rng.random(shape, np.float32) < 0.01)).astype(np.uint8)
    flip = lambda v: np.ascontiguousarray(np.flip(v, 2))
    return flip(m), flip(ct), flip(air)


def timed(fn, reps):
    fn()
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(DM.last_kernel_ms)
    return float(np.median(ms)), float(np.median(wall))


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shape', type=int, nargs=3, default=[448, 448, 384])
    ap.add_argument('--no-oracle', action='store_true')
    a = ap.parse_args()
    devs = DM.InitDomain()
    shape = tuple(a.shape)
    labels, ct, air = phantom(shape)
    h = 1102.515 / 500e3 / 6
    hu = np.sort(np.random.default_rng(1).uniform(-200, 2600, N_HU)).astype(np.float32)
    res = {'device': devs[DM._device][1], 'shape': shape, 'voxels': labels.size, 'reps': a.reps, 'paths': {}}
    print('%r: %d voxels, %d of bone' % (shape, labels.size, int(np.count_nonzero(ct))), flush=True)
    k, w = timed(lambda: DM.survey(labels), a.reps)
    res['survey'] = {'kernel_ms': k, 'call_ms': w, 'bytes': labels.size, 'gb_per_s': labels.size / k / 1e6}
    print('survey of the whole volume: kernel %.3f ms, call %.1f ms, %d MB, %.0f GB/s' % (k, w, labels.size // 10 ** 6, res['survey']['gb_per_s']), flush=True)
    for tight in (True, False):
        kw = dict(FocalLength=63.2e-3, Aperture=64e-3, bTightNarrowBeamDomain=tight, zLengthBeyonFocalPointWhenNarrow=8e-3)
        out = {}
        survey_ms = []
        inner = DM.survey

        def counted(*args, **kwargs):
            r = inner(*args, **kwargs)
            survey_ms.append(DM.last_kernel_ms)
            return r
        DM.survey = counted
        try:
            _, pw = timed(lambda: out.__setitem__('plan', DM.plan_domain(labels, h, **kw)), a.reps)
        finally:
            DM.survey = inner
        plan = out['plan']
        ak, aw = timed(lambda: out.__setitem__('maps', DM.assemble(labels, plan, ct, air, N_HU + 3)), a.reps)
        stats = out['maps'][3]
        sk, sw = timed(lambda: out.__setitem__('sdr', DM.skull_density_ratio(ct, hu, plan, h * 1e3, return_rays=True)), a.reps)
        n_out = int(np.prod(plan.shape))
        crop = int(np.prod(np.array(plan.box_hi) - np.array(plan.box_lo)))
        # three uint32 outputs; inside the crop a label and an air byte per voxel, a CT word under the bone
        nbytes = 12 * n_out + 2 * crop + 4 * stats['bone_voxels']
        row = {'domain': plan.shape, 'crop': [list(plan.box_lo), list(plan.box_hi)], 'region_count': plan.region_count, 'plan_domain_ms': pw,
               'plan_survey_kernel_ms': float(np.sum(survey_ms[-2:])), 'assemble_kernel_ms': ak, 'assemble_call_ms': aw, 'assemble_bytes': nbytes,
               'assemble_gb_per_s': nbytes / ak / 1e6, 'stats': stats, 'sdr_kernel_ms': sk, 'sdr_call_ms': sw, 'sdr': float(out['sdr'][0]),
               'rays': int(out['sdr'][1][0].size), 'rays_counted': int((out['sdr'][1][2] == 1).sum())}
        print('%s: domain %r, plan_domain %.1f ms (its two survey kernels %.3f ms); assemble kernel %.3f ms, call %.1f ms, %d MB, %.0f GB/s; '
              'sdr kernel %.3f ms, call %.1f ms, %d of %d rays, SDR %.6f' % ('tight' if tight else 'not tight', plan.shape, pw, row['plan_survey_kernel_ms'], ak, aw,
                                                                             nbytes // 10 ** 6, row['assemble_gb_per_s'], sk, sw, row['rays_counted'], row['rays'],
                                                                             row['sdr']), flush=True)
        if not a.no_oracle:
            o, t_plan = once(lambda: DO.plan(labels, h, **kw))
            region = o.RegionMap
            o.RegionMap = None
            same_plan = all(getattr(o, f) == getattr(plan, f) for f in DO.PLAN_FIELDS) and np.array_equal(o.ZDim, plan.ZDim)
            A, Z = plan.region_sets()
            same_plan = bool(same_plan and np.array_equal(A[:, :, None] & Z[None, None, :], region))
            del region
            om, t_asm = once(lambda: DO.assemble(labels, o, ct, air, N_HU + 3))
            same_maps = bool(all(np.array_equal(x, y) for x, y in zip(om[:3], out['maps'][:3])) and om[3] == stats)
            del om
            osdr, t_sdr = once(lambda: DO.sdr(ct, hu, o, h * 1e3))
            row.update(oracle_plan_ms=t_plan, oracle_assemble_ms=t_asm, oracle_sdr_ms=t_sdr, plan_equal=same_plan, maps_equal=same_maps,
                       sdr_equal=bool(osdr == out['sdr'][0]))
            print('  the numpy restatement on this host: plan %.0f ms, maps %.0f ms, SDR %.0f ms; plan equal %s, maps equal %s, SDR equal %s'
                  % (t_plan, t_asm, t_sdr, same_plan, same_maps, row['sdr_equal']), flush=True)
        res['paths']['tight' if tight else 'not_tight'] = row
    print(json.dumps(res))


if __name__ == '__main__':
    main()
