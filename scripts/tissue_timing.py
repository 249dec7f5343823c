"""Timing record of the tissue-mask entries (bfd_paint_components3d, bfd_quantize_values3d, bfd_clear_beyond_bone3d; babelbrain_amd/TissueMask.py) on a
head-sized volume, 448 x 448 x 384: skin, a skull-like shell, brain, scattered skin islands inside it and a patch of brain in the skin above the skull, CT values in the shell. Per entry:
  - kernelMs (HIP events, the kernels alone) and the whole call under a host clock (copies to and from the device included);
  - the bytes the entry's passes move, computed from the shapes, and what that is in GB/s of kernelMs;
  - the host lines the entry replaces, restated in numpy and scipy, on the same machine's CPU;
  - for the cleanup, once, the loop in the reference's own shape (BabelDatasetPreps.py:1122-1133).
bfd_label3d's largest-component call on the same volume stands beside the painting: the difference is what the two new kernels cost.
Median of --reps after one warm-up. Prints one JSON line last.

    python scripts/tissue_timing.py [--reps 3] [--shape 448 448 384] [--no-loop]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from scipy import ndimage

from babelbrain_amd import LabelImage as LI, TissueMask as TM


def phantom(shape, seed=0, islands=400):
    """(FinalMask uint8, nfct bool, ndataCT float32, focal voxel)"""
    rng = np.random.default_rng(seed)
    ax = [((np.arange(n, dtype=np.float32) - (n - 1) / 2) / (n / 2)) ** 2 for n in shape]
    rad2 = ax[0][:, None, None] + ax[1][None, :, None] + ax[2][None, None, :]
    m = np.zeros(shape, np.uint8)
    m[rad2 < 0.95 ** 2] = 1
    m[rad2 < 0.8 ** 2] = 2
    m[rad2 < 0.7 ** 2] = 4
    nfct = m == 2
    for _ in range(islands):
        c = [int(rng.integers(n // 2 - n // 4, n // 2 + n // 4)) for n in shape]
        e = int(rng.integers(2, 7))
        m[c[0]:c[0] + e, c[1]:c[1] + e, c[2]:c[2] + e] = 1
    m[nfct] = 2
    # brain in the skin layer above the skull, over a sixteenth of the lines: what the pre-focal cleanup turns back into skin
    q = [n // 8 for n in shape]
    top = m[shape[0] // 2 - q[0]:shape[0] // 2 + q[0], shape[1] // 2 - q[1]:shape[1] // 2 + q[1], shape[2] // 2:]
    top[top == 1] = 4
    ct = np.zeros(shape, np.float32)
    ct[nfct] = rng.normal(1200, 350, int(nfct.sum())).astype(np.float32)
    return m, nfct, ct, tuple(n // 2 for n in shape)


def timed(fn, reps, kernel=True):
    fn()
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(TM.last_kernel_ms if kernel else 0.0)
    return float(np.median(ms)), float(np.median(wall))


def host_paint(m):
    """:1077-1097 with scipy's label and the bincount for regionprops' areas"""
    lab, n = ndimage.label(m == 1, np.ones((3, 3, 3), int))
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    order = np.argsort(sizes, kind='stable') + 1
    out = m.copy()
    out[np.isin(lab, order[:-1])] = 4
    return out


def host_quantize(ct, nfct, bits):
    """:1019-1027 and the index map by bisection"""
    ct = ct.copy()
    mx, mn = ct[nfct].max(), ct[nfct].min()
    A = mx - mn
    M = 2 ** bits - 1
    ct[nfct] = (A / M) * np.round((M / A) * (ct[nfct] - mn)) + mn
    unique = np.unique(ct[nfct])
    cmap = np.zeros(ct.shape, np.uint32)
    cmap[nfct] = np.searchsorted(unique, ct[nfct])
    return unique, cmap


def host_cleanup(m, kf):
    k = np.arange(m.shape[2])
    kb = np.where(((m == 2) | (m == 3)) & (k > kf), k, -1).max(axis=2)
    out = m.copy()
    out[(kb[:, :, None] >= 0) & (k > kb[:, :, None]) & (m == 4)] = 1
    return out


def host_cleanup_loop(FinalMask):
    """:1122-1133 as the reference has them"""
    FinalMask = np.flip(FinalMask.copy(), axis=2)
    Rloc = np.array(np.where(FinalMask == 5)).flatten()
    for i in range(FinalMask.shape[0]):
        for j in range(FinalMask.shape[1]):
            Line = FinalMask[i, j, :Rloc[2]]
            bone = np.array(np.where((Line == 2) | (Line == 3))).flatten()
            if len(bone) > 0:
                subline = Line[:bone.min()]
                subline[subline == 4] = 1
                FinalMask[i, j, :len(subline)] = subline
    return np.flip(FinalMask, axis=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shape', type=int, nargs=3, default=[448, 448, 384])
    ap.add_argument('--no-loop', action='store_true')
    a = ap.parse_args()
    devs = TM.InitTissueMask()
    LI.InitLabel()
    shape = tuple(a.shape)
    m, nfct, ct, loc = phantom(shape)
    n, bone = m.size, int(nfct.sum())
    res = {'device': devs[TM._device][1], 'shape': shape, 'voxels': n, 'bone_voxels': bone, 'reps': a.reps}
    print('%r: %d voxels, %d of bone' % (shape, n, bone), flush=True)

    def gbs(nbytes, ms):
        return nbytes / ms / 1e6

    # ---- paint
    out = {}

    def paint():
        out['paint'], out['counts'] = TM.paint_components(m, 1, 4, 0)
    k, w = timed(paint, a.reps)
    skin = m == 1
    lk, lw = [], []
    LI.largest_component(skin)
    for _ in range(a.reps):
        t0 = time.perf_counter()
        LI.largest_component(skin)
        lw.append((time.perf_counter() - t0) * 1e3)
        lk.append(LI.last_kernel_ms)
    _, h = timed(lambda: out.__setitem__('host_paint', host_paint(m)), max(1, a.reps - 1), kernel=False)
    res['paint'] = {'kernel_ms': k, 'call_ms': w, 'counts': [int(v) for v in out['counts']], 'label3d_largest_kernel_ms': float(np.median(lk)),
                    'label3d_largest_call_ms': float(np.median(lw)), 'paint_write_bytes': 6 * n, 'host_ms': h,
                    'voxels_differing_from_host': int(np.count_nonzero(out['paint'] != out['host_paint']))}
    print('paint: kernels %.3f ms (bfd_label3d with the largest mask: %.3f ms), call %.1f ms; the write pass moves %d MB; host lines %.0f ms; differing voxels %d'
          % (k, res['paint']['label3d_largest_kernel_ms'], w, 6 * n // 10 ** 6, h, res['paint']['voxels_differing_from_host']), flush=True)

    # ---- quantise
    res['quantize'] = []
    for bits in (10, 15, 16):
        def quant():
            out['q'] = TM.quantize_values(ct, nfct, bits)
        k, w = timed(quant, a.reps)
        # minmax and presence: the mask and the values under it; apply: the same and the map
        nbytes = 2 * (n + 4 * bone) + (n + 4 * bone + 4 * n)
        row = {'bits': bits, 'kernel_ms': k, 'call_ms': w, 'rows': int(len(out['q'][0])), 'bytes': nbytes, 'gb_per_s': gbs(nbytes, k)}
        if bits == 10:
            _, h = timed(lambda: out.__setitem__('host_q', host_quantize(ct, nfct, bits)), max(1, a.reps - 1), kernel=False)
            row['host_ms'] = h
            row['table_equal'] = bool(np.array_equal(out['q'][0], out['host_q'][0]))
            row['voxels_differing_from_host'] = int(np.count_nonzero(out['q'][1] != out['host_q'][1]))
        res['quantize'].append(row)
        print('quantize %d bits: kernels %.3f ms, call %.1f ms, %d rows, %d MB, %.0f GB/s%s' %
              (bits, k, w, row['rows'], nbytes // 10 ** 6, row['gb_per_s'],
               '; host lines %.0f ms, differing voxels %d' % (row['host_ms'], row['voxels_differing_from_host']) if bits == 10 else ''), flush=True)

    # ---- cleanup
    fm = out['paint'].copy()
    fm[loc] = 5

    def clean():
        out['clean'] = TM.prefocal_cleanup(fm, loc[2])
    k, w = timed(clean, a.reps)
    _, h = timed(lambda: out.__setitem__('host_clean', host_cleanup(fm, loc[2])), max(1, a.reps - 1), kernel=False)
    res['cleanup'] = {'kernel_ms': k, 'call_ms': w, 'counts': [int(v) for v in TM.last_counts], 'bytes': 2 * n, 'gb_per_s': gbs(2 * n, k), 'host_vectorised_ms': h,
                      'voxels_differing_from_host': int(np.count_nonzero(out['clean'] != out['host_clean']))}
    print('cleanup: kernel %.3f ms, call %.1f ms, %d MB, %.0f GB/s; %d lines with bone beyond the focal plane, %d voxels changed; vectorised host lines %.0f ms; differing voxels %d' %
          (k, w, 2 * n // 10 ** 6, res['cleanup']['gb_per_s'], res['cleanup']['counts'][0], res['cleanup']['counts'][1], h, res['cleanup']['voxels_differing_from_host']), flush=True)
    if not a.no_loop:
        t0 = time.perf_counter()
        loop = host_cleanup_loop(fm)
        res['cleanup']['host_loop_ms'] = (time.perf_counter() - t0) * 1e3
        res['cleanup']['voxels_differing_from_loop'] = int(np.count_nonzero(out['clean'] != loop))
        print('  the reference loop, once: %.0f ms; differing voxels %d' % (res['cleanup']['host_loop_ms'], res['cleanup']['voxels_differing_from_loop']), flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
