"""Timing record of the bone-rim correction as one device call (bfd_bone_rim_correct3d behind babelbrain_amd.BoneRim) on a skull-like shell at
448 x 448 x 384, median of --reps after one warm-up, and, in the same process and order, of the chain it replaces: the four public calls (BinaryErode,
distance_transform_edt with its float64 result, gaussian_filter twice) and the host's numpy lines between and after them (:948-951, :957, :970-1000,
:1010 of BabelBrain/BabelDatasetPreps.py).
  - kernelMs of the new call (HIP events around its three timed sections) and its wall time (allocation, copies, kernels, the weight table);
  - kernelMs and wall time of each of the four calls, and the wall time of the host lines;
  - the bytes the three new passes must move at the least: prepare 13 B per voxel (ct 4 and bone 1 read; f 4 and the dense mask 4 written) and a
    bit per voxel of packed mask; edge: two bits per voxel and 4 B per edge voxel; blend: two bits per voxel, 16 B read and 4 B written per edge voxel.
    Their times one by one come from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python scripts/bonerim_timing.py --reps 3
    --no-chain: rim_prepare, rim_count, rim_edge, rim_blend_pass beside morph_box_pass, edt_rows, edt_lines and the gauss kernels).
The two results are compared (equal bits are expected wherever the device mean equals numpy's or no voxel takes it). Prints one JSON line last.

    python scripts/bonerim_timing.py [--reps 5] [--shape 448 448 384] [--ratio 3 3 3] [--no-chain]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from babelbrain_amd import BinaryClosing as BC, BoneRim as BR, DistanceTransform as DT, GaussianFilter as GF


def shell_head(shape, seed=0):
    """(ct float32, bone bool): a skull-like ellipsoidal shell, radii 0.75-0.85, dense in its middle (0.77-0.83), partial-volume values on both faces"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[((np.arange(n, dtype=np.float32) - (n - 1) / 2) / (n / 2)) for n in shape], indexing='ij', sparse=True)
    rad = np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2)
    bone = (rad < 0.85) & (rad >= 0.75)
    core = (rad < 0.83) & (rad >= 0.77)
    ct = np.where(rad < 0.75, np.float32(40), np.float32(-1000)).astype(np.float32)
    ct[bone] = np.maximum(rng.normal(450, 80, int(bone.sum())), 300).astype(np.float32)
    ct[core] = rng.normal(1500, 300, int(core.sum())).astype(np.float32)
    return ct, bone


def median_of(fn, reps):
    fn()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return r, float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shape', type=int, nargs=3, default=[448, 448, 384])
    ap.add_argument('--ratio', type=int, nargs=3, default=[3, 3, 3])
    ap.add_argument('--no-chain', action='store_true', help='the new call alone (for a kernel trace)')
    a = ap.parse_args()
    shape = tuple(a.shape)
    devs = BR.InitBoneRim()
    for init in (BC.InitBinaryClosing, DT.InitDistanceTransform, GF.InitGaussianFilter):
        init()
    n = int(np.prod(shape))
    ct, bone = shell_head(shape)
    box = BR.odd_box(a.ratio)
    print('device: %s; %d x %d x %d = %d voxels; box %s; reps %d' % ((devs[BR._device][1],) + shape + (n, box, a.reps)), flush=True)
    res = {'device': devs[BR._device][1], 'shape': shape, 'box': box}

    kms = []

    def one_call():
        out = BR.maximize_bone_rim(ct, bone, a.ratio)
        kms.append(BR.last_kernel_ms)
        return out

    new, wall = median_of(one_call, a.reps)
    st = BR.last_stats
    kernel = float(np.median(kms[1:]))
    least = 13 * n + n // 8 + 2 * n // 8 + 4 * st['edge'] + 2 * n // 8 + 20 * st['edge']
    print('one call: kernels %.3f ms, call %.1f ms; %s; mean %r' % (kernel, wall, st, BR.last_global_mean), flush=True)
    print('the three new passes must move %.3f GB at the least (prepare %.3f GB)' % (least / 1e9, (13 * n + n // 8) / 1e9), flush=True)
    res.update(kernel_ms=kernel, call_ms=wall, stats=st, new_pass_min_bytes=least, copies_bytes=9 * n)

    if not a.no_chain:
        parts = {}

        def stage(name, fn, module):
            r, w = median_of(fn, a.reps)
            parts[name] = {'kernel_ms': float(module.last_kernel_ms), 'call_ms': w}
            print('%-40s kernel %8.3f ms, call %8.1f ms' % (name, module.last_kernel_ms, w), flush=True)
            return r

        interior = stage('BinaryErode', lambda: BC.BinaryErode(bone, np.ones(box)), BC)
        dist = stage('distance_transform_edt, float64 out', lambda: DT.distance_transform_edt(interior, invert=True), DT)
        t0 = time.perf_counter()
        dense = ct >= 800.0
        gmean = ct[dense].mean()
        f = ct * dense
        m = dense.astype(np.float32)
        host_a = (time.perf_counter() - t0) * 1e3
        bi = stage('gaussian_filter(ct * dense)', lambda: GF.gaussian_filter(f, sigma=box[0]), GF)
        bm = stage('gaussian_filter(dense)', lambda: GF.gaussian_filter(m, sigma=box[0]), GF)
        t0 = time.perf_counter()
        edge = bone & ~interior
        w = np.exp(-dist[edge] / (float(box[0]) / 2.0))
        with np.errstate(invalid='ignore', divide='ignore'):
            lm = np.where(bm > 1e-6, bi / bm, gmean)[edge]
        o = ct[edge]
        c = o + w * (lm - o)
        delta = np.clip(c - o, a_min=None, a_max=1000.0)
        old = ct.copy()
        old[edge] = o + delta
        host_b = (time.perf_counter() - t0) * 1e3
        four_k = sum(p['kernel_ms'] for p in parts.values())
        four_w = sum(p['call_ms'] for p in parts.values())
        differ = int(np.count_nonzero(old.view(np.uint32) != new.view(np.uint32)))
        print('the four calls: kernels %.3f ms, calls %.1f ms; the host lines %.1f ms (%.1f before the filters, %.1f after); chain %.1f ms'
              % (four_k, four_w, host_a + host_b, host_a, host_b, four_w + host_a + host_b), flush=True)
        print('one call %.1f ms against the four calls alone %.1f ms: %.2f x; against the chain: %.2f x; %d voxels differ (numpy mean %r)'
              % (wall, four_w, four_w / wall, (four_w + host_a + host_b) / wall, differ, gmean), flush=True)
        res.update(chain=parts, chain_kernel_ms=four_k, chain_calls_ms=four_w, chain_host_ms=host_a + host_b, differ=differ)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
