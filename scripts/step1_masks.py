"""Timing record of the device mask clean-up of Step 1 (bfd_binary_morphology3d, bfd_label3d) on a Step-1-sized mask: a synthetic skull shell of
448 x 448 x 384 uint8 voxels at 0.3675 mm. Every case runs in a process of its own under its own time limit, and the first one that fails ends
the script. Each prints last_kernel_ms (HIP events around the kernels) and the wall time of the whole call (allocation, copies, kernels), both as
the median of --reps calls after one warm-up (the single calls on a line of their own before it):
  - closing with an all-ones structure of 5, 14 and 27 (the box path; 14 is round(5 mm / 0.3675 mm)); the bytes the passes move over the kernel
    time, as a share of the 8 TB/s peak; the ratio of the kernel times at 27 and 5, which a non-separable path would put near (27 / 5)^3 = 157
  - labelling with 26 neighbours of the closed mask, and of a 30 % random fill
  - largest_component against LabelImage followed by np.bincount and == on the host
  - CPU, same host: scipy.ndimage.label and np.bincount on the whole volume; scipy.ndimage.binary_closing on a --scipy-edge^3 corner with the
    whole-volume time that rate gives (an extrapolation, not a measurement: the whole volume would take minutes)
Prints one JSON line per case.

    python scripts/step1_masks.py [--reps 5] [--shape 448 448 384] [--scipy-edge 32] [--limit 300]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

CASES = ['close5', 'close14', 'close27', 'label_closed', 'label_random', 'largest', 'cpu']
PEAK_BYTES_PER_S = 8e12


def shell(shape, voxel_mm=0.3675):
    """a skull-like shell, 6 mm thick, with 20 % of its voxels knocked out and specks around it: uint8 0 / 1"""
    rng = np.random.default_rng(0)
    ax = [((np.arange(n, dtype=np.float32) - (n - 1) / 2) / (0.46 * n)) ** 2 for n in shape]
    r = np.sqrt(ax[0][:, None, None] + ax[1][None, :, None] + ax[2][None, None, :])
    thick = 6.0 / (voxel_mm * 0.46 * min(shape))
    a = (r > 0.9 - thick) & (r < 0.9)
    a &= rng.random(shape, dtype=np.float32) > 0.2
    a |= rng.random(shape, dtype=np.float32) < 1e-4
    return a.view(np.uint8)


def timed(fn, module, reps):
    fn()
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(module.last_kernel_ms)
    print(json.dumps({'repetitions': {'kernel_ms': ms, 'call_ms': wall}}), flush=True)
    return float(np.median(ms)), float(np.median(wall))


def box_bytes(shape, passes):
    """what the box path moves: the volume in and out (1 B per voxel each), the packed mask written once and read once around the passes, and
    one packed read and write per pass; rows padded to 64 voxels"""
    packed = shape[0] * shape[1] * ((shape[2] + 63) // 64) * 8
    return 2 * shape[0] * shape[1] * shape[2] + packed * (2 + 2 * passes)


def run_case(name, a):
    from babelbrain_amd import BinaryClosing as BC, LabelImage as LI
    shape = tuple(a.shape)
    out = {'case': name, 'shape': shape, 'reps': a.reps}
    if name != 'cpu':
        out['device'] = BC.InitBinaryClosing()[BC._device][1]
        LI.InitLabel()
    vol = shell(shape)
    out['foreground'] = float(vol.mean())
    if name.startswith('close'):
        s = int(name[5:])
        st = np.ones((s, s, s), int)
        ms, wall = timed(lambda: BC.BinaryClose(vol, st), BC, a.reps)
        nbytes = box_bytes(shape, 6)
        out.update(structure=s, kernel_ms=ms, call_ms=wall, bytes=nbytes, share_of_8TBs=nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S)
    elif name in ('label_closed', 'label_random'):
        img = BC.BinaryClose(vol, np.ones((14, 14, 14), int)) if name == 'label_closed' else np.random.default_rng(1).random(shape, dtype=np.float32) < 0.3
        res = []
        ms, wall = timed(lambda: res.append(LI.LabelImage(img, return_num=True, connectivity=3)[1]), LI, a.reps)
        out.update(components=int(res[-1]), foreground=float(img.mean()), kernel_ms=ms, call_ms=wall)
    elif name == 'largest':
        img = BC.BinaryClose(vol, np.ones((14, 14, 14), int))
        ms, wall = timed(lambda: LI.largest_component(img), LI, a.reps)

        def on_host():
            lab = LI.LabelImage(img)
            return lab == (np.bincount(lab.ravel())[1:].argmax() + 1)
        ms2, wall2 = timed(on_host, LI, a.reps)
        assert np.array_equal(on_host(), LI.largest_component(img))         # no tie in this mask
        out.update(largest_component={'kernel_ms': ms, 'call_ms': wall}, label_then_host_reduction={'kernel_ms': ms2, 'call_ms': wall2})
    else:
        from scipy import ndimage as ndi
        e = a.scipy_edge
        lo = [max(0, n // 8) for n in shape]                                  # a corner that the shell crosses
        sub = np.ascontiguousarray(vol[lo[0]:lo[0] + e, lo[1]:lo[1] + e, lo[2]:lo[2] + e]) != 0
        out['cpu_closing_corner_edge'] = e
        for s in (5, 14, 27):
            t0 = time.perf_counter()
            ndi.binary_closing(sub, np.ones((s, s, s), int))
            dt = time.perf_counter() - t0
            out['cpu_closing_%d' % s] = {'corner_s': dt, 'whole_volume_s_extrapolated': dt / sub.size * vol.size}
        img = vol != 0
        t0 = time.perf_counter()
        lab, n = ndi.label(img, ndi.generate_binary_structure(3, 3))
        t1 = time.perf_counter()
        big = lab == (np.bincount(lab.ravel())[1:].argmax() + 1)
        t2 = time.perf_counter()
        out.update(cpu_label_of_the_shell={'s': t1 - t0, 'components': int(n)}, cpu_bincount_and_select_s=t2 - t1, largest_voxels=int(big.sum()))
        rnd = np.random.default_rng(1).random(shape, dtype=np.float32) < 0.3
        t0 = time.perf_counter()
        n = ndi.label(rnd, ndi.generate_binary_structure(3, 3))[1]
        out['cpu_label_of_30_percent_fill'] = {'s': time.perf_counter() - t0, 'components': int(n)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shape', type=int, nargs=3, default=[448, 448, 384])
    ap.add_argument('--scipy-edge', type=int, default=32)
    ap.add_argument('--limit', type=int, default=300, help='seconds a case may take')
    ap.add_argument('--case', choices=CASES, help='run this one case in this process (what the script starts for each of them)')
    a = ap.parse_args()
    a.shape = tuple(a.shape)
    if a.case:
        run_case(a.case, a)
        return 0
    results = {}
    for name in CASES:
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--case', name, '--reps', str(a.reps),
               '--scipy-edge', str(a.scipy_edge), '--shape'] + [str(n) for n in a.shape]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print('case %s ended with status %d: nothing more is started' % (name, p.returncode))
            return p.returncode if p.returncode > 0 else 1
        results[name] = json.loads(p.stdout.strip().splitlines()[-1])
    ratio = results['close27']['kernel_ms'] / results['close5']['kernel_ms']
    print('box path, kernel time at structure 27 over structure 5: %.2f (a non-separable path: near (27 / 5)^3 = 157)' % ratio)
    return 0


if __name__ == '__main__':
    sys.exit(main())
