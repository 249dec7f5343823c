"""Kernel times of the six pseudo-CT entries and of PseudoCT.convert_pseudo_ct (profiles/README.md, "Pseudo-CT"):

    python scripts/pseudoct_timing.py 256x256x256 448x448x384 oracle:256x256x256

Per shape, for PETRA and ZTE intensities of tests/pseudoct_oracle.py's phantom at that shape and for float32 and float64 input: kernelMs (HIP
events inside the call), the least and the largest of three calls after a warm-up, one JSON line each. bytes_must_move is formed from the shapes:
the two reads of the integer histogram; masks, output and the values under the bone region for the conversion. `oracle:<shape>` times the
statements of tests/pseudoct_oracle.py on the host, the 11^3 closing on a quarter slab times four (marked in the key)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from babelbrain_amd import BinaryClosing as BC, LabelImage as LI, PseudoCT as PC  # noqa: E402
from tests import pseudoct_oracle as PO  # noqa: E402



def note(**kw):
    print(json.dumps(kw), flush=True)


def best(fn, module=PC, n=4):
    ms = []
    for _ in range(n):
        fn()
        ms.append(module.last_kernel_ms)
    return min(ms[1:]), max(ms[1:])


def oracle_times(shape):
    """wall time of the oracle's statements on this host; the closing on a slab of a quarter of the volume, times 4 (marked)"""
    p = PO.phantom(shape, petra=True)
    z = p['zte']
    t = {}
    t0 = time.time(); PO.petra_normaliser(z); t['petra_normaliser'] = time.time() - t0
    t0 = time.time(); PO.zte_cutoff(z, p['csf']); t['zte_cutoff'] = time.time() - t0
    t0 = time.time(); PO.uniform_histogram(z, 15, 200.0); t['uniform_histogram'] = time.time() - t0
    import scipy.ndimage
    t0 = time.time(); er = scipy.ndimage.binary_erosion(p['head'], iterations=3); t['erosion'] = time.time() - t0
    t0 = time.time(); cand, _ = PO.candidates(z, 1800.0, None, er, 0.1, 0.6); t['candidates'] = time.time() - t0
    t0 = time.time()
    lab = PO.label(cand); sizes = np.bincount(lab.ravel())[1:]; before = lab == int(np.argmax(sizes)) + 1
    t['label_largest'] = time.time() - t0
    slab = before[:shape[0] // 4]
    t0 = time.time(); scipy.ndimage.binary_closing(slab, structure=np.ones((11, 11, 11))); t['closing_extrapolated_x4_from_quarter_slab'] = 4 * (time.time() - t0)
    t0 = time.time(); PO.hounsfield(z, 1800.0, None, before, p['skin'], p['cavities'], -2080.0, 2133.0); t['hounsfield'] = time.time() - t0
    t['flow_total_with_extrapolated_closing'] = sum(v for k, v in t.items() if k not in ('zte_cutoff', 'uniform_histogram'))
    note(kind='oracle_wall_s', shape=shape, **{k: round(v, 3) for k, v in t.items()})


def measure(shape):
    n = shape[0] * shape[1] * shape[2]
    for petra in (True, False):
        p64 = PO.phantom(shape, petra=petra)
        for dtype in (np.float32, np.float64):
            z = p64['zte'].astype(dtype)
            item = z.itemsize
            tag = dict(shape=shape, dtype=np.dtype(dtype).name, petra=petra)
            if petra:
                # entry 1 on a volume that is 60 % one value
                v = z.copy()
                rng = np.random.default_rng(1)
                v[rng.random(shape) < 0.6] = 0
                share = float((v == 0).mean())
                lo, hi = best(lambda: PC.integer_histogram(v))
                note(entry='bfd_integer_histogram3d', ms=lo, ms_max=hi, share_one_value=round(share, 3), bytes_must_move=2 * n * item,
                     TBps=2 * n * item / lo / 1e9, **tag)
                lo, hi = best(lambda: PC.integer_histogram(z))
                note(entry='bfd_integer_histogram3d', ms=lo, ms_max=hi, share_one_value='phantom', bytes_must_move=2 * n * item,
                     TBps=2 * n * item / lo / 1e9, **tag)
                norm = PC.petra_normaliser(z)
            else:
                lo, hi = best(lambda: PC.masked_percentile(z, p64['csf']))
                note(entry='bfd_order_statistics3d', ms=lo, ms_max=hi, passes=4 if item == 4 else 8, **tag)
                norm = float(PC.masked_percentile(z, p64['csf']))
                lo, hi = best(lambda: PC.uniform_histogram(z, 15, 200.0))
                note(entry='bfd_uniform_histogram3d', ms=lo, ms_max=hi, bins=15, both_forms=True, **tag)
                lo, hi = best(lambda: PC.uniform_histogram(z, 1024, 200.0))
                note(entry='bfd_uniform_histogram3d', ms=lo, ms_max=hi, bins=1024, both_forms=True, **tag)
            head = None if petra else p64['head']
            hb = p64['head'] != 0
            er = BC.BinaryErode(hb, iterations=3)
            lo, hi = best(lambda: PC.candidates(z, norm, head, er, 0.1, 0.6))
            note(entry='bfd_pseudo_ct_candidates3d', ms=lo, ms_max=hi, **tag)
            cand = PC.candidates(z, norm, head, er, 0.1, 0.6)[0]
            lo, hi = best(lambda: LI.largest_component(cand, connectivity=3, ties='first'), LI)
            note(entry='bfd_select_component3d', ms=lo, ms_max=hi, components=LI.last_component[0], **tag)
            bone = BC.BinaryClose(LI.largest_component(cand, connectivity=3, ties='first'), np.ones((11, 11, 11)))
            for odt in (np.float64, np.float32):
                lo, hi = best(lambda: PC.hounsfield(z, norm, head, bone, p64['skin'], p64['cavities'], -2085.0, 2329.0, odt))
                masks = 3 + (0 if head is None else 1)
                must = n * (masks + np.dtype(odt).itemsize) + int(bone.sum()) * item      # the values matter under the bone region alone
                note(entry='bfd_pseudo_ct_convert3d', ms=lo, ms_max=hi, out=np.dtype(odt).name, bytes_must_move=must, TBps=must / lo / 1e9,
                     bone_share=round(float(bone.mean()), 4), **tag)
            t0 = time.time()
            lo, hi = best(lambda: PC.convert_pseudo_ct(z, p64['head'], p64['skin'], p64['cavities'], p64['csf'], petra=petra), n=3)
            note(entry='convert_pseudo_ct', ms=lo, ms_max=hi, parts={k: round(v, 4) for k, v in PC.last_parts_ms.items()}, wall_s_per_call=(time.time() - t0) / 3, **tag)


if __name__ == '__main__':
    for arg in sys.argv[1:]:
        shape = tuple(int(x) for x in arg.split(':')[-1].split('x'))
        if arg.startswith('oracle:'):
            oracle_times(shape)
        else:
            measure(shape)
