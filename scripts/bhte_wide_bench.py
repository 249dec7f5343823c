"""Rate of the bio-heat solver on 8-bit and on 16-bit material ids (one MI355X): Gvoxel-steps/s of a heating and of a cooling run at 320^3 and
512^3, on a five-row tissue list and on the same volume relabelled into a 1030-row CT-shaped list (the five rows scattered over it, so both runs
compute the same numbers). Kernel time = the HIP-event time the C-ABI call reports (uploads / downloads excluded).

    scripts/bhte_wide_bench.py narrow            five-row list (works on any build)
    scripts/bhte_wide_bench.py wide [S ...]      1030-row list, default pass length and BFD_BHTE_STEPS=S for each S given"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from babelbrain_amd import RayleighAndBHTE as R

mode, forced = sys.argv[1], sys.argv[2:]
ML5 = dict(Density=np.array([1000., 1116., 1896.5, 1738., 1041.]), SoS=np.array([1500., 1537., 2476., 2205., 1562.]), Attenuation=np.array([0., 2.3, 81., 81., 3.45]),
           SpecificHeat=np.array([4178., 3391., 1313., 2274., 3630.]), Conductivity=np.array([0.6, 0.37, 0.32, 0.31, 0.51]), Perfusion=np.array([0., 106., 10., 30., 559.]),
           Absorption=np.array([0., 0.85, 0.16, 0.15, 0.85]), InitTemperature=np.full(5, 37.))
WHERE = np.array([3, 255, 256, 517, 1029])
steps, h = 120, 4e-4
for n in (320, 512):
    N = (n, n, n)
    rng = np.random.default_rng(0)
    mm = np.zeros(N, np.uint8); mm[:, :, n // 8:n // 4] = 1; mm[:, :, n // 4:n // 3] = 2; mm[:, n // 2:, n // 4:n // 3] = 3; mm[:, :, n // 3:] = 4
    P = (2e5 * rng.random(N, dtype=np.float32)).astype(np.float32)
    if mode == 'wide':
        ml = {k: np.linspace(0.9, 1.1, 1030) * v[4] for k, v in ML5.items()}
        for k in ml:
            ml[k][WHERE] = ML5[k]
        ids, runs = WHERE[mm], [None] + forced
    else:
        ml, ids, runs = ML5, mm, [None]
    for S in runs:
        if S is None: os.environ.pop('BFD_BHTE_STEPS', None)
        else: os.environ['BFD_BHTE_STEPS'] = S
        for what, on in (('heating', steps), ('cooling', 0)):
            out = R.BHTE(P, ids, ml, h, steps, on, -1, dt=0.02)
            ms = R.last_kernel_ms
            print('%s ids, %d rows, %d^3, %d steps %s, %s: kernel %.2f ms -> %.0f Gvoxel-steps/s; Tmax %.4f dose sum %.6e'
                  % ('16-bit' if len(ml['Density']) > 256 else '8-bit', len(ml['Density']), n, steps, what, 'default passes' if S is None else 'BFD_BHTE_STEPS=' + S,
                     ms, float(n) ** 3 * steps / ms / 1e6, float(out[0].max()), float(out[1].astype(np.float64).sum())), flush=True)
