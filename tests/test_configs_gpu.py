"""Every BASELINE.json configuration on the MI355X at its stated size.

  C1 128^3 water, SingleTx 500 kHz, 500 steps        -> against the oracle, full size
  C2 256^3 skull+brain (3 materials), 2000 steps     -> against the oracle, full size
  C3 512^3 CT-like skull, CTX-500, 140 steps         -> against the oracle, full size (+ tests/test_fullsize_gpu.py)
  C4 512x512x1024, H317 phased array, 700 kHz        -> against the oracle at 128x128x256 (600 steps) and at FULL size
                                                        for 80 steps; size-independent properties at full size
  C5 1024^3, 1 MHz                                   -> against the oracle at 192^3 (600 steps); properties at full size

The oracle cannot finish C4 / C5 in seconds, so those are held through properties that the small-grid parity tests tie
to the oracle: the independent device implementations (dense LDS-tiled variant 2, class-specialised variant 3) agree
exactly on the same inputs, and a Z-slab decomposed run (8 slabs on this one GPU, halo planes exchanged by device
copies of the tensors the RCCL path sends) equals the single-domain run bit for bit. The step counts are chosen so that
the wave has crossed the first slab interface (k = N3/8) when the RMS window opens."""
import numpy as np
import pytest

from babelbrain_amd import harness as H
from babelbrain_amd import slab
from babelbrain_amd._engine import HALO_STRESS, HALO_VELOCITY
from tests.util import compare_runs, geometry_of, oracle_dt

pytestmark = pytest.mark.gpu


def _hip_dt(ml, f, h, c):
    from babelbrain_amd import _engine
    return _engine.stable_dt(ml, f, True, h, c)


def test_c1_full_size_against_oracle():
    """BASELINE configs[0]: 128^3 water-only domain, SingleTx 500 kHz, 500 time steps, every output compared."""
    from babelbrain_amd import PropagationModel
    from oracle import oracle as O
    a, k, info = H.make_problem('C1', steps=500, stable_dt_fn=oracle_dt)
    assert a[0].shape == (128, 128, 128) and info['nt'] == 500
    out_h = PropagationModel().StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, **k)
    out_o = O.StaggeredFDTD_3D_with_relaxation(*a, **k)
    worst = compare_runs(out_h, out_o, geometry=geometry_of(a, k))
    assert out_o[2]['Pressure'].max() > 0 and out_h[0]['Pressure'].shape[0] == 104 * 104 * 103
    print('C1 128^3 x 500 steps: worst rel L2 vs oracle %.3e' % worst)


@pytest.mark.timeout(900)
def test_c2_full_size_against_oracle():
    """BASELINE configs[1]: 256^3 synthetic skull + brain (water / cortical bone with shear / brain), SingleTx 500 kHz,
    2000 time steps: RMS map, last map and the full sensor block against the oracle."""
    from babelbrain_amd import PropagationModel
    from oracle import oracle as O
    a, k, info = H.make_problem('C2', steps=2000, stable_dt_fn=oracle_dt)
    assert a[0].shape == (256, 256, 256) and info['nt'] == 2000 and len(a[1]) == 3 and a[1][1][2] > 0
    out_h = PropagationModel().StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, **k)
    out_o = O.StaggeredFDTD_3D_with_relaxation(*a, **k)
    worst = compare_runs(out_h, out_o, geometry=geometry_of(a, k))
    rms = out_o[2]['Pressure']
    inside = rms[128, 128, 150]              # behind the skull: the wave went through bone
    assert rms.max() > 0 and inside > 0
    print('C2 256^3 x 2000 steps: worst rel L2 vs oracle %.3e (oracle step loop %.1f s)' % (worst, out_o[-1]['stepLoopSeconds']))


@pytest.mark.timeout(600)
def test_c2_medium_at_320_cubed_against_oracle():
    """A mid-size grid of the kind BabelBrain users run (C2's skull + brain at 320^3, 2000 columns of 32 planes): since round 6
    the run lists of this size are cut into 8-plane runs (16 from 3000 columns); 400 steps -- the wave is through the bone --
    and, with the wave front half way, the quiet runs of a production call on the same grid."""
    from babelbrain_amd import PropagationModel
    from oracle import oracle as O
    a, k, info = H.make_problem('C2', N=(320, 320, 320), steps=400, stable_dt_fn=oracle_dt, full_sensors=False)
    assert a[0].shape == (320, 320, 320) and info['nt'] == 400
    out_h = PropagationModel().StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, **k)
    out_o = O.StaggeredFDTD_3D_with_relaxation(*a, **k)
    worst = compare_runs(out_h, out_o, geometry=geometry_of(a, k))
    assert out_o[2]['Pressure'].max() > 0
    print('C2 medium 320^3 x 400 steps: worst rel L2 vs oracle %.3e (oracle step loop %.1f s)' % (worst, out_o[-1]['stepLoopSeconds']))


@pytest.mark.timeout(900)
def test_c3_full_size_against_oracle():
    """BASELINE configs[2], the configuration the metric is quoted on: 512^3 CT-derived heterogeneous skull (515 materials,
    QCorrection 3 on bone), CTX-500 annular array, absorbing layer on -- compared with the oracle DIRECTLY at full size:
    140 steps (the wave reaches the skull), Pressure RMS + last map + the sensors of two lines through the focus. The
    oracle needs about 30 s on the box's 16 threads and 9 GB of host memory. Both the default kernels and the fused time
    step (variant 4) are held to it."""
    from babelbrain_amd import PropagationModel, RayleighAndBHTE
    from oracle import oracle as O
    a, k, info = H.make_problem('C3', steps=140, stable_dt_fn=oracle_dt, full_sensors=False, forward=RayleighAndBHTE.ForwardSimple)
    assert a[0].shape == (512, 512, 512) and info['nt'] == 140 and info['n_mat'] == 515
    out_o = O.StaggeredFDTD_3D_with_relaxation(*a, **k)
    assert out_o[2]['Pressure'].max() > 0 and np.count_nonzero(out_o[1]['Pressure']) > 1e6
    for variant in (0, 4):
        out_h = PropagationModel(kernelVariant=variant).StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, **k)
        worst = compare_runs(out_h, out_o, geometry=geometry_of(a, k))
        print('C3 512^3 x 140 steps, variant %d: worst rel L2 vs oracle %.3e (oracle step loop %.1f s)' % (variant, worst, out_o[-1]['stepLoopSeconds']))
        del out_h


def _reduced_against_oracle(config, N, steps):
    """A BASELINE configuration's own material rows (MatFreq[f], BASE:140-167), transducer source plane, spatial step and
    time plan (PPP rule at that frequency) on a reduced grid, default kernels against the oracle on every output. The
    shell's top lies 6 cells below the source plane, so the wave is inside bone (with shear) for most of the run."""
    from babelbrain_amd import PropagationModel, RayleighAndBHTE
    from oracle import oracle as O
    a, k, info = H.make_problem(config, N=N, steps=steps, stable_dt_fn=oracle_dt, forward=RayleighAndBHTE.ForwardSimple)
    assert a[0].shape == N and info['nt'] == steps and info['freq'] == H.CONFIGS[config]['freq']
    assert np.array_equal(a[1], np.array([H.MATERIALS[info['freq']][m] for m in ('Water', 'Cortical', 'Brain')]))
    out_o = O.StaggeredFDTD_3D_with_relaxation(*a, **k)
    rms, last = out_o[2]['Pressure'], out_o[1]['Pressure']
    bone, brain = a[0] == 1, a[0] == 2
    assert bone.sum() > 1e4 and rms[bone].max() > 0 and rms[brain].max() > 0, 'the wave should have gone through bone'
    for variant in (0, 2):
        out_h = PropagationModel(kernelVariant=variant).StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, **k)
        worst = compare_runs(out_h, out_o, geometry=geometry_of(a, k))
        print('%s at %s x %d steps, variant %d: worst rel L2 vs oracle %.3e' % (config, N, steps, variant, worst))
    return info, out_o


def test_c4_reduced_against_oracle():
    """BASELINE configs[3] at 128x128x256: the 700 kHz rows, the H317 source plane (128 elements on an F = 135 mm cap,
    H317.py:19,56-125; the plane the phased-array caller builds, CONCAVE_PHASEDARRAY:296-320) and the 700 kHz time plan."""
    info, _ = _reduced_against_oracle('C4', (128, 128, 256), 600)
    assert info['tx'] == 'h317' and info['freq'] == 700e3 and info['n_sources'] > 1000


def test_c5_reduced_against_oracle():
    """BASELINE configs[4] at 192^3: the 1 MHz rows (cS 1716 m/s, alphaS 329 Np/m in cortical bone) and time plan."""
    info, _ = _reduced_against_oracle('C5', (192, 192, 192), 600)
    assert info['freq'] == 1000e3


@pytest.mark.timeout(900)
def test_c4_full_size_first_steps_against_oracle():
    """BASELINE configs[3] at its FULL size (512x512x1024) for the first 80 steps against the oracle, Pressure RMS over all
    of them + last map + two sensor lines. The dense oracle holds 26 arrays of 1 GiB: needs 45 GB of free host memory
    (skipped below that) and about 0.3 s per step on 16 threads."""
    psutil = pytest.importorskip('psutil')
    if psutil.virtual_memory().available < 45 * 2 ** 30:
        pytest.skip('less than 45 GB of host memory available for the dense oracle at 512x512x1024')
    from babelbrain_amd import PropagationModel, RayleighAndBHTE
    from oracle import oracle as O
    a, k, info = H.make_problem('C4', steps=80, stable_dt_fn=oracle_dt, full_sensors=False, accumulate_all_steps=True,
                                forward=RayleighAndBHTE.ForwardSimple)
    assert a[0].shape == (512, 512, 1024) and info['tx'] == 'h317' and info['n_sources'] > 1e5
    out_h = PropagationModel().StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, **k)
    out_o = O.StaggeredFDTD_3D_with_relaxation(*a, **k)
    worst = compare_runs(out_h, out_o, geometry=geometry_of(a, k))
    rms = out_o[2]['Pressure']
    assert rms[a[0] == 1].max() > 0 and np.count_nonzero(out_o[1]['Pressure']) > 1e6
    print('C4 512x512x1024 x 80 steps: worst rel L2 vs oracle %.3e (oracle step loop %.1f s)' % (worst, out_o[-1]['stepLoopSeconds']))


def _exchange(slabs, group):
    for r in range(len(slabs) - 1):
        lo, hi = slabs[r], slabs[r + 1]
        for f in hi.halo_fields()[group]:
            hi.halo(group, f, 0, False).copy_(lo.halo(group, f, 1, True))
        for f in lo.halo_fields()[group]:
            lo.halo(group, f, 1, False).copy_(hi.halo(group, f, 0, True))


def _single(a, k, variant):
    from babelbrain_amd import PropagationModel
    out = PropagationModel(kernelVariant=variant).StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, **k)
    return out[0]['Pressure'], out[1]['Pressure'], out[2]['Pressure']


def _properties(config, steps_long, steps_short, world):
    import torch
    from babelbrain_amd import RayleighAndBHTE
    N = H.CONFIGS[config]['N']
    # inputs the way a rank of the multi-GPU run builds them (size-1 Ox/Oy/Oz), for the whole domain
    a, k, info = H.make_problem(config, steps=steps_short, stable_dt_fn=_hip_dt, zslab=(0, N[2]), full_sensors=False,
                                forward=RayleighAndBHTE.ForwardSimple)
    assert a[0].shape == N and info['n_sources'] > 1000
    # (1) dense variant 2 == class-specialised variant 3 on a reduced step count
    s3, l3, r3 = _single(a, k, 3)
    assert r3.max() > 0 and np.count_nonzero(l3) > 1e6
    s2, l2, r2 = _single(a, k, 2)
    assert np.array_equal(s2, s3) and np.array_equal(r2, r3) and np.array_equal(l2, l3)
    del s2, l2, r2, s3, l3, r3
    # (2) slabs == single domain, long enough for the wave to cross the first interface
    a, k, info = H.make_problem(config, steps=steps_long, stable_dt_fn=_hip_dt, zslab=(0, N[2]), full_sensors=False,
                                forward=RayleighAndBHTE.ForwardSimple)
    _, l3, r3 = _single(a, k, 3)
    kcut = slab.partition(N[2], world)[1][0]
    assert np.abs(l3[:, :, kcut:kcut + 8]).max() > 0, 'the wave should have crossed the first slab interface'
    # the split goes through the drop-in call itself (bfd_group_*: every slab on this one GPU, step loop and halo copies
    # inside the library), as a caller with several GPUs would make it
    from babelbrain_amd import PropagationModel
    out = PropagationModel(devices=[0] * world, kernelVariant=3).StaggeredFDTD_3D_with_relaxation(*a, SILENT=True, **k)
    assert len(out[-1]['slabs']) == world and out[-1]['timing']['overlapped']
    assert np.array_equal(out[2]['Pressure'], r3), 'RMS map of the %d-slab call' % world
    assert np.array_equal(out[1]['Pressure'], l3), 'last map of the %d-slab call' % world
    return info


@pytest.mark.timeout(1200)
def test_c4_h317_512x512x1024_properties():
    """BASELINE configs[3]: 512x512x1024 domain, H317 phased array (128 elements, F = 135 mm), 700 kHz."""
    info = _properties('C4', steps_long=700, steps_short=200, world=8)
    assert info['freq'] == 700e3 and info['tx'] == 'h317'


@pytest.mark.timeout(1800)
def test_c5_1024_cubed_1mhz_properties():
    """BASELINE configs[4]: 1024^3 full-head domain at 1 MHz, 6 points per wavelength (81 GB on the one GPU)."""
    info = _properties('C5', steps_long=700, steps_short=200, world=8)
    assert info['freq'] == 1000e3 and info['N'] == (1024, 1024, 1024)
