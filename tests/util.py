import numpy as np

from oracle import oracle as O


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    den = np.sqrt(np.sum(b * b))
    if den == 0:
        return float(np.sqrt(np.sum(a * a)))
    return float(np.sqrt(np.sum((a - b) ** 2)) / den)


def free_port():
    """A TCP port nobody listens on (rendezvous of spawned ranks on 127.0.0.1)."""
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def run_ranks(worker, world, timeout=800, extra=()):
    """Spawn `world` processes running worker(rank, world, port, queue, *extra), return what rank 0 put on the queue.
    Polls the children while waiting (a crashed rank fails the test at once instead of stalling it) and never leaves
    orphans behind."""
    import queue
    import time
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, q) + tuple(extra)) for r in range(world)]
    for p in procs:
        p.start()
    result = None
    try:
        deadline = time.time() + timeout
        while result is None:
            try:
                result = q.get(timeout=2)
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead, 'a rank died (exit codes %s)' % dead
                assert time.time() < deadline, 'ranks timed out'
        for p in procs:
            p.join(120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
            p.join(10)
    return result


def oracle_dt(ml, f, h, acfl):
    return O.stable_dt(ml, f, True, h, acfl)


ALL_MAPS = ['Vx', 'Vy', 'Vz', 'Sigmaxx', 'Sigmayy', 'Sigmazz', 'Sigmaxy', 'Sigmaxz', 'Sigmayz', 'Pressure']


def geometry_of(args, kwargs):
    """(N, NDelta, MaterialMap) of a solver call: what assert_same needs to say where a differing cell lies."""
    return args[0].shape, int(kwargs['NDelta']), args[0]


def _ordered_bits(a):
    """float32 -> int64 that counts representable values in order (-0 and +0 both map to 0): differences are distances in ulps"""
    b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff), b)


def _where(idx, shape, geometry, sensors):
    """One element's position in words a kernel author can use."""
    idx = tuple(int(v) for v in idx)
    if len(shape) == 3:
        i, j, k = idx
        s = '(i, j, k) = (%d, %d, %d)' % (i, j, k)
        if geometry is not None:
            N, nd, mm = geometry
            layer = any(c < nd or c >= n - nd for c, n in zip(idx, N))
            s += ', %s the absorbing layer, material %d, sub-tile (%d, %d, %d) cell (%d, %d, %d) of 64x8x8' % (
                'inside' if layer else 'outside', int(np.asarray(mm)[i, j, k]), i // 64, j // 8, k // 8, i % 64, j % 8, k % 8)
        return s
    if len(shape) == 2:
        s = '(sensor, sample) = (%d, %d)' % idx
        if sensors is not None:
            index, N = sensors
            u = int(index[idx[0]]) - 1                          # IndexSensorMap is 1-based, x fastest
            s += ', sensor voxel ' + _where((u % N[0], (u // N[0]) % N[1], u // (N[0] * N[1])), tuple(N), geometry, None)
        return s
    return 'index %s' % (idx,)


def assert_same(got, ref, what, geometry=None, sensors=None):
    """got == ref element by element: same shape, both float32, every element finite on both sides, every element equal in
    value. Equal in value, not in bits: +0 == -0 is accepted (a sum that cancels may carry either sign; no output depends
    on it), everything else must be the same float32. geometry = (N, NDelta, MaterialMap) lets the failure message say
    whether a differing cell of a volume lies in the absorbing layer, its material and its 64x8x8 sub-tile; sensor blocks
    (sensor, sample) name the sensor's voxel when sensors = (IndexSensorMap, N) comes with it. The message also carries
    the number and share of differing elements, the first and the worst one (by |got - ref|), the largest distance in
    float32 ulps and the whole-array rel L2 the suite used to assert."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, '%s: shape %s against %s' % (what, got.shape, ref.shape)
    assert got.dtype == np.float32 and ref.dtype == np.float32, '%s: dtypes %s / %s, expected float32' % (what, got.dtype, ref.dtype)
    for side, a in (('result', got), ('reference', ref)):
        if not np.isfinite(a).all():
            bad = ~np.isfinite(a)
            first = np.unravel_index(int(np.flatnonzero(bad)[0]), a.shape)
            raise AssertionError('%s: %d non-finite element(s) in the %s, first %r at %s' % (
                what, int(bad.sum()), side, float(a[first]), _where(first, a.shape, geometry, sensors)))
    if np.array_equal(got, ref):
        return
    diff = got != ref
    n = int(diff.sum())
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    first = np.unravel_index(int(np.flatnonzero(diff)[0]), got.shape)
    worst = np.unravel_index(int(np.argmax(err)), got.shape)
    ulps = np.abs(_ordered_bits(got) - _ordered_bits(ref))

    def one(name, idx):
        return '%s: got %.9g, expected %.9g (%d ulp) at %s' % (name, float(got[idx]), float(ref[idx]), int(ulps[idx]),
                                                             _where(idx, got.shape, geometry, sensors))
    raise AssertionError('%s: %d of %d elements differ (%.4g %%); %s; %s; largest distance %d ulp; whole-array rel L2 %.3e' % (
        what, n, got.size, 100.0 * n / got.size, one('first', first), one('worst', worst), int(ulps.max()), rel_l2(got, ref)))


def compare_runs(out_hip, out_ref, tol=1e-5, both=False, exact=True, geometry=None):
    """out_* are the tuples StaggeredFDTD_3D_with_relaxation returns. Returns the worst rel-L2.
    exact (the default): every output goes through assert_same -- the form for the device against the oracle, and for two
    device runs that must agree bit for bit; the rel-L2 is still computed, held to tol and returned. exact=False asserts the
    whole-array rel-L2 bound alone: only for two schemes that differ on purpose, never with the oracle on one side.
    geometry: see assert_same (optional; without it a failure names indices only)."""
    worst = 0.0
    Sh, Lh = out_hip[0], out_hip[1]
    Sr, Lr = out_ref[0], out_ref[1]
    assert np.array_equal(out_hip[-1]['IndexSensorMap'], out_ref[-1]['IndexSensorMap'])
    np.testing.assert_allclose(Sh['time'], Sr['time'], rtol=0, atol=1e-15)
    N = geometry[0] if geometry is not None else next((v.shape for v in Lr.values()), None)
    sensors = None if N is None else (out_ref[-1]['IndexSensorMap'], N)
    dicts = [(Sh, Sr, 'sensor'), (Lh, Lr, 'last'), (out_hip[2], out_ref[2], 'rms/peak')]
    if both:
        dicts.append((out_hip[3], out_ref[3], 'peak'))
    for dh, dr, what in dicts:
        assert set(dh.keys()) == set(dr.keys()), (what, dh.keys(), dr.keys())
        for k in dr:
            if k == 'time':
                continue
            assert dh[k].shape == dr[k].shape, (what, k, dh[k].shape, dr[k].shape)
            assert dh[k].dtype == np.float32
            if exact:
                assert_same(dh[k], dr[k], '%s[%s]' % (what, k), geometry, sensors)
            e = rel_l2(dh[k], dr[k])
            assert e <= tol, '%s[%s]: rel L2 %.3e > %.1e' % (what, k, e, tol)
            worst = max(worst, e)
    return worst
