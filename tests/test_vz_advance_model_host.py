"""Advanced Vz, the plane range (bfd_kernels_fluid.hip, stress_fluid_body): a float32 model of the fluid time step on columns cut into z-runs. The
stress pass of a run, which holds the column's Vz, also stores the new Vz of the planes [kbeg + lo, kend - hi]; the velocity pass skips Vz there.
Runs are visited in a random order in either pass and work on the live arrays, as workgroups do. With lo = 1, hi = 3 every order must equal the
plain two-pass scheme bit for bit; one plane more at either end must differ for some order (the run below reads Vz(kbeg); the run above
reads Vz(kend-2), and the new Szz(kend) is not this run's)."""
import numpy as np

F = np.float32
C0, C1 = F(9.0 / 8.0), F(1.0 / 24.0)
NX, NY, NZ = 6, 5, 40
G = 2           # ghost cells on every side, zero


def d4(a, b, c, d):
    """both staggered differences: dminus4(v(-2), v(-1), v(0), v(+1)) and dplus4(s(-1), s(0), s(+1), s(+2))"""
    return C0 * (c - b) - C1 * (d - a)


def make_state(seed):
    rng = np.random.default_rng(seed)
    shape = (NX + 2 * G, NY + 2 * G, NZ + 2 * G)
    st = {}
    for n in ('Vx', 'Vy', 'Vz', 'S'):
        st[n] = np.zeros(shape, F)
        st[n][G:-G, G:-G, G:-G] = rng.standard_normal((NX, NY, NZ)).astype(F)
    st['A'] = (0.05 + 0.1 * rng.random(shape)).astype(F)
    st['r'] = (0.05 + 0.1 * rng.random(shape)).astype(F)
    return st


def make_runs(seed):
    """per column: cuts into runs of 1 .. 16 planes"""
    rng = np.random.default_rng(seed)
    runs = []
    for i in range(NX):
        for j in range(NY):
            k = 0
            while k < NZ:
                e = min(NZ, k + int(rng.integers(1, 17)))
                runs.append((i, j, k, e))
                k = e
    return runs


def stress_run(st, run, lo, hi):
    i, j, kb, ke = run
    I, J = i + G, j + G
    k = slice(kb + G, ke + G)
    n = ke - kb
    Vx, Vy, S = st['Vx'], st['Vy'], st['S']
    vz = st['Vz'][I, J, kb:ke + 3].copy()          # planes kb-2 .. ke: the kernel's z-queue, all read before the store that could touch them
    dx = d4(Vx[I - 2, J, k], Vx[I - 1, J, k], Vx[I, J, k], Vx[I + 1, J, k])
    dy = d4(Vy[I, J - 2, k], Vy[I, J - 1, k], Vy[I, J, k], Vy[I, J + 1, k])
    dz = d4(vz[0:n], vz[1:n + 1], vz[2:n + 2], vz[3:n + 3])
    S[I, J, k] = S[I, J, k] + st['A'][I, J, k] * ((dx + dy) + dz)
    if lo is None:
        return
    p0, p1 = kb + lo, ke - hi                      # advanced planes p0 .. p1: new Szz of p-1 .. p+2 from the live array (this run's, if the range is right)
    if p1 < p0:
        return
    p = slice(p0 + G, p1 + 1 + G)
    sm1, s0, sp1, sp2 = (S[I, J, p0 + G + o:p1 + 1 + G + o] for o in (-1, 0, 1, 2))
    r = st['r']
    old = vz[p0 - kb + 2:p1 + 1 - kb + 2]
    st['Vz'][I, J, p] = old + (F(0.5) * (r[I, J, p] + r[I, J, p0 + G + 1:p1 + 2 + G])) * d4(sm1, s0, sp1, sp2)


def velocity_run(st, run, lo, hi):
    i, j, kb, ke = run
    I, J = i + G, j + G
    k = slice(kb + G, ke + G)
    S, r = st['S'], st['r']
    s0 = S[I, J, k]
    st['Vx'][I, J, k] = st['Vx'][I, J, k] + (F(0.5) * (r[I, J, k] + r[I + 1, J, k])) * d4(S[I - 1, J, k], s0, S[I + 1, J, k], S[I + 2, J, k])
    st['Vy'][I, J, k] = st['Vy'][I, J, k] + (F(0.5) * (r[I, J, k] + r[I, J + 1, k])) * d4(S[I, J - 1, k], s0, S[I, J + 1, k], S[I, J + 2, k])
    for kk in range(kb, ke):
        if lo is not None and kb + lo <= kk <= ke - hi:
            continue                               # the stress pass has stored this plane's new Vz
        K = kk + G
        st['Vz'][I, J, K] = st['Vz'][I, J, K] + (F(0.5) * (r[I, J, K] + r[I, J, K + 1])) * d4(S[I, J, K - 1], S[I, J, K], S[I, J, K + 1], S[I, J, K + 2])


def evolve(runs, steps, lo, hi, order_seed, state_seed=1):
    st = make_state(state_seed)
    rng = np.random.default_rng(order_seed)
    for n in range(steps):
        for q in rng.permutation(len(runs)):
            stress_run(st, runs[q], lo, hi)
        for q in rng.permutation(len(runs)):
            velocity_run(st, runs[q], lo, hi)
        st['Vz'][G + NX // 2, G + NY // 2, G + 3] += F(np.sin(0.7 * n))        # a velocity-type source, after the velocity pass
    return st


def same(a, b):
    return all(np.array_equal(a[n], b[n]) for n in ('Vx', 'Vy', 'Vz', 'S'))


def test_inner_planes_equal_the_two_pass_scheme():
    runs = make_runs(7)
    assert any(e - b < 4 for _, _, b, e in runs) and any(e - b == 16 for _, _, b, e in runs)
    whole = [(i, j, 0, NZ) for i in range(NX) for j in range(NY)]
    ref = evolve(whole, 30, None, None, 0)
    assert same(ref, evolve(runs, 30, None, None, 11))          # the cut into runs and the order alone change nothing
    for order_seed in (21, 22, 23):
        assert same(ref, evolve(runs, 30, 1, 3, order_seed))
    assert np.isfinite(ref['S']).all() and np.abs(ref['Vz']).max() > 0


def test_one_plane_more_at_either_end_differs():
    runs = make_runs(7)
    whole = [(i, j, 0, NZ) for i in range(NX) for j in range(NY)]
    ref = evolve(whole, 3, None, None, 0)
    for lo, hi in ((0, 3), (1, 2)):
        assert any(not same(ref, evolve(runs, 3, lo, hi, order_seed)) for order_seed in range(31, 36)), (lo, hi)
