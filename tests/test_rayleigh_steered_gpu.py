"""Element-resolved Rayleigh integral on the device (bfd_rayleigh_forward_elements through RayleighAndBHTE.ForwardSteered /
ForwardElements): G[e][n], the field at point n of element e alone, and steered fields sum_e w[e][s] G[e][n].

Geometry and field points are those of tests/test_rayleigh_gpu.py, rebuilt here with the same harness calls and seeds: the 1 MHz
bowl of 24 rings (first 1100 records), and per point count a near-field plane, the mid-field cloud, 2048 far points and a partly
filled last workgroup. The kernel holds 1 field point per lane below 2^18 points and 2 from there on (bfd_rayleigh.hip), so 4097
and 2^18 + 37 points reach both; 2^20 + 1029 is added where the result is tied to ForwardSimple, which holds 4 there.

Bit-for-bit checks rest on the kernel's order of summation: float32 sums of 16 records counted from the element's first record,
float64 per element, the weights applied in float64 per element in ascending order. Against the float64 oracle
(oracle.rayleigh_oracle.ForwardSimple with u0 = w[elem(m)][s] sub[m], or on one element's records) every point is held to
|got - ref| <= RAYLEIGH_C s_n.

The largest |got - ref| / s_n measured on the MI355X is recorded beside RAYLEIGH_C below."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from babelbrain_amd import harness as H
from oracle import rayleigh_oracle as RO

pytestmark = pytest.mark.gpu

# The project's bound for this kernel's pair arithmetic (tests/test_rayleigh_gpu.py: 4 x the largest ratio measured there over
# 32 cases of rayleigh_forward, 3.552e-7 on one attenuated source). The element kernel has the same roundings per term and
# applies the weights in float64 to float64 sums, so the same constant is the claim. A term dropped or doubled among M = 1100
# equal ones moves a point by 1 / M = 9.1e-4 of s_n, 640 x the bound.
RAYLEIGH_C = 4 * 3.552e-7
assert RAYLEIGH_C * 100 < 1.0 / 1100
# Largest |got - ref| / s_n measured on the MI355X in this file: 4.270e-7 (test_every_record_its_own_element, an attenuated element of
# one record; 3.47e-7 without attenuation), 0.30 of the bound. Per test: test_against_float64_point_by_point element fields 3.18e-7 ..
# 4.03e-7 (the one-record elements), steered columns 2.6e-8 .. 4.6e-8; nElem = M steered columns 1.3e-8 .. 2.2e-8;
# test_reference_loops_on_h317 element fields 8.7e-8, steered columns 1.1e-8, and 0 against the loop of ForwardSimple calls.
# The whole file takes 25 s, 11 s of them the import of torch in the devices test.

HERE = os.path.dirname(os.path.abspath(__file__))
M_ALL = 1100
# Partition A of the first 1100 records: sizes from {1, 15, 16, 17, 31, 33, 511}; one empty element (index 3); element 7 has 511
# records from record 113 (not a multiple of 16) to 623, across the LDS block edge at record 512.
PART_A = [17, 1, 15, 0, 16, 33, 31, 511] + [33, 17, 31, 16, 15, 1] * 4 + [17] + [1] * 7
STRADDLE_A = 7
# Partition B of the first 1074 records: element 1 has 513 records from record 16 (a multiple of 16) across record 512, element 3
# has 512 records from record 530 across record 1024; an empty element between.
PART_B = [16, 513, 1, 512, 0, 17, 15]
assert sum(PART_A) == M_ALL and sum(PART_A[:STRADDLE_A]) == 113 and sum(PART_B) == 1074


def _template_of(n_points):
    """field points per lane the library picks for a launch of that many points in rayleigh_elements (bfd_rayleigh.hip)"""
    return 2 if n_points >= 1 << 18 else 1


def _template_of_forward_simple(n_points):
    return 4 if n_points >= 1 << 20 else 2 if n_points >= 1 << 18 else 1


N_BY_TEMPLATE = {1: 4097, 2: (1 << 18) + 37}
assert all(_template_of(n) == p for p, n in N_BY_TEMPLATE.items())
N_WIDE = (1 << 20) + 1029


def _k(kimag):
    return complex(np.array(2 * np.pi * 1e6 / 1500.0 + 1j * kimag).astype(np.complex64))


@functools.lru_cache(maxsize=None)
def _bowl_1mhz():
    pts, ds = H._bowl_points(60e-3, 55e-3, 24, 0.0)
    assert len(ds) > M_ALL and pts[:28, 2].max() < 0.08e-3
    rng = np.random.default_rng(11)
    u0 = (rng.normal(size=len(ds)) + 1j * rng.normal(size=len(ds))).astype(np.complex64)
    out = pts.astype(np.float32), ds.astype(np.float32), u0
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _field_points(N):
    """As in tests/test_rayleigh_gpu.py: a 32 x 32 plane 0.5 mm above the flat centre of the bowl, the mid-field cloud, 2048 points
    0.25 m away. The subset held point by point: the plane, the last 256 x 4 + 64 points (the last, partly filled workgroup and
    the one before it at any number of points per lane), 4096 random ones."""
    rng = np.random.default_rng(N)
    g = (np.arange(32) - 15.5) * (10e-3 / 32)
    X, Y = np.meshgrid(g, g, indexing='ij')
    plane = np.stack([X.ravel(), Y.ravel(), np.full(X.size, 0.5e-3)], 1)
    nfar = 2048
    n = N - len(plane) - nfar
    cloud = np.stack([rng.uniform(-40e-3, 40e-3, n), rng.uniform(-40e-3, 40e-3, n), rng.uniform(20e-3, 160e-3, n)], 1)
    far = np.stack([rng.uniform(-20e-3, 20e-3, nfar), rng.uniform(-20e-3, 20e-3, nfar), rng.uniform(0.25, 0.26, nfar)], 1)
    rf = np.concatenate([plane, cloud, far]).astype(np.float32)
    tail = 256 * 4 + 64
    sub = np.unique(np.concatenate([np.arange(1024), np.arange(N - tail, N), rng.integers(0, N, 4096)]))
    assert rf.shape == (N, 3) and tail < nfar and N % 1024 != 0 and N % 512 != 0 and N % 256 != 0
    rf.setflags(write=False)
    sub.setflags(write=False)
    return rf, sub


@functools.lru_cache(maxsize=None)
def _weights(nElem, S, seed=5):
    rng = np.random.default_rng(seed)
    w = (rng.normal(size=(nElem, S)) + 1j * rng.normal(size=(nElem, S))).astype(np.complex64)
    w.setflags(write=False)
    return w


def _elem_of(counts):
    return np.repeat(np.arange(len(counts)), counts)


def _term_scale(k, cen, ds, u0, rf):
    """s_n = |k| / 2 pi  sum_m |u0_m ds_m| exp(Im k R_nm) / R_nm: the sum of the magnitudes of a point's terms (float64)"""
    R = np.sqrt(((rf.astype(np.float64)[:, None, :] - cen.astype(np.float64)[None, :, :]) ** 2).sum(axis=2))
    w = np.abs(np.asarray(u0).astype(np.complex128)) * ds.astype(np.float64)
    return abs(k) / (2 * np.pi) * ((np.exp(k.imag * R) / R) @ w)


def _R():
    from babelbrain_amd import RayleighAndBHTE as R
    # one device, one launch: points shared among several devices would reach other templates than _template_of says
    R.set_devices(None)
    assert R._devices is None and not os.environ.get('BABELFDTD_DEVICES')
    return R


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same_bits(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = a == b
    assert same.all(), '%s: %d of %d words differ, first at flat position %d' % (what, same.size - same.sum(), same.size, np.flatnonzero(~same.ravel())[0])


def _hold(got, ref, s, what):
    """|got - ref| <= RAYLEIGH_C s_n for every point; prints the largest ratio before it asserts"""
    assert np.isfinite(_bits(got).view(np.float32)).all() and np.abs(ref).min() > 0, what
    ratio = np.abs(got.astype(np.complex128) - ref) / s
    worst = int(np.argmax(ratio))
    print('%s: max |err| / s_n = %.3e at position %d of %d' % (what, ratio[worst], worst, len(ratio)))
    assert ratio[worst] <= RAYLEIGH_C, (what, ratio[worst], worst)
    return ratio[worst]


# ---- 1. tie to rayleigh_forward ----
@pytest.mark.parametrize('kimag', [0.0, -4.5])
@pytest.mark.parametrize('N', [N_BY_TEMPLATE[1], N_BY_TEMPLATE[2], N_WIDE])
def test_one_element_one_column_is_forward_simple(N, kimag, monkeypatch):
    """nElem = 1, S = 1, w = 1 + 0i, u0 = the seeded u0: the groups of 16 of the one element are those of rayleigh_forward and
    1 g - 0 g' is exact, so ForwardSteered equals ForwardSimple word for word -- at source counts on the edges of the groups of
    16 and of the LDS blocks of 512, in both templates, and against ForwardSimple's 4 points per lane at 2^20 + 1029 points.
    ForwardElements gives the same row."""
    monkeypatch.delenv('BABELFDTD_DEVICES', raising=False)
    R = _R()
    assert _template_of(N) == (1 if N < 1 << 18 else 2) and _template_of_forward_simple(N) == (1 if N < 1 << 18 else 2 if N < 1 << 20 else 4)
    rf, sub = _field_points(N)
    k = _k(kimag)
    for M in (1, 16, 17, 512, 513, 1100):
        cen, ds, u0 = (v[:M] for v in _bowl_1mhz())
        want = R.ForwardSimple(k, cen, ds, u0, rf)
        got = R.ForwardSteered(k, cen, ds, M, np.ones(1, np.complex64), rf, u0=u0)
        assert got.shape == (1, N) and got.dtype == np.complex64 and R.last_kernel_ms > 0
        _assert_same_bits(got[0], want, 'N=%d M=%d kimag=%g steered' % (N, M, kimag))
        if N != N_WIDE or M == 1100:
            el = R.ForwardElements(k, cen, ds, [M], rf, u0=u0)
            _assert_same_bits(el[0], want, 'N=%d M=%d kimag=%g elements' % (N, M, kimag))


# ---- 2. column independence ----
@pytest.mark.parametrize('kimag', [0.0, -4.5])
@pytest.mark.parametrize('ppl', [1, 2])
def test_columns_do_not_depend_on_the_launch(ppl, kimag, monkeypatch):
    """S = 11 columns (two launches of 8): every column equals the S = 1 call of that column alone; column 9 repeats column 2 (another
    launch, another place) and gives the same words; the values of the subset out of the large launch equal those of a launch of
    the subset alone (one point per lane)."""
    monkeypatch.delenv('BABELFDTD_DEVICES', raising=False)
    R = _R()
    N = N_BY_TEMPLATE[ppl]
    rf, sub = _field_points(N)
    assert _template_of(N) == ppl and _template_of(len(sub)) == 1
    cen, ds, u0 = (v[:M_ALL] for v in _bowl_1mhz())
    k = _k(kimag)
    W = _weights(len(PART_A), 11).copy()
    W[:, 9] = W[:, 2]
    big = R.ForwardSteered(k, cen, ds, PART_A, W, rf, u0=u0)
    assert big.shape == (11, N) and big.dtype == np.complex64
    assert np.isfinite(_bits(big).view(np.float32)).all() and np.abs(big).min() > 0
    _assert_same_bits(big[9], big[2], 'repeated column')
    for s in range(11):
        alone = R.ForwardSteered(k, cen, ds, PART_A, W[:, s], rf, u0=u0)
        assert alone.shape == (1, N)
        _assert_same_bits(alone[0], big[s], 'column %d alone' % s)
    small = R.ForwardSteered(k, cen, ds, PART_A, W, rf[sub], u0=u0)
    _assert_same_bits(small, big[:, sub], 'launch of the subset alone')


# ---- 3. element isolation ----
@pytest.mark.parametrize('kimag', [0.0, -4.5])
@pytest.mark.parametrize('ppl', [1, 2])
def test_an_element_does_not_depend_on_its_neighbours(ppl, kimag, monkeypatch):
    """ForwardElements(...)[e] equals ForwardElements on the records of element e alone (where it is the one element, from record 0
    on): for the element of 511 records from record 113 across record 512, for elements that start at records 17 and 33, and in
    partition B for 513 records from record 16 and 512 from record 530. An empty element gives zeros. The steered call with the
    unit vector of e gives the same words as row e."""
    monkeypatch.delenv('BABELFDTD_DEVICES', raising=False)
    R = _R()
    N = N_BY_TEMPLATE[ppl]
    rf, sub = _field_points(N)
    k = _k(kimag)
    for part, picks in ((PART_A, (1, 2, STRADDLE_A, 9, len(PART_A) - 1)), (PART_B, (1, 3, 6))):
        M = sum(part)
        cen, ds, u0 = (v[:M] for v in _bowl_1mhz())
        start = np.concatenate([[0], np.cumsum(part)])
        G = R.ForwardElements(k, cen, ds, [[c] for c in part], rf, u0=u0)
        assert G.shape == (len(part), N) and G.dtype == np.complex64 and np.isfinite(_bits(G).view(np.float32)).all()
        empty = part.index(0)
        assert (G[empty] == 0).all()
        assert all(np.abs(G[e]).min() > 0 for e in range(len(part)) if part[e])
        unit = np.zeros((len(part), len(picks)), np.complex64)
        for j, e in enumerate(picks):
            a, b = start[e], start[e + 1]
            alone = R.ForwardElements(k, cen[a:b], ds[a:b], [b - a], rf, u0=u0[a:b])
            _assert_same_bits(alone[0], G[e], 'element %d (records %d..%d) alone' % (e, a, b - 1))
            unit[e, j] = 1.0
        st = R.ForwardSteered(k, cen, ds, part, unit, rf, u0=u0)
        _assert_same_bits(st, G[list(picks)], 'unit-vector steering')


# ---- 4. against float64 ----
@functools.lru_cache(maxsize=None)
def _float64_case(N, kimag, which):
    """Oracle values on the subset of N's points: the 8 steered columns, the element fields, and their term scales."""
    part = PART_A if which == 'A' else PART_B
    M = sum(part)
    cen, ds, u0 = (v[:M] for v in _bowl_1mhz())
    rf, sub = _field_points(N)
    k = _k(kimag)
    W = _weights(len(part), 8)
    elem = _elem_of(part)
    R = np.sqrt(((rf[sub].astype(np.float64)[:, None, :] - cen.astype(np.float64)[None, :, :]) ** 2).sum(axis=2))
    mag = abs(k) / (2 * np.pi) * np.exp(k.imag * R) / R
    cols, scol = [], []
    for s in range(8):
        u = W[:, s].astype(np.complex128)[elem] * u0.astype(np.complex128)
        cols.append(RO.ForwardSimple(k, cen, ds, u, rf[sub]))
        scol.append(mag @ (np.abs(u) * ds.astype(np.float64)))
    start = np.concatenate([[0], np.cumsum(part)])
    els, sel = [], []
    for e in range(len(part)):
        a, b = start[e], start[e + 1]
        els.append(RO.ForwardSimple(k, cen[a:b], ds[a:b], u0[a:b], rf[sub]) if b > a else None)
        sel.append(mag[:, a:b] @ (np.abs(u0[a:b].astype(np.complex128)) * ds[a:b].astype(np.float64)))
    return cols, scol, els, sel


@pytest.mark.parametrize('N,kimag,which', [(N_BY_TEMPLATE[1], 0.0, 'A'), (N_BY_TEMPLATE[1], -4.5, 'A'), (N_BY_TEMPLATE[2], 0.0, 'A'),
                                           (N_BY_TEMPLATE[2], -4.5, 'A'), (N_BY_TEMPLATE[1], 0.0, 'B'), (N_BY_TEMPLATE[2], -4.5, 'B')])
def test_against_float64_point_by_point(N, kimag, which, monkeypatch):
    """Every column of a seeded S = 8 matrix against oracle.ForwardSimple with u0 = w[elem(m)][s] u0[m], and every element field
    against oracle.ForwardSimple on the element's records: |got_n - ref_n| <= RAYLEIGH_C s_n per point, s_n the sum of the
    magnitudes of the point's terms, weights included."""
    monkeypatch.delenv('BABELFDTD_DEVICES', raising=False)
    R = _R()
    part = PART_A if which == 'A' else PART_B
    M = sum(part)
    cen, ds, u0 = (v[:M] for v in _bowl_1mhz())
    rf, sub = _field_points(N)
    k = _k(kimag)
    cols, scol, els, sel = _float64_case(N, kimag, which)
    got = R.ForwardSteered(k, cen, ds, part, _weights(len(part), 8), rf, u0=u0)
    assert got.shape == (8, N) and np.isfinite(_bits(got).view(np.float32)).all()
    worst = max(_hold(got[s][sub], cols[s], scol[s], 'N=%d kimag=%g %s column %d' % (N, kimag, which, s)) for s in range(8))
    G = R.ForwardElements(k, cen, ds, part, rf, u0=u0)
    assert G.shape == (len(part), N) and np.isfinite(_bits(G).view(np.float32)).all()
    worst_e = 0.0
    for e in range(len(part)):
        if els[e] is None:
            assert (G[e] == 0).all()
        else:
            worst_e = max(worst_e, _hold(G[e][sub], els[e], sel[e], 'N=%d kimag=%g %s element %d (%d records)' % (N, kimag, which, e, part[e])))
    print('N=%d (PPL=%d, ATT=%d) partition %s: largest ratio, columns %.3e, elements %.3e; bound %.3e' % (
        N, _template_of(N), kimag != 0, which, worst, worst_e, RAYLEIGH_C))


@pytest.mark.parametrize('kimag', [0.0, -4.5])
def test_every_record_its_own_element(kimag, monkeypatch):
    """nElem = M = 1100 (every element ends after its first record): the element fields on 512 of the points against the oracle on
    one record each, and two steered columns against the oracle with the expanded u0."""
    monkeypatch.delenv('BABELFDTD_DEVICES', raising=False)
    R = _R()
    N = N_BY_TEMPLATE[1]
    cen, ds, u0 = (v[:M_ALL] for v in _bowl_1mhz())
    rf, sub = _field_points(N)
    sub = sub[::8]
    k = _k(kimag)
    G = R.ForwardElements(k, cen, ds, 1, rf, u0=u0)
    assert G.shape == (M_ALL, N)
    Rr = np.sqrt(((rf[sub].astype(np.float64)[None, :, :] - cen.astype(np.float64)[:, None, :]) ** 2).sum(axis=2))       # [m][n]
    amp = (u0.astype(np.complex128) * ds.astype(np.float64))[:, None]
    ref = 1j * k / (2 * np.pi) * amp * np.exp(-1j * k * Rr) / Rr
    s = abs(k) / (2 * np.pi) * np.abs(amp) * np.exp(k.imag * Rr) / Rr
    for e in (0, 1, 511, 512, 1099):        # the formula above is oracle.ForwardSimple on one record
        assert np.allclose(ref[e], RO.ForwardSimple(k, cen[e:e + 1], ds[e:e + 1], u0[e:e + 1], rf[sub]), rtol=1e-13, atol=0)
    _hold(G[:, sub].ravel(), ref.ravel(), s.ravel(), 'nElem = M, kimag=%g, element fields' % kimag)
    W = _weights(M_ALL, 2)
    got = R.ForwardSteered(k, cen, ds, np.ones(M_ALL, np.int64), W, rf, u0=u0)
    for c in range(2):
        u = W[:, c].astype(np.complex128) * u0.astype(np.complex128)
        _hold(got[c][sub], RO.ForwardSimple(k, cen, ds, u, rf[sub]), _term_scale(k, cen, ds, u, rf[sub]), 'nElem = M, kimag=%g, column %d' % (kimag, c))


# ---- 5. the reference's loops ----
def test_reference_loops_on_h317(monkeypatch):
    """The 128 H317 element centres, each element a seeded patch of 9 records within 4 mm of its centre. (i) The per-element
    back-propagation loops (H246:333-339, ANNULAR:379-384, TxCalibration:323-328): ForwardElements at one point against the loop of
    128 ForwardSimple calls. (ii) Multi-point steering (CONCAVE:91-107, 298-314): ForwardSteered with harness.steering_weights
    columns for three foci against ForwardSimple with the expanded u0."""
    monkeypatch.delenv('BABELFDTD_DEVICES', raising=False)
    R = _R()
    ec = np.array(json.load(open(os.path.join(HERE, 'golden', 'h317_elements.json')))['centres_m'], np.float64)
    rng = np.random.default_rng(317)
    per = 9
    cen = (ec[:, None, :] + rng.uniform(-4e-3, 4e-3, (128, per, 3))).reshape(-1, 3).astype(np.float32)
    ds = rng.uniform(0.5e-6, 1.5e-6, 128 * per).astype(np.float32)
    k = complex(np.array(2 * np.pi * 250e3 / 1500.0).astype(np.complex64))
    point = np.array([[2e-3, -1e-3, 135e-3]], np.float32)
    G = R.ForwardElements(k, cen, ds, per, point)
    assert G.shape == (128, 1)
    ones = np.ones(per, np.complex64)
    loop = np.array([R.ForwardSimple(k, cen[e * per:(e + 1) * per], ds[e * per:(e + 1) * per], ones, point)[0] for e in range(128)])
    ref = np.array([RO.ForwardSimple(k, cen[e * per:(e + 1) * per], ds[e * per:(e + 1) * per], ones, point)[0] for e in range(128)])
    s = np.array([_term_scale(k, cen[e * per:(e + 1) * per], ds[e * per:(e + 1) * per], ones, point)[0] for e in range(128)])
    assert np.isfinite(_bits(G).view(np.float32)).all() and np.abs(ref).min() > 0
    r_loop = np.abs(G[:, 0].astype(np.complex128) - loop.astype(np.complex128)) / s
    print('ForwardElements against the loop of 128 ForwardSimple calls: max |diff| / s_n = %.3e' % r_loop.max())
    assert r_loop.max() <= RAYLEIGH_C
    _hold(G[:, 0], ref, s, 'ForwardElements against the float64 oracle, one point')
    foci = np.array([[0.0, 0.0, 135e-3], [8e-3, -4e-3, 128e-3], [-5e-3, 6e-3, 150e-3]])
    W = H.steering_weights(k, ec, foci)
    rf = np.concatenate([foci, np.stack([rng.uniform(-15e-3, 15e-3, 2000), rng.uniform(-15e-3, 15e-3, 2000), rng.uniform(100e-3, 170e-3, 2000)], 1)]).astype(np.float32)
    got = R.ForwardSteered(k, cen, ds, per, W, rf)
    assert got.shape == (3, len(rf))
    for c in range(3):
        u = np.repeat(W[:, c].astype(np.complex128), per)
        want = R.ForwardSimple(k, cen, ds, u.astype(np.complex64), rf)
        sc = _term_scale(k, cen, ds, u, rf)
        r = np.abs(got[c].astype(np.complex128) - want.astype(np.complex128)) / sc
        print('steering column %d against ForwardSimple with the expanded u0: max |diff| / s_n = %.3e' % (c, r.max()))
        assert r.max() <= RAYLEIGH_C
        _hold(got[c], RO.ForwardSimple(k, cen, ds, u, rf), sc, 'steering column %d against the float64 oracle' % c)


# ---- 6. devices ----
def test_field_points_shared_among_devices(monkeypatch):
    """As for ForwardSimple: set_devices([...]) / BABELFDTD_DEVICES deal the field points to the listed devices in contiguous
    shares, one host thread each (ordinals may repeat). The result is the single-device one bit for bit."""
    import torch
    from babelbrain_amd import RayleighAndBHTE as R
    rng = np.random.default_rng(3)
    pts, ds = H._bowl_points(60e-3, 55e-3, 14, 0.0)
    M = len(ds) - len(ds) % 7
    pts, ds = pts[:M], ds[:M]
    u0 = (rng.normal(size=M) + 1j * rng.normal(size=M)).astype(np.complex64)
    W = _weights(7, 9, seed=6)
    N = 10007
    rf = np.stack([rng.uniform(-40e-3, 40e-3, N), rng.uniform(-40e-3, 40e-3, N), rng.uniform(20e-3, 160e-3, N)], 1).astype(np.float32)
    k = 2 * np.pi * 700e3 / 1500.0
    R.set_devices(None)
    monkeypatch.delenv('BABELFDTD_DEVICES', raising=False)
    calls = (lambda p: R.ForwardSteered(k, pts, ds, M // 7, W, p, u0=u0), lambda p: R.ForwardElements(k, pts, ds, M // 7, p, u0=u0))
    one = [f(rf) for f in calls]
    assert one[0].shape == (9, N) and one[1].shape == (7, N)
    try:
        for f, want in zip(calls, one):
            R.set_devices([0, 0, 0])
            assert np.array_equal(f(rf), want)
            assert R.last_kernel_ms > 0
            assert np.array_equal(f(rf[:50]), want[:, :50])           # too few points to share: one device
            R.set_devices('all')
            assert np.array_equal(f(rf), want)
            nd = torch.cuda.device_count()
            R.set_devices(list(range(nd)) + [nd])                       # one ordinal too many: refused, not skipped
            with pytest.raises(Exception):
                f(rf)
    finally:
        R.set_devices(None)
    monkeypatch.setenv('BABELFDTD_DEVICES', '0,0')
    try:
        for f, want in zip(calls, one):
            assert np.array_equal(f(rf), want)
    finally:
        R.set_devices(None)


# ---- 7. errors through the C ABI ----
def test_c_abi_errors():
    from babelbrain_amd import _engine
    lib = _engine.load_library()
    M, nE, N = 6, 2, 5
    cen = np.arange(3 * M, dtype=np.float32).reshape(M, 3) * 1e-3
    ds = np.full(M, 1e-6, np.float32)
    rf = np.array([[0, 0, 0.1 + 0.01 * i] for i in range(N)], np.float32)
    w = np.ones((nE, 3, 2), np.float32)
    out = np.full((3, N, 2), 7.0, np.float32)
    ms = C.c_double(-1.0)

    def call(es, nSteer, wts, nPts=N, device=0, o=out, cen_=cen):
        es = np.ascontiguousarray(es, np.int64)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        return lib.bfd_rayleigh_forward_elements(device, M, p(cen_), p(ds), None, len(es) - 1, p(es), nSteer, p(wts), 1000.0, 0.0, nPts, p(rf), p(o), C.byref(ms))

    assert call([0, 3, 6], 3, w) == 0 and ms.value > 0 and np.isfinite(out).all() and not (out == 7.0).any()
    for es in ([1, 3, 6], [0, 3, 5], [0, 3, 7], [0, 4, 3, 6]):
        assert call(es, 3 if len(es) == 3 else 0, w if len(es) == 3 else None) == -1, es
        assert b'elemStart' in lib.bfd_last_error()
    assert call([0, 3, 6], 0, w) == -1 and b'weights' in lib.bfd_last_error()
    assert call([0, 3, 6], 3, None) == -1 and b'weights' in lib.bfd_last_error()
    assert call([0, 3, 6], 3, w, cen_=None) == -1 and b'null' in lib.bfd_last_error()
    assert call([0, 3, 6], 3, w, o=None) == -1 and b'null' in lib.bfd_last_error()
    assert call([0, 3, 6], 3, w, device=lib.bfd_device_count()) == -3
    out[:] = 7.0
    assert call([0, 3, 6], 3, w, nPts=0) == 0 and (out == 7.0).all()
    assert call([0, 3, 6], 3, w, nPts=0, o=None) == 0
    # element mode: an empty element gives zeros, sub = NULL is 1
    G = np.full((3, N, 2), 7.0, np.float32)
    assert call([0, 3, 3, 6], 0, None, o=G) == 0
    assert not G[1].any() and np.abs(G[0]).min() > 0 and np.abs(G[2]).min() > 0
