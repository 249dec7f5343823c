"""SeparableSource (babelbrain_amd/sources.py), host side: the meaning of the object (dense()), the CW builders against the
caller's own float64 tables, input checks, and the two new C-ABI entry points."""
import numpy as np
import pytest

from babelbrain_amd import SeparableSource, harness as H, refocus as R

FLT_MIN = np.finfo(np.float32).tiny
F, DT = 500e3, 1 / 500e3 / 13


def _plane(seed=0, n1=20, n2=18, amp=1e5):
    rng = np.random.default_rng(seed)
    p = (rng.normal(size=(n1, n2)) + 1j * rng.normal(size=(n1, n2))) * amp
    p[rng.uniform(size=(n1, n2)) < 0.3] = 0
    return p


def _within_ulps(dense, table, amp, n_ulps=8):
    """|dense - table| <= n_ulps float32 ulps of each row's amplitude"""
    ulp = np.spacing(np.asarray(amp, np.float32)).astype(np.float64)
    err = np.abs(dense - table) / ulp[:, None]
    assert err.max() <= n_ulps, err.max()
    return err.max()


def test_cw_pulse_sources_matches_pulse_sources():
    plane = _plane()
    T = 300 * DT
    smap, pulse = H.pulse_sources(plane, F, DT, T, 10, 3)
    smap2, src = H.cw_pulse_sources(plane, F, DT, T, 10, 3)
    assert isinstance(src, SeparableSource) and src.K == 2
    assert np.array_equal(smap, smap2) and smap2.dtype == np.uint32
    assert src.shape == pulse.shape
    d = src.dense()
    assert d.dtype == np.float64 and d.shape == pulse.shape
    ii, jj = np.where(np.abs(plane) > 0)
    _within_ulps(d, pulse, np.abs(plane[ii, jj]))
    assert src.nbytes < pulse.nbytes / 50


def test_cw_both_ends_matches_punctual_source():
    T = 250 * DT
    p = H.punctual_source(F, DT, T)
    src = SeparableSource.cw(np.ones(1), F, DT, T, ramp_both_ends=True)
    _within_ulps(src.dense(), p, np.ones(1))
    # the K = 1 counterpart holds punctual_source's row rounded once: exactly its float32 form
    k1 = H.punctual_source_separable(F, DT, T)
    assert k1.K == 1 and k1.shape == p.shape
    assert np.array_equal(k1.dense(), p.astype(np.float32).astype(np.float64))
    # DOME-style rows (ramp at both ends) with phases
    u = _plane(1, 6, 5).reshape(-1)
    u = u[np.abs(u) > 0]
    tv = np.arange(0, np.floor(T * F) / F + DT, DT)
    rp = int(np.round(4 / F / DT))
    ramp = (-np.cos(np.arange(0, np.pi, np.pi / rp)) + 1) * 0.5
    ref = np.abs(u)[:, None] * np.sin(2 * np.pi * F * tv[None, :] + np.angle(u)[:, None])
    ref[:, :len(ramp)] *= ramp
    ref[:, -len(ramp):] *= np.flip(ramp)
    _within_ulps(SeparableSource.cw(u, F, DT, T, ramp_both_ends=True).dense(), ref, np.abs(u))


def test_refocus_sources_separable_rows():
    rng = np.random.default_rng(4)
    orig = _plane(2, 16, 16)
    refoc = _plane(3, 16, 16) * (np.abs(orig) > 0)
    refoc[rng.uniform(size=refoc.shape) < 0.1] = 0        # fewer refocused voxels than original ones: rows are cut
    T = 200 * DT
    dense = R.refocus_sources(orig, refoc, F, DT, T)
    src = R.refocus_sources_separable(orig, refoc, F, DT, T)
    assert src.shape == dense.shape
    ii, jj = np.where(np.abs(orig) > 0)
    amp = np.abs(refoc[ii, jj])[:dense.shape[0]]
    amp = np.where(amp > 0, amp, 1.0)
    _within_ulps(src.dense(), dense, amp)


def _ftz(x):
    return np.float32(0) if abs(x) < FLT_MIN else x


def test_dense_is_the_stated_float32_evaluation():
    """K = 3, element by element: acc = w0*s0; acc = acc + w1*s1; acc = acc + w2*s2 in float32, every product and sum flushed"""
    rng = np.random.default_rng(7)
    nS, nT = 7, 9
    w = rng.normal(size=(nS, 3)).astype(np.float32)
    s = rng.normal(size=(3, nT)).astype(np.float32)
    w[0, :] = [1e-20, 3e-20, -2e-20]          # products of ~1e-40: below FLT_MIN
    s[:, 0] = [1e-20, 2e-20, 1e-20]
    w[1, :] = [3e-19, -2.5e-19, 0]            # w0*s0 and w1*s1 are normal, their sum is not
    s[:2, 1] = [1e-19, 1e-19]
    w[2, 2] = 1e-39                           # a denormal input: flushed by the constructor
    src = SeparableSource(w, s)
    assert src.weights[2, 2] == 0
    wf, sf = src.weights, src.signals
    ref = np.zeros((nS, nT))
    flushed = 0
    with np.errstate(under='ignore'):
        for r in range(nS):
            for n in range(nT):
                acc = _ftz(np.float32(wf[r, 0]) * np.float32(sf[0, n]))
                for k in (1, 2):
                    p = _ftz(np.float32(wf[r, k]) * np.float32(sf[k, n]))
                    raw = np.float32(acc + p)
                    flushed += raw != 0 and abs(raw) < FLT_MIN
                    acc = _ftz(raw)
                ref[r, n] = float(acc)
    assert flushed >= 1
    got = src.dense()
    assert np.array_equal(got, ref)
    assert got[0, 0] == 0 and got[1, 1] == 0
    # float64 table of float32 values
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got)


@pytest.mark.parametrize('K', [0, 5])
def test_bad_K(K):
    with pytest.raises(ValueError):
        SeparableSource(np.ones((3, K)), np.ones((K, 10)))


def test_bad_shapes_and_values():
    with pytest.raises(ValueError):
        SeparableSource(np.ones((3, 2)), np.ones((3, 10)))          # K mismatch
    with pytest.raises(ValueError):
        SeparableSource(np.ones(3), np.ones((1, 10)))               # weights not 2-D
    with pytest.raises(ValueError):
        SeparableSource(np.ones((3, 1)), np.ones(10))               # signals not 2-D
    for bad in (np.nan, np.inf, -np.inf, 1e300):                    # 1e300 is not finite in float32
        w = np.ones((3, 2)); w[1, 1] = bad
        with pytest.raises(ValueError):
            SeparableSource(w, np.ones((2, 10)))
        s = np.ones((2, 10)); s[0, 4] = bad
        with pytest.raises(ValueError):
            SeparableSource(np.ones((3, 2)), s)


def test_make_problem_separable_is_opt_in():
    dt_fn = lambda ml, f, h, c: 5e-8  # noqa: E731
    a, k, info = H.make_problem('C2', N=(48, 40, 56), steps=150, stable_dt_fn=dt_fn)
    a2, k2, info2 = H.make_problem('C2', N=(48, 40, 56), steps=150, stable_dt_fn=dt_fn, separable=True)
    assert isinstance(a[4], np.ndarray) and a[4].dtype == np.float64
    assert isinstance(a2[4], SeparableSource) and a2[4].shape == a[4].shape
    assert np.array_equal(a[3], a2[3]) and info['n_sources'] == info2['n_sources']
    # a Z-slab without the source plane: an empty separable table
    a3, _, _ = H.make_problem('C2', N=(48, 40, 56), steps=150, stable_dt_fn=dt_fn, zslab=(28, 28), separable=True)
    assert a3[4].shape[0] == 0 and not a3[3].any()


def test_library_exports_separable_entry_points():
    from babelbrain_amd import _engine
    lib = _engine.load_library()
    for name in ('bfd_set_sources_separable', 'bfd_group_set_sources_separable'):
        assert hasattr(lib, name) and name in _engine.ABI_SYMBOLS
    assert lib.bfd_abi_version() == _engine.ABI_VERSION
