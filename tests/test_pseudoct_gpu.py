"""The pseudo-CT on the device: the six entries and PseudoCT.convert_pseudo_ct equal their numpy / scipy restatements (tests/pseudoct_oracle.py)
element for element, dtype and shape included, for float32 and float64 volumes."""
import numpy as np
import pytest

from babelbrain_amd import LabelImage as LI, PseudoCT as PC
from tests import pseudoct_oracle as PO

pytestmark = pytest.mark.gpu

N3S = (1, 31, 32, 33, 63, 64, 65, 130)
SHAPES = [(3, 5, n3) for n3 in N3S] + [(1, 1, 1), (3, 70, 2), (9, 17, 130)]
DTYPES = (np.float32, np.float64)


def same(got, want, what=''):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()))


def mri(shape, seed, dtype, share=0.6, integers=True):
    """An MRI-like volume: `share` of the voxels are one value (0, the background), the rest spread over tissue levels, some negative"""
    rng = np.random.default_rng(seed)
    v = rng.normal(900, 400, shape)
    v[rng.random(shape) < 0.1] -= 1500
    if integers:
        v = np.round(v)
    else:
        v = np.round(v * 8) / 8 + 0.0625                          # exact in float32, never on an integer
    v[rng.random(shape) < share] = 0
    return v.astype(dtype)


def masks(shape, seed):
    rng = np.random.default_rng(seed + 1000)
    head = rng.random(shape) > 0.15
    eroded = head & (rng.random(shape) > 0.3)
    return dict(head=head, eroded=eroded, bone=rng.random(shape) > 0.5, skin=(rng.random(shape) > 0.2).astype(np.float32),
                cavities=(rng.random(shape) > 0.9).astype(np.int16), csf=rng.random(shape) > 0.4)


def check_integer_histogram(v, what=''):
    counts, first, (mn, mx) = PC.integer_histogram(v)
    want, edges = PO.integer_histogram(v)
    same(counts, want, what)
    w = np.asarray(v, np.float64)
    assert first == int(w.min()) and isinstance(first, int) and (mn, mx) == (w.min(), w.max()), what
    assert PC.last_kernel_ms > 0
    return counts


def check_percentile(v, mask, q, above, what=''):
    got = PC.masked_percentile(v, mask, q, above)
    want = PO.masked_percentile(v, mask, q, above)
    assert type(got) is type(want) and got == want, (what, q, above, got, want)


def check_order(v, mask, above, inclusive, ranks, what=''):
    w = np.asarray(v, np.float64)
    sel = (np.ones(w.shape, bool) if mask is None else np.asarray(mask) != 0) & (w >= above if inclusive else w > above)
    s = np.sort(w[sel])
    n, used, stats = PC.order_statistics(v, mask, above, inclusive, ranks=ranks)
    assert n == s.size and list(used) == list(ranks), what
    same(stats, s[list(ranks)], what)


def check_uniform(v, bins, above, inclusive, what=''):
    counts, edges = PC.uniform_histogram(v, bins, above, inclusive)
    want, wedges = PO.uniform_histogram(v, bins, above, inclusive)
    same(edges, wedges, what)
    same(counts, want, what)


def check_candidates(v, divisor, head, eroded, lo, hi, what=''):
    mask, mx, n = PC.candidates(v, divisor, head, eroded, lo, hi)
    want, wmx = PO.candidates(v, divisor, head, eroded, lo, hi)
    same(mask, want, what)
    assert mx == wmx and n == int(want.sum()), what
    return mask, mx


def check_hounsfield(v, divisor, head, m, slope, offset, what=''):
    want = PO.hounsfield(v, divisor, head, m['bone'], m['skin'], m['cavities'], slope, offset)
    for dt in DTYPES:
        same(PC.hounsfield(v, divisor, head, m['bone'], m['skin'], m['cavities'], slope, offset, dt), want.astype(dt), (what, dt))
    return want


def largest(x, ties):
    lab = PO.label(x)
    sizes = np.bincount(lab.ravel())[1:]
    if sizes.size == 0:
        return np.zeros(x.shape, bool)
    first = int(np.argmax(sizes))
    last = sizes.size - 1 - int(np.argmax(sizes[::-1]))
    return lab == (first if ties == 'first' else last) + 1


# ---------------------------------------------------------------- every entry, every shape ----------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_every_entry_at_row_lengths_and_shapes(shape, dtype):
    seed = sum(shape)
    v = mri(shape, seed, dtype)
    v.flat[0] = 700                                               # one voxel beyond every threshold below, under every mask
    m = masks(shape, seed)
    for k in ('head', 'eroded', 'csf'):
        m[k].flat[0] = True
    check_integer_histogram(v, shape)
    w = mri(shape, seed, dtype, integers=False)
    check_integer_histogram(w, shape)
    for q in (0, 50, 95, 100):
        check_percentile(w, m['csf'], q, -500.0, shape)
    n = int(((m['csf'] != 0) & (np.asarray(v, np.float64) > -500)).sum())
    check_order(v, m['csf'], -500.0, False, sorted({0, n // 3, n // 2, n - 1}), shape)
    check_order(w, None, -np.inf, True, [v.size - 1], shape)
    for inclusive in (False, True):
        check_uniform(w, 15, 200.0, inclusive, shape)
        check_uniform(v, 30, 200.0, inclusive, shape)
    for head in (m['head'], None):
        check_candidates(w, 1500.0, head, m['eroded'], 0.1, 0.6, shape)
        check_hounsfield(w, 1500.0, head, m, -2085.0, 2329.0, shape)
    x = m['bone']
    for ties in ('first', 'last'):
        same(LI.largest_component(x, ties=ties), largest(x, ties), (shape, ties))
    same(LI.largest_component(x), largest(x, 'last'), shape)


# ---------------------------------------------------------------- integer histogram ----------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
def test_integer_histogram_edge_volumes(dtype):
    shape = (7, 9, 65)
    one = np.full(shape, -37.5, dtype)
    assert list(check_integer_histogram(one)) == [one.size]
    two = one.copy()
    two[::2, 1::3, ::5] = 2200.25
    check_integer_histogram(two)
    # truncation toward zero: the bin of 0 collects (-1, 1)
    t = np.zeros(shape, dtype)
    t.flat[:8] = [-0.9, -0.0, 0.9, -1.0, 1.0, 1.9, -1.5, 0.5]
    c = check_integer_histogram(t)
    assert c[1] == t.size - 4 and PC.integer_histogram(t)[1] == -1
    # a range of exactly 65535 passes, with 65536 bins where min and max are integers; 65536 is refused
    rng = np.random.default_rng(7)
    wide = rng.integers(-30000, 35535, shape).astype(dtype)
    wide.flat[0], wide.flat[-1] = -30000, 35535
    c = check_integer_histogram(wide)
    assert c.size == 65536
    for lowest, highest in ((-30000, 35536), (-30000.5, 35535.5 + 2.0 ** -7)):
        wide.flat[0], wide.flat[-1] = lowest, highest
        with pytest.raises(ValueError, match=r'^The range of values in the ZTE file exceeds 2\^16$'):
            PC.integer_histogram(wide)
        with pytest.raises(ValueError, match='exceeds'):
            PO.integer_histogram(wide)
    wide.flat[0], wide.flat[-1] = -65535, 0
    check_integer_histogram(wide.clip(-65535, 0))
    wide.flat[0], wide.flat[-1] = -0.5, 65534.5                   # range 65535, the minimum truncates to 0
    assert check_integer_histogram(wide.clip(-0.5, 65534.5)).size == 65535


@pytest.mark.parametrize('dtype', DTYPES)
def test_integer_histogram_on_both_sides_of_the_lds_window(dtype):
    """The first PC.INT_WINDOW bins are counted in LDS, the rest in global memory: values on both sides of the switch, the last bin inside and
    the first outside it, hot values on either side, and a negative minimum so that the window does not start at 0"""
    W = PC.INT_WINDOW
    rng = np.random.default_rng(8)
    shape = (9, 17, 130)
    first = -123
    v = (first + rng.integers(0, 3 * W, shape)).astype(dtype)
    hot = rng.random(shape)
    v[hot < 0.3] = first + W - 1                                  # the last bin of the window
    v[(hot >= 0.3) & (hot < 0.6)] = first + W                     # the first bin beyond it
    v[(hot >= 0.6) & (hot < 0.65)] = first + 2 * W + 0.75
    v.flat[0] = first
    c = check_integer_histogram(v)
    assert c[W - 1] > 0.25 * v.size and c[W] > 0.25 * v.size and c[:W].sum() and c[W + 1:].sum()
    exactly = (first + rng.integers(0, W, shape)).astype(dtype)   # a range that fills the window and no more
    exactly.flat[:2] = [first, first + W - 1]
    assert check_integer_histogram(exactly).size == W
    exactly.flat[1] = first + W
    assert check_integer_histogram(exactly).size == W + 1


def test_integer_histogram_repeats_are_byte_identical():
    v = mri((9, 17, 130), 9, np.float32)
    v[v != 0] += 9000                                             # beyond the window too
    a, b = PC.integer_histogram(v), PC.integer_histogram(v)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]


@pytest.mark.parametrize('dtype', DTYPES)
def test_integer_histogram_beyond_one_sweep(dtype):
    """More voxels than one sweep of the histogram's launch (PC.HIST_SWEEP_VOXELS) and of the reduction's (PC.SWEEP_VOXELS): the grid-stride loops
    turn; 60 % of the volume is one value"""
    n = max(PC.HIST_SWEEP_VOXELS, PC.SWEEP_VOXELS)
    shape = (5, 512, n // (4 * 512) + 3)
    assert shape[0] * shape[1] * shape[2] > n and shape[0] * shape[1] * shape[2] <= 2 ** 26
    v = mri(shape, 10, dtype)
    v.flat[-1] = 12345                                            # beyond the window, in the last quad
    c = check_integer_histogram(v)
    assert c[int(0 - np.asarray(v, np.float64).min())] > 0.55 * v.size


# ---------------------------------------------------------------- order statistics ----------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
def test_order_statistics_edge_selections(dtype):
    shape = (5, 6, 33)
    rng = np.random.default_rng(11)
    every = np.ones(shape, bool)
    equal = np.full(shape, 3.25, dtype)
    for q in (0, 50, 95, 100):
        check_percentile(equal, every, q, -500.0)
    check_order(equal, None, 0.0, False, [0, 1, equal.size // 2, equal.size - 1])
    # duplicates straddling the rank: ten distinct values, each a tenth of the volume
    dup = rng.integers(0, 10, shape).astype(dtype) * 7 - 20
    n = dup.size
    check_order(dup, None, -np.inf, True, [n // 10 - 1, n // 10, n // 2, n - 1])
    for q in (0, 10, 50, 90, 95, 99.9, 100):
        check_percentile(dup, every, q, -500.0)
    # n = 1 and n = 2, by the mask
    v = rng.normal(0, 50, shape).astype(dtype)
    one = np.zeros(shape, np.uint8)
    one[2, 3, 17] = 5
    two = one.copy()
    two[4, 5, 32] = 1
    for q in (0, 37, 50, 95, 100):
        check_percentile(v, one, q, -500.0)
        check_percentile(v, two, q, -500.0)
    check_order(v, one, -500.0, False, [0])
    check_order(v, two, -500.0, False, [0, 1])
    # +-0.0 and mixed signs: -0.0 == 0.0, so a threshold of 0 leaves both out and >= 0 keeps both
    z = rng.normal(0, 2, shape).astype(dtype)
    z[::2] = 0.0
    z[1::4] = -0.0
    n = z.size
    check_order(z, None, -np.inf, True, [0, n // 3, n // 2, n - 1])
    check_order(z, None, 0.0, False, [0])
    check_order(z, None, 0.0, True, [0, n // 3])
    check_order(z, None, -0.0, True, [0, n // 3])
    for q in (0, 25, 50, 75, 100):
        check_percentile(z, every, q, -500.0)
        check_percentile(z, every, q, 0.0)
    # the threshold equal to a value
    t = np.sort(np.asarray(v, np.float64).ravel())[v.size // 2]
    check_order(v, None, t, False, [0])
    check_order(v, None, t, True, [0])
    assert PC.order_statistics(v, None, t, True, ranks=[0])[0] == PC.order_statistics(v, None, t, False, ranks=[0])[0] + 1
    check_percentile(v, every, 95, t)
    # an all-zero mask, and a threshold beyond every value
    for mask, above in ((np.zeros(shape), -500.0), (every, 1e9)):
        with pytest.raises(ValueError, match='no voxel is selected'):
            PC.masked_percentile(v, mask, 95, above)
    # NaNs are never selected, as in numpy's comparison
    v[1, 2, 3] = np.nan
    check_order(v, None, -np.inf, True, [0, v.size - 2])


def test_order_statistics_float32_denormals():
    """The build flushes float32 denormals in float32 instructions; the selection and the keys are formed from the bits"""
    rng = np.random.default_rng(12)
    shape = (4, 5, 65)
    tiny = np.float32(1e-45)
    v = (rng.integers(-40, 40, shape) * tiny).astype(np.float32)
    assert np.count_nonzero(v) > 0.9 * v.size and np.abs(v).max() < np.finfo(np.float32).tiny
    n = v.size
    check_order(v, None, -np.inf, True, [0, n // 2, n - 2, n - 1])
    check_order(v, None, 0.0, False, [0, 1])                       # the smallest positive denormals, not zero
    check_order(v, None, float(5 * tiny), False, [0])
    check_order(v, None, float(5 * tiny), True, [0])
    for q in (0, 50, 95, 100):
        check_percentile(v, np.ones(shape, bool), q, 0.0)
        check_percentile(v, np.ones(shape, bool), q, -500.0)
    d = (rng.integers(-40, 40, shape) * 5e-324)
    check_order(d, None, 0.0, False, [0, 1])
    check_percentile(d, np.ones(shape, bool), 95, -500.0)


# ---------------------------------------------------------------- uniform histogram ----------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('bins', [15, 30, 1024])
def test_uniform_histogram_values_on_edges(bins, dtype):
    rng = np.random.default_rng(bins)
    shape = (6, 11, 65)
    v = mri(shape, bins, dtype, integers=False)
    lo, hi = 256.0, 256.0 + 4 * bins                              # edges that are exact in both formats
    v = np.clip(v, -2000, hi).astype(dtype)
    edges = np.linspace(lo, hi, bins + 1)
    idx = rng.choice(v.size, 3 * (bins + 1), replace=False)
    v.flat[idx[:bins + 1]] = edges
    v.flat[idx[bins + 1:2 * (bins + 1)]] = np.nextafter(edges.astype(dtype), dtype(np.inf))
    v.flat[idx[2 * (bins + 1):]] = np.nextafter(edges.astype(dtype), dtype(-np.inf))
    for inclusive in (False, True):
        check_uniform(v, bins, lo, inclusive, (bins, inclusive))         # the threshold is a value: > drops the first edge, >= keeps it
        check_uniform(v, bins, -2500.0, inclusive, (bins, inclusive))
    assert PO.uniform_histogram(v, bins, lo, True)[1][0] == lo and PO.uniform_histogram(v, bins, lo, False)[1][0] > lo


@pytest.mark.parametrize('dtype', DTYPES)
def test_uniform_histogram_one_value_and_none(dtype):
    v = mri((3, 7, 33), 13, dtype)
    top = float(np.asarray(v, np.float64).max())
    for bins in (15, 30):
        check_uniform(v, bins, top, True, 'one value')                  # min == max: the interval is +-0.5
        check_uniform(v, bins, top, False, 'none')                      # nothing selected: numpy's 0 .. 1
        check_uniform(np.full((2, 3, 4), 7.5, dtype), bins, 0.0, False, 'all equal')
    counts, edges = PC.uniform_histogram(v, 15, top, True)
    assert counts.sum() == (v == top).sum() and edges[0] == top - 0.5 and edges[-1] == top + 0.5


# ---------------------------------------------------------------- largest component ----------------------------------------------------------------

def test_largest_component_ties_across_label_tiles():
    x = np.zeros((9, 17, 130), bool)
    x[1:3, 1:3, 2:5] = True                                       # 12 voxels in the first tile: label 1
    x[6, 12, 70] = True                                           # a single voxel: label 2
    x[7:9, 14:16, 126:129] = True                                 # 12 voxels in the last tile along k: label 3
    x[4, 8, 60:68] = True                                         # 8 voxels across a tile face
    first, last = LI.largest_component(x, ties='first'), LI.largest_component(x, ties='last')
    same(first, largest(x, 'first'))
    same(last, largest(x, 'last'))
    assert first[1, 1, 2] and not first[7, 14, 126] and last[7, 14, 126] and not last[1, 1, 2] and first.sum() == last.sum() == 12
    assert LI.last_component is not None
    LI.largest_component(x, ties='first')
    assert LI.last_component == (4, 12)
    same(LI.largest_component(x), last)                           # the default is unchanged
    one = np.zeros((3, 70, 2), bool)
    one[2, 69, 1] = True
    for ties in ('first', 'last'):
        same(LI.largest_component(one, ties=ties), one)
        same(LI.largest_component(np.zeros((3, 4, 5), bool), ties=ties), np.zeros((3, 4, 5), bool))
    rng = np.random.default_rng(14)
    for conn in (1, 2, 3):
        r = rng.random((8, 9, 70)) > 0.8
        lab = __import__('scipy.ndimage').ndimage.label(r, __import__('scipy.ndimage').ndimage.generate_binary_structure(3, conn))[0]
        sizes = np.bincount(lab.ravel())[1:]
        same(LI.largest_component(r, connectivity=conn, ties='first'), lab == int(np.argmax(sizes)) + 1, conn)
        same(LI.largest_component(r, connectivity=conn), lab == sizes.size - int(np.argmax(sizes[::-1])), conn)


# ---------------------------------------------------------------- candidates and conversion ----------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
def test_candidates_with_the_maximum_inside_and_outside_the_range(dtype):
    shape = (6, 9, 65)
    v = np.abs(mri(shape, 15, dtype, share=0.2, integers=False))
    m = masks(shape, 15)
    top = float(np.asarray(v, np.float64).max())
    for head in (m['head'], None):
        inside, mx = check_candidates(v, top / 0.5, head, m['eroded'], 0.1, 0.6)      # the maximum is 0.5 (with a head: where the head is)
        outside, _ = check_candidates(v, top, head, m['eroded'], 0.1, 0.6)            # the maximum is 1
        assert 0.1 <= mx <= 0.6 and inside[~m['eroded']].all() and not outside[~m['eroded']].any()
        check_candidates(v, top, head, m['eroded'], 1.0, 1.0)                         # lo == hi == the maximum
        check_candidates(v, -top, head, m['eroded'], -0.6, -0.1)                      # a negative divisor: with a head the maximum is -0.0 or -0.5
    # the whole head eroded away, and none of it
    check_candidates(v, top, m['head'], np.zeros(shape, bool), 0.1, 0.6)
    check_candidates(v, top, None, np.ones(shape, bool), 0.1, 0.6)


@pytest.mark.parametrize('dtype', DTYPES)
def test_hounsfield_on_and_one_step_beyond_the_limits(dtype):
    """-1000 and 3300 are kept, the next value beyond either becomes -1000: quotients that land on them and to either side, with the divisor 1
    (exact in both formats only for float64; for float32 the volume holds the quotients' float32 roundings and the oracle sees the same)"""
    shape = (4, 7, 65)
    m = masks(shape, 16)
    rng = np.random.default_rng(16)
    for slope, offset in ((-2085.0, 2329.0), (-2080.02235771, 2133.22867303), (1.0, 0.0), (-0.5, 100.0)):
        edge = PO.hu_edge_quotients(slope, offset)
        v = rng.uniform(-1, 2, shape) * (1.0 if abs(slope) > 1 else 3000.0)
        idx = rng.choice(v.size, edge.size, replace=False)
        v.flat[idx] = edge
        v = v.astype(dtype)
        m['bone'].flat[idx] = True
        m['cavities'].flat[idx] = 0
        for head in (None, m['head']):
            want = check_hounsfield(v, 1.0, head, m, slope, offset, (slope, head is None))
        if dtype == np.float64:
            got = want.flat[idx]
            assert (got == 3300.0).any() and (got == -1000.0).any() and got.max() == 3300.0 and ((got > 3299.0) & (got < 3300.0)).any()
        check_hounsfield(v, 0.37, m['head'], m, slope, offset, slope)
    v[0, 0, :3] = [np.nan, np.inf, -np.inf]                        # under the bone region a NaN stays, as in numpy; the infinities become air
    m['bone'][0, 0, :3], m['cavities'][0, 0, :3] = True, 0
    want = PO.hounsfield(v, 1.0, None, m['bone'], m['skin'], m['cavities'], 2.0, 1.0)
    got = PC.hounsfield(v, 1.0, None, m['bone'], m['skin'], m['cavities'], 2.0, 1.0)
    assert np.isnan(got[0, 0, 0]) and got[0, 0, 1] == got[0, 0, 2] == -1000.0 and np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize('dtype', DTYPES)
def test_hounsfield_beyond_one_sweep(dtype):
    """More voxels than one sweep of the launch (PC.SWEEP_VOXELS): the grid-stride loop turns"""
    shape = (9, 512, PC.SWEEP_VOXELS // (8 * 512) + 1)
    n = shape[0] * shape[1] * shape[2]
    assert PC.SWEEP_VOXELS < n <= 2 ** 26
    rng = np.random.default_rng(17)
    v = rng.uniform(0, 1500, shape).astype(dtype)
    bits = rng.integers(0, 16, shape, dtype=np.uint8)
    m = dict(head=bits & 1, bone=bits & 2, skin=bits & 4, cavities=(bits & 8) & (bits >> 1))
    want = PO.hounsfield(v, 960.5, m['head'], m['bone'], m['skin'], m['cavities'], -2085.0, 2329.0)
    same(PC.hounsfield(v, 960.5, m['head'], m['bone'], m['skin'], m['cavities'], -2085.0, 2329.0), want)
    same(PC.hounsfield(v, 960.5, None, m['bone'], m['skin'], m['cavities'], -2085.0, 2329.0, np.float32),
         PO.hounsfield(v, 960.5, None, m['bone'], m['skin'], m['cavities'], -2085.0, 2329.0).astype(np.float32))
    eroded = (bits & 1) & (bits >> 2)
    check_candidates(v, 960.5, m['head'], eroded, 0.1, 0.6)


# ---------------------------------------------------------------- the flow ----------------------------------------------------------------

@pytest.fixture(scope='module')
def flows():
    """The oracle's flow on the phantom, once per kind of volume"""
    out = {}
    for petra in (False, True):
        for dtype in DTYPES:
            p = PO.phantom(petra=petra, dtype=dtype)
            out[petra, dtype] = (p, PO.convert(p['zte'], p['head'], p['skin'], p['cavities'], p['csf'], bIsPetra=petra))
    return out


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('petra', [False, True])
def test_convert_pseudo_ct_equals_the_oracle_s_flow(flows, petra, dtype):
    p, (want, wparts) = flows[petra, dtype]
    before = p['zte'].copy()
    got, parts = PC.convert_pseudo_ct(p['zte'], p['head'], p['skin'], p['cavities'], None if petra else p['csf'], petra=petra, return_parts=True)
    same(got, want)
    assert parts['normaliser'] == wparts['normaliser'] and parts['maximum'] == wparts['maximum'] and isinstance(parts['normaliser'], float)
    for k in ('candidates', 'bone_before_closing', 'bone'):
        same(parts[k], wparts[k], k)
    assert np.array_equal(p['zte'], before) and PC.last_kernel_ms > 0 and set(PC.last_parts_ms) >= {'normaliser', 'closing', 'hounsfield'}
    same(PC.convert_pseudo_ct(p['zte'], p['head'], p['skin'], p['cavities'], p['csf'], petra=petra, dtype=np.float32), want.astype(np.float32))
    # other slopes, another range, and PETRA's other arguments
    kw = dict(slope=-1900.0, offset=2100.5, pct_range=(0.2, 0.5))
    other, _ = PO.convert(p['zte'], p['head'], p['skin'], p['cavities'], p['csf'], bIsPetra=petra, slope=-1900.0, offset=2100.5, pseudo_CT_range=(0.2, 0.5))
    same(PC.convert_pseudo_ct(p['zte'], p['head'], p['skin'], p['cavities'], p['csf'], petra=petra, **kw), other)
    assert not np.array_equal(other, want)
    if petra:
        assert PC.petra_normaliser(p['zte']) == PO.petra_normaliser(p['zte']) == 1800.0
        for distance, peaks in ((5, 3), (400, 1), (1, 4)):
            assert PC.petra_normaliser(p['zte'], distance, peaks) == PO.petra_normaliser(p['zte'], distance, peaks)
    else:
        assert PC.masked_percentile(p['zte'], p['csf']) == PO.zte_cutoff(p['zte'], p['csf'])


def test_convert_pseudo_ct_refusals(flows):
    p, _ = flows[False, np.float64]
    a = (p['head'], p['skin'], p['cavities'], p['csf'])
    with pytest.raises(ValueError, match='no voxel of the normalised volume'):
        PC.convert_pseudo_ct(p['zte'], *a, pct_range=(5.0, 6.0))
    with pytest.raises(ValueError, match='finite and positive'):
        PC.convert_pseudo_ct(-np.abs(p['zte']) / 10 - 1, *a)                  # beyond -500, below 0
    with pytest.raises(ValueError, match='no voxel is selected'):
        PC.convert_pseudo_ct(p['zte'], p['head'], p['skin'], p['cavities'], np.zeros_like(p['csf']))
    flat = np.zeros_like(p['zte'])
    with pytest.raises(ValueError, match='fewer than two bins'):
        PC.convert_pseudo_ct(flat, *a, petra=True)


def test_charm_masks_equal_the_oracle():
    rng = np.random.default_rng(18)
    c = np.zeros((12, 20, 70))
    c[2:10, 3:17, 4:66] = rng.choice([1, 2, 3, 4, 5, 9, 10], (8, 14, 62))
    c[4:6, 5:8, 10:14] = 0                                        # cavities inside
    c[7, 12, 40:66] = 0                                           # a channel open to the outside: part of the background
    c[8, 4, 30] = 0
    for data in (c, c.astype(np.float32), c.astype(np.int16)):
        got, want = PC.charm_masks(data), PO.charm_masks(data)
        for g, w in zip(got, want):
            same(g, w)
    assert got[2].sum() == 2 * 3 * 4 + 1 and not got[2][7, 12, 50]
