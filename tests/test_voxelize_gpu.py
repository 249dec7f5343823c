"""Device mesh voxelisation (bfd_voxelize_mesh, bfd_voxel_points behind babelbrain_amd.Voxelize) against the numpy restatement of its definition
(tests/voxelize_oracle.py; checked against analytic solids in test_voxelize_host.py): EQUALITY voxel for voxel, for the packed table, the mask and
the count, with nothing left out. Both sides perform the same float64 operations in the same order."""
import numpy as np
import pytest

from babelbrain_amd import BinaryClosing as BC, LabelImage as LI, Voxelize as VX
from tests import voxelize_oracle as VO

pytestmark = pytest.mark.gpu

CUBE = VO.box_triangles((0, 0, 0), (8, 8, 8))
_cases = {}
_reference = {}


def rotated_box(lo, hi, seed):
    return (VO.box_triangles(lo, hi).astype(np.float64) @ VO.rotation(seed).T).astype(np.float32)


def hemisphere():
    """An icosphere's triangles on one side of a plane, without a cap: an open surface."""
    v, f = VO.icosphere(2)
    tri = v[f]
    keep = tri.mean(axis=1)[:, 2] > 0.05
    return ((tri[keep] * 4.0) @ VO.rotation(21).T).astype(np.float32)


def with_degenerates(tri, seed=4):
    """10 % more triangles, none of which the definition counts: zero projected area (two vertices over the same (y, z), x apart) and repeated
    vertices. The signed area of each is 0 exactly, in any arithmetic: its two products have the same factors."""
    rng = np.random.default_rng(seed)
    extra = tri[rng.integers(0, len(tri), max(4, len(tri) // 10))].copy()
    for q, t in enumerate(extra):
        if q % 4 == 0:
            t[2, 1:] = t[1, 1:]                               # v2 over v1: the projection is a segment
        elif q % 4 == 1:
            t[2, 1:] = t[0, 1:]                               # v2 over v0
        elif q % 4 == 2:
            t[1] = t[0]; t[2] = t[0]                          # one point three times
        else:
            t[2] = t[1]                                       # a repeated vertex
    e = extra.astype(np.float64)
    assert np.all((e[:, 1, 1] - e[:, 0, 1]) * (e[:, 2, 2] - e[:, 0, 2]) - (e[:, 2, 1] - e[:, 0, 1]) * (e[:, 1, 2] - e[:, 0, 2]) == 0)
    mixed = np.concatenate([tri, extra])
    return mixed[rng.permutation(len(mixed))]


def case(name):
    """(triangles, min, max, grid), built once"""
    if name in _cases:
        return _cases[name]
    if name.startswith('ico'):
        level, grid = {'ico80': (1, (12, 14, 10)), 'ico320': (2, (20, 24, 18)), 'ico1280': (3, (28, 36, 28)), 'ico5120': (4, (16, 16, 16))}[name]
        tri = VO.ellipsoid_triangles(level, (3.0, 4.0, 2.5), 10 + level)
        c = (tri,) + VO.bounds_of(tri) + (grid,)
    elif name == 'cube':
        c = (CUBE, np.zeros(3), np.full(3, 8.0), (8, 8, 8))
    elif name == 'cube_reversed_flipped':                     # triangle order reversed, every winding flipped
        c = (np.ascontiguousarray(CUBE[::-1, ::-1]), np.zeros(3), np.full(3, 8.0), (8, 8, 8))
    elif name == 'nested':
        c = (np.concatenate([CUBE, VO.box_triangles((2, 2, 2), (6, 6, 6))[:, ::-1]]), np.zeros(3), np.full(3, 8.0), (8, 8, 8))
    elif name == 'offset':
        c = (VO.box_triangles((-3, 1, 2), (5, 9, 6)), np.array([-3.0, 1, 2]), np.array([5.0, 9, 6]), (16, 16, 8))
    elif name == 'box_96_96_8':                               # few triangles, hundreds to thousands of columns each
        tri = rotated_box((-4, -5, -1), (4, 5, 1), 8)
        c = (tri,) + VO.bounds_of(tri) + ((96, 96, 8),)
    elif name == 'box_8_96_96':
        tri = rotated_box((-1, -5, -4), (1, 5, 4), 9)
        c = (tri,) + VO.bounds_of(tri) + ((8, 96, 96),)
    elif name.startswith('gx'):
        tri = rotated_box((-2, -3, -1.5), (2, 3, 1.5), 3)
        c = (tri,) + VO.bounds_of(tri) + ((int(name[2:]), 5, 5),)
    elif name == 'clamped':                                   # the box cuts the mesh: surfaces beyond max_x, below min_x, columns outside in y and z
        c = (VO.ellipsoid_triangles(2, (3.0, 4.0, 2.5), 7), np.array([-1.0, -2.0, -5.0]), np.array([1.5, 6.0, 1.0]), (9, 17, 13))
    elif name == 'hemisphere':
        tri = hemisphere()
        c = (tri,) + VO.bounds_of(tri) + ((22, 19, 23),)
    elif name == 'past_one_sweep':
        # The crossing kernel's launch covers 4096 x 256 = 2^20 (triangle, column) pairs and takes longer ranges in further rounds: the four
        # triangles of this box's two x faces cover about 2^20 columns each, about 2^22 pairs.
        c = (VO.box_triangles((0.6, 0.2, 0.3), (1.9, 1023.7, 1023.6)), np.zeros(3), np.array([2.0, 1024.0, 1024.0]), (2, 1024, 1024))
    elif name == 'two_huge_triangles':                        # an open sheet of two triangles across a 1024 x 1024 x 2 grid
        q = np.array([[300.5, -5, -1], [700.25, 1030, -1], [800.5, 1030, 3], [200.75, -5, 3]], np.float32)
        c = (np.stack([q[[0, 1, 2]], q[[0, 2, 3]]]), np.zeros(3), np.array([1024.0, 1024.0, 2.0]), (1024, 1024, 2))
    else:
        raise KeyError(name)
    _cases[name] = c
    return c


def reference(name, atomics=False):
    """The oracle's mask [gx][gy][gz] (or the number of crossings it issued), computed once per case, read-only."""
    if name not in _reference:
        tri, lo, hi, grid = case(name)
        m, _, issued, _ = VO.voxelize(tri, lo, hi, grid, want_passes=True)
        m.setflags(write=False)
        _reference[name] = (m, issued)
    return _reference[name][1 if atomics else 0]


def device(tri, lo, hi, grid):
    """(table, mask [gx][gy][gz], count) of one call"""
    table, mask, count = VX._run(tri, np.stack([lo, hi]), grid, want_table=True, want_mask=True)
    return table, mask.view(np.bool_).transpose(2, 1, 0), count


def check(name):
    tri, lo, hi, grid = case(name)
    want = reference(name)
    before = tri.copy()
    table, mask, count = device(tri, lo, hi, grid)
    assert np.array_equal(tri, before)
    assert mask.shape == tuple(grid) and count == int(want.sum())
    assert np.count_nonzero(mask != want) == 0
    assert np.array_equal(table, VO.pack_table(want))
    assert VX.last_kernel_ms > 0
    return want


@pytest.mark.parametrize('name', ['ico80', 'ico320', 'ico1280', 'cube', 'nested', 'offset'])
def test_oracle_cases(name):
    want = check(name)
    if name in ('cube', 'nested', 'offset'):
        assert int(want.sum()) == {'cube': 512, 'nested': 448, 'offset': 2048}[name]


def test_top_left_rule():
    """Eight column centres lie on the diagonal of each x face of the cube: exactly one of the two triangles must take each."""
    assert check('cube').all()
    assert check('cube_reversed_flipped').all()


@pytest.mark.parametrize('name', ['box_96_96_8', 'box_8_96_96', 'ico5120'])
def test_load_shapes(name):
    """Few triangles with many columns each; many triangles with 0-1 columns each."""
    want = check(name)
    assert want.any() and not want.all()


@pytest.mark.parametrize('gx', [1, 31, 32, 33, 63, 64, 65, 130])
def test_word_boundaries_of_the_scan(gx):
    assert check('gx%d' % gx).any()


def test_clamping():
    want = check('clamped')
    assert want[0].any() and want[-1].any()                   # the solid reaches both x faces of the box


def test_degenerate_triangles_change_nothing():
    tri, lo, hi, grid = case('ico320')
    mixed = with_degenerates(tri)
    assert len(mixed) > len(tri)
    t0, m0, c0 = device(tri, lo, hi, grid)
    t1, m1, c1 = device(mixed, lo, hi, grid)
    assert np.array_equal(t0, t1) and np.array_equal(m0, m1) and c0 == c1
    assert np.array_equal(m1, reference('ico320')) and np.array_equal(VO.voxelize(mixed, lo, hi, grid), reference('ico320'))


def test_open_mesh():
    want = check('hemisphere')
    assert want.any()


def test_reproducible_and_order_free():
    """Every crossing is one XOR of one bit: the table is the same bytes whatever order the atomics arrive in."""
    tri, lo, hi, grid = case('ico1280')
    first = VX.voxelize_table(tri, np.stack([lo, hi]), grid)
    for _ in range(2):
        assert first.tobytes() == VX.voxelize_table(tri, np.stack([lo, hi]), grid).tobytes()
    perm = np.random.default_rng(5).permutation(len(tri))
    assert first.tobytes() == VX.voxelize_table(tri[perm], np.stack([lo, hi]), grid).tobytes()
    assert first.tobytes() == VX.voxelize_table(np.roll(tri, 1, axis=1)[::-1], np.stack([lo, hi]), grid).tobytes()
    assert np.array_equal(first, VO.pack_table(reference('ico1280')))


@pytest.mark.parametrize('name', ['past_one_sweep', 'two_huge_triangles'])
def test_past_one_launch(name):
    want = check(name)
    if name == 'past_one_sweep':
        assert reference(name, atomics=True) > 2 ** 20        # more pairs pass than one sweep holds, let alone are looked at
    assert want.any() and not want.all()


# ---------------------------------------------------------------- points ----------------------------------------------------------------

@pytest.mark.parametrize('name', ['ico320', 'clamped', 'gx33'])
def test_points_in_index_order(name):
    tri, lo, hi, grid = case(name)
    want = reference(name)
    unit = VO.unit_of(lo, hi, grid)
    pts = VX.voxel_points(VO.pack_table(want), grid, lo, unit)
    ref = VO.points_of(want, lo, unit)
    assert pts.dtype == np.float32 and pts.shape == ref.shape
    assert np.array_equal(pts, ref)
    assert VX.last_kernel_ms > 0


def test_points_capacity_and_edge_tables():
    import ctypes as C
    from babelbrain_amd import _engine
    lib = _engine.load_library()
    P = _engine._ptr
    _, lo, hi, grid = case('ico80')
    want = reference('ico80')
    table, unit, n = VO.pack_table(want), VO.unit_of(lo, hi, grid), int(want.sum())
    cnt = C.c_int64(-1)
    short = np.full((n - 1, 3), -7.0, np.float32)
    rc = lib.bfd_voxel_points(0, P(table), grid[0], grid[1], grid[2], P(lo), P(unit), P(short), n - 1, C.byref(cnt), None)
    assert rc == -1 and cnt.value == n and np.all(short == -7.0)
    # an empty table
    assert VX.voxel_points(np.zeros_like(table), grid, lo, unit).shape == (0, 3)
    # every bit set, the padding of the partial last word included: 7 x 5 x 3 = 105 voxels in four words
    g = (7, 5, 3)
    pts = VX.voxel_points(np.full(4, 0xFFFFFFFF, np.uint32), g, (1.0, 2.0, 3.0), (0.5, 0.25, 2.0))
    assert np.array_equal(pts, VO.points_of(np.ones(g, bool), (1.0, 2.0, 3.0), (0.5, 0.25, 2.0)))
    # the device's own table of the full cube: 512 voxels, no padding
    assert np.array_equal(VX.voxelize_table(CUBE, [[0, 0, 0], [8, 8, 8]], (8, 8, 8)), np.full(16, 0xFFFFFFFF, np.uint32))


class DuckMesh:
    class _BB:
        pass

    def __init__(self, triangles, bounds):
        self.triangles = triangles
        self.bounding_box = DuckMesh._BB()
        self.bounding_box.bounds = bounds


def test_voxelize_end_to_end():
    tri = VO.ellipsoid_triangles(3, (30.0, 40.0, 25.0), 13, centre=(5.0, -7.0, 11.0))
    lo, hi = VO.bounds_of(tri)
    mesh = DuckMesh(tri.astype(np.float64), np.stack([lo, hi]))
    res = 2.5
    pts = VX.Voxelize(mesh, res, GPUBackend='OpenCL')
    grid, unit = VX.grid_rule(np.stack([lo, hi]), res)
    want = VO.voxelize(tri, lo, hi, grid)
    assert pts.dtype == np.float32 and pts.shape == (int(want.sum()), 3)
    assert np.all(pts >= lo) and np.all(pts <= hi)
    assert np.array_equal(pts, VO.points_of(want, lo, unit))
    assert VX.voxelize_count(tri, np.stack([lo, hi]), grid) == pts.shape[0]
    # the same without a bounding_box attribute, and from a bare array
    assert np.array_equal(VX.Voxelize(tri, res), pts)


def test_chain_with_closing_and_largest_component():
    """voxelize_mask -> BinaryClose -> largest_component, as Step 1 strings them, against scipy on the oracle's mask."""
    ndi = pytest.importorskip('scipy.ndimage')
    big = VO.ellipsoid_triangles(2, (9.0, 9.0, 9.0), 2)
    small = VO.ellipsoid_triangles(1, (2.0, 2.0, 2.0), 3, centre=(14.0, 13.0, 12.0))
    tri = np.concatenate([big, small])
    lo, hi = VO.bounds_of(tri)
    grid = (34, 32, 30)
    st = np.ones((3, 3, 3), int)
    got = LI.largest_component(BC.BinaryClose(VX.voxelize_mask(tri, np.stack([lo, hi]), grid), st))
    m = ndi.binary_closing(VO.voxelize(tri, lo, hi, grid), structure=st)
    lab, n = ndi.label(m, ndi.generate_binary_structure(3, 3))
    assert n == 2
    sizes = np.bincount(lab.ravel())[1:]
    want = lab == (n - int(np.argmax(sizes[::-1])))
    assert got.shape == want.shape and np.array_equal(got, want) and want.any()
