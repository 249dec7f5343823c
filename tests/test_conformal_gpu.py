"""The conformal-mask scatter on the device (bfd_voxel_scatter3d, bfd_voxelize_scatter3d behind babelbrain_amd.ConformalMask) against the numpy
restatement of its definition (tests/conformal_oracle.py; held to the reference's np.dot expression in test_conformal_host.py): EQUALITY, for the
volume voxel for voxel, for lo and hi, and for all four counts. Both sides perform the same float32 operations in the same order."""
import numpy as np
import pytest

from babelbrain_amd import BinaryClosing as BC, ConformalMask as CM, LabelImage as LI, Voxelize as VX, _engine
from tests import conformal_calls as CC, conformal_oracle as CO, voxelize_oracle as VO

pytestmark = pytest.mark.gpu

GX = [1, 31, 32, 33, 63, 64, 65, 130]
ORIGIN, UNIT = (-3.25, 1.5, 0.125), (0.75, 0.7, 0.8)


def device_table(table, grid, origin, unit, m, shape):
    """(out, lo, hi, counts) of bfd_voxel_scatter3d; shape None: the bounds pass. Below-points are reported, not raised."""
    return CM._run(CM._source(np.asarray(table), None, None, grid, origin, unit), CM._matrix(m), shape, True)


def device_mesh(tri, lo, hi, grid, m, shape):
    return CM._run(CM._source(tri, None, np.stack([lo, hi]), grid, None, None), CM._matrix(m), shape, True)


def check_table(table, grid, origin, unit, m, shape, what=''):
    pts = CO.table_points(table, grid, origin, unit)
    want = CO.scatter(pts, m, shape)
    before = table.copy()
    got = device_table(table, grid, origin, unit, m, shape)
    assert np.array_equal(table, before)
    CO.agree(got, want, what)
    CO.agree(device_table(table, grid, origin, unit, m, None), CO.scatter(pts, m, None), what)         # the bounds pass: counts[1..3] are 0
    return want


def full_table(grid):
    return np.full((grid[0] * grid[1] * grid[2] + 31) // 32, 0xFFFFFFFF, np.uint32)          # the padding bits too


def last_voxel_table(grid):
    n = grid[0] * grid[1] * grid[2]
    t = np.zeros((n + 31) // 32, np.uint32)
    t[-1] = np.uint32(1) << np.uint32(31 - (n - 1) % 32)
    return t


# ---------------------------------------------------------------- tables ----------------------------------------------------------------

@pytest.mark.parametrize('gx', GX)
def test_rows_across_words_and_waves(gx):
    """Rows of gx voxels straddle the table's 32-bit words and the 64 lanes of a wave; the padding bits of the last word hold garbage."""
    grid = (gx, 5, 3)
    reach = int(gx * 0.75) + 6                                 # no point lies further than this from the grid's origin
    m = CO.rotated_about(4, 1.0, ORIGIN, (reach, reach, reach))
    shape = (2 * reach + 1,) * 3
    want = check_table(CO.random_table(grid, gx), grid, ORIGIN, UNIT, m, shape, 'random')
    assert want[3][0] > 0 and want[0].any() and want[3][1] == 0 and want[3][3] == 0           # the volume holds every point
    full = check_table(full_table(grid), grid, ORIGIN, UNIT, m, shape, 'full')
    assert full[3][0] == gx * 15
    one = check_table(last_voxel_table(grid), grid, ORIGIN, UNIT, m, shape, 'last')
    assert one[3][0] == 1 and np.array_equal(one[1], one[2])


def _perm_matrix(perm, signs, scale, offset):
    m = np.zeros((3, 4), np.float32)
    for a in range(3):
        m[a, perm[a]] = signs[a] * scale
        m[a, 3] = offset[a]
    return m


PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


@pytest.mark.parametrize('q', range(6))
def test_axis_permutations_with_sign_flips(q):
    """The source i axis lands on each output axis, forwards and backwards; the negative directions go through numpy's wrap."""
    grid = (70, 5, 3)
    signs = [(1, -1, 1), (-1, 1, 1), (1, 1, -1), (-1, -1, 1), (1, -1, -1), (-1, 1, -1)][q]
    m = _perm_matrix(PERMS[q], signs, 1.0, (0.25, -0.25, 0.5))
    ext = [0, 0, 0]
    for a in range(3):
        ext[a] = grid[PERMS[q][a]] + 2
    table = CO.random_table(grid, 20 + q, 0.7)
    want = check_table(table, grid, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), m, tuple(ext), (PERMS[q], signs))
    assert want[3][2] > 0 and want[3][3] == 0 and want[3][1] == 0            # wrapped, nothing dropped
    assert int(want[0].sum()) == want[3][0]                                   # a permutation: one voxel per point


def test_scaled_identity_takes_several_points_per_voxel():
    grid = (65, 7, 5)
    m = _perm_matrix((0, 1, 2), (1, 1, 1), 0.25, (0.0, 0.0, 0.0))
    want = check_table(full_table(grid), grid, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), m, (17, 3, 2))
    assert want[0].all() and want[3][0] == 65 * 35 and want[3][1] == 0


def test_rotation_at_ratio_three_quarters():
    grid = (40, 33, 29)
    m = CO.rotated_matrix(7, 1.0, (-40.0, -38.0, -36.0))
    table = CO.random_table(grid, 3, 0.9)
    want = check_table(table, grid, (-15.0, -12.4, -10.9), (0.75, 0.75, 0.75), m, (70, 67, 71))
    assert want[3][1] == 0 and want[3][3] == 0 and 0.2 * want[3][0] < want[0].sum() < 0.8 * want[3][0]       # several points per voxel


@pytest.mark.parametrize('offset,shape', [((-4.0, 0.25, 0.25), (5, 7, 5)), ((0.25, -2.0, 1.0), (3, 2, 4)), ((-9.0, 0.0, 0.0), (4, 6, 4)),
                                          ((3.0, -5.0, -1.0), (6, 3, 3)), ((-70.0, 0.0, 0.0), (33, 6, 4))])
def test_points_above_and_below(offset, shape):
    grid = (67, 6, 4)
    m = _perm_matrix((0, 1, 2), (1, 1, 1), 1.0, offset)
    table = CO.random_table(grid, 5, 0.8)
    want = check_table(table, grid, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), m, shape, offset)
    assert want[3][1] > 0 or want[3][3] > 0
    if want[3][3]:
        with pytest.raises(IndexError, match='below'):
            CM.scatter_mask(table, m, shape, grid=grid, origin=(0, 0, 0), unit=(1, 1, 1))
    else:
        assert np.array_equal(CM.scatter_mask(table, m, shape, grid=grid, origin=(0, 0, 0), unit=(1, 1, 1)), want[0])
        assert np.array_equal(CM.last_counts, want[3])


def test_saturated_indices():
    grid = (33, 3, 3)
    table = CO.random_table(grid, 6)
    big = np.float32(3e38)
    for row in ([1.0, 0, 0, 3e9], [1.0, 0, 0, -3e9], [big, big, 0, 0], [big, -big, 0, 0]):
        m = _perm_matrix((0, 1, 2), (1, 1, 1), 1.0, (0, 0, 0))
        m[1] = row
        want = check_table(table, grid, (4.0, 4.0, 4.0), (1.0, 1.0, 1.0), m, (40, 40, 40), row)
        assert want[3][1] + want[3][3] == want[3][0] and abs(int(want[1][1])) >= 2 ** 31 - 1


def test_exact_ties():
    """unit 1, min 0 and the identity: t = idx + 0.5 exactly, half to even; then the ties on the negative side."""
    grid = (66, 4, 3)
    table = full_table(grid)
    for off in (0.0, -0.5, -1.0, -7.0):
        m = _perm_matrix((0, 1, 2), (1, 1, 1), 1.0, (off, off, off))
        want = check_table(table, grid, (0, 0, 0), (1, 1, 1), m, (67, 5, 5), off)
        if off == 0.0:
            assert not want[0][1::2].any() and not want[0][:, 1::2].any() and want[0][0::2, 0::2, 0:3:2].all()


@pytest.mark.parametrize('shape', [(50, 21, 1), (37, 21, 19), (33, 15, 7)])
def test_output_shapes(shape):
    """M3 = 1; extents that are no multiple of 32; and (33, 15, 7): the last source voxel lands on the last voxel of out."""
    grid = (33, 15, 7)
    m = _perm_matrix((0, 1, 2), (1, 1, 1), 1.0, (-0.5, -0.5, -0.5))           # voxel (i, j, k) to (i, j, k)
    table = CO.random_table(grid, 8, 0.6)
    table[-1] |= np.uint32(1) << np.uint32(31 - (33 * 15 * 7 - 1) % 32)
    want = check_table(table, grid, (0, 0, 0), (1, 1, 1), m, shape, shape)
    if shape == (33, 15, 7):
        assert want[0][-1, -1, -1] == 1 and want[3][1] == 0 and np.array_equal(want[2], [32, 14, 6])
        assert np.array_equal(want[0].astype(bool), CO.table_mask(table, grid).transpose(2, 1, 0))
    elif shape[2] == 1:
        assert want[3][1] > 0                                     # every point with k > 0 is above


# ---------------------------------------------------------------- launch limits ----------------------------------------------------------------

def test_more_points_than_one_launch_sweeps():
    """A full table of 2^26 voxels: one launch of the scatter kernel sweeps 2^21 source voxels, the rest goes through its grid-stride rounds. The
    restatement is taken plane by plane."""
    grid = (1024, 256, 256)
    origin, unit = (-100.0, -20.0, -30.0), (0.25, 0.125, 0.25)
    m = np.array([[0.0, 0.5, 0.0, 10.25], [0.0, 0.0, 0.5, 15.0], [0.5, 0.0, 0.0, 50.5]], np.float32)
    shape = (17, 33, 120)
    out = np.zeros(shape, np.uint8)
    lo, hi, counts = np.full(3, 2 ** 40), np.full(3, -2 ** 40), np.zeros(4, np.int64)
    ij = np.stack(np.meshgrid(np.arange(1024), np.arange(256), indexing='xy'), axis=-1).reshape(-1, 2).astype(np.float64)      # i fastest
    x = (origin[0] + (ij[:, 0] + 0.5) * unit[0]).astype(np.float32)
    y = (origin[1] + (ij[:, 1] + 0.5) * unit[1]).astype(np.float32)
    for k in range(256):
        z = np.full(x.shape, np.float32(origin[2] + (k + 0.5) * unit[2]), np.float32)
        o, l, h, c = CO.scatter(np.stack([x, y, z], axis=1), m, shape)
        out |= o
        lo, hi, counts = np.minimum(lo, l), np.maximum(hi, h), counts + c
    assert counts[0] == 2 ** 26 and counts[1] > 0 and out.any() and not out.all()
    got = device_table(full_table(grid), grid, origin, unit, m, shape)
    CO.agree(got, (out, lo, hi, counts))


def test_the_same_bytes_in_every_run():
    grid = (130, 33, 29)
    m = CO.rotated_matrix(9, 1.0, (-60.0, -58.0, -56.0))
    table = CO.random_table(grid, 10, 0.9)
    runs = [device_table(table, grid, (-15.0, -12.4, -10.9), (0.75, 0.75, 0.75), m, (140, 120, 125)) for _ in range(3)]
    assert runs[0][0].any()
    for r in runs[1:]:
        assert r[0].tobytes() == runs[0][0].tobytes()
        assert np.array_equal(r[1], runs[0][1]) and np.array_equal(r[2], runs[0][2]) and np.array_equal(r[3], runs[0][3])
    assert CM.last_kernel_ms > 0


# ---------------------------------------------------------------- the fused entry ----------------------------------------------------------------

def mesh_case(name):
    if name == 'ico1280':
        tri = VO.ellipsoid_triangles(3, (3.0, 4.0, 2.5), 13)
        return (tri,) + VO.bounds_of(tri) + ((28, 36, 28),)
    if name == 'rotated_box':
        tri = (VO.box_triangles((-2, -3, -1.5), (2, 3, 1.5)).astype(np.float64) @ VO.rotation(3).T).astype(np.float32)
        return (tri,) + VO.bounds_of(tri) + ((33, 21, 17),)
    if name == 'clamped':                                         # the box cuts the mesh
        return VO.ellipsoid_triangles(2, (3.0, 4.0, 2.5), 7), np.array([-1.0, -2.0, -5.0]), np.array([1.5, 6.0, 1.0]), (9, 17, 13)
    raise KeyError(name)


@pytest.mark.parametrize('name', ['ico1280', 'rotated_box', 'clamped'])
def test_fused_entry_equals_table_then_scatter(name):
    tri, lo, hi, grid = mesh_case(name)
    unit = VO.unit_of(lo, hi, grid)
    m = CO.rotated_about(12, 0.2, (0.0, 0.0, 0.0), (30.0, 34.0, 28.0))
    shape = (66, 70, 61)
    table = VX.voxelize_table(tri, np.stack([lo, hi]), grid)
    assert np.array_equal(table, VO.pack_table(VO.voxelize(tri, lo, hi, grid)))
    pts = VX.voxel_points(table, grid, lo, unit)
    want = CO.scatter(pts, m, shape)
    assert want[3][0] == len(pts) > 0 and want[0].any()
    before = tri.copy()
    fused = device_mesh(tri, lo, hi, grid, m, shape)
    assert np.array_equal(tri, before) and CM.last_kernel_ms > 0
    CO.agree(fused, want, 'fused against voxel_points -> restatement')
    CO.agree(fused, device_table(table, grid, lo, unit, m, shape), 'fused against table -> scatter')
    CO.agree(device_mesh(tri, lo, hi, grid, m, None), CO.scatter(pts, m, None), 'bounds pass')
    # the public calls
    blo, bhi, n = CM.rotated_bounds(tri, m, bounds=np.stack([lo, hi]), grid=grid)
    assert n == len(pts) and np.array_equal(blo, want[1]) and np.array_equal(bhi, want[2])
    assert np.array_equal(CM.scatter_mask(tri, m, shape, bounds=np.stack([lo, hi]), grid=grid), want[0])


# ---------------------------------------------------------------- conformal_masks ----------------------------------------------------------------

def test_conformal_masks_on_nested_ellipsoids():
    """Masks, baseaffineRot and LocFocalPoint equal the numpy flow over Voxelize's points; then the chain conformal mask -> closing -> largest
    component, as Step 1 strings them, against scipy."""
    ndi = pytest.importorskip('scipy.ndimage')
    meshes = [VO.ellipsoid_triangles(3, r, 41, centre=(12.0, -7.0, 30.0)) for r in ((9.0, 11.0, 8.0), (7.5, 9.0, 6.5), (6.0, 7.5, 5.0))]
    step, R, location = 1.0, VO.rotation(17), (13.0, -6.0, 29.0)
    got = CM.conformal_masks(meshes[0], meshes[1], meshes[2], step, R, location)
    assert CM.last_kernel_ms > 0
    pts = [VX.Voxelize(mesh, 0.75 * step) for mesh in meshes]
    want = CO.conformal_flow(pts[0], pts[1], pts[2], step, R, location)
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
    assert got[2].sum() > got[3].sum() > got[4].sum() > 1000 and got[2][tuple(got[1])] == 1
    st = np.ones((3, 3, 3), int)
    chain = LI.largest_component(BC.BinaryClose(got[3].astype(bool), st))
    closed = ndi.binary_closing(want[3].astype(bool), structure=st)
    lab, n = ndi.label(closed, ndi.generate_binary_structure(3, 3))
    sizes = np.bincount(lab.ravel())[1:]
    ref = lab == (n - int(np.argmax(sizes[::-1])))
    assert n >= 1 and chain.shape == ref.shape and np.array_equal(chain, ref) and ref.any()


# ---------------------------------------------------------------- the call contract ----------------------------------------------------------------

@pytest.fixture(scope='module')
def lib():
    return _engine.load_library()


@pytest.mark.parametrize('entry', CC.ENTRIES)
def test_ordinal_out_of_range(lib, entry):
    case = CC.Case(entry)
    assert case.run(lib, lib.bfd_device_count()) == -3
    assert lib.bfd_last_error().decode() == entry + ': device ordinal out of range'
    assert case.untouched()


@pytest.mark.parametrize('entry', CC.ENTRIES)
def test_refusals_in_order_leave_everything_untouched(lib, entry):
    words = {n: w for n, w, _ in CC.faults(entry)}
    for names, first in CC.ordered_plants(entry):
        c = CC.planted(entry, names)
        assert c.run(lib) == -1 and words[first] in lib.bfd_last_error().decode() and c.untouched(), names


@pytest.mark.parametrize('entry', CC.ENTRIES)
def test_empty_table(lib, entry):
    """Not an error: out all zero, counts all zero, lo and hi untouched, kernelMs written."""
    case = CC.Case(entry, empty=True)
    assert case.run(lib, 0) == 0, lib.bfd_last_error().decode()
    o = case.outputs
    assert not o['out'].any() and not o['counts'].any()
    assert np.array_equal(o['lo'], case.pristine['lo']) and np.array_equal(o['hi'], case.pristine['hi'])
    assert case.ms[0] >= 0


@pytest.mark.parametrize('entry', CC.ENTRIES)
def test_valid_call_twice(lib, entry):
    case = CC.Case(entry)
    assert case.run(lib, 0) == 0, lib.bfd_last_error().decode()
    assert case.ms[0] > 0
    first = case.snapshot()
    assert all(not np.array_equal(first[k], case.pristine[k]) for k in first)         # the call wrote every output
    assert first['counts'][0] > 0 and first['out'].max() == 1 and set(np.unique(first['out'])) <= {0, 1}
    for k, v in case.outputs.items():                 # sentinels again: the second call has to write everything itself
        v[...] = case.pristine[k]
    case.ms[:] = CC.MS_SENTINEL
    assert case.run(lib, 0) == 0, lib.bfd_last_error().decode()
    assert case.ms[0] > 0
    for k, v in case.outputs.items():
        assert np.array_equal(v, first[k]), k
