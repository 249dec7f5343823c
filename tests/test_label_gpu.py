"""Device component labelling (bfd_label3d behind babelbrain_amd.LabelImage) against scipy.ndimage.label with generate_binary_structure(3, c),
element by element: labels, their number, the sizes (np.bincount of the reference) and the largest component (most voxels, among equals the
highest label). The kernel's workgroup-local union-find works on tiles of T x T x W = 8 x 8 x 64 voxels (i, j, k) and joins them across faces, edges
and corners afterwards: the shapes and the hand-placed voxels below straddle those."""
import numpy as np
import pytest

from babelbrain_amd import BinaryClosing as BC, LabelImage as LI, MedianFilter as MF

ndi = pytest.importorskip('scipy.ndimage')

pytestmark = pytest.mark.gpu

T = 8
W = 64
CONNECTIVITIES = [1, 2, 3]
_reference = {}


def reference(a, c, key=None):
    """(labels, n, sizes, largest) of scipy; computed once per key and shared"""
    if key is not None and (key, c) in _reference:
        return _reference[(key, c)]
    lab, n = ndi.label(a, ndi.generate_binary_structure(3, c))
    sizes = np.bincount(lab.ravel())[1:].astype(np.int64)
    if n:
        best = n - int(np.argmax(sizes[::-1]))              # the last of the labels with the largest count
        largest = lab == best
    else:
        largest = np.zeros(a.shape, bool)
    lab.setflags(write=False)
    out = (lab, n, sizes, largest)
    if key is not None:
        _reference[(key, c)] = out
    return out


def check(a, c, what, key=None):
    ref, n, sizes, largest = reference(a, c, key)
    before = a.copy()
    got, gn = LI.LabelImage(a, return_num=True, connectivity=c)
    assert np.array_equal(a, before), '%s: the input was modified' % what
    assert got.dtype == np.int32 and got.shape == a.shape and gn == n, (what, got.dtype, got.shape, gn, n)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        p = tuple(bad[0])
        raise AssertionError('%s: %d of %d labels differ, first at %s: got %d, expected %d' % (what, len(bad), got.size, p, got[p], ref[p]))
    gs = LI.component_sizes(a, connectivity=c)
    assert gs.dtype == np.int64 and np.array_equal(gs, sizes), (what, gs[:8], sizes[:8])
    gl = LI.largest_component(a, connectivity=c)
    assert gl.dtype == np.bool_ and np.array_equal(gl, largest), what
    return got, gn


@pytest.mark.parametrize('c', CONNECTIVITIES)
@pytest.mark.parametrize('fill', [0.05, 0.12, 0.30, 0.60])
@pytest.mark.parametrize('shape', [(12, 13, 70), (2 * T + 2, T + 1, 2 * W + 5)], ids=str)
def test_random_fill(shape, fill, c):
    a = np.random.default_rng(int(fill * 100)).random(shape) < fill
    check(a, c, 'fill %g of %s, c = %d' % (fill, shape, c))


@pytest.mark.parametrize('c', CONNECTIVITIES)
def test_empty_full_single(c):
    shape = (T + 1, 2 * T + 2, W + 6)
    got, n = check(np.zeros(shape, bool), c, 'empty')
    assert n == 0 and not got.any()
    got, n = check(np.ones(shape, bool), c, 'full')
    assert n == 1 and (got == 1).all()
    a = np.zeros(shape, bool)
    a[T, 2 * T + 1, W + 5] = True                    # the last voxel
    got, n = check(a, c, 'single voxel')
    assert n == 1 and got[T, 2 * T + 1, W + 5] == 1 and got.sum() == 1


@pytest.mark.parametrize('c', CONNECTIVITIES)
def test_pairs_across_tile_corners_and_edges(c):
    shape = (2 * T, 2 * T, 2 * W)
    a = np.zeros(shape, bool)
    a[T - 1, T - 1, W - 1] = a[T, T, W] = True       # touch by a corner, across the corner that eight tiles share
    _, n = check(a, c, 'corner pair, c = %d' % c)
    assert n == (1 if c == 3 else 2)
    a[:] = False
    a[T - 1, T, W - 1] = a[T, T - 1, W] = True       # the same with j descending: the later voxel's neighbour lies at j + 1
    _, n = check(a, c, 'corner pair (j + 1), c = %d' % c)
    assert n == (1 if c == 3 else 2)
    for p, q in ((((T - 1, T - 1, 5)), (T, T, 5)), ((3, T - 1, W - 1), (3, T, W)), ((T - 1, 3, W), (T, 3, W - 1)), ((T - 1, T, 70), (T, T - 1, 70))):
        a[:] = False
        a[p] = a[q] = True                           # touch by an edge (two coordinates differ), across an edge that four tiles share
        _, n = check(a, c, 'edge pair %s %s, c = %d' % (p, q, c))
        assert n == (1 if c >= 2 else 2)
    a[:] = False
    a[T - 1, 4, 4] = a[T, 4, 4] = a[2, T - 1, 9] = a[2, T, 9] = a[5, 5, W - 1] = a[5, 5, W] = True      # three pairs across a face
    _, n = check(a, c, 'face pairs, c = %d' % c)
    assert n == 3


def serpentines(shape=(3 * T, 3 * T, 200)):
    """Two paths, one voxel thick, each through every tile of the volume. A: the rows (i, j) = (4 I, 4 J), whole in k, taken in boustrophedon order
    and joined end to end at k = 0 / N3 - 1; it starts at voxel (0, 0, 0), so its root lies in the first tile and its end in the last plane of
    rows. B: the same two voxels further in i and j, with rows from k = 2 to N3 - 3: nowhere within reach of A, except for one spur that ends
    diagonally (i and j differ) beside a row of A."""
    N1, N2, N3 = shape
    a = np.zeros(shape, bool)
    for off, klo, khi in ((0, 0, N3 - 1), (2, 2, N3 - 3)):
        nodes = []
        for I in range(N1 // 4):
            js = list(range(N2 // 4))
            for J in (js if I % 2 == 0 else js[::-1]):
                nodes.append((4 * I + off, 4 * J + off))
        for t, (i, j) in enumerate(nodes):
            a[i, j, klo:khi + 1] = True
            if t + 1 < len(nodes):
                i2, j2 = nodes[t + 1]
                kend = khi if t % 2 == 0 else klo
                a[min(i, i2):max(i, i2) + 1, min(j, j2):max(j, j2) + 1, kend] = True
    a[4 * 2 + 1, 4 * 3 + 2, 100] = True              # the spur of B: beside B's row (10, 14) ...
    a[4 * 2 + 1, 4 * 3 + 1, 100] = True              # ... and on to the voxel diagonal to A's row (8, 12)
    return a


@pytest.mark.parametrize('c', CONNECTIVITIES)
def test_serpentines(c):
    a = serpentines()
    got, n = check(a, c, 'serpentines, c = %d' % c, key='serpentines')
    assert n == (2 if c == 1 else 1)
    assert got[0, 0, 0] == 1 and got[20, 0, 199] == 1           # both ends of A
    assert got[2, 2, 2] == n


@pytest.mark.parametrize('c', CONNECTIVITIES)
def test_checkerboard(c):
    """(i + j + k) even on (40, 41, 90): 73,800 single voxels for c = 1 -- more than 65,535 labels -- and one component for c = 2 and 3"""
    i, j, k = np.indices((40, 41, 90))
    a = (i + j + k) % 2 == 0
    _, n = check(a, c, 'checkerboard, c = %d' % c)
    assert n == (73800 if c == 1 else 1)


def test_tie_for_the_largest():
    a = np.zeros((T + 1, T + 1, W + 6), bool)
    a[0, 0, 0:5] = True                              # label 1: 5 voxels
    a[2, 2, 10:13] = True                            # label 2: 3
    a[T, T, W - 2:W + 3] = True                      # label 3: 5 again, across the word boundary -- the one to choose
    got, n = check(a, 1, 'tie')
    assert n == 3
    big = LI.largest_component(a)
    assert np.array_equal(big, got == 3) and big.sum() == 5
    assert np.array_equal(LI.component_sizes(a), [5, 3, 5])


def test_background_return_num_and_init():
    a = np.random.default_rng(4).random((12, 13, 70)) < 0.7
    before = a.copy()
    inv = LI.LabelImage(a, background=1)
    ref, n = ndi.label(~a, ndi.generate_binary_structure(3, 3))
    assert isinstance(inv, np.ndarray) and inv.dtype == np.int32 and np.array_equal(inv, ref) and np.array_equal(a, before)
    lab, m = LI.LabelImage(a, background=1, return_num=True, connectivity=1, GPUBackend='OpenCL')
    ref1, n1 = ndi.label(~a, ndi.generate_binary_structure(3, 1))
    assert m == n1 and np.array_equal(lab, ref1)
    t = np.ascontiguousarray(a.transpose(2, 1, 0)).transpose(2, 1, 0)           # not C-contiguous
    assert np.array_equal(LI.LabelImage(t), ndi.label(a, ndi.generate_binary_structure(3, 3))[0])
    assert LI.last_kernel_ms is not None and LI.last_kernel_ms > 0
    assert LI.InitLabel(DeviceName='no such device', GPUBackend='Metal')


def skull_shell(shape=(64, 60, 140)):
    """a spherical shell with holes and a few detached specks, uint8 0 / 1"""
    rng = np.random.default_rng(9)
    x = np.indices(shape).astype(np.float32)
    r = np.sqrt(sum(((x[d] - (shape[d] - 1) / 2) / (shape[d] / 2)) ** 2 for d in range(3)))
    a = (r > 0.72) & (r < 0.86)
    a &= rng.random(shape) > 0.25                    # holes, which the median and the closing fill
    a[rng.random(shape) < 2e-3] = True               # specks
    a[2:5, 2:5, 2:6] = True                          # and a block well away from the shell
    return a.astype(np.uint8)


def test_chain_median_closing_largest():
    """threshold -> median -> closing -> label -> largest region (BabelDatasetPreps.py:870-894), every step on the device, against the scipy chain
    on the device median's output; regionprops is replaced by np.bincount"""
    ct = skull_shell()
    fct = MF.MedianFilter(ct, 3)
    st = np.ones((5, 5, 5), int)
    closed = BC.BinaryClose(fct, structure=st, GPUBackend='OpenCL') != 0
    ref_closed = ndi.binary_closing(fct, structure=st)
    assert np.array_equal(closed, ref_closed)
    nfct = closed
    label_img = LI.LabelImage(nfct, GPUBackend='OpenCL')
    ref_img, n = ndi.label(ref_closed, ndi.generate_binary_structure(3, 3))
    assert np.array_equal(label_img, ref_img) and n > 1
    areas = np.bincount(ref_img.ravel())[1:]
    regions = sorted(range(1, n + 1), key=lambda lab: areas[lab - 1])
    want = ref_img == regions[-1]
    assert np.array_equal(LI.largest_component(nfct), want)
    assert want.sum() > 0.5 * nfct.sum()             # the shell, not a speck
