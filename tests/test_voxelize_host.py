"""Mesh voxelisation and CT value mapping without a GPU: Voxelize / MapFilter refuse bad arguments before the library is loaded and the C ABI
before a device is looked for; the reference's grid rule; the numpy restatement of the definition (voxelize_oracle.py), which the device tests hold
the kernels to, is itself checked against analytic solids; and bfd_voxelize_core.h, compiled for the host, equals that restatement bit for bit."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from babelbrain_amd import MappingFilter as MF, Voxelize as VX, _engine
from tests import voxelize_oracle as VO


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """The library is out of reach: its path names a missing file and loading it is an error. The refusals below must come first."""
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_engine, 'LIB_PATH', str(tmp_path / 'no_such_library.so'))
    monkeypatch.setattr(_engine, '_lib', None)
    monkeypatch.setattr(_engine, 'load_library', boom)


CUBE = VO.box_triangles((0, 0, 0), (8, 8, 8))
CUBE_BOUNDS = np.array([[0.0, 0, 0], [8, 8, 8]])


class Mesh:
    """What Voxelize needs of a trimesh object."""
    class _BB:
        def __init__(self, bounds):
            self.bounds = bounds

    def __init__(self, triangles, bounds=None):
        self.triangles = triangles
        if bounds is not None:
            self.bounding_box = Mesh._BB(bounds)


# ---------------------------------------------------------------- refusals ----------------------------------------------------------------

def test_voxelize_refuses_before_the_library(no_library):
    bad = CUBE.copy()
    bad[3, 1, 2] = np.nan
    with pytest.raises(ValueError, match='finite'):
        VX.Voxelize(bad, 1.0)
    bad[3, 1, 2] = np.inf
    with pytest.raises(ValueError, match='finite'):
        VX.Voxelize(Mesh(bad), 1.0)
    with pytest.raises(ValueError, match='finite'):
        VX.Voxelize(CUBE.astype(np.float64) * 1e39, 1e38)         # finite as float64, not as float32
    with pytest.raises(ValueError, match='shape'):
        VX.Voxelize(CUBE.reshape(-1, 9), 1.0)
    with pytest.raises(ValueError, match='shape'):
        VX.Voxelize(CUBE[:, :2], 1.0)
    with pytest.raises(ValueError, match='no triangle'):
        VX.Voxelize(np.zeros((0, 3, 3), np.float32), 1.0)
    with pytest.raises(TypeError):
        VX.Voxelize(np.zeros((4, 3, 3), complex), 1.0)
    flat = CUBE.copy()
    flat[:, :, 1] = 2.0                                           # zero thickness along y
    with pytest.raises(ValueError, match='thickness on axis 1'):
        VX.Voxelize(flat, 1.0)
    for res in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='targetResolution'):
            VX.Voxelize(CUBE, res)
    with pytest.raises(ValueError, match='bounds'):
        VX.voxelize_table(CUBE, np.zeros((3, 2)), (8, 8, 8))
    with pytest.raises(ValueError, match='thickness'):
        VX.voxelize_mask(CUBE, [[0, 0, 0], [8, 0, 8]], (8, 8, 8))
    with pytest.raises(ValueError, match='finite'):
        VX.voxelize_mask(CUBE, [[0, 0, 0], [8, np.inf, 8]], (8, 8, 8))
    for grid in ((8, 8), (8, 0, 8), (8, 8, 1.5), (2 ** 31, 1, 1), (2 ** 20, 2 ** 20, 2)):
        with pytest.raises(ValueError, match='grid'):
            VX.voxelize_table(CUBE, CUBE_BOUNDS, grid)
    with pytest.raises(ValueError, match='2\\^31'):
        VX.voxelize_mask(CUBE, CUBE_BOUNDS, (2048, 1024, 1024))
    with pytest.raises(ValueError, match='table'):
        VX.voxel_points(np.zeros(15, np.uint32), (8, 8, 8), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match='table'):
        VX.voxel_points(np.zeros(16, np.int32), (8, 8, 8), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match='finite'):
        VX.voxel_points(np.zeros(16, np.uint32), (8, 8, 8), (0, np.nan, 0), (1, 1, 1))
    for call in (lambda: VX.Voxelize(Mesh(CUBE, CUBE_BOUNDS), 1.0, GPUBackend='OpenCL'), lambda: VX.voxelize_mask(CUBE, CUBE_BOUNDS, (8, 8, 8)),
                 lambda: VX.voxel_points(np.zeros(16, np.uint32), (8, 8, 8), (0, 0, 0), (1, 1, 1))):
        with pytest.raises(AssertionError, match='library was loaded'):        # a good call gets as far as the library
            call()


def test_mapfilter_refuses_before_the_library(no_library):
    hu = np.zeros((4, 5, 6), np.float32)
    sel = np.ones((4, 5, 6), np.uint8)
    uni = np.array([0.0, 1.0], np.float32)
    with pytest.raises(TypeError):
        MF.MapFilter(hu.astype(np.float64), sel, uni)
    with pytest.raises(TypeError):
        MF.MapFilter(hu, sel.astype(bool), uni)
    with pytest.raises(TypeError):
        MF.MapFilter(hu, sel, uni.astype(np.float64))
    with pytest.raises(TypeError):
        MF.MapFilter(hu.tolist(), sel, uni)
    with pytest.raises(ValueError, match='shape'):
        MF.MapFilter(hu, sel[:, :, :5], uni)
    with pytest.raises(ValueError, match='Fortran'):
        MF.MapFilter(np.asfortranarray(hu), np.asfortranarray(sel), uni)
    with pytest.raises(ValueError, match='rows'):
        MF.MapFilter(hu, sel, np.zeros(0, np.float32))
    with pytest.raises(ValueError, match='rows'):
        MF.MapFilter(hu, sel, np.arange(65537, dtype=np.float32))
    with pytest.raises(ValueError, match='rows'):
        MF.MapFilter(hu, sel, uni.reshape(1, 2))
    for table in ([1.0, 0.0], [0.0, 0.0], [0.0, np.nan], [np.nan], [-0.0, 0.0]):
        with pytest.raises(ValueError, match='increasing'):
            MF.MapFilter(hu, sel, np.array(table, np.float32))
    with pytest.raises(AssertionError, match='library was loaded'):
        MF.MapFilter(hu, sel, uni, GPUBackend='OpenCL')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


def test_abi_refuses_before_a_device(lib):
    """-1 with text, whether or not a device exists; a good call reaches the device question (-3 without one)."""
    P = _engine._ptr
    lo, hi = np.zeros(3), np.full(3, 8.0)
    table = np.zeros(16, np.uint32)
    cnt = C.c_int64(-5)

    def vox(tri=CUBE, n=12, lo=lo, hi=hi, g=(8, 8, 8), table=table, mask=None, count=cnt):
        return lib.bfd_voxelize_mesh(0, P(tri), n, P(lo), P(hi), g[0], g[1], g[2], P(table), P(mask), C.byref(count) if count is not None else None, None)
    nan = CUBE.copy()
    nan[11, 2, 2] = np.nan
    for kw, word in ((dict(n=0), 'triangle'), (dict(tri=nan), 'finite'), (dict(hi=np.array([8.0, 0.0, 8.0])), 'max > min'),
                     (dict(lo=np.array([0.0, -np.inf, 0.0])), 'finite'), (dict(g=(8, 0, 8)), 'grid'), (dict(g=(2 ** 31, 1, 1)), 'grid'),
                     (dict(g=(2 ** 20, 2 ** 20, 2)), 'grid'), (dict(table=None, count=None), 'no output'),
                     (dict(g=(2048, 1024, 1024), mask=np.zeros(1, np.uint8)), 'mask'), (dict(tri=None), 'null'),
                     (dict(hi=np.array([8.0, 1e-320, 8.0]), lo=np.zeros(3), g=(8, 2 ** 20, 8)), 'voxel size')):
        assert vox(**kw) == -1, kw
        assert word in lib.bfd_last_error().decode(), (kw, lib.bfd_last_error().decode())

    def pts(table=table, g=(8, 8, 8), lo=lo, unit=np.ones(3), points=None, cap=0, count=cnt):
        return lib.bfd_voxel_points(0, P(table), g[0], g[1], g[2], P(lo), P(unit), P(points), cap, C.byref(count), None)
    full = np.full(16, 0xFFFFFFFF, np.uint32)
    for kw, word in ((dict(table=None), 'null'), (dict(g=(0, 8, 8)), 'grid'), (dict(cap=-1), 'capacity'), (dict(unit=np.array([1.0, np.nan, 1.0])), 'finite'),
                     (dict(table=full, cap=511, points=np.zeros((511, 3), np.float32)), 'capacity')):
        assert pts(**kw) == -1, kw
        assert word in lib.bfd_last_error().decode(), (kw, lib.bfd_last_error().decode())
    assert cnt.value == 512                                       # reported with the refusal
    partial = np.full(1, 0xFFFFFFFF, np.uint32)                   # 3 x 3 x 3 = 27 voxels: the 5 padding bits do not count
    assert pts(table=partial, g=(3, 3, 3)) == -1 and cnt.value == 27

    hu, sel, out = np.zeros(10, np.float32), np.ones(10, np.uint8), np.zeros(10, np.uint32)

    def mp(hu=hu, sel=sel, uni=np.array([0.0, 1.0], np.float32), nU=None, out=out, N=10):
        return lib.bfd_map_values3d(0, P(hu), P(sel), P(uni), uni.size if nU is None else nU, P(out), N, None)
    for kw, word in ((dict(hu=None), 'null'), (dict(N=-1), 'negative'), (dict(nU=0), 'rows'), (dict(uni=np.arange(65537, dtype=np.float32)), 'rows'),
                     (dict(uni=np.array([1.0, 1.0], np.float32)), 'increasing'), (dict(uni=np.array([np.nan], np.float32)), 'NaN'),
                     (dict(uni=np.array([0.0, np.nan], np.float32)), 'increasing'), (dict(out=hu.view(np.uint32)), 'alias')):
        assert mp(**kw) == -1, kw
        assert word in lib.bfd_last_error().decode(), (kw, lib.bfd_last_error().decode())
    if lib.bfd_device_count() == 0:
        assert vox() == -3 and mp() == -3 and pts(table=full, cap=512, points=np.zeros((512, 3), np.float32)) == -3
        assert pts(unit=np.ones(3)) == -3                         # an empty table passes the capacity check too


# ---------------------------------------------------------------- the grid rule ----------------------------------------------------------------

def test_grid_rule_is_the_reference_s():
    r = np.array([[-71.3, -100.2, -50.0], [80.9, 95.5, 77.25]])
    res = VX.DEFAULT_RESOLUTION
    assert res == 1333 / 500e3 / 6 * 0.75 * 1e3
    g, unit = VX.grid_rule(r, res)
    dims = np.diff(r, axis=0).flatten()
    assert g == (int(np.ceil(dims[0] / res)), int(np.ceil(dims[1] / res)), int(np.ceil(dims[2] / res)))
    assert np.array_equal(unit, dims / np.array(g)) and np.all(unit <= res)
    assert VX.grid_rule([[0, 0, 0], [8, 8, 4]], 1.0)[0] == (8, 8, 4)
    assert VX.grid_rule([[0, 0, 0], [8.001, 8, 4]], 1.0)[0] == (9, 8, 4)
    # bounds: the mesh's own bounding box when it has one, the vertices otherwise
    assert np.array_equal(VX.mesh_bounds(Mesh(CUBE, CUBE_BOUNDS - 1)), CUBE_BOUNDS - 1)
    assert np.array_equal(VX.mesh_bounds(Mesh(CUBE)), CUBE_BOUNDS)
    assert np.array_equal(VX.mesh_bounds(CUBE), CUBE_BOUNDS)


# ---------------------------------------------------------------- the oracle against analytic solids ----------------------------------------------------------------

ICO_CASES = [(1, (12, 14, 10)), (2, (20, 24, 18)), (3, (28, 36, 28))]        # 80, 320, 1280 triangles


@pytest.mark.parametrize('level,grid', ICO_CASES)
def test_oracle_equals_the_half_space_test(level, grid):
    """A convex polyhedron is the intersection of its faces' half-spaces: no parity, no projection, no edge rule in this yardstick."""
    tri = VO.ellipsoid_triangles(level, (3.0, 4.0, 2.5), 10 + level)
    assert len(tri) == 20 * 4 ** level
    lo, hi = VO.bounds_of(tri)
    mask, passes, _, _ = VO.voxelize(tri, lo, hi, grid, want_passes=True)
    ii = np.stack(np.meshgrid(*[np.arange(n) for n in grid], indexing='ij'), -1).reshape(-1, 3)
    inside, margin = VO.inside_polyhedron(tri, lo + (ii + 0.5) * VO.unit_of(lo, hi, grid))
    assert margin.min() > 1e-9                                    # no centre sits on a face: the yardstick is decided everywhere
    assert np.count_nonzero(inside.reshape(grid) != mask) == 0
    assert np.count_nonzero(passes & 1) == 0                      # a closed surface is crossed an even number of times in every column
    assert mask.any() and not mask.all()


def test_oracle_counts_of_boxes():
    """Column centres on the diagonals of the x faces (eight each) and on no other edge: the top-left rule gives each to one triangle."""
    mask, passes, atomics, ref = VO.voxelize(CUBE, (0, 0, 0), (8, 8, 8), (8, 8, 8), want_passes=True)
    assert mask.sum() == 512 and np.all(passes == 2)
    assert atomics == 64 and ref == 512                           # one crossing per column here; one per voxel in the per-voxel formulation
    nested = np.concatenate([CUBE, VO.box_triangles((2, 2, 2), (6, 6, 6))[:, ::-1]])
    m = VO.voxelize(nested, (0, 0, 0), (8, 8, 8), (8, 8, 8))
    assert m.sum() == 448 and not m[2:6, 2:6, 2:6].any()
    assert VO.voxelize(VO.box_triangles((-3, 1, 2), (5, 9, 6)), (-3, 1, 2), (5, 9, 6), (16, 16, 8)).sum() == 2048


def test_oracle_invariances():
    tri = VO.ellipsoid_triangles(2, (3.0, 4.0, 2.5), 5)
    lo, hi = VO.bounds_of(tri)
    want = VO.voxelize(tri, lo, hi, (20, 24, 18))
    rng = np.random.default_rng(0)
    assert np.array_equal(VO.voxelize(tri[rng.permutation(len(tri))], lo, hi, (20, 24, 18)), want)
    for shift in (1, 2):
        assert np.array_equal(VO.voxelize(np.roll(tri, shift, axis=1), lo, hi, (20, 24, 18)), want)
    for cube in (CUBE[::-1], CUBE[:, ::-1], CUBE[::-1, ::-1], np.roll(CUBE, 1, axis=1)):        # where the edge rule decides
        assert VO.voxelize(cube, (0, 0, 0), (8, 8, 8), (8, 8, 8)).sum() == 512


def test_oracle_packing_and_points():
    mask = np.zeros((3, 2, 7), bool)
    mask[1, 0, 0] = mask[2, 1, 6] = mask[0, 1, 5] = True
    t = VO.pack_table(mask)
    assert t.dtype == np.uint32 and t.size == 2
    for i, j, k in ((1, 0, 0), (2, 1, 6), (0, 1, 5)):
        idx = i + 3 * (j + 2 * k)
        assert (t[idx // 32] >> (31 - idx % 32)) & 1
    assert sum(bin(int(w)).count('1') for w in t) == 3
    p = VO.points_of(mask, (10.0, 20.0, 30.0), (1.0, 2.0, 0.5))
    assert p.dtype == np.float32 and np.array_equal(p, np.array([[11.5, 21, 30.25], [10.5, 23, 32.75], [12.5, 23, 33.25]], np.float32))


def test_map_oracles_agree():
    rng = np.random.default_rng(1)
    uni = np.unique(rng.integers(-50, 50, 40).astype(np.float32))
    hu = rng.integers(-60, 60, (5, 6, 7)).astype(np.float32)
    hu[0, 0, :3] = [np.nan, np.inf, -np.inf]
    sel = (rng.random(hu.shape) < 0.7).astype(np.uint8)
    assert np.array_equal(VO.map_values(hu, sel, uni), VO.map_values_host_loop(hu, sel, uni))


# ---------------------------------------------------------------- bfd_voxelize_core.h on the host ----------------------------------------------------------------

CORE_PROGRAM = r"""
#include "bfd_voxelize_core.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>
// argv[1]: int64 n, gx, gy, gz; double min[3], max[3]; float triangles[n][9]. argv[2] receives the table. The kernels' steps, serially.
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t h[4];
    double b[6];
    if (fread(h, 8, 4, f) != 4 || fread(b, 8, 6, f) != 6) return 4;
    std::vector<float> tri((size_t)h[0] * 9);
    if (fread(tri.data(), 4, tri.size(), f) != tri.size()) return 5;
    fclose(f);
    const vox_grid g = vox_make_grid(b, b + 3, h[1], h[2], h[3]);
    std::vector<uint64_t> cross((size_t)(g.nColumns * g.rowWords), 0), occ(cross.size());
    for (int64_t t = 0; t < h[0]; t++) {
        vox_tri r;
        const int64_t pairs = vox_setup_triangle(&tri[9 * t], g, &r);
        for (int64_t local = 0; local < pairs; local++) {
            const int64_t kk = local / r.nj, jj = local - kk * r.nj, j = r.jl + jj, k = r.kl + kk;
            if (j < 0 || j >= g.gy || k < 0 || k >= g.gz) return 6;
            const int64_t c = vox_crossing(r, g, j, k);
            if (c < 0 || c > g.gx) return 7;
            if (c > 0) cross[(size_t)((j + g.gy * k) * g.rowWords + (c >> 6))] ^= (uint64_t)1 << (c & 63);
        }
    }
    for (int64_t wd = 0; wd < (int64_t)occ.size(); wd++) {
        const int64_t col = wd / g.rowWords;
        occ[wd] = vox_scan_word(&cross[(size_t)(col * g.rowWords)], wd - col * g.rowWords, g);
    }
    const int64_t nTable = (g.nVoxels + 31) / 32;
    std::vector<uint32_t> table((size_t)nTable);
    for (int64_t o = 0; o < nTable; o++) {
        table[o] = vox_table_word(occ.data(), o, g);
        if (table[o] & ~vox_table_valid(o, g.nVoxels)) return 8;
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(table.data(), 4, table.size(), f) != table.size()) return 9;
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope='module')
def core_program(tmp_path_factory):
    """bfd_voxelize_core.h compiled for the host by a plain C++ compiler, as its first lines say it can be."""
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx, 'no C++ compiler found'
    d = tmp_path_factory.mktemp('voxcore')
    src = d / 'voxcore.cpp'
    src.write_text(CORE_PROGRAM)
    exe = str(d / 'voxcore')
    subprocess.run([cxx, '-O1', '-ffp-contract=off', '-I', os.path.join(os.path.dirname(_engine.LIB_PATH), 'csrc'), str(src), '-o', exe, '-lm'], check=True)

    def run(tri, lo, hi, grid):
        inp, out = str(d / 'in.bin'), str(d / 'out.bin')
        with open(inp, 'wb') as f:
            f.write(np.array([len(tri)] + list(grid), np.int64).tobytes())
            f.write(np.concatenate([np.asarray(lo, np.float64), np.asarray(hi, np.float64)]).tobytes())
            f.write(np.ascontiguousarray(tri, np.float32).tobytes())
        subprocess.run([exe, inp, out], check=True)
        return np.fromfile(out, np.uint32)
    return run


def _rotated_box(seed=3):
    c = VO.box_triangles((-2, -3, -1.5), (2, 3, 1.5)).astype(np.float64)
    return (c @ VO.rotation(seed).T).astype(np.float32)


@pytest.mark.parametrize('gx', [1, 31, 32, 33, 63, 64, 65, 130])
def test_core_header_word_boundaries(core_program, gx):
    tri = _rotated_box()
    lo, hi = VO.bounds_of(tri)
    want = VO.voxelize(tri, lo, hi, (gx, 5, 5))
    assert want.any()
    assert np.array_equal(core_program(tri, lo, hi, (gx, 5, 5)), VO.pack_table(want))


def test_core_header_equals_the_oracle(core_program):
    for level, grid in ICO_CASES:
        tri = VO.ellipsoid_triangles(level, (3.0, 4.0, 2.5), 10 + level)
        lo, hi = VO.bounds_of(tri)
        assert np.array_equal(core_program(tri, lo, hi, grid), VO.pack_table(VO.voxelize(tri, lo, hi, grid)))
    assert np.array_equal(core_program(CUBE, (0, 0, 0), (8, 8, 8), (8, 8, 8)), np.full(16, 0xFFFFFFFF, np.uint32))
    # a box that cuts the mesh: surfaces beyond max_x and below min_x, columns outside in y and z
    tri = VO.ellipsoid_triangles(2, (3.0, 4.0, 2.5), 7)
    lo, hi = np.array([-1.0, -2.0, -5.0]), np.array([1.5, 6.0, 1.0])
    want = VO.voxelize(tri, lo, hi, (9, 17, 13))
    assert want.any() and not want.all()
    assert np.array_equal(core_program(tri, lo, hi, (9, 17, 13)), VO.pack_table(want))
