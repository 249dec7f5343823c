"""Conformal masks without a GPU: the pieces of bfd_voxelize_core.h the scatter kernel is made of, compiled for the host, equal the numpy restatement
(tests/conformal_oracle.py) number for number; the restatement itself is held to np.round(np.dot(...)), the reference's expression, and to float64 by
derived bounds; ConformalMask refuses bad arguments before the library is loaded, the C ABI before a device is looked for and in the header's order;
and conformal_masks follows BabelDatasetPreps.py:696-759 (its device calls stood in for by the restatement)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from babelbrain_amd import ConformalMask as CM, _engine
from tests import conformal_calls as CC, conformal_oracle as CO, voxelize_oracle as VO


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """The library is out of reach: its path names a missing file and loading it is an error. The refusals below must come first."""
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_engine, 'LIB_PATH', str(tmp_path / 'no_such_library.so'))
    monkeypatch.setattr(_engine, '_lib', None)
    monkeypatch.setattr(_engine, 'load_library', boom)


# ---------------------------------------------------------------- bfd_voxelize_core.h on the host ----------------------------------------------------------------

CORE_PROGRAM = r"""
#include "bfd_voxelize_core.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
// argv[1]: int64 gx, gy, gz, M[3] (M[0] = 0: the bounds pass); double min[3], unit[3]; float m[12]; uint32 table[]. argv[2] receives int64 lo[3],
// hi[3], counts[4], then the volume. The scatter kernel's steps, serially, with the kernel's own functions.
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t h[6];
    double b[6];
    float m[3][4];
    if (fread(h, 8, 6, f) != 6 || fread(b, 8, 6, f) != 6 || fread(m, 4, 12, f) != 12) return 4;
    const int64_t nVoxels = h[0] * h[1] * h[2], nTable = (nVoxels + 31) / 32;
    std::vector<uint32_t> table((size_t)nTable);
    if (fread(table.data(), 4, table.size(), f) != table.size()) return 5;
    fclose(f);
    const bool write = h[3] > 0;
    const int64_t M[3] = {h[3], h[4], h[5]};
    std::vector<uint8_t> out(write ? (size_t)(M[0] * M[1] * M[2]) : 0, 0);
    int64_t r[10] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN, 0, 0, 0, 0};
    for (int64_t idx = 0; idx < nVoxels; idx++) {
        if (!vox_table_bit(table.data(), idx)) continue;
        const int64_t row = idx / h[0], i = idx - row * h[0], k = row / h[1], j = row - k * h[1];
        int32_t n[3];
        conf_point(m, vox_centre(b[0], b[3], i), vox_centre(b[1], b[4], j), vox_centre(b[2], b[5], k), n);
        for (int a = 0; a < 3; a++) {
            if (n[a] < r[a]) r[a] = n[a];
            if (n[a] > r[3 + a]) r[3 + a] = n[a];
        }
        r[6]++;
        if (!write) continue;
        int64_t at = -1;
        const int c = conf_target(n, M, &at);
        if (c != CONF_INSIDE) r[6 + c]++;
        if (c == CONF_ABOVE || c == CONF_BELOW) continue;
        if (at < 0 || at >= (int64_t)out.size()) return 6;
        out[(size_t)at] = 1;
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(r, 8, 10, f) != 10 || (!out.empty() && fwrite(out.data(), 1, out.size(), f) != out.size())) return 7;
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope='module')
def core_scatter(tmp_path_factory):
    """(table, grid, origin, unit, matrix, shape or None) -> (out, lo, hi, counts) through bfd_voxelize_core.h and a plain C++ compiler."""
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx, 'no C++ compiler found'
    d = tmp_path_factory.mktemp('confcore')
    src = d / 'confcore.cpp'
    src.write_text(CORE_PROGRAM)
    exe = str(d / 'confcore')
    subprocess.run([cxx, '-O1', '-ffp-contract=off', '-I', os.path.join(os.path.dirname(_engine.LIB_PATH), 'csrc'), str(src), '-o', exe, '-lm'], check=True)

    def run(table, grid, origin, unit, matrix, shape):
        inp, outp = str(d / 'in.bin'), str(d / 'out.bin')
        with open(inp, 'wb') as f:
            f.write(np.array(list(grid) + list(shape or (0, 0, 0)), np.int64).tobytes())
            f.write(np.concatenate([np.asarray(origin, np.float64), np.asarray(unit, np.float64)]).tobytes())
            f.write(np.ascontiguousarray(matrix, np.float32).tobytes())
            f.write(np.ascontiguousarray(table, np.uint32).tobytes())
        subprocess.run([exe, inp, outp], check=True)
        r = np.fromfile(outp, np.int64, 10)
        out = np.fromfile(outp, np.uint8, offset=80).reshape(shape) if shape else None
        return out, r[:3], r[3:6], r[6:]
    return run


def test_core_header_random_points(core_scatter):
    grid, origin, unit = (13, 7, 5), (-3.25, 1.5, 0.125), (0.75, 0.7, 0.8)
    table = CO.random_table(grid, 1)
    pts = CO.table_points(table, grid, origin, unit)
    assert len(pts) and len(pts) < 13 * 7 * 5
    m = CO.rotated_matrix(4, 1.0, (-9.0, -4.0, -6.0))
    want = CO.scatter(pts, m, (14, 15, 13))
    assert want[3][0] == len(pts) and want[0].any()
    CO.agree(core_scatter(table, grid, origin, unit, m, (14, 15, 13)), want)
    CO.agree(core_scatter(table, grid, origin, unit, m, None), CO.scatter(pts, m, None))


def test_core_header_exact_ties(core_scatter):
    """unit 1, min 0 and the identity give t = idx + 0.5 exactly: even indices round down, odd ones up (half to even), so only even targets."""
    grid = (9, 4, 3)
    table = np.full((9 * 4 * 3 + 31) // 32, 0xFFFFFFFF, np.uint32)
    m = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
    pts = CO.table_points(table, grid, (0, 0, 0), (1, 1, 1))
    assert np.array_equal(pts[:3, 0], [0.5, 1.5, 2.5])
    want = CO.scatter(pts, m, (10, 5, 5))
    assert want[0][0::2, 0::2, 0::2].any() and not want[0][1::2].any() and not want[0][:, 1::2].any() and not want[0][:, :, 1::2].any()
    assert want[0][8, 4, 2] == 1 and want[0][2, 2, 2] == 1 and np.array_equal(want[2], [8, 4, 2])
    CO.agree(core_scatter(table, grid, (0, 0, 0), (1, 1, 1), m, (10, 5, 5)), want)
    # with -0.5 in the offset column every t is an integer; with -1 the ties are at idx - 0.5: negative ties round to even too
    for off in (-0.5, -1.0, -7.0):
        m[:, 3] = off
        CO.agree(core_scatter(table, grid, (0, 0, 0), (1, 1, 1), m, (10, 5, 5)), CO.scatter(pts, m, (10, 5, 5)), off)


def test_core_header_wrap_above_below(core_scatter):
    grid, origin, unit = (8, 6, 4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    table = CO.random_table(grid, 2, 0.8)
    pts = CO.table_points(table, grid, origin, unit)
    seen = np.zeros(4, np.int64)
    for off, shape in (((-4.0, 0.25, 0.25), (5, 7, 5)), ((0.25, -2.0, 1.0), (3, 2, 4)), ((-9.0, 0.0, 0.0), (4, 6, 4)), ((3.0, -5.0, -1.0), (6, 3, 3)),
                       ((0.0, 0.0, -4.25), (8, 6, 1))):
        m = np.hstack([np.eye(3), np.array(off).reshape(3, 1)]).astype(np.float32)
        want = CO.scatter(pts, m, shape)
        seen += want[3] > 0
        CO.agree(core_scatter(table, grid, origin, unit, m, shape), want, off)
    assert np.all(seen[1:] >= 2)                                # above, wrapped and below each occur in several of the cases
    # the saturated side: an offset past 2^31, an infinite and an indefinite t (0 * inf cannot arise from a finite matrix; inf - inf can)
    big = np.float32(3e38)
    for row in ([1.0, 0, 0, 3e9], [1.0, 0, 0, -3e9], [big, big, 0, 0], [big, -big, 0, 0]):
        m = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
        m[1] = row
        p2 = CO.table_points(table, grid, (4.0, 4.0, 4.0), unit)
        want = CO.scatter(p2, m, (16, 16, 16))
        assert want[3][1] + want[3][3] == want[3][0] and not want[0].any()
        CO.agree(core_scatter(table, grid, (4.0, 4.0, 4.0), unit, m, (16, 16, 16)), want, row)


def test_restatement_against_blas_and_float64():
    """The elementwise float32 restatement against the reference's own expression np.round(np.dot(M32, XYZ)) and against float64, on a rotated
    97 x 83 x 71 grid at ratio 0.75. The bound is derived, not measured. With u = 2^-24 (half an ulp, relative) and S = sum_b |m_ab x_b|, |m_a3| among
    the terms: the three products err by at most u |m_ab x_b| each, u S together; each of the three sums errs by at most u times its result, which
    is at most S to first order. So |t32 - t64| <= 4 u S, and the rounded indices can differ only where the float64 value lies within 4 * 2^-24 * S
    of a half-integer (float64's own error, 2^-53 S, is far inside). A BLAS product may order and fuse the same operations in any way; it gets twice
    that. The counts of differing points are printed and carried in the assertion message; no share is asserted."""
    g = (97, 83, 71)
    unit, step = 0.375, 0.5
    i, j, k = np.meshgrid(*[np.arange(n) for n in g], indexing='ij')
    idx = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(np.float64)
    pts = (np.array([-17.3, -14.9, -12.1]) + (idx + 0.5) * unit).astype(np.float32)
    assert pts.shape == (571621, 3)
    a = np.eye(4)
    a[:3, :3] = VO.rotation(11) * step
    a[:3, 3] = (-30.0, -28.0, -26.0)
    inv32 = np.linalg.inv(a).astype(np.float32)
    t32 = CO.transform(pts, inv32[:3])
    n32 = CO.indices(t32)
    xyz = np.hstack([pts, np.ones((len(pts), 1), np.float32)]).T
    blas = np.round(np.dot(inv32, xyz)).astype(np.int64).T[:, :3]
    m64 = inv32[:3].astype(np.float64)
    t64 = pts.astype(np.float64) @ m64[:, :3].T + m64[:, 3]
    n64 = np.round(t64).astype(np.int64)
    S = np.abs(pts.astype(np.float64)) @ np.abs(m64[:, :3]).T + np.abs(m64[:, 3])
    half = np.abs(t64 - np.floor(t64) - 0.5)                     # distance of the float64 value from the nearest half-integer
    d64, dblas = n32 != n64, n32 != blas
    message = 'restatement differs from float64 at %d and from the BLAS product at %d of %d points' % (d64.any(axis=1).sum(), dblas.any(axis=1).sum(), len(pts))
    print(message)
    assert np.all(half[d64] <= 4 * 2.0 ** -24 * S[d64]), message
    assert np.all(half[dblas] <= 8 * 2.0 ** -24 * S[dblas]), message
    assert np.all(np.abs(n32 - n64) <= 1) and np.all(np.abs(n32 - blas) <= 1), message
    assert len(np.unique(n32, axis=0)) > 0.3 * len(pts), message          # a real scatter: about 2.4 points per target


# ---------------------------------------------------------------- refusals ----------------------------------------------------------------

CUBE = VO.box_triangles((0, 0, 0), (8, 8, 8))
EYE = np.hstack([np.eye(3), np.zeros((3, 1))])


def test_python_refuses_before_the_library(no_library):
    table = np.zeros(16, np.uint32)
    tk = dict(grid=(8, 8, 8), origin=(0, 0, 0), unit=(1, 1, 1))
    for bad in (np.eye(3), np.zeros((4, 3)), np.zeros(12)):
        with pytest.raises(ValueError, match='shape'):
            CM.rotated_bounds(table, bad, **tk)
    with pytest.raises(TypeError):
        CM.rotated_bounds(table, EYE.astype(complex), **tk)
    for bad in (np.where(EYE == 1, np.nan, EYE), EYE * 1e39):                  # finite as float64, not as float32
        with pytest.raises(ValueError, match='finite'):
            CM.rotated_bounds(table, bad, **tk)
    with pytest.raises(ValueError, match='grid, origin and unit'):
        CM.rotated_bounds(table, EYE, grid=(8, 8, 8))
    with pytest.raises(ValueError, match='table'):
        CM.rotated_bounds(table[:15], EYE, **tk)
    with pytest.raises(ValueError, match='grid'):
        CM.rotated_bounds(table, EYE, grid=(8, 0, 8), origin=(0, 0, 0), unit=(1, 1, 1))
    with pytest.raises(ValueError, match='finite'):
        CM.rotated_bounds(table, EYE, grid=(8, 8, 8), origin=(0, np.inf, 0), unit=(1, 1, 1))
    for shape in ((4, 4), (4, 0, 4), (4, 4, 1.5), (2048, 1024, 1024)):
        with pytest.raises(ValueError, match='shape|2\\^31'):
            CM.scatter_mask(table, EYE, shape, **tk)
    # meshes: Voxelize's own refusals, and the ways to name a grid
    nan = CUBE.copy()
    nan[3, 1, 2] = np.nan
    with pytest.raises(ValueError, match='finite'):
        CM.rotated_bounds(nan, EYE, 1.0)
    with pytest.raises(ValueError, match='shape'):
        CM.scatter_mask(CUBE.reshape(-1, 9), EYE, (4, 4, 4), 1.0)
    with pytest.raises(ValueError, match='targetResolution'):
        CM.rotated_bounds(CUBE, EYE)
    with pytest.raises(ValueError, match='targetResolution'):
        CM.rotated_bounds(CUBE, EYE, 0.0)
    with pytest.raises(ValueError, match='come together'):
        CM.rotated_bounds(CUBE, EYE, grid=(8, 8, 8))
    with pytest.raises(ValueError, match='not both'):
        CM.rotated_bounds(CUBE, EYE, 1.0, bounds=[[0, 0, 0], [8, 8, 8]], grid=(8, 8, 8))
    with pytest.raises(ValueError, match='thickness'):
        CM.rotated_bounds(CUBE, EYE, bounds=[[0, 0, 0], [8, 0, 8]], grid=(8, 8, 8))
    with pytest.raises(ValueError, match='belong to a table'):
        CM.rotated_bounds(CUBE, EYE, 1.0, unit=(1, 1, 1))
    # conformal_masks
    good = dict(SpatialStep=1.0, RMat=np.eye(3), Location=(4.0, 4.0, 4.0))
    for kw, exc, word in ((dict(SpatialStep=0.0), ValueError, 'SpatialStep'), (dict(SpatialStep=np.nan), ValueError, 'SpatialStep'),
                          (dict(RMat=np.eye(4)), ValueError, 'RMat'), (dict(RMat=np.zeros((3, 3))), np.linalg.LinAlgError, ''),
                          (dict(Location=(1.0, 2.0)), ValueError, 'Location'), (dict(Location=(1.0, np.nan, 0.0)), ValueError, 'Location'),
                          (dict(targetResolution=-1.0), ValueError, 'targetResolution')):
        with pytest.raises(exc, match=word or None):
            CM.conformal_masks(CUBE, CUBE, CUBE, **dict(good, **kw))
    with pytest.raises(ValueError, match='finite'):
        CM.conformal_masks(CUBE, nan, CUBE, **good)
    for call in (lambda: CM.rotated_bounds(table, EYE, **tk), lambda: CM.scatter_mask(CUBE, np.eye(4), (8, 8, 8), 1.0),
                 lambda: CM.scatter_mask(CUBE, EYE, (8, 8, 8), bounds=[[0, 0, 0], [8, 8, 8]], grid=(8, 8, 8)),
                 lambda: CM.conformal_masks(CUBE, CUBE, CUBE, **good)):
        with pytest.raises(AssertionError, match='library was loaded'):        # a good call gets as far as the library
            call()


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


@pytest.mark.parametrize('entry', CC.ENTRIES)
def test_abi_refuses_before_a_device_in_the_header_s_order(lib, entry):
    """-1 with the text of the first fault the header lists, whether or not a device exists, with every output and kernelMs untouched."""
    assert entry in _engine.ABI_SYMBOLS and hasattr(lib, entry)
    words = {n: w for n, w, _ in CC.faults(entry)}
    for names, first in CC.ordered_plants(entry):
        c = CC.planted(entry, names)
        assert c.run(lib) == -1, names
        text = lib.bfd_last_error().decode()
        assert text.startswith(entry) and words[first] in text, (names, text)
        assert c.untouched(), names
    for kw, word in ((dict(want_hi=False), 'come together'), (dict(want_lo=False), 'come together'), (dict(matrix=None), 'null'), (dict(a=None), 'null')):
        c = CC.Case(entry, **kw)
        assert c.run(lib) == -1 and word in lib.bfd_last_error().decode() and c.untouched(), kw
    if entry == 'bfd_voxelize_scatter3d':
        nan = CC.Case(entry).tri.copy()
        nan[0, 2, 1] = np.nan
        for kw, word in ((dict(nTri=0), 'triangle'), (dict(tri=nan), 'vertex'), (dict(b=np.array([4.0, 1e-320, 8.0]), grid=(4, 2 ** 20, 8)), 'voxel size')):
            c = CC.Case(entry, **kw)
            assert c.run(lib) == -1 and word in lib.bfd_last_error().decode() and c.untouched(), kw
    # the bounds pass ignores M; counts alone, or the bounds alone, are an output
    for kw in (dict(want_out=False, M=(0, -1, 2 ** 40)), dict(want_out=False, want_lo=False, want_hi=False), dict(want_out=False, want_counts=False)):
        c = CC.Case(entry, **kw)
        rc = c.run(lib)
        assert rc == (-3 if lib.bfd_device_count() == 0 else 0), (kw, lib.bfd_last_error().decode())
    if lib.bfd_device_count() == 0:
        for empty in (False, True):
            c = CC.Case(entry, empty=empty)
            assert c.run(lib) == -3 and c.untouched()


# ---------------------------------------------------------------- conformal_masks ----------------------------------------------------------------

class HostDevice:
    """Stands in for ConformalMask._run where there is no device: the oracle's voxelisation and the restatement of the scatter, through the same
    arguments the device call takes. What is tested is the flow of conformal_masks around its calls."""

    def __init__(self):
        self.calls = []

    def __call__(self, src, m, shape, want_bounds):
        kind, tri, g, lo, hi = src
        assert kind == 'mesh'
        unit = VO.unit_of(lo, hi, g)
        pts = VO.points_of(VO.voxelize(tri, lo, hi, g), lo, unit)
        out, plo, phi, counts = CO.scatter(pts, m, shape)
        self.calls.append((shape, want_bounds))
        CM.last_kernel_ms, CM.last_counts = 0.5, counts
        return out, (plo if want_bounds else None), (phi if want_bounds else None), counts


def nested_boxes(seed):
    r = VO.rotation(seed).T
    boxes = [VO.box_triangles((-h, -h * 1.25, -h * 0.75), (h, h * 1.25, h * 0.75)).astype(np.float64) for h in (4.0, 3.0, 2.0)]
    return [((b @ r) + np.array([10.0, -5.0, 3.0])).astype(np.float32) for b in boxes]


@pytest.mark.parametrize('seed,location', [(31, (10.5, -5.25, 3.0)), (32, (22.0, 6.0, 14.0))])
def test_conformal_masks_follow_the_reference(monkeypatch, seed, location):
    """Three tiny nested boxes; the focal point inside the skin, and far outside it (it then sets the mask's shape and a voxel of the skin mask)."""
    host = HostDevice()
    monkeypatch.setattr(CM, '_run', host)
    skin, skull, csf = nested_boxes(seed)
    step, R = 1.0, VO.rotation(seed + 100)
    got = CM.conformal_masks(skin, skull, csf, step, R, location)
    assert host.calls[:2] == [(None, True), (None, True)] and len(host.calls) == 5 and CM.last_kernel_ms == 2.5
    pts = []
    for tri in (skin, skull, csf):
        lo, hi = VO.bounds_of(tri)
        g = tuple(int(np.ceil(d / (0.75 * step))) for d in hi - lo)
        pts.append(VO.points_of(VO.voxelize(tri, lo, hi, g), lo, VO.unit_of(lo, hi, g)))
    want = CO.conformal_flow(pts[0], pts[1], pts[2], step, R, location)
    assert [x.dtype for x in got] == [np.float64, np.int64, np.int8, np.int8, np.uint8]
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
    assert got[2].sum() > got[3].sum() > got[4].sum() > 0 and got[2][tuple(got[1])] == 1
    # the restatement of the flow against the reference's own expressions, np.dot included, on the same points: the same masks unless a point sits
    # within rounding of a half-integer (none does here)
    inv = np.linalg.inv(got[0]).astype(np.float32)
    xyz = np.hstack([pts[1], np.ones((len(pts[1]), 1), np.float32)]).T
    ijk = np.round(np.dot(inv, xyz)).astype(np.int64).T
    ijk = ijk[(ijk[:, 0] < got[3].shape[0]) & (ijk[:, 1] < got[3].shape[1]) & (ijk[:, 2] < got[3].shape[2])]
    ref = np.zeros_like(got[2])
    ref[ijk[:, 0], ijk[:, 1], ijk[:, 2]] = 1
    assert np.array_equal(ref, got[3])
