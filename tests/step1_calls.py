"""The smallest valid call of each of the eight Step-1 entries of the C ABI, for the tests of the call contract they share (csrc/bfd_call.h):
a 4 x 4 x 4 volume, one triangle on a 4 x 4 x 4 grid, a 4-word table, a two-row value table. A case owns its arrays; every output and kernelMs start
as sentinels, so a test sees whether the library touched them."""
import ctypes as C

import numpy as np

from babelbrain_amd import _engine

ENTRIES = ('bfd_median_filter3d', 'bfd_binary_morphology3d', 'bfd_label3d', 'bfd_affine_transform3d', 'bfd_spline_filter3d',
           'bfd_voxelize_mesh', 'bfd_voxel_points', 'bfd_map_values3d')
# entries that admit an empty problem: an N1 = 0 volume, N = 0 for the value map, a table without a set voxel
ADMIT_EMPTY = tuple(e for e in ENTRIES if e != 'bfd_voxelize_mesh')
MS_SENTINEL = -1.0
P = _engine._ptr


def _i64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


class Case:
    """args(device): the argument tuple; outputs: name -> array the entry may write; ms: kernelMs (two floats, the second used by the affine map)"""

    def __init__(self, entry, empty=False):
        self.entry, self.empty = entry, empty
        self.ms = np.full(2, MS_SENTINEL, np.float32)
        rng = np.random.default_rng(ENTRIES.index(entry))
        n1 = 0 if empty else 4
        shape = (n1, 4, 4)
        vol = (rng.random((4, 4, 4)) < 0.5).astype(np.uint8)[:n1].copy()
        ms = self.ms.ctypes.data_as(C.POINTER(C.c_float))
        keep = self.inputs = [vol]
        if entry == 'bfd_median_filter3d':
            out = np.full(shape, 7, np.uint8)
            self.outputs = {'out': out}
            # an empty axis takes size 1: a larger window is refused where the axis is shorter than size / 2
            self.args = lambda d: (d, 0, P(vol), P(out), None, n1, 4, 4, 1 if empty else 3, 3, 3, 0, 0.0, ms)
        elif entry == 'bfd_binary_morphology3d':
            out = np.full(shape, 7, np.uint8)
            self.outputs = {'out': out}
            self.args = lambda d: (d, 2, P(vol), P(out), n1, 4, 4, None, 3, 3, 3, 1, 0, ms)
        elif entry == 'bfd_label3d':
            self.outputs = {'labels': np.full(shape, -7, np.int32), 'numLabels': np.full(1, -7, np.int64), 'sizes': np.full(64, -7, np.int64),
                            'largest': np.full(shape, 7, np.uint8)}
            o = self.outputs
            self.args = lambda d: (d, P(vol), P(o['labels']), n1, 4, 4, 3, _i64(o['numLabels']), P(o['sizes']), 64, P(o['largest']), ms)
        elif entry == 'bfd_affine_transform3d':
            src = rng.standard_normal((4, 4, 4)).astype(np.float32)[:n1].copy()
            out = np.full(shape, 7, np.float32)
            matrix = np.hstack([np.eye(3), np.full((3, 1), 0.25)])
            keep += [src, matrix]
            self.outputs = {'out': out}
            self.args = lambda d: (d, 1, P(src), P(out), n1, 4, 4, n1, 4, 4, P(matrix), 3, 0, 0.0, 1, P(self.ms))
        elif entry == 'bfd_spline_filter3d':
            src = rng.standard_normal((4, 4, 4)).astype(np.float32)[:n1].copy()
            out = np.full(shape, 7, np.float64)
            keep += [src]
            self.outputs = {'out': out}
            self.args = lambda d: (d, 1, P(src), P(out), n1, 4, 4, 3, 2, ms)
        elif entry == 'bfd_voxelize_mesh':
            # the plane x = 2.2 over part of the grid: the voxels below it in the columns whose centre it covers
            tri = np.array([[[2.2, 0.2, 0.2], [2.2, 3.9, 0.2], [2.2, 0.2, 3.9]]], np.float32)
            lo, hi = np.zeros(3), np.full(3, 4.0)
            keep += [tri, lo, hi]
            self.outputs = {'table': np.full(2, 0x07070707, np.uint32), 'mask': np.full((4, 4, 4), 7, np.uint8), 'count': np.full(1, -7, np.int64)}
            o = self.outputs
            self.args = lambda d: (d, P(tri), 1, P(lo), P(hi), 4, 4, 4, P(o['table']), P(o['mask']), _i64(o['count']), ms)
        elif entry == 'bfd_voxel_points':
            table = np.zeros(4, np.uint32) if empty else rng.integers(0, 1 << 32, 4, dtype=np.uint64).astype(np.uint32)       # 4 x 4 x 8 voxels
            total = sum(bin(int(w)).count('1') for w in table)
            lo, unit = np.zeros(3), np.full(3, 0.5)
            keep += [table, lo, unit]
            # count is written with the population before a device is looked for (it comes with the refusal of a small capacity): no sentinel there
            self.count = np.full(1, -7, np.int64)
            self.outputs = {'points': np.full((max(total, 1), 3), 7, np.float32)}
            self.args = lambda d: (d, P(table), 4, 4, 8, P(lo), P(unit), P(self.outputs['points']), total, _i64(self.count), ms)
        elif entry == 'bfd_map_values3d':
            uni = np.array([-1.5, 2.0], np.float32)
            n = 0 if empty else 64
            hu = uni[rng.integers(0, 2, 64)]
            hu[::5] = 3.0
            sel = (rng.random(64) < 0.7).astype(np.uint8)
            out = np.full(64, 7, np.uint32)
            keep += [uni, hu, sel]
            self.outputs = {'out': out}
            self.args = lambda d: (d, P(hu), P(sel), P(uni), 2, P(out), n, ms)
        else:
            raise KeyError(entry)
        self.pristine = self.snapshot()

    def run(self, lib, device):
        return getattr(lib, self.entry)(*self.args(device))

    def snapshot(self):
        return {k: v.copy() for k, v in self.outputs.items()}

    def untouched(self):
        """outputs and kernelMs as they were made"""
        return all(np.array_equal(v, self.pristine[k]) for k, v in self.outputs.items()) and np.all(self.ms == np.float32(MS_SENTINEL))
