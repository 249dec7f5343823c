"""The smallest valid calls of the two conformal-mask entries (bfd_voxel_scatter3d, bfd_voxelize_scatter3d) for the tests of the Step-1 call contract
(csrc/bfd_call.h), in the manner of tests/step1_calls.py: a case owns its arrays; every output and kernelMs start as sentinels, so a test sees whether
the library touched them. `faults` are the argument errors of include/babelfdtd.h in the order the header lists them: (name, word of the message,
keyword arguments that plant the fault)."""
import ctypes as C

import numpy as np

from babelbrain_amd import _engine

ENTRIES = ('bfd_voxel_scatter3d', 'bfd_voxelize_scatter3d')
MS_SENTINEL = -1.0
P = _engine._ptr


class Case:
    """4 x 4 x 8 source voxels into a 5 x 6 x 7 volume under a half-step matrix. Keyword arguments replace arguments of the valid call."""

    def __init__(self, entry, empty=False, **kw):
        self.entry = entry
        rng = np.random.default_rng(ENTRIES.index(entry))
        self.ms = np.full(1, MS_SENTINEL, np.float32)
        self.matrix = np.array([[0.5, 0, 0, 1], [0, 0.5, 0, 2], [0, 0, 0.5, 1]], np.float32)
        self.M = (5, 6, 7)
        self.grid = (4, 4, 8)
        self.outputs = {'out': np.full(self.M, 7, np.uint8), 'lo': np.full(3, -7, np.int64), 'hi': np.full(3, -7, np.int64),
                        'counts': np.full(4, -7, np.int64)}
        if entry == 'bfd_voxel_scatter3d':
            self.table = np.zeros(4, np.uint32) if empty else rng.integers(0, 1 << 32, 4, dtype=np.uint64).astype(np.uint32)
            self.a, self.b = np.zeros(3), np.full(3, 0.5)                       # min, unit
        else:
            # the plane x = 2.2 over part of the grid, as tests/step1_calls.py has it; empty: a plane below the first voxel centre sets nothing
            x = 0.1 if empty else 2.2
            self.tri = np.array([[[x, 0.2, 0.2], [x, 3.9, 0.2], [x, 0.2, 3.9]]], np.float32)
            self.nTri = 1
            self.a, self.b = np.zeros(3), np.array([4.0, 4.0, 8.0])             # min, max: unit 1
        self.want = dict(out=True, lo=True, hi=True, counts=True)
        for k, v in kw.items():
            if k.startswith('want_'):
                self.want[k[5:]] = v
            else:
                assert hasattr(self, k), k
                setattr(self, k, v)
        self.pristine = self.snapshot()

    def args(self, device):
        o = {k: (P(v) if self.want[k] else None) for k, v in self.outputs.items()}
        g, M = self.grid, self.M
        tail = (P(self.matrix), M[0], M[1], M[2], o['out'], o['lo'], o['hi'], o['counts'], self.ms.ctypes.data_as(C.POINTER(C.c_float)))
        if self.entry == 'bfd_voxel_scatter3d':
            return (device, P(self.table), g[0], g[1], g[2], P(self.a), P(self.b)) + tail
        return (device, P(self.tri), self.nTri, P(self.a), P(self.b), g[0], g[1], g[2]) + tail

    def run(self, lib, device=0):
        return getattr(lib, self.entry)(*self.args(device))

    def snapshot(self):
        return {k: v.copy() for k, v in self.outputs.items()}

    def untouched(self):
        return all(np.array_equal(v, self.pristine[k]) for k, v in self.outputs.items()) and np.all(self.ms == np.float32(MS_SENTINEL))


def _bad_matrix():
    return np.array([[0.5, 0, 0, 1], [0, 0.5, np.inf, 2], [0, 0, 0.5, 1]], np.float32)


def faults(entry):
    """The -1 refusals in the header's order. The overlap is planted by handing the matrix's own bytes as `out` (M = 6 x 4 x 2 = 48 bytes)."""
    if entry == 'bfd_voxel_scatter3d':
        first = [('grid', 'grid', dict(grid=(4, 0, 8))), ('box', 'min and unit', dict(b=np.array([0.5, np.nan, 0.5])))]
    else:
        first = [('grid', 'grid', dict(grid=(4, 0, 8))), ('box', 'max > min', dict(b=np.array([4.0, 0.0, 8.0])))]
    return first + [
        ('matrix', 'matrix', dict(matrix=_bad_matrix())),
        ('extent', 'extent of out', dict(M=(5, 0, 7))),
        ('size', 'out has 2^31', dict(M=(2048, 1024, 1024))),
        ('overlap', 'alias', 'overlap'),
        ('none', 'no output', dict(want_out=False, want_lo=False, want_hi=False, want_counts=False)),
    ]


def planted(entry, names):
    """A case with the named faults planted together: the library must report the one the header lists first."""
    table = dict((n, kw) for n, _, kw in faults(entry))
    kw = {}
    overlap = False
    for n in names:
        if table[n] == 'overlap':
            overlap = True
        else:
            kw.update(table[n])
    if 'extent' in names and 'size' in names:
        kw['M'] = (2 ** 31, 0, 1)
    c = Case(entry, **kw)
    if overlap:
        if 'M' not in kw:
            c.M = (6, 4, 2)
        c.outputs['out'] = c.matrix.view(np.uint8).reshape(6, 4, 2)
        c.pristine = c.snapshot()
    return c


def ordered_plants(entry):
    """[(names planted together, the name that must be reported)]: every fault alone, with every later one, and the argument faults with 'no output'
    (which silences the checks of `out`, so it is not planted beside them)."""
    names = [n for n, _, _ in faults(entry)]
    combos = [([n], n) for n in names]
    combos += [(names[i:-1], names[i]) for i in range(len(names) - 2)]
    combos += [([n, 'none'], n) for n in names[:3]]
    return combos
