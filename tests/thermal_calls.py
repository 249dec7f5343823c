"""The smallest valid calls of the two exposure-analysis entries (bfd_class_extrema3d, bfd_loss_survey3d) for the tests of the Step-1 call contract
(csrc/bfd_call.h), in the manner of tests/tissue_calls.py: a case owns its arrays; every output and kernelMs start as sentinels, so a test sees
whether the library touched them. `faults` are the argument errors of include/babelfdtd.h in the order the header lists them: (name, word of the
message, keyword arguments that plant the fault)."""
import ctypes as C

import numpy as np

from babelbrain_amd import _engine

ENTRIES = ('bfd_class_extrema3d', 'bfd_loss_survey3d')
MS_SENTINEL = -1.0
P = _engine._ptr


class Case:
    """A 3 x 4 x 9 volume over 5 materials. Keyword arguments replace arguments of the valid call; want_<output>=False hands NULL for it."""

    def __init__(self, entry, **kw):
        self.entry = entry
        rng = np.random.default_rng(ENTRIES.index(entry) + 20)
        self.ms = np.full(1, MS_SENTINEL, np.float32)
        self.N = (3, 4, 9)
        self.idBytes, self.nMat = 4, 5
        self.map = rng.integers(0, 5, self.N).astype(np.uint32)
        self.classOf = np.array([2, 4, 8, 8, 1 | 16], np.uint8)
        self.map_given = self.table_given = True
        if entry == 'bfd_class_extrema3d':
            self.nVol = 2
            self.vols = [rng.normal(40, 3, self.N).astype(np.float32) for _ in range(2)]
            self.vols_given = True
            self.null_volume = None
            self.outputs = {'count': np.full(8, -7, np.int64), 'maxIn': np.full((2, 8), -7, np.float32), 'argIn': np.full((2, 8), -7, np.int64),
                            'maxKey': np.full((2, 8), -7, np.float32), 'argKey': np.full((2, 8), -7, np.int64)}
        else:
            self.nFields = 2
            self.p = rng.uniform(1e4, 3e5, (2,) + self.N).astype(np.float32)
            self.pw = rng.uniform(1e4, 6e5, (2,) + self.N).astype(np.float32)
            self.p_given = self.rho_given = True
            self.mask = None
            self.rho = np.array([1000.0, 1100.0, 1900.0, 1700.0, 1040.0])
            self.c = np.array([1500.0, 1610.0, 2800.0, 2300.0, 1560.0])
            self.rhoWater, self.cWater, self.dx2 = 1000.0, 1500.0, 0.25e-6
            self.outputs = {'maxTissue': np.full(2, -7, np.float32), 'argTissue': np.full(2, -7, np.int64), 'maxWater': np.full(2, -7, np.float32),
                            'argWater': np.full(2, -7, np.int64), 'eWaterRaw': np.full((2, 9), -7.0), 'eWater': np.full((2, 9), -7.0),
                            'eTissue': np.full((2, 9), -7.0), 'waterOut': np.full((2,) + self.N, -7, np.float32)}
        self.want = {k: True for k in self.outputs}
        for k, v in kw.items():
            if k.startswith('want_'):
                self.want[k[5:]] = v
            else:
                assert hasattr(self, k), k
                setattr(self, k, v)
        self.pristine = self.snapshot()

    def args(self, device):
        o = {k: (P(v) if self.want[k] else None) for k, v in self.outputs.items()}
        N = self.N
        ms = self.ms.ctypes.data_as(C.POINTER(C.c_float))
        m = P(self.map) if self.map_given else None
        t = P(self.classOf) if self.table_given else None
        if self.entry == 'bfd_class_extrema3d':
            self.ptrs = (C.c_void_p * max(len(self.vols), 1))(*[None if q == self.null_volume else v.ctypes.data for q, v in enumerate(self.vols)])
            return (device, C.cast(self.ptrs, C.c_void_p) if self.vols_given else None, self.nVol, m, self.idBytes, N[0], N[1], N[2], t, self.nMat, o['count'],
                    o['maxIn'], o['argIn'], o['maxKey'], o['argKey'], ms)
        return (device, P(self.p) if self.p_given else None, P(self.pw), self.nFields, m, self.idBytes, N[0], N[1], N[2], t, self.nMat, P(self.mask),
                P(self.rho) if self.rho_given else None, P(self.c), self.rhoWater, self.cWater, self.dx2, o['maxTissue'], o['argTissue'], o['maxWater'],
                o['argWater'], o['eWaterRaw'], o['eWater'], o['eTissue'], o['waterOut'], ms)

    def run(self, lib, device=0):
        return getattr(lib, self.entry)(*self.args(device))

    def snapshot(self):
        return {k: v.copy() for k, v in self.outputs.items()}

    def untouched(self, but_ms=False):
        same = all(np.array_equal(v, self.pristine[k]) for k, v in self.outputs.items())
        return same and (but_ms or np.all(self.ms == np.float32(MS_SENTINEL)))


def required(entry):
    """the outputs that may not be NULL"""
    return [k for k in Case(entry).outputs if k != 'waterOut']


def faults(entry):
    """The -1 refusals that come before a device is looked for, in the header's order. 'overlap' hands an input's own bytes as an output."""
    shared = [('negative', 'negative', dict(N=(3, -4, 9))), ('size', '2^31', dict(N=(2048, 1024, 1024))), ('idBytes', 'idBytes', dict(idBytes=3)),
              ('nMat', 'nMat', dict(nMat=65537))]
    if entry == 'bfd_class_extrema3d':
        return [('null', 'null', dict(map_given=False))] + shared + [('nVol', 'nVol', dict(nVol=0)), ('volume', 'null', dict(null_volume=1)),
                                                                     ('overlap', 'alias', 'overlap')]
    bad = np.array([1000.0, 1100.0, -1.0, 1700.0, 1040.0])
    return [('null', 'null', dict(rho_given=False))] + shared + [('nFields', 'nFields', dict(nFields=0)), ('water', 'rhoWater', dict(cWater=np.inf)),
                                                                 ('rho', 'every rho', dict(c=bad)), ('dx2', 'dx2', dict(dx2=-1e-6)),
                                                                 ('overlap', 'alias', 'overlap')]


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
    if 'negative' in names and 'size' in names:
        kw['N'] = (2 ** 31, -1, 1)
    c = Case(entry, **kw)
    if overlap:
        if entry == 'bfd_class_extrema3d':
            c.outputs['maxIn'] = c.vols[1].reshape(-1)[:16].reshape(2, 8)
        else:
            c.outputs['eWater'] = np.frombuffer(c.p, np.float64, 18).reshape(2, 9)
        c.pristine = c.snapshot()
    return c


def ordered_plants(entry):
    """[(names planted together, the name that must be reported)]: every fault alone, and each with all the later ones. The overlap is looked for
    with the volume's true size only, so it is planted alone or beside faults that leave the size and the counts alone."""
    names = [n for n, _, _ in faults(entry)]
    combos = [([n], n) for n in names]
    combos += [(names[i:-1], names[i]) for i in range(len(names) - 2)]
    combos += [([n, 'overlap'], n) for n in names[3:-1] if n not in ('nVol', 'nFields', 'volume')]
    return combos
