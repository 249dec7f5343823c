"""The smallest valid calls of the three domain entries (bfd_label_survey3d, bfd_assemble_material_map3d, bfd_sdr_rays3d) for the tests of the Step-1
call contract (csrc/bfd_call.h), in the manner of tests/tissue_calls.py: a case owns its arrays; every output and kernelMs start as sentinels, so a
test sees whether the library touched them. `faults` are the argument errors of include/babelfdtd.h in the order the header lists them: (name, word
of the message, keyword arguments that plant the fault). survey / assemble / rays are the plain calls the device tests compare with the oracle."""
import ctypes as C

import numpy as np

from babelbrain_amd import _engine

ENTRIES = ('bfd_label_survey3d', 'bfd_assemble_material_map3d', 'bfd_sdr_rays3d')
MS_SENTINEL = -1.0
P = _engine._ptr


def i64(v):
    return np.array(v, np.int64)


class Case:
    """A 3 x 4 x 9 volume. Keyword arguments replace arguments of the valid call; want_<output>=False hands NULL for it, <input>=None for an input."""

    def __init__(self, entry, **kw):
        self.entry = entry
        rng = np.random.default_rng(ENTRIES.index(entry))
        self.ms = np.full(1, MS_SENTINEL, np.float32)
        self.M = (3, 4, 9)
        self.labels = rng.integers(0, 5, self.M).astype(np.uint8)
        self.labels[1, 2, 3] = 5
        self.flipK = 1
        self.lo, self.hi = i64([0, 1, 2]), i64([3, 4, 8])
        if entry == 'bfd_label_survey3d':
            self.outputs = {'hist': np.full(256, -7, np.int64), 'bounds': np.full(6, -7, np.int64), 'focal': np.full(2, -7, np.int64)}
        elif entry == 'bfd_assemble_material_map3d':
            self.ct = rng.integers(1, 9, self.M).astype(np.uint32)
            self.ctBytes = 4
            self.air = rng.integers(0, 2, self.M).astype(np.uint8)
            self.size, self.padLo, self.padHi = self.hi - self.lo, i64([1, 0, 2]), i64([0, 2, 1])
            self.lut = np.arange(256, dtype=np.uint32)
            self.lut[2:4] |= np.uint32(1 << 31)
            self.ctOffset, self.zWater, self.nMaterials, self.focalIJ = 3, 2, 12, i64([2, 1])
            N = tuple(self.size + self.padLo + self.padHi)
            self.outputs = {'map': np.full(N, 77, np.uint32), 'mapNoCT': np.full(N, 77, np.uint32), 'airOut': np.full(N, 77, np.uint32),
                            'stats': np.full(8, -7, np.int64)}
        else:
            self.ct = rng.integers(0, 6, self.M).astype(np.uint32)
            self.ctBytes = 4
            self.size = self.hi - self.lo
            self.hu = np.linspace(-50, 900, 6).astype(np.float32)
            self.huBytes, self.nHU = 4, 6
            self.stepI, self.stepJ, self.minSkull, self.centerRegion = 1, 2, 2, 0.5
            self.outputs = {'value': np.full((3, 2), -7, np.float32), 'count': np.full((3, 2), -7, np.int32), 'state': np.full((3, 2), 77, np.uint8)}
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
        M = self.M
        ms = self.ms.ctypes.data_as(C.POINTER(C.c_float))
        if self.entry == 'bfd_label_survey3d':
            return (device, P(self.labels), M[0], M[1], M[2], P(self.lo), P(self.hi), self.flipK, o['hist'], o['bounds'], o['focal'], ms)
        if self.entry == 'bfd_assemble_material_map3d':
            return (device, P(self.labels), P(self.ct), self.ctBytes, P(self.air), M[0], M[1], M[2], P(self.lo), P(self.size), P(self.padLo), P(self.padHi),
                    self.flipK, P(self.lut), self.ctOffset, self.zWater, self.nMaterials, P(self.focalIJ), o['map'], o['mapNoCT'], o['airOut'], o['stats'], ms)
        return (device, P(self.ct), self.ctBytes, M[0], M[1], M[2], P(self.lo), P(self.size), self.flipK, P(self.hu), self.huBytes, self.nHU, self.stepI,
                self.stepJ, self.minSkull, self.centerRegion, o['value'], o['count'], o['state'], ms)

    def run(self, lib, device=0):
        return getattr(lib, self.entry)(*self.args(device))

    def snapshot(self):
        return {k: v.copy() for k, v in self.outputs.items()}

    def untouched(self, but_ms=False):
        same = all(np.array_equal(v, self.pristine[k]) for k, v in self.outputs.items())
        return same and (but_ms or np.all(self.ms == np.float32(MS_SENTINEL)))


def faults(entry):
    """The -1 refusals that come before a device is looked for, in the header's order. 'overlap' hands an input's own bytes as an output."""
    head = [('negative', 'negative', dict(M=(3, -4, 9))), ('size', '2^31', dict(M=(2048, 1024, 1024)))]
    if entry == 'bfd_label_survey3d':
        return [('null', 'null', dict(labels=None))] + head + [('box', 'box', dict(hi=i64([3, 5, 8]))), ('flip', 'flipK', dict(flipK=2))]
    if entry == 'bfd_assemble_material_map3d':
        return [('null', 'null', dict(lut=None))] + head + [
            ('ctBytes', 'ctBytes', dict(ctBytes=3)), ('box', 'box', dict(lo=i64([0, 1, 4]))), ('padding', 'padding', dict(padHi=i64([0, -1, 1]))),
            ('map', 'the map has 2^31', dict(padLo=i64([2 ** 20, 2 ** 10, 1]))), ('flip', 'flipK', dict(flipK=-1)),
            ('lut', 'no ct', dict(ct=None, ctBytes=0)), ('zWater', 'zWater', dict(zWater=-2)), ('materials', 'nMaterials', dict(nMaterials=2 ** 32)), ('focal', 'focalIJ', dict(focalIJ=i64([4, 1]))),
            ('overlap', 'alias', 'overlap')]
    return [('null', 'null', dict(ct=None))] + head + [
        ('ctBytes', 'ctBytes', dict(ctBytes=1)), ('box', 'box', dict(size=i64([3, 4, 6]))), ('flip', 'flipK', dict(flipK=2)),
        ('huBytes', 'huBytes', dict(huBytes=2)), ('nHU', 'nHU', dict(nHU=0)), ('finite', 'finite', dict(hu=np.array([0, 1, np.inf, 3, 4, 5], np.float32))),
        ('step', 'stepI', dict(stepJ=0)), ('minSkull', 'minSkullVoxels', dict(minSkull=0)), ('center', 'centerRegion', dict(centerRegion=-0.5))]


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
        kw['M'] = (2 ** 31, -1, 1)
    c = Case(entry, **kw)
    if overlap:                                   # the map's 4 x 5 x 9 voxels begin on the CT's own bytes
        shape = c.outputs['map'].shape
        big = np.zeros(int(np.prod(shape)), np.uint32)
        big[:c.ct.size] = c.ct.ravel()
        c.ct = big[:c.ct.size].reshape(c.M)
        c.outputs['map'] = big.reshape(shape)
        c.pristine = c.snapshot()
    return c


def ordered_plants(entry):
    """[(names planted together, the name that must be reported)]: every fault alone, and each with all the later ones that leave the volume's size
    and the box alone (the overlap and the focal column are looked for with the true sizes only)."""
    names = [n for n, _, _ in faults(entry)]
    combos = [([n], n) for n in names]
    tail = [n for n in names[3:] if n not in ('overlap', 'map', 'padding', 'box', 'focal', 'lut')]
    combos += [([names[i]] + [n for n in tail if names.index(n) > i], names[i]) for i in range(len(names) - 1) if names[i] not in ('overlap',)]
    combos += [(['null', 'negative', 'size'], 'null'), (['negative', 'size'], 'negative')]
    return combos


# ---------------------------------------------------------------- plain calls ----------------------------------------------------------------

def check(lib, rc):
    assert rc == 0, lib.bfd_last_error().decode()


def survey(lib, labels, lo, hi, flipK, device=0):
    hist, bounds, focal, ms = np.zeros(256, np.int64), np.zeros(6, np.int64), np.zeros(2, np.int64), C.c_float(-1)
    check(lib, lib.bfd_label_survey3d(device, P(labels), *labels.shape, P(i64(lo)), P(i64(hi)), int(flipK), P(hist), P(bounds), P(focal), C.byref(ms)))
    return hist, bounds, focal, ms.value


def assemble(lib, labels, ct, air, lo, size, padLo, padHi, flipK, lut, ctOffset, zWater, nMaterials, focalIJ, want_noct=True, want_air=True, device=0):
    N = tuple(int(s + a + b) for s, a, b in zip(size, padLo, padHi))
    out = np.full(N, 0xDEAD, np.uint32)
    noct = np.full(N, 0xDEAD, np.uint32) if want_noct else None
    airOut = np.full(N, 0xDEAD, np.uint32) if want_air else None
    stats, ms = np.zeros(8, np.int64), C.c_float(-1)
    keep = [i64(lo), i64(size), i64(padLo), i64(padHi), np.ascontiguousarray(lut, np.uint32), i64(focalIJ)]
    check(lib, lib.bfd_assemble_material_map3d(device, P(labels), P(ct), 0 if ct is None else ct.itemsize, P(air), *labels.shape, P(keep[0]), P(keep[1]),
                                               P(keep[2]), P(keep[3]), int(flipK), P(keep[4]), int(ctOffset), int(zWater), int(nMaterials), P(keep[5]),
                                               P(out), P(noct), P(airOut), P(stats), C.byref(ms)))
    return out, noct, airOut, stats, ms.value


def rays(lib, ct, hu, lo, hi, flipK, stepI, stepJ, minSkull, centerRegion, device=0):
    size = i64(hi) - i64(lo)
    lattice = (-(-int(size[0]) // stepI), -(-int(size[1]) // stepJ))
    value, count, state, ms = np.full(lattice, -7, hu.dtype), np.full(lattice, -7, np.int32), np.full(lattice, 77, np.uint8), C.c_float(-1)
    keep = i64(lo)
    check(lib, lib.bfd_sdr_rays3d(device, P(ct), ct.itemsize, *ct.shape, P(keep), P(size), int(flipK), P(hu), hu.itemsize, hu.size, stepI, stepJ, minSkull,
                                  float(centerRegion), P(value), P(count), P(state), C.byref(ms)))
    return value, count, state, ms.value
