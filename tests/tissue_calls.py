"""The smallest valid calls of the three tissue-mask entries (bfd_paint_components3d, bfd_quantize_values3d, bfd_clear_beyond_bone3d) for the tests of
the Step-1 call contract (csrc/bfd_call.h), in the manner of tests/conformal_calls.py: a case owns its arrays; every output and kernelMs start as
sentinels, so a test sees whether the library touched them. `faults` are the argument errors of include/babelfdtd.h in the order the header lists
them: (name, word of the message, keyword arguments that plant the fault)."""
import ctypes as C

import numpy as np

from babelbrain_amd import _engine

ENTRIES = ('bfd_paint_components3d', 'bfd_quantize_values3d', 'bfd_clear_beyond_bone3d')
MS_SENTINEL = -1.0
P = _engine._ptr


class Case:
    """A 3 x 4 x 9 volume. Keyword arguments replace arguments of the valid call; want_<output>=False hands NULL for it."""

    def __init__(self, entry, **kw):
        self.entry = entry
        rng = np.random.default_rng(ENTRIES.index(entry))
        self.ms = np.full(1, MS_SENTINEL, np.float32)
        self.N = (3, 4, 9)
        self.vol = rng.integers(0, 5, self.N).astype(np.uint8)
        self.vol[0, 0, 0] = 1
        self.want = {}
        if entry == 'bfd_paint_components3d':
            self.value, self.connectivity, self.select, self.fill = 1, 3, 0, 4
            self.outputs = {'out': np.full(self.N, 7, np.uint8), 'counts': np.full(4, -7, np.int64)}
        elif entry == 'bfd_quantize_values3d':
            self.values = rng.normal(0, 100, self.N).astype(np.float32)
            self.vol = (self.vol > 1).astype(np.uint8)
            self.vol[0, 0, :2] = 1
            self.bits = 4
            self.outputs = {'quantized': np.full(self.N, -7, np.float32), 'map': np.full(self.N, 77, np.uint32), 'table': np.full(16, -7, np.float32),
                            'numValues': np.full(1, -7, np.int64), 'range': np.full(2, -7, np.float32)}
        else:
            self.kFocal, self.boneA, self.boneB, self.from_, self.to = 2, 2, 3, 4, 1
            self.outputs = {'out': np.full(self.N, 7, np.uint8), 'counts': np.full(2, -7, np.int64)}
        self.want = {k: True for k in self.outputs}
        self.in_ = True
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
        vol = P(self.vol) if self.in_ else None
        if self.entry == 'bfd_paint_components3d':
            return (device, vol, o['out'], N[0], N[1], N[2], self.value, self.connectivity, self.select, self.fill, o['counts'], ms)
        if self.entry == 'bfd_quantize_values3d':
            return (device, P(self.values), vol, N[0], N[1], N[2], self.bits, o['quantized'], o['map'], o['table'],
                    self.outputs['numValues'].ctypes.data_as(C.POINTER(C.c_int64)) if self.want['numValues'] else None, o['range'], ms)
        return (device, vol, o['out'], N[0], N[1], N[2], self.kFocal, self.boneA, self.boneB, self.from_, self.to, o['counts'], ms)

    def run(self, lib, device=0):
        return getattr(lib, self.entry)(*self.args(device))

    def snapshot(self):
        return {k: v.copy() for k, v in self.outputs.items()}

    def untouched(self, but_ms=False):
        same = all(np.array_equal(v, self.pristine[k]) for k, v in self.outputs.items())
        return same and (but_ms or np.all(self.ms == np.float32(MS_SENTINEL)))


def faults(entry):
    """The -1 refusals that come before a device is looked for, in the header's order. 'overlap' hands the input's own bytes as an output."""
    head = [('null', 'null', dict(in_=False)), ('negative', 'negative', dict(N=(3, -4, 9))), ('size', '2^31', dict(N=(2048, 1024, 1024)))]
    if entry == 'bfd_paint_components3d':
        return head + [('byte', 'uint8', dict(fill=256)), ('connectivity', 'connectivity', dict(connectivity=4)), ('select', 'select', dict(select=3)),
                       ('overlap', 'alias', 'overlap')]
    if entry == 'bfd_quantize_values3d':
        return head + [('bits', 'bits', dict(bits=17)), ('overlap', 'alias', 'overlap')]
    return head + [('kFocal', 'kFocal', dict(kFocal=9)), ('byte', 'uint8', dict(boneB=-1)), ('overlap', 'alias', 'overlap')]


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
        if entry == 'bfd_quantize_values3d':
            c.outputs['map'] = c.values.view(np.uint32)
        else:
            c.outputs['out'] = c.vol
        c.pristine = c.snapshot()
    return c


def ordered_plants(entry):
    """[(names planted together, the name that must be reported)]: every fault alone, and each with all the later ones. The overlap is looked for
    with the volume's true size only, so it is planted alone or beside faults that leave the size alone."""
    names = [n for n, _, _ in faults(entry)]
    combos = [([n], n) for n in names]
    combos += [(names[i:-1], names[i]) for i in range(len(names) - 2)]
    combos += [([n, 'overlap'], n) for n in names[3:-1]]
    return combos
