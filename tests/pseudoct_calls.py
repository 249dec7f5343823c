"""The smallest valid calls of the six pseudo-CT entries (the five of csrc/bfd_pseudoct.hip and bfd_select_component3d) for the tests of the
Step-1 call contract (csrc/bfd_call.h), in the manner of tests/tissue_calls.py: a case owns its arrays; every output and kernelMs start as
sentinels, so a test sees whether the library touched them. `faults` are the argument errors of include/babelfdtd.h in the order the header lists
them: (name, word of the message, keyword arguments that plant the fault)."""
import ctypes as C

import numpy as np

from babelbrain_amd import _engine

ENTRIES = ('bfd_integer_histogram3d', 'bfd_order_statistics3d', 'bfd_uniform_histogram3d', 'bfd_pseudo_ct_candidates3d', 'bfd_pseudo_ct_convert3d',
           'bfd_select_component3d')
DATA_ENTRIES = ENTRIES[:4]                        # the entries that refuse data as well
MS_SENTINEL = -1.0
P = _engine._ptr


def I64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


class Case:
    """A 3 x 4 x 9 volume. Keyword arguments replace arguments of the valid call; want_<output>=False hands NULL for it."""

    def __init__(self, entry, **kw):
        self.entry = entry
        rng = np.random.default_rng(ENTRIES.index(entry))
        self.ms = np.full(1, MS_SENTINEL, np.float32)
        self.N = (3, 4, 9)
        self.dtype = 3
        self.values = np.round(rng.normal(300, 200, self.N), 1)
        self.in_ = True
        self.head = (rng.random(self.N) > 0.2).astype(np.uint8)
        self.eroded = (self.head & (rng.random(self.N) > 0.3)).astype(np.uint8)
        if entry == 'bfd_integer_histogram3d':
            self.outputs = {'counts': np.full(65536, -7, np.int64), 'first': np.full(1, -7, np.int64), 'numBins': np.full(1, -7, np.int64),
                            'range': np.full(2, -7.0)}
        elif entry == 'bfd_order_statistics3d':
            self.mask = (rng.random(self.N) > 0.3).astype(np.uint8)
            self.above, self.inclusive, self.ranks, self.R, self.quantile = 100.0, 0, np.array([0, 3, 5], np.int64), 3, 95.0
            self.outputs = {'count': np.full(1, -7, np.int64), 'ranksUsed': np.full(4, -7, np.int64), 'statistics': np.full(4, -7.0)}
        elif entry == 'bfd_uniform_histogram3d':
            self.above, self.inclusive, self.bins = 100.0, 0, 15
            self.edges = np.linspace(100.0, 1000.0, 16)
            self.outputs = {'counts': np.full(15, -7, np.int64), 'range': np.full(2, -7.0), 'count': np.full(1, -7, np.int64)}
        elif entry == 'bfd_pseudo_ct_candidates3d':
            self.divisor, self.lo, self.hi = 500.0, 0.1, 0.6
            self.outputs = {'mask': np.full(self.N, 7, np.uint8), 'maximum': np.full(1, -7.0), 'count': np.full(1, -7, np.int64)}
        elif entry == 'bfd_pseudo_ct_convert3d':
            self.divisor, self.slope, self.offset, self.outDtype = 500.0, -2085.0, 2329.0, 3
            self.bone = (rng.random(self.N) > 0.5).astype(np.uint8)
            self.skin = (rng.random(self.N) > 0.2).astype(np.uint8)
            self.cavities = (rng.random(self.N) > 0.9).astype(np.uint8)
            self.outputs = {'out': np.full(self.N, -7.0)}
        else:
            self.vol = (rng.random(self.N) > 0.6).astype(np.uint8)
            self.connectivity, self.tie = 3, 1
            self.outputs = {'out': np.full(self.N, 7, np.uint8), 'info': np.full(2, -7, np.int64)}
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
        val = P(self.values) if self.in_ else None
        e = self.entry
        if e == 'bfd_integer_histogram3d':
            return (device, self.dtype, val, N[0], N[1], N[2], o['counts'], I64(self.outputs['first']) if self.want['first'] else None,
                    I64(self.outputs['numBins']) if self.want['numBins'] else None, o['range'], ms)
        if e == 'bfd_order_statistics3d':
            return (device, self.dtype, val, P(self.mask), N[0], N[1], N[2], self.above, self.inclusive, P(self.ranks), self.R, self.quantile,
                    I64(self.outputs['count']) if self.want['count'] else None, o['ranksUsed'], o['statistics'], ms)
        if e == 'bfd_uniform_histogram3d':
            return (device, self.dtype, val, N[0], N[1], N[2], self.above, self.inclusive, self.bins, P(self.edges), o['counts'], o['range'],
                    I64(self.outputs['count']) if self.want['count'] else None, ms)
        if e == 'bfd_pseudo_ct_candidates3d':
            return (device, self.dtype, val, N[0], N[1], N[2], self.divisor, P(self.head), P(self.eroded), self.lo, self.hi, o['mask'],
                    self.outputs['maximum'].ctypes.data_as(C.POINTER(C.c_double)) if self.want['maximum'] else None,
                    I64(self.outputs['count']) if self.want['count'] else None, ms)
        if e == 'bfd_pseudo_ct_convert3d':
            return (device, self.dtype, val, N[0], N[1], N[2], self.divisor, P(self.head), P(self.bone), P(self.skin), P(self.cavities), self.slope,
                    self.offset, self.outDtype, o['out'], ms)
        return (device, P(self.vol) if self.in_ else None, o['out'], N[0], N[1], N[2], self.connectivity, self.tie, o['info'], ms)

    def run(self, lib, device=0):
        return getattr(lib, self.entry)(*self.args(device))

    def snapshot(self):
        return {k: v.copy() for k, v in self.outputs.items()}

    def untouched(self, but_ms=False):
        same = all(np.array_equal(v, self.pristine[k]) for k, v in self.outputs.items())
        return same and (but_ms or np.all(self.ms == np.float32(MS_SENTINEL)))


# the outputs whose NULL is an argument error (ranksUsed may be NULL; a form of the uniform histogram needs its own alone: the valid case has edges)
REQUIRED = {'bfd_integer_histogram3d': ('counts', 'first', 'numBins', 'range'), 'bfd_order_statistics3d': ('count', 'statistics'),
            'bfd_uniform_histogram3d': ('counts',), 'bfd_pseudo_ct_candidates3d': ('mask', 'maximum', 'count'), 'bfd_pseudo_ct_convert3d': ('out',),
            'bfd_select_component3d': ('out', 'info')}


def faults(entry):
    """The -1 refusals that come before a device is looked for, in the header's order. 'overlap' hands an input's own bytes as an output."""
    volume = [('null', 'null', dict(in_=False)), ('negative', 'negative', dict(N=(3, -4, 9))), ('size', '2^31', dict(N=(2048, 1024, 1024)))]
    if entry == 'bfd_select_component3d':
        return volume + [('connectivity', 'connectivity', dict(connectivity=4)), ('tie', 'tie', dict(tie=2)), ('overlap', 'alias', 'overlap')]
    head = [('dtype', 'dtype', dict(dtype=2))] + volume + [('output', 'null', {'want_' + REQUIRED[entry][-1]: False})]
    if entry == 'bfd_integer_histogram3d':
        return head + [('overlap', 'alias', 'overlap')]
    if entry == 'bfd_order_statistics3d':
        return head + [('above', 'threshold', dict(above=float('nan'))), ('inclusive', 'inclusive', dict(inclusive=2)), ('R', 'R must', dict(R=5))]
    if entry == 'bfd_uniform_histogram3d':
        return head + [('above', 'threshold', dict(above=float('nan'))), ('inclusive', 'inclusive', dict(inclusive=-1)), ('bins', 'bins', dict(bins=1025)),
                       ('edges', 'edges', dict(edges=np.linspace(1000.0, 100.0, 16)))]
    if entry == 'bfd_pseudo_ct_candidates3d':
        return head + [('divisor', 'divisor', dict(divisor=0.0)), ('range', 'lo or hi', dict(hi=float('nan'))), ('overlap', 'alias', 'overlap')]
    return head + [('outDtype', 'outDtype', dict(outDtype=2)), ('divisor', 'divisor', dict(divisor=float('inf'))),
                   ('slope', 'slope', dict(slope=float('nan'))), ('overlap', 'alias', 'overlap')]


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
    if 'bins' in names and 'edges' in names:
        kw['edges'] = np.linspace(1000.0, 100.0, 1026)
    c = Case(entry, **kw)
    if overlap:
        if entry == 'bfd_integer_histogram3d':
            big = np.zeros(65536, np.float64)           # the volume lies in the first bytes of the counts
            big[:c.values.size] = c.values.ravel()
            c.values = big[:c.values.size].reshape(c.values.shape)
            c.outputs['counts'] = big.view(np.int64)
        elif entry == 'bfd_pseudo_ct_candidates3d':
            c.outputs['mask'] = c.eroded
        elif entry == 'bfd_pseudo_ct_convert3d':
            c.outputs['out'] = c.values
        else:
            c.outputs['out'] = c.vol
        c.pristine = c.snapshot()
    return c


def ordered_plants(entry):
    """[(names planted together, the name that must be reported)]: every fault alone, and each with all the later ones. The overlap is looked for
    with the volume's true size only, so it is planted alone or beside faults that leave the size alone."""
    names = [n for n, _, _ in faults(entry)]
    last = -1 if names[-1] == 'overlap' else None
    combos = [([n], n) for n in names]
    combos += [(names[i:last], names[i]) for i in range(len(names) - 2)]
    if last:
        shape = ('null', 'negative', 'size')
        combos += [([n, 'overlap'], n) for n in names[:-1] if n not in shape]
    return combos
