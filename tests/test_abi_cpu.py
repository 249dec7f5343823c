"""The signature table of babelbrain_amd/_abi.py agrees with the prototypes of include/babelfdtd.h, entry by entry and argument by
argument (no library needed: the table is data); the C-ABI library loads and exports every symbol the header declares; host-only
entry points (no GPU needed) agree with the oracle. No compute call is made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from babelbrain_amd import _abi, _engine, harness as H
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


def _header():
    """include/babelfdtd.h without its comments"""
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'babelfdtd.h')).read(), flags=re.S)


# what the header's scalar types and the table's ctypes types are compared as; anything else in the header must be a pointer
C_KINDS = {'void': 'void', 'int': 'int32', 'int32_t': 'int32', 'uint32_t': 'uint32', 'int64_t': 'int64', 'size_t': 'size', 'double': 'double',
           'float': 'float'}
CTYPES_KINDS = {None: 'void', C.c_int32: 'int32', C.c_uint32: 'uint32', C.c_int64: 'int64', C.c_size_t: 'size', C.c_double: 'double', C.c_float: 'float'}
assert C.sizeof(C.c_int32) == 4 and C.sizeof(C.c_uint32) == 4 and C.c_int32(-1).value == -1 and C.c_uint32(-1).value == 2 ** 32 - 1


def _c_kind(decl, handles):
    """Kind of a C declaration `type [name]`: 'pointer' for T *, char * and the handle typedefs, else the scalar's kind."""
    words = [w for w in decl.replace('*', ' * ').split() if w != 'const']
    if '*' in words or words[0] in handles:
        return 'pointer'
    return C_KINDS.get(words[0], 'unknown C type %r' % decl)


def _ctypes_kind(t):
    if t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer)):
        return 'pointer'
    return CTYPES_KINDS.get(t, 'unknown ctypes type %r' % (t,))


def header_prototypes():
    """{entry: (kind of the return value, [kind of each argument])} of every prototype of the header."""
    hdr = _header()
    handles = set(re.findall(r'typedef\s+struct\s+\w+\s*\*\s*(\w+)\s*;', hdr))      # bfd_thermal, bfd_acoustic: pointers by typedef
    protos = {}
    for ret, name, args in re.findall(r'^[ \t]*((?:const[ \t]+)?\w+[ \t]*\*?)[ \t]*\b(bfd_[a-z_0-9]+)[ \t]*\(([^)]*)\)[ \t]*;', hdr, flags=re.M):
        args = [a.strip() for a in args.split(',')]
        assert name not in protos, name
        protos[name] = (_c_kind(ret, handles), [] if args == ['void'] else [_c_kind(a, handles) for a in args])
    return protos


def signature_mismatches(table, protos):
    """One line per disagreement between the table and the prototypes, each starting with the entry's name."""
    bad = ['%s: in the header only' % n for n in sorted(set(protos) - set(table))] + ['%s: in the table only' % n for n in sorted(set(table) - set(protos))]
    for name in sorted(set(table) & set(protos)):
        restype, argtypes = table[name]
        ret, args = protos[name]
        if _ctypes_kind(restype) != ret:
            bad.append('%s: returns %s in the header, %s in the table' % (name, ret, _ctypes_kind(restype)))
        if len(argtypes) != len(args):
            bad.append('%s: %d arguments in the header, %d in the table' % (name, len(args), len(argtypes)))
            continue
        bad += ['%s: argument %d is %s in the header, %s in the table' % (name, i, a, _ctypes_kind(t))
                for i, (a, t) in enumerate(zip(args, argtypes)) if _ctypes_kind(t) != a]
    return bad


def test_signature_table_matches_the_prototypes():
    protos = header_prototypes()
    assert len(protos) == len(set(re.findall(r'\b(bfd_[a-z_0-9]+)\s*\(', _header()))) >= 137         # the pattern misses no prototype
    assert set(protos) == set(_abi.SIGNATURES)
    assert signature_mismatches(_abi.SIGNATURES, protos) == []
    assert _engine.ABI_SYMBOLS == list(_abi.SIGNATURES) and len(set(_engine.ABI_SYMBOLS)) == len(_engine.ABI_SYMBOLS)
    # only what takes no argument has no argtypes (tests/test_acoustic_calls_host.py relies on the rest being non-empty)
    assert sorted(n for n, (_, a) in _abi.SIGNATURES.items() if not a) == sorted(n for n, (_, a) in protos.items() if not a)


def _planted(name, restype=None, argtypes=None):
    table = dict(_abi.SIGNATURES)
    r, a = table[name]
    table[name] = (r if restype is None else restype, list(a) if argtypes is None else argtypes(list(a)))
    return table


def _replace(i, old, new):
    def f(a):
        assert a[i] is old, a[i]
        a[i] = new
        return a
    return f


@pytest.mark.parametrize('name,fault,says', [
    ('bfd_set_sources', dict(argtypes=_replace(1, C.c_int64, C.c_int32)), 'argument 1 is int64 in the header, int32 in the table'),
    ('bfd_group_get_map', dict(argtypes=lambda a: a[:-1]), '7 arguments in the header, 6 in the table'),
    ('bfd_thermal_get', dict(argtypes=_replace(2, C.c_void_p, C.c_int64)), 'argument 2 is pointer in the header, int64 in the table'),
    ('bfd_acoustic_create', dict(argtypes=_replace(6, C.POINTER(C.c_void_p), C.c_int64)), 'argument 6 is pointer in the header, int64 in the table'),
    ('bfd_num_sensors', dict(restype=C.c_int), 'returns int64 in the header, int32 in the table'),
    ('bfd_placement_cache_release', dict(restype=C.c_int), 'returns int64 in the header, int32 in the table'),
    ('bfd_bone_rim_correct3d', dict(argtypes=_replace(8, C.c_float, C.c_double)), 'argument 8 is float in the header, double in the table'),
    ('bfd_halo_fields', dict(argtypes=_replace(1, C.c_int32, C.c_uint32)), 'argument 1 is int32 in the header, uint32 in the table'),
    ('bfd_destroy', dict(restype=C.c_int), 'returns void in the header, int32 in the table'),
])
def test_signature_check_sees_a_planted_fault(name, fault, says):
    """The faults that no other test sees and x86-64 mostly forgives: each is reported, once, under the entry's name."""
    assert signature_mismatches(_planted(name, **fault), header_prototypes()) == ['%s: %s' % (name, says)]


def test_signature_check_sees_a_missing_and_an_extra_entry():
    table = dict(_abi.SIGNATURES)
    table['bfd_no_such_entry'] = table.pop('bfd_sync')
    assert signature_mismatches(table, header_prototypes()) == ['bfd_sync: in the header only', 'bfd_no_such_entry: in the table only']


def test_header_symbols_exported(lib):
    for s in header_prototypes():
        assert hasattr(lib, s), s
    assert lib.bfd_abi_version() == _abi.ABI_VERSION


def test_abi_version_matches_header():
    assert [int(v) for v in re.findall(r'^#define\s+BFD_ABI_VERSION\s+(\d+)\s*$', _header(), flags=re.M)] == [_abi.ABI_VERSION]


def header_struct(name):
    """[(field, C type, array length or None)] of `typedef struct name { ... } name;`"""
    hdr = _header()
    body = hdr[hdr.index('typedef struct %s {' % name) + len('typedef struct %s {' % name):hdr.index('} %s;' % name)]
    fields = []
    for ctype, decl in re.findall(r'(\w+)\s+([^;]+);', body):
        for d in decl.split(','):
            m = re.fullmatch(r'(\w+)(?:\[(\d+)\])?', d.strip())
            fields.append((m.group(1), C_KINDS[ctype], int(m.group(2)) if m.group(2) else None))
    return fields


def test_struct_layout_matches_header():
    """Names, order, types and array lengths of the fields of both structs."""
    def field(n, t):
        return (n, _ctypes_kind(t._type_), t._length_) if issubclass(t, C.Array) else (n, _ctypes_kind(t), None)
    for name, struct in (('bfd_config', _abi.Config), ('bfd_pack_spec', _abi.PackSpec)):
        assert header_struct(name) == [field(n, t) for n, t in struct._fields_], name
    assert _engine.Config is _abi.Config and _engine.PackSpec is _abi.PackSpec


def test_stable_dt_and_tables_host_side(lib):
    ml = H.ct_material_rows(500e3, 32)
    h = H.spatial_step(500e3, 6)
    q = np.ones(len(ml)); q[2:] = 3
    for corr in (True, False):
        dt = _engine.stable_dt(ml, 500e3, corr, h, 0.5, q)
        assert dt == O.stable_dt(ml, 500e3, corr, h, 0.5, q)
        th, ch, cm = _engine.material_tables(ml, 500e3, corr, h, dt, q)
        to, co, cmo = O.tables(ml, 500e3, h, dt, corr, q)
        assert np.array_equal(th, to) and np.array_equal(ch, co) and cm == cmo
    # CFL: cmax dt / h = 0.5 * (6/7)/sqrt(3)
    assert abs(cm * dt / h - 0.5 * 6 / 7 / np.sqrt(3)) < 1e-12


def test_engine_refuses_without_gpu(lib):
    if lib.bfd_device_count() > 0:
        pytest.skip('a GPU is present')
    with pytest.raises(_engine.EngineError):
        _engine.Engine(64, 64, 64, 1, 1e-3, 1e-7, 5e5, 10)


@pytest.mark.parametrize('k0,nk', [(0, 3), (30, 2), (61, 3), (20, 0)])
def test_engine_refuses_a_slab_thinner_than_the_splitters_allow(lib, k0, nk):
    """One rule in three places: slab.partition, partition() of bfd_group.hip and bfd_create all want 4 planes in a slab. The
    arguments are checked before a device is looked for, so this holds with and without a GPU."""
    import ctypes as C
    from babelbrain_amd import slab
    assert slab.MIN_PLANES == 4

    def create(k0, nk):
        cfg = _engine.Config(N1=64, N2=64, N3=64, k0=k0, nk=nk, nMat=1, NDelta=12, typeSource=0, sensorSub=1, sensorStart=0, nt=10,
                             selRMSorPeak=1, selMapsRMS=_engine.mask_of(['Pressure']), selMapsSensors=_engine.mask_of(['Pressure']),
                             qfactorCorrection=1, device=0, kernelVariant=0, rmsFirstStep=0, sensorMode=0, h=1e-3, dt=1e-7, freq=5e5,
                             reflectionLimit=1e-5)
        handle = C.c_void_p()
        rc = lib.bfd_create(C.byref(cfg), C.byref(handle))
        assert not handle
        return rc, lib.bfd_last_error().decode()

    assert create(k0, nk) == (-2, 'bfd_create: every slab needs at least 4 planes')
    rc, msg = create(62, 4)
    assert rc == -2 and 'outside the domain' in msg


def test_backend_entry_points_of_the_reference_exist(lib):
    """The names BabelBrain imports from the solver package's tools (BabelBrain.py:429-439, SelFiles.py:245-263)."""
    import babelbrain_amd
    from babelbrain_amd import RayleighAndBHTE as R
    for name in ('InitCuda', 'InitOpenCL', 'InitMetal', 'InitMLX', 'ForwardSimple', 'GenerateFocusTx', 'SpeedofSoundWater', 'BHTE',
                 'BHTEMultiplePressureFields'):
        assert callable(getattr(R, name)), name
    names = babelbrain_amd.ListDevices()
    assert isinstance(names, list) and len(names) == lib.bfd_device_count()
    if not names:
        with pytest.raises(_engine.EngineError):
            R.InitMLX('MI355X')
