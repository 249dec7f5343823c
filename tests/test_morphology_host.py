"""Binary morphology and labelling without a GPU: BinaryClosing / LabelImage refuse bad arguments before the library is loaded, tell an all-ones box
from a general structure, and the per-axis taps of the box path (three 1-D passes, restated in numpy here) equal scipy's 3-D operations."""
import os

import numpy as np
import pytest

from babelbrain_amd import BinaryClosing as BC, LabelImage as LI, _engine

ndi = pytest.importorskip('scipy.ndimage')


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """The library is out of reach: its path names a missing file and loading it is an error. The refusals below must come first."""
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_engine, 'LIB_PATH', str(tmp_path / 'no_such_library.so'))
    monkeypatch.setattr(_engine, '_lib', None)
    monkeypatch.setattr(_engine, 'load_library', boom)


MASK = np.zeros((8, 9, 10), bool)
ALL_OPS = [BC.BinaryClose, BC.BinaryOpen, BC.BinaryDilate, BC.BinaryErode]


@pytest.mark.parametrize('fn', ALL_OPS, ids=lambda f: f.__name__)
def test_unsupported_arguments(no_library, fn):
    st = np.ones((3, 3, 3), int)
    with pytest.raises((NotImplementedError, ValueError)):
        fn(MASK, st, origin=1)
    with pytest.raises((NotImplementedError, ValueError)):
        fn(MASK, st, origin=(0, -1, 0))
    with pytest.raises((NotImplementedError, ValueError)):
        fn(MASK, st, mask=np.ones(MASK.shape, bool))
    with pytest.raises((NotImplementedError, ValueError)):
        fn(MASK, st, output=np.zeros(MASK.shape, bool))
    with pytest.raises(ValueError):
        fn(MASK, st, iterations=0)
    with pytest.raises(ValueError):
        fn(MASK, st, iterations=-1)
    with pytest.raises(ValueError):
        fn(MASK, st, iterations=1.5)
    with pytest.raises(ValueError):
        fn(MASK, st, border_value=2)
    with pytest.raises(ValueError):
        fn(np.zeros((8, 9), bool), st)
    with pytest.raises(ValueError):
        fn(MASK, np.ones((3, 3), int))
    with pytest.raises(ValueError):
        fn(MASK, np.zeros((3, 3, 3), int))                           # no true element
    with pytest.raises(ValueError):
        fn(MASK, np.ones((32, 3, 3), int))
    with pytest.raises(TypeError):
        fn(np.zeros((8, 9, 10), np.float32), st)
    with pytest.raises(AssertionError, match='library was loaded'):    # a good call gets as far as the library
        fn(MASK, st, origin=0, GPUBackend='OpenCL')


def test_border_value_of_closing_and_opening(no_library):
    for fn in (BC.BinaryClose, BC.BinaryOpen):
        with pytest.raises(ValueError):
            fn(MASK, np.ones((3, 3, 3), int), border_value=1)
    for fn in (BC.BinaryDilate, BC.BinaryErode):                       # 0 and 1 both pass the checks there
        with pytest.raises(AssertionError, match='library was loaded'):
            fn(MASK, border_value=1)


def test_box_against_general_structure():
    assert BC.structure_path(None) == ('general', None)
    for shape in ((1, 1, 1), (14, 14, 14), (31, 31, 31), (14, 13, 10), (31, 1, 2)):
        path, s = BC.structure_path(np.ones(shape, int))
        assert path == 'box' and s.dtype == np.uint8 and s.shape == shape and s.flags.c_contiguous
    for shape in ((32, 32, 32), (3, 32, 3), (1, 1, 32)):
        with pytest.raises(ValueError):
            BC.structure_path(np.ones(shape, int))
    one_zero = np.ones((7, 7, 7), int)
    one_zero[6, 0, 3] = 0
    path, s = BC.structure_path(one_zero)
    assert path == 'general' and np.array_equal(s, one_zero.astype(np.uint8))
    larger = np.ones((8, 7, 7), int)
    larger[0, 0, 0] = 0
    with pytest.raises(ValueError):
        BC.structure_path(larger)
    assert BC.structure_path(ndi.generate_binary_structure(3, 1))[0] == 'general'
    assert BC.structure_path(np.ones((5, 5, 5)) * 7.5)[0] == 'box'         # non-zero counts as true
    path, s = BC.structure_path(np.ones((3, 4, 5), bool).transpose(2, 1, 0))
    assert path == 'box' and s.flags.c_contiguous and s.shape == (5, 4, 3)


def test_inputs_are_taken_strided_and_bool(no_library):
    b = np.zeros((8, 9, 10), bool)
    b[2:5] = True
    a, s, it, border = BC._checked('closing', b, np.ones((14, 13, 10), int), 2, None, 0, None, 0)
    assert a.dtype == np.uint8 and a.flags.c_contiguous and np.array_equal(a, b.astype(np.uint8)) and s.shape == (14, 13, 10) and (it, border) == (2, 0)
    v = (np.arange(8 * 9 * 10).reshape(8, 9, 10) % 5).astype(np.uint8).transpose(2, 1, 0)
    a, s, it, border = BC._checked('erosion', v, None, 1, None, (0, 0, 0), None, True)
    assert a.flags.c_contiguous and np.array_equal(a, v) and s is None and border == 1


# ---- the taps of the box path ----

def taps(s, dilate):
    """d range of one axis of an all-ones structure of size s: out[x] = AND / OR of in[x + d] (what bfd_morph_core.h's morph_box_taps states)"""
    return (-(s - 1 - s // 2), s // 2) if dilate else (-(s // 2), s - 1 - s // 2)


def pass_1d(a, axis, s, dilate, border=False):
    lo, hi = taps(s, dilate)
    n = a.shape[axis]
    pad = [(0, 0)] * 3
    pad[axis] = (-lo, hi)
    p = np.pad(a, pad, constant_values=border)
    out = np.zeros_like(a) if dilate else np.ones_like(a)
    for d in range(lo, hi + 1):
        cut = [slice(None)] * 3
        cut[axis] = slice(d - lo, d - lo + n)
        out = (out | p[tuple(cut)]) if dilate else (out & p[tuple(cut)])
    return out


def separable(a, s, dilate, border=False):
    for axis in (2, 1, 0):
        a = pass_1d(a, axis, s[axis], dilate, border)
    return a


BOXES = [((20, 17, 70), (s, s, s)) for s in (1, 2, 3, 4, 5, 14)] + [((20, 17, 70), (14, 13, 10)), ((9, 10, 11), (14, 14, 14))]


@pytest.mark.parametrize('shape,s', BOXES, ids=str)
def test_three_1d_passes_equal_scipy(shape, s):
    rng = np.random.default_rng(3)
    st = np.ones(s, int)
    for density in (0.02, 0.6):
        a = rng.random(shape) < density
        assert np.array_equal(separable(a, s, True), ndi.binary_dilation(a, st))
        assert np.array_equal(separable(separable(a, s, True), s, False), ndi.binary_closing(a, st))
        assert np.array_equal(separable(a, s, False), ndi.binary_erosion(a, st))
        for border in (False, True):
            assert np.array_equal(separable(a, s, True, border), ndi.binary_dilation(a, st, border_value=border))
            assert np.array_equal(separable(a, s, False, border), ndi.binary_erosion(a, st, border_value=border))


def test_closing_erodes_the_faces():
    """an all-ones volume closed with 14 loses floor(14 / 2) = 7 layers at the low end and 14 - 1 - 7 = 6 at the high end of each axis"""
    a = np.ones((30, 31, 40), bool)
    want = np.zeros_like(a)
    want[7:-6, 7:-6, 7:-6] = True
    assert np.array_equal(separable(separable(a, (14,) * 3, True), (14,) * 3, False), want)
    assert np.array_equal(ndi.binary_closing(a, np.ones((14,) * 3, int)), want)


# ---- labelling ----

def test_label_refusals(no_library):
    b = np.zeros((4, 5, 6), bool)
    for dtype in (np.uint8, np.int32, np.float32):
        with pytest.raises(RuntimeError, match='boolean'):
            LI.LabelImage(np.zeros((4, 5, 6), dtype))
    for c in (0, 4, -1, 2.5, 'a'):
        with pytest.raises(ValueError):
            LI.LabelImage(b, connectivity=c)
        with pytest.raises(ValueError):
            LI.component_sizes(b, connectivity=c)
        with pytest.raises(ValueError):
            LI.largest_component(b, connectivity=c)
    with pytest.raises(ValueError):
        LI.LabelImage(np.zeros((4, 5), bool))
    with pytest.raises(AssertionError, match='library was loaded'):
        LI.LabelImage(b, background=1, return_num=True, connectivity=None, GPUBackend='OpenCL')


def test_label_inputs(no_library):
    b = np.zeros((4, 5, 6), bool)
    b[1, 2, 3] = True
    before = b.copy()
    a, c = LI._checked(b.transpose(2, 1, 0), 1, None)
    assert c == 3 and a.dtype == np.uint8 and a.flags.c_contiguous and np.array_equal(a, (~b).transpose(2, 1, 0).astype(np.uint8))
    assert np.array_equal(b, before)
    a, c = LI._checked(b, None, 1)
    assert c == 1 and np.array_equal(a, b.astype(np.uint8))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _engine.load_library()


def test_library_refuses_bad_arguments_before_any_device(lib):
    """bfd_binary_morphology3d and bfd_label3d report argument errors (rc -1) before they look for a device; nothing is read or written."""
    for name in ('bfd_binary_morphology3d', 'bfd_label3d'):
        assert name in _engine.ABI_SYMBOLS and hasattr(lib, name)
    a, o = np.zeros(64, np.uint8), np.full(64, 7, np.uint8)
    pa, po = _engine._ptr(a), _engine._ptr(o)

    def morph(op=2, i=pa, out=po, N=(4, 4, 4), st=None, s=(3, 3, 3), it=1, border=0):
        return lib.bfd_binary_morphology3d(0, op, i, out, N[0], N[1], N[2], _engine._ptr(st), s[0], s[1], s[2], it, border, None)
    holed = np.ones((8, 7, 7), np.uint8)
    holed[0, 0, 0] = 0
    for kw, word in ((dict(op=4), 'op'), (dict(i=None), 'null'), (dict(out=pa), 'alias'), (dict(N=(1 << 11, 1 << 10, 1 << 10)), '2^31'),
                     (dict(it=0), 'iterations'), (dict(border=2), 'borderValue'), (dict(op=2, border=1), 'closing'),
                     (dict(st=np.ones((32, 1, 1), np.uint8), s=(32, 1, 1)), '31'), (dict(st=holed, s=(8, 7, 7)), '7'),
                     (dict(st=np.zeros((3, 3, 3), np.uint8)), 'no true'), (dict(N=(-1, 4, 4)), 'negative')):
        assert morph(**kw) == -1, kw
        assert word in lib.bfd_last_error().decode(), (kw, lib.bfd_last_error().decode())

    lab = np.full(64, 7, np.int32)
    n = np.full(1, 7, np.int64)

    def label(i=pa, out=_engine._ptr(lab), N=(4, 4, 4), c=3, cap=0, largest=None):
        return lib.bfd_label3d(0, i, out, N[0], N[1], N[2], c, n.ctypes.data_as(_engine.C.POINTER(_engine.C.c_int64)), None, cap, largest, None)
    for kw, word in ((dict(i=None), 'null'), (dict(c=0), 'connectivity'), (dict(c=4), 'connectivity'), (dict(N=(1 << 40, 1 << 40, 1 << 40)), '2^31'),
                     (dict(cap=-1), 'sizesCapacity'), (dict(largest=pa), 'alias'), (dict(N=(4, -4, 4)), 'negative')):
        assert label(**kw) == -1, kw
        assert word in lib.bfd_last_error().decode(), (kw, lib.bfd_last_error().decode())
    assert lib.bfd_label3d(0, pa, None, 4, 4, 4, 3, None, None, 0, None, None) == -1 and 'no output' in lib.bfd_last_error().decode()
    assert np.all(a == 0) and np.all(o == 7) and np.all(lab == 7) and n[0] == 7
