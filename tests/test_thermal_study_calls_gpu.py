"""The call contract of the bfd_thermal_* entries on a device: a bad ordinal, stages out of order (-6), an id beyond the table (-5, nothing kept), the
argument errors that need a live handle in the header's order with the outputs untouched, and the empty schedule."""
import ctypes as C

import numpy as np
import pytest

from babelbrain_amd import _engine

pytestmark = pytest.mark.gpu
P = _engine._ptr
N = (4, 5, 6)
n = 4 * 5 * 6


@pytest.fixture(scope='module')
def lib():
    return _engine.load_library()


def err(lib):
    return lib.bfd_last_error().decode()


@pytest.fixture
def handle(lib):
    h = C.c_void_p()
    assert lib.bfd_thermal_create(0, N[0], N[1], N[2], 1, 5, C.byref(h)) == 0
    yield h
    lib.bfd_thermal_destroy(h)


def inputs(seed=0, top=5):
    rng = np.random.default_rng(seed)
    return (rng.uniform(1e5, 3e5, N).astype(np.float32), rng.uniform(1e5, 3e5, N).astype(np.float32), rng.integers(0, top, N).astype(np.uint32))


TABLES = [np.full(5, v, np.float32) for v in (0.01, 0.001, 1e-13, 37.0)]


def run(lib, h, nSteps=4, flags=0, T0=None, dose0=None, sched=None, pts=None, idx=None, caps=None):
    sched = np.zeros(max(nSteps, 1), np.int32) if sched is None else sched
    ms = C.c_double(-1.0)
    rc = lib.bfd_thermal_run(h, P(TABLES[0]), P(TABLES[1]), P(TABLES[2]), P(TABLES[3]), flags, P(T0), P(dose0), 37.0, 0.01, nSteps, P(sched), 1,
                             0 if idx is None else len(idx), P(idx), P(pts), 0 if caps is None else len(caps), P(caps), C.byref(ms))
    return rc, ms.value


def test_bad_ordinal(lib):
    h = C.c_void_p()
    for device in (-1, lib.bfd_device_count()):
        assert lib.bfd_thermal_create(device, 4, 4, 4, 1, 5, C.byref(h)) == -3 and 'ordinal' in err(lib) and not h


def test_stages_out_of_order(lib, handle):
    p, pw, m = inputs()
    out, one = np.full(N, 7.0, np.float32), np.full(1, 1.5)
    table = np.array([1, 4, 8, 8, 1], np.uint8)
    ms = C.c_float(7.0)
    big = [np.full(8, 7, np.int64), np.full(8, 7.0, np.float32), np.full(8, 7, np.int64), np.full(8, 7.0, np.float32), np.full(8, 7, np.int64)]
    which = np.array([2], np.int32)
    # nothing set yet
    assert lib.bfd_thermal_set_scale(handle, P(one), 0) == -6 and 'set_inputs comes first' in err(lib)
    assert lib.bfd_thermal_median_region(handle, P(table), 3, 7, C.byref(ms)) == -6
    assert run(lib, handle)[0] == -6 and 'set_inputs comes first' in err(lib)
    assert lib.bfd_thermal_get(handle, 7, P(out), 0) == -6
    assert lib.bfd_thermal_set_inputs(handle, P(p), P(pw), P(m), 4) == 0
    # inputs, no scale
    assert run(lib, handle) == (-6, -1.0) and 'set_scale comes first' in err(lib)
    assert lib.bfd_thermal_get(handle, 5, P(out), 0) == -6 and 'set_scale' in err(lib)
    assert lib.bfd_thermal_get_plane(handle, 5, 1, P(out)) == -6
    assert lib.bfd_thermal_set_scale(handle, P(one), 0) == 0
    # scaled, no run
    for name in (0, 1, 2, 3, 4):
        assert lib.bfd_thermal_get(handle, name, P(out), 0) == -6 and 'bfd_thermal_run comes first' in err(lib)
    assert lib.bfd_thermal_merge_max(handle, 0, P(p)) == -6
    assert lib.bfd_thermal_extrema(handle, P(which), 1, P(table), *[P(a) for a in big], C.byref(ms)) == -6
    assert (out == 7).all() and ms.value == 7.0 and all((a == 7).all() for a in big)
    assert run(lib, handle)[0] == 0
    assert lib.bfd_thermal_get(handle, 2, P(out), 0) == 0 and (out != 7).all()
    # new inputs forget the scale and the run
    assert lib.bfd_thermal_set_inputs(handle, P(p), P(pw), P(m), 4) == 0
    assert lib.bfd_thermal_get(handle, 2, P(out), 0) == -6 and run(lib, handle)[0] == -6


def test_an_id_beyond_the_table_is_refused_and_nothing_is_kept(lib, handle):
    p, pw, m = inputs()
    one, out = np.full(1, 1.5), np.full(N, 7.0, np.float32)
    assert lib.bfd_thermal_set_inputs(handle, P(p), P(pw), P(m), 4) == 0
    for dtype, bad in ((np.uint32, 5), (np.uint32, 70000), (np.uint16, 256), (np.uint8, 255)):
        mb = m.astype(dtype)
        mb[3, 4, 5] = bad                                  # the last voxel: in the last, partly filled quad of no volume here, so also one before
        assert lib.bfd_thermal_set_inputs(handle, P(p), P(pw), P(mb), mb.dtype.itemsize) == -5 and 'not below nMat' in err(lib)
        assert lib.bfd_thermal_set_scale(handle, P(one), 0) == -6             # nothing kept, the good inputs of before included
        assert lib.bfd_thermal_get(handle, 7, P(out), 0) == -6 and (out == 7).all()
        assert lib.bfd_thermal_set_inputs(handle, P(p), P(pw), P(m.astype(dtype)), mb.dtype.itemsize) == 0
        assert lib.bfd_thermal_get(handle, 7, P(out), 0) == 0 and np.array_equal(out, p)
        out[...] = 7.0


def test_argument_errors_with_a_live_handle_in_the_headers_order(lib, handle):
    p, pw, m = inputs()
    one = np.full(1, 1.5)
    out = np.full(N, 7.0, np.float32)
    table = np.array([1, 4, 8, 8, 1], np.uint8)
    ms = C.c_float(7.0)
    assert lib.bfd_thermal_set_inputs(handle, None, P(pw), P(m), 4) == -1 and 'null argument' in err(lib)
    assert lib.bfd_thermal_set_inputs(handle, P(p), P(pw), P(m), 3) == -1 and 'idBytes' in err(lib)
    assert lib.bfd_thermal_set_inputs(handle, P(p), P(pw), P(m), 4) == 0
    assert lib.bfd_thermal_median_region(handle, None, 3, 7, C.byref(ms)) == -1 and 'null argument' in err(lib)
    assert lib.bfd_thermal_median_region(handle, P(table), 8, 0, C.byref(ms)) == -1 and 'bit must be' in err(lib)           # bit before which
    assert lib.bfd_thermal_median_region(handle, P(table), 3, 5, C.byref(ms)) == -1 and 'which must be' in err(lib)
    rho = np.full(5, 1000.0)
    outs = [np.full(1, 7.0, np.float32), np.full(1, 7, np.int64), np.full(1, 7.0, np.float32), np.full(1, 7, np.int64), np.full(N[2], 7.0), np.full(N[2], 7.0),
            np.full(N[2], 7.0)]

    def survey(rhoW=1000.0, cW=1500.0, dx2=1e-6, rho=rho, c=rho):
        return lib.bfd_thermal_loss_survey(handle, P(table), None, P(rho), P(c), rhoW, cW, dx2, *[P(a) for a in outs], C.byref(ms))
    assert survey(rhoW=0.0, dx2=-1.0) == -1 and 'rhoWater' in err(lib)
    bad = rho.copy(); bad[4] = np.inf
    assert survey(c=bad, dx2=-1.0) == -1 and 'every rho and c' in err(lib)
    assert survey(dx2=np.nan) == -1 and 'dx2' in err(lib)
    assert all((a == 7).all() for a in outs) and ms.value == 7.0
    assert lib.bfd_thermal_set_scale(handle, P(one), 2) == -1 and 'mode' in err(lib)
    assert lib.bfd_thermal_set_scale(handle, P(np.full(1, np.nan)), 0) == -1 and 'finite' in err(lib)
    assert lib.bfd_thermal_set_scale(handle, P(one), 0) == 0
    # run: flags, announced volumes, schedule, points, captures
    pts, idx = np.full((1, 4), 7.0, np.float32), np.array([n], np.uint32)
    assert run(lib, handle, flags=32)[0] == -1 and 'flags' in err(lib)
    assert run(lib, handle, flags=17, T0=p)[0] == -1 and 'flags' in err(lib)
    assert run(lib, handle, flags=16)[0] == -6 and 'set_previous comes first' in err(lib)
    assert lib.bfd_thermal_set_previous(handle, P(p), None, P(p)) == -1 and 'null argument' in err(lib)
    assert run(lib, handle, flags=1)[0] == -1 and 'announce' in err(lib)
    assert run(lib, handle, nSteps=-1)[0] == -1 and 'nSteps' in err(lib)
    assert run(lib, handle, sched=np.array([0, 0, 1, 0], np.int32))[0] == -1 and 'fieldOfStep entry' in err(lib)
    assert run(lib, handle, pts=pts, idx=idx) == (-1, -1.0) and 'outside the volume' in err(lib) and (pts == 7).all()
    assert run(lib, handle, caps=np.array([3, 2], np.int32))[0] == -1 and 'captureStep' in err(lib)
    assert run(lib, handle, caps=np.array([5], np.int32))[0] == -1 and 'captureStep' in err(lib)
    assert run(lib, handle)[0] == 0
    assert lib.bfd_thermal_merge_max(handle, 5, P(p)) == -1 and 'which' in err(lib)
    assert lib.bfd_thermal_get(handle, 9, P(out), 0) == -1 and lib.bfd_thermal_get(handle, 0, P(out), 2) == -1 and 'dtype' in err(lib)
    assert lib.bfd_thermal_get(handle, 0, P(out), 1) == -1 and 'float64' in err(lib)
    assert lib.bfd_thermal_get_plane(handle, 0, 0, P(out)) == -1 and lib.bfd_thermal_get_plane(handle, 5, N[1], P(out)) == -1 and 'outside' in err(lib)
    big = [np.full(8, 7, np.int64), np.full(8, 7.0, np.float32), np.full(8, 7, np.int64), np.full(8, 7.0, np.float32), np.full(8, 7, np.int64)]
    assert lib.bfd_thermal_extrema(handle, P(np.array([6], np.int32)), 1, P(table), *[P(a) for a in big], C.byref(ms)) == -1 and 'a volume must be' in err(lib)
    assert lib.bfd_thermal_extrema(handle, P(np.array([0], np.int32)), 0, P(table), *[P(a) for a in big], C.byref(ms)) == -1 and 'nVol' in err(lib)
    assert (out == 7).all() and all((a == 7).all() for a in big)


def test_the_empty_schedule_sets_the_start_state(lib, handle):
    p, pw, m = inputs()
    assert lib.bfd_thermal_set_inputs(handle, P(p), P(pw), P(m), 4) == 0
    assert lib.bfd_thermal_set_scale(handle, P(np.full(1, 1.5)), 0) == 0
    initT = np.array([36.0, 36.5, 37.0, 37.5, 38.0], np.float32)
    ms = C.c_double(-1.0)
    assert lib.bfd_thermal_run(handle, P(TABLES[0]), P(TABLES[1]), P(TABLES[2]), P(initT), 0, None, None, 37.0, 0.01, 0, None, 1, 0, None, None, 0, None,
                               C.byref(ms)) == 0
    T, D, Tmax = (np.full(N, 7.0, np.float32) for _ in range(3))
    assert lib.bfd_thermal_get(handle, 2, P(T), 0) == 0 and lib.bfd_thermal_get(handle, 3, P(D), 0) == 0 and lib.bfd_thermal_get(handle, 0, P(Tmax), 0) == 0
    assert np.array_equal(T, initT[m]) and np.array_equal(Tmax, T) and (D == 0).all() and ms.value >= 0.0
    # a second run continues from the resident state unless told to start over
    assert run(lib, handle, nSteps=3)[0] == 0
    T3 = np.empty(N, np.float32)
    assert lib.bfd_thermal_get(handle, 2, P(T3), 0) == 0 and not np.array_equal(T3, T)
    assert run(lib, handle, nSteps=0)[0] == 0
    T4 = np.empty(N, np.float32)
    assert lib.bfd_thermal_get(handle, 2, P(T4), 0) == 0 and np.array_equal(T4, T3)
    assert run(lib, handle, nSteps=0, flags=4)[0] == 0
    assert lib.bfd_thermal_get(handle, 2, P(T4), 0) == 0 and np.array_equal(T4, np.full(N, 37.0, np.float32))
    up, down = C.c_int64(), C.c_int64()
    assert lib.bfd_thermal_traffic(handle, C.byref(up), C.byref(down)) == 0 and up.value > 3 * n * 4 and down.value >= 6 * n * 4
