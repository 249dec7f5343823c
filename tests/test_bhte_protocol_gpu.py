"""RunBHTECycles (one bfd_bhte_run_protocol call for a whole repeated-sonication protocol) against the reference's loop of
BHTE / BHTEMultiplePressureFields calls (CalculateTemperatureEffects.py:259-460), restated here over the existing drop-ins:
every output is bit-equal. And against the numpy oracle run over protocol_schedule (tests/bhte_reference.py): the temperature maximum over the capture
steps, the final temperature and the whole point series to equality, the dose at the last capture and the final dose voxel by voxel to the
derived bound. Small grids: the whole file takes a few seconds."""
import numpy as np
import pytest

from oracle import bhte_oracle as BO
from tests import bhte_reference as BR
from tests.util import rel_l2

pytestmark = pytest.mark.gpu


def _materials():
    # water, skin, cortical, trabecular, brain rows of CalculateTemperatureEffects.py:780-791; acoustic columns of MatFreq[500e3]
    return {'Density': np.array([1000.0, 1116.0, 1896.5, 1738.0, 1041.0]), 'SoS': np.array([1500.0, 1537.0, 2476.0, 2205.0, 1562.0]),
            'Attenuation': np.array([0.0, 2.3, 81.0, 81.0, 3.45]), 'SpecificHeat': np.array([4178.0, 3391.0, 1313.0, 2274.0, 3630.0]),
            'Conductivity': np.array([0.6, 0.37, 0.32, 0.31, 0.51]), 'Perfusion': np.array([0.0, 106.0, 10.0, 30.0, 559.0]),
            'Absorption': np.array([0.0, 0.85, 0.16, 0.15, 0.85]), 'InitTemperature': np.full(5, 37.0)}


def _problem(N, seed, centres=((0, 0),), amp=5.0e6):
    rng = np.random.default_rng(seed)
    mm = rng.integers(0, 5, N).astype(np.uint8)
    x, y, z = np.meshgrid(*[np.arange(n) - n / 2 for n in N], indexing='ij')
    fields = np.stack([amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z / 2) ** 2) / 30.0) for cx, cy in centres])
    mpm = np.zeros(N, np.uint32)
    mpm[N[0] // 2, N[1] // 2, N[2] // 2] = 1; mpm[N[0] // 4, N[1] // 4, 3 * N[2] // 4] = 2; mpm[3 * N[0] // 5, N[1] // 2, N[2] // 4] = 3
    return mm, fields, mpm


def _chained(nCurrent, rep, total, pause, off, limit, single, PMaps, mm, ml, dx, nOn, nStepsOn, dt, duty, mpm, stable, TP, FT, FD, prev,
             sub=False):
    """The reference's loop (:349-459) restated over R.BHTE / R.BHTEMultiplePressureFields: one call per ON period, OFF period and
    group pause, T and dose through the host in between. ResTempMax folds from this call's first ON end (the defined resume)."""
    from babelbrain_amd import RayleighAndBHTE as R
    cool = np.zeros(mm.shape)
    kw = dict(dt=dt, MonitoringPointsMap=mpm, stableTemp=stable)
    n = nCurrent
    for n in range(nCurrent, total):
        if n > 0:
            T0, D0 = FT, FD
        elif prev is not None:
            T0, D0 = prev['FinalTemp'], prev['FinalDose']
        else:
            T0 = D0 = None
        if single:
            Ton, Don, _, _, Pon = R.BHTE(PMaps, mm, ml, dx, nOn, nStepsOn, -1, DutyCycle=duty, initT0=T0, initDose=D0, **kw)
        else:
            Ton, Don, _, _, Pon = R.BHTEMultiplePressureFields(PMaps, mm, ml, dx, nOn, nStepsOn, -1, initT0=T0, initDose=D0, **kw)
        Tmax = Ton if n == nCurrent else np.maximum(Tmax, Ton)
        new = [Pon]
        if off > 0:
            FT, FD, _, _, Poff = R.BHTE(cool, mm, ml, dx, off, 0, -1, DutyCycle=duty, initT0=Ton, initDose=Don, **kw)
            new.append(Poff)
        else:
            FT, FD = Ton, Don
        TP = np.hstack(new) if n == 0 else np.hstack([TP] + new)
        if (n + 1) % rep == 0 and pause > 0:
            FT, FD, _, _, Pp = R.BHTE(cool, mm, ml, dx, pause, 0, -1, DutyCycle=duty, initT0=FT, initDose=FD, **kw)
            TP = np.hstack((TP, Pp))
        if sub and ((n + 1) % limit == 0 or n + 1 == total):
            break
    return Tmax, Don, FT, FD, TP, n + 1


def _equal(a, b):
    assert len(a) == len(b) == 6
    for k, (x, y) in enumerate(zip(a[:5], b[:5])):
        assert x.shape == y.shape and np.array_equal(x, y), 'return %d differs' % k
    assert a[5] == b[5]


def _ftz(a):
    """the library flushes subnormal float32 results to zero (tests/test_bhte_gpu.py holds the returned heat source to this)"""
    a = np.array(a, np.float32)
    a[np.abs(a) < np.finfo(np.float32).tiny] = 0
    return a


def _against_oracle(got, args, fields, mm, ml, dx, nOn, nStepsOn, dt, duty, mpm, T0, what):
    """RunBHTECycles' six returns of a run from nCurrent = 0 (start T0, no dose) against the oracle's history over protocol_schedule"""
    from babelbrain_amd import RayleighAndBHTE as R
    fields = np.asarray(fields)
    single = fields.ndim == 3
    sched, caps, _, nNext = R.protocol_schedule(*args, nOn, nStepsOn, multi_field=not single)
    cd, cp, qf = R.bhte_coefficients(ml, dx, dt, duty if single else 1.0)
    q = _ftz((fields.astype(np.float32) ** 2) * qf[mm])
    h = BR.history(T0, np.zeros(mm.shape, np.float32), q, mm, cd, cp, 37.0, dt, sched)
    assert h.n == len(sched) == got[4].shape[1] and got[5] == nNext and len(caps) >= 1
    BR.assert_equal(got[0], h.running_max(caps), what + ': maximum over the captures', 'ijk', mm)
    BR.assert_equal(got[2], h.T, what + ': final temperature', 'ijk', mm)
    BR.assert_equal(got[4], h.points(BR.points_of(mpm)), what + ': point series', 'ps')
    last = int(caps[-1])
    a = BR.assert_dose(got[1], h.dose64(last), last, what + ': dose at the last capture', T=h.at_boundary(last), mat=mm)
    b = BR.assert_dose(got[3], h.dose64(), h.n, what + ': final dose', T=h.T, mat=mm)
    print('%s: dose at the last capture at %.3f of the bound, final dose at %.3f' % (what, a, b))
    return h


def test_single_field_protocol_equals_chained_calls():
    from babelbrain_amd import RayleighAndBHTE as R
    N = (40, 36, 44)
    mm, fields, mpm = _problem(N, 11)
    ml = _materials()
    dx, dt = 4e-4, 0.02
    args = (0, 3, 6, 14, 9, 100)                      # nCurrent, Repetitions, 2 groups, pause, OFF, limit
    got = R.RunBHTECycles(*args, 'pressure.npz', fields[0], mm, ml, dx, 13, 7, -1, 1, dt, 0.7, 'HIP', mpm, 37.0, None, None, None, None)
    ref = _chained(*args, True, fields[0], mm, ml, dx, 13, 7, dt, 0.7, mpm, 37.0, None, None, None, None)
    _equal(got, ref)
    assert got[4].shape == (3, 6 * (13 + 9) + 2 * 14) and got[5] == 6
    assert got[0].max() > 39.0 and got[0].max() > got[2].max()  # the peak over the ON ends is above the cooled end state
    assert not np.array_equal(got[1], got[3])                   # the dose at the last ON end is not the final dose


def test_steered_fields_protocol_equals_chained_calls():
    from babelbrain_amd import RayleighAndBHTE as R
    N = (36, 40, 44)
    mm, fields, mpm = _problem(N, 12, centres=((-6, 0), (5, 4), (0, -7)), amp=4.0e6)
    ml = _materials()
    dx, dt = 4e-4, 0.02
    onoff = np.array([[5, 3]] * 3, np.int32)
    args = (0, 2, 4, 10, 6, 100)
    got = R.RunBHTECycles(*args, np.zeros(3), fields, mm, ml, dx, 29, onoff, -1, 1, dt, 0.5, 'HIP', mpm, 37.0, None, None, None, None)
    ref = _chained(*args, False, fields, mm, ml, dx, 29, onoff, dt, 0.5, mpm, 37.0, None, None, None, None)
    _equal(got, ref)
    assert got[0].max() > 38.0
    _against_oracle(got, args, fields, mm, ml, dx, 29, onoff, dt, 0.5, mpm, np.full(N, 37.0, np.float32), 'steered protocol 36x40x44')


def test_no_off_no_pause_from_previous_data():
    from babelbrain_amd import RayleighAndBHTE as R
    N = (30, 28, 34)
    mm, fields, mpm = _problem(N, 13)
    ml = _materials()
    rng = np.random.default_rng(3)
    prev = {'FinalTemp': (37.0 + rng.random(N)).astype(np.float32), 'FinalDose': (1e-3 * rng.random(N)).astype(np.float32)}
    args = (0, 2, 4, 0, 0, 100)
    got = R.RunBHTECycles(*args, 'p.npz', fields[0], mm, ml, 4e-4, 11, 6, -1, 1, 0.02, 1.0, 'HIP', mpm, 37.0, None, None, None, prev)
    ref = _chained(*args, True, fields[0], mm, ml, 4e-4, 11, 6, 0.02, 1.0, mpm, 37.0, None, None, None, prev)
    _equal(got, ref)
    assert np.array_equal(got[1], got[3]) and got[4].shape == (3, 44)       # no OFF call: the last ON end is the end


def test_chunked_calls_combine_to_the_whole_run():
    """bRunInSubProcess chunks of 2 iterations (splitting the groups of 3), combined as the caller does (:1094-1104)."""
    from babelbrain_amd import RayleighAndBHTE as R
    N = (32, 30, 36)
    mm, fields, mpm = _problem(N, 14)
    ml = _materials()
    common = ('p.npz', fields[0], mm, ml, 4e-4, 9, 5, -1, 1, 0.02, 1.0, 'HIP', mpm, 37.0)
    whole = R.RunBHTECycles(0, 3, 6, 7, 4, 2, *common, None, None, None, None)
    nCurrent, TP, FT, FD = 0, None, None, None
    chunks = 0
    while nCurrent < 6:
        res = R.RunBHTECycles(nCurrent, 3, 6, 7, 4, 2, *common, TP, FT, FD, None, bRunInSubProcess=True)
        ResTemp = res[0] if nCurrent == 0 else np.maximum(ResTemp, res[0])
        ResDose, FT, FD, TP, nCurrent = res[1:]
        chunks += 1
    assert chunks == 3
    _equal((ResTemp, ResDose, FT, FD, TP, nCurrent), whole)
    # and the chained reference calls, chunk by chunk
    nCurrent, TPc, FTc, FDc = 0, None, None, None
    while nCurrent < 6:
        res = _chained(nCurrent, 3, 6, 7, 4, 2, True, fields[0], mm, ml, 4e-4, 9, 5, 0.02, 1.0, mpm, 37.0, TPc, FTc, FDc, None, sub=True)
        RT = res[0] if nCurrent == 0 else np.maximum(RT, res[0])
        RD, FTc, FDc, TPc, nCurrent = res[1:]
    _equal((RT, RD, FTc, FDc, TPc, nCurrent), whole)


@pytest.mark.parametrize('nOn,nStepsOn,off,pause', [(1, 1, 2, 3), (3, 2, 1, 5), (5, 3, 2, 1), (2, 1, 3, 2), (5, 5, 5, 5)])
def test_short_segments_split_the_passes(nOn, nStepsOn, off, pause):
    """Segments of 1, 2, 3 and 5 steps put captures and changes of field inside would-be 4-step passes."""
    from babelbrain_amd import RayleighAndBHTE as R
    N = (24, 20, 28)
    mm, fields, mpm = _problem(N, 15)
    ml = _materials()
    dx, dt = 4e-4, 0.02
    args = (0, 2, 4, pause, off, 100)
    got = R.RunBHTECycles(*args, 'p.npz', fields[0], mm, ml, dx, nOn, nStepsOn, -1, 1, dt, 1.0, 'HIP', mpm, 37.0, None, None, None, None)
    ref = _chained(*args, True, fields[0], mm, ml, dx, nOn, nStepsOn, dt, 1.0, mpm, 37.0, None, None, None, None)
    _equal(got, ref)
    sched, _, _, _ = R.protocol_schedule(*args, nOn, nStepsOn)
    cd, cp, qf = R.bhte_coefficients(ml, dx, dt, 1.0)
    q = (fields.astype(np.float32) ** 2) * qf[mm]
    To, Do = BO.bhte(np.full(N, 37.0, np.float32), np.zeros(N, np.float32), q, mm, cd, cp, 37.0, dt, len(sched), 0, field_of_step=sched)
    assert rel_l2(got[2] - 37.0, To - 37.0) < 1e-5 and rel_l2(got[3], Do) < 1e-5
    h = _against_oracle(got, args, fields[0], mm, ml, dx, nOn, nStepsOn, dt, 1.0, mpm, np.full(N, 37.0, np.float32), 'protocol on %d off %d pause %d' % (nOn, off, pause))
    assert np.array_equal(h.T, To)
