"""Host side of RunBHTECycles (CalculateTemperatureEffects.py:259-460): the protocol schedule against a restatement of the
reference loop's step accounting, and the argument checks that run before any device call. No GPU needed."""
import itertools

import numpy as np
import pytest

from babelbrain_amd import RayleighAndBHTE as R


def _reference_calls(nCurrent, Repetitions, TotalIterations, pause, off, limit, nOn, nStepsOn, multi, sub):
    """The BHTE calls the reference loop makes (:349-459), one (kind, iteration, fields of its steps) per call."""
    calls, n = [], nCurrent
    for n in range(nCurrent, TotalIterations):
        if multi:
            on = R.field_schedule(nStepsOn, nOn).tolist()
        else:
            on = [0 if s < nStepsOn else -1 for s in range(nOn)]
        calls.append(('on', n, on))
        if off > 0:
            calls.append(('off', n, [-1] * off))
        if (n + 1) % Repetitions == 0 and pause > 0:
            calls.append(('pause', n, [-1] * pause))
        if sub and ((n + 1) % limit == 0 or n + 1 == TotalIterations):
            break
    return calls, n + 1


CASES = [
    # nCurrent, Repetitions, TotalIterations, pause, off, limit, TotalDurationSteps, nStepsOn, sub
    (0, 1, 3, 0, 0, 100, 7, 3, False),
    (0, 3, 6, 14, 9, 100, 13, 7, False),
    (0, 3, 6, 0, 9, 100, 13, 13, False),
    (0, 1, 4, 5, 0, 100, 4, 9, False),          # nStepsOn beyond the ON call
    (0, 3, 9, 4, 2, 2, 5, 3, True),             # chunks of 2 split the groups of 3
    (2, 3, 9, 4, 2, 2, 5, 3, True),
    (4, 3, 9, 4, 2, 4, 5, 3, True),
    (5, 3, 9, 4, 2, 100, 5, 3, False),          # resume, no chunking
    (7, 3, 9, 0, 0, 5, 1, 1, True),
]


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('multi', [False, True])
def test_schedule_matches_reference_loop(case, multi):
    nCurrent, rep, total, pause, off, limit, nOn, nStepsOn, sub = case
    onoff = np.array([[2, 1], [1, 3], [3, 0]]) if multi else nStepsOn
    sched, caps, calls, nNext = R.protocol_schedule(nCurrent, rep, total, pause, off, limit, nOn, onoff, multi, sub)
    ref, refNext = _reference_calls(nCurrent, rep, total, pause, off, limit, nOn, onoff, multi, sub)
    assert nNext == refNext
    assert sched.dtype == np.int32 and caps.dtype == np.int32
    assert sched.tolist() == list(itertools.chain.from_iterable(c[2] for c in ref))
    # every call's slice of TemperaturePoints: calls back to back, in the reference's order
    first = np.cumsum([0] + [len(c[2]) for c in ref])[:-1]
    assert [(k, n, f, s) for k, n, f, s in calls] == [(c[0], c[1], int(f0), len(c[2])) for c, f0 in zip(ref, first)]
    assert len(sched) == sum(len(c[2]) for c in ref)
    # one capture at the end of every ON call
    assert caps.tolist() == [int(f0) + len(c[2]) for c, f0 in zip(ref, first) if c[0] == 'on']
    assert np.all(np.diff(caps) >= 0) and (len(caps) == 0 or caps[-1] <= len(sched))


def test_schedule_chunks_cover_the_whole_run():
    """Chunks resumed from the returned nCurrent give the schedule of one unchunked run."""
    whole, wcaps, _, n = R.protocol_schedule(0, 3, 8, 6, 4, 100, 5, 2)
    assert n == 8
    parts, caps, n, base = [], [], 0, 0
    while n < 8:
        s, c, _, n = R.protocol_schedule(n, 3, 8, 6, 4, 3, 5, 2, bRunInSubProcess=True)
        parts.append(s); caps += (c + base).tolist(); base += len(s)
    assert len(parts) == 3 and np.array_equal(np.concatenate(parts), whole) and caps == wcaps.tolist()


def test_schedule_rejects():
    with pytest.raises(ValueError):
        R.protocol_schedule(3, 3, 3, 0, 0, 100, 5, 2)          # nothing left to run
    with pytest.raises(ValueError):
        R.protocol_schedule(0, 0, 3, 0, 0, 100, 5, 2)
    with pytest.raises(ValueError):
        R.protocol_schedule(0, 1, 3, 0, 0, 0, 5, 2, bRunInSubProcess=True)
    with pytest.raises(ValueError):
        R.protocol_schedule(0, 1, 3, 0, -1, 100, 5, 2)
    with pytest.raises(ValueError):
        R.protocol_schedule(0, 1, 2, 0, 0, 100, 2 ** 30, 2)     # 2^31 steps
    s, _, _, _ = R.protocol_schedule(0, 1, 1, 0, 0, 100, 2 ** 20, 2)
    assert len(s) == 2 ** 20


def _args(**kw):
    N = (8, 7, 9)
    ml = {k: np.array(v) for k, v in dict(Density=[1000.0, 1041.0], SoS=[1500.0, 1562.0], Attenuation=[0.0, 3.45],
                                          SpecificHeat=[4178.0, 3630.0], Conductivity=[0.6, 0.51], Perfusion=[0.0, 559.0],
                                          Absorption=[0.0, 0.85], InitTemperature=[37.0, 37.0]).items()}
    mpm = np.zeros(N, np.uint32); mpm[4, 3, 4] = 1
    a = dict(nCurrent=0, Repetitions=2, TotalIterations=4, TotalDurationBetweenGroups=3, TotalDurationStepsOff=2,
             LimitBHTEIterationsPerProcess=100, InputPData='p.npz', PMaps=np.ones(N), MaterialMap=np.ones(N, np.uint8),
             MaterialList=ml, dx=1e-3, TotalDurationSteps=5, nStepsOn=3, cy=-1, nFactorMonitoring=1, dt=0.01, DutyCycle=1.0,
             Backend='HIP', MonitoringPointsMap=mpm, stableTemp=37.0, TemperaturePoints=None, FinalTemp=None, FinalDose=None,
             PreviousData=None)
    a.update(kw)
    return a


@pytest.mark.parametrize('bad', [
    dict(MaterialMap=np.ones((8, 7, 8), np.uint8)),                                       # shapes disagree
    dict(PMaps=np.ones((2, 8, 7, 9))),                                                    # one field expected
    dict(InputPData=np.ones(1), PMaps=np.ones((8, 7, 9))),                                # steered fields expected
    dict(MonitoringPointsMap=None),
    dict(MonitoringPointsMap=np.ones((8, 7, 8), np.uint32)),
    dict(InputPData=np.ones(1), PMaps=np.ones((3, 8, 7, 9)), nStepsOn=np.array([[2, 1], [2, 1]])),   # rows != fields
    dict(InputPData=np.ones(1), PMaps=np.ones((2, 8, 7, 9)), nStepsOn=np.array([2, 1])),
    dict(TotalDurationSteps=2 ** 30, TotalIterations=2),                                  # schedule over 2^31 - 1 steps
    dict(nCurrent=4),                                                                     # nothing to run
    dict(nCurrent=1, FinalTemp=np.full((8, 7, 8), 37.0), FinalDose=np.zeros((8, 7, 9)),
         TemperaturePoints=np.zeros((1, 10), np.float32)),                                # resume state of another shape
    dict(nCurrent=1, FinalTemp=np.full((8, 7, 9), 37.0), FinalDose=np.zeros((8, 7, 9)), TemperaturePoints=None),
    dict(PreviousData={'FinalTemp': np.full((8, 7, 8), 37.0), 'FinalDose': np.zeros((8, 7, 9))}),
])
def test_run_cycles_rejects_before_any_device_call(bad, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(R._engine, 'load_library', no_device)
    with pytest.raises(ValueError):
        R.RunBHTECycles(**_args(**bad))
