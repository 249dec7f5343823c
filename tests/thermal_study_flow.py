"""The Step-3 flow of CalculateTemperatureEffects.py:847-1193 written with the SEPARATE public calls and numpy glue, volumes through the host between
them: `flow_by_calls(case)`. It is what babelbrain_amd.ThermalStudy.thermal_exposure is compared with, one line per comparison. `make_case` builds
the inputs from tests/thermal_oracle.build_case (the selections already pinned to the reference) plus the thermal property rows and a time plan;
`oracle_calls()` substitutes the numpy oracles (tests/thermal_oracle.py, tests/median_oracle.py, oracle/bhte_oracle.py) for the device calls, so
the flow itself runs without a GPU."""
import types

import numpy as np

from tests import thermal_oracle as TO

VOLUMES = ('p_map', 'TempEndFUS', 'DoseEndFUS', 'FinalTemp', 'FinalDose')
SMALL = ('mSkin', 'mBrain', 'mSkull', 'PressureRatio', 'RatioLosses', 'p_map_central', 'MaterialMap_central', 'MaxBrainPressure', 'TimeProfileTarget',
         'TempProfileTarget', 'TemperaturePoints', 'MI', 'TI', 'TIC', 'TIS', 'CEMBrain', 'CEMSkin', 'CEMSkull', 'MaxIsppa', 'MaxIspta', 'Ispta', 'Isppa')


def make_case(shape=(24, 22, 40), seed=0, fields=1, previous=False, Repetitions=2, NumberGroupedSonications=2, DurationUS=0.06, DurationOff=0.03,
              Pause=0.02, limit=100, dt=0.01, **build):
    """A whole case: build_case(shape, seed, **build) with the bio-heat rows of the material list, `fields` pressure fields (1: the 3-D arrays of
    the one-field flow), the time plan and, with `previous`, the PreviousData of an earlier run."""
    c = TO.build_case(shape, seed, **build)
    rng = np.random.default_rng(seed + 1000)
    nMat = c['nMat']
    ML = dict(c['MaterialList'])
    ML['SpecificHeat'] = np.concatenate(([4178.0], rng.uniform(1300.0, 3700.0, nMat - 1)))
    ML['Conductivity'] = np.concatenate(([0.6], rng.uniform(0.3, 0.55, nMat - 1)))
    ML['Perfusion'] = np.concatenate(([0.0], rng.uniform(10.0, 560.0, nMat - 1)))
    ML['Absorption'] = np.concatenate(([0.0], rng.uniform(0.15, 0.85, nMat - 1)))
    ML['Attenuation'] = np.concatenate(([0.0], rng.uniform(2.0, 80.0, nMat - 1)))
    ML['InitTemperature'] = np.full(nMat, 37.0)
    c['MaterialList'] = ML
    if fields > 1:
        c['pAmp'] = np.stack([np.roll(c['pAmp'], f, axis=0) * np.float32(1.0 + 0.07 * f) for f in range(fields)])
        c['pAmpWater'] = np.stack([np.roll(c['pAmpWater'], f, axis=0) * np.float32(1.0 + 0.05 * f) for f in range(fields)])
        c['nStepsOnOffList'] = np.array([[2, 1]] * fields, np.int64)
    c['Input']['TargetLocation'] = c['LocIJK']
    c.update(fields=fields, Isppa=5.0, DutyCycle=0.3, Frequency=500e3, dt=dt, DurationUS=DurationUS, DurationOff=DurationOff, Repetitions=Repetitions,
             NumberGroupedSonications=NumberGroupedSonications, PauseBetweenGroupedSonications=Pause, BaselineTemperature=37.0, TxSystem='CTX_500',
             bSegmentedBrain=bool(build.get('segmented')), bForceHomogenousMedium=bool(build.get('homogeneous')), benchmark=build.get('benchmark'),
             bApplyMedianPressure=True, FixedAcousticPower=0.0, LimitBHTEIterationsPerProcess=limit, PreviousData=None)
    if previous:
        c['PreviousData'] = dict(FinalTemp=(37.0 + rng.uniform(0.0, 0.5, shape)).astype(np.float32), FinalDose=rng.uniform(0.0, 1e-3, shape).astype(np.float32),
                                 TempEndFUS=(37.0 + rng.uniform(0.0, 1.5, shape)).astype(np.float32), TimeProfileTarget=np.arange(5) * dt,
                                 TempProfileTarget=np.full(5, 37.25, np.float32), TemperaturePoints=np.full((4, 5), 37.25, np.float32))
    return c


def exposure_arguments(c):
    """(args, kwargs) of thermal_exposure for a case"""
    kw = {k: c[k] for k in ('Repetitions', 'NumberGroupedSonications', 'PauseBetweenGroupedSonications', 'BaselineTemperature', 'TxSystem', 'bSegmentedBrain',
                            'bForceHomogenousMedium', 'benchmark', 'bApplyMedianPressure', 'FixedAcousticPower', 'PreviousData', 'LimitBHTEIterationsPerProcess')}
    kw['nStepsOnOffList'] = c.get('nStepsOnOffList')
    return (c['pAmp'], c['pAmpWater'], c['MaterialMap'], c['MaterialList'], c['Input'], c['LocIJK'], c['Isppa'], c['DutyCycle'], c['Frequency'], c['dt'],
            c['DurationUS'], c['DurationOff']), kw


# ---------------------------------------------------------------- the two sets of calls ----------------------------------------------------------------

def device_calls():
    """today's public calls on the device"""
    from babelbrain_amd import MedianFilter as MF, RayleighAndBHTE as R, ThermalAnalysis as TA

    def analyze(pAmp, MaterialMap, LocIJK, Input, MaterialList, pAmpWater, Isppa, xf, yf, zf, SelBrain, homogeneous, segmented, TxSystem, IdRegionBenchmark,
                FixedAcousticPower):
        return TA.AnalyzeLosses(pAmp, MaterialMap, LocIJK, Input, MaterialList, pAmpWater, Isppa, xf, yf, zf, SelBrain, homogeneous, segmented, TxSystem,
                                IdRegionBenchmark, FixedAcousticPower=FixedAcousticPower)

    def hottest(ResTemp, MaterialMap, sel):
        return TA.hottest_points(ResTemp, MaterialMap, sel['classOf'])

    def metrics(ResTemp, FinalDose, p_map, MaterialMap, sel, MaterialList, BrainID, Frequency, DutyCycle, Isppa):
        return TA.exposure_metrics(ResTemp, FinalDose, p_map, MaterialMap, sel['classOf'], MaterialList, BrainID, Frequency, DutyCycle, Isppa)
    return types.SimpleNamespace(median_in_region=MF.median_in_region, AnalyzeLosses=analyze, BHTE=R.BHTE, BHTEMultiplePressureFields=R.BHTEMultiplePressureFields,
                                 RunBHTECycles=R.RunBHTECycles, hottest_points=hottest, exposure_metrics=metrics)


def oracle_calls():
    """the numpy oracles in place of the device calls: same signatures"""
    from babelbrain_amd import RayleighAndBHTE as R         # bhte_coefficients, field_schedule, protocol_schedule: host arithmetic
    from oracle import bhte_oracle as BO
    from tests import bhte_reference as BR
    from tests.median_oracle import median_oracle

    def median_in_region(volume, region, size=3):
        v = np.asarray(volume)
        if v.ndim == 4:
            return np.stack([median_in_region(f, region, size) for f in v])
        out = v.copy()
        out[region] = median_oracle(v, size)[region]
        return out

    def analyze(pAmp, MaterialMap, LocIJK, Input, MaterialList, pAmpWater, Isppa, xf, yf, zf, SelBrain, homogeneous, segmented, TxSystem, IdRegionBenchmark,
                FixedAcousticPower):
        return TO.AnalyzeLosses(pAmp, MaterialMap, LocIJK, Input, MaterialList, pAmpWater, Isppa, xf, yf, zf, SelBrain, homogeneous, segmented, TxSystem,
                                IdRegionBenchmark, FixedAcousticPower)

    def run(fields, sched, MaterialMap, MaterialList, dx, dt, duty, stableTemp, mpm, initT0, initDose):
        cd, cp, qf = R.bhte_coefficients(MaterialList, dx, dt, duty)
        P32 = np.asarray(fields, np.float32)
        q = (P32 * P32) * qf[MaterialMap]
        T0 = np.full(MaterialMap.shape, 0, np.float32) + np.asarray(MaterialList['InitTemperature'], np.float32)[MaterialMap] if initT0 is None else initT0
        D0 = np.zeros(MaterialMap.shape, np.float32) if initDose is None else initDose
        T, D = BO.bhte(T0, D0, q, MaterialMap, cd, cp, stableTemp, dt, len(sched), 0, field_of_step=list(sched))
        out = (T, D, np.zeros((0,), np.float32), q)
        if mpm is not None:
            where = BR.points_of(mpm)
            steps = list(BO.bhte_steps(T0, q, MaterialMap, cd, cp, stableTemp, list(sched)))
            out = out + (np.array([[s[w] for s in steps] for w in where], np.float32).reshape(len(where), len(sched)),)
        return out

    def BHTE(P, MaterialMap, MaterialList, dx, nSteps, nStepsOn, cy, nFactorMonitoring=1, dt=0.1, DutyCycle=1.0, Backend='', stableTemp=37.0,
             MonitoringPointsMap=None, initT0=None, initDose=None):
        sched = BO.single_field_schedule(int(nSteps), int(nStepsOn))
        out = run(np.asarray(P)[None], sched, MaterialMap, MaterialList, dx, dt, DutyCycle, stableTemp, MonitoringPointsMap, initT0, initDose)
        return out[:3] + (out[3][0],) + out[4:]

    def BHTEMulti(P, MaterialMap, MaterialList, dx, nSteps, nStepsOnOffList, cy, nFactorMonitoring=1, dt=0.1, Backend='', stableTemp=37.0,
                  MonitoringPointsMap=None, initT0=None, initDose=None):
        return run(P, R.field_schedule(nStepsOnOffList, int(nSteps)), MaterialMap, MaterialList, dx, dt, 1.0, stableTemp, MonitoringPointsMap, initT0, initDose)

    def RunBHTECycles(nCurrent, Repetitions, TotalIterations, pause, off, limit, InputPData, PMaps, MaterialMap, MaterialList, dx, nOn, nStepsOn, cy, fm, dt,
                      DutyCycle, Backend, mpm, stableTemp, TP, FT, FD, PreviousData, bRunInSubProcess=False):
        """the reference's loop (:349-459) over the oracle's BHTE"""
        single = isinstance(InputPData, str)
        cool = np.zeros(MaterialMap.shape)
        kw = dict(dt=dt, MonitoringPointsMap=mpm, stableTemp=stableTemp)
        n = nCurrent
        for n in range(nCurrent, TotalIterations):
            if n > 0:
                T0, D0 = FT, FD
            elif PreviousData is not None:
                T0, D0 = PreviousData['FinalTemp'], PreviousData['FinalDose']
            else:
                T0 = D0 = None
            if single:
                Ton, Don, _, _, Pon = BHTE(PMaps, MaterialMap, MaterialList, dx, nOn, nStepsOn, -1, DutyCycle=DutyCycle, initT0=T0, initDose=D0, **kw)
            else:
                Ton, Don, _, _, Pon = BHTEMulti(PMaps, MaterialMap, MaterialList, dx, nOn, nStepsOn, -1, initT0=T0, initDose=D0, **kw)
            Tmax = Ton if n == nCurrent else np.maximum(Tmax, Ton)
            new = [Pon]
            if off > 0:
                FT, FD, _, _, Poff = BHTE(cool, MaterialMap, MaterialList, dx, off, 0, -1, DutyCycle=DutyCycle, initT0=Ton, initDose=Don, **kw)
                new.append(Poff)
            else:
                FT, FD = Ton, Don
            TP = np.hstack(new) if n == 0 else np.hstack([TP] + new)
            if (n + 1) % Repetitions == 0 and pause > 0:
                FT, FD, _, _, Pp = BHTE(cool, MaterialMap, MaterialList, dx, pause, 0, -1, DutyCycle=DutyCycle, initT0=FT, initDose=FD, **kw)
                TP = np.hstack((TP, Pp))
            if bRunInSubProcess and ((n + 1) % limit == 0 or n + 1 == TotalIterations):
                break
        return Tmax, Don, FT, FD, TP, n + 1

    def hottest(ResTemp, MaterialMap, sel):
        return TO.monitoring_points_map(ResTemp, sel['SelSkin'], sel['SelBrain'], sel['SelSkull'], [0, 0, 0])[1:]

    def metrics(ResTemp, FinalDose, p_map, MaterialMap, sel, MaterialList, BrainID, Frequency, DutyCycle, Isppa):
        if isinstance(p_map, tuple):
            p_map = p_map[0] * p_map[1]
        return TO.exposure_metrics(ResTemp, FinalDose, p_map, sel['SelBrain'], sel['SelSkin'], sel['SelSkull'], MaterialList, BrainID, Frequency, DutyCycle, Isppa)
    return types.SimpleNamespace(median_in_region=median_in_region, AnalyzeLosses=analyze, BHTE=BHTE, BHTEMultiplePressureFields=BHTEMulti,
                                 RunBHTECycles=RunBHTECycles, hottest_points=hottest, exposure_metrics=metrics)


# ---------------------------------------------------------------- the flow ----------------------------------------------------------------

def flow_by_calls(c, calls=None, skip=()):
    """:847-1193 statement by statement over `calls` (default: the device's public calls). Returns the volume-derived entries of SaveDict, its five
    volumes included, and 'kernel_ms' where the calls report it. skip: statements left out on purpose ('median', 'merge', 'scale'): the planted
    faults of the host test."""
    from babelbrain_amd import RayleighAndBHTE as R, ThermalAnalysis as TA
    calls = calls or device_calls()
    dt, DutyCycle, Isppa, Frequency = c['dt'], c['DutyCycle'], c['Isppa'], c['Frequency']
    MaterialMap, MaterialList, Input = c['MaterialMap'], c['MaterialList'], c['Input']
    single = c['fields'] == 1
    InputPData = 'file' if single else ['file'] * c['fields']
    kernel_ms = [0.0]

    def timed(module):
        if getattr(module, 'last_kernel_ms', None) is not None:
            kernel_ms[0] += module.last_kernel_ms
    nFactorMonitoring = int(50e-3 / dt)
    if nFactorMonitoring == 0:
        nFactorMonitoring = 1
    TotalDurationSteps = int((c['DurationUS'] + .001) / dt)
    nStepsOn = int(c['DurationUS'] / dt)
    if nFactorMonitoring > TotalDurationSteps:
        nFactorMonitoring = 1
    TotalDurationStepsOff = int((c['DurationOff'] + .001) / dt)
    TotalDurationBetweenGroups = int(c['PauseBetweenGroupedSonications'] / dt)
    xf, yf, zf = Input['x_vec'], Input['y_vec'], Input['z_vec']
    LocIJK = Input['TargetLocation'].flatten()
    homogeneous, segmented, benchmark = c['bForceHomogenousMedium'], c['bSegmentedBrain'], c['benchmark']
    SelBrain, SelSkin, SelSkull, BrainID, IdRegionBenchmark = TO.selections(MaterialMap, 'MaterialMapCT' in Input, segmented, homogeneous, benchmark)
    bench = None
    if benchmark is not None and not homogeneous:
        bench = dict(benchmark)
        if bench['TestType'] == 3:
            bench['maxMaterial'] = int(MaterialMap.max())
    sel = dict(SelBrain=SelBrain, SelSkin=SelSkin, SelSkull=SelSkull,
               classOf=TA.region_tables(c['nMat'], 'MaterialMapCT' in Input, segmented, homogeneous, bench)['classOf'])
    bNormalOperation = not homogeneous and benchmark is None
    cx, cy, cz = LocIJK[0], LocIJK[1], LocIJK[2]
    pAmp, pAmpWater = c['pAmp'].copy(), c['pAmpWater'].copy()
    AllInputs, AllInputsWater = pAmp, pAmpWater
    from babelbrain_amd import MedianFilter as MF
    if bNormalOperation and c['bApplyMedianPressure'] and 'median' not in skip:
        if single:
            pAmp = calls.median_in_region(pAmp, SelSkull, 3)
        else:
            AllInputsWater = calls.median_in_region(AllInputsWater, SelSkull, 3)
        timed(MF)
    tail = (xf, yf, zf, SelBrain, homogeneous, segmented, c['TxSystem'], IdRegionBenchmark, c['FixedAcousticPower'])
    if single:
        PressureRatio, RatioLosses = calls.AnalyzeLosses(pAmp, MaterialMap, LocIJK, Input, MaterialList, pAmpWater, Isppa, *tail)
        timed(TA)
    else:
        PressureRatio = np.zeros(len(InputPData), dtype=AllInputs.dtype)
        RatioLosses = np.zeros(len(InputPData), dtype=AllInputs.dtype)
        for n in range(len(InputPData)):
            PressureRatio[n], RatioLosses[n] = calls.AnalyzeLosses(AllInputs[n], MaterialMap, LocIJK, Input, MaterialList, AllInputsWater[n], Isppa, *tail)
            timed(TA)
    PreviousData = c['PreviousData']
    initT0 = initDose = None
    if PreviousData is not None:
        initT0, initDose = PreviousData['FinalTemp'], PreviousData['FinalDose']
    dx = Input['x_vec'][1] - Input['x_vec'][0]
    if single:
        PMaps = pAmp * PressureRatio if 'scale' not in skip else pAmp
        ResTemp, ResDose, MonitorSlice, Qarr = calls.BHTE(PMaps, MaterialMap, MaterialList, dx, TotalDurationSteps, nStepsOn, -1, nFactorMonitoring=nFactorMonitoring,
                                                          dt=dt, DutyCycle=DutyCycle, Backend='HIP', stableTemp=c['BaselineTemperature'], initT0=initT0,
                                                          initDose=initDose)
    else:
        InputsBHTE = AllInputs.copy()
        for n in range(len(InputPData)):
            if 'scale' not in skip:
                InputsBHTE[n, :, :, :] *= PressureRatio[n]
        ResTemp, ResDose, MonitorSlice, Qarr = calls.BHTEMultiplePressureFields(InputsBHTE, MaterialMap, MaterialList, dx, TotalDurationSteps, c['nStepsOnOffList'],
                                                                                -1, nFactorMonitoring=nFactorMonitoring, dt=dt, Backend='HIP',
                                                                                stableTemp=c['BaselineTemperature'], initT0=initT0, initDose=initDose)
        PMaps = InputsBHTE
    timed(R)
    if PreviousData is not None and 'merge' not in skip:
        ResTemp = np.maximum(ResTemp, PreviousData['TempEndFUS'])
    mSkin, mBrain, mSkull = calls.hottest_points(ResTemp, MaterialMap, sel)
    timed(TA)
    MonitoringPointsMap = TA.monitoring_points_map(mSkin, mBrain, mSkull, LocIJK, MaterialMap.shape, homogeneous, bench)
    TOTAL_Iterations = c['NumberGroupedSonications'] * c['Repetitions']
    nStepsOnIn = nStepsOn if single else c['nStepsOnOffList']
    FinalTemp = FinalDose = TemperaturePoints = None
    limit = c['LimitBHTEIterationsPerProcess']
    args = (c['Repetitions'], TOTAL_Iterations, TotalDurationBetweenGroups, TotalDurationStepsOff, limit, InputPData, PMaps, MaterialMap, MaterialList, dx,
            TotalDurationSteps, nStepsOnIn, -1, nFactorMonitoring, dt, DutyCycle, 'HIP', MonitoringPointsMap, c['BaselineTemperature'])
    if TOTAL_Iterations <= limit:
        ResTemp, ResDose, FinalTemp, FinalDose, TemperaturePoints, nCurrent = calls.RunBHTECycles(0, *args, TemperaturePoints, FinalTemp, FinalDose, PreviousData)
        timed(R)
    else:
        nCurrent = 0
        while nCurrent < TOTAL_Iterations:                   # the chunks of :1070-1105, without the processes
            first = nCurrent == 0
            res = calls.RunBHTECycles(nCurrent, *args, TemperaturePoints, FinalTemp, FinalDose, PreviousData, bRunInSubProcess=True)
            timed(R)
            ResTemp = res[0] if first else np.maximum(ResTemp, res[0])
            ResDose, FinalTemp, FinalDose, TemperaturePoints, nCurrent = res[1:]
    if PreviousData is not None and 'merge' not in skip:
        ResTemp = np.maximum(ResTemp, PreviousData['TempEndFUS'])
    S = dict(mSkin=np.array(mSkin).astype(int), mBrain=np.array(mBrain).astype(int), mSkull=np.array(mSkull).astype(int), dt=dt)
    if single:
        S['p_map'] = PMaps if 'scale' in skip else pAmp * PressureRatio
        S['p_map_central'] = pAmp[:, cy, :] * PressureRatio if 'scale' not in skip else pAmp[:, cy, :]
    else:
        S['p_map'] = InputsBHTE.max(axis=0)
        S['p_map_central'] = InputsBHTE.max(axis=0)[:, cy, :]
    S['MaterialMap_central'] = MaterialMap[:, cy, :]
    S['PressureRatio'], S['RatioLosses'] = PressureRatio, RatioLosses
    p_for_metrics = ((pAmp, PressureRatio) if 'scale' not in skip else pAmp) if single else S['p_map']
    met = calls.exposure_metrics(ResTemp, FinalDose, p_for_metrics, MaterialMap, sel, MaterialList, BrainID, Frequency, DutyCycle, Isppa)
    timed(TA)
    S['MaxBrainPressure'] = met['MaxBrainPressure']
    if homogeneous:
        IndTarget = 0
    elif benchmark is not None:
        IndTarget = 0 if benchmark['TestType'] == 1 else 1
    elif cx == mBrain[0] and cy == mBrain[1] and cz == mBrain[2]:
        IndTarget = 2
    else:
        IndTarget = 3
    if PreviousData is None:
        S['TimeProfileTarget'] = np.arange(TemperaturePoints.shape[1]) * dt
        S['TempProfileTarget'] = TemperaturePoints[IndTarget, :]
        S['TemperaturePoints'] = TemperaturePoints
    else:
        S['TimeProfileTarget'] = np.hstack((PreviousData['TimeProfileTarget'], PreviousData['TimeProfileTarget'][-1] + dt + np.arange(TemperaturePoints.shape[1]) * dt))
        S['TempProfileTarget'] = np.hstack((PreviousData['TempProfileTarget'], TemperaturePoints[IndTarget, :]))
        S['TemperaturePoints'] = np.hstack((PreviousData['TemperaturePoints'], TemperaturePoints))
    S['MI'] = met['MI']
    S['TI'], S['TIC'], S['TIS'] = met['TI'] - c['BaselineTemperature'], met['TIC'] - c['BaselineTemperature'], met['TIS'] - c['BaselineTemperature']
    for k in ('CEMBrain', 'CEMSkin', 'CEMSkull', 'MaxIsppa', 'MaxIspta', 'Ispta'):
        S[k] = met[k]
    S['Isppa'] = Isppa
    S.update(TempEndFUS=ResTemp, DoseEndFUS=ResDose, FinalTemp=FinalTemp, FinalDose=FinalDose, kernel_ms=kernel_ms[0], Qarr=Qarr)
    return S


def same(got, ref, what):
    """one line per comparison: equal shape, dtype kind and values (float32 volumes go through tests.util.assert_same)"""
    from tests.util import assert_same
    got, ref = np.asarray(got), np.asarray(ref)
    if ref.dtype == np.float32 and ref.ndim >= 1:
        assert_same(got, ref, what)
        return
    assert got.shape == ref.shape, '%s: shape %s against %s' % (what, got.shape, ref.shape)
    assert got.dtype == ref.dtype, '%s: dtype %s against %s' % (what, got.dtype, ref.dtype)
    assert np.array_equal(got, ref), '%s differs: %r against %r' % (what, got, ref)
