"""Step 3 as one device-resident study: the volumes of the reference's ThermalModeling/CalculateTemperatureEffects.py:908-1193 are uploaded once and
stay on the MI355X until a result is asked for (the bfd_thermal handle of include/babelfdtd.h, csrc/bfd_thermal_study.hip).

    with ThermalStudy(pAmp, pAmpWater, MaterialMap, MaterialList, dx) as st:
        st.median_in_region(classOf)                        :908-918
        ratio, losses = st.analyze_losses(LocIJK, Input, Isppa, xf, yf, zf, SelBrain, ...)      :920-946
        st.scale(ratio)                                     pAmp * PressureRatio, without a pass over the volume
        st.bhte(TotalDurationSteps, nStepsOn, ...)          :960-990
        st.merge_previous(PreviousData['TempEndFUS'])       :994, :1108
        st.hottest_points(classOf)                          :996-1001
        st.run_cycles(...)                                  :1042
        st.exposure_metrics(classOf, BrainID, ...)          :1126-1151
        st.fetch('Tmax')                                    one volume to the host, when it is wanted

Every method runs the launch sequence of the public call it mirrors (MedianFilter.median_in_region, ThermalAnalysis.loss_survey / tissue_extrema,
RayleighAndBHTE.BHTE / BHTEMultiplePressureFields / RunBHTECycles) on the resident volumes, so its results equal theirs element by element.
`thermal_exposure` is the whole flow on top of them. The material property tables of :749-841 stay with the caller. There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import RayleighAndBHTE as R
from . import ThermalAnalysis as TA
from . import _engine

NAMES = {'Tmax': 0, 'doseAtCapture': 1, 'T': 2, 'dose': 3, 'q': 4, 'p_map': 5, 'pw': 6, 'p': 7, 'MaterialMap': 8}
FLAG_T0, FLAG_DOSE0, FLAG_START_OVER, FLAG_MERGE_CAPTURES, FLAG_FROM_PREVIOUS = 1, 2, 4, 8, 16
last_kernel_ms = None


class ThermalStudy:
    """The volumes of one thermal calculation on one device. pAmp, pAmpWater: float32 [N1][N2][N3] (one field: the reference's InputPData is a file
    name) or [nFields][N1][N2][N3] (steered fields). MaterialMap: integer ids below len(MaterialList['Density']). dx: the voxel size. The host arrays
    are read once, here; the caller's arrays are never written."""

    def __init__(self, pAmp, pAmpWater, MaterialMap, MaterialList, dx, device=None):
        self._h = None
        p, pw = np.asarray(pAmp), np.asarray(pAmpWater)
        if p.dtype != np.float32 or pw.dtype != np.float32:
            raise TypeError('the pressure fields must be float32, not %s and %s' % (p.dtype, pw.dtype))
        self.single = p.ndim == 3
        if self.single:
            p, pw = p[None], (pw[None] if pw.ndim == 3 else pw)
        m = TA._map(MaterialMap)
        if p.ndim != 4 or p.shape != pw.shape or p.shape[1:] != m.shape or p.shape[0] < 1:
            raise ValueError('the pressure fields have shapes %r and %r, the map %r' % (np.shape(pAmp), np.shape(pAmpWater), m.shape))
        if min(m.shape) < 3:
            raise ValueError('every dimension must be at least 3')
        self.MaterialList, self.MaterialMap, self.dx = MaterialList, MaterialMap, float(dx)
        self.nMat = len(MaterialList['Density'])
        self.nFields, self.shape = p.shape[0], m.shape
        self.device = TA._device if device is None else int(device)
        self.ratio = None
        self.previous = None
        self.kernel_ms = 0.0
        lib = self._lib = _engine.load_library()
        if self.nMat > int(lib.bfd_bhte_max_materials()):
            raise ValueError('MaterialList has %d rows: the bio-heat solver takes at most %d materials' % (self.nMat, lib.bfd_bhte_max_materials()))
        h = C.c_void_p()
        self._check(lib.bfd_thermal_create(self.device, m.shape[0], m.shape[1], m.shape[2], self.nFields, self.nMat, C.byref(h)), 'bfd_thermal_create')
        self._h = h
        try:
            p, pw = np.ascontiguousarray(p), np.ascontiguousarray(pw)
            self._check(lib.bfd_thermal_set_inputs(h, _engine._ptr(p), _engine._ptr(pw), _engine._ptr(m), m.dtype.itemsize), 'bfd_thermal_set_inputs')
        except Exception:
            self.close()
            raise

    # ---------------------------------------------------------------- lifetime ----------------------------------------------------------------
    def close(self):
        if self._h is not None:
            self._lib.bfd_thermal_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        self.close()

    def _check(self, rc, entry):
        if rc == 0:
            return
        msg = '%s failed (rc=%d): %s' % (entry, rc, self._lib.bfd_last_error().decode())
        if rc == -5 or (rc == -1 and TA.DATA_REFUSED in msg):
            raise ValueError(msg)
        raise _engine.EngineError(msg)

    def _handle(self):
        if self._h is None:
            raise _engine.EngineError('the thermal study is closed')
        return self._h

    def _timed(self, ms):
        global last_kernel_ms
        last_kernel_ms = ms
        self.kernel_ms += ms

    # ---------------------------------------------------------------- stages ----------------------------------------------------------------
    def median_in_region(self, classOf, bit=TA.BIT_SKULL, which=None):
        """:908-918: the 3 x 3 x 3 median merged under class `bit` of classOf, in place on the resident fields. which: 'p' or 'pw'; by default what
        the reference's statements filter: pAmp for one field (:911-913), AllInputsWater for several (:915-918)."""
        t = TA._table(classOf)
        if t.size != self.nMat:
            raise ValueError('classOf needs one row per material (%d)' % self.nMat)
        which = which or ('p' if self.single else 'pw')
        if which not in ('p', 'pw'):
            raise ValueError("which must be 'p' or 'pw'")
        ms = C.c_float()
        self._check(self._lib.bfd_thermal_median_region(self._handle(), _engine._ptr(t), int(bit), NAMES[which], C.byref(ms)), 'bfd_thermal_median_region')
        self._timed(ms.value)

    def loss_survey(self, classOf, rhoWater, cWater, dx2, brainMask=None):
        """ThermalAnalysis.loss_survey on the resident fields (rho, c from MaterialList); the resident water fields are cleared over class bit 1."""
        t = TA._table(classOf)
        if t.size != self.nMat:
            raise ValueError('classOf needs one row per material (%d)' % self.nMat)
        rho, c = np.ascontiguousarray(self.MaterialList['Density'], np.float64), np.ascontiguousarray(self.MaterialList['SoS'], np.float64)
        mask = None
        if brainMask is not None:
            mask = np.asarray(brainMask)
            if mask.shape != self.shape:
                raise ValueError('brainMask has shape %r, the map %r' % (mask.shape, self.shape))
            mask = np.ascontiguousarray((mask != 0).view(np.uint8))
        F, N3 = self.nFields, self.shape[2]
        res = dict(maxTissue=np.zeros(F, np.float32), argTissue=np.zeros(F, np.int64), maxWater=np.zeros(F, np.float32), argWater=np.zeros(F, np.int64),
                   eWaterRaw=np.zeros((F, N3)), eWater=np.zeros((F, N3)), eTissue=np.zeros((F, N3)))
        ms = C.c_float()
        P = _engine._ptr
        self._check(self._lib.bfd_thermal_loss_survey(self._handle(), P(t), P(mask), P(rho), P(c), float(rhoWater), float(cWater), float(dx2), P(res['maxTissue']),
                                                      P(res['argTissue']), P(res['maxWater']), P(res['argWater']), P(res['eWaterRaw']), P(res['eWater']),
                                                      P(res['eTissue']), C.byref(ms)), 'bfd_thermal_loss_survey')
        self._timed(ms.value)
        return res

    def analyze_losses(self, LocIJK, Input, Isppa, xf, yf, zf, SelBrain, bForceHomogenousMedium, bSegmentedBrain, TxSystem, IdRegionBenchmark=[],
                       FixedAcousticPower=0.0, verbose=False, details=None):
        """AnalyzeLosses (:94-256) on the resident fields: its positional arguments without the volumes and the tables. (PressureRatio, RatioLosses):
        scalars for one field, float32 arrays over the fields for several (:930-944). SelBrain: the bool volume, or the list of brain ids."""
        nMat = self.nMat
        sel = TA.selregion_table(nMat, 'MaterialMapCT' in Input, bool(bSegmentedBrain), bool(bForceHomogenousMedium), IdRegionBenchmark)
        classOf = (sel.astype(np.uint8) << TA.BIT_SELREGION)
        mask = None
        if np.ndim(SelBrain) == 3:
            mask = SelBrain
        else:
            classOf = classOf | (np.isin(np.arange(nMat), SelBrain).astype(np.uint8) << TA.BIT_BRAIN)
        ML = self.MaterialList
        survey = self.loss_survey(classOf, ML['Density'][0], ML['SoS'][0], (xf[1] - xf[0]) ** 2, brainMask=mask)
        out = []
        for f in range(self.nFields):
            r = TA.losses_from_survey(survey, f, self.shape, LocIJK, self.MaterialMap, ML, Isppa, xf, yf, zf, Input, TxSystem, bSegmentedBrain,
                                      IdRegionBenchmark, FixedAcousticPower, report=print if verbose else None)
            if details is not None:
                details.setdefault('fields', []).append(r)
            out.append((r['PressureRatio'], r['RatioLosses']))
        if self.single:
            return out[0]
        return np.array([o[0] for o in out], np.float32), np.array([o[1] for o in out], np.float32)

    def set_previous(self, PreviousData):
        """PreviousData's 'FinalTemp', 'FinalDose' and 'TempEndFUS' (:948-956) to the device, once. bhte, run_cycles and merge_previous then take this
        very dict in place of its volumes: they start from, and merge with, the copies held."""
        vols = [TA._volume(PreviousData[k], k, self.shape) for k in ('FinalTemp', 'FinalDose', 'TempEndFUS')]
        self._check(self._lib.bfd_thermal_set_previous(self._handle(), *[_engine._ptr(v) for v in vols]), 'bfd_thermal_set_previous')
        self.previous = PreviousData

    def scale(self, PressureRatio):
        """pAmp * PressureRatio (one field, :960) or InputsBHTE[n] *= PressureRatio[n] (:975-977) without a pass over the volume: the ratio is kept and
        applied wherever the scaled pressure is used."""
        if self.single:
            r = np.array([np.float64(PressureRatio)], np.float64)
        else:
            r = np.asarray(PressureRatio, np.float32).astype(np.float64).reshape(-1)         # the reference's ratios are float32 there
            if r.size != self.nFields:
                raise ValueError('one PressureRatio per field is needed (%d)' % self.nFields)
        if not np.all(np.isfinite(r)):
            raise ValueError('PressureRatio must be finite')
        self._check(self._lib.bfd_thermal_set_scale(self._handle(), _engine._ptr(r), 0 if self.single else 1), 'bfd_thermal_set_scale')
        self.ratio = r

    def _points(self, MonitoringPointsMap):
        if MonitoringPointsMap is None:
            return None
        if hasattr(MonitoringPointsMap, 'ids') and hasattr(MonitoringPointsMap, 'indices'):
            if tuple(MonitoringPointsMap.shape) != self.shape:
                raise ValueError('MonitoringPointsMap must have the shape of the pressure field')
            ids, lin = np.asarray(MonitoringPointsMap.ids), np.asarray(MonitoringPointsMap.indices, np.int64)
            if lin.size and (lin.min() < 0 or lin.max() >= np.prod(self.shape) or ids.min() == 0):
                raise ValueError('MonitoringPointsMap holds an index outside the volume or the id 0')
            return np.ascontiguousarray(lin[np.lexsort((lin, ids))], np.uint32)
        mp = np.asarray(MonitoringPointsMap)
        if mp.shape != self.shape:
            raise ValueError('MonitoringPointsMap must have the shape of the pressure field')
        mp = mp.ravel()
        lin = np.flatnonzero(mp)
        return np.ascontiguousarray(lin[np.argsort(mp[lin], kind='stable')], np.uint32)

    def _run(self, sched, caps, dt, DutyCycle, blood_rho, blood_ct, stableTemp, MonitoringPointsMap, initT0, initDose, flags):
        cd, cp, qf = R.bhte_coefficients(self.MaterialList, self.dx, dt, DutyCycle, blood_rho, blood_ct)
        initT = np.ascontiguousarray(self.MaterialList['InitTemperature'], np.float32)
        T0 = dose0 = None
        if initT0 is not None:
            T0 = np.ascontiguousarray(initT0, np.float32); flags |= FLAG_T0
            if T0.shape != self.shape:
                raise ValueError('initT0 must have the shape of the pressure field')
        if initDose is not None:
            dose0 = np.ascontiguousarray(initDose, np.float32); flags |= FLAG_DOSE0
            if dose0.shape != self.shape:
                raise ValueError('initDose must have the shape of the pressure field')
        idx = self._points(MonitoringPointsMap)
        sched = np.ascontiguousarray(sched, np.int32)
        nSteps = len(sched)
        pts = None if idx is None else np.zeros((len(idx), nSteps), np.float32)
        caps = None if caps is None else np.ascontiguousarray(caps, np.int32)
        ms = C.c_double()
        P = _engine._ptr
        self._check(self._lib.bfd_thermal_run(self._handle(), P(cd), P(cp), P(qf), P(initT), flags, P(T0), P(dose0), float(stableTemp), float(dt), nSteps,
                                              P(sched) if nSteps else None, 1, 0 if idx is None else len(idx), P(idx), P(pts), 0 if caps is None else len(caps),
                                              P(caps), C.byref(ms)), 'bfd_thermal_run')
        self._timed(ms.value)
        return pts

    def bhte(self, TotalDurationSteps, nStepsOn, nFactorMonitoring=1, dt=0.1, blood_rho=1050, blood_ct=3617, stableTemp=37.0, DutyCycle=1.0,
             MonitoringPointsMap=None, initT0=None, initDose=None, PreviousData=None):
        """BHTE (one field: nStepsOn an int, DutyCycle in the heat source) or BHTEMultiplePressureFields (several: nStepsOn the (nFields, 2) on / off
        list, duty cycle 1) on the resident, scaled pressure; a fresh start. ResTemp, ResDose and Qarr stay on the device ('T' / 'Tmax', 'dose', 'q');
        the point series comes back (None without a MonitoringPointsMap). PreviousData, the dict given to set_previous: start from its state as held."""
        nSteps = int(TotalDurationSteps)
        if self.single:
            sched = np.full(nSteps, -1, np.int32)
            sched[:max(min(int(nStepsOn), nSteps), 0)] = 0
        else:
            oo = np.asarray(nStepsOn).reshape(-1, 2)
            if oo.shape[0] != self.nFields:
                raise ValueError('nStepsOnOffList needs one (on, off) row per pressure field')
            sched = R.field_schedule(oo, nSteps)
        flags = FLAG_START_OVER
        if PreviousData is not None:
            if PreviousData is not self.previous or initT0 is not None or initDose is not None:
                raise ValueError('PreviousData must be the dict given to set_previous, without initT0 and initDose')
            flags |= FLAG_FROM_PREVIOUS
        return self._run(sched, None, dt, DutyCycle if self.single else 1.0, blood_rho, blood_ct, stableTemp, MonitoringPointsMap, initT0, initDose, flags)

    def run_cycles(self, nCurrent, Repetitions, TotalIterations, TotalDurationBetweenGroups, TotalDurationStepsOff, LimitBHTEIterationsPerProcess,
                   TotalDurationSteps, nStepsOn, nFactorMonitoring, dt, DutyCycle, MonitoringPointsMap, stableTemp, TemperaturePoints=None, PreviousData=None,
                   bRunInSubProcess=False):
        """RunBHTECycles without its volumes: (TemperaturePoints, nCurrent_next). At nCurrent == 0 the state starts over, from PreviousData['FinalTemp' /
        'FinalDose'] (uploaded once) where given; at nCurrent > 0 it continues from the resident temperature and dose, and 'Tmax' goes on as the
        maximum over every ON call since nCurrent == 0 (the np.maximum of :1094-1098). 'Tmax', 'doseAtCapture', 'T' and 'dose' are ResTempMax, ResDose,
        FinalTemp and FinalDose."""
        if MonitoringPointsMap is None:
            raise ValueError('run_cycles needs a MonitoringPointsMap')
        sched, caps, _, nNext = R.protocol_schedule(nCurrent, Repetitions, TotalIterations, TotalDurationBetweenGroups, TotalDurationStepsOff,
                                                    LimitBHTEIterationsPerProcess, TotalDurationSteps, nStepsOn, not self.single, bRunInSubProcess)
        initT0 = initDose = None
        if int(nCurrent) > 0:
            flags = FLAG_MERGE_CAPTURES
            if TemperaturePoints is None or np.ndim(TemperaturePoints) != 2:
                raise ValueError('TemperaturePoints must hold one row per monitoring point when resuming (nCurrent > 0)')
        else:
            flags = FLAG_START_OVER
            if PreviousData is not None and PreviousData is self.previous:
                flags |= FLAG_FROM_PREVIOUS                   # the copies held
            elif PreviousData is not None:
                initT0, initDose = PreviousData['FinalTemp'], PreviousData['FinalDose']
        pts = self._run(sched, caps, dt, DutyCycle if self.single else 1.0, 1050, 3617, stableTemp, MonitoringPointsMap, initT0, initDose, flags)
        if int(nCurrent) > 0:
            if np.shape(TemperaturePoints)[0] != pts.shape[0]:
                raise ValueError('TemperaturePoints must hold one row per monitoring point when resuming (nCurrent > 0)')
            pts = np.hstack((TemperaturePoints, pts))
        return pts, nNext

    def merge_previous(self, volume=None, name='Tmax'):
        """np.maximum(ResTemp, PreviousData['TempEndFUS']) of :994 and :1108 on the resident volume `name`; volume None: the TempEndFUS of set_previous"""
        v = None if volume is None else TA._volume(volume, 'volume', self.shape)
        self._check(self._lib.bfd_thermal_merge_max(self._handle(), NAMES[name], _engine._ptr(v)), 'bfd_thermal_merge_max')

    def tissue_extrema(self, names, classOf):
        """ThermalAnalysis.tissue_extrema over resident volumes named in `names` ('Tmax', 'doseAtCapture', 'T', 'dose', 'p_map'; 'p' with one field)"""
        t = TA._table(classOf)
        if t.size != self.nMat:
            raise ValueError('classOf needs one row per material (%d)' % self.nMat)
        which = np.array([NAMES[n] for n in names], np.int32)
        nV = len(which)
        if nV < 1:
            raise ValueError('at least one volume is needed')
        count = np.zeros(TA.CLASSES, np.int64)
        maxIn, maxKey = np.zeros((nV, TA.CLASSES), np.float32), np.zeros((nV, TA.CLASSES), np.float32)
        argIn, argKey = np.zeros((nV, TA.CLASSES), np.int64), np.zeros((nV, TA.CLASSES), np.int64)
        ms = C.c_float()
        P = _engine._ptr
        self._check(self._lib.bfd_thermal_extrema(self._handle(), P(which), nV, P(t), P(count), P(maxIn), P(argIn), P(maxKey), P(argKey), C.byref(ms)),
                    'bfd_thermal_extrema')
        self._timed(ms.value)
        return dict(count=count, maxIn=maxIn, argIn=argIn, maxKey=maxKey, argKey=argKey)

    def hottest_points(self, classOf, name='Tmax'):
        """(mSkin, mBrain, mSkull) of :996-1001 from the resident temperature"""
        e = self.tissue_extrema([name], classOf)
        return tuple(np.array(np.unravel_index(e['argKey'][0, b], self.shape)).astype(int) for b in (TA.BIT_SKIN, TA.BIT_BRAIN, TA.BIT_SKULL))

    def exposure_metrics(self, classOf, BrainID, Frequency, DutyCycle, Isppa):
        """ThermalAnalysis.exposure_metrics (:1126-1151) from the resident 'Tmax', 'dose' and pressure. One field: the maximum of the unscaled p over
        the brain times the ratio, formed with numpy's scalar types as exposure_metrics does for (pAmp, PressureRatio); several: the maximum of p_map."""
        if self.ratio is None:
            raise _engine.EngineError('exposure_metrics: scale comes first')
        if self.single and not self.ratio[0] > 0:
            raise ValueError('PressureRatio must be positive')
        e = self.tissue_extrema(['Tmax', 'dose', 'p' if self.single else 'p_map'], classOf)
        for b, name in ((TA.BIT_BRAIN, 'brain'), (TA.BIT_SKIN, 'skin'), (TA.BIT_SKULL, 'skull')):
            if e['count'][b] == 0:
                raise ValueError('zero-size array to reduction operation maximum which has no identity (the %s class is empty)' % name)
        mx = e['maxIn']
        r = dict(TI=mx[0, TA.BIT_BRAIN], TIS=mx[0, TA.BIT_SKIN], TIC=mx[0, TA.BIT_SKULL], CEMBrain=mx[1, TA.BIT_BRAIN] / 60, CEMSkin=mx[1, TA.BIT_SKIN] / 60,
                 CEMSkull=mx[1, TA.BIT_SKULL] / 60)
        MaxBrainPressure = mx[2, TA.BIT_BRAIN] * np.float64(self.ratio[0]) if self.single else mx[2, TA.BIT_BRAIN]
        ML = self.MaterialList
        r['MaxBrainPressure'] = MaxBrainPressure
        r['MaxBrainPressureIndex'] = int(e['argIn'][2, TA.BIT_BRAIN])
        r['MI'] = MaxBrainPressure / 1e6 / np.sqrt(Frequency / 1e6)
        MaxIsppa = MaxBrainPressure ** 2 / (2.0 * ML['SoS'][BrainID] * ML['Density'][BrainID])
        r['MaxIsppa'] = MaxIsppa / 1e4
        r['MaxIspta'] = DutyCycle * r['MaxIsppa']
        r['Ispta'] = DutyCycle * Isppa
        return r

    # ---------------------------------------------------------------- results ----------------------------------------------------------------
    def fetch(self, name, dtype=None):
        """One named result to the host: 'Tmax', 'doseAtCapture', 'T', 'dose', 'p_map' [N1][N2][N3]; 'q', 'pw', 'p' with the field axis first for
        several fields. float32; dtype=np.float64 gives p_map of one field as the reference saves it (:1115, pAmp * PressureRatio under NumPy >= 2)."""
        if name not in NAMES or name == 'MaterialMap':
            raise ValueError('no such volume: %r' % (name,))
        wide = dtype is not None and np.dtype(dtype) == np.float64
        if dtype is not None and not wide and np.dtype(dtype) != np.float32:
            raise TypeError('dtype must be float32 or float64')
        fields = name in ('q', 'pw', 'p')
        out = np.empty(((self.nFields,) if fields else ()) + self.shape, np.float64 if wide else np.float32)
        self._check(self._lib.bfd_thermal_get(self._handle(), NAMES[name], _engine._ptr(out), 1 if wide else 0), 'bfd_thermal_get')
        return out[0] if fields and self.single else out

    def fetch_plane(self, name, j):
        """[:, j, :] of 'p_map' (float32), of the unscaled 'p' (one field) or of 'MaterialMap' (the dtype of the map as passed): p_map_central and MaterialMap_central of :1116-1120"""
        if name not in ('p_map', 'MaterialMap', 'p'):
            raise ValueError("fetch_plane takes 'p_map', 'MaterialMap' or, with one field, 'p'")
        out = np.empty((self.shape[0], self.shape[2]), np.uint32 if name == 'MaterialMap' else np.float32)
        self._check(self._lib.bfd_thermal_get_plane(self._handle(), NAMES[name], int(j), _engine._ptr(out)), 'bfd_thermal_get_plane')
        return out.astype(np.asarray(self.MaterialMap).dtype) if name == 'MaterialMap' else out

    def traffic(self):
        """(bytes copied host -> device, bytes copied device -> host) since the study was created, counted where the copies are issued"""
        up, down = C.c_int64(), C.c_int64()
        self._check(self._lib.bfd_thermal_traffic(self._handle(), C.byref(up), C.byref(down)), 'bfd_thermal_traffic')
        return up.value, down.value


VOLUMES = {'p_map': 'p_map', 'TempEndFUS': 'Tmax', 'DoseEndFUS': 'doseAtCapture', 'FinalTemp': 'T', 'FinalDose': 'dose'}


def thermal_exposure(pAmp, pAmpWater, MaterialMap, MaterialList, Input, LocIJK, Isppa, DutyCycle, Frequency, dt, DurationUS, DurationOff, Repetitions=1,
                     NumberGroupedSonications=1, PauseBetweenGroupedSonications=0.0, nStepsOnOffList=None, BaselineTemperature=37.0, TxSystem='',
                     bSegmentedBrain=False, bForceHomogenousMedium=False, benchmark=None, bApplyMedianPressure=True, FixedAcousticPower=0.0,
                     PreviousData=None, LimitBHTEIterationsPerProcess=100, keep=(), device=None, return_study=False):
    """The volume flow of CalculateTemperatureEffects.py:847-1193 on one ThermalStudy, for the normal, CT ('MaterialMapCT' in Input), segmented,
    homogeneous and benchmark (dict(TestType=, nMaterials=)) selections, for one field (pAmp 3-D) and for several (4-D, with nStepsOnOffList).
    Returns the volume-derived entries of SaveDict. Its volumes ('p_map', 'TempEndFUS', 'DoseEndFUS', 'FinalTemp', 'FinalDose') stay on the device
    unless named in `keep`; with return_study the open study comes back under 'study' (fetch what is wanted, then close it). 'kernel_ms' and
    'traffic' report the study's kernels and copies."""
    for k in keep:
        if k not in VOLUMES:
            raise ValueError('keep names %r; the volumes are %s' % (k, sorted(VOLUMES)))
    nFactorMonitoring = int(50e-3 / dt) or 1
    TotalDurationSteps = int((DurationUS + .001) / dt)
    nStepsOn = int(DurationUS / dt)
    if nFactorMonitoring > TotalDurationSteps:
        nFactorMonitoring = 1
    TotalDurationStepsOff = int((DurationOff + .001) / dt)
    TotalDurationBetweenGroups = int(PauseBetweenGroupedSonications / dt)
    xf, yf, zf = Input['x_vec'], Input['y_vec'], Input['z_vec']
    LocIJK = np.asarray(LocIJK).flatten()
    cx, cy, cz = LocIJK[0], LocIJK[1], LocIJK[2]
    nMat = len(MaterialList['Density'])
    bench = None
    if benchmark is not None and not bForceHomogenousMedium:
        bench = dict(benchmark)
        if bench['TestType'] == 3:
            bench['maxMaterial'] = int(np.asarray(MaterialMap).max())
    tables = TA.region_tables(nMat, 'MaterialMapCT' in Input, bool(bSegmentedBrain), bool(bForceHomogenousMedium), bench)
    classOf, BrainID, IdRegionBenchmark = tables['classOf'], tables['BrainID'], tables['IdRegionBenchmark']
    bNormalOperation = not bForceHomogenousMedium and bench is None
    dx = Input['x_vec'][1] - Input['x_vec'][0]
    st = ThermalStudy(pAmp, pAmpWater, MaterialMap, MaterialList, dx, device)
    try:
        single = st.single
        if not single and nStepsOnOffList is None:
            raise ValueError('several fields need nStepsOnOffList')
        if bNormalOperation and bApplyMedianPressure:
            st.median_in_region(classOf, TA.BIT_SKULL)
        PressureRatio, RatioLosses = st.analyze_losses(LocIJK, Input, Isppa, xf, yf, zf, BrainID, bForceHomogenousMedium, bSegmentedBrain, TxSystem,
                                                       IdRegionBenchmark, FixedAcousticPower)
        if PreviousData is not None:
            st.set_previous(PreviousData)                     # three volumes, once
        st.scale(PressureRatio)
        st.bhte(TotalDurationSteps, nStepsOn if single else nStepsOnOffList, nFactorMonitoring=nFactorMonitoring, dt=dt, DutyCycle=DutyCycle,
                stableTemp=BaselineTemperature, PreviousData=PreviousData)
        if PreviousData is not None:
            st.merge_previous()
        mSkin, mBrain, mSkull = st.hottest_points(classOf)
        mp = TA.monitoring_points(mSkin, mBrain, mSkull, LocIJK, st.shape, bool(bForceHomogenousMedium), bench)
        TOTAL_Iterations = NumberGroupedSonications * Repetitions
        chunks = TOTAL_Iterations > LimitBHTEIterationsPerProcess
        nCurrent, TemperaturePoints = 0, None
        while True:
            TemperaturePoints, nCurrent = st.run_cycles(nCurrent, Repetitions, TOTAL_Iterations, TotalDurationBetweenGroups, TotalDurationStepsOff,
                                                        LimitBHTEIterationsPerProcess, TotalDurationSteps, nStepsOn if single else nStepsOnOffList, nFactorMonitoring,
                                                        dt, DutyCycle, mp, BaselineTemperature, TemperaturePoints, PreviousData, bRunInSubProcess=chunks)
            if not chunks or nCurrent >= TOTAL_Iterations:
                break
        if PreviousData is not None:
            st.merge_previous()
        S = dict(mSkin=mSkin, mBrain=mBrain, mSkull=mSkull, dt=dt, PressureRatio=PressureRatio, RatioLosses=RatioLosses)
        # :1116: for one field pAmp[:, cy, :] * PressureRatio, a float64 plane under NumPy >= 2, formed here from the plane of the unscaled p
        S['p_map_central'] = st.fetch_plane('p', cy) * PressureRatio if single else st.fetch_plane('p_map', cy)
        S['MaterialMap_central'] = st.fetch_plane('MaterialMap', cy)
        met = st.exposure_metrics(classOf, BrainID, Frequency, DutyCycle, Isppa)
        S['MaxBrainPressure'] = met['MaxBrainPressure']
        if bForceHomogenousMedium:
            IndTarget = 0
        elif bench is not None:
            IndTarget = 0 if bench['TestType'] == 1 else 1
        elif cx == mBrain[0] and cy == mBrain[1] and cz == mBrain[2]:
            IndTarget = 2
        else:
            IndTarget = 3
        if PreviousData is None:
            S['TimeProfileTarget'] = np.arange(TemperaturePoints.shape[1]) * dt
            S['TempProfileTarget'] = TemperaturePoints[IndTarget, :]
            S['TemperaturePoints'] = TemperaturePoints
        else:
            S['TimeProfileTarget'] = np.hstack((PreviousData['TimeProfileTarget'],
                                                PreviousData['TimeProfileTarget'][-1] + dt + np.arange(TemperaturePoints.shape[1]) * dt))
            S['TempProfileTarget'] = np.hstack((PreviousData['TempProfileTarget'], TemperaturePoints[IndTarget, :]))
            S['TemperaturePoints'] = np.hstack((PreviousData['TemperaturePoints'], TemperaturePoints))
        S['MI'] = met['MI']
        S['TI'], S['TIC'], S['TIS'] = met['TI'] - BaselineTemperature, met['TIC'] - BaselineTemperature, met['TIS'] - BaselineTemperature
        for k in ('CEMBrain', 'CEMSkin', 'CEMSkull', 'MaxIsppa', 'MaxIspta', 'Ispta'):
            S[k] = met[k]
        S['Isppa'] = Isppa
        for k in keep:
            S[k] = st.fetch(VOLUMES[k], np.float64 if (k == 'p_map' and single) else None)
        S['kernel_ms'] = st.kernel_ms
        S['traffic'] = st.traffic()
        if return_study:
            S['study'] = st
        else:
            st.close()
        return S
    except BaseException:
        st.close()
        raise
