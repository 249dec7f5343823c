"""The exposure analysis of Step 3 in the reference's ThermalModeling/CalculateTemperatureEffects.py, around its two heavy calls (the bio-heat
solver and the median filter), with the whole-volume work on the device:

    InitThermalAnalysis(DeviceName, GPUBackend)
    region_tables(nMat, ct, segmented, homogeneous, benchmark)     :864-906, :165-179: the selections as one class table over the material ids
    tissue_extrema(volumes, MaterialMap, classOf)                   :996-1001, :1126-1144: maxima and first indices by class, one pass
    loss_survey(pAmp, pAmpWater, MaterialMap, classOf, ...)         :142-216: the maxima and every plane energy of AnalyzeLosses, one pass per spot
    losses_from_survey(survey, field, ...)                          :199-254: the scalar lines, float64 on the host
    AnalyzeLosses(...)                                              :94-256: the reference's positional signature and return value
    hottest_points(ResTemp, MaterialMap, classOf)                   :996-1001
    monitoring_points(...), monitoring_points_map(...)              :1003-1023, sparse (RayleighAndBHTE takes it as it is) and dense
    exposure_metrics(...)                                           :1126-1151: TI, TIS, TIC, the three CEM, MaxBrainPressure, MI, MaxIsppa, MaxIspta

The work runs on the MI355X through the C ABI (bfd_class_extrema3d and bfd_loss_survey3d in csrc/bfd_thermal.hip; definitions in
include/babelfdtd.h); there is no CPU fallback. Maxima, indices, counts and the zeroed water field equal the literal numpy restatement
(tests/thermal_oracle.py); a plane energy is the sum of the same float64 terms in a fixed order of the device's, within Higham's bound of the exact
sum. The energy terms have the reference's types under NumPy >= 2 promotion: under numpy 1.x the reference's water energies are float32 sums, a
stated deviation. Argument errors are raised before the library is loaded."""
import ctypes as C

import numpy as np

from . import _engine, _step1

_device = 0
last_kernel_ms = None
CLASSES = 8
MAX_MATERIALS = 65536
BIT_BRAIN, BIT_SELREGION, BIT_SKIN, BIT_SKULL = 0, 1, 2, 3
# every data refusal of the two entries (rc -1 after the device pick) carries these words after the entry's name (csrc/bfd_thermal.hip,
# DATA_REFUSED; include/babelfdtd.h): they become ValueError with the library's text
DATA_REFUSED = 'refused data'
ROWS = 128                                         # rows of (i, j) one workgroup of the survey owns (csrc/bfd_thermal.hip)
SWEEP_VOXELS = 1024 * 256 * 4                      # voxels one sweep of the extrema launch covers before its grid-stride loop turns
LDS_MATERIALS, LDS_PROPERTIES = 2048, 1280         # rows of the class table, and of rho and c, the kernels keep in LDS; longer ones are read from global memory


def InitThermalAnalysis(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as InitMedianFilter does. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


def _call(entry, *args):
    """_step1.call with the data refusals of the entry as ValueError"""
    try:
        _step1.call(entry, *args)
    except _engine.EngineError as e:
        if '(rc=-1)' in str(e) and DATA_REFUSED in str(e):
            raise ValueError(str(e)) from None
        raise


def _volume(a, name, shape=None):
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise TypeError('%s must be float32, not %s' % (name, a.dtype))
    if a.ndim != 3:
        raise ValueError('%s must be a 3-D volume, not %d-D' % (name, a.ndim))
    if shape is not None and a.shape != shape:
        raise ValueError('%s has shape %r, the map %r' % (name, a.shape, shape))
    return np.ascontiguousarray(a)


def _map(MaterialMap):
    """the map as uint8, uint16 or uint32, C-contiguous: those dtypes go as they are (Step 3 reads uint32 from its file), any other integer
    dtype is narrowed to uint32 after its range is checked"""
    m = np.asarray(MaterialMap)
    if m.ndim != 3:
        raise ValueError('MaterialMap must be a 3-D volume, not %d-D' % m.ndim)
    if m.size >= 2 ** 31:
        raise ValueError('the volume has 2^31 voxels or more')
    if m.dtype not in (np.uint8, np.uint16, np.uint32):
        if m.dtype.kind not in 'iu':
            raise TypeError('MaterialMap must hold integers, not %s' % m.dtype)
        if m.size and (m.min() < 0 or m.max() >= 2 ** 32):
            raise ValueError('MaterialMap ids must lie in 0 .. 2^32 - 1')
        m = m.astype(np.uint32)
    return np.ascontiguousarray(m)


def _table(classOf):
    t = np.asarray(classOf)
    if t.ndim != 1 or not 1 <= t.size <= MAX_MATERIALS:
        raise ValueError('classOf must be a vector of 1 .. %d rows' % MAX_MATERIALS)
    if t.dtype != np.uint8:
        if t.dtype.kind not in 'iub' or (t.size and (t.min() < 0 or t.max() > 255)):
            raise ValueError('classOf must hold 8-bit masks')
        t = t.astype(np.uint8)
    return np.ascontiguousarray(t)


# ---------------------------------------------------------------- the selections ----------------------------------------------------------------

def region_tables(nMat, ct, segmented, homogeneous=False, benchmark=None):
    """The selections of :864-906 and selregion of :165-179 over the ids 0 .. nMat - 1, every branch. ct: 'MaterialMapCT' in Input; benchmark: None
    or dict(TestType=1 | 2 | 3, nMaterials=len(BenchmarkInput['Materials']), maxMaterial=MaterialMap.max() (TestType 3 alone)).
    Returns dict(classOf uint8 [nMat] with bit BIT_BRAIN, BIT_SELREGION, BIT_SKIN, BIT_SKULL; BrainID; IdRegionBenchmark)."""
    nMat = int(nMat)
    if not 1 <= nMat <= MAX_MATERIALS:
        raise ValueError('nMat must be 1 .. %d, not %d' % (MAX_MATERIALS, nMat))
    ids = np.arange(nMat)
    IdRegionBenchmark = []
    if homogeneous:
        skull = ids > 0
        BrainID = [1]
    elif benchmark is not None:
        BrainID = [int(benchmark['nMaterials']) - 1]
        if benchmark['TestType'] == 1:
            skull = ids > 0
            IdRegionBenchmark = [0]
        elif benchmark['TestType'] == 2:
            skull = ids == 1
            IdRegionBenchmark = [0, 1]
        elif benchmark['TestType'] == 3:
            maxMaterial = int(benchmark['maxMaterial'])
            skull = (ids > 1) & (ids <= maxMaterial - 2)
            IdRegionBenchmark = [maxMaterial - 2, maxMaterial - 2 - 1]
        else:
            raise ValueError('TestType must be 1, 2 or 3, not %r' % (benchmark['TestType'],))
    elif ct:
        if segmented:
            BrainID = [2, 3, 4, 5]
            skull = ids >= 6
        else:
            BrainID = [2]
            skull = ids > 2
    else:
        BrainID = [4, 5, 6, 7] if segmented else [4]
        skull = (ids > 1) & (ids < 4)
    brain = np.isin(ids, BrainID)
    skin = ids == 1
    sel = selregion_table(nMat, ct, segmented, homogeneous, IdRegionBenchmark)
    classOf = (brain.astype(np.uint8) << BIT_BRAIN) | (sel.astype(np.uint8) << BIT_SELREGION) | (skin.astype(np.uint8) << BIT_SKIN) | \
        (skull.astype(np.uint8) << BIT_SKULL)
    return dict(classOf=classOf.astype(np.uint8), BrainID=BrainID, IdRegionBenchmark=IdRegionBenchmark)


def selregion_table(nMat, ct, segmented, homogeneous, IdRegionBenchmark):
    """selregion of :165-179 as bool [nMat]: the ids whose water pressure AnalyzeLosses clears"""
    ids = np.arange(int(nMat))
    if homogeneous:
        return ids == 0
    if len(IdRegionBenchmark) > 0:
        return np.isin(ids, IdRegionBenchmark)
    if segmented:
        return ~np.isin(ids, [2, 3, 4, 5]) if ct else np.isin(ids, [0, 1, 2, 3])
    return ids != 2 if ct else ids != 4


# ---------------------------------------------------------------- the two entries ----------------------------------------------------------------

def tissue_extrema(volumes, MaterialMap, classOf):
    """volumes: a list of float32 volumes of the map's shape. dict(count [8], maxIn, argIn, maxKey, argKey, each [nVol][8]): for class c (bit c of
    classOf[id]) the voxels, the maximum of each volume over the class with the lowest C-order linear index that attains it (X[Sel].max() and
    np.flatnonzero(Sel)[X[Sel].argmax()]; 0 and -1 for an empty class), and np.argmax(X * Sel.astype(np.float32)) with the product there.
    ValueError for an id beyond the table and for a value that is not finite."""
    global last_kernel_ms
    m = _map(MaterialMap)
    t = _table(classOf)
    vols = [_volume(v, 'volume %d' % q, m.shape) for q, v in enumerate(volumes)]
    if not vols:
        raise ValueError('at least one volume is needed')
    nV = len(vols)
    ptrs = (C.c_void_p * nV)(*[v.ctypes.data for v in vols])
    count = np.zeros(CLASSES, np.int64)
    maxIn, maxKey = np.zeros((nV, CLASSES), np.float32), np.zeros((nV, CLASSES), np.float32)
    argIn, argKey = np.zeros((nV, CLASSES), np.int64), np.zeros((nV, CLASSES), np.int64)
    ms = C.c_float()
    P = _engine._ptr
    _call('bfd_class_extrema3d', _device, C.cast(ptrs, C.c_void_p), nV, P(m), m.dtype.itemsize, m.shape[0], m.shape[1], m.shape[2], P(t), t.size, P(count),
          P(maxIn), P(argIn), P(maxKey), P(argKey), C.byref(ms))
    last_kernel_ms = ms.value
    return dict(count=count, maxIn=maxIn, argIn=argIn, maxKey=maxKey, argKey=argKey)


def loss_survey(pAmp, pAmpWater, MaterialMap, classOf, rho, c, rhoWater, cWater, dx2, brainMask=None, waterOut=None):
    """The volume work of AnalyzeLosses for one focal spot ([N1][N2][N3]) or several ([nFields][N1][N2][N3]), float32. Bit 0 of classOf is the brain
    (brainMask, a volume read as != 0, replaces it), bit 1 selregion. rho, c: Density and SoS by id; dx2 = (xf[1] - xf[0]) ** 2.
    waterOut: None, a float32 array of pAmpWater's shape, or pAmpWater itself (the reference's in-place store): it receives the cleared water field.
    dict, every entry with the field axis first: maxTissue, argTissue, maxWater, argWater [nFields]; eWaterRaw, eWater, eTissue [nFields][N3]."""
    global last_kernel_ms
    m = _map(MaterialMap)
    t = _table(classOf)
    p, pw = np.asarray(pAmp), np.asarray(pAmpWater)
    if p.dtype != np.float32 or pw.dtype != np.float32:
        raise TypeError('the pressure fields must be float32, not %s and %s' % (p.dtype, pw.dtype))
    if p.ndim == 3:
        p, pw = p[None], (pw[None] if pw.ndim == 3 else pw)
    if p.ndim != 4 or p.shape != pw.shape or p.shape[1:] != m.shape or p.shape[0] < 1:
        raise ValueError('the pressure fields have shapes %r and %r, the map %r' % (np.shape(pAmp), np.shape(pAmpWater), m.shape))
    in_place = waterOut is pAmpWater
    if in_place and not (pw.flags.c_contiguous and pw.flags.writeable):
        raise ValueError('pAmpWater must be C-contiguous and writeable to be cleared in place')
    p, pw = np.ascontiguousarray(p), np.ascontiguousarray(pw)
    out = None
    if in_place:
        out = pw
    elif waterOut is not None:
        out = np.asarray(waterOut)
        if out.dtype != np.float32 or out.size != pw.size or not (out.flags.c_contiguous and out.flags.writeable):
            raise ValueError('waterOut must be a C-contiguous writeable float32 array of the water field\'s size')
    rho, c = np.ascontiguousarray(rho, np.float64), np.ascontiguousarray(c, np.float64)
    if rho.shape != (t.size,) or c.shape != (t.size,):
        raise ValueError('rho and c need one value per row of classOf (%d)' % t.size)
    for name, v in (('rho', rho), ('c', c), ('rhoWater', np.float64(rhoWater)), ('cWater', np.float64(cWater))):
        if not np.all(np.isfinite(v) & (v > 0)):
            raise ValueError('%s must be finite and positive' % name)
    dx2 = float(dx2)
    if not (np.isfinite(dx2) and dx2 >= 0):
        raise ValueError('dx2 must be finite and not negative')
    mask = None
    if brainMask is not None:
        mask = np.asarray(brainMask)
        if mask.shape != m.shape:
            raise ValueError('brainMask has shape %r, the map %r' % (mask.shape, m.shape))
        mask = np.ascontiguousarray(_step1.bool_as_uint8(mask) if mask.dtype == np.bool_ else (mask != 0).view(np.uint8))
    F, N3 = p.shape[0], m.shape[2]
    res = dict(maxTissue=np.zeros(F, np.float32), argTissue=np.zeros(F, np.int64), maxWater=np.zeros(F, np.float32), argWater=np.zeros(F, np.int64),
               eWaterRaw=np.zeros((F, N3)), eWater=np.zeros((F, N3)), eTissue=np.zeros((F, N3)))
    ms = C.c_float()
    P = _engine._ptr
    _call('bfd_loss_survey3d', _device, P(p), P(pw), F, P(m), m.dtype.itemsize, m.shape[0], m.shape[1], m.shape[2], P(t), t.size, P(mask), P(rho), P(c),
          float(rhoWater), float(cWater), dx2, P(res['maxTissue']), P(res['argTissue']), P(res['maxWater']), P(res['argWater']), P(res['eWaterRaw']),
          P(res['eWater']), P(res['eTissue']), P(out), C.byref(ms))
    last_kernel_ms = ms.value
    return res


# ---------------------------------------------------------------- AnalyzeLosses ----------------------------------------------------------------

def losses_from_survey(survey, field, shape, LocIJK, MaterialMap, MaterialList, Isppa, xf, yf, zf, Input, TxSystem, bSegmentedBrain,
                       IdRegionBenchmark=(), FixedAcousticPower=0.0, report=None):
    """The scalar lines of AnalyzeLosses (:149-254) from loss_survey's result for one field, with the reference's scalar types (float32 maxima,
    float64 energies). A dict of every intermediate the reference prints (its own names) with PressureRatio and RatioLosses; `report(label,
    *values)` receives what the reference prints, in its order."""
    report = report or (lambda *a: None)
    r = {}
    cz = LocIJK[2]
    eRaw, eWater, eTissue = survey['eWaterRaw'][field], survey['eWater'][field], survey['eTissue'][field]
    maxWater, maxTissue = survey['maxWater'][field], survey['maxTissue'][field]
    r['AcousticEnergy'] = eTissue[cz]
    report('Acoustic Energy at maximum plane', r['AcousticEnergy'])
    xfr, yfr = Input['x_vec'], Input['y_vec']
    r['AcousticEnergyWater'] = eRaw[2]
    report('Water Acoustic Energy entering', r['AcousticEnergyWater'])
    cxw, cyw, czw = (int(v) for v in np.unravel_index(survey['argWater'][field], shape))
    report('Location Max Pessure Water', cxw, cyw, czw, xf[cxw], yf[cyw], zf[czw] - zf[0], maxWater / 1e6)
    cxr, cyr, czr = (int(v) for v in np.unravel_index(survey['argTissue'][field], shape))
    report('Location Max Pressure Tissue', cxr, cyr, czr, xfr[cxr], yfr[cyr], Input['z_vec'][czr] - Input['z_vec'].min(), maxTissue / 1e6)
    r.update(LocWater=(cxw, cyw, czw), LocTissue=(cxr, cyr, czr))
    if TxSystem in ['DomeTx']:
        RatioLosses = (maxTissue / maxWater) ** 2
        report('Total losses ratio using single punctual measurement for dome Tx', RatioLosses, np.log10(RatioLosses) * 10)
    else:
        r['AcousticEnergyWaterMaxLocWat'] = eWater[czw]
        report('Water Acoustic Energy at maximum plane water max loc', r['AcousticEnergyWaterMaxLocWat'])
        r['AcousticEnergyTissueMaxLocWat'] = eTissue[czw]
        report('Tissue Acoustic Energy at maximum plane water max loc', r['AcousticEnergyTissueMaxLocWat'])
        r['AcousticEnergyWaterMaxLoc'] = eWater[czr]
        report('Water Acoustic Energy at maximum plane tissue max loc', r['AcousticEnergyWaterMaxLoc'])
        r['AcousticEnergyTissue'] = eTissue[czr]
        report('Tissue Acoustic Energy at maximum plane tissue', r['AcousticEnergyTissue'])
        r['RatioLossesLoc'] = r['AcousticEnergyTissueMaxLocWat'] / r['AcousticEnergyWaterMaxLocWat']
        report('Total losses ratio using Water loc and in dB', r['RatioLossesLoc'], np.log10(r['RatioLossesLoc']) * 10)
        RatioLosses = r['AcousticEnergyTissue'] / r['AcousticEnergyWaterMaxLoc']
        report('Total losses ratio and in dB', RatioLosses, np.log10(RatioLosses) * 10)
        r['RatioLossesPeak'] = (maxTissue / maxWater) ** 2
        report('Total losses ratio using single punctual measurement', r['RatioLossesPeak'], np.log10(r['RatioLossesPeak']) * 10)
        r['UsedWaterLoc'] = bool(RatioLosses > (r['RatioLossesLoc'] + 0.2))
        if r['UsedWaterLoc']:
            report('Warning: RatioLossesLoc is bigger than RatioLosses by more than 20%\nUsing water loc for ratio losses')
            RatioLosses = r['RatioLossesLoc']
        if FixedAcousticPower > 0.0:
            report('OVERWRITTING LOSSES with Fixed Acoustic Power', FixedAcousticPower)
            RatioLosses = FixedAcousticPower / r['AcousticEnergyWaterMaxLoc']
            report('RatioLosses with Fixed Acoustic Power', RatioLosses)
    target = (cxr, cyr, czr) if (bSegmentedBrain or len(IdRegionBenchmark) > 0) else (LocIJK[0], LocIJK[1], LocIJK[2])
    target_id = MaterialMap[target[0], target[1], target[2]]
    r['SoSTarget'], r['DensityTarget'] = MaterialList['SoS'][target_id], MaterialList['Density'][target_id]
    if FixedAcousticPower > 0.0:
        PressureRatio = np.sqrt(RatioLosses)
        report('PressureRatio with FixedAcousticPower ', PressureRatio)
    else:
        r['PressureAdjust'] = np.sqrt(Isppa * 1e4 * 2.0 * r['SoSTarget'] * r['DensityTarget'])
        PressureRatio = r['PressureAdjust'] / maxTissue
        report('PressureRatio', PressureRatio)
    r.update(PressureRatio=PressureRatio, RatioLosses=RatioLosses)
    return r


def AnalyzeLosses(pAmp, MaterialMap, LocIJK, Input, MaterialList, pAmpWater, Isppa, xf, yf, zf, SelBrain, bForceHomogenousMedium, bSegmentedBrain,
                  TxSystem, IdRegionBenchmark=[], FixedAcousticPower=0.0, verbose=False, details=None):
    """Drop-in for the reference's AnalyzeLosses (:94-256): the same positional signature, (PressureRatio, RatioLosses) back, and pAmpWater cleared
    in place over selregion as the reference leaves it. SelBrain: the bool volume the reference passes, or the list of brain ids. Prints what the
    reference prints with verbose alone; `details`, a dict, receives losses_from_survey's intermediates."""
    nMat = len(MaterialList['SoS'])
    sel = selregion_table(nMat, 'MaterialMapCT' in Input, bool(bSegmentedBrain), bool(bForceHomogenousMedium), IdRegionBenchmark)
    classOf = (sel.astype(np.uint8) << BIT_SELREGION)
    mask = None
    if np.ndim(SelBrain) == 3:
        mask = SelBrain
    else:
        classOf = classOf | (np.isin(np.arange(nMat), SelBrain).astype(np.uint8) << BIT_BRAIN)
    water = np.asarray(pAmpWater)
    direct = water.dtype == np.float32 and water.flags.c_contiguous and water.flags.writeable
    work = pAmpWater if direct else np.ascontiguousarray(water, np.float32).copy()
    survey = loss_survey(np.ascontiguousarray(pAmp, np.float32), work, MaterialMap, classOf, MaterialList['Density'], MaterialList['SoS'],
                         MaterialList['Density'][0], MaterialList['SoS'][0], (xf[1] - xf[0]) ** 2, brainMask=mask, waterOut=work)
    if not direct:
        pAmpWater[...] = work
    r = losses_from_survey(survey, 0, np.shape(MaterialMap), LocIJK, MaterialMap, MaterialList, Isppa, xf, yf, zf, Input, TxSystem, bSegmentedBrain,
                           IdRegionBenchmark, FixedAcousticPower, report=print if verbose else None)
    if details is not None:
        details.update(r)
    return r['PressureRatio'], r['RatioLosses']


# ---------------------------------------------------------------- monitoring points and metrics ----------------------------------------------------------------

class MonitoringPoints:
    """The reference's MonitoringPointsMap (:1003-1023) without the volume: `ids` uint32 and `indices` int64 (C-order linear), one per point, over a
    volume of `shape`. RayleighAndBHTE.BHTE, BHTEMultiplePressureFields and RunBHTECycles take it wherever they take the dense map."""

    def __init__(self, ids, indices, shape):
        self.ids = np.asarray(ids, np.uint32)
        self.indices = np.asarray(indices, np.int64)
        self.shape = tuple(int(n) for n in shape)

    def dense(self):
        out = np.zeros(self.shape, np.uint32)
        out.reshape(-1)[self.indices] = self.ids
        return out


def hottest_points(ResTemp, MaterialMap, classOf):
    """(mSkin, mBrain, mSkull) of :996-1001, each an (i, j, k) array: np.argmax(ResTemp * Sel.astype(np.float32)) for the classes BIT_SKIN,
    BIT_BRAIN and BIT_SKULL of classOf (region_tables)."""
    e = tissue_extrema([ResTemp], MaterialMap, classOf)
    shape = np.shape(MaterialMap)
    return tuple(np.array(np.unravel_index(e['argKey'][0, b], shape)).astype(int) for b in (BIT_SKIN, BIT_BRAIN, BIT_SKULL))


def monitoring_points(mSkin, mBrain, mSkull, LocIJK, shape, homogeneous=False, benchmark=None):
    """:1003-1023 as MonitoringPoints: the stores in the reference's order, a later store replacing an earlier one at the same voxel. Points are
    listed by ascending linear index, as np.flatnonzero of the dense map gives them."""
    stores = []
    if homogeneous:
        stores = [(mBrain, 1)]
    elif benchmark is not None:
        if benchmark['TestType'] == 1:
            stores = [(mBrain, 1)]
        elif benchmark['TestType'] in (2, 3):
            stores = [(mBrain, 1), (mSkull, 2)]
        else:
            raise ValueError('TestType must be 1, 2 or 3, not %r' % (benchmark['TestType'],))
    else:
        stores = [(mSkin, 1), (mBrain, 2), (mSkull, 3)]
        if not (LocIJK[0] == mBrain[0] and LocIJK[1] == mBrain[1] and LocIJK[2] == mBrain[2]):
            stores.append((LocIJK, 4))
    held = {}
    for ijk, pid in stores:
        held[int(np.ravel_multi_index((int(ijk[0]), int(ijk[1]), int(ijk[2])), shape))] = pid
    lin = sorted(held)
    return MonitoringPoints([held[q] for q in lin], lin, shape)


def monitoring_points_map(*args, **kw):
    """the dense uint32 MonitoringPointsMap of :1003-1023 (monitoring_points(...).dense())"""
    return monitoring_points(*args, **kw).dense()


def exposure_metrics(ResTemp, FinalDose, p_map, MaterialMap, classOf, MaterialList, BrainID, Frequency, DutyCycle, Isppa):
    """:1126-1151 as a dict: TI, TIS, TIC, CEMBrain, CEMSkin, CEMSkull, MaxBrainPressure, MI, MaxIsppa, MaxIspta, Ispta, from one pass over the
    three volumes. classOf: region_tables' table. p_map: the float32 volume the reference saves, or (pAmp, PressureRatio) for its
    pAmp * PressureRatio (:1115) without the product over the volume: with PressureRatio > 0 the product is strictly increasing in pAmp (float32
    neighbours differ by 2^-24 relative, a float64 product errs by 2^-53), so the first maximum of pAmp over the brain is the product's, and the value
    there is formed with numpy's own scalar types. An empty class raises ValueError, as numpy's max of nothing does."""
    scale = None
    if isinstance(p_map, tuple):
        p_map, scale = p_map
        if not scale > 0:
            raise ValueError('PressureRatio must be positive')
    e = tissue_extrema([ResTemp, FinalDose, p_map], MaterialMap, classOf)
    for b, name in ((BIT_BRAIN, 'brain'), (BIT_SKIN, 'skin'), (BIT_SKULL, 'skull')):
        if e['count'][b] == 0:
            raise ValueError('zero-size array to reduction operation maximum which has no identity (the %s class is empty)' % name)
    mx = e['maxIn']
    r = dict(TI=mx[0, BIT_BRAIN], TIS=mx[0, BIT_SKIN], TIC=mx[0, BIT_SKULL], CEMBrain=mx[1, BIT_BRAIN] / 60, CEMSkin=mx[1, BIT_SKIN] / 60,
             CEMSkull=mx[1, BIT_SKULL] / 60)
    MaxBrainPressure = mx[2, BIT_BRAIN] if scale is None else mx[2, BIT_BRAIN] * scale
    r['MaxBrainPressure'] = MaxBrainPressure
    r['MaxBrainPressureIndex'] = int(e['argIn'][2, BIT_BRAIN])
    r['MI'] = MaxBrainPressure / 1e6 / np.sqrt(Frequency / 1e6)
    MaxIsppa = MaxBrainPressure ** 2 / (2.0 * MaterialList['SoS'][BrainID] * MaterialList['Density'][BrainID])
    r['MaxIsppa'] = MaxIsppa / 1e4
    r['MaxIspta'] = DutyCycle * r['MaxIsppa']
    r['Ispta'] = DutyCycle * Isppa
    return r
