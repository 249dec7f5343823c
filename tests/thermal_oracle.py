"""The Step-3 exposure analysis of the reference's ThermalModeling/CalculateTemperatureEffects.py restated literally in numpy: the selections of
:864-906, AnalyzeLosses (:94-256), the monitoring points (:996-1023) and the exposure metrics (:1126-1151), and the definitions of the two device
entries (bfd_class_extrema3d, bfd_loss_survey3d in include/babelfdtd.h) in the same terms. Statement for statement the reference's, except:

  * the energy terms carry explicit casts: float32 for the square and the halving, float64 from the first division on. Those are the reference's
    own types under NumPy >= 2 promotion; with the casts written out every numpy gives them (under numpy 1.x the reference's water energies are
    float32 sums, because a float64 scalar did not widen a float32 array);
  * print goes to `report(label, *values)`, so a test can compare every intermediate the reference prints.

Inputs come from the seeded builder `build_case`, so fixtures hold parameters, seeds and results only."""
import numpy as np

BIT_BRAIN, BIT_SELREGION, BIT_SKIN, BIT_SKULL = 0, 1, 2, 3


# ---------------------------------------------------------------- :864-906 ----------------------------------------------------------------

def selections(MaterialMap, ct, segmented, homogeneous=False, benchmark=None):
    """(SelBrain, SelSkin, SelSkull, BrainID, IdRegionBenchmark) of :864-906. ct: 'MaterialMapCT' in Input. benchmark: None or
    dict(TestType=1 | 2 | 3, nMaterials=len(BenchmarkInput['Materials']))."""
    IdRegionBenchmark = []
    if homogeneous:
        SelSkull = MaterialMap > 0
        BrainID = [1]
    elif benchmark is not None:
        BrainID = [benchmark['nMaterials'] - 1]
        if benchmark['TestType'] == 1:
            SelSkull = MaterialMap > 0
            IdRegionBenchmark = [0]
        elif benchmark['TestType'] == 2:
            SelSkull = MaterialMap == 1
            IdRegionBenchmark = [0, 1]
        else:
            assert benchmark['TestType'] == 3
            maxMaterial = MaterialMap.max()
            SelSkull = (MaterialMap > 1) & (MaterialMap <= maxMaterial - 2)
            IdRegionBenchmark = [maxMaterial - 2, maxMaterial - 2 - 1]
    elif ct:
        if segmented:
            BrainID = [2, 3, 4, 5]
            SelSkull = MaterialMap >= 6
        else:
            BrainID = [2]
            SelSkull = MaterialMap > 2
    else:
        if segmented:
            BrainID = [4, 5, 6, 7]
        else:
            BrainID = [4]
        SelSkull = (MaterialMap > 1) & (MaterialMap < 4)
    SelBrain = np.isin(MaterialMap, BrainID)
    SelSkin = MaterialMap == 1
    return SelBrain, SelSkin, SelSkull, BrainID, [int(v) for v in IdRegionBenchmark]


def selregion(MaterialMap, ct, segmented, homogeneous, IdRegionBenchmark):
    """:165-179"""
    if homogeneous:
        return MaterialMap == 0
    if len(IdRegionBenchmark) > 0:
        return np.isin(MaterialMap, IdRegionBenchmark)
    if segmented:
        if ct:
            return np.isin(MaterialMap, [2, 3, 4, 5]) == False  # noqa: E712
        return np.isin(MaterialMap, [0, 1, 2, 3])
    if ct:
        return MaterialMap != 2
    return MaterialMap != 4


# ---------------------------------------------------------------- energy terms ----------------------------------------------------------------

def plane_terms(plane, R, C, dx2):
    """The terms of one plane energy, float64 [N1][N2]: plane**2/2/R/C*dx2 with the reference's types under NumPy >= 2 spelled out. plane float32;
    R, C float64 scalars or [N1][N2] arrays; dx2 a float64."""
    assert plane.dtype == np.float32
    half = (plane * plane) / np.float32(2)
    assert half.dtype == np.float32
    return ((half.astype(np.float64) / np.asarray(R, np.float64)) / np.asarray(C, np.float64)) * np.float64(dx2)


def plane_energy(plane, R, C, dx2):
    """the reference's (...).sum() of a plane: numpy's pairwise sum of the C-contiguous [N1][N2] result"""
    return np.ascontiguousarray(plane_terms(plane, R, C, dx2)).sum()


# ---------------------------------------------------------------- AnalyzeLosses ----------------------------------------------------------------

def AnalyzeLosses(pAmp, MaterialMap, LocIJK, Input, MaterialList, pAmpWater, Isppa, xf, yf, zf, SelBrain, bForceHomogenousMedium, bSegmentedBrain,
                  TxSystem, IdRegionBenchmark=[], FixedAcousticPower=0.0, report=None):
    """:94-256, statement for statement. pAmpWater is zeroed in place. Returns (PressureRatio, RatioLosses)."""
    report = report or (lambda *a: None)
    dx2 = (xf[1] - xf[0]) ** 2
    pAmpBrain = pAmp.copy()
    SoSMap = MaterialList['SoS'][MaterialMap]
    DensityMap = MaterialList['Density'][MaterialMap]
    pAmpBrain[SelBrain == False] = 0.0  # noqa: E712
    cz = LocIJK[2]
    AcousticEnergy = plane_energy(pAmpBrain[:, :, cz], DensityMap[:, :, cz], SoSMap[:, :, cz], dx2)
    report('Acoustic Energy at maximum plane', AcousticEnergy)
    xfr = Input['x_vec']
    yfr = Input['y_vec']
    zfr = Input['z_vec'].copy()
    zfr -= zfr.min()
    AcousticEnergyWater = plane_energy(pAmpWater[:, :, 2], MaterialList['Density'][0], MaterialList['SoS'][0], dx2)
    report('Water Acoustic Energy entering', AcousticEnergyWater)
    sel = selregion(MaterialMap, 'MaterialMapCT' in Input, bSegmentedBrain, bForceHomogenousMedium, IdRegionBenchmark)
    pAmpWater[sel] = 0.0
    cxw, cyw, czw = np.where(pAmpWater == pAmpWater.max())
    cxw, cyw, czw = cxw[0], cyw[0], czw[0]
    report('Location Max Pessure Water', cxw, cyw, czw, xf[cxw], yf[cyw], zf[czw] - zf[0], pAmpWater.max() / 1e6)
    pAmpTissue = pAmp.copy()
    pAmpTissue[SelBrain == False] = 0.0  # noqa: E712
    cxr, cyr, czr = np.where(pAmpTissue == pAmpTissue.max())
    cxr, cyr, czr = cxr[0], cyr[0], czr[0]
    report('Location Max Pressure Tissue', cxr, cyr, czr, xfr[cxr], yfr[cyr], zfr[czr], pAmpTissue.max() / 1e6)
    if TxSystem in ['DomeTx']:
        RatioLosses = (pAmpTissue.max() / pAmpWater.max()) ** 2
        report('Total losses ratio using single punctual measurement for dome Tx', RatioLosses, np.log10(RatioLosses) * 10)
    else:
        rhoW, cW = MaterialList['Density'][0], MaterialList['SoS'][0]
        AcousticEnergyWaterMaxLocWat = plane_energy(pAmpWater[:, :, czw], rhoW, cW, dx2)
        report('Water Acoustic Energy at maximum plane water max loc', AcousticEnergyWaterMaxLocWat)
        AcousticEnergyTissueMaxLocWat = plane_energy(pAmpTissue[:, :, czw], DensityMap[:, :, czw], SoSMap[:, :, czw], dx2)
        report('Tissue Acoustic Energy at maximum plane water max loc', AcousticEnergyTissueMaxLocWat)
        AcousticEnergyWaterMaxLoc = plane_energy(pAmpWater[:, :, czr], rhoW, cW, dx2)
        report('Water Acoustic Energy at maximum plane tissue max loc', AcousticEnergyWaterMaxLoc)
        AcousticEnergyTissue = plane_energy(pAmpTissue[:, :, czr], DensityMap[:, :, czr], SoSMap[:, :, czr], dx2)
        report('Tissue Acoustic Energy at maximum plane tissue', AcousticEnergyTissue)
        RatioLossesLoc = AcousticEnergyTissueMaxLocWat / AcousticEnergyWaterMaxLocWat
        report('Total losses ratio using Water loc and in dB', RatioLossesLoc, np.log10(RatioLossesLoc) * 10)
        RatioLosses = AcousticEnergyTissue / AcousticEnergyWaterMaxLoc
        report('Total losses ratio and in dB', RatioLosses, np.log10(RatioLosses) * 10)
        RatioLossesPeak = (pAmpTissue.max() / pAmpWater.max()) ** 2
        report('Total losses ratio using single punctual measurement', RatioLossesPeak, np.log10(RatioLossesPeak) * 10)
        if RatioLosses > (RatioLossesLoc + 0.2):
            report('Warning: RatioLossesLoc is bigger than RatioLosses by more than 20%\nUsing water loc for ratio losses')
            RatioLosses = RatioLossesLoc
        if FixedAcousticPower > 0.0:
            report('OVERWRITTING LOSSES with Fixed Acoustic Power', FixedAcousticPower)
            RatioLosses = FixedAcousticPower / AcousticEnergyWaterMaxLoc
            report('RatioLosses with Fixed Acoustic Power', RatioLosses)
    if bSegmentedBrain or len(IdRegionBenchmark) > 0:
        SoSTarget = SoSMap[cxr, cyr, czr]
        DensityTarget = DensityMap[cxr, cyr, czr]
    else:
        SoSTarget = SoSMap[LocIJK[0], LocIJK[1], LocIJK[2]]
        DensityTarget = DensityMap[LocIJK[0], LocIJK[1], LocIJK[2]]
    if FixedAcousticPower > 0.0:
        PressureRatio = np.sqrt(RatioLosses)
        report('PressureRatio with FixedAcousticPower ', PressureRatio)
    else:
        PressureAdjust = np.sqrt(Isppa * 1e4 * 2.0 * SoSTarget * DensityTarget)
        PressureRatio = PressureAdjust / pAmpTissue.max()
        report('PressureRatio', PressureRatio)
    return PressureRatio, RatioLosses


# ---------------------------------------------------------------- :996-1023, :1126-1151 ----------------------------------------------------------------

def monitoring_points_map(ResTemp, SelSkin, SelBrain, SelSkull, LocIJK, homogeneous=False, benchmark=None):
    """(MonitoringPointsMap uint32, mSkin, mBrain, mSkull) of :996-1023"""
    cx, cy, cz = LocIJK[0], LocIJK[1], LocIJK[2]
    ResTempSkin = ResTemp * SelSkin.astype(np.float32)
    ResTempBrain = ResTemp * SelBrain.astype(np.float32)
    ResTempSkull = ResTemp * SelSkull.astype(np.float32)
    mxSkin, mySkin, mzSkin = np.unravel_index(np.argmax(ResTempSkin, axis=None), ResTempSkin.shape)
    mxBrain, myBrain, mzBrain = np.unravel_index(np.argmax(ResTempBrain, axis=None), ResTempBrain.shape)
    mxSkull, mySkull, mzSkull = np.unravel_index(np.argmax(ResTempSkull, axis=None), ResTempSkull.shape)
    MonitoringPointsMap = np.zeros(ResTemp.shape, np.uint32)
    if homogeneous:
        MonitoringPointsMap[mxBrain, myBrain, mzBrain] = 1
    elif benchmark is not None:
        if benchmark['TestType'] == 1:
            MonitoringPointsMap[mxBrain, myBrain, mzBrain] = 1
        else:
            assert benchmark['TestType'] in (2, 3)
            MonitoringPointsMap[mxBrain, myBrain, mzBrain] = 1
            MonitoringPointsMap[mxSkull, mySkull, mzSkull] = 2
    else:
        MonitoringPointsMap[mxSkin, mySkin, mzSkin] = 1
        MonitoringPointsMap[mxBrain, myBrain, mzBrain] = 2
        MonitoringPointsMap[mxSkull, mySkull, mzSkull] = 3
        if not (cx == mxBrain and cy == myBrain and cz == mzBrain):
            MonitoringPointsMap[cx, cy, cz] = 4
    return (MonitoringPointsMap, np.array([mxSkin, mySkin, mzSkin]).astype(int), np.array([mxBrain, myBrain, mzBrain]).astype(int),
            np.array([mxSkull, mySkull, mzSkull]).astype(int))


METRICS = ('TI', 'TIS', 'TIC', 'CEMBrain', 'CEMSkin', 'CEMSkull', 'MaxBrainPressure', 'MI', 'MaxIsppa', 'MaxIspta', 'Ispta')


def exposure_metrics(ResTemp, FinalDose, p_map, SelBrain, SelSkin, SelSkull, MaterialList, BrainID, Frequency, DutyCycle, Isppa):
    """:1126-1151 as a dict of METRICS. MaxIsppa and MaxIspta are arrays over BrainID, as the reference's indexing with a list makes them."""
    TI = ResTemp[SelBrain].max()
    TIS = ResTemp[SelSkin].max()
    TIC = ResTemp[SelSkull].max()
    CEMBrain = FinalDose[SelBrain].max() / 60
    CEMSkin = FinalDose[SelSkin].max() / 60
    CEMSkull = FinalDose[SelSkull].max() / 60
    maxPressureLocation = p_map[SelBrain].argmax()
    MaxBrainPressure = p_map[SelBrain][maxPressureLocation]
    MI = MaxBrainPressure / 1e6 / np.sqrt(Frequency / 1e6)
    MaxIsppa = MaxBrainPressure ** 2 / (2.0 * MaterialList['SoS'][BrainID] * MaterialList['Density'][BrainID])
    MaxIsppa = MaxIsppa / 1e4
    MaxIspta = DutyCycle * MaxIsppa
    Ispta = DutyCycle * Isppa
    loc = locals()
    return {k: loc[k] for k in METRICS}


# ---------------------------------------------------------------- the two entries ----------------------------------------------------------------

def class_extrema(volumes, MaterialMap, classOf):
    """bfd_class_extrema3d in numpy: (count [8], maxIn, argIn, maxKey, argKey, each [nVol][8]). maxKey is the product at argKey."""
    classOf = np.asarray(classOf, np.uint8)
    cls = classOf[MaterialMap]
    nV = len(volumes)
    count = np.zeros(8, np.int64)
    maxIn, maxKey = np.zeros((nV, 8), np.float32), np.zeros((nV, 8), np.float32)
    argIn, argKey = np.full((nV, 8), -1, np.int64), np.full((nV, 8), -1, np.int64)
    for c in range(8):
        Sel = ((cls >> c) & 1).astype(bool)
        count[c] = np.count_nonzero(Sel)
        where = np.flatnonzero(Sel)
        for v, X in enumerate(volumes):
            assert X.dtype == np.float32 and X.shape == MaterialMap.shape
            if X.size == 0:
                continue
            if count[c]:
                at = X[Sel].argmax()
                maxIn[v, c], argIn[v, c] = X[Sel][at], where[at]
            prod = X * Sel.astype(np.float32)
            argKey[v, c] = np.argmax(prod, axis=None)
            maxKey[v, c] = prod.reshape(-1)[argKey[v, c]]
    return count, maxIn, argIn, maxKey, argKey


def loss_survey(p, pw, MaterialMap, classOf, rho, c, rhoWater, cWater, dx2, brainMask=None):
    """bfd_loss_survey3d in numpy for one field. A dict: maxTissue, argTissue, maxWater, argWater, water (the zeroed field), and the terms of every
    plane as float64 volumes termsWaterRaw, termsWater, termsTissue, with numpy's own plane sums eWaterRaw, eWater, eTissue [N3]."""
    classOf = np.asarray(classOf, np.uint8)
    cls = classOf[MaterialMap]
    SelBrain = (cls & 1).astype(bool) if brainMask is None else np.asarray(brainMask) != 0
    sel = ((cls >> 1) & 1).astype(bool)
    rho, c = np.asarray(rho, np.float64), np.asarray(c, np.float64)
    DensityMap, SoSMap = rho[MaterialMap], c[MaterialMap]
    raw = pw.copy()
    water = pw.copy()
    water[sel] = 0.0
    tissue = p.copy()
    tissue[SelBrain == False] = 0.0  # noqa: E712
    out = dict(water=water)
    for name, x in (('Water', water), ('Tissue', tissue)):
        if x.size:
            where = np.where(x == x.max())
            idx = np.ravel_multi_index((where[0][0], where[1][0], where[2][0]), x.shape)
            out['max' + name], out['arg' + name] = x.max(), int(idx)
        else:
            out['max' + name], out['arg' + name] = np.float32(0), -1
    N3 = p.shape[2]
    for name, x, R, C in (('WaterRaw', raw, None, None), ('Water', water, None, None), ('Tissue', tissue, DensityMap, SoSMap)):
        terms = np.zeros(p.shape, np.float64)
        sums = np.zeros(N3, np.float64)
        for k in range(N3):
            t = plane_terms(x[:, :, k], rhoWater if R is None else R[:, :, k], cWater if C is None else C[:, :, k], dx2)
            terms[:, :, k] = t
            sums[k] = np.ascontiguousarray(t).sum()
        out['terms' + name], out['e' + name] = terms, sums
    return out


# ---------------------------------------------------------------- the seeded builder ----------------------------------------------------------------

def build_case(shape=(24, 22, 40), seed=0, ct=False, segmented=False, homogeneous=False, benchmark=None, n_ct=0, split=False, target_at_max=False,
               map_dtype=np.uint32):
    """Everything a case needs, from parameters and a seed: a layered head along k (water, skin, bone, brain), the tissue and water pressure
    amplitudes of a focused beam with noise, temperature and dose fields, tables and grids. split: the tissue and the water field peak in different
    planes, with little water energy in the tissue's plane (the +0.2 switch of :230). target_at_max: the brain's temperature maximum is the target."""
    rng = np.random.default_rng(seed)
    N1, N2, N3 = shape
    k = np.arange(N3)
    wobble = rng.integers(0, 2, (N1, N2))
    depth = k[None, None, :] - wobble[:, :, None]
    M = np.zeros(shape, np.int64)
    s0, b0, t0, b1, br = (int(round(N3 * f)) for f in (0.15, 0.22, 0.27, 0.32, 0.38))
    if homogeneous:
        M[depth >= s0] = 1
        M[(depth >= b0) & (depth < br)] = 2
        nMat = 3
    elif benchmark is not None:
        nMat = benchmark['nMaterials']
        layers = np.linspace(s0, br, nMat)[1:].astype(int)
        for q, z in enumerate(layers):
            M[depth >= z] = q + 1
    elif ct:
        first = 6 if segmented else 3
        M[depth >= s0] = 1
        bone = (depth >= b0) & (depth < br)
        M[bone] = first + rng.integers(0, max(n_ct, 1), shape)[bone]
        M[depth >= br] = 2
        if segmented:
            inner = depth >= br
            M[inner] = 2 + rng.integers(0, 4, shape)[inner]
        nMat = first + max(n_ct, 1)
    else:
        M[depth >= s0] = 1
        M[depth >= b0] = 2
        M[(depth >= t0) & (depth < b1)] = 3
        M[(depth >= b1) & (depth < br)] = 2
        M[depth >= br] = 4
        nMat = 5
        if segmented:
            inner = depth >= br
            M[inner] = 4 + rng.integers(0, 4, shape)[inner]
            nMat = 8
    MaterialMap = M.astype(map_dtype)
    SoS = np.concatenate(([1500.0], rng.uniform(1450.0, 3100.0, nMat - 1)))
    Density = np.concatenate(([1000.0], rng.uniform(950.0, 2200.0, nMat - 1)))
    MaterialList = dict(SoS=SoS, Density=Density)
    h = 0.5e-3
    xf, yf, zf = (np.arange(N1) - N1 // 2) * h, (np.arange(N2) - N2 // 2) * h, np.arange(N3) * h + 1.25e-3
    Input = dict(x_vec=xf.copy(), y_vec=yf.copy(), z_vec=zf.copy())
    if ct:
        Input['MaterialMapCT'] = True
    LocIJK = np.array([N1 // 2 + 1, N2 // 2 - 1, int(N3 * 0.7)])          # beside the beam's axis
    i, j = np.meshgrid(np.arange(N1), np.arange(N2), indexing='ij')
    lateral = np.exp(-(((i - N1 / 2 + 0.3) / (N1 / 5)) ** 2 + ((j - N2 / 2 - 0.4) / (N2 / 5)) ** 2))

    def beam(zc, width, amp):
        axial = np.exp(-((k - zc) / width) ** 2) + 0.02
        return (amp * lateral[:, :, None] * axial[None, None, :] * rng.uniform(0.8, 1.2, shape)).astype(np.float32)
    if split:
        pAmp, pAmpWater = beam(N3 * 0.55, N3 / 20, 2.0e5), beam(N3 * 0.85, N3 / 30, 6.0e5)
    else:
        pAmp, pAmpWater = beam(N3 * 0.7, N3 / 8, 2.5e5), beam(N3 * 0.72, N3 / 8, 6.0e5)
    ResTemp = (37.0 + 4.0 * (pAmp / pAmp.max()) + rng.normal(0, 0.05, shape)).astype(np.float32)
    if target_at_max:
        ResTemp[tuple(LocIJK)] = 50.0
    FinalDose = (rng.uniform(0, 1, shape) * (ResTemp - 36.0) ** 2).astype(np.float32)
    # every maximum over the brain is attained twice, the second time one row and two columns on in the same plane: the first must win
    SelBrain = selections(MaterialMap, ct, segmented, homogeneous, benchmark)[0]
    for x in (pAmp, pAmpWater, ResTemp, FinalDose):
        a = np.unravel_index(np.argmax(np.where(SelBrain, x, -np.inf)), shape)
        b = ((a[0] + 1) % N1, (a[1] + 2) % N2, a[2])
        assert SelBrain[b] and np.ravel_multi_index(b, shape) != np.ravel_multi_index(a, shape)
        if np.ravel_multi_index(b, shape) < np.ravel_multi_index(a, shape):
            a, b = b, a
        x[b] = x[a] = max(x[a], x[b])
        if x is pAmp and segmented and not homogeneous and benchmark is None:
            # the target and the pressure maximum lie in different brain tissues: which of them AnalyzeLosses reads (:240-245) shows
            tissues = [2, 3, 4, 5] if ct else [4, 5, 6, 7]
            MaterialMap[tuple(LocIJK)] = next(t for t in tissues if t != MaterialMap[a])
    return dict(MaterialMap=MaterialMap, MaterialList=MaterialList, nMat=nMat, xf=xf, yf=yf, zf=zf, Input=Input, LocIJK=LocIJK, pAmp=pAmp,
                pAmpWater=pAmpWater, ResTemp=ResTemp, FinalDose=FinalDose)
