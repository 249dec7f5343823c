"""The domain setup between the mask file of Step 1 and the solver call of Step 2, TranscranialModeling/BabelIntegrationBASE.py, on the device:

    InitDomain(DeviceName, GPUBackend)
    survey(labels, box, flip_k)                            :1163, :1903-1908, :2162: label counts, tissue bounds and the focal voxel in one pass
    plan_domain(labels, SpatialStep, FocalLength=..., ...) :1840-2074: the two passes that size the domain around the incident beam cone
    assemble(labels, plan, ct_index, air, ...)             :2111-2201: MaterialMap, MaterialMapNoCT, SubAirRegions
    skull_density_ratio(ct_index, UniqueHU, plan, ...)     :816-854, :1384-1393: the skull density ratio, ray by ray

The volumes are the files as stored: the driver flips axis 2 of each when it loads it (:1161, :1176, :1179, :1844), here flip_k says so and the flipped
copy never exists; every index taken or returned is the driver's. The work on volumes runs on the MI355X through the C ABI (bfd_label_survey3d,
bfd_assemble_material_map3d and bfd_sdr_rays3d in csrc/bfd_domain.hip; definitions in include/babelfdtd.h); there is no CPU fallback. The cone of
:1967-1998 is a product of a set over (i, j) and a set over k, and what the loop reads from it are index bounds: plan_domain forms the two sets on
the host with the reference's own float64 expressions. Every result equals its literal numpy restatement (tests/domain_oracle.py) element for element.
Argument errors are raised before the library is loaded."""
import ctypes as C
import operator

import numpy as np

from . import _engine, _step1, harness, results

_device = 0
last_kernel_ms = None
LUT_BONE = 1 << 31                  # DM_LUT_BONE of csrc/bfd_domain_core.h
RAY_FEW, RAY_COUNTED, RAY_NOT_POSITIVE, RAY_EMPTY_CENTRE, RAY_BAD_INDEX = range(5)
STATS = ('bone_voxels', 'ct_min', 'ct_max', 'tissue_voxels', 'max_id', 'first_k', 'first_k_focal', 'ids_beyond_materials')


def InitDomain(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as InitMedianFilter does. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


def _exact(a, dtype, name):
    """`a` as a C-contiguous array of `dtype`. Another integer or float dtype (or bool) is taken if every value is an integer `dtype` holds."""
    a = np.asarray(a)
    dtype = np.dtype(dtype)
    if a.dtype != dtype:
        if a.dtype.kind not in 'buif':
            raise ValueError('%s must hold numbers, not %s' % (name, a.dtype))
        if a.size:
            mn, mx = a.min(), a.max()
            if not (mn >= 0 and mx <= np.iinfo(dtype).max):          # a NaN fails both
                raise ValueError('%s holds values outside what %s holds (min %r, max %r)' % (name, dtype, mn, mx))
        b = a.astype(dtype)
        if not np.array_equal(b, a):
            raise ValueError('%s holds values that are not integers' % name)
        a = b
    return np.ascontiguousarray(a)


def _volume(a, dtype, name, shape=None):
    a = _exact(a, dtype, name)
    if a.ndim != 3:
        raise ValueError('%s must be a 3-D volume, not %d-D' % (name, a.ndim))
    if a.size >= 2 ** 31:
        raise ValueError('%s has 2^31 voxels or more' % name)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError('%s has shape %r, the labels %r' % (name, a.shape, tuple(shape)))
    return a


def _ct_volume(ct_index, shape=None):
    """The index map as uint16 or uint32: those as they are, anything else as uint32 if its values allow"""
    a = np.asarray(ct_index)
    return _volume(a, a.dtype if a.dtype in (np.uint16, np.uint32) else np.uint32, 'ct_index', shape)


def _box(box, shape):
    if box is None:
        return np.zeros(3, np.int64), np.array(shape, np.int64)
    try:
        lo, hi = (np.array([operator.index(x) for x in b], np.int64) for b in box)
    except (TypeError, ValueError):
        raise ValueError('box must be (lo[3], hi[3]) of ints, not %r' % (box,))
    if lo.shape != (3,) or hi.shape != (3,) or np.any(lo < 0) or np.any(lo > hi) or np.any(hi > np.array(shape)):
        raise ValueError('box %r is not 0 <= lo <= hi <= %r' % (box, tuple(shape)))
    return lo, hi


def survey(labels, box=None, flip_k=True):
    """(hist, bounds, focal) of bfd_label_survey3d. labels: the uint8 label volume as stored; box: (lo, hi), half-open, in driver coordinates (None:
    the whole volume). hist: int64 [256], the label counts inside the box; bounds: int64 [6], per axis the smallest and the largest index inside the
    box with label > 0, relative to lo, -1 where none; focal: int64 [2], the number of voxels equal to 5 in the whole volume and the smallest C-order
    linear index of one in driver coordinates, -1 if none."""
    global last_kernel_ms
    a = _volume(labels, np.uint8, 'labels')
    lo, hi = _box(box, a.shape)
    hist, bounds, focal = np.zeros(256, np.int64), np.zeros(6, np.int64), np.zeros(2, np.int64)
    ms = C.c_float()
    _step1.call('bfd_label_survey3d', _device, _engine._ptr(a), a.shape[0], a.shape[1], a.shape[2], _engine._ptr(lo), _engine._ptr(hi), int(bool(flip_k)),
                _engine._ptr(hist), _engine._ptr(bounds), _engine._ptr(focal), C.byref(ms))
    last_kernel_ms = ms.value
    return hist, bounds, focal


class DomainPlan:
    """What the loop of :1874-2068 leaves on `self`, under the reference's names without the underscore: N1..N3, the six offsets (XLOffset ..
    ZROffset), the six shrinks (XShrink_L .. ZShrink_R), FocalSpotLocation, ZSourceLocation, XDim / YDim / ZDim, and region_count, the number of
    voxels of the cone of the last pass. box_lo / box_hi: the part of the label volume the domain holds, in driver coordinates."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def shape(self):
        return (self.N1, self.N2, self.N3)

    @property
    def pad_lo(self):
        return (self.XLOffset, self.YLOffset, self.ZLOffset)

    @property
    def pad_hi(self):
        return (self.XROffset, self.YROffset, self.ZROffset)

    def region_sets(self):
        """(A, Z): bool [N1][N2] and bool [N3]. The cone of the last pass, RegionMap of :1980-1997, is A[:, :, None] & Z[None, None, :]; the debug mask
        of :2127-2151 is formed from it."""
        return self._region_ij, self._region_k

    def crop(self):
        return results.Crop(self.XLOffset, self.XROffset, self.YLOffset, self.YROffset, self.ZLOffset, self.ZROffset, self.XShrink_L, self.YShrink_L,
                            self.ZShrink_L)

    def time_plan(self, dt, ppp, c0, sensor_sub=0, cycles=harness.CYCLES_TO_TRACK):
        """TimeSimulation, nt, SensorSubSampling, SensorStart of :2082-2109 for this domain (harness.time_plan)"""
        return harness.time_plan(self.N1, self.N2, self.N3, self.SpatialStep, dt, ppp, c0, pml=self.PMLThickness, sensor_sub=sensor_sub, cycles=cycles)


def _axis_rule(ind, ffs, stepf, N, pml, tight, isZ, LOffset, ROffset, Shrink_L, Shrink_R):
    """The rule the reference writes out per axis at :2026-2048. ind: the sorted indices of the axis the cone holds; ffs: the rows of AllFF."""
    edgeDist = np.min(np.vstack(ffs), axis=0)

    def bound(fn):
        if ind.size == 0:
            raise ValueError('the beam cone holds no voxel of the domain: there is no bound to read (:2038, :2046)')
        return int(fn(ind))
    if np.any(ind < pml):
        LOffset += int(np.ceil((1.0 - edgeDist[pml]) / stepf))
    elif tight:
        if LOffset == pml:
            Shrink_L += bound(np.min) - LOffset
    if np.any(ind >= N - pml) and not (isZ and tight):
        ROffset += int(np.ceil((1.0 - edgeDist[-pml]) / stepf))
    elif tight and not isZ:
        if ROffset == pml:
            Shrink_R += N - ROffset - bound(np.max) - 1
    return LOffset, ROffset, Shrink_L, Shrink_R


def plan_domain(labels, SpatialStep, *, PMLThickness=12, FocalLength, Aperture, ZIntoSkin=0.0, TxMechanicalAdjustmentX=0.0, TxMechanicalAdjustmentY=0.0,
                TxMechanicalAdjustmentZ=0.0, ExtraDepthAdjust=0.0, ExtraAdjustX=(0.0,), ExtraAdjustY=(0.0,), PaddingForRayleigh=0, PaddingForKArray=0,
                ZTxCorrecton=0.0, bTightNarrowBeamDomain=False, zLengthBeyonFocalPointWhenNarrow=4e-2, DomeType=False, flip_k=True, survey=None):
    """The DomainPlan of UpdateConditions, :1840-2074, for the label volume `labels` (uint8, as stored) and the parameters the method reads from
    `self`, under their names there. Two passes: the first grows an offset where the cone reaches into the absorbing layer and, with
    bTightNarrowBeamDomain, shrinks the crop to the cone; the second sizes the domain. Each pass calls survey once on the crop in force; no
    volume is formed on the host. survey: a callable with survey's signature that the two passes call instead (None: survey itself, which uploads the
    labels for each call; AcousticStudy.survey reads labels that are on the device already). ValueError where the reference raises: not exactly one voxel of 5, no tissue in the crop, empty ExtraAdjust lists,
    a bound read from an empty cone. NotImplementedError for DomeType."""
    if DomeType:
        raise NotImplementedError('DomeType domains are not planned here')
    a = _volume(labels, np.uint8, 'labels')
    pml = operator.index(PMLThickness)
    if pml < 1:
        raise ValueError('PMLThickness must be at least 1, not %r' % (PMLThickness,))
    if not (np.isfinite(SpatialStep) and SpatialStep > 0):
        raise ValueError('SpatialStep must be positive, not %r' % (SpatialStep,))
    ExtraAdjustX, ExtraAdjustY = list(ExtraAdjustX), list(ExtraAdjustY)
    if not ExtraAdjustX or not ExtraAdjustY:
        raise ValueError('ExtraAdjustX and ExtraAdjustY must hold at least one entry (the reference raises at :1991 otherwise)')
    tight = bool(bTightNarrowBeamDomain)
    survey_of = globals()['survey'] if survey is None else survey          # the keyword carries the function's name; the module's is looked up per call
    M = np.array(a.shape, np.int64)
    ZSourceLocation = int(np.round(ZIntoSkin / SpatialStep)) + pml
    LOff = [pml, pml, pml + operator.index(PaddingForRayleigh) + operator.index(PaddingForKArray) + int(np.round(ZTxCorrecton / SpatialStep))]
    ROff = [pml, pml, pml]
    ShL, ShR = [0, 0, 0], [0, 0, 0]
    adjust = (TxMechanicalAdjustmentX, TxMechanicalAdjustmentY)
    bComplete = False
    with np.errstate(all='ignore'):
        while True:
            N = [int(M[q]) + LOff[q] + ROff[q] - ShL[q] - ShR[q] for q in range(3)]
            hi = [int(M[q]) - ShR[q] for q in range(3)]
            if any(ShL[q] < 0 or ShL[q] > hi[q] for q in range(3)):
                raise ValueError('the crop %r : %r is empty or outside the label volume' % (ShL, hi))
            _, bounds, focal = survey_of(a, (list(ShL), hi), flip_k)
            if bounds[4] < 0:
                raise ValueError('no tissue in the crop %r : %r of the label volume (np.min of an empty array at :1904)' % (ShL, hi))
            FirstVoxelTissueZ = int(bounds[4]) + LOff[2]
            if focal[0] != 1:
                raise ValueError('the label volume must hold exactly one voxel equal to 5, not %d (:1908-1910)' % focal[0])
            orig = np.array(np.unravel_index(int(focal[1]), a.shape))
            Focal = orig + np.array(LOff) - np.array(ShL)
            fields = [np.arange(N[q]) * SpatialStep for q in range(3)]
            for q in range(3):
                fields[q] -= fields[q][Focal[q]]
            xfield, yfield, zfield = fields
            zfield += FocalLength
            TopZ = zfield[pml]
            if FocalLength != 0:
                Alpha = np.arcsin(Aperture / 2 / (FocalLength + ExtraDepthAdjust))
                DistanceToFocus = FocalLength - TopZ + TxMechanicalAdjustmentZ + ExtraDepthAdjust
                RadiusFace = DistanceToFocus * np.tan(Alpha)
                if RadiusFace > Aperture / 2:
                    RadiusFace = Aperture / 2
                RadiusFace *= 1.1
                ZReZero = -FocalLength - TxMechanicalAdjustmentZ - +ExtraDepthAdjust
                ZConeLimit = -DistanceToFocus
            else:
                RadiusFace = Aperture / 2 * 1.10
                ZReZero = 0
                ZConeLimit = TopZ - TxMechanicalAdjustmentZ
            f2 = [(fields[q] - adjust[q]) / RadiusFace for q in range(2)]
            ffs = [[np.abs(f2[0])], [np.abs(f2[1])]]
            zf2 = (zfield + ZReZero) / ZConeLimit
            Zffs = [zf2]
            # the cone of :1978-1989: every term of the union carries the same conditions on z (the operator precedence of :1987-1989)
            A = (f2[0] ** 2)[:, None] + (f2[1] ** 2)[None, :] <= 1.0
            for EX, EY in zip(ExtraAdjustX, ExtraAdjustY):
                ffs[0].append(np.abs(f2[0] - EX / RadiusFace))
                ffs[1].append(np.abs(f2[1] - EY / RadiusFace))
                Zffs.append(zf2)
                A = A | ((ffs[0][-1] ** 2)[:, None] + (ffs[1][-1] ** 2)[None, :] <= 1.0)
            Z = (zf2 >= 0) & (zf2 <= 1.0) & (zf2 <= zf2[FirstVoxelTissueZ])
            nA, nZ = int(A.sum()), int(Z.sum())
            region_count = nA * nZ
            if bComplete:
                break
            empty = np.zeros(0, np.int64)
            ind = [np.nonzero(A.any(axis=1))[0] if nZ else empty, np.nonzero(A.any(axis=0))[0] if nZ else empty, np.nonzero(Z)[0] if nA else empty]
            steps = [np.abs(np.mean(np.diff(f2[0]))), np.abs(np.mean(np.diff(f2[1]))), np.abs(np.mean(np.diff(zf2)))]
            allffs = [ffs[0], ffs[1], Zffs]
            for q in range(3):
                LOff[q], ROff[q], ShL[q], ShR[q] = _axis_rule(ind[q], allffs[q], steps[q], N[q], pml, tight, q == 2, LOff[q], ROff[q], ShL[q], ShR[q])
            if tight:
                nStepsZReduction = int(zLengthBeyonFocalPointWhenNarrow / SpatialStep)
                ShR[2] = max(N[2] - (int(Focal[2]) + nStepsZReduction) - ROff[2], 0)
            bComplete = True
    return DomainPlan(N1=N[0], N2=N[1], N3=N[2], XLOffset=LOff[0], YLOffset=LOff[1], ZLOffset=LOff[2], XROffset=ROff[0], YROffset=ROff[1], ZROffset=ROff[2],
                      XShrink_L=ShL[0], YShrink_L=ShL[1], ZShrink_L=ShL[2], XShrink_R=ShR[0], YShrink_R=ShR[1], ZShrink_R=ShR[2],
                      FocalSpotLocation=Focal, ZSourceLocation=ZSourceLocation, XDim=xfield, YDim=yfield, ZDim=zfield, region_count=region_count,
                      _region_ij=A, _region_k=Z, box_lo=tuple(ShL), box_hi=tuple(hi), mask_shape=tuple(a.shape), flip_k=bool(flip_k),
                      SpatialStep=SpatialStep, PMLThickness=pml, bTightNarrowBeamDomain=tight)


def relabel_lut(ct, brain_segmentation):
    """The 256-entry table of bfd_assemble_material_map3d: the sequential in-place relabels of :2169-2173 (with a CT) or :2196-2198 (without), run in
    the reference's order on every raw label; with a CT, bit 31 marks the bone (:2165, :2181)."""
    v = np.arange(256, dtype=np.uint32)
    bone = (v == 2) | (v == 3)
    if ct:
        if brain_segmentation:
            v[v == 4] = 2
            v[v == 5] = 2
            v[v >= 6] -= 3
        else:
            v[v >= 4] = 2
        v[bone] |= np.uint32(LUT_BONE)
    elif brain_segmentation:
        v[v >= 5] -= 1
    else:
        v[v == 5] = 4
    return v


def _check_plan(plan, shape):
    if tuple(plan.mask_shape) != tuple(shape):
        raise ValueError('the plan was made for a label volume of shape %r, not %r' % (tuple(plan.mask_shape), tuple(shape)))


def assemble(labels, plan, ct_index=None, air=None, n_materials=None, water_only=False, ct_offset=None):
    """(MaterialMap, MaterialMapNoCT, SubAirRegions, stats) of :2111-2201 on the plan's domain. labels: uint8, as stored; ct_index: the index map of
    *CT.nii.gz as stored (uint16 or uint32, without the offset of :1241-1244) or None; air: the mask of *AirRegions.nii.gz or None (read with a CT
    only, as in the reference); n_materials: the rows of the material list (None: not checked). ct_offset: 6 where the whole label volume holds a label
    above 5 and 3 otherwise (:1241-1244) unless given. MaterialMapNoCT is None without a CT, SubAirRegions without air. stats: a dict of the names
    in STATS. With water_only the map is all water and nothing else is returned (:2203). ValueError with the reference's condition where :2191-2192
    would assert, and where there is no bone under a CT. bForceHomogenousMedium and BenchmarkTestFile stay with the caller."""
    global last_kernel_ms
    a = _volume(labels, np.uint8, 'labels')
    _check_plan(plan, a.shape)
    if water_only:
        return np.zeros(plan.shape, np.uint32), None, None, None
    ct = None if ct_index is None else _ct_volume(ct_index, a.shape)
    ar = None if air is None or ct is None else _volume(_step1.bool_as_uint8(np.asarray(air)), np.uint8, 'air', a.shape)
    if n_materials is not None:
        n_materials = operator.index(n_materials)
        if not 0 <= n_materials < 2 ** 32:
            raise ValueError('n_materials must be 0 .. 2^32 - 1, not %r' % (n_materials,))
    lo, hi = _box((plan.box_lo, plan.box_hi), a.shape)
    flip = bool(plan.flip_k)
    segmented = bool(survey(a, (lo, hi), flip)[0][6:].any())                         # :2162, on the crop
    offset = 0
    if ct is not None:
        offset = operator.index(ct_offset) if ct_offset is not None else (6 if survey(a, None, flip)[0][6:].any() else 3)       # :1163, on the whole volume
        if not 0 <= offset < 2 ** 32:
            raise ValueError('ct_offset must be 0 .. 2^32 - 1, not %r' % (ct_offset,))
    lut = relabel_lut(ct is not None, segmented)
    size = hi - lo
    padLo, padHi = np.array(plan.pad_lo, np.int64), np.array(plan.pad_hi, np.int64)
    if tuple(size + padLo + padHi) != tuple(plan.shape):
        raise ValueError('the plan is not consistent: box %r, offsets %r and %r, domain %r' % (tuple(size), plan.pad_lo, plan.pad_hi, plan.shape))
    focalIJ = np.array(plan.FocalSpotLocation[:2], np.int64)
    out = np.empty(plan.shape, np.uint32)
    noct = np.empty(plan.shape, np.uint32) if ct is not None else None
    airOut = np.empty(plan.shape, np.uint32) if ar is not None else None
    stats = np.zeros(8, np.int64)
    ms = C.c_float()
    _step1.call('bfd_assemble_material_map3d', _device, _engine._ptr(a), _engine._ptr(ct), 0 if ct is None else ct.itemsize, _engine._ptr(ar), a.shape[0],
                a.shape[1], a.shape[2], _engine._ptr(lo), _engine._ptr(size), _engine._ptr(padLo), _engine._ptr(padHi), int(flip), _engine._ptr(lut), offset,
                int(plan.ZSourceLocation), 2 ** 32 - 1 if n_materials is None else n_materials, _engine._ptr(focalIJ), _engine._ptr(out), _engine._ptr(noct),
                _engine._ptr(airOut), _engine._ptr(stats), C.byref(ms))
    last_kernel_ms = ms.value
    st = dict(zip(STATS, (int(x) for x in stats)))
    if ct is not None:
        if st['bone_voxels'] == 0:
            raise ValueError('the crop holds no bone (labels 2, 3): SubCTMap[BoneRegion].min() of an empty array (:2191)')
        if not st['ct_min'] >= 3:
            raise ValueError('SubCTMap[BoneRegion].min()>=3 does not hold: the minimum is %d (:2191)' % st['ct_min'])
        if n_materials is not None and not st['ct_max'] <= n_materials:
            raise ValueError('SubCTMap[BoneRegion].max()<=self.ReturnArrayMaterial().shape[0] does not hold: the maximum is %d, the rows %d (:2192)'
                             % (st['ct_max'], n_materials))
    return out, noct, airOut, st


def sdr_rays(ct_index, UniqueHU, box, step_i, step_j, min_skull_voxels=3, center_region=0.5, flip_k=True):
    """(value, count, state) of bfd_sdr_rays3d, each of the lattice's shape. UniqueHU: float32 or float64 (any other dtype is taken as float64)."""
    global last_kernel_ms
    ct = _ct_volume(ct_index)
    hu = np.asarray(UniqueHU)
    if hu.dtype not in (np.float32, np.float64):
        hu = hu.astype(np.float64)
    hu = np.ascontiguousarray(hu)
    if hu.ndim != 1 or hu.size < 1:
        raise ValueError('UniqueHU must be a table of at least one value, not an array of shape %r' % (hu.shape,))
    if not np.all(np.isfinite(hu)):
        raise ValueError('UniqueHU holds a value that is not finite')
    lo, hi = _box(box, ct.shape)
    try:
        step_i, step_j, min_skull_voxels = operator.index(step_i), operator.index(step_j), operator.index(min_skull_voxels)
    except TypeError:
        raise ValueError('step_i, step_j and min_skull_voxels must be ints')
    if not (1 <= step_i < 2 ** 31 and 1 <= step_j < 2 ** 31):
        raise ValueError('step_i and step_j must be at least 1, not %r, %r' % (step_i, step_j))
    if not 1 <= min_skull_voxels < 2 ** 31:
        raise ValueError('min_skull_voxels must be at least 1, not %r' % (min_skull_voxels,))
    center_region = float(center_region)
    if not (np.isfinite(center_region) and center_region >= 0):
        raise ValueError('center_region must be finite and not negative, not %r' % (center_region,))
    size = hi - lo
    lattice = (-(-int(size[0]) // step_i), -(-int(size[1]) // step_j))
    value, count, state = np.zeros(lattice, hu.dtype), np.zeros(lattice, np.int32), np.zeros(lattice, np.uint8)
    ms = C.c_float()
    _step1.call('bfd_sdr_rays3d', _device, _engine._ptr(ct), ct.itemsize, ct.shape[0], ct.shape[1], ct.shape[2], _engine._ptr(lo), _engine._ptr(size),
                int(bool(flip_k)), _engine._ptr(hu), hu.itemsize, hu.size, step_i, step_j, min_skull_voxels, center_region, _engine._ptr(value),
                _engine._ptr(count), _engine._ptr(state), C.byref(ms))
    last_kernel_ms = ms.value
    return value, count, state


def skull_density_ratio(ct_index, UniqueHU, plan, spacing_mm, ray_spacing_mm=1.8, min_skull_voxels=3, center_region=0.5, return_rays=False):
    """The skull density ratio of :1384-1393 and compute_sdr_from_rays (:816-854) on the plan's crop of the CT index volume (as stored, without the
    offset). spacing_mm: the voxel size along axes 0 and 1 (one number for both). The mean of the rays that counted, in the table's dtype, nan where
    none did; with return_rays also (value, count, state). IndexError where an index on a ray is beyond the table, ValueError where the centre slice
    of a ray is empty, as numpy raises in the reference."""
    ct = _ct_volume(ct_index)
    _check_plan(plan, ct.shape)
    sp = np.broadcast_to(np.asarray(spacing_mm, np.float64), (2,)) if np.ndim(spacing_mm) == 0 else np.asarray(spacing_mm, np.float64)
    if sp.shape[0] < 2 or not np.all(sp[:2] > 0):
        raise ValueError('spacing_mm must be one or two positive numbers, not %r' % (spacing_mm,))
    step_i = max(1, int(round(ray_spacing_mm / sp[0])))
    step_j = max(1, int(round(ray_spacing_mm / sp[1])))
    value, count, state = sdr_rays(ct, UniqueHU, (plan.box_lo, plan.box_hi), step_i, step_j, min_skull_voxels, center_region, plan.flip_k)
    if np.any(state == RAY_BAD_INDEX):
        raise IndexError('the CT index volume holds an index beyond the %d rows of UniqueHU' % np.size(UniqueHU))
    if np.any(state == RAY_EMPTY_CENTRE):
        raise ValueError('the centre slice of a ray is empty: center_region %r selects no voxel (min of an empty array at :846)' % (center_region,))
    sel = value[state == RAY_COUNTED]
    sdr = np.mean(sel) if sel.size else float('nan')
    return (sdr, (value, count, state)) if return_rays else sdr
