"""Literal numpy restatements of the domain setup of Step 2 (include/babelfdtd.h: bfd_label_survey3d, bfd_assemble_material_map3d, bfd_sdr_rays3d;
babelbrain_amd/Domain.py), for the host and the device tests: the flipped copy, the 3-D cone from np.meshgrid, np.nonzero over whole volumes, slices,
sequential in-place relabels and the Python ray loop. Written from the definitions; slow on purpose. The `fault` arguments plant the mistakes the
tests must be able to see."""
import numpy as np

PLAN_FIELDS = ('N1', 'N2', 'N3', 'XLOffset', 'YLOffset', 'ZLOffset', 'XROffset', 'YROffset', 'ZROffset', 'XShrink_L', 'YShrink_L', 'ZShrink_L',
               'XShrink_R', 'YShrink_R', 'ZShrink_R', 'ZSourceLocation', 'region_count')
DEFAULTS = dict(PMLThickness=12, ZIntoSkin=0.0, TxMechanicalAdjustmentX=0.0, TxMechanicalAdjustmentY=0.0, TxMechanicalAdjustmentZ=0.0,
                ExtraDepthAdjust=0.0, ExtraAdjustX=(0.0,), ExtraAdjustY=(0.0,), PaddingForRayleigh=0, PaddingForKArray=0, ZTxCorrecton=0.0,
                bTightNarrowBeamDomain=False, zLengthBeyonFocalPointWhenNarrow=4e-2)


def driver(volume, flip_k=True):
    """The volume as the driver holds it"""
    return np.flip(volume, axis=2) if flip_k else np.asarray(volume)


# ---------------------------------------------------------------- survey ----------------------------------------------------------------

def survey(labels, box=None, flip_k=True):
    """(hist, bounds, focal) of bfd_label_survey3d"""
    D = driver(np.asarray(labels), flip_k)
    lo, hi = ((0, 0, 0), D.shape) if box is None else box
    sub = D[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    hist = np.bincount(sub.ravel().astype(np.int64), minlength=256).astype(np.int64)
    idx = np.nonzero(sub > 0)
    bounds = np.full(6, -1, np.int64)
    if idx[0].size:
        bounds[:] = [idx[0].min(), idx[0].max(), idx[1].min(), idx[1].max(), idx[2].min(), idx[2].max()]
    five = np.flatnonzero(np.ascontiguousarray(D) == 5)
    focal = np.array([five.size, five[0] if five.size else -1], np.int64)
    return hist, bounds, focal


# ---------------------------------------------------------------- the plan ----------------------------------------------------------------

class Plan:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def shape(self):
        return (self.N1, self.N2, self.N3)


def plan(labels, SpatialStep, FocalLength, Aperture, flip_k=True, **kw):
    """The two passes of the domain loop with the cone as a 3-D volume. Returns a Plan with the fields of Domain.DomainPlan and RegionMap, the 3-D
    cone of the last pass."""
    p = dict(DEFAULTS, **kw)
    pml, tight = p['PMLThickness'], p['bTightNarrowBeamDomain']
    D = driver(np.asarray(labels), flip_k)
    M = D.shape
    ZSourceLocation = int(np.round(p['ZIntoSkin'] / SpatialStep)) + pml
    off = {'XL': pml, 'YL': pml, 'XR': pml, 'YR': pml, 'ZR': pml,
           'ZL': pml + p['PaddingForRayleigh'] + p['PaddingForKArray'] + int(np.round(p['ZTxCorrecton'] / SpatialStep))}
    sh = {k: 0 for k in ('XL', 'XR', 'YL', 'YR', 'ZL', 'ZR')}
    done = False
    while True:
        N = [M[q] + off[ax + 'L'] + off[ax + 'R'] - sh[ax + 'L'] - sh[ax + 'R'] for q, ax in enumerate('XYZ')]
        upper = [M[q] if sh[ax + 'R'] == 0 else -sh[ax + 'R'] for q, ax in enumerate('XYZ')]
        Temp = np.zeros(N, np.uint32)
        Temp[off['XL']:-off['XR'], off['YL']:-off['YR'], off['ZL']:-off['ZR']] = D.astype(np.uint32)[sh['XL']:upper[0], sh['YL']:upper[1], sh['ZL']:upper[2]]
        mz = np.where(Temp > 0)[2]
        FirstVoxelTissueZ = np.min(mz)
        Focal = np.array(np.where(D == 5)).flatten()
        Focal = Focal + np.array([off['XL'], off['YL'], off['ZL']])
        Focal = Focal - np.array([sh['XL'], sh['YL'], sh['ZL']])
        xfield, yfield, zfield = (np.arange(n) * SpatialStep for n in N)
        xfield -= xfield[Focal[0]]
        yfield -= yfield[Focal[1]]
        zfield -= zfield[Focal[2]]
        zfield += FocalLength
        TopZ = zfield[pml]
        with np.errstate(all='ignore'):
            if FocalLength != 0:
                Alpha = np.arcsin(Aperture / 2 / (FocalLength + p['ExtraDepthAdjust']))
                DistanceToFocus = FocalLength - TopZ + p['TxMechanicalAdjustmentZ'] + p['ExtraDepthAdjust']
                RadiusFace = DistanceToFocus * np.tan(Alpha)
                if RadiusFace > Aperture / 2:
                    RadiusFace = Aperture / 2
                RadiusFace *= 1.1
                ZReZero = -FocalLength - p['TxMechanicalAdjustmentZ'] - +p['ExtraDepthAdjust']
                ZConeLimit = -DistanceToFocus
            else:
                RadiusFace = Aperture / 2 * 1.10
                ZReZero = 0
                ZConeLimit = TopZ - p['TxMechanicalAdjustmentZ']
            xf2 = (xfield - p['TxMechanicalAdjustmentX']) / RadiusFace
            yf2 = (yfield - p['TxMechanicalAdjustmentY']) / RadiusFace
            ffs = {'X': [np.abs(xf2)], 'Y': [np.abs(yf2)]}
            zf2 = (zfield + ZReZero) / ZConeLimit
            ffs['Z'] = [zf2]
            xpp, ypp, zpp = np.meshgrid(xf2 ** 2, yf2 ** 2, zf2, indexing='ij')
            RegionMap = ((xpp + ypp) <= 1.0) & (zpp >= 0) & (zpp <= 1.0)
            for EX, EY in zip(p['ExtraAdjustX'], p['ExtraAdjustY']):
                ffs['X'].append(np.abs(xf2 - EX / RadiusFace))
                ffs['Y'].append(np.abs(yf2 - EY / RadiusFace))
                ffs['Z'].append(zf2)
                xpp2, ypp2, zpp2 = np.meshgrid(ffs['X'][-1] ** 2, ffs['Y'][-1] ** 2, zf2, indexing='ij')
                RegionMap = RegionMap | (((xpp2 + ypp2) <= 1.0) & (zpp2 >= 0) & (zpp <= 1.0))
            RegionMap = RegionMap & (zpp <= zf2[FirstVoxelTissueZ])
        Ind = dict(zip('XYZ', np.nonzero(RegionMap)))
        if done:
            break
        step = {'X': np.abs(np.mean(np.diff(xf2))), 'Y': np.abs(np.mean(np.diff(yf2))), 'Z': np.abs(np.mean(np.diff(zf2)))}
        for q, ax in enumerate('XYZ'):
            edgeDist = np.min(np.vstack(ffs[ax]), axis=0)
            if np.any(Ind[ax] < pml):
                off[ax + 'L'] += int(np.ceil((1.0 - edgeDist[pml]) / step[ax]))
            elif tight:
                if off[ax + 'L'] == pml:
                    sh[ax + 'L'] += Ind[ax].min() - off[ax + 'L']
            if np.any(Ind[ax] >= N[q] - pml) and (ax != 'Z' or not tight):
                off[ax + 'R'] += int(np.ceil((1.0 - edgeDist[-pml]) / step[ax]))
            elif tight and ax != 'Z':
                if off[ax + 'R'] == pml:
                    sh[ax + 'R'] += N[q] - off[ax + 'R'] - Ind[ax].max() - 1
        if tight:
            sh['ZR'] = N[2] - (Focal[2] + int(p['zLengthBeyonFocalPointWhenNarrow'] / SpatialStep)) - off['ZR']
            if sh['ZR'] < 0:
                sh['ZR'] = 0
        done = True
    box_hi = tuple(int(M[q] - sh[ax + 'R']) for q, ax in enumerate('XYZ'))
    return Plan(N1=N[0], N2=N[1], N3=N[2], XLOffset=off['XL'], YLOffset=off['YL'], ZLOffset=off['ZL'], XROffset=off['XR'], YROffset=off['YR'],
                ZROffset=off['ZR'], XShrink_L=int(sh['XL']), YShrink_L=int(sh['YL']), ZShrink_L=int(sh['ZL']), XShrink_R=int(sh['XR']),
                YShrink_R=int(sh['YR']), ZShrink_R=int(sh['ZR']), FocalSpotLocation=Focal, ZSourceLocation=ZSourceLocation, XDim=xfield, YDim=yfield,
                ZDim=zfield, region_count=int(RegionMap.sum()), RegionMap=RegionMap, box_lo=(int(sh['XL']), int(sh['YL']), int(sh['ZL'])), box_hi=box_hi,
                mask_shape=tuple(M), flip_k=flip_k, SpatialStep=SpatialStep, PMLThickness=pml)


# ---------------------------------------------------------------- the maps ----------------------------------------------------------------

def padded(volume, pl):
    """The plan's crop of a driver volume inside a zero volume of the domain's shape, uint32"""
    out = np.zeros(pl.shape, np.uint32)
    lo, hi = pl.box_lo, pl.box_hi
    out[pl.XLOffset:pl.shape[0] - pl.XROffset, pl.YLOffset:pl.shape[1] - pl.YROffset, pl.ZLOffset:pl.shape[2] - pl.ZROffset] = \
        np.asarray(volume).astype(np.uint32)[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    return out


def relabel(MaterialMap, ct, brain_segmentation):
    """The in-place statements, in order"""
    if ct:
        if brain_segmentation:
            MaterialMap[MaterialMap == 4] = 2
            MaterialMap[MaterialMap == 5] = 2
            MaterialMap[MaterialMap >= 6] -= 3
        else:
            MaterialMap[MaterialMap >= 4] = 2
    elif brain_segmentation:
        MaterialMap[MaterialMap >= 5] -= 1
    else:
        MaterialMap[MaterialMap == 5] = 4
    return MaterialMap


def assemble(labels, pl, ct_index=None, air=None, n_materials=None, fault=None):
    """(MaterialMap, MaterialMapNoCT, SubAirRegions, stats) as Domain.assemble returns them; stats without the checks. fault: 'water_short' (the water
    layer one plane short), 'offset3' (3 where 6 is due), 'noct_late' (MaterialMapNoCT taken after the relabelling)."""
    D = driver(np.asarray(labels), pl.flip_k)
    MaterialMap = padded(D, pl)
    seg = bool(np.any(MaterialMap > 5))
    noct = airOut = None
    bone_n, ct_min, ct_max = 0, -1, -1
    if ct_index is not None:
        offset = 6 if np.any(D > 5) and fault != 'offset3' else 3
        DensityCTMap = driver(np.asarray(ct_index), pl.flip_k).astype(np.uint32) + np.uint32(offset)
        BoneRegion = (MaterialMap == 2) | (MaterialMap == 3)
        if fault != 'noct_late':
            noct = MaterialMap.copy()
        relabel(MaterialMap, True, seg)
        if fault == 'noct_late':
            noct = MaterialMap.copy()
        SubCTMap = padded(DensityCTMap, pl)
        MaterialMap[BoneRegion] = SubCTMap[BoneRegion]
        if air is not None:
            airOut = padded(driver(np.asarray(air), pl.flip_k), pl)
        bone_n = int(BoneRegion.sum())
        if bone_n:
            ct_min, ct_max = int(SubCTMap[BoneRegion].min()), int(SubCTMap[BoneRegion].max())
    else:
        relabel(MaterialMap, False, seg)
    MaterialMap[:, :, :pl.ZSourceLocation + (0 if fault == 'water_short' else 1)] = 0
    kk = np.where(MaterialMap > 0)[2]
    line = np.where(MaterialMap[pl.FocalSpotLocation[0], pl.FocalSpotLocation[1], :] > 0)[0]
    limit = 2 ** 32 - 1 if n_materials is None else n_materials
    stats = dict(bone_voxels=bone_n, ct_min=ct_min, ct_max=ct_max, tissue_voxels=int((MaterialMap > 0).sum()), max_id=int(MaterialMap.max()),
                 first_k=int(kk.min()) if kk.size else -1, first_k_focal=int(line.min()) if line.size else -1,
                 ids_beyond_materials=int((MaterialMap.astype(np.int64) >= limit).sum()))
    return MaterialMap, noct, airOut, stats


def assemble_entry(labels, ct, air, lo, size, padLo, padHi, flip_k, lut, ctOffset, zWater, nMaterials, focalIJ):
    """(map, mapNoCT, airOut, stats[8]) of bfd_assemble_material_map3d, from its definition"""
    N = tuple(int(s + a + b) for s, a, b in zip(size, padLo, padHi))

    def pad(v):
        out = np.zeros(N, np.uint32)
        out[padLo[0]:padLo[0] + size[0], padLo[1]:padLo[1] + size[1], padLo[2]:padLo[2] + size[2]] = \
            driver(v, flip_k)[lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]]
        return out
    raw = pad(labels)
    inside = pad(np.ones(labels.shape, np.uint8)) > 0
    lut = np.asarray(lut, np.uint32)
    e = lut[raw]
    e[~inside] = 0
    bone = (e >> 31).astype(bool)
    m = e.copy()
    if ct is not None:
        m[bone] = (pad(ct) + np.uint32(ctOffset))[bone]
    stats = np.array([bone.sum(), m[bone].min() if bone.any() else -1, m[bone].max() if bone.any() else -1, 0, 0, -1, -1, 0], np.int64)
    if zWater >= 0:
        m[:, :, :zWater + 1] = 0
    kk = np.where(m > 0)[2]
    line = np.where(m[focalIJ[0], focalIJ[1], :] > 0)[0]
    stats[3:] = [(m > 0).sum(), m.max(), kk.min() if kk.size else -1, line.min() if line.size else -1, (m.astype(np.int64) >= nMaterials).sum()]
    return m, raw, (pad(air) if air is not None else np.zeros(N, np.uint32)), stats


# ---------------------------------------------------------------- the rays ----------------------------------------------------------------

def segment(count, center_region, away=False):
    """(beg, end) of a ray with `count` skull voxels. away: the planted fault, halves rounded away from zero"""
    rnd = (lambda x: np.floor(x + 0.5)) if away else np.round
    mid_idx = count // 2
    l_half = float(count) * center_region
    beg = np.max([0, int(rnd(mid_idx - l_half / 2))])
    end = np.min([count - 1, 1 + int(rnd(mid_idx + l_half / 2))])
    return int(beg), int(end)


def sdr_rays(ct_index, hu, box, step_i, step_j, min_skull_voxels=3, center_region=0.5, flip_k=True, away=False):
    """(value, count, state) of bfd_sdr_rays3d: the loop over rays"""
    D = driver(np.asarray(ct_index), flip_k)
    lo, hi = ((0, 0, 0), D.shape) if box is None else box
    sub = D[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    hu = np.asarray(hu)
    rows, cols = -(-sub.shape[0] // step_i), -(-sub.shape[1] // step_j)
    value, count, state = np.zeros((rows, cols), hu.dtype), np.zeros((rows, cols), np.int32), np.zeros((rows, cols), np.uint8)
    for r in range(rows):
        for c in range(cols):
            ray = sub[r * step_i, c * step_j, :].astype(np.int64)
            skull_indices = np.where(ray > 0)[0]
            count[r, c] = skull_indices.size
            if np.any(ray >= hu.size):
                state[r, c] = 4
                continue
            if skull_indices.size < min_skull_voxels:
                continue
            ray_hu = hu[ray]
            beg, end = segment(skull_indices.size, center_region, away)
            centre = ray_hu[skull_indices[beg]:skull_indices[end]]
            if beg >= end or centre.size == 0:
                state[r, c] = 3
                continue
            hu_max = ray_hu[skull_indices].max()
            if hu_max > 0:
                state[r, c] = 1
                value[r, c] = centre.min() / hu_max
            else:
                state[r, c] = 2
    return value, count, state


def sdr(ct_index, hu, pl, spacing_mm, ray_spacing_mm=1.8, min_skull_voxels=3, center_region=0.5):
    """The skull density ratio as the driver forms it: the crop, HU = hu[index], the mean over the rays that counted"""
    step_i = max(1, int(round(ray_spacing_mm / spacing_mm)))
    value, _, state = sdr_rays(ct_index, hu, (pl.box_lo, pl.box_hi), step_i, step_i, min_skull_voxels, center_region, pl.flip_k)
    values = [value[r, c] for r in range(value.shape[0]) for c in range(value.shape[1]) if state[r, c] == 1]
    return np.mean(values) if values else float('nan')


# ---------------------------------------------------------------- phantoms ----------------------------------------------------------------

def head(shape, segmented=False, flipped=True):
    """The label volume of the golden cases, as stored: nested spheres about (M1/2, M2/2, 0.9 M3) of radius R = 0.75 M3, shells of labels 1, 2, 3, 2, 4
    at R, R - 3, R - 5, R - 8, R - 10 (with `segmented` 6, 7, 8 inside R - 14, R - 18, R - 22), 5 at (M1 // 2, M2 // 2, int(0.55 M3))."""
    M1, M2, M3 = shape
    x, y, z = np.meshgrid(np.arange(M1) - M1 / 2, np.arange(M2) - M2 / 2, np.arange(M3) - 0.9 * M3, indexing='ij')
    d = np.sqrt(x * x + y * y + z * z)
    R = 0.75 * M3
    m = np.zeros(shape, np.uint8)
    shells = [(R, 1), (R - 3, 2), (R - 5, 3), (R - 8, 2), (R - 10, 4)] + ([(R - 14, 6), (R - 18, 7), (R - 22, 8)] if segmented else [])
    for radius, label in shells:
        m[d <= radius] = label
    m[M1 // 2, M2 // 2, int(0.55 * M3)] = 5
    return np.ascontiguousarray(np.flip(m, 2)) if flipped else m


def ct_for(labels, n_hu, seed=0, dtype=np.uint32):
    """A CT index volume for a stored label volume: 1 .. n_hu - 1 under the bone and at a few voxels beside it, 0 elsewhere; and an air mask"""
    rng = np.random.default_rng(seed)
    bone = (labels == 2) | (labels == 3)
    ct = np.zeros(labels.shape, dtype)
    ct[bone] = rng.integers(1, n_hu, int(bone.sum()))
    extra = (labels == 1) & (rng.random(labels.shape) < 0.02)
    ct[extra] = rng.integers(1, n_hu, int(extra.sum()))
    air = ((labels == 4) & (rng.random(labels.shape) < 0.01)).astype(np.uint8)
    return ct, air
