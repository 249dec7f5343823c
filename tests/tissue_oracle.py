"""numpy restatements of the three tissue-mask definitions of include/babelfdtd.h (bfd_paint_components3d, bfd_quantize_values3d,
bfd_clear_beyond_bone3d) and of the flow TissueMask.finish_mask, for the host and the device tests. Written from the definitions; skimage's
regionprops(...).area is the bincount of the labels."""
import numpy as np
from scipy import ndimage


# ---------------------------------------------------------------- paint ----------------------------------------------------------------

def choose_labels(sizes, select):
    """(labels painted, label of the largest) from the sizes of labels 1..n, as
        regions = sorted(regionprops(label_img), key=lambda d: d.area)
    orders them: a stable sort of the labels by area, the last one the largest (among equals the highest label)."""
    sizes = np.asarray(sizes, np.int64)
    order = sorted(range(1, len(sizes) + 1), key=lambda l: sizes[l - 1])         # Python's sort is stable; regionprops lists by label
    largest = order[-1]
    if select == 0:
        return order[:-1], largest
    if select == 1:
        return [l for l in order[:-1] if int(sizes[l - 1]) < 0.1 * int(sizes[largest - 1])], largest
    return [largest], largest


def paint(volume, value, connectivity, select, fill):
    """(out, counts[4]) of bfd_paint_components3d"""
    volume = np.asarray(volume, np.uint8)
    lab, n = ndimage.label(volume == value, ndimage.generate_binary_structure(3, connectivity))
    out = volume.copy()
    if n == 0:
        return out, np.zeros(4, np.int64)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    painted, largest = choose_labels(sizes, select)
    sel = np.isin(lab, np.array(painted, np.int64)) if painted else np.zeros(lab.shape, bool)
    out[sel] = fill
    return out, np.array([n, sizes[largest - 1], len(painted), sel.sum()], np.int64)


# ---------------------------------------------------------------- quantise ----------------------------------------------------------------

def quantize_levels(x, mn, mx, bits):
    """(levels int64, values float32, s, r): the explicit float32 form, one rounding per operation"""
    x = np.asarray(x, np.float32)
    mn, mx = np.float32(mn), np.float32(mx)
    A = np.float32(mx - mn)
    M = np.float32(2 ** bits - 1)
    s, r = np.float32(M / A), np.float32(A / M)
    d = (x - mn).astype(np.float32)
    t = (s * d).astype(np.float32)
    lev = np.rint(t)
    return lev.astype(np.int64), level_values(lev, mn, r), s, r


def level_values(levels, mn, r):
    t = (np.float32(r) * np.asarray(levels).astype(np.float32)).astype(np.float32)
    return (t + np.float32(mn)).astype(np.float32)


def quantize(values, mask, bits):
    """(quantized, table, map, (mn, mx)) of bfd_quantize_values3d"""
    values = np.asarray(values, np.float32)
    sel = np.asarray(mask) != 0
    under = values[sel]
    mn, mx = under.min(), under.max()
    _, q, _, _ = quantize_levels(under, mn, mx, bits)
    quantized = values.copy()
    quantized[sel] = q
    table = np.unique(q)
    cmap = np.zeros(values.shape, np.uint32)
    cmap[sel] = np.searchsorted(table, q)
    return quantized, table, cmap, (mn, mx)


def quantize_literal(ndataCT, nfct, CT_quantification):
    """BabelDatasetPreps.py:1019-1027 in the reference's own words: (ndataCT after :1026, UniqueHU)"""
    ndataCT = ndataCT.copy()
    maxData = ndataCT[nfct].max()
    minData = ndataCT[nfct].min()
    A = maxData - minData
    M = 2 ** CT_quantification - 1
    ResStep = A / M
    qx = ResStep * np.round((M / A) * (ndataCT[nfct] - minData)) + minData
    ndataCT[nfct] = qx
    return ndataCT, np.unique(ndataCT[nfct])


# ---------------------------------------------------------------- cleanup ----------------------------------------------------------------

def clear_beyond_bone(volume, kFocal, boneA=2, boneB=3, from_value=4, to_value=1):
    """(out, counts[2]) of bfd_clear_beyond_bone3d, vectorised"""
    volume = np.asarray(volume, np.uint8)
    N3 = volume.shape[2]
    k = np.arange(N3)
    bone = ((volume == boneA) | (volume == boneB)) & (k > kFocal)
    kb = np.where(bone, k, -1).max(axis=2)                          # -1: no such bone on the line
    change = (kb[:, :, None] >= 0) & (k > kb[:, :, None]) & (volume == from_value)
    out = volume.copy()
    out[change] = to_value
    return out, np.array([(kb >= 0).sum(), change.sum()], np.int64)


def clear_beyond_bone_loop(FinalMask):
    """BabelDatasetPreps.py:1122-1133 in the reference's shape: the two flips and the double loop, the focal voxel found as the one that holds 5"""
    FinalMask = np.flip(FinalMask.copy(), axis=2)
    Rloc = np.array(np.where(FinalMask == 5)).flatten()
    for i in range(FinalMask.shape[0]):
        for j in range(FinalMask.shape[1]):
            Line = FinalMask[i, j, :Rloc[2]]
            bone = np.array(np.where((Line == 2) | (Line == 3))).flatten()
            if len(bone) > 0:
                subline = Line[:bone.min()]
                subline[subline == 4] = 1
                FinalMask[i, j, :len(subline)] = subline
    return np.flip(FinalMask, axis=2)


# ---------------------------------------------------------------- flow ----------------------------------------------------------------

def finish_mask_host(FinalMask, LocFocalPoint, TrabecularProportion=0.8, nfct=None, box_fov=False, cleanup_k=None):
    """(mask, erosion degree, the cleanup's counts or None): TissueMask.finish_mask with scipy and the restatements above in place of the device
    calls. cleanup_k plants a fault for the tests of the phantom: an index other than LocFocalPoint[2] for the cleanup, or -1 for no cleanup."""
    m = np.asarray(FinalMask, np.uint8).copy()
    loc = tuple(LocFocalPoint)
    counts = None
    if nfct is not None:
        m[m == 2] = 1
    m = ndimage.median_filter(m, 7)
    if nfct is not None:
        m[nfct] = 2
        m = paint(m, 1, 3, 1 if box_fov else 0, 4)[0]
    bone = m == 2
    degree = int(np.round(bone[loc[0], loc[1], loc[2]:].sum() * (1 - TrabecularProportion)))
    if degree != 0:
        m[ndimage.binary_erosion(bone, iterations=degree)] = 3
    else:
        m[bone] = 3
    m[loc] = 5
    if nfct is not None and cleanup_k != -1:
        m, counts = clear_beyond_bone(m, loc[2] if cleanup_k is None else cleanup_k)
    return m, degree, counts


def head_phantom(shape=(40, 44, 48), seed=0):
    """(FinalMask uint8, nfct bool, focal voxel): nested ellipsoids -- skin 1 down to radius 0.72, a bone shell 2 down to 0.55, brain 4 inside --
    made so that every step of the flow has something to do:
      - skin islands in the brain: small ones, and a box of 18 x 18 x 19 cut to the brain that is more than a tenth of the skin (box_fov keeps it);
      - a pocket of brain (4) in the skin layer above the skull, beyond the focal plane: the cleanup turns it into skin;
      - a hole in the upper skull over lines whose lower bone lies between k = 11 and 17: with the focal plane at 30 those lines have no bone
        beyond it and stay as they are, with a focal index of 14 (the focal voxel's i) or 0 their brain would become skin."""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[(np.arange(n) - (n - 1) / 2) / (n / 2) for n in shape], indexing='ij')
    rad = np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2)
    i, j, k = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')
    m = np.zeros(shape, np.uint8)
    m[rad < 0.95] = 1
    m[rad < 0.72] = 2
    m[rad < 0.55] = 4
    hole = (m == 2) & (i >= 7) & (i < 13) & (j >= 19) & (j < 25) & (k > shape[2] // 2)
    m[hole] = 4
    nfct = m == 2
    pocket = (m == 1) & (rad >= 0.72) & (i >= 20) & (i < 30) & (j >= 16) & (j < 28) & (k > shape[2] // 2)
    m[pocket] = 4
    big = m[16:34, 21:39, 5:24]                                      # the large island: what of the box lies in the brain
    big[big == 4] = 1
    for c in ((24, 8, 26), (27, 12, 14), (16, 30, 30)):
        e = [int(rng.integers(8, 11)) for _ in range(3)]
        sub = m[c[0]:c[0] + e[0], c[1]:c[1] + e[1], c[2]:c[2] + e[2]]
        sub[sub == 4] = 1
    return m, nfct, (14, 22, 30)
