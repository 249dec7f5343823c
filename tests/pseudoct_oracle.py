"""The numpy / scipy restatement of the reference's pseudo-CT (BabelBrain/CTZTEProcessing.py:553-621, :523-528, :476-477 and
BabelDatasetPreps.py:828), statement by statement in float64, for the tests of babelbrain_amd/PseudoCT.py. The volumes arrive as nibabel's
get_fdata hands them to the reference: float64. skimage.measure.label is restated by scipy.ndimage.label with the 3 x 3 x 3 structure (26
neighbours, the same raster numbering; LabelImage is held to both elsewhere), regionprops by np.bincount in label order, and the phantom the
host and the GPU tests share is built here."""
import numpy as np
import scipy.ndimage
from scipy import signal

PETRA = dict(slope=-2080.02235771, offset=2133.22867303)           # :509-512
ZTE = dict(slope=-2085.0, offset=2329.0)


def label(x):
    return scipy.ndimage.label(x, np.ones((3, 3, 3)))[0]


def integer_histogram(arrZTE):
    """:559-562: (hist_vals, edges)"""
    arrZTE = np.asarray(arrZTE, np.float64)
    if (arrZTE.max() - arrZTE.min()) > 2 ** 16 - 1:
        raise ValueError('The range of values in the ZTE file exceeds 2^16')
    edgesin = np.arange(int(arrZTE.min()), int(arrZTE.max()) + 2) - 0.5
    return np.histogram(arrZTE.flatten().astype(int), bins=edgesin)


def petra_normaliser(arrZTE, PetraMRIPeakDistance=50, PetraNPeaks=2):
    """:559-577: np.max(locs)"""
    hist_vals, edges = integer_histogram(arrZTE)
    bins = (edges[1:] + edges[:-1]) / 2
    bins = bins[1:]
    hist_vals = hist_vals[1:]
    PeakDistance = int(PetraMRIPeakDistance / np.mean(np.diff(bins)))
    pks, _ = signal.find_peaks(hist_vals, distance=PeakDistance)
    locs = bins[pks]
    pks = hist_vals[pks]
    ind = np.argsort(pks)
    ind = ind[::-1][:PetraNPeaks]
    pks = pks[ind]
    locs = locs[ind]
    return np.max(locs)


def zte_cutoff(arrZTE, arrMask, q=95, above=-500):
    """:588-591"""
    maskedZTE = np.asarray(arrZTE, np.float64).copy()
    maskedZTE[np.asarray(arrMask) == 0] = -1000
    return np.percentile(maskedZTE[maskedZTE > above].flatten(), q)


def masked_percentile(volume, mask, q, above):
    """what :588-591 select, for any threshold (the -1000 of the masked copy is below -500 only)"""
    v = np.asarray(volume, np.float64)
    return np.percentile(v[(np.asarray(mask) != 0) & (v > above)], q)


def uniform_histogram(volume, bins, above, inclusive=False):
    """:476-477 (inclusive) and BabelDatasetPreps.py:828"""
    v = np.asarray(volume, np.float64)
    return np.histogram(v[v >= above] if inclusive else v[v > above], bins=bins)


def charm_masks(charmdata):
    """:523-528"""
    arrSkin = charmdata > 0
    arrMask = (charmdata == 1) | (charmdata == 2) | (charmdata == 3) | (charmdata == 9)
    label_img = label(charmdata == 0)
    areas = np.bincount(label_img.ravel())[1:]
    regions = sorted(range(1, areas.size + 1), key=lambda d: areas[d - 1])
    arrCavities = (label_img != 0) & (label_img != regions[-1])
    return arrSkin, arrMask, arrCavities


def convert(arrZTE, arrHead, arrSkin, arrCavities, arrMask=None, bIsPetra=False, pseudo_CT_range=(0.1, 0.6), slope=None, offset=None,
            PetraMRIPeakDistance=50, PetraNPeaks=2, erode=True, close=True, cavities=True, first_tie=True, hu_from_gauss=False):
    """:553-621: (arrCT, parts). The last five switches are not the reference's: each leaves out or swaps one step, for the tests that show the
    phantom gives that step work."""
    arrZTE = np.asarray(arrZTE, np.float64).copy()
    arrHead = np.asarray(arrHead).astype(np.float64)
    arrSkin, arrCavities = np.asarray(arrSkin).astype(np.float64), np.asarray(arrCavities).astype(np.float64)
    k = PETRA if bIsPetra else ZTE
    slope = k['slope'] if slope is None else slope
    offset = k['offset'] if offset is None else offset
    if bIsPetra:
        normaliser = petra_normaliser(arrZTE, PetraMRIPeakDistance, PetraNPeaks)
        arrZTE /= normaliser
    else:
        normaliser = cutoff = zte_cutoff(arrZTE, arrMask)
        arrZTE /= cutoff
        arrZTE[arrHead == 0] = -0.5

    arrGauss = arrZTE.copy()
    if erode:
        arrGauss[scipy.ndimage.binary_erosion(arrHead, iterations=3) == 0] = np.max(arrGauss)
    else:
        arrGauss[arrHead == 0] = np.max(arrGauss)
    maximum = np.max(arrGauss)
    arr = (arrGauss >= pseudo_CT_range[0]) & (arrGauss <= pseudo_CT_range[1])

    label_img = label(arr)
    pixelcount = np.bincount(label_img.ravel())[1:]
    props = sorted(range(1, pixelcount.size + 1), key=lambda d: pixelcount[d - 1], reverse=True)       # stable: among equals the lowest label first
    chosen = props[0] if first_tie else sorted(range(1, pixelcount.size + 1), key=lambda d: pixelcount[d - 1])[-1]
    before = label_img == chosen
    arr2 = (scipy.ndimage.binary_closing(before, structure=np.ones((11, 11, 11))) if close else before).astype(np.uint8)

    arrCT = np.zeros_like(arrGauss)
    arrCT[arrSkin == 0] = -1000
    arrCT[arrSkin != 0] = 42.0
    src = arrGauss if hu_from_gauss else arrZTE
    arrCT[arr2 != 0] = slope * src[arr2 != 0] + offset
    arrCT[arrCT < -1000] = -1000
    arrCT[arrCT > 3300] = -1000
    if cavities:
        arrCT[arrCavities != 0] = -1000
    return arrCT, dict(normaliser=float(normaliser), candidates=arr, bone_before_closing=before, bone=arr2 != 0, maximum=float(maximum))


def candidates(values, divisor, head, eroded, lo, hi):
    """:577 / :592-597 from given parts: (mask, maximum)"""
    q = np.asarray(values, np.float64) / divisor
    if head is not None:
        q[np.asarray(head) == 0] = -0.5
    g = q.copy()
    g[np.asarray(eroded) == 0] = np.max(g)
    return (g >= lo) & (g <= hi), float(np.max(q))


def hounsfield(values, divisor, head, bone, skin, cavities, slope, offset):
    """:608-621 from given parts"""
    q = np.asarray(values, np.float64) / divisor
    if head is not None:
        q[np.asarray(head) == 0] = -0.5
    bone = np.asarray(bone) != 0
    ct = np.zeros_like(q)
    ct[np.asarray(skin) == 0] = -1000
    ct[np.asarray(skin) != 0] = 42.0
    ct[bone] = slope * q[bone] + offset
    ct[ct < -1000] = -1000
    ct[ct > 3300] = -1000
    ct[np.asarray(cavities) != 0] = -1000
    return ct


def hu_edge_quotients(slope, offset):
    """quotients whose HU lands exactly on -1000 and on 3300 and on the nearest values the expression reaches to either side of them"""
    out = []
    for target in (-1000.0, 3300.0):
        q0 = (target - offset) / slope
        cand = q0 + np.arange(-50, 51) * np.spacing(q0)
        hu = slope * cand + offset
        assert (hu == target).any() and (hu < target).any() and (hu > target).any(), target
        if slope == 1.0 and offset == 0.0:                             # the expression is exact: one ulp beyond is reached
            assert (hu == np.nextafter(target, np.inf)).any() and (hu == np.nextafter(target, -np.inf)).any()
        out.append(cand)
    return np.concatenate(out)


def phantom(shape=(40, 48, 70), petra=False, seed=0, dtype=np.float64):
    """Nested ellipsoids: skin, skull, brain. Returns dict(zte, head, skin, cavities, csf), masks in several dtypes. Planted so that every step of
    the flow has work (tests/test_pseudoct_host.py shows each):
      - the outermost voxels of the head read like bone (partial volume): only the erosion hides them behind the maximum;
      - a slab of soft-tissue signal in the mid-plane of j cuts the skull into two mirror halves of exactly equal size, the two largest components:
        the tie rule decides which becomes the bone region (the lower label is the half at low j);
      - two bone-range islands of equal size (two voxels each) in the scalp, outside the skull: candidates that the largest component drops;
      - in each half a sinus: air (3 x 3 x 5) whose core (1 x 1 x 3) the head mask leaves out. The erosion takes the core's surroundings out of
        the candidates, which leaves a hole through the skull that only the 11^3 closing fills; inside the filled hole the normalised volume and
        its copy with the maximum differ, and the air there would be called bone without the cavities."""
    rng = np.random.default_rng(seed)
    n1, n2, n3 = shape
    i, j, k = np.meshgrid(np.arange(n1), np.arange(n2), np.arange(n3), indexing='ij')
    ci, cj, ck = (n1 - 1) / 2, (n2 - 1) / 2, (n3 - 1) / 2
    r = np.sqrt(((i - ci) / (n1 / 2 - 2)) ** 2 + ((j - cj) / (n2 / 2 - 2)) ** 2 + ((k - ck) / (n3 / 2 - 2)) ** 2)
    head = r <= 1.0
    skull = (r > 0.55) & (r <= 0.72) & (np.abs(j - cj) > 2)
    # intensities in units of the soft-tissue level: soft tissue 1, bone 0.35, air 0.02
    level = np.full(shape, 0.02)
    level[head] = 1.0
    level[skull] = 0.35
    level[(r > 0.95) & head] = 0.4
    air = np.zeros(shape, bool)
    i0, k0 = n1 // 2, n3 // 2
    j0 = int(round(cj - 0.635 * (n2 / 2 - 2)))
    for jj in (j0, n2 - 1 - j0):
        air[i0 - 1:i0 + 2, jj - 1:jj + 2, k0 - 2:k0 + 3] = True
        head[i0, jj, k0 - 1:k0 + 2] = False
    level[air] = 0.02
    for kk in (6, n3 - 8):
        level[i0, n2 // 2, kk:kk + 2] = 0.3
    scale, sigma = (1800.0, 12.0) if petra else (950.0, 6.0)
    zte = level * scale + sigma * rng.standard_normal(shape)
    if petra:
        zte = np.round(zte)                           # PETRA volumes hold integers
        zte[r > 1.0] = np.round(np.abs(rng.standard_normal(shape)) * 20)[r > 1.0]
    csf = (r > 0.45) & (r <= 0.55)
    return dict(zte=zte.astype(dtype), head=head.astype(np.float32), skin=(r <= 1.0).astype(np.uint8), cavities=air.astype(np.float64), csf=csf)
