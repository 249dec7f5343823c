"""The whole-volume steps of the pseudo-CT from ZTE / PETRA in the reference's BabelBrain/CTZTEProcessing.py (ConvertZTE_PETRA_pCT, :501-628) and of the
histograms its caller and GeneratePseudoCTHistogram take, on the device:

    InitPseudoCT(DeviceName, GPUBackend)
    integer_histogram(volume)                              :559-562: min, max, the 2^16 check, np.histogram of astype(int)
    petra_normaliser(volume, peak_distance, n_peaks)       :559-577: the histogram, find_peaks, the highest peaks, np.max(locs)
    masked_percentile(volume, mask, q, above)              :588-591: np.percentile of the brain without the masked copy and without a sort
    uniform_histogram(volume, bins, above, inclusive)      :476-477, BabelDatasetPreps.py:828: np.histogram(x[x > t], bins)
    charm_masks(charmdata)                                 :523-528: skin, csf and cavities from charm's final_tissues
    convert_pseudo_ct(zte, head, skin, cavities, csf, ...) :553-621, the flow around these, BinaryErode, largest_component and BinaryClose

The work runs on the MI355X through the C ABI (bfd_integer_histogram3d, bfd_order_statistics3d, bfd_uniform_histogram3d, bfd_pseudo_ct_candidates3d
and bfd_pseudo_ct_convert3d in csrc/bfd_pseudoct.hip, bfd_select_component3d in csrc/bfd_morphology.hip; definitions in include/babelfdtd.h);
there is no CPU fallback. Every result equals its numpy / scipy restatement in float64 (tests/pseudoct_oracle.py) element for element; a float32
volume is widened exactly first, as nibabel's get_fdata does. Argument errors are raised before the library is loaded."""
import contextlib
import ctypes as C
import math
import operator

import numpy as np

from . import BinaryClosing, LabelImage, TissueMask, _engine, _step1

_device = 0
last_kernel_ms = None
last_parts_ms = None               # convert_pseudo_ct's kernel milliseconds step by step
F32, F64 = 1, 3                    # the dtype codes of the C ABI
MAX_INT_BINS = 65536
MAX_BINS = 1024
# every data refusal of the five entries (rc -1 after the device pick) carries these words after the entry's name (csrc/bfd_pseudoct.hip,
# DATA_REFUSED; include/babelfdtd.h): they become ValueError with the library's text
DATA_REFUSED = 'refused data'
RANGE_REFUSED = 'The range of values in the ZTE file exceeds 2^16'          # the reference's text, :560
# voxels one sweep of a launch covers before its grid-stride loop turns (csrc/bfd_pseudoct.hip: blocks x threads x 4)
HIST_SWEEP_VOXELS = 512 * 512 * 4                  # HIST_BLOCKS x HIST_THREADS: the two histograms
SWEEP_VOXELS = 2048 * 256 * 4                      # SWEEP_BLOCKS x THREADS: every other kernel (the reductions: REDUCE_BLOCKS, half of it)
INT_WINDOW = 8192                                  # bins of the integer histogram counted in LDS; those beyond go to global memory
PETRA_SLOPE, PETRA_OFFSET = -2080.02235771, 2133.22867303                   # :509-512
ZTE_SLOPE, ZTE_OFFSET = -2085.0, 2329.0


def InitPseudoCT(DeviceName=None, GPUBackend=None):
    """Selects the HIP device by name substring, as InitMedianFilter does. convert_pseudo_ct and charm_masks run their BinaryClosing, LabelImage and
    TissueMask calls on this device too, without changing what those modules' own Init functions selected. GPUBackend is accepted and ignored."""
    global _device
    devs, _device = _step1.pick_device(DeviceName, _device)
    return devs


@contextlib.contextmanager
def _on_my_device(module):
    """A call of another drop-in on this module's device: its own selection is put back afterwards"""
    theirs = module._device
    module._device = _device
    try:
        yield
    finally:
        module._device = theirs


def _values(a, name):
    """(float32 or float64 volume, C-contiguous; its dtype code)"""
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        raise TypeError('%s must be float32 or float64, not %s' % (name, a.dtype))
    if a.ndim != 3:
        raise ValueError('%s must be a 3-D volume, not %d-D' % (name, a.ndim))
    if a.size >= 2 ** 31:
        raise ValueError('the volume has 2^31 voxels or more')
    return np.ascontiguousarray(a), (F64 if a.dtype == np.float64 else F32)


def _mask(m, shape, name):
    """a mask of any dtype as uint8 of 0 / 1: it is read as != 0"""
    m = np.asarray(m)
    if m.shape != shape:
        raise ValueError('%s has shape %r, the volume %r' % (name, m.shape, shape))
    if m.dtype == np.bool_:
        return np.ascontiguousarray(_step1.bool_as_uint8(m))
    return np.ascontiguousarray((m != 0).view(np.uint8))


def _call(entry, *args):
    """_step1.call with the data refusals of the entry as ValueError"""
    try:
        _step1.call(entry, *args)
    except _engine.EngineError as e:
        if '(rc=-1)' in str(e) and DATA_REFUSED in str(e):
            raise ValueError(RANGE_REFUSED if RANGE_REFUSED in str(e) else str(e)) from None
        raise


def integer_histogram(volume):
    """(counts, first, (min, max)): counts int64 [int(max) - int(min) + 1] equals
        np.histogram(volume.flatten().astype(int), bins=np.arange(int(min), int(max) + 2) - 0.5)[0]
    and first = int(min) is the integer of counts[0] (:559-562). astype(int) truncates toward zero, so the bin of 0 collects (-1, 1). ValueError with
    the reference's text where max - min > 2^16 - 1, and for a value that is not finite or an empty volume."""
    global last_kernel_ms
    v, code = _values(volume, 'volume')
    counts = np.empty(MAX_INT_BINS, np.int64)
    first, bins = C.c_int64(), C.c_int64()
    rng = np.zeros(2, np.float64)
    ms = C.c_float()
    _call('bfd_integer_histogram3d', _device, code, _engine._ptr(v), v.shape[0], v.shape[1], v.shape[2], _engine._ptr(counts), C.byref(first), C.byref(bins),
          _engine._ptr(rng), C.byref(ms))
    last_kernel_ms = ms.value
    return counts[:bins.value].copy(), int(first.value), (float(rng[0]), float(rng[1]))


def _local_maxima(x):
    """scipy.signal._peak_finding_utils._local_maxima_1d: the middle sample (rounded down) of every plateau that is higher than both of its
    neighbours; the first and the last sample are never peaks"""
    n = x.size
    if n < 3:
        return np.zeros(0, np.intp)
    # the runs of equal samples: start and last index of each
    starts = np.concatenate(([0], np.flatnonzero(x[1:] != x[:-1]) + 1))
    ends = np.concatenate((starts[1:] - 1, [n - 1]))
    h = x[starts]
    inner = np.arange(1, starts.size - 1)
    is_peak = (h[inner] > h[inner - 1]) & (h[inner] > h[inner + 1])
    return ((starts[inner][is_peak] + ends[inner][is_peak]) // 2).astype(np.intp)


def find_peaks(x, distance=None):
    """scipy.signal.find_peaks(x, distance=distance)[0], restated: the package has no scipy. Local maxima, then scipy's removal by priority: from the
    highest peak down, a peak that is still kept removes every peak closer than `distance` samples. The order among equal heights is that of the
    np.argsort call scipy makes."""
    x = np.asarray(x, dtype=np.float64, order='C')
    if x.ndim != 1:
        raise ValueError('`x` must be a 1-D array')
    if distance is not None and distance < 1:
        raise ValueError('`distance` must be greater or equal to 1')
    peaks = _local_maxima(x)
    if distance is None:
        return peaks
    d = math.ceil(distance)
    order = np.argsort(x[peaks])
    keep = np.ones(peaks.size, bool)
    for i in range(peaks.size - 1, -1, -1):
        j = order[i]
        if not keep[j]:
            continue
        k = j - 1
        while k >= 0 and peaks[j] - peaks[k] < d:
            keep[k] = False
            k -= 1
        k = j + 1
        while k < peaks.size and peaks[k] - peaks[j] < d:
            keep[k] = False
            k += 1
    return peaks[keep]


def _normaliser_from_histogram(counts, first, peak_distance, n_peaks):
    """:562-577 from the counts: (np.max(locs), bins, hist_vals)"""
    edges = np.arange(first, first + counts.size + 1) - 0.5
    bins = (edges[1:] + edges[:-1]) / 2
    bins = bins[1:]
    hist_vals = counts[1:]
    if bins.size < 2:
        raise ValueError('fewer than two bins remain after the first: there is no peak distance')
    PeakDistance = int(peak_distance / np.mean(np.diff(bins)))
    pks = find_peaks(hist_vals, distance=PeakDistance)
    if pks.size == 0:
        raise ValueError('the histogram has no peak')
    locs = bins[pks]
    pks = hist_vals[pks]
    ind = np.argsort(pks)
    ind = ind[::-1][:n_peaks]
    locs = locs[ind]
    if locs.size == 0:
        raise ValueError('n_peaks selects no peak')
    return float(np.max(locs))


def petra_normaliser(volume, peak_distance=50, n_peaks=2):
    """np.max(locs) of :563-577: the integer histogram without its first bin, find_peaks at distance int(peak_distance / np.mean(np.diff(bins))), the
    n_peaks highest through np.argsort(pks)[::-1][:n_peaks], the largest location among them. ValueError where fewer than two bins remain or no peak
    exists (the reference fails there with int(nan) or max of an empty array)."""
    counts, first, _ = integer_histogram(volume)
    return _normaliser_from_histogram(counts, first, peak_distance, operator.index(n_peaks))


def order_statistics(volume, mask=None, above=-np.inf, inclusive=False, ranks=None, q=None):
    """(n, ranks, values): the number of voxels with mask != 0 and volume > above (>= with inclusive), and the values at the given ranks (up to 4,
    0-based, in ascending order of value) or at the two ranks np.percentile(..., q) reads. Exact: a radix select on the device, no sort."""
    global last_kernel_ms
    v, code = _values(volume, 'volume')
    m = None if mask is None else _mask(mask, v.shape, 'mask')
    if (ranks is None) == (q is None):
        raise ValueError('give ranks or q, not both')
    if ranks is not None:
        rk = np.ascontiguousarray([operator.index(r) for r in ranks], np.int64)
        if not 1 <= rk.size <= 4:
            raise ValueError('1 to 4 ranks, not %d' % rk.size)
    else:
        rk = None
        if not 0 <= q <= 100:
            raise ValueError('Percentiles must be in the range [0, 100]')
    if math.isnan(above):
        raise ValueError('above is not a number')
    R = 2 if rk is None else rk.size
    n = C.c_int64()
    used = np.zeros(4, np.int64)
    stats = np.zeros(4, np.float64)
    ms = C.c_float()
    _call('bfd_order_statistics3d', _device, code, _engine._ptr(v), _engine._ptr(m), v.shape[0], v.shape[1], v.shape[2], float(above), int(bool(inclusive)),
          _engine._ptr(rk), 0 if rk is None else R, 0.0 if q is None else float(q), C.byref(n), _engine._ptr(used), _engine._ptr(stats), C.byref(ms))
    last_kernel_ms = ms.value
    return int(n.value), used[:R].copy(), stats[:R].copy()


def percentile_from_statistics(n, q, A, B):
    """np.percentile's linear interpolation between the order statistics A (rank lo) and B (rank min(lo + 1, n - 1)), as numpy forms it:
    A + (B - A) * g, and B - (B - A) * (1 - g) where g >= 0.5, with g = (n - 1) * (q / 100) - lo"""
    pos = (n - 1) * np.true_divide(q, 100)
    g = pos - np.floor(pos)
    A, B = np.float64(A), np.float64(B)
    d = B - A
    return np.float64(B - d * (1 - g)) if g >= 0.5 else np.float64(A + d * g)


def masked_percentile(volume, mask, q=95.0, above=-500.0):
    """np.percentile(volume[(mask != 0) & (volume > above)].astype(np.float64), q), which is what :588-591 compute. ValueError when nothing is
    selected."""
    n, _, s = order_statistics(volume, mask, above, q=q)
    return percentile_from_statistics(n, q, s[0], s[1])


def uniform_histogram(volume, bins, above, inclusive=False):
    """(counts int64 [bins], edges float64 [bins + 1]) equal to np.histogram(volume[volume > above], bins=bins); volume >= above with inclusive
    (:476-477; the > form is BabelDatasetPreps.py:828). bins: an int in 1 .. 1024. The edges are np.linspace(min, max, bins + 1) of the selected
    values, +-0.5 where they are equal, 0 .. 1 where nothing is selected, as numpy has it. ValueError for a selected value that is not finite."""
    global last_kernel_ms
    v, code = _values(volume, 'volume')
    try:
        nb = operator.index(bins)
    except TypeError:
        raise ValueError('bins must be an int in 1 .. %d, not %r' % (MAX_BINS, bins))
    if not 1 <= nb <= MAX_BINS:
        raise ValueError('bins must be an int in 1 .. %d, not %r' % (MAX_BINS, bins))
    if math.isnan(above):
        raise ValueError('above is not a number')
    shape = (v.shape[0], v.shape[1], v.shape[2])
    rng = np.zeros(2, np.float64)
    n = C.c_int64()
    ms1, ms2 = C.c_float(), C.c_float()
    _call('bfd_uniform_histogram3d', _device, code, _engine._ptr(v), *shape, float(above), int(bool(inclusive)), 0, None, None, _engine._ptr(rng),
          C.byref(n), C.byref(ms1))
    first, last = (float(rng[0]), float(rng[1])) if n.value else (0.0, 1.0)
    if first == last:
        first, last = first - 0.5, last + 0.5
    edges = np.linspace(first, last, nb + 1, endpoint=True, dtype=np.float64)
    counts = np.zeros(nb, np.int64)
    if n.value:
        _call('bfd_uniform_histogram3d', _device, code, _engine._ptr(v), *shape, float(above), int(bool(inclusive)), nb, _engine._ptr(edges),
              _engine._ptr(counts), None, None, C.byref(ms2))
    last_kernel_ms = ms1.value + ms2.value
    return counts, edges


def charm_masks(charmdata):
    """(skin, csf, cavities), bool, of :523-528: skin = charmdata > 0; csf = the labels 1, 2, 3 and 9; cavities = the components of charmdata == 0
    without the largest (among equals the highest label, TissueMask.drop_largest's rule and the reference's regions[-1])."""
    c = np.asarray(charmdata)
    if c.ndim != 3:
        raise ValueError('charmdata must be a 3-D volume, not %d-D' % c.ndim)
    skin = c > 0
    csf = (c == 1) | (c == 2) | (c == 3) | (c == 9)
    with _on_my_device(TissueMask):
        cavities = TissueMask.drop_largest(c == 0).view(np.bool_)
    return skin, csf, cavities


def candidates(zte, divisor, head, eroded, lo, hi):
    """(mask bool, maximum, count) of :577 / :592-597: g = zte / divisor (-0.5 where head == 0, with a head), g = np.max(g) where eroded == 0,
    mask = (g >= lo) & (g <= hi)."""
    global last_kernel_ms
    v, code = _values(zte, 'zte')
    h = None if head is None else _mask(head, v.shape, 'head')
    e = _mask(eroded, v.shape, 'eroded')
    divisor = float(divisor)
    if not math.isfinite(divisor) or divisor == 0.0:
        raise ValueError('the divisor must be finite and not zero, not %r' % divisor)
    out = np.empty(v.shape, np.uint8)
    mx = C.c_double()
    n = C.c_int64()
    ms = C.c_float()
    _call('bfd_pseudo_ct_candidates3d', _device, code, _engine._ptr(v), v.shape[0], v.shape[1], v.shape[2], divisor, _engine._ptr(h), _engine._ptr(e),
          float(lo), float(hi), _engine._ptr(out), C.byref(mx), C.byref(n), C.byref(ms))
    last_kernel_ms = ms.value
    return out.view(np.bool_), float(mx.value), int(n.value)


def hounsfield(zte, divisor, head, bone, skin, cavities, slope, offset, dtype=np.float64):
    """:608-621: -1000 or 42 by skin; slope * q + offset under the bone region, q = zte / divisor (-0.5 where head == 0, with a head); -1000 where
    that is < -1000 or > 3300; -1000 in the cavities. float64, one multiplication and one addition, each rounded; float32 rounds the result once."""
    global last_kernel_ms
    v, code = _values(zte, 'zte')
    dt = np.dtype(dtype)
    if dt not in (np.float32, np.float64):
        raise TypeError('dtype must be float32 or float64, not %s' % dt)
    h = None if head is None else _mask(head, v.shape, 'head')
    b, s, c = _mask(bone, v.shape, 'bone'), _mask(skin, v.shape, 'skin'), _mask(cavities, v.shape, 'cavities')
    divisor = float(divisor)
    if not math.isfinite(divisor) or divisor == 0.0:
        raise ValueError('the divisor must be finite and not zero, not %r' % divisor)
    out = np.empty(v.shape, dt)
    ms = C.c_float()
    _call('bfd_pseudo_ct_convert3d', _device, code, _engine._ptr(v), v.shape[0], v.shape[1], v.shape[2], divisor, _engine._ptr(h), _engine._ptr(b),
          _engine._ptr(s), _engine._ptr(c), float(slope), float(offset), F64 if dt == np.float64 else F32, _engine._ptr(out), C.byref(ms))
    last_kernel_ms = ms.value
    return out


def convert_pseudo_ct(zte, head, skin, cavities, csf=None, petra=False, pct_range=(0.1, 0.6), slope=None, offset=None, peak_distance=50, n_peaks=2,
                      dtype=np.float64, return_parts=False):
    """arrCT of CTZTEProcessing.py:553-621. zte: float32 or float64 volume (left as it was); head, skin, cavities, csf: masks of its shape, of any
    dtype, read as != 0 (csf is needed for ZTE alone). The normaliser is petra_normaliser(zte) for PETRA and masked_percentile(zte, csf) for ZTE;
    then the quotient, the head eroded three times, the candidate mask, its largest component (26 neighbours, among equals the lowest label), the
    11 x 11 x 11 closing and the HU values. slope, offset: None for the reference's defaults. With return_parts also a dict: normaliser,
    candidates, bone_before_closing, bone, maximum. ValueError for a normaliser that is not finite or not positive and for a candidate mask without
    a voxel (the reference fails at props[0])."""
    global last_kernel_ms, last_parts_ms
    v, _ = _values(zte, 'zte')
    dt = np.dtype(dtype)
    if dt not in (np.float32, np.float64):
        raise TypeError('dtype must be float32 or float64, not %s' % dt)
    h, s, c = _mask(head, v.shape, 'head'), _mask(skin, v.shape, 'skin'), _mask(cavities, v.shape, 'cavities')
    if len(pct_range) != 2:
        raise ValueError('pct_range must be two values, not %r' % (pct_range,))
    if not petra and csf is None:
        raise ValueError('the ZTE conversion needs the csf mask')
    if slope is None:
        slope = PETRA_SLOPE if petra else ZTE_SLOPE
    if offset is None:
        offset = PETRA_OFFSET if petra else ZTE_OFFSET
    parts = {}
    if petra:
        norm = petra_normaliser(v, peak_distance, n_peaks)
    else:
        norm = float(masked_percentile(v, _mask(csf, v.shape, 'csf')))
    parts['normaliser'] = last_kernel_ms
    if not math.isfinite(norm) or norm <= 0.0:
        raise ValueError('the normaliser is %r: it must be finite and positive' % norm)
    quotient_head = None if petra else h
    with _on_my_device(BinaryClosing):
        eroded = BinaryClosing.BinaryErode(h.view(np.bool_), iterations=3)
        parts['erosion'] = BinaryClosing.last_kernel_ms
    cand, maximum, count = candidates(v, norm, quotient_head, eroded, pct_range[0], pct_range[1])
    parts['candidates'] = last_kernel_ms
    if count == 0:
        raise ValueError('no voxel of the normalised volume lies in %r: there is no bone region' % (tuple(pct_range),))
    with _on_my_device(LabelImage):
        before = LabelImage.largest_component(cand, connectivity=3, ties='first')
        parts['largest_component'] = LabelImage.last_kernel_ms
    with _on_my_device(BinaryClosing):
        bone = BinaryClosing.BinaryClose(before, np.ones((11, 11, 11)))
        parts['closing'] = BinaryClosing.last_kernel_ms
    out = hounsfield(v, norm, quotient_head, bone, s, c, slope, offset, dt)
    parts['hounsfield'] = last_kernel_ms
    last_parts_ms = parts
    last_kernel_ms = sum(parts.values())
    if return_parts:
        return out, dict(normaliser=norm, candidates=cand, bone_before_closing=before, bone=bone, maximum=maximum)
    return out
