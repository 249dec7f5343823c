"""numpy oracle of the 3-D median filter (tests/test_median_host.py holds it to scipy.ndimage.median_filter; the device tests compare with
it): pad ('symmetric' is scipy's 'reflect'), all windows, sort, element n // 2."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def sizes3(size):
    return (int(size),) * 3 if np.ndim(size) == 0 else tuple(int(v) for v in size)


def median_oracle(a, size, mode='reflect', cval=0):
    a = np.asarray(a)
    s = sizes3(size)
    pad = [(v // 2, v // 2) for v in s]
    if mode == 'reflect':
        p = np.pad(a, pad, mode='symmetric')
    else:
        p = np.pad(a, pad, mode='constant', constant_values=np.asarray(cval).astype(a.dtype))
    w = sliding_window_view(p, s).reshape(a.shape + (-1,))
    n = s[0] * s[1] * s[2]
    return np.ascontiguousarray(np.sort(w, axis=-1)[..., n // 2])


def median_oracle_block(a, size, lo, hi, mode='reflect', cval=0):
    """The oracle on the sub-block [lo, hi) of a large volume: evaluated on the block plus a halo of size // 2 cut from the volume (the
    volume's own boundary handling where the block touches a face), so that no window array of the whole volume is built."""
    s = sizes3(size)
    cut, keep = [], []
    for ax in range(3):
        r = s[ax] // 2
        b, e = max(lo[ax] - r, 0), min(hi[ax] + r, a.shape[ax])
        cut.append(slice(b, e))
        keep.append(slice(lo[ax] - b, lo[ax] - b + hi[ax] - lo[ax]))
    return np.ascontiguousarray(median_oracle(a[tuple(cut)], s, mode, cval)[tuple(keep)])
