"""The bone-rim correction as one device call (bfd_bone_rim_correct3d behind babelbrain_amd.BoneRim) against the literal numpy / scipy flow of
tests/bonerim_oracle.py.

The oracle's two filters are scipy's. The device filter has differed from scipy's float32 result on no element so far, but it is only BOUNDED against
scipy (tests/test_distance_gpu.py). So the comparison with the plain oracle asserts this: every element of the corrected CT that differs from the
oracle's lies where the device's bi or bm differs from scipy's float32 field (the count is printed; 0 is expected), and the statistics are equal.
With the device's own bi and bm fed into the oracle's blend, equality holds with no exception (tests.util.assert_same)."""
import numpy as np
import pytest
from scipy import ndimage

from babelbrain_amd import BinaryClosing as BC, BoneRim as BR, DistanceTransform as DT, GaussianFilter as GF, TissueMask as TM, _engine
from tests import bonerim_calls as TC, bonerim_oracle as BO, tissue_oracle as TO
from tests.util import assert_same

pytestmark = pytest.mark.gpu

F32 = np.float32
_cache = {}


def head():
    if 'head' not in _cache:
        _cache['head'] = BO.phantom()
    return _cache['head']


def oracle(key, ct, bone, ratio, floor, mean='numpy'):
    """the oracle's flow, computed once per case and left unchanged"""
    k = (key, tuple(ratio), floor, mean)
    if k not in _cache:
        gm = None
        if mean == 'exact':
            c = ct.copy()
            if floor is not None:
                b = np.asarray(bone) != 0
                c[b & (c < floor)] = floor
            gm = BO.exact_mean(c)
        _cache[k] = BO.correct(ct, bone, ratio, floor=floor, global_mean=gm)
        for a in (_cache[k][0],) + tuple(v for v in _cache[k][1].values() if isinstance(v, np.ndarray)):
            a.flags.writeable = False
    return _cache[k]


def check_against_oracle(key, ct, bone, ratio, floor=None, inplace=False, mean='numpy'):
    ref, rf, rstats = oracle(key, ct, bone, ratio, floor, mean)
    given = ct.copy()
    mask = bone.copy()
    out, f = BR.maximize_bone_rim(given, mask, list(ratio), floor=floor, global_mean=rf['global_mean'] if mean == 'numpy' else None, inplace=inplace,
                                  return_fields=True)
    assert (out is given) == bool(inplace) and out.dtype == np.float32 and out.shape == ct.shape
    if not inplace:
        assert given.tobytes() == ct.tobytes()
    assert mask.tobytes() == bone.tobytes() and BR.last_kernel_ms > 0
    if mean == 'exact':
        assert f['global_mean'].dtype == np.float32 and f['global_mean'] == rf['global_mean'] == BR.last_global_mean
    assert np.array_equal(f['interior'], rf['interior']) and np.array_equal(f['d2'], rf['d2'])
    filters_differ = (f['bi'] != rf['bi']) | (f['bm'] != rf['bm'])
    print('%s %s floor %s: %d elements of bi or bm differ from scipy in float32 (0 expected); %s' % (key, tuple(ratio), floor, int(filters_differ.sum()), BR.last_stats))
    assert not np.any((out != ref) & ~filters_differ)
    assert BR.last_stats == rstats
    # with the device's own fields in the oracle's blend: equality, no exception
    own, _, ostats = BO.correct(ct, bone, ratio, floor=floor, global_mean=rf['global_mean'], filtered=(f['bi'], f['bm']))
    assert_same(out, own, 'corrected CT, %s %s' % (key, tuple(ratio)))
    assert np.array_equal(out.view(np.uint32), own.view(np.uint32)) and BR.last_stats == ostats
    return out, f


@pytest.mark.parametrize('inplace', [False, True])
@pytest.mark.parametrize('floor', [None, 300.0, 450.0])
@pytest.mark.parametrize('ratio', [(3, 3, 3), (2, 2, 4), (5, 5, 3), (7, 3, 5)])
def test_phantom_equals_the_oracle_with_numpy_s_mean(ratio, floor, inplace):
    ct, bone = head()
    check_against_oracle('head', ct, bone, ratio, floor, inplace)
    if floor == 450.0:
        assert np.count_nonzero(bone & (ct < floor)) > 0            # this floor raises voxels of the phantom


def slab(N3, seed):
    rng = np.random.default_rng(seed)
    shape = (9, 7, N3)
    bone = np.zeros(shape, bool)
    bone[1:8, 1:6, :] = True
    ct = rng.normal(0, 5, shape)
    ct[bone] = np.maximum(rng.normal(1100, 400, int(bone.sum())), 300.0)
    return ct.astype(F32), bone


@pytest.mark.parametrize('N3', [1, 2, 63, 64, 65, 127, 128, 129, 130])
def test_rows_along_k_across_the_word_and_wave_boundaries(N3):
    ct, bone = slab(N3, N3)
    if N3 < 3:                                                      # the erosion along k, border value 0, leaves nothing: the refusal
        assert BO.correct(ct, bone, (3, 3, 3))[2]['interior'] == 0
        with pytest.raises(ValueError, match='interior'):
            BR.maximize_bone_rim(ct, bone, [3, 3, 3])
        return
    for ratio in ((3, 3, 3), (2, 2, 4)):
        out, f = check_against_oracle('slab%d' % N3, ct, bone, ratio)
        assert BR.last_stats['edge'] > 0 and BR.last_stats['interior'] > 0
    # bone up to the last voxel of a row and a lone voxel at the far end of every row
    bone2 = bone.copy()
    bone2[:, :, -1] = True
    check_against_oracle('slab%d-end' % N3, ct, bone2, (3, 3, 3))


@pytest.mark.parametrize('seed', [7, 8])
def test_mean_on_the_device_is_the_exact_mean(seed):
    ct, bone = BO.phantom(seed=seed)
    check_against_oracle('head%d' % seed, ct, bone, (3, 3, 3), mean='exact')
    print('seed %d: exact mean %r, numpy mean %r; global-mean voxels %d' % (seed, BR.last_global_mean, BO.numpy_mean(ct), BR.last_stats['global_mean_voxels']))
    assert BR.last_stats['global_mean_voxels'] > 0
    check_against_oracle('head%d' % seed, ct, bone, (2, 2, 4), floor=450.0, mean='exact')


def test_fields_equal_the_single_stages():
    ct, bone = head()
    for ratio in ((3, 3, 3), (2, 2, 4), (7, 3, 5)):
        box = BR.odd_box(ratio)
        _, f = BR.maximize_bone_rim(ct, bone, list(ratio), return_fields=True)
        interior = BC.BinaryErode(bone, np.ones(box))
        assert np.array_equal(f['interior'], interior.astype(bool))
        assert np.array_equal(f['interior'], ndimage.binary_erosion(bone, structure=np.ones(box)))
        assert np.array_equal(f['d2'], DT.distance_transform_edt(interior, invert=True, squared=True))
        dense = ct >= 800.0
        bi, bm = GF.gaussian_filter(ct * dense, float(box[0])), GF.gaussian_filter(dense.astype(F32), float(box[0]))
        assert f['bi'].tobytes() == bi.tobytes() and f['bm'].tobytes() == bm.tobytes()


def refused(lib, c, word):
    assert c.run(lib) == -1
    text = lib.bfd_last_error().decode()
    assert text.startswith(TC.ENTRY + ': ' + BR.DATA_REFUSED) and word in text, text
    assert c.untouched(but_ms=True) and c.ms[0] == 0.0, text


def test_data_refusals_write_nothing():
    lib = _engine.load_library()
    c = TC.Case(N=(0, 6, 9))
    refused(lib, c, 'empty')
    for bad in (np.nan, np.inf, -np.inf):
        c = TC.Case()
        c.ct[3, 3, 3] = bad
        refused(lib, c, 'not finite')
    c = TC.Case()
    c.ct[0, 0, 0] = 131072.0                                        # outside the bone, but dense
    refused(lib, c, '2^17')
    c = TC.Case()
    c.ct[3, 3, 4] = np.nextafter(F32(131072), F32(0))               # the largest value the sum takes
    assert c.run(lib) == 0
    c = TC.Case()
    c.ct[...] = np.minimum(c.ct, F32(700.0))
    refused(lib, c, 'global mean')
    c = TC.Case(given=1, mean=F32(1500.0))                          # with a mean given, no dense voxel is no refusal
    c.ct[...] = np.minimum(c.ct, F32(700.0))
    assert c.run(lib) == 0 and c.outputs['stats'][2] == 0 and c.outputs['globalMean'][0] == F32(1500.0) and c.ms[0] > 0
    c = TC.Case()
    c.bone[...] = 0
    c.bone[1:3, 1:5, 1:8] = 1                                       # two planes: a box of 3 leaves nothing
    refused(lib, c, 'interior')
    # several at once: the first of the header's order
    c = TC.Case()
    c.bone[...] = 0
    c.ct[0, 0, 0] = np.nan
    c.ct[0, 0, 1] = 2.0e5
    refused(lib, c, 'not finite')
    c = TC.Case()
    assert c.run(lib, device=lib.bfd_device_count()) == -3 and c.untouched()
    c = TC.Case()
    assert c.run(lib) == 0 and c.ms[0] > 0 and not c.untouched(but_ms=True)
    ct, bone = head()
    with pytest.raises(ValueError, match='refused data'):
        BR.maximize_bone_rim(np.where(bone, F32(np.nan), ct), bone, [3, 3, 3])


def test_volume_beyond_one_sweep_of_the_new_kernels():
    rng = np.random.default_rng(12)
    ct, bone = BO.phantom(shape=(70, 90, 100), seed=12)
    assert ct.size > BR.SWEEP_VOXELS and ct.shape[0] * ct.shape[1] * ((ct.shape[2] + 63) // 64) * 64 > BR.SWEEP_VOXELS
    # a block of bone with dense values that lies wholly beyond the first sweep (rows from i = 46 on), beside the shell in the middle
    far = np.zeros(ct.shape, bool)
    far[50:66, 20:80, 30:90] = True
    ct[far] = np.maximum(rng.normal(1200, 500, int(far.sum())), 300.0).astype(F32)
    bone = bone | far
    check_against_oracle('large', ct, bone, (3, 3, 3))
    assert BR.last_stats['edge'] > 0
    check_against_oracle('large', ct, bone, (3, 3, 3), mean='exact')


def test_two_runs_give_the_same_bytes():
    ct, bone = head()
    a, fa = BR.maximize_bone_rim(ct, bone, [2, 2, 4], floor=450.0, return_fields=True)
    sa = dict(BR.last_stats)
    b, fb = BR.maximize_bone_rim(ct, bone, [2, 2, 4], floor=450.0, return_fields=True)
    assert a.tobytes() == b.tobytes() and sa == BR.last_stats
    for name in ('interior', 'd2', 'bi', 'bm', 'global_mean'):
        assert fa[name].tobytes() == fb[name].tobytes(), name


def test_chain_with_the_quantisation():
    ct, bone = head()
    out, f = BR.maximize_bone_rim(ct, bone, [3, 3, 3], floor=300.0, global_mean=BO.numpy_mean(ct), return_fields=True)
    table, cmap, (mn, mx) = TM.quantize_values(out, bone, 10)
    host = BO.correct(ct, bone, (3, 3, 3), floor=300.0, filtered=(f['bi'], f['bm']))[0]
    _, want_table, want_map, (wmn, wmx) = TO.quantize(host, bone, 10)
    assert np.array_equal(table, want_table) and np.array_equal(cmap, want_map) and (mn, mx) == (wmn, wmx)
    ref = oracle('head', ct, bone, (3, 3, 3), 300.0)[0]
    print('chain: %d voxels of the corrected CT differ from the oracle with scipy filters (0 expected); %d levels' % (int(np.count_nonzero(out != ref)), table.size))
