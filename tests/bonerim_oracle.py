"""The bone-rim partial-volume correction of BabelBrain/BabelDatasetPreps.py:935-1017 (bMaximizeBoneRim), restated literally in numpy and scipy for the
tests of babelbrain_amd.BoneRim: the statements of the reference in their order and in their types, each with its line. `correct` returns the
corrected CT, the fields and the eight statistics of bfd_bone_rim_correct3d (include/babelfdtd.h). `fault` plants one deviation, for the tests that
show each of them changes the result. The phantom of the tests is here too."""
import numpy as np
from scipy import ndimage

STAT_NAMES = ('bone', 'interior', 'dense', 'edge', 'global_mean_voxels', 'clipped', 'changed', 'max_d2')
FAULTS = ('no_clip', 'bone_for_eroded', 'float32_weights', 'scale_is_box0', 'local_mean_float64', 'sigma_of_axis_2')


def odd_box(ratio):
    """:942-946"""
    RatioCTVoxels = [int(r) for r in ratio]
    for ntr in range(len(RatioCTVoxels)):
        if RatioCTVoxels[ntr] % 2 == 0:
            RatioCTVoxels[ntr] += 1
        if RatioCTVoxels[ntr] == 1:
            RatioCTVoxels[ntr] = 3
    return RatioCTVoxels


def numpy_mean(ct, interior_high_th=800.0):
    """:951 and :957: numpy's own pairwise float32 mean, a float32 scalar"""
    return ct[ct >= interior_high_th].mean()


def exact_mean(ct, interior_high_th=800.0):
    """float32(double(S) / (16384.0 * count)) with S = the sum of ct * 2^14 over the dense voxels in Python integers: what the device forms"""
    vals = ct[ct >= interior_high_th]
    fixed = vals.astype(np.float64) * 16384.0
    assert np.array_equal(fixed, np.rint(fixed)) and vals.size
    S = sum(int(v) for v in fixed)
    return np.float32(float(S) / (16384.0 * vals.size))


def correct(ct, bone, ratio, interior_high_th=800.0, max_boost=1000.0, floor=None, global_mean=None, filtered=None, fault=None):
    """(corrected CT float32, fields dict, stats dict). ct is left as it was. global_mean None: numpy's own mean. filtered: (bi, bm) to take in place
    of scipy's two filters (the device's own fields)."""
    assert ct.dtype == np.float32 and fault in (None,) + FAULTS
    ndataCT = ct.copy()
    nfct = np.asarray(bone) != 0
    if floor is not None:                                                       # :931-933
        CTBone = ndataCT[nfct]
        CTBone[CTBone < floor] = floor
        ndataCT[nfct] = CTBone
    before = ndataCT.copy()
    RatioCTVoxels = odd_box(ratio)                                              # :942-946
    interior_mask = nfct.copy().astype(np.uint8)                                # :948
    interior_mask_val = (ndataCT >= interior_high_th)                           # :951
    if fault != 'bone_for_eroded':
        interior_mask = ndimage.binary_erosion(interior_mask, structure=np.ones(RatioCTVoxels), iterations=1)      # :953
    global_interior_mean = ndataCT[interior_mask_val].mean() if global_mean is None else np.float32(global_mean)   # :957
    assert global_interior_mean.dtype == np.float32
    inv_interior = 1 - interior_mask                                            # :964
    dist_to_interior = ndimage.distance_transform_edt(inv_interior)             # :967
    edge_voxels = (nfct == 1) & (interior_mask == 0)                            # :970
    distance_scale = float(RatioCTVoxels[0]) / 2.0                              # :974
    if fault == 'scale_is_box0':
        distance_scale = float(RatioCTVoxels[0])
    dist = dist_to_interior[edge_voxels]                                        # :975
    weights = np.exp(-dist / distance_scale)                                    # :976
    if fault == 'float32_weights':
        weights = np.exp(-dist.astype(np.float32) / np.float32(distance_scale))
    interior_f = ndataCT * interior_mask_val                                    # :980
    assert interior_f.dtype == np.float32
    sigma_local = RatioCTVoxels[2 if fault == 'sigma_of_axis_2' else 0]         # :982
    if filtered is None:
        blur_interior = ndimage.gaussian_filter(interior_f, sigma=sigma_local)  # :984
        blur_mask = ndimage.gaussian_filter(interior_mask_val.astype(np.float32), sigma=sigma_local)               # :986
    else:
        blur_interior, blur_mask = filtered
    assert blur_interior.dtype == np.float32 and blur_mask.dtype == np.float32
    with np.errstate(invalid='ignore', divide='ignore'):
        if fault == 'local_mean_float64':
            local_interior_mean_img = np.where(blur_mask.astype(np.float64) > 1e-6, blur_interior.astype(np.float64) / blur_mask.astype(np.float64),
                                               global_interior_mean)
        else:
            local_interior_mean_img = np.where(blur_mask > 1e-6, blur_interior / blur_mask, global_interior_mean)  # :988
            assert local_interior_mean_img.dtype == np.float32
    local_means = local_interior_mean_img[edge_voxels]                          # :991
    orig_vals = ndataCT[edge_voxels]                                            # :994
    correct_vals = orig_vals + weights * (local_means - orig_vals)              # :995
    delta = correct_vals - orig_vals                                            # :998
    delta_clipped = delta if fault == 'no_clip' else np.clip(delta, a_min=None, a_max=max_boost)                   # :999
    correct_vals = orig_vals + delta_clipped                                    # :1000
    if fault not in ('float32_weights',):
        assert correct_vals.dtype == np.float64
    ndataCT[edge_voxels] = correct_vals                                         # :1010
    fields = dict(interior=interior_mask.astype(bool), d2=np.rint(dist_to_interior * dist_to_interior).astype(np.int32), bi=blur_interior, bm=blur_mask,
                  edge=edge_voxels, global_mean=global_interior_mean, lowered=int(np.count_nonzero(correct_vals < orig_vals)))
    stats = dict(bone=int(nfct.sum()), interior=int(np.count_nonzero(interior_mask)), dense=int(interior_mask_val.sum()), edge=int(edge_voxels.sum()),
                 global_mean_voxels=int(np.count_nonzero(~(blur_mask[edge_voxels] > np.float32(1e-6)))), clipped=int(np.count_nonzero(delta > max_boost)),
                 changed=int(np.count_nonzero(ndataCT.view(np.uint32) != before.view(np.uint32))),
                 max_d2=int(fields['d2'][edge_voxels].max()) if edge_voxels.any() else 0)
    return ndataCT, fields, stats


def phantom(shape=(40, 36, 70), seed=7):
    """(ct float32, bone bool): an ellipsoidal shell of bone, radii 0.62-0.95 of the semi-axes 18, 16, 33 about the centre; a dense core of
    1500 +- 300 HU at radii 0.70-0.87, 2700 +- 50 where k > 50; rim values of 450 +- 80, floored at 300; a detached 2 x 10 x 10 plate of 500 +- 30 HU
    in a corner, far from every dense voxel; soft tissue inside, air outside."""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(n) - (n - 1) / 2 for n in shape], indexing='ij')
    rad = np.sqrt((g[0] / 18.0) ** 2 + (g[1] / 16.0) ** 2 + (g[2] / 33.0) ** 2)
    k = np.broadcast_to(np.arange(shape[2]), shape)
    bone = (rad >= 0.62) & (rad < 0.95)
    core = (rad >= 0.70) & (rad < 0.87)
    ct = np.where(rad < 0.62, 40.0, -1000.0) + rng.normal(0, 5, shape)
    ct[bone] = np.maximum(rng.normal(450, 80, int(bone.sum())), 300.0)
    ct[core] = rng.normal(1500, 300, int(core.sum()))
    high = core & (k > 50)
    ct[high] = rng.normal(2700, 50, int(high.sum()))
    plate = np.zeros(shape, bool)
    plate[:2, :10, :10] = True
    ct[plate] = rng.normal(500, 30, int(plate.sum()))
    return ct.astype(np.float32), bone | plate
