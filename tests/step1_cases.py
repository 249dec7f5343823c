"""What tests/golden/make_step1_golden.py and the two tests of its fixtures (test_step1_golden_host.py, test_step1_golden_gpu.py) share: the cases of
each family, the inputs rebuilt from seeds with the phantoms of the oracles, the stand-ins for skimage's label and regionprops, the conformal
condition, the reading of tests/golden/step1_golden.npz + .json, and the few host statements that stand between two device calls of a flow
(`before_merge`: the stores of :904-907). The restatements of the stages are the oracles'; the expected results are the fixture's."""
import hashlib
import json
import os

import numpy as np
import scipy.ndimage

from tests import bonerim_oracle as BO, conformal_oracle as CO, pseudoct_oracle as PO, tissue_oracle as TO, voxelize_oracle as VO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TYPE_THRESHOLD = 300.0                  # HUThreshold's default, TypeThresold of the CT branch
REGION_AIR = (-1200, -400)              # RegionAirCT's default


# ---------------------------------------------------------------- skimage's two functions ----------------------------------------------------------------

def label(image):
    """skimage.measure.label(image) for a 3-D array: full connectivity (26 neighbours), labels numbered in raster order, int32 as skimage's."""
    return scipy.ndimage.label(np.asarray(image) != 0, np.ones((3, 3, 3)))[0].astype(np.int32)


class Region:
    """What the reference reads of a skimage RegionProperties: .label, .area, and r['name'] for an extra property."""

    def __init__(self, number, area, label_img, extra):
        self.label, self.area, self._img, self._extra = number, area, label_img, extra

    def __getitem__(self, name):
        if name in ('label', 'area'):
            return getattr(self, name)
        return self._extra[name](self._regionmask())

    def __getattr__(self, name):
        if name.startswith('_') or name not in self._extra:
            raise AttributeError(name)
        return self[name]

    def _regionmask(self):
        sl = scipy.ndimage.find_objects((self._img == self.label).astype(np.int32))[0]
        return self._img[sl] == self.label


def regionprops(label_img, extra_properties=()):
    """skimage.measure.regionprops(label_img): one Region per label that occurs, in ascending label order; area is the voxel count;
    extra_properties are functions of the region's bool mask (cut to its bounding box), looked up by their __name__."""
    label_img = np.asarray(label_img)
    counts = np.bincount(label_img.ravel())
    extra = {f.__name__: f for f in extra_properties}
    return [Region(n, int(counts[n]), label_img, extra) for n in range(1, counts.size) if counts[n]]


# ---------------------------------------------------------------- fixture ----------------------------------------------------------------

def sha1(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha1(('%s%r' % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def pack(mask):
    return np.packbits(np.asarray(mask) != 0)


def unpack(bits, shape):
    n = int(np.prod(shape))
    return np.unpackbits(bits)[:n].reshape(shape).astype(bool)


_loaded = {}


def golden():
    """(meta, arrays) of the fixture, read once"""
    if not _loaded:
        with open(os.path.join(GOLDEN, 'step1_golden.json')) as fh:
            _loaded['meta'] = json.load(fh)
        with np.load(os.path.join(GOLDEN, 'step1_golden.npz')) as z:
            _loaded['arrays'] = {k: z[k] for k in z.files}
    return _loaded['meta'], _loaded['arrays']


def case(family, name):
    """(record of the json, the case's arrays by their short names)"""
    meta, arrays = golden()
    prefix = '%s.%s.' % (family, name)
    return meta['families'][family][name], {k[len(prefix):]: v for k, v in arrays.items() if k.startswith(prefix)}


def same_major(meta):
    """True where this NumPy has the major version the fixture was made with: the condition of the comparisons whose types follow NumPy's
    promotion rules"""
    return np.__version__.split('.')[0] == meta['numpy'].split('.')[0]


def before_merge(inp, dilated):
    """FinalMask as the labelling of :909-913 finds it, from the conformal masks, the CT's bone and the dilated CSF (:904-907)"""
    m = inp['FinalMask'].astype(np.uint8)
    m[np.asarray(dilated) != 0] = 4
    m[inp['BinMaskConformalSkullRot'] == 1] = 4
    m[inp['nfct']] = 2
    return m


# ---------------------------------------------------------------- cases ----------------------------------------------------------------

PSEUDO_CT = {('%s_%s_%s' % (kind, dt, seg)): dict(petra=kind == 'petra', dtype=dt, simNIBS_type=seg, seed=3 + (kind == 'petra'), shape=(32, 36, 70))
             for kind in ('zte', 'petra') for dt in ('float32', 'float64') for seg in ('headreco', 'charm')}
BONE_MASK = {'zoom_1': dict(zooms=(1.0, 1.0, 1.0), seed=21, shape=(40, 36, 70)), 'zoom_uneven': dict(zooms=(1.25, 1.25, 1.7), seed=22, shape=(40, 36, 70))}
ISLANDS = {'all': dict(bApplyBOXFOV=False, seed=31, shape=(40, 44, 70)), 'box_fov': dict(bApplyBOXFOV=True, seed=31, shape=(40, 44, 70))}
BONE_RIM = {'box_3': dict(ratio=(2, 2, 2), seed=7, shape=(40, 36, 70)), 'box_5': dict(ratio=(4, 4, 4), seed=8, shape=(40, 36, 70)),
            'box_mixed': dict(ratio=(3, 3, 4), seed=9, shape=(40, 36, 70))}
QUANTIZE = {'bits_%d' % b: dict(CT_quantification=b, seed=40 + b, shape=(20, 18, 70)) for b in (1, 10, 16)}
AIR = {'two_pockets': dict(seed=51, shape=(40, 36, 70))}
FINISH = {'ct': dict(ct=True, bApplyBOXFOV=False, TrabecularProportion=0.8), 'ct_box_fov': dict(ct=True, bApplyBOXFOV=True, TrabecularProportion=0.8),
          'ct_degree_0': dict(ct=True, bApplyBOXFOV=False, TrabecularProportion=1.0), 'no_ct': dict(ct=False, bApplyBOXFOV=False, TrabecularProportion=0.5),
          'no_ct_degree_0': dict(ct=False, bApplyBOXFOV=True, TrabecularProportion=1.0)}
for _n, _c in FINISH.items():           # 70 along k crosses a 64-lane row; at 48 the phantom's large island is more than a tenth of the scalp
    _c.update(seed=0, shape=(40, 44, 48) if 'box_fov' in _n or _n == 'no_ct_degree_0' else (40, 44, 70))
CONFORMAL = {'rot_a': dict(rotation=61, step=1.0, location=(2.5, -1.0, 2.5)), 'rot_b': dict(rotation=64, step=0.8, location=(1.5, -2.0, 3.5)),
             'focal_outside': dict(rotation=63, step=1.0, location=(14.0, 3.0, 12.0))}
CONFORMAL_REFUSED = dict(rotation=73, step=1.0, location=(2.5, -1.0, 2.5))         # a rotation that fails conformal_condition: what the generator refuses
FAMILIES = dict(pseudo_ct=PSEUDO_CT, bone_mask=BONE_MASK, islands=ISLANDS, bone_rim=BONE_RIM, quantize=QUANTIZE, air=AIR, finish=FINISH, conformal=CONFORMAL)


# ---------------------------------------------------------------- inputs from seeds ----------------------------------------------------------------

def pseudo_ct_inputs(case):
    """The phantom of the pseudo-CT oracle; for charm also a final_tissues volume (4-D) whose labels give the phantom's masks another reading:
    0 outside the head and in the air, 5 skin, 7 skull, 1 / 2 / 3 / 9 in the csf shell and the brain."""
    p = PO.phantom(case['shape'], case['petra'], case['seed'], np.dtype(case['dtype']))
    if case['simNIBS_type'] == 'charm':
        shape = case['shape']
        n1, n2, n3 = shape
        i, j, k = np.meshgrid(np.arange(n1), np.arange(n2), np.arange(n3), indexing='ij')
        r = np.sqrt(((i - (n1 - 1) / 2) / (n1 / 2 - 2)) ** 2 + ((j - (n2 - 1) / 2) / (n2 / 2 - 2)) ** 2 + ((k - (n3 - 1) / 2) / (n3 / 2 - 2)) ** 2)
        charm = np.zeros(shape, np.float64)
        charm[r <= 1.0] = 5
        charm[(r > 0.55) & (r <= 0.72)] = 7
        charm[r <= 0.55] = 3
        charm[r <= 0.45] = np.where((i + j + k) % 3 == 0, 1, np.where((i + j + k) % 3 == 1, 2, 9))[r <= 0.45]
        charm[p['cavities'] != 0] = 0
        charm[n1 // 2, n2 // 2, 1] = 6                              # a lone voxel of tissue outside the head: skin, not csf
        p['charm'] = charm[:, :, :, None].repeat(2, axis=3)
        p['charm'][..., 1] = 0
    return p


def bone_mask_inputs(case):
    """ndataCT float32: the bone-rim phantom with salt (bone-like voxels anywhere) and pepper (soft voxels in the bone), so that the median, the
    closing and the choice of the largest component each have work (the detached plate is the second component)."""
    ct, bone = BO.phantom(case['shape'], case['seed'])
    rng = np.random.default_rng(case['seed'] + 1000)
    u = rng.random(ct.shape)
    ct = ct.copy()
    ct[u < 0.04] = np.float32(1200.0)
    ct[(u > 0.93) & bone] = np.float32(20.0)
    ct[1:10, 1:10, 1:12] = np.float32(-1000.0)
    ct[0:8, 0:8, 0:9] = np.float32(900.0)          # a block in the corner, outside the shell: its core survives the median and stays detached in the closing
    return dict(ndataCT=ct)


def nested(shape):
    g = np.meshgrid(*[(np.arange(n) - (n - 1) / 2) / (n / 2) for n in shape], indexing='ij')
    return np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2)


def islands_inputs(case):
    """The three conformal masks and the CT's bone mask of nested ellipsoids: the dilated CSF ends short of the skull, which leaves a closed shell
    of skin between them (more than a tenth of the scalp); pockets inside the CT bone that the skull mesh does not cover are small islands."""
    shape = case['shape']
    rad = nested(shape)
    rng = np.random.default_rng(case['seed'])
    skin = (rad < 0.95).astype(np.int8)
    csf = (rad < 0.22).astype(np.uint8)
    nfct = (rad >= 0.56) & (rad < 0.80)
    skull = ((rad >= 0.64) & (rad < 0.68)).astype(np.int8)
    enclosed = scipy.ndimage.binary_erosion(nfct, np.ones((3, 3, 3))) & (skull == 0)      # voxels whose 26 neighbours are all bone
    where = np.flatnonzero(enclosed)
    nfct.reshape(-1)[rng.choice(where, 8, replace=False)] = False
    return dict(FinalMask=skin, BinMaskConformalSkullRot=skull, BinMaskConformalCSFRot=csf, nfct=nfct)


def bone_rim_inputs(case):
    ct, bone = BO.phantom(case['shape'], case['seed'])
    return dict(ndataCT=ct, nfct=bone)


def quantize_inputs(case):
    ct, bone = BO.phantom(case['shape'], case['seed'])
    return dict(ndataCT=ct, nfct=bone)


def air_inputs(case):
    """ndataCTForAir float32: the bone-rim phantom (air outside the head) with two closed air pockets in the brain, one lone air voxel that the
    median removes, and a pocket of -500 HU, inside RegionAirCT's range though no air."""
    ct, _ = BO.phantom(case['shape'], case['seed'])
    ct = ct.copy()
    ct[15:20, 14:19, 30:36] = np.float32(-1000.0)
    ct[22:26, 16:22, 40:45] = np.float32(-950.0)
    ct[12, 20, 25] = np.float32(-1000.0)
    ct[18:21, 10:13, 20:23] = np.float32(-500.0)
    return dict(ndataCTForAir=ct)


def finish_inputs(case):
    m, nfct, loc = TO.head_phantom(case['shape'], case['seed'])
    return dict(FinalMask=m.astype(np.int8), nfct=nfct, LocFocalPoint=np.array(loc, np.int64))


CONFORMAL_CENTRE = (2.0, -1.5, 3.0)
CONFORMAL_RADII = ((6.5, 8.0, 5.5), (5.5, 6.5, 4.5), (4.0, 5.0, 3.5))           # skin, skull, csf


def conformal_inputs(case):
    """Three packed tables (bfd_voxelize_mesh's packing) of nested ellipsoids on grids of 0.75 * step about one centre, each with its own grid,
    origin and unit, and the float32 points the library derives from them."""
    unit = 0.75 * case['step']
    out = dict(tables=[], grids=[], origins=[], units=[], points=[], RMat=VO.rotation(case['rotation']))
    for n, radii in enumerate(CONFORMAL_RADII):
        lo = np.asarray(CONFORMAL_CENTRE) - np.asarray(radii) - 0.3 * (n + 1)
        grid = tuple(int(np.ceil((2 * r + 0.6 * (n + 1)) / unit)) for r in radii)
        idx = np.meshgrid(*[np.arange(g) for g in grid], indexing='ij')
        c = [lo[a] + (idx[a] + 0.5) * unit for a in range(3)]
        mask = sum(((c[a] - CONFORMAL_CENTRE[a]) / radii[a]) ** 2 for a in range(3)) <= 1.0
        table = VO.pack_table(mask)
        out['tables'].append(table)
        out['grids'].append(grid)
        out['origins'].append(tuple(float(v) for v in lo))
        out['units'].append((unit,) * 3)
        out['points'].append(CO.table_points(table, grid, lo, (unit,) * 3))
    return out


INPUTS = dict(pseudo_ct=pseudo_ct_inputs, bone_mask=bone_mask_inputs, islands=islands_inputs, bone_rim=bone_rim_inputs, quantize=quantize_inputs,
              air=air_inputs, finish=finish_inputs, conformal=conformal_inputs)


def inputs(family, name):
    return INPUTS[family](FAMILIES[family][name])


def input_hashes(d):
    """sha1 of every array (and of every array in a list) of an inputs dict"""
    out = {}
    for k, v in sorted(d.items()):
        if isinstance(v, np.ndarray):
            out[k] = sha1(v)
        elif isinstance(v, list) and v and isinstance(v[0], np.ndarray):
            out[k] = [sha1(a) for a in v]
    return out


# ---------------------------------------------------------------- the conformal condition ----------------------------------------------------------------

def conformal_margin(points, matrix32):
    """(smallest distance of a transformed coordinate from a half-integer, the bound at that coordinate's point): float64 on the CPU. The bound is
    the one tests/test_conformal_host.py derives for a float32 product in any order, 8 * 2^-24 * S with S = sum_b |m_ab x_b| + |m_a3|. A coordinate
    at least that far from every half-integer rounds to the same index under np.dot with any BLAS, under the element-wise float32 form and in
    float64; the upper filter's edge (index < M) is a comparison of those indices, so it is decided with them."""
    m64 = np.asarray(matrix32, np.float32)[:3].astype(np.float64)
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    t = p @ m64[:, :3].T + m64[:, 3]
    S = np.abs(p) @ np.abs(m64[:, :3]).T + np.abs(m64[:, 3])
    half = np.abs(t - np.floor(t) - 0.5)
    slack = half - 8 * 2.0 ** -24 * S
    at = np.unravel_index(np.argmin(slack), slack.shape)
    return float(half[at]), float(8 * 2.0 ** -24 * S[at])


def conformal_condition(inp, case):
    """True where both passes of :696-759 (the bare rotated affine, then the moved one) keep every point of the three lists and the focal point
    outside the bound of conformal_margin."""
    affine = np.eye(4)
    affine[:3, :3] = np.asarray(inp['RMat'], np.float64) * case['step']
    inv = np.linalg.inv(affine).astype(np.float32)
    half, bound = conformal_margin(inp['points'][0], inv)
    if half <= bound:
        return False
    first = np.round(inp['points'][0].astype(np.float64) @ inv[:3, :3].astype(np.float64).T + inv[:3, 3].astype(np.float64)).astype(np.int64)
    affine[:, 3] = affine @ np.array([first[:, 0].min(), first[:, 1].min(), first[:, 2].min(), 1.0])
    inv = np.linalg.inv(affine).astype(np.float32)
    everything = np.vstack(inp['points'] + [np.asarray(case['location'], np.float32).reshape(1, 3)])
    half, bound = conformal_margin(everything, inv)
    return half > bound
