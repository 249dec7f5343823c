"""The Step-3 exposure analysis without a GPU: the numpy restatement (tests/thermal_oracle.py) against the golden made from the reference's own
statements, by equality; planted faults the golden comparison must report; bfd_thermal_core.h, compiled for the host, against numpy (terms bit for
bit, the pair comparison on ties, +-0 and negatives); numpy's own plane sums against math.fsum within the bound the device sums are held to; the host
side of babelbrain_amd/ThermalAnalysis.py (tables, scalar lines, monitoring points) against the restatement and the golden."""
import hashlib
import inspect
import json
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from babelbrain_amd import ThermalAnalysis as TA, _engine
from tests import thermal_oracle as TO

HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, 'golden', 'thermal_analysis_golden.json')))
GOLD = np.load(os.path.join(HERE, 'golden', 'thermal_analysis_golden.npz'))
CASES = sorted(META['cases'])
U = 2.0 ** -53


def sum_bound(n, exact):
    """Higham's bound for any order of summing n non-negative float64 terms: (n - 1) u / (1 - (n - 1) u) * the exact sum"""
    g = (n - 1) * U
    return g / (1 - g) * exact


def numbers(args):
    return [float(a) for a in args if not isinstance(a, str)]


def flags_of(rec):
    b = rec['build']
    return dict(ct=bool(b.get('ct')), segmented=bool(b.get('segmented')), homogeneous=bool(b.get('homogeneous')), benchmark=b.get('benchmark'))


def same_scalar(got, want):
    return float(got) == want['value'] and np.asarray(got).dtype.name == want['dtype']


def run_restatement(mod, name):
    """What the restatement `mod` gives for a golden case, in the golden's own form"""
    rec = META['cases'][name]
    case = mod.build_case(tuple(META['shape']), **rec['build'])
    f = flags_of(rec)
    SelBrain, SelSkin, SelSkull, BrainID, IdRegionBenchmark = mod.selections(case['MaterialMap'], f['ct'], f['segmented'], f['homogeneous'], f['benchmark'])
    reports = []
    water = case['pAmpWater'].copy()
    call = rec['call']
    PressureRatio, RatioLosses = mod.AnalyzeLosses(case['pAmp'], case['MaterialMap'], case['LocIJK'], case['Input'], case['MaterialList'], water, call['Isppa'],
                                                   case['xf'], case['yf'], case['zf'], SelBrain, f['homogeneous'], f['segmented'], call['TxSystem'],
                                                   IdRegionBenchmark, FixedAcousticPower=call['FixedAcousticPower'],
                                                   report=lambda *a: reports.append([a[0].split('\n')[0]] + numbers(a[1:])))
    mp, mSkin, mBrain, mSkull = mod.monitoring_points_map(case['ResTemp'], SelSkin, SelBrain, SelSkull, case['LocIJK'], f['homogeneous'], f['benchmark'])
    met = mod.exposure_metrics(case['ResTemp'], case['FinalDose'], case['pAmp'] * PressureRatio, SelBrain, SelSkin, SelSkull, case['MaterialList'], BrainID,
                               call['Frequency'], call['DutyCycle'], call['Isppa'])
    return dict(case=case, SelBrain=SelBrain, SelSkin=SelSkin, SelSkull=SelSkull, BrainID=BrainID, IdRegionBenchmark=IdRegionBenchmark, reports=reports,
                water=water, PressureRatio=PressureRatio, RatioLosses=RatioLosses, mp=mp, mSkin=mSkin, mBrain=mBrain, mSkull=mSkull, metrics=met)


def differences(mod, name):
    """The names of what differs from the golden in case `name`: empty for a faithful restatement"""
    rec, r, bad = META['cases'][name], run_restatement(mod, name), []
    for k in ('SelBrain', 'SelSkin', 'SelSkull'):
        if not np.array_equal(np.packbits(r[k]), GOLD[name + '_' + k]):
            bad.append(k)
    if [int(v) for v in r['BrainID']] != rec['BrainID'] or r['IdRegionBenchmark'] != rec['IdRegionBenchmark']:
        bad.append('ids')
    if r['reports'] != rec['reports']:
        bad.append('reports')
    if hashlib.sha1(r['water'].tobytes()).hexdigest() != rec['water_sha1']:
        bad.append('water')
    for k in ('PressureRatio', 'RatioLosses'):
        if not same_scalar(r[k], rec[k]):
            bad.append(k)
    for k in ('mSkin', 'mBrain', 'mSkull'):
        if [int(v) for v in r[k]] != rec[k]:
            bad.append(k)
    where = np.flatnonzero(r['mp'])
    if not (np.array_equal(where, GOLD[name + '_monitor_index']) and np.array_equal(r['mp'].reshape(-1)[where], GOLD[name + '_monitor_id'])):
        bad.append('monitor')
    for k, want in rec['metrics'].items():
        if not same_scalar(r['metrics'][k], want):
            bad.append(k)
    for k in ('MaxIsppa', 'MaxIspta'):
        if not np.array_equal(r['metrics'][k], GOLD[name + '_' + k]):
            bad.append(k)
    return bad


@pytest.mark.parametrize('name', CASES)
def test_restatement_equals_the_reference(name):
    assert differences(TO, name) == []


def test_the_golden_covers_the_branches():
    took = [n for n in CASES if any(r[0].startswith('Warning: RatioLossesLoc') for r in META['cases'][n]['reports'])]
    assert took == ['switch']
    assert META['cases']['dome']['RatioLosses']['dtype'] == 'float32'
    assert len(GOLD['target_at_max_monitor_id']) == 3 and len(GOLD['plain_monitor_id']) == 4
    assert any(r[0].startswith('OVERWRITTING') for r in META['cases']['fixed_power']['reports'])
    assert len({json.dumps(flags_of(META['cases'][n]), sort_keys=True) for n in CASES}) == 8          # plain, ct, segmented, both, homogeneous, 3 tests


PLANTS = {
    'ties to the last index': [('cxr, cyr, czr = cxr[0], cyr[0], czr[0]', 'cxr, cyr, czr = cxr[-1], cyr[-1], czr[-1]')],
    'the raw-water plane read after the zeroing': [("    AcousticEnergyWater = plane_energy(pAmpWater[:, :, 2], MaterialList['Density'][0], MaterialList['SoS'][0], dx2)\n", ''),
                                                   ('    pAmpWater[sel] = 0.0\n', "    pAmpWater[sel] = 0.0\n    AcousticEnergyWater = plane_energy(pAmpWater[:, :, 2], "
                                                    "MaterialList['Density'][0], MaterialList['SoS'][0], dx2)\n"),
                                                   ("    report('Water Acoustic Energy entering', AcousticEnergyWater)\n    sel =", '    sel ='),
                                                   ('    cxw, cyw, czw = np.where(pAmpWater == pAmpWater.max())\n',
                                                    "    report('Water Acoustic Energy entering', AcousticEnergyWater)\n    cxw, cyw, czw = np.where(pAmpWater == pAmpWater.max())\n")],
    'selregion complemented': [('    pAmpWater[sel] = 0.0\n', '    pAmpWater[~sel] = 0.0\n')],
    'a division in float32': [('half.astype(np.float64) / np.asarray(R, np.float64))', '(half / np.asarray(R, np.float32)).astype(np.float64))')],
    'the +0.2 switch dropped': [('if RatioLosses > (RatioLossesLoc + 0.2):', 'if False:')],
    'the target voxel taken at LocIJK when segmented': [('    if bSegmentedBrain or len(IdRegionBenchmark) > 0:\n        SoSTarget', '    if len(IdRegionBenchmark) > 0:\n        SoSTarget')],
}


@pytest.mark.parametrize('fault', sorted(PLANTS))
def test_planted_fault_is_reported(fault):
    """Each fault in a patched copy of the restatement: the comparison with the golden must name a difference in at least one case"""
    text = inspect.getsource(TO)
    for old, new in PLANTS[fault]:
        assert text.count(old) == 1, (fault, old)
        text = text.replace(old, new)
    mod = types.ModuleType('thermal_oracle_planted')
    exec(compile(text, 'thermal_oracle_planted', 'exec'), mod.__dict__)
    found = {n: differences(mod, n) for n in CASES}
    assert any(found.values()), fault
    print(fault, {n: d for n, d in found.items() if d})


# ---------------------------------------------------------------- energy sums ----------------------------------------------------------------

@pytest.mark.parametrize('name', ['plain', 'segmented_ct', 'switch'])
def test_numpy_plane_sums_lie_within_the_bound_of_the_exact_sums(name):
    rec = META['cases'][name]
    case = TO.build_case(tuple(META['shape']), **rec['build'])
    f = flags_of(rec)
    t = TA.region_tables(case['nMat'], f['ct'], f['segmented'], f['homogeneous'], f['benchmark'])
    ml = case['MaterialList']
    dx2 = (case['xf'][1] - case['xf'][0]) ** 2
    s = TO.loss_survey(case['pAmp'], case['pAmpWater'], case['MaterialMap'], t['classOf'], ml['Density'], ml['SoS'], ml['Density'][0], ml['SoS'][0], dx2)
    n = case['pAmp'].shape[0] * case['pAmp'].shape[1]
    for which in ('WaterRaw', 'Water', 'Tissue'):
        for k in range(case['pAmp'].shape[2]):
            exact = math.fsum(s['terms' + which][:, :, k].reshape(-1).tolist())
            assert abs(s['e' + which][k] - exact) <= sum_bound(n, exact), (which, k)
    assert sum_bound(200000, 1.0) < 2.3e-11          # the bound hides no float32 division (6e-8)


# ---------------------------------------------------------------- the core header ----------------------------------------------------------------

CORE_PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bfd_thermal_core.h"
// terms:  in  int64 n; uint32 x[n]; double R[n], C[n], dx2          out double term[n]
// pairs:  in  int64 n; uint32 x[n]; uint8 in[n]                     out int64 {argIn, argKey}; float {maxIn, maxKey}; the fold goes over the
//         voxels in DESCENDING index order, so a fold that kept the first pair it saw would give the last index
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[2], "rb");
    int64_t n;
    if (!f || fread(&n, 8, 1, f) != 1) return 2;
    uint32_t *x = (uint32_t *)malloc(4 * n + 4);
    if (fread(x, 4, n, f) != (size_t)n) return 2;
    FILE *g = fopen(argv[3], "wb");
    if (!strcmp(argv[1], "terms")) {
        double *R = (double *)malloc(8 * n + 8), *C = (double *)malloc(8 * n + 8), dx2;
        if (fread(R, 8, n, f) != (size_t)n || fread(C, 8, n, f) != (size_t)n || fread(&dx2, 8, 1, f) != 1) return 2;
        for (int64_t i = 0; i < n; i++) { const double t = th_term(x[i], R[i], C[i], dx2); fwrite(&t, 8, 1, g); }
    } else {
        uint8_t *in = (uint8_t *)malloc(n + 1);
        if (fread(in, 1, n, f) != (size_t)n) return 2;
        uint64_t best = TH_NO_PAIR;
        int64_t firstOut = -1;
        for (int64_t i = n - 1; i >= 0; i--) {
            if (in[i]) best = th_pair_max(best, th_pair(th_key(x[i]), (uint32_t)i));
            else firstOut = i;
        }
        const uint64_t keyed = th_keyed_pair(best, firstOut);
        int64_t arg[2] = {th_pair_index(best), th_pair_index(keyed)};
        float mx[2] = {best == TH_NO_PAIR ? 0.f : th_key_value(th_pair_key(best)), keyed == TH_NO_PAIR ? 0.f : th_key_value(th_pair_key(keyed))};
        fwrite(arg, 8, 2, g);
        fwrite(mx, 4, 2, g);
    }
    fclose(g);
    return 0;
}
"""


@pytest.fixture(scope='module')
def core(tmp_path_factory):
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx, 'no C++ compiler found'
    d = tmp_path_factory.mktemp('thermalcore')
    src = d / 'thermalcore.cpp'
    src.write_text(CORE_PROGRAM)
    exe = str(d / 'thermalcore')
    subprocess.run([cxx, '-O1', '-ffp-contract=off', '-I', os.path.join(os.path.dirname(_engine.LIB_PATH), 'csrc'), str(src), '-o', exe, '-lm'], check=True)
    inp, outp = str(d / 'in.bin'), str(d / 'out.bin')

    def terms(x, R, C, dx2):
        x = np.ascontiguousarray(x, np.float32)
        with open(inp, 'wb') as f:
            f.write(np.int64(x.size).tobytes() + x.tobytes() + np.ascontiguousarray(R, np.float64).tobytes() + np.ascontiguousarray(C, np.float64).tobytes() +
                    np.float64(dx2).tobytes())
        subprocess.run([exe, 'terms', inp, outp], check=True)
        return np.fromfile(outp, np.float64, x.size)

    def pairs(x, sel):
        x = np.ascontiguousarray(x, np.float32)
        with open(inp, 'wb') as f:
            f.write(np.int64(x.size).tobytes() + x.tobytes() + np.ascontiguousarray(sel, np.uint8).tobytes())
        subprocess.run([exe, 'pairs', inp, outp], check=True)
        return np.fromfile(outp, np.int64, 2), np.fromfile(outp, np.float32, 2, offset=16)
    return terms, pairs


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def test_core_terms_equal_numpy_bit_for_bit(core):
    terms, _ = core
    rng = np.random.default_rng(7)
    n = 20000
    # random pressures; squares that are exact ties of the float32 rounding ((1 + m 2^-12)^2 = 1 + m 2^-11 + m^2 2^-24, a tie for odd m) and their
    # float32 neighbours, over many exponents; squares and halves that are float32 denormals; zeros of both signs; the largest finite value
    m = rng.integers(1, 4096, 4000) | 1
    ties = ((1.0 + m * 2.0 ** -12) * 2.0 ** rng.integers(-40, 40, m.size)).astype(np.float32)
    tiny = (rng.uniform(1, 2, 4000) * 2.0 ** rng.integers(-80, -58, 4000)).astype(np.float32)
    x = np.concatenate([rng.normal(0, 3e5, n).astype(np.float32), ties, np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(4e38)), tiny, -tiny,
                        np.array([0.0, -0.0, 2.0 ** -149, 2.0 ** -75, 2.0 ** -74.5, 2.0 ** -63, 2.0 ** -62.5, 3.4028235e38, 1.8e19], np.float32)])
    R = rng.uniform(900.0, 2300.0, x.size)
    C = rng.uniform(1400.0, 3200.0, x.size)
    dx2 = (0.37e-3) ** 2
    with np.errstate(over='ignore', under='ignore'):
        want = TO.plane_terms(x.reshape(1, -1), R.reshape(1, -1), C.reshape(1, -1), dx2).reshape(-1)
        half = (x * x) / np.float32(2)
    assert np.count_nonzero((half > 0) & (half < 2.0 ** -126)) > 1000          # the denormal halves are there
    assert bits_equal(terms(x, R, C, dx2), want)
    # the water form: scalars
    want = TO.plane_terms(x[:n].reshape(1, -1), 1000.0, 1500.0, dx2).reshape(-1)
    assert bits_equal(terms(x[:n], np.full(n, 1000.0), np.full(n, 1500.0), dx2), want)


def test_core_pairs_on_ties_signed_zeros_and_negatives(core):
    _, pairs = core
    rng = np.random.default_rng(8)

    def check(x, sel):
        x, sel = np.asarray(x, np.float32), np.asarray(sel, bool)
        arg, mx = pairs(x, sel)
        prod = x * sel.astype(np.float32)
        assert arg[1] == np.argmax(prod) and mx[1] == prod[np.argmax(prod)], (x, sel)
        if sel.any():
            at = np.flatnonzero(sel)[x[sel].argmax()]
            assert arg[0] == at and mx[0] == x[at] and (x[at] != 0 or True)
        else:
            assert arg[0] == -1 and mx[0] == 0
    check([1, 5, 5, 2], [1, 1, 1, 1])                      # a tie: the first
    check([5, 1, 5], [0, 1, 1])                            # a larger value outside the class
    check([-3, -1, -2], [1, 1, 1])                         # negatives, nothing outside
    check([-3, -1, -2, 7], [1, 1, 1, 0])                   # a class of negatives loses to the first zero outside it
    check([-0.0, 0.0, -0.0], [1, 1, 1])                    # -0 == +0: index 0
    check([-1, -0.0, 0.0], [1, 1, 1])
    check([3, -0.0, 0.0], [0, 1, 1])                       # the product outside is +0 at index 0, equal to the -0 inside
    check([-3, 0.0], [0, 1])                               # -3 * 0 = -0 at index 0 equals the +0 inside
    check([0, 0, 0], [0, 0, 0])                            # an empty class, an all-zero product: index 0
    check([2.0 ** -140, 2.0 ** -149, 0], [1, 1, 1])        # denormals are values like any other
    check([-2.0 ** -149, -2.0 ** -140], [1, 1])
    for _ in range(200):
        n = int(rng.integers(1, 40))
        x = rng.choice(np.array([-2, -1, -0.0, 0.0, 1, 2, 2.0 ** -149, -2.0 ** -149], np.float32), n)
        check(x, rng.integers(0, 2, n))


# ---------------------------------------------------------------- the module's host side ----------------------------------------------------------------

@pytest.mark.parametrize('name', CASES)
def test_region_tables_equal_the_selections(name):
    rec = META['cases'][name]
    case = TO.build_case(tuple(META['shape']), **rec['build'])
    f = flags_of(rec)
    M = case['MaterialMap']
    bench = dict(f['benchmark'], maxMaterial=int(M.max())) if f['benchmark'] else None
    t = TA.region_tables(case['nMat'], f['ct'], f['segmented'], f['homogeneous'], bench)
    SelBrain, SelSkin, SelSkull, BrainID, Ids = TO.selections(M, f['ct'], f['segmented'], f['homogeneous'], f['benchmark'])
    cls = t['classOf'][M]
    assert t['classOf'].dtype == np.uint8 and t['BrainID'] == BrainID and t['IdRegionBenchmark'] == Ids
    assert np.array_equal((cls >> TA.BIT_BRAIN) & 1, SelBrain) and np.array_equal((cls >> TA.BIT_SKIN) & 1, SelSkin)
    assert np.array_equal((cls >> TA.BIT_SKULL) & 1, SelSkull)
    assert np.array_equal((cls >> TA.BIT_SELREGION) & 1, TO.selregion(M, f['ct'], f['segmented'], f['homogeneous'], Ids))


@pytest.mark.parametrize('name', CASES)
def test_scalar_lines_and_monitoring_points_equal_the_golden(name):
    """losses_from_survey fed by the restatement's survey (numpy's own plane sums: equality), monitoring_points fed by the golden's maxima"""
    rec = META['cases'][name]
    case = TO.build_case(tuple(META['shape']), **rec['build'])
    f, call, ml, M = flags_of(rec), rec['call'], case['MaterialList'], case['MaterialMap']
    bench = dict(f['benchmark'], maxMaterial=int(M.max())) if f['benchmark'] else None
    t = TA.region_tables(case['nMat'], f['ct'], f['segmented'], f['homogeneous'], bench)
    s = TO.loss_survey(case['pAmp'], case['pAmpWater'], M, t['classOf'], ml['Density'], ml['SoS'], ml['Density'][0], ml['SoS'][0],
                       (case['xf'][1] - case['xf'][0]) ** 2)
    survey = {k: np.asarray(s[k])[None] for k in ('maxTissue', 'argTissue', 'maxWater', 'argWater', 'eWaterRaw', 'eWater', 'eTissue')}
    reports = []
    r = TA.losses_from_survey(survey, 0, M.shape, case['LocIJK'], M, ml, call['Isppa'], case['xf'], case['yf'], case['zf'], case['Input'], call['TxSystem'],
                              f['segmented'], t['IdRegionBenchmark'], call['FixedAcousticPower'],
                              report=lambda *a: reports.append([a[0].split('\n')[0]] + numbers(a[1:])))
    assert reports == rec['reports']
    assert same_scalar(r['PressureRatio'], rec['PressureRatio']) and same_scalar(r['RatioLosses'], rec['RatioLosses'])
    assert hashlib.sha1(s['water'].tobytes()).hexdigest() == rec['water_sha1']
    mp = TA.monitoring_points(rec['mSkin'], rec['mBrain'], rec['mSkull'], case['LocIJK'], M.shape, f['homogeneous'], f['benchmark'])
    assert np.array_equal(mp.indices, GOLD[name + '_monitor_index']) and np.array_equal(mp.ids, GOLD[name + '_monitor_id'])
    dense = TA.monitoring_points_map(rec['mSkin'], rec['mBrain'], rec['mSkull'], case['LocIJK'], M.shape, f['homogeneous'], f['benchmark'])
    assert dense.dtype == np.uint32 and np.array_equal(np.flatnonzero(dense), mp.indices)


def test_monitoring_points_later_stores_replace_earlier_ones():
    mp = TA.monitoring_points((1, 1, 1), (1, 1, 1), (2, 0, 0), (2, 0, 0), (3, 3, 3))
    want = np.zeros((3, 3, 3), np.uint32)
    want[1, 1, 1] = 1; want[1, 1, 1] = 2; want[2, 0, 0] = 3; want[2, 0, 0] = 4
    assert np.array_equal(mp.dense(), want) and list(mp.ids) == [2, 4]


def test_sparse_monitoring_points_give_the_rows_of_the_dense_map():
    from babelbrain_amd import RayleighAndBHTE as R
    rng = np.random.default_rng(3)
    shape = (5, 6, 7)
    lin = rng.choice(5 * 6 * 7, 4, replace=False)
    mp = TA.MonitoringPoints([3, 1, 4, 2], lin, shape)
    ml = dict(Density=np.array([1000.0, 1100.0]), SoS=np.array([1500.0, 1600.0]), Attenuation=np.array([0.0, 5.0]), SpecificHeat=np.array([4178.0, 3600.0]),
              Conductivity=np.array([0.6, 0.5]), Perfusion=np.array([0.0, 500.0]), Absorption=np.array([0.0, 0.8]), InitTemperature=np.array([37.0, 37.0]))
    P = np.ones((1,) + shape, np.float32)
    M = np.zeros(shape, np.uint8)
    a = R._bhte_inputs(P, M, ml, 1e-3, 0.1, 1050, 3617, 1.0, mp, None, None)['idx']
    b = R._bhte_inputs(P, M, ml, 1e-3, 0.1, 1050, 3617, 1.0, mp.dense(), None, None)['idx']
    assert a.dtype == b.dtype and np.array_equal(a, b) and list(a) == [lin[1], lin[3], lin[0], lin[2]]
    with pytest.raises(ValueError):
        R._bhte_inputs(P, M, ml, 1e-3, 0.1, 1050, 3617, 1.0, TA.MonitoringPoints([1], [0], (5, 6, 8)), None, None)


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """The library is out of reach: loading it is an error. The refusals below must come first."""
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_engine, 'LIB_PATH', str(tmp_path / 'no_such_library.so'))
    monkeypatch.setattr(_engine, '_lib', None)
    monkeypatch.setattr(_engine, 'load_library', boom)


def test_argument_errors_come_before_the_library(no_library):
    M = np.zeros((2, 3, 4), np.uint32)
    x = np.zeros((2, 3, 4), np.float32)
    t = np.zeros(2, np.uint8)
    one = np.ones(2)
    for bad in (lambda: TA.tissue_extrema([], M, t), lambda: TA.tissue_extrema([x.astype(np.float64)], M, t), lambda: TA.tissue_extrema([x[:1]], M, t),
                lambda: TA.tissue_extrema([x], M.astype(np.float32), t), lambda: TA.tissue_extrema([x], M, np.zeros(0, np.uint8)),
                lambda: TA.tissue_extrema([x], M, np.full(2, 256)), lambda: TA.loss_survey(x, x[:1], M, t, one, one, 1000.0, 1500.0, 1e-6),
                lambda: TA.loss_survey(x, x, M, t, one[:1], one, 1000.0, 1500.0, 1e-6), lambda: TA.loss_survey(x, x, M, t, one, one * 0, 1000.0, 1500.0, 1e-6),
                lambda: TA.loss_survey(x, x, M, t, one, one, np.inf, 1500.0, 1e-6), lambda: TA.loss_survey(x, x, M, t, one, one, 1000.0, 1500.0, -1.0),
                lambda: TA.loss_survey(x, x, M, t, one, one, 1000.0, 1500.0, 1e-6, brainMask=x[:1]), lambda: TA.region_tables(0, False, False),
                lambda: TA.region_tables(5, False, False, benchmark=dict(TestType=4, nMaterials=3))):
        with pytest.raises((ValueError, TypeError)):
            bad()
