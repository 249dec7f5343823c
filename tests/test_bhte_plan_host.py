"""The bio-heat solver's planner without a GPU: csrc/bfd_bhte_plan_core.h -- the cut of a schedule into passes, the grid of a pass, the switches and the
pads of the volumes -- compiled for the host with a stock compiler and held to (1) RayleighAndBHTE.bhte_pass_plan, the restatement the benchmark takes
its bytes per voxel-step from, pass for pass, (2) a numpy restatement of the run-length choice, (3) a brute-force walk over every cell the multi-step
kernels' regions address, which must stay inside the pads."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from babelbrain_amd import _engine, RayleighAndBHTE as R

CSRC = os.path.join(os.path.dirname(_engine.LIB_PATH), 'csrc')

CORE_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "bfd_bhte_plan_core.h"
// plan <fits mask>: in  int32 nCases; per case int32 nSteps, nCaptures, fieldOfStep[nSteps], captureStep[nCaptures]; knobs from the environment
//                   out int32 fuse, stepsHeating, stepsCooling, zrun; per case int32 nPasses, then {first, length, kind, fieldA, fieldB} per pass
// geom: in  int32 nCases; per case int32 N1, N2, N3, S, forcedZrun       out per case int64 tilesX, tilesY, zrun, nBlocks
// pads: in  int32 nCases; per case int32 N1                               out int64 H, then W and output rows for S = 2, 3, 4; per case int64 front, back
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[argc - 2], "rb"), *o = fopen(argv[argc - 1], "wb");
    int32_t n;
    if (!f || !o || fread(&n, 4, 1, f) != 1) return 2;
    if (!strcmp(argv[1], "plan")) {
        const int mask = atoi(argv[2]);
        const bool fits[BHTE_SMAX + 1] = {false, false, (mask & 4) != 0, (mask & 8) != 0, (mask & 16) != 0};
        const bhte_knobs k = bhte_knobs_from_env();
        const int32_t kw[4] = {k.fuse, k.stepsHeating, k.stepsCooling, k.zrun};
        fwrite(kw, 4, 4, o);
        for (int q = 0; q < n; q++) {
            int32_t h[2];
            if (fread(h, 4, 2, f) != 2) return 2;
            std::vector<int32_t> sched(h[0] + 1), caps(h[1] + 1);
            if (fread(sched.data(), 4, h[0], f) != (size_t)h[0] || fread(caps.data(), 4, h[1], f) != (size_t)h[1]) return 2;
            const std::vector<bhte_pass> plan = bhte_plan_passes(sched.data(), h[0], caps.data(), h[1], k, fits);
            const int32_t np = (int32_t)plan.size();
            fwrite(&np, 4, 1, o);
            for (const bhte_pass &p : plan) { const int32_t w[5] = {p.first, p.length, p.kind, p.fieldA, p.fieldB}; fwrite(w, 4, 5, o); }
        }
    } else if (!strcmp(argv[1], "geom")) {
        for (int q = 0; q < n; q++) {
            int32_t c[5];
            if (fread(c, 4, 5, f) != 5) return 2;
            const bhte_geom g = bhte_pass_geom(c[0], c[1], c[2], c[3], c[4]);
            const int64_t w[4] = {g.tilesX, g.tilesY, g.zrun, g.nBlocks};
            fwrite(w, 8, 4, o);
        }
    } else {
        const int64_t w[7] = {BHTE_REGION_H, bhte_region_w(2), bhte_tile_rows(2), bhte_region_w(3), bhte_tile_rows(3), bhte_region_w(4), bhte_tile_rows(4)};
        fwrite(w, 8, 7, o);
        for (int q = 0; q < n; q++) {
            int32_t N1; size_t fb[2];
            if (fread(&N1, 4, 1, f) != 1) return 2;
            bhte_pads(N1, &fb[0], &fb[1]);
            const int64_t v[2] = {(int64_t)fb[0], (int64_t)fb[1]};
            fwrite(v, 8, 2, o);
        }
    }
    fclose(o);
    return 0;
}
"""

_ENV = ('BFD_BHTE_FUSE', 'BFD_BHTE_STEPS', 'BFD_BHTE_ZRUN')


class Core:
    def __init__(self, d, flags=()):
        cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
        assert cxx, 'no C++ compiler found'
        src = d / 'plancore.cpp'
        src.write_text(CORE_PROGRAM)
        self.exe, self.inp, self.outp = str(d / 'plancore'), str(d / 'in.bin'), str(d / 'out.bin')
        subprocess.run([cxx, '-O1', '-std=c++17', '-Wall', '-Werror', *flags, '-I', CSRC, str(src), '-o', self.exe], check=True)

    def run(self, mode, words, env=None, dtype=np.int32):
        full = {k: v for k, v in os.environ.items() if k not in _ENV}
        full.update(env or {})
        np.asarray(words, np.int32).tofile(self.inp)
        subprocess.run([self.exe, *mode, self.inp, self.outp], check=True, env=full)
        return np.fromfile(self.outp, dtype)

    def plans(self, cases, env=None, mask=28):
        """cases: [(sched, caps)] -> (knobs, [[(first, length, kind, fieldA, fieldB)]])"""
        words = [len(cases)]
        for sched, caps in cases:
            words += [len(sched), len(caps), *sched, *caps]
        flat = self.run(['plan', str(mask)], words, env)
        knobs, p, out = tuple(int(v) for v in flat[:4]), 4, []
        for _ in cases:
            k = int(flat[p])
            out.append([tuple(int(v) for v in flat[p + 1 + 5 * i:p + 6 + 5 * i]) for i in range(k)])
            p += 1 + 5 * k
        assert p == flat.size
        return knobs, out

    def geoms(self, cases):
        return self.run(['geom'], [len(cases)] + [v for c in cases for v in c], dtype=np.int64).reshape(-1, 4)

    def pads(self, N1s):
        flat = self.run(['pads'], [len(N1s), *N1s], dtype=np.int64)
        H, regions = int(flat[0]), {S: (int(flat[1 + 2 * i]), int(flat[2 + 2 * i])) for i, S in enumerate((2, 3, 4))}
        return H, regions, flat[7:].reshape(-1, 2)


@pytest.fixture(scope='module')
def core(tmp_path_factory):
    return Core(tmp_path_factory.mktemp('plancore'))


# ---------------------------------------------------------------- plans ----------------------------------------------------------------

def _schedules():
    """300 random schedules of at most 40 steps (fields -1 .. 2 in stretches of 1 .. 9 steps) with ascending capture lists that hold duplicates, 0 and
    nSteps; then nSteps = 0 .. 3 with every capture list over their boundaries."""
    rng = np.random.default_rng(20)
    cases = []
    for q in range(300):
        n = int(rng.integers(1, 41))
        sched = []
        while len(sched) < n:
            sched += [int(rng.integers(-1, 3))] * int(rng.integers(1, 10))
        sched = sched[:n]
        caps = sorted(int(c) for c in rng.integers(0, n + 1, int(rng.integers(0, 6)))) if q % 3 else []
        if q % 6 == 1:
            caps = sorted(caps + [0, n, caps[len(caps) // 2] if caps else n])
        cases.append((sched, caps))
    for n in range(4):
        for fields in ([-1] * n, [0] * n, [0, -1, 1][:n]):
            for caps in ([], [0], [n], [0, n, n], list(range(n + 1)), [1] if n > 1 else [0, 0]):
                cases.append((fields, caps))
    return cases


def _check_plan(sched, caps, plan, fuse, steps):
    n = len(sched)
    assert [p[0] for p in plan] == [sum(q[1] for q in plan[:i]) for i in range(len(plan))] and sum(p[1] for p in plan) == n, 'tiles [0, nSteps) once, in order'
    for first, L, kind, fa, fb in plan:
        assert L in (1, 2, 3, 4) and not any(first < c < first + L for c in caps), 'a capture strictly inside a pass'
        assert fa == sched[first] and fb == sched[first + (1 if L == 2 else 0)]
        if L >= 3:
            assert len(set(sched[first:first + L])) == 1 and fuse and L == (steps or 4), 'an S-pass carries one field'
        heats = [f >= 0 for f in sched[first:first + L]]
        assert kind == (0 if not any(heats) else 1 if len(set(sched[first:first + L])) == 1 else 2)
        assert fuse or L == 1


def test_plans_tile_the_schedule_and_equal_the_python_restatement(core):
    cases = _schedules()
    assert {len(s) for s, _ in cases} >= {0, 1, 2, 3, 40} and any(len(set(c)) < len(c) for _, c in cases)
    seen = set()
    for fuse in (1, 0):
        for steps in (0, 2, 3, 4):
            env = {'BFD_BHTE_FUSE': str(fuse)} if (steps or not fuse) else {}              # default knobs: nothing set at all
            if steps:
                env['BFD_BHTE_STEPS'] = str(steps)
            knobs, plans = core.plans(cases, env)
            assert knobs == (fuse, steps or 4, steps or 4, 0)
            for (sched, caps), plan in zip(cases, plans):
                _check_plan(sched, caps, plan, fuse, steps)
                want = R.bhte_pass_plan(sched, steps_heating=steps or 4, steps_cooling=steps or 4, capture_steps=caps, fuse=bool(fuse))
                assert [(p[0], p[1], p[2] != 0) for p in plan] == want, (sched, caps, fuse, steps)
                if not caps and fuse and not steps:
                    assert want == R.bhte_pass_plan(sched, 10, True), "the call of bench.py"
                seen.update((p[1], p[2]) for p in plan)
    assert seen == {(1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (4, 0), (4, 1)}, 'every pass kind occurred'


def test_switches_are_read_as_before(core):
    """BFD_BHTE_FUSE: only a value that reads as 0 turns fusing off; BFD_BHTE_STEPS outside 2 .. 4 and BFD_BHTE_ZRUN <= 0 are ignored"""
    for env, want in (({'BFD_BHTE_FUSE': '1'}, (1, 4, 4, 0)), ({'BFD_BHTE_FUSE': 'x'}, (0, 4, 4, 0)), ({'BFD_BHTE_STEPS': '5'}, (1, 4, 4, 0)),
                      ({'BFD_BHTE_STEPS': '1'}, (1, 4, 4, 0)), ({'BFD_BHTE_ZRUN': '-3'}, (1, 4, 4, 0)), ({'BFD_BHTE_ZRUN': '12', 'BFD_BHTE_STEPS': '3'}, (1, 3, 3, 12))):
        assert core.plans([], env)[0] == want, env


def test_a_pass_kind_that_does_not_fit_the_grid_falls_back(core):
    """nBlocks >= 2^31 for a kind: its stretches go to the next shorter kind, as if it had not been asked for"""
    cases = [c for c in _schedules() if not c[1]][:60]
    _, no4 = core.plans(cases, mask=4)                        # only two steps fit
    _, none = core.plans(cases, mask=0)
    for (sched, _), a, b in zip(cases, no4, none):
        assert [(p[0], p[1], p[2] != 0) for p in a] == R.bhte_pass_plan(sched, steps_heating=2, steps_cooling=2)
        assert [(p[0], p[1], p[2] != 0) for p in b] == R.bhte_pass_plan(sched, fuse=False)


# ---------------------------------------------------------------- geometry ----------------------------------------------------------------

GRIDS = ((3, 3, 3), (64, 22, 16), (65, 23, 9), (150, 61, 37), (320, 320, 320), (512, 512, 512))


def test_pass_geometry_equals_the_numpy_arg_min(core):
    cases = [(*g, S, forced) for g in GRIDS for S in (2, 3, 4) for forced in (0, 1, 5, 64)]
    got = core.geoms(cases)
    for (N1, N2, N3, S, forced), (tx, ty, zrun, nblocks) in zip(cases, got):
        assert tx == -(-N1 // 64) and ty == -(-N2 // (28 - 2 * S))
        if forced:
            assert zrun == forced
        else:
            z = np.arange(8, (64 if S == 2 else 96) + 1)
            cost = -(-(tx * ty * -(-N3 // z)) // 256) * (z + 2 * S - 2)
            assert zrun == z[np.flatnonzero(cost == cost.min())[-1]], (N1, N2, N3, S)
        assert nblocks == tx * ty * -(-N3 // zrun)


# ---------------------------------------------------------------- pads ----------------------------------------------------------------

def _reach(N1, N2, S, W, H, rows):
    """lowest and highest element index, relative to a plane's first element, that a cell of any region addresses on that plane: region (bx, by) holds
    the cells (by rows - S + ry) N1 + bx 64 - S + rx, rx < W, ry < H. The index grows with the row and with the column, so its extremes are those of
    the rows and of the columns (test_reach_is_separable walks every cell)."""
    gi = (np.arange(-(-N1 // 64))[:, None] * 64 - S + np.arange(W)[None, :]).ravel()
    gj = (np.arange(-(-N2 // rows))[:, None] * rows - S + np.arange(H)[None, :]).ravel()
    return int(gj.min()) * N1 + int(gi.min()), int(gj.max()) * N1 + int(gi.max())


def _check_pads(core, N1s, N2s):
    """Returns the worst use of the front and of the back pad. N3 = 3: the kernels clamp the plane to [0, N3 - 1], so the first plane has the lowest and
    the last plane the highest address whatever N3 is."""
    H, regions, pads = core.pads(N1s)
    use_f = use_b = 0.0
    for N1, (front, back) in zip(N1s, pads):
        assert front == -(-(4 * N1 + 64) // 256) * 256 and back == 49 * N1 + 256, 'the pads every volume has been sized with'
        for N2 in N2s:
            pl, n = N1 * N2, N1 * N2 * 3
            assert 4 * -(-n // 4) - 1 < n + back, 'the last float4 of bhte_capture'
            for S in (2, 3, 4):
                W, rows = regions[S]
                assert (W, rows) == (64 + 2 * S, H - 2 * S)
                lo, hi = _reach(N1, N2, S, W, H, rows)
                assert -front <= lo and 2 * pl + hi < n + back, (N1, N2, S)
                use_f, use_b = max(use_f, -lo / front), max(use_b, (hi - pl + 1) / back)
    return H, use_f, use_b


N1S, N2S = list(range(3, 140)) + [320, 512], list(range(3, 60)) + [320]


def test_reach_is_separable():
    for N1, N2, S in ((3, 3, 2), (65, 23, 3), (150, 61, 4), (139, 59, 2)):
        W, H, rows = 64 + 2 * S, 28, 28 - 2 * S
        idx = [(by * rows - S + ry) * N1 + bx * 64 - S + rx for by in range(-(-N2 // rows)) for bx in range(-(-N1 // 64)) for ry in range(H) for rx in range(W)]
        assert (min(idx), max(idx)) == _reach(N1, N2, S, W, H, rows)


def test_regions_stay_inside_the_pads(core):
    """Worst use, brute-forced: 0.89 of the front pad, 0.51 of the back pad (S = 4 at N1 = 112; S = 2 at large N1)."""
    H, use_f, use_b = _check_pads(core, N1S, N2S)
    assert H == 28 and 0 < use_f <= 1 and 0 < use_b <= 1
    print('worst use of the pads: front %.3f, back %.3f' % (use_f, use_b))


def test_a_planted_region_height_fails_the_pad_check(tmp_path):
    """A region of 30 rows: the header's pads follow its geometry, so they are no longer the ones the volumes are sized with and the check must refuse"""
    planted = Core(tmp_path, flags=('-DBFD_BHTE_REGION_H=30',))
    with pytest.raises(AssertionError):
        _check_pads(planted, N1S[:8], N2S[:4])
