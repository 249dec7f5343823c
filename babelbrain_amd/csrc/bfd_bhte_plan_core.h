// The bio-heat solver (bfd_bhte.hip, bfd_bhte_kernels.hip): what a run decides before it launches a kernel -- the regions of the multi-step kernels, the
// pads the volumes carry for them, the grid of a pass, the switches, the cut of a schedule into passes. Plain C++ for the host, no HIP header: the tests
// compile it with a stock compiler (tests/test_bhte_plan_host.py); RayleighAndBHTE.bhte_pass_plan mirrors bhte_plan_passes for the benchmark's bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>

// ---- regions: a workgroup of an S-step kernel (S = 2: bhte_step2g; 3, 4: bhte_stepNg) marches a z-run over (64 + 2 S) x 28 cells, S rings around its
// 64 x (28 - 2 S) output cells. The height does not grow with S: a thread owns cells H / 4 (or H / 2) rows apart in one column. ----
#ifndef BFD_BHTE_REGION_H
#define BFD_BHTE_REGION_H 28       // the tests plant another height to see their pad check fail
#endif
constexpr int BHTE_TILE_W = 64, BHTE_REGION_H = BFD_BHTE_REGION_H, BHTE_SMIN = 2, BHTE_SMAX = 4;
constexpr int bhte_region_w(int S) { return BHTE_TILE_W + 2 * S; }
constexpr int bhte_tile_rows(int S) { return BHTE_REGION_H - 2 * S; }
constexpr int BHTE_STEPS_HEATING = 4, BHTE_STEPS_COOLING = 4;      // steps per pass of the default path (bfd_bhte.hip says how that was chosen)

// ---- pads, in elements: the multi-step kernels address every cell of their regions, also those that hang over the faces of the volume (what must not be
// used is masked where it is used). The first region starts S rows and S cells before the volume; the last starts S rows above a row of the volume and
// ends at most 63 + S cells behind a row's end: S N1 + S elements before the first, (H - 1 - S) N1 + 63 + S behind the last; bhte_capture reads whole
// float4, up to 3 behind. The pads kept are wider (front: whole KiB, so that padded volumes stay aligned; back: about twice the reach); every run and the
// thermal study have sized their volumes with them. ----
constexpr int BHTE_PAD_FRONT_ROWS = BHTE_SMAX, BHTE_PAD_FRONT_CELLS = BHTE_TILE_W;
constexpr int BHTE_PAD_BACK_ROWS = 2 * (BHTE_REGION_H - 1 - BHTE_SMIN) - 1, BHTE_PAD_BACK_CELLS = 4 * BHTE_TILE_W;
static_assert(BHTE_SMAX <= BHTE_PAD_FRONT_CELLS && BHTE_REGION_H - 1 - BHTE_SMIN <= BHTE_PAD_BACK_ROWS && BHTE_TILE_W - 1 + BHTE_SMAX <= BHTE_PAD_BACK_CELLS,
              "the pads cover the reach of every region for 2 <= S <= 4");
inline void bhte_pads(int N1, size_t *front, size_t *back)
{
    *front = (((size_t)BHTE_PAD_FRONT_ROWS * N1 + BHTE_PAD_FRONT_CELLS + 255) / 256) * 256;
    *back = (size_t)BHTE_PAD_BACK_ROWS * N1 + BHTE_PAD_BACK_CELLS;
}

// ---- the grid of an S-step pass ----
struct bhte_geom { int tilesX, tilesY, zrun; long nBlocks; };
// The multi-step kernels run at the memory system's rate with one to three workgroups per CU alike (profiles/r4/bhte_two_step_kernel_rewrite.txt), so a
// CU's time is the number of workgroups it gets times the planes each of them marches (its run + 2 S - 2: every run re-reads and recomputes the planes
// its levels need around it): the run length minimises ceil(workgroups / 256) x (zrun + 2 S - 2), the longest among equals. The measured order of run
// lengths follows this count at 256^3, 384^3 and 512^3. forcedZrun > 0 (BFD_BHTE_ZRUN) is taken as given.
inline bhte_geom bhte_pass_geom(int N1, int N2, int N3, int S, int forcedZrun)
{
    bhte_geom g;
    g.tilesX = (N1 + BHTE_TILE_W - 1) / BHTE_TILE_W;
    g.tilesY = (N2 + bhte_tile_rows(S) - 1) / bhte_tile_rows(S);
    g.zrun = forcedZrun > 0 ? forcedZrun : 0;
    if (!g.zrun) {
        long best = -1;
        for (int z = 8; z <= (S == 2 ? 64 : 96); z++) {
            const long w = (long)g.tilesX * g.tilesY * ((N3 + z - 1) / z), cost = ((w + 255) / 256) * (z + 2 * S - 2);
            if (best < 0 || cost <= best) { best = cost; g.zrun = z; }
        }
    }
    g.nBlocks = (long)g.tilesX * g.tilesY * ((N3 + g.zrun - 1) / g.zrun);
    return g;
}
inline bool bhte_geom_fits(const bhte_geom &g) { return g.nBlocks < 0x7fffffffL; }       // the block index is an int in the kernels

// ---- switches (the tests' cross-checks), read once per run ----
// BFD_BHTE_FUSE=0: one step per launch. BFD_BHTE_STEPS=2 / 3 / 4: that many steps per pass, heating and cooling. BFD_BHTE_ZRUN=n: z-runs of n planes.
struct bhte_knobs { bool fuse; int stepsHeating, stepsCooling, zrun; };
inline bhte_knobs bhte_knobs_from_env()
{
    auto num = [](const char *name, int unset) { const char *ev = getenv(name); return ev ? atoi(ev) : unset; };
    const int steps = num("BFD_BHTE_STEPS", 0), zrun = num("BFD_BHTE_ZRUN", 0);
    const bool forced = steps >= BHTE_SMIN && steps <= BHTE_SMAX;
    return {num("BFD_BHTE_FUSE", 1) != 0, forced ? steps : BHTE_STEPS_HEATING, forced ? steps : BHTE_STEPS_COOLING, zrun > 0 ? zrun : 0};
}

// ---- the passes of a schedule ----
// kind: what heats during the pass -- nothing, the same field in every step, or anything else (two steps with different fields, or one of them without)
enum { BHTE_COOLING = 0, BHTE_ONE_FIELD = 1, BHTE_MIXED = 2 };
struct bhte_pass { int first, length, kind, fieldA, fieldB; };      // fields of the first and the second step (-1: none; a pass of one step: fieldB = fieldA)
// S steps per pass (S = stepsHeating or stepsCooling by the first step's field) where S >= 3, S steps are left, all of them carry the same field and no
// capture boundary lies strictly inside; else two steps, under fuse, where two are left and no capture lies between them; else one. Without fuse every
// step is a pass. fits[S]: an S-step pass fits the grid (bhte_geom_fits), S = 2 .. 4. captureStep ascends within [0, nSteps] (HOST array).
inline std::vector<bhte_pass> bhte_plan_passes(const int32_t *fieldOfStep, int nSteps, const int32_t *captureStep, int nCaptures, const bhte_knobs &k,
                                               const bool fits[BHTE_SMAX + 1])
{
    std::vector<bhte_pass> plan;
    int nextCap = 0;
    auto capFree = [&](int s, int L) { return nextCap >= nCaptures || (long)s + L <= captureStep[nextCap]; };
    for (int s = 0; s < nSteps;) {
        while (nextCap < nCaptures && captureStep[nextCap] == s) nextCap++;     // the captures due at this boundary are taken before the pass
        const int fa = fieldOfStep[s];
        const int S = !k.fuse ? BHTE_SMIN : fa >= 0 ? k.stepsHeating : k.stepsCooling;
        bool passN = S >= 3 && S <= BHTE_SMAX && s + S <= nSteps && fits[S] && capFree(s, S);
        for (int j = 1; j < S && passN; j++) passN = fieldOfStep[s + j] == fa;
        if (passN) plan.push_back({s, S, fa >= 0 ? BHTE_ONE_FIELD : BHTE_COOLING, fa, fa});
        else if (k.fuse && s + 1 < nSteps && fits[2] && capFree(s, 2)) {
            const int fb = fieldOfStep[s + 1];
            plan.push_back({s, 2, (fa < 0 && fb < 0) ? BHTE_COOLING : fa == fb ? BHTE_ONE_FIELD : BHTE_MIXED, fa, fb});
        } else plan.push_back({s, 1, fa >= 0 ? BHTE_ONE_FIELD : BHTE_COOLING, fa, fa});
        s += plan.back().length;
    }
    return plan;
}
