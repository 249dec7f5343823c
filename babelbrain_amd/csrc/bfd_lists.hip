// The planner of the class-specialised path of libbabelfdtd_hip.so: from the cell classes to the run lists of the tiled kernels, the sparse shear
// list, the compact solid state, the byte tables and the activity map of the quiet runs; it also decides the engine's mode when the lists are built
// (advanced Vz, quiet runs). gfx950 only. bfd_api.hip reaches it through build_tile_lists, setup_activity_map, bind_compact_views and
// quiet_runs_wanted (bfd_internal.h).
#include "bfd_internal.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <hipcub/hipcub.hpp>

namespace {

// number of non-zero edge coefficients A (active shear updates) in the sparse shear list
__global__ void count_active_edges(const float *__restrict__ coef, const unsigned *__restrict__ codes, long n, unsigned long long *__restrict__ out)
{
    unsigned c = 0, x = 0;          // out[0] active edges, out[1] edges with explicit coefficients
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
        c += (coef[6 * t] != 0.f) + (coef[6 * t + 2] != 0.f) + (coef[6 * t + 4] != 0.f);
        const unsigned w = codes[t];
        x += ((w & 255u) == 255u) + (((w >> 8) & 255u) == 255u) + (((w >> 16) & 255u) == 255u);
    }
    if (c) atomicAdd(out, (unsigned long long)c);
    if (x) atomicAdd(out + 1, (unsigned long long)x);
}

}  // namespace

// where the ten compact arrays live (bfd_tiles::cssHosted); called when the list is built and again whenever the state buffers change hands
// (bfd_choose_placement exchanges them at step 0, when everything is still zero)
void bind_compact_views(bfd_sim *s)
{
    bfd_dev &d = s->d;
    if (!d.cssRow) return;
    float **cp[10] = {&d.cSxx, &d.cSyy, &d.cSxy, &d.cSxz, &d.cSyz, &d.cRxx, &d.cRyy, &d.cRxy, &d.cRxz, &d.cRyz};
    static const int host[10] = {3, 4, 6, 7, 8, 9, 10, 12, 13, 14};      // Sxx Syy Sxy Sxz Syz Rxx Ryy Rxy Rxz Ryz among the 15 state arrays
    for (int a = 0; a < 10; a++)
        *cp[a] = s->tiles.cssHosted ? s->stateBase[host[a]] + 4 * (size_t)d.plane : s->tiles.css + (size_t)a * s->tiles.cssCap;
}

// The tile grid of one build: tx x ty columns of nsub sub-tiles (n in all) of SUB planes; a z-chunk, the longest run, is perChunk sub-tiles.
// "boundary" sub-tiles hold the 2 first / 2 last planes of the slab (what a Z-neighbour reads): they form the
// small part 1 of a split half-step; everything else is part 2. lowPlanes / hiStart delimit them in planes.
struct TileGrid {
    int tx, ty, nsub, n, SUB, perChunk, nChunks, nk, lowPlanes, hiStart;
    bool subBnd(int q) const { return q * SUB < lowPlanes || std::min((q + 1) * SUB, nk) > hiStart; }
};
// Not a getter: it chooses the run length of this build and stores it in s->zchunk (bfd_sim keeps the choice; perChunk is derived from it).
static TileGrid choose_tile_grid(bfd_sim *s)
{
    int tx, ty, nsub; bfd_tile_grid(s->d, &tx, &ty, &nsub);
    const int n = tx * ty * nsub;
    const int SUB = bfd_tile_subz();
    // longest run one workgroup marches: 16 planes; 8 on small grids so that the launch still has a few thousand
    // workgroups (measured: 256^3 49 -> 58, 128^3 29 -> 46 Gvoxel-steps/s). 32 was best at 512^3 while the z-chunks of
    // a column were consecutive in the list; under the banded order 16 is 2.5 % faster than 32 and 3 % faster than 8.
    const int t32 = tx * ty * ((s->d.nk + 31) / 32);
    // round 6: the switch point moved from 1500 to 3000 columns (320^3: 8 planes +4 % in water, +7 % with bone -- velocity_solid wants the workgroups; 352^3: +1.5 %;
    // 384^3: 16 planes +4 %; profiles/r6/pml_flavour_cost_and_run_length_mid_size.txt)
    s->zchunk = t32 >= 3000 ? 16 : 8;
    if (const char *ev = getenv("BFD_ZRUN")) { const int z = atoi(ev); if (z >= SUB && z % SUB == 0) s->zchunk = z; }   // tuning experiments
    if (s->zchunk > bfd_tile_zchunk()) s->zchunk = bfd_tile_zchunk();
    const int perChunk = s->zchunk / SUB;
    const int nChunks = (nsub + perChunk - 1) / perChunk;
    const int nkl = s->d.nk;
    const int lowPlanes = std::min(SUB, nkl);
    const int hiStart = std::max(((nkl - 2) / SUB) * SUB, lowPlanes);
    return {tx, ty, nsub, n, SUB, perChunk, nChunks, nkl, lowPlanes, hiStart};
}

// class flags and material of every sub-tile, from the device
static int fetch_tile_classes(bfd_sim *s, int n, std::vector<int> &flags, std::vector<int> &mats)
{
    DevTemp<int> dflags, dmats;
    BFD_HIP(dflags.alloc(n));
    hipError_t e = dmats.alloc(n);
    if (e == hipSuccess) {
        bfd_launch_classify(s->d, s->stream, dflags, dmats);
        e = hipMemcpyAsync(flags.data(), dflags, n * sizeof(int), hipMemcpyDeviceToHost, s->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(mats.data(), dmats, n * sizeof(int), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) BFD_FAIL(-10, std::string("classify tiles: ") + hipGetErrorString(e));
    return 0;
}

// Runs of the fused time step (variant 4, bfd_kernels_fused.hip): 64 x 24 cells = three tiles of this grid in y, a z-run of
// 2 .. fusedSub sub-tiles. A sub-tile qualifies (bit5) when it is fluid, has nothing of the absorbing layer or the domain
// edge within 2 cells (bit6), is not a boundary sub-tile of the slab, and the sources are of velocity type. Per column and
// z-chunk the rows are scanned upwards: where three consecutive tile rows qualify over a z-stretch they form a run and the
// scan moves on by three rows. A run is UNI when every sub-tile is (one material in the grown regions) and lossy when a
// cell of a grown region relaxes (bit7); stretches are cut where that class changes (a single sub-tile joins its neighbour).
static void form_fused_runs(bfd_sim *s, const TileGrid &G, std::vector<int> &flags, const std::vector<int> &mats, std::vector<char> &taken, std::vector<int4> &fused)
{
    const int tx = G.tx, ty = G.ty, nsub = G.nsub, SUB = G.SUB;
    const int fusedSub = 32 / SUB;
    struct FusedRun { int bx, by, q0, q1, cls, mat; };
    std::vector<FusedRun> fruns;
    if (s->pingpong && s->cfg.typeSource < 2) {
        const int FRW = bfd_fused_rows() / 8;
        const size_t layer = (size_t)tx * ty;
        for (int q = 0; q < nsub; q++)
            for (size_t txy = 0; txy < layer; txy++) { int &f = flags[(size_t)q * layer + txy]; if (!(f & 1) && !(f & 64) && !(f & 256) && !G.subBnd(q)) f |= 32; }
        for (int bx = 0; bx < tx; bx++)
            for (int qc = 0; qc < nsub; qc += fusedSub) {
                const int qe = std::min(qc + fusedSub, nsub), L = qe - qc;
                int by = 0;
                while (by + FRW <= ty) {
                    // class of the three rows at every q of the chunk: -1 = not available, else bit0 UNI, bit1 lossy
                    std::vector<int> cls(L, -1);
                    for (int q = qc; q < qe; q++) {
                        bool ok = true; int uni = 1, lossy = 0;
                        const int m0 = mats[(size_t)q * layer + (size_t)by * tx + bx];
                        for (int r = 0; r < FRW; r++) {
                            const size_t id = (size_t)q * layer + (size_t)(by + r) * tx + bx;
                            const int f = flags[id];
                            if (!(f & 32) || taken[id]) ok = false;
                            if (!(f & 4) || mats[id] != m0) uni = 0;
                            if (f & 128) lossy = 1;
                        }
                        if (!uni && s->cfg.nMat > bfd_fused_max_materials()) ok = false;
                        if (ok) cls[q - qc] = uni | (lossy << 1);
                    }
                    bool any = false;
                    int a = 0;
                    while (a < L) {
                        if (cls[a] < 0) { a++; continue; }
                        int b = a; while (b < L && cls[b] >= 0) b++;        // stretch [a, b)
                        if (b - a >= 2) {
                            any = true;
                            // segments of equal class (start, end, class); a segment of one sub-tile joins a neighbour
                            std::vector<std::array<int, 3>> seg;
                            for (int q = a; q < b; q++) {
                                if (seg.empty() || seg.back()[2] != cls[q]) seg.push_back({q, q + 1, cls[q]});
                                else seg.back()[1] = q + 1;
                            }
                            for (size_t u = 0; u < seg.size() && seg.size() > 1;) {
                                if (seg[u][1] - seg[u][0] >= 2) { u++; continue; }
                                const size_t v = u > 0 ? u - 1 : u + 1;      // UNI only if both are, lossy if either is
                                seg[v][0] = std::min(seg[v][0], seg[u][0]); seg[v][1] = std::max(seg[v][1], seg[u][1]);
                                seg[v][2] = (seg[v][2] & seg[u][2] & 1) | ((seg[v][2] | seg[u][2]) & 2);
                                seg.erase(seg.begin() + u);
                                u = 0;
                            }
                            for (const auto &rq : seg) {
                                fruns.push_back({bx, by, qc + rq[0], qc + rq[1], rq[2], mats[(size_t)(qc + rq[0]) * layer + (size_t)by * tx + bx]});
                                for (int q = qc + rq[0]; q < qc + rq[1]; q++)
                                    for (int r = 0; r < FRW; r++) { taken[(size_t)q * layer + (size_t)(by + r) * tx + bx] = 1; s->tiles.nFusedSub++; }
                            }
                        }
                        a = b;
                    }
                    by += any ? FRW : 1;
                }
            }
        // list order like the other runs: eight y-bands, inside a band z-chunk slowest, then row, bx fastest
        auto key = [&](const FusedRun &r) { const long band = (long)r.by * 8 / ty; return ((band * 4096 + r.q0 / fusedSub) * 4096 + r.by) * 4096 + r.bx; };
        std::stable_sort(fruns.begin(), fruns.end(), [&](const FusedRun &x, const FusedRun &y) { return key(x) < key(y); });
        for (const auto &r : fruns) {
            int4 run; run.x = r.by * tx + r.bx; run.y = (r.q0 * SUB) | (std::min(r.q1 * SUB, s->d.nk) << 16);
            run.z = 32 | 16 | ((r.cls & 2) ? 2 : 0) | ((r.cls & 1) ? 4 : 0); run.w = r.mat;
            fused.push_back(run);
        }
    }
}

// The runs of the two-kernel path: fluid boundary / interior (lists[0], [1]), solid boundary / interior (lists[2], [3]) and all of them in list
// order (listsAll: boundary, interior); sub-tiles the fused runs have taken are left out.
static void form_two_kernel_runs(bfd_sim *s, const TileGrid &G, const std::vector<int> &flags, const std::vector<int> &mats, std::vector<char> &taken, std::vector<int4> *lists, std::vector<int4> *listsAll)
{
    const int tx = G.tx, ty = G.ty, nsub = G.nsub, SUB = G.SUB, perChunk = G.perChunk, nChunks = G.nChunks;
    bfd_tiles &T = s->tiles;
    // List order = what is in flight together. The launch gives XCD e the e-th contiguous eighth of the list
    // (remap_block) and an XCD keeps ~100 workgroups in flight, all marching in z at the same pace; a halo line
    // (128 B for 2 or 3 floats of a neighbour tile's row) is an L2 hit only if that neighbour is in flight on the
    // same XCD. Default (2): eight y-bands, inside a band z-chunk slowest, then by, bx fastest -> x neighbours are
    // 1 apart, y neighbours tilesX apart. Measured at 512^3 (rocprofv3 FETCH/WRITE_SIZE, water): stress traffic
    // 3.55 -> 3.10 GB and 79 -> 88 Gvoxel-steps/s against (0) column order (z-chunks of a column consecutive);
    // (1) z-chunk slowest over the whole plane moves as few bytes but piles the absorbing-layer and lossy
    // z-levels onto single XCDs (C3: 75 -> 72). BFD_RUN_ORDER=0/1 select the other orders for experiments.
    std::vector<std::pair<int, int>> seq;       // (column, z-chunk) in list order
    {
        const char *ev = getenv("BFD_RUN_ORDER");
        const int mode = ev ? atoi(ev) : 2;
        if (mode == 1) {            // z-chunk slowest
            for (int c = 0; c < nChunks; c++) for (int txy = 0; txy < tx * ty; txy++) seq.push_back({txy, c});
        } else if (mode == 0) {     // column order
            for (int txy = 0; txy < tx * ty; txy++) for (int c = 0; c < nChunks; c++) seq.push_back({txy, c});
        } else {                    // 8 y-bands (one per XCD part), inside a band z-chunk slowest
            // (the two z-chunks of the absorbing layer first, so that the cheapest workgroups end every XCD's part of the list: no gain, removed;
            // profiles/r4/)
            for (int e = 0; e < 8; e++) {
                const int y0 = (int)((long)ty * e / 8), y1 = (int)((long)ty * (e + 1) / 8);
                for (int c = 0; c < nChunks; c++) for (int by = y0; by < y1; by++) for (int bx = 0; bx < tx; bx++) seq.push_back({by * tx + bx, c});
            }
        }
    }
    for (const auto &pc : seq) {
        const int txy = pc.first, c = pc.second;
        const int sb = c * perChunk, se0 = std::min(sb + perChunk, nsub);
        int q = sb;
        while (q < se0) {
            if (taken[(size_t)q * tx * ty + txy]) { q++; continue; }
            const int f = flags[(size_t)q * tx * ty + txy], m = mats[(size_t)q * tx * ty + txy];
            const bool solid = f & 1;
            const bool bnd = G.subBnd(q);
            int r = q + 1, pmlAny = f & 8;
            while (r < se0) {
                const int f2 = flags[(size_t)r * tx * ty + txy], m2 = mats[(size_t)r * tx * ty + txy];
                if (G.subBnd(r) != bnd || taken[(size_t)r * tx * ty + txy]) break;
                if (solid ? !(f2 & 1) : (((f2 ^ f) & ~(32 | 128 | 256)) != 0 || ((f & 4) && m2 != m))) break;
                pmlAny |= f2 & 8;
                r++;
            }
            const int kbeg = q * SUB, kend = std::min(r * SUB, s->d.nk);
            // solid runs: bit0 + bit3 (a sub-tile of the run touches the absorbing layer)
            int4 run; run.x = txy; run.y = kbeg | (kend << 16); run.z = solid ? (1 | pmlAny) : (f & ~(32 | 128 | 256)); run.w = m;
            lists[(solid ? 2 : 0) + (bnd ? 0 : 1)].push_back(run);
            listsAll[bnd ? 0 : 1].push_back(run);
            for (int u = q; u < r; u++) {
                taken[(size_t)u * tx * ty + txy] = 1;
                if (solid) T.nSolidSub++;
                else { if (f & 2) T.nLossy++; else T.nLossless++; if (f & 4) T.nUni++; if (f & 8) T.nPml++; if (f & 16) T.nLean++; }
            }
            q = r;
        }
    }
    // solid runs that touch the absorbing layer go to the two ends of the solid list: [boundary: PML | plain][interior: plain | PML]
    auto isPml = [](const int4 &r) { return (r.z & 8) != 0; };
    auto mid = std::stable_partition(lists[2].begin(), lists[2].end(), isPml);
    T.nSolidBP = (int)(mid - lists[2].begin());
    auto mid2 = std::stable_partition(lists[3].begin(), lists[3].end(), [&](const int4 &r) { return !isPml(r); });
    T.nSolidIP = (int)(lists[3].end() - mid2);
}

// Cost-balanced block -> run maps (experiment, BFD_XCD_BALANCE=1; default off). A launch's blocks go to the 8 XCDs round-robin and every
// XCD works through its own blocks at its own pace (-DBFD_EXP_XCD_CLOCK build: block b always runs on XCD (x0 + b) mod 8). With equal
// COUNTS per XCD (remap_block) the XCD that holds the short boundary runs is idle for the last fifth of every fluid launch and the bands
// with more tissue finish last. Here the contiguous parts of the list are cut by estimated cost instead (planes + prologue, weighted by
// the bytes per cell of the run's class), the launch gets 8 x (longest part) blocks and a block beyond its part returns at once.
// Measured: the ends of the XCDs move together (spread 19 % -> 13 % of a launch) and the step time does not -- C3 +1.2 %, shear medium
// -0.4 %, other weightings +-2 % either way: an XCD that runs dry leaves its share of the memory system to the others.
// profiles/r4/xcd_balance.txt.
static int build_balance_maps(bfd_sim *s, const std::vector<int4> &all)
{
    bfd_tiles &T = s->tiles;
    bool on = false;
    if (const char *ev = getenv("BFD_XCD_BALANCE")) on = atoi(ev) != 0 && s->cfg.kernelVariant != 2 && s->cfg.kernelVariant != 1;
    memset(s->tiles.xmapH, 0, sizeof s->tiles.xmapH);
    if (on) {
        const double wPml = 0.25, wLossy = 8, wMulti = 2, wRun = 2.0;
        // cost of run r for kernel class c: 0 fluid stress, 1 fluid velocity, 2 solid stress, 3 solid velocity
        auto cost = [&](const int4 &r, int c) {
            const double planes = (double)((r.y >> 16) - (r.y & 0xFFFF)) + wRun;
            const int f = r.z;
            double w;
            if (c == 0) w = 20 + ((f & 2) ? wLossy : 0) + ((f & 4) ? 0 : wMulti);
            else if (c == 1) w = 36 + ((f & 4) ? 0 : wMulti);
            else w = 40;
            if (f & 8) w *= 1.0 + wPml;
            return planes * w;
        };
        auto make = [&](int m, size_t a0, size_t a1, int c) {
            int *seg = s->tiles.xmapH[m];
            const size_t n = a1 > a0 ? a1 - a0 : 0;
            std::vector<double> cum(n + 1, 0.0);
            for (size_t i = 0; i < n; i++) cum[i + 1] = cum[i] + cost(all[a0 + i], c);
            int maxcnt = 0;
            seg[0] = 0;
            for (int x = 1; x <= 8; x++) {
                const double target = cum[n] * x / 8.0;
                size_t j = std::lower_bound(cum.begin(), cum.end(), target) - cum.begin();
                if (j > n || x == 8) j = n;
                if ((int)j < seg[x - 1]) j = seg[x - 1];
                seg[x] = (int)j;
                maxcnt = std::max(maxcnt, seg[x] - seg[x - 1]);
            }
            seg[9] = std::max(maxcnt, 1);
        };
        const size_t F = T.nFluid, FB = T.nFluidB, S0 = F, SB = T.nSolidB, SN = T.nSolid;
        for (int c = 0; c < 2; c++) {            // fluid stress (c = 0), fluid velocity (c = 1): parts 0, 1, 2
            const int m = c == 0 ? BFD_XM_SF : BFD_XM_VF;
            make(m + 0, 0, F, c); make(m + 1, 0, FB, c); make(m + 2, FB, F, c);
        }
        make(BFD_XM_SS + 0, S0, S0 + SN, 2); make(BFD_XM_SS + 1, S0, S0 + SB, 2); make(BFD_XM_SS + 2, S0 + SB, S0 + SN, 2);
        const size_t bp = T.nSolidBP, ip = T.nSolidIP;          // solid list = [boundary: PML | plain][interior: plain | PML]
        make(BFD_XM_VS + 0, S0 + bp, S0 + SN - ip, 3); make(BFD_XM_VS + 1, S0 + bp, S0 + SB, 3); make(BFD_XM_VS + 2, S0 + SB, S0 + SN - ip, 3);
        make(BFD_XM_VSP_LO, S0, S0 + bp, 3); make(BFD_XM_VSP_HI, S0 + SN - ip, S0 + SN, 3);
        make(BFD_XM_FUSED, S0 + SN, S0 + SN + T.nFused, 0);
        const int rc = dev_alloc(s, &s->tiles.xmap, (size_t)BFD_XMAP_COUNT * 10, false);
        if (rc) return rc;
        BFD_HIP(hipMemcpy(s->tiles.xmap, s->tiles.xmapH, sizeof s->tiles.xmapH, hipMemcpyHostToDevice));
    }
    return 0;
}

// sparse shear list: cells with a solid centre, ascending index (hostCells), in list order on the device, + their edge coefficients;
// decides whether the solid state is compact
static int build_shear_list(bfd_sim *s, const TileGrid &G, int *countOut, bool *compactOut, std::vector<unsigned> &hostCells)
{
    DevTemp<unsigned char> flag; DevTemp<unsigned> sel; DevTemp<int> dcount; DevTemp<char> work;
    hipError_t e = flag.alloc(s->nloc);
    if (e == hipSuccess) e = sel.alloc(s->nloc);
    if (e == hipSuccess) e = dcount.alloc(1);
    int count = 0, rc = 0;
    if (e == hipSuccess) {
        bfd_launch_mark_solid(s->d, s->stream, flag, (long)s->nloc);
        e = select_flagged(flag, sel, dcount, (int)s->nloc, s->stream, work);
        if (e == hipSuccess) e = hipMemcpyAsync(&count, dcount, sizeof(int), hipMemcpyDeviceToHost, s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    }
    hostCells.resize((size_t)count);
    if (e == hipSuccess && count) e = hipMemcpy(hostCells.data(), sel, (size_t)count * sizeof(unsigned), hipMemcpyDeviceToHost);
    // list order (bfd_kernels_shear.hip, shear_order_keys): by z-chunk and band of 8 rows, so that the z neighbours a cell gathers were
    // touched one band-plane earlier instead of one whole plane of the shell
    if (e == hipSuccess && count > 0) {
        DevTemp<unsigned long long> k0, k1; DevTemp<unsigned> v1; DevTemp<char> w2; size_t w2b = 0;
        e = k0.alloc((size_t)count);
        if (e == hipSuccess) e = k1.alloc((size_t)count);
        if (e == hipSuccess) e = v1.alloc((size_t)count);
        if (e == hipSuccess) {
            bfd_launch_shear_order_keys(s->d, s->stream, sel, k0, count, G.lowPlanes, G.hiStart);
            e = hipcub::DeviceRadixSort::SortPairs(nullptr, w2b, k0.p, k1.p, sel.p, v1.p, count, 0, 46, s->stream);
        }
        if (e == hipSuccess) e = w2.alloc(std::max<size_t>(w2b, 1));
        if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs((void *)w2.p, w2b, k0.p, k1.p, sel.p, v1.p, count, 0, 46, s->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(sel, v1, (size_t)count * 4, hipMemcpyDeviceToDevice, s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    }
    // Compact solid state (bfd_dev::cssRow): Sxx, Syy, the shear stresses and the five memory variables Rxx, Ryy, Rxy, Rxz, Ryz of the listed cells in
    // list order. Needs the row-contiguous list order. In a Z-slab the ghost planes of Sxz / Syz stay in the
    // full-volume arrays (the sparse kernel keeps full-volume copies of the planes a neighbour reads, the velocity kernel takes ghost planes from
    // there): the halo exchange is unchanged. BFD_COMPACT_SOLID=0 keeps the full-volume arrays.
    bool compact = count > 0 && s->d.N1 <= 4095;
    if (const char *ev = getenv("BFD_COMPACT_SOLID")) compact = compact && atoi(ev) != 0;
    if (e == hipSuccess) {
        rc = dev_alloc(s, &s->tiles.shearCells, (size_t)std::max(count, 1), false);
        if (!rc) rc = dev_alloc(s, &s->tiles.shearCoef, 6 * (size_t)std::max(count, 1), false);
        if (!rc && !compact) rc = dev_alloc(s, &s->tiles.shearR, 3 * (size_t)std::max(count, 1), true);      // lists are built at step 0: the memory variables start at zero (compact form: they are among the compact arrays)
        if (!rc && count) e = hipMemcpyAsync(s->tiles.shearCells, sel, (size_t)count * sizeof(unsigned), hipMemcpyDeviceToDevice, s->stream);
        if (!rc) rc = dev_alloc(s, &s->tiles.shearCodes, (size_t)std::max(count, 1), false);
        if (!rc) rc = dev_alloc(s, &s->tiles.shearTab, 8 * (size_t)s->cfg.nMat, false);
        if (!rc && e == hipSuccess) bfd_launch_shear_coefficients(s->d, s->stream, s->tiles.shearCells, s->tiles.shearCoef, s->tiles.shearCodes, s->tiles.shearTab, s->cfg.nMat, count);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    }
    if (e != hipSuccess) BFD_FAIL(-10, std::string("shear list: ") + hipGetErrorString(e));
    if (rc) return rc;
    s->tiles.nShear = count;
    if (s->step > 0 && s->tiles.shearR) { bfd_launch_gather_shear_memory(s->d, s->stream, &s->tiles); BFD_HIP(hipStreamSynchronize(s->stream)); }
    *countOut = count; *compactOut = compact;
    return 0;
}

// compact solid state: the row table, the ten arrays (hosted in the full-volume buffers or in a block of their own) and the combined run list
static int setup_compact_state(bfd_sim *s, const TileGrid &G, int count, const std::vector<int4> *listsAll)
{
    const int stride = G.tx + 1;
    int rc = dev_alloc(s, &s->tiles.cssRow, (size_t)(s->d.nk + 4) * s->d.N2 * stride, false);
    // the compact arrays live inside the full-volume buffers of their fields when the listed cells fit between the planes a Z-neighbour
    // exchanges (local planes 0, 1 and nk-2, nk-1 of Sxz / Syz travel: allocation planes 4 .. nk-1 are free); BFD_COMPACT_HOSTED=0 or
    // too many solid cells: one block of their own
    bool hosted = (size_t)count <= (size_t)std::max(s->d.nk - 4, 0) * s->d.plane;
    if (const char *ev = getenv("BFD_COMPACT_HOSTED")) hosted = hosted && atoi(ev) != 0;
    if (!rc && !hosted) rc = dev_alloc(s, &s->tiles.css, 10 * (size_t)count, true);
    if (rc) return rc;
    s->tiles.cssCap = count; s->tiles.cssHosted = hosted;
    bfd_launch_css_row_table(s->d, s->stream, s->tiles.shearCells, count, s->tiles.cssRow, stride, G.lowPlanes, G.hiStart);
    s->d.cssRow = s->tiles.cssRow; s->d.cssStride = stride;
    bind_compact_views(s);
    BFD_HIP(hipStreamSynchronize(s->stream));
    std::vector<int4> ra(listsAll[0]);
    ra.insert(ra.end(), listsAll[1].begin(), listsAll[1].end());
    rc = dev_alloc(s, &s->tiles.runsAll, ra.size(), false);
    if (rc) return rc;
    BFD_HIP(hipMemcpy(s->tiles.runsAll, ra.data(), ra.size() * sizeof(int4), hipMemcpyHostToDevice));
    s->tiles.nAllB = (int)listsAll[0].size(); s->tiles.nAll = (int)ra.size();
    return 0;
}

// a compact state set aside before a rebuild in the middle of a run: the values of the old list into the new one (or, should the new state not be compact -- the
// form was switched off, or no solid run is left and build_tile_lists calls with count 0 -- into the full-volume arrays)
static int carry_compact_in(bfd_sim *s, int count, const unsigned *oldCells, long oldN, const float *oldComp)
{
    DevTemp<float> tmp(true);
    const size_t g = 2 * (size_t)s->d.plane;
    float *newComp[10] = {s->d.cSxx, s->d.cSyy, s->d.cSxy, s->d.cSxz, s->d.cSyz, s->d.cRxx, s->d.cRyy, s->d.cRxy, s->d.cRxz, s->d.cRyz};
    float *full[10] = {s->d.Sxx, s->d.Syy, s->d.Sxy, s->d.Sxz, s->d.Syz, s->d.Rxx, s->d.Ryy, s->d.Rxy, s->d.Rxz, s->d.Ryz};
    hipError_t e2 = s->d.cssRow ? tmp.alloc(s->nalloc) : hipSuccess;
    // the new state is not compact (no solid cell left, or the form was switched off): the full-volume arrays take over, and the owned planes
    // of buffers that hosted compact arrays hold list-ordered values, not fields: cleared before the old values are scattered into them
    for (int a = 0; a < 10 && e2 == hipSuccess && !s->d.cssRow; a++) e2 = hipMemsetAsync(full[a], 0, s->nloc * sizeof(float), s->stream);
    for (int a = 0; a < 10 && e2 == hipSuccess; a++) {
        if (s->d.cssRow) {
            e2 = hipMemsetAsync(tmp, 0, s->nalloc * sizeof(float), s->stream);
            bfd_launch_css_scatter(s->stream, oldCells, oldN, oldComp + (size_t)a * oldN, tmp + g);
            bfd_launch_css_gather(s->stream, s->tiles.shearCells, count, tmp + g, newComp[a]);
        } else bfd_launch_css_scatter(s->stream, oldCells, oldN, oldComp + (size_t)a * oldN, full[a]);
    }
    if (e2 == hipSuccess) e2 = hipStreamSynchronize(s->stream);
    if (e2 != hipSuccess) BFD_FAIL(-10, std::string("compact solid state, list rebuilt in the middle of a run: ") + hipGetErrorString(e2));
    if (!s->d.cssRow && s->tiles.shearR) { bfd_launch_gather_shear_memory(s->d, s->stream, &s->tiles); BFD_HIP(hipStreamSynchronize(s->stream)); }
    return 0;
}

// algorithmic bytes per launch and kernel class (DESIGN.md "Kernels": per-cell byte tables of the tile classes):
// what each kernel has to move once per half-step if every value were fetched exactly once -- float32 fields 4 B,
// material ids 2 B; absorbing-layer memory variables, tables and halo re-reads excluded
static int account_algorithmic_bytes(bfd_sim *s, int tx, const std::vector<int4> &all)
{
    bfd_tiles &T = s->tiles;
    double (*B)[BFD_K_COUNT] = s->algBytes;
    memset(s->algBytes, 0, sizeof s->algBytes);
    const int N1 = s->d.N1, N2 = s->d.N2, N3 = s->d.N3, ND = s->d.ND, k0g = s->d.k0;
    // class counts over the cells of the solid runs (fluid / solid centre, with / without memory variables, active edges)
    unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
    if (T.nSolid && s->cfg.kernelVariant != 2) {
        DevTemp<unsigned long long> dc;
        BFD_HIP(dc.alloc(6));
        hipMemsetAsync(dc, 0, sizeof cnt, s->stream);
        bfd_launch_count_solid_cells(s->d, s->stream, s->tiles.runs + T.nFluid, T.nSolid, dc);
        hipMemcpyAsync(cnt, dc, sizeof cnt, hipMemcpyDeviceToHost, s->stream);
        const hipError_t e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) BFD_FAIL(-10, std::string("solid cell counts: ") + hipGetErrorString(e));
    }
    auto overlap = [](int a, int b, int lo, int hi) { return (double)std::max(0, std::min(b, hi) - std::max(a, lo)); };
    const bool pairAcc = pair_engine(s, quiet_runs_wanted(s), T.nFluid);      // the predicate the launches follow (pairing_step)
    for (size_t r = 0; r < all.size(); r++) {
        const int4 &run = all[r];
        const int bx = run.x % tx, by = run.x / tx, kb = run.y & 0xFFFF, ke = run.y >> 16, f = run.z;
        const int xa = bx * 64, xb = std::min(xa + 64, N1), ya = by * 8, yb = std::min(ya + 8, N2);
        const double cells = (double)(xb - xa) * (yb - ya) * (ke - kb);
        const double inner = overlap(xa, xb, ND, N1 - ND) * overlap(ya, yb, ND, N2 - ND) * overlap(k0g + kb, k0g + ke, ND, N3 - ND);
        const bool fusedRun = r >= (size_t)(T.nFluid + T.nSolid);
        if (fusedRun) {          // 64 x 24 cells per plane, all outside the absorbing layer: V, Szz (Rzz) read and written once per step (+ ids)
            const double fc = 64.0 * bfd_fused_rows() * (ke - kb);
            const double b = 32.0 + ((f & 2) ? 8.0 : 0.0) + ((f & 4) ? 0.0 : 2.0);
            B[0][BFD_K_FUSED] += b * fc; B[1][BFD_K_FUSED] += b * fc + 8.0 * fc;
        } else if (r < (size_t)T.nFluid) {
            const bool lossy = f & 2, uni = f & 4, single = (f & 16) != 0;
            double bs = 12.0 + 8.0 + (lossy ? 8.0 : 0.0) + (uni ? 0.0 : 2.0);
            if (!single) bs += 8.0 + (lossy ? 8.0 : 0.0);
            const double bv = 4.0 + 24.0 + (uni ? 0.0 : 2.0);
            for (int a = 0; a < 2; a++) { B[a][BFD_K_STRESS_FLUID] += bs * cells; B[a][BFD_K_VELOCITY_FLUID] += bv * cells; }
            // Pressure sum read and written: by velocity_fluid in every accumulating step, or (paired accumulation) by stress_fluid in
            // every second one: 4 B per launch averaged over a step pair
            if (pairAcc) B[1][BFD_K_STRESS_FLUID] += 4.0 * inner; else B[1][BFD_K_VELOCITY_FLUID] += 8.0 * inner;
            // advanced Vz: planes kbeg+1 .. kend-3 of the run get their new Vz from stress_fluid (a write; the read is in its 12 B of V already)
            // and velocity_fluid neither reads nor writes it there
            if (f & BFD_RUN_ADV_VZ) {
                const double advCells = (double)(xb - xa) * (yb - ya) * std::max(0, ke - kb - 3);
                for (int a = 0; a < 2; a++) { B[a][BFD_K_STRESS_FLUID] += 4.0 * advCells; B[a][BFD_K_VELOCITY_FLUID] -= 8.0 * advCells; }
            }
        } else if (s->cfg.kernelVariant == 2) {     // dense: V + 6 S + 6 R read, 6 S + 6 R written, id; 6 S + V read, V written, id
            for (int a = 0; a < 2; a++) { B[a][BFD_K_STRESS_SOLID] += 110.0 * cells; B[a][BFD_K_VELOCITY_SOLID] += 50.0 * cells + (a ? 8.0 * inner : 0.0); }
        } else {                                    // class-predicated solid kernels: per-cell terms come from the class counts below
            for (int a = 0; a < 2; a++) B[a][BFD_K_VELOCITY_SOLID] += (a ? 8.0 * inner : 0.0);
        }
    }
    if (T.nSolid && s->cfg.kernelVariant != 2) {
        // stress: V 12 + id 2 + class 1, + Szz r/w 8 (+ Rzz r/w 8) at a fluid cell, + 3 S r/w 24 + 3 R r/w 24 at a solid one
        // (a reflector cell: 48 B of zero stores); velocity: V r/w 24 + ids 2 + class 1 + Szz 4, + Sxx, Syy 8 at a solid cell,
        // + 4 per active shear edge
        const double nF0 = (double)cnt[0], nF1 = (double)cnt[1], nS = (double)cnt[2] + (double)cnt[3], nE = (double)cnt[4], nR = (double)cnt[5];
        const double all = nF0 + nF1 + nS + nR;
        const double bs = 15.0 * all + 8.0 * nF0 + 16.0 * nF1 + 48.0 * nS + 48.0 * nR;
        const double bv = 31.0 * all + 8.0 * (nS + nR) + 4.0 * nE;
        // compact solid state: the fluid kernel takes Szz / Rzz of the solid runs too (V 12 + id 2, + Szz r/w 8 (+ Rzz r/w 8); no class byte), the
        // sparse kernel Sxx, Syy, Rxx, Ryy of its cells (+ 32 + id 2 per listed cell, below)
        const double bsf = 14.0 * all + 8.0 * nF0 + 16.0 * nF1 + 16.0 * nS + 8.0 * nR;
        for (int a = 0; a < 2; a++) { if (s->d.cssRow) B[a][BFD_K_STRESS_FLUID] += bsf; else B[a][BFD_K_STRESS_SOLID] += bs; B[a][BFD_K_VELOCITY_SOLID] += bv; }
    }
    if (s->tiles.nShear) {       // sparse shear: cell index + 6 coefficients + V of the cell + read-modify-write of S and R per active edge
        DevTemp<unsigned long long> dc; unsigned long long hc[2] = {0, 0};
        BFD_HIP(dc.alloc(2));
        hipMemsetAsync(dc, 0, sizeof hc, s->stream);
        hipLaunchKernelGGL(count_active_edges, dim3(grid_for(s->tiles.nShear)), dim3(256), 0, s->stream, s->tiles.shearCoef, s->tiles.shearCodes, s->tiles.nShear, dc.p);
        hipMemcpyAsync(hc, dc, sizeof hc, hipMemcpyDeviceToHost, s->stream);
        const hipError_t e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) BFD_FAIL(-10, std::string("shear edge count: ") + hipGetErrorString(e));
        s->tiles.nShearExplicit = (long)hc[1];
        // per listed cell: index 4 + edge codes 4 + V 12; per edge with explicit coefficients 8; per active edge S and R r/w 16; compact solid
        // state: + Sxx, Syy, Rxx, Ryy r/w 32 (+ the cell's id 2 when it does not fit the code word's fourth byte)
        const double perCell = s->d.cssRow ? (s->cfg.nMat <= 255 ? 52.0 : 54.0) : 20.0;
        for (int a = 0; a < 2; a++) B[a][BFD_K_STRESS_SHEAR] = perCell * (double)s->tiles.nShear + 8.0 * (double)hc[1] + 16.0 * (double)hc[0];
    }
    return 0;
}

// ---- advanced Vz -----------------------------------------------------------------------------------------------------------
// velocity_fluid reads and writes Vz (8 B per cell), yet its Vz update needs only the column's new Szz, which stress_fluid produces plane by plane
// while it holds the column's Vz in its z-queue. In a plain fluid run outside the absorbing layer stress_fluid therefore stores the new Vz of
// the planes whose stencil lies inside the run (kbeg+1 .. kend-3; the range proof is at stress_fluid_body) and velocity_fluid skips Vz there:
// + 4 B and - 8 B per advanced cell. The same expression in the same order (-ffp-contract=off): bit-identical. BFD_ADV_VZ=0 switches it off.
// ONE bit in the run record (BFD_RUN_ADV_VZ), set here when the lists are built, tells both kernels; they cannot disagree. An engine qualifies with
// the class-specialised kernels (variants 0 / 3) updating V in place, velocity-type sources (a stress-type source changes Szz between the two
// kernels), no solid run (velocity_solid and the sparse kernel read their fluid neighbours' Vz) and no quiet runs (those flavours ignore the bit).
// Z-slabs qualify: the planes a neighbour's stress half-step reads are a slab's first and last two, never inner planes of a run.
// Between the two half-steps of a step Vz is of mixed time level (bfd_sim::midStep): the setters that would rebuild the lists refuse until the step ends.
static bool adv_vz_engine(const bfd_sim *s, int nSolid)          // run lists just formed
{
    return s->advEnv && class_kernels_in_place(s) && s->d.VzW == s->d.Vz &&
           s->cfg.typeSource < 2 && nSolid == 0 && !quiet_runs_wanted(s);
}

// Build the run lists of the tiled kernels (bfd_kernels_fluid / _solid / _dense.hip; their order: bfd_kernels_tiled.hip). Sub-tiles of 64 x 8 x 8 cells are
// classified on the device; consecutive sub-tiles of one (bx,by) column with identical class merge into
// runs that never cross a 32-plane chunk boundary. Variant 2: every sub-tile counts as solid (dense kernels).
int build_tile_lists(bfd_sim *s)
{
    // a list rebuilt in the middle of a run (inputs set again at step > 0): the shear memory variables travel through the
    // full-volume arrays
    const bool carryShearMemory = s->step > 0 && s->tilesReady == false && s->tiles.shearR && s->tiles.nShear > 0;
    if (carryShearMemory) { bfd_launch_scatter_shear_memory(s->d, s->stream, &s->tiles); BFD_HIP(hipStreamSynchronize(s->stream)); }
    // the same for a compact solid state: its ten arrays are set aside with their list (the full-volume buffers may host the compact arrays
    // themselves) and re-entered into the new list through one full-volume temporary, array by array, once that list exists
    const bool carryCompact = s->step > 0 && s->d.cssRow && s->tiles.nShear > 0;
    unsigned *oldCells = nullptr; DevTemp<float> oldComp; const long oldN = s->tiles.nShear;
    if (carryCompact) {
        float *src[10] = {s->d.cSxx, s->d.cSyy, s->d.cSxy, s->d.cSxz, s->d.cSyz, s->d.cRxx, s->d.cRyy, s->d.cRxy, s->d.cRxz, s->d.cRyz};
        BFD_HIP(oldComp.alloc(10 * (size_t)oldN));
        for (int a = 0; a < 10; a++) BFD_HIP(hipMemcpyAsync(oldComp + (size_t)a * oldN, src[a], (size_t)oldN * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
        BFD_HIP(hipStreamSynchronize(s->stream));
        oldCells = s->tiles.shearCells; s->tiles.shearCells = nullptr;       // released below, after the new list has taken the values over
    }
    s->sensEntValid = false;
    s->d.cssRow = nullptr; s->d.cSxx = s->d.cSyy = s->d.cSxy = s->d.cSxz = s->d.cSyz = s->d.cRxx = s->d.cRyy = s->d.cRxy = s->d.cRxz = s->d.cRyz = nullptr;
    dev_release(s, &s->tiles.cssRow); dev_release(s, &s->tiles.css); s->tiles.cssCap = 0; s->tiles.cssHosted = false;
    dev_release(s, &s->tiles.runsAll); s->tiles.nAll = s->tiles.nAllB = 0;
    dev_release(s, &s->tiles.runs); dev_release(s, &s->tiles.xmap); dev_release(s, &s->tiles.shearCells); dev_release(s, &s->tiles.shearCoef); dev_release(s, &s->tiles.shearR);    // lists of an earlier build
    dev_release(s, &s->tiles.shearCodes); dev_release(s, &s->tiles.shearTab);
    const TileGrid G = choose_tile_grid(s);
    std::vector<int> flags(G.n, 1), mats(G.n, 0);
    if (s->cfg.kernelVariant != 2) { const int rc = fetch_tile_classes(s, G.n, flags, mats); if (rc) return rc; }
    bfd_tiles &T = s->tiles;
    T.nMat = s->cfg.nMat;
    T.nFluid = T.nFluidB = T.nSolid = T.nSolidB = T.nSolidBP = T.nSolidIP = T.nFused = T.nLossless = T.nLossy = T.nSolidSub = T.nUni = T.nPml = T.nLean = T.nFusedSub = 0;
    s->d.tilesX = G.tx; s->d.tilesY = G.ty;
    // Every fluid sub-tile is LEAN (bit4): fluid cells keep a single copy of their identical normal stresses, whatever
    // tile they sit in and whatever reads them (bfd_dev::cls)
    if (s->cfg.kernelVariant != 2) for (int id = 0; id < G.n; id++) if (!(flags[id] & 1)) flags[id] |= 16;
    std::vector<int4> lists[5];      // fluid boundary, fluid interior, solid boundary, solid interior, fused fluid
    std::vector<int4> listsAll[2];   // every run of the two-kernel path in list order: boundary, interior (bfd_tiles::runsAll)
    std::vector<char> taken((size_t)G.n, 0);
    form_fused_runs(s, G, flags, mats, taken, lists[4]);
    form_two_kernel_runs(s, G, flags, mats, taken, lists, listsAll);
    T.nFluidB = (int)lists[0].size(); T.nFluid = T.nFluidB + (int)lists[1].size();
    T.nSolidB = (int)lists[2].size(); T.nSolid = T.nSolidB + (int)lists[3].size();
    T.nFused = (int)lists[4].size();
    T.advVz = false;
    if (adv_vz_engine(s, T.nSolid))
        for (int a = 0; a < 2; a++)
            for (int4 &run : lists[a])
                if (!(run.z & (1 | 8)) && (run.y >> 16) - (run.y & 0xFFFF) >= 4) { run.z |= BFD_RUN_ADV_VZ; T.advVz = true; }
    std::vector<int4> all;
    for (int a = 0; a < 5; a++) all.insert(all.end(), lists[a].begin(), lists[a].end());
    int rc = dev_alloc(s, &s->tiles.runs, all.size(), false);
    if (rc) return rc;
    BFD_HIP(hipMemcpy(s->tiles.runs, all.data(), all.size() * sizeof(int4), hipMemcpyHostToDevice));
    rc = build_balance_maps(s, all);
    if (rc) return rc;
    s->tiles.nShearExplicit = 0;
    s->tiles.nShear = s->tiles.shearLowEnd = s->tiles.shearHighBeg = 0;
    if (T.nSolid && s->cfg.kernelVariant != 2) {     // variant 2 stays monolithic and fully dense
        int count = 0; bool compact = false; std::vector<unsigned> hostCells;
        rc = build_shear_list(s, G, &count, &compact, hostCells);
        if (!rc && compact) rc = setup_compact_state(s, G, count, listsAll);
        if (!rc && carryCompact) rc = carry_compact_in(s, count, oldCells, oldN, oldComp);
        if (!rc && compact && s->step > 0 && !carryCompact) {
            // the first solid cells of a run in progress (they may only appear where every field is zero, include/babelfdtd.h): the compact arrays
            // start at zero. Hosted, they lie in full-volume buffers that an all-fluid engine uses as output scratch (expand_if_collapsed).
            float *comp[10] = {s->d.cSxx, s->d.cSyy, s->d.cSxy, s->d.cSxz, s->d.cSyz, s->d.cRxx, s->d.cRyy, s->d.cRxy, s->d.cRxz, s->d.cRyz};
            for (int a = 0; a < 10; a++) BFD_HIP(hipMemsetAsync(comp[a], 0, (size_t)count * sizeof(float), s->stream));
            BFD_HIP(hipStreamSynchronize(s->stream));
        }
        if (rc) return rc;
        s->tiles.shearLowEnd = std::lower_bound(hostCells.begin(), hostCells.end(), (unsigned)G.lowPlanes * (unsigned)s->d.plane) - hostCells.begin();
        s->tiles.shearHighBeg = std::lower_bound(hostCells.begin(), hostCells.end(), (unsigned)G.hiStart * (unsigned)s->d.plane) - hostCells.begin();
    } else if (carryCompact) {                       // no solid run is left: the full-volume arrays take the old compact values back
        rc = carry_compact_in(s, 0, oldCells, oldN, oldComp);
        if (rc) return rc;
    }
    {   // sources of the first / last z-chunk (bfd_set_sources sorted them by voxel)
        std::vector<uint32_t> lin((size_t)s->nSrcVox);
        if (s->nSrcVox) BFD_HIP(hipMemcpy(lin.data(), s->srcLin, lin.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        s->srcLowEnd = std::lower_bound(lin.begin(), lin.end(), (uint32_t)G.lowPlanes * (uint32_t)s->d.plane) - lin.begin();
        s->srcHighBeg = std::lower_bound(lin.begin(), lin.end(), (uint32_t)G.hiStart * (uint32_t)s->d.plane) - lin.begin();
    }
    rc = account_algorithmic_bytes(s, G.tx, all);
    if (rc) return rc;
    if (oldCells) dev_release(s, &oldCells);
    s->tilesReady = true;
    return 0;
}

// Quiet runs (bfd_dev::act; bfd_tile.h): a production call lets the runs ahead of the wave front return at entry. On when the
// engine (a whole domain or a Z-slab of at least three sub-tiles: its boundary runs always work) accumulates its maps over the caller's own window (rmsFirstStep = 0: bench.py's timed windows, which accumulate from
// step 1, never see it), runs the class-specialised kernels (variants 0 / 3, in-place update) and keeps solid-only values compact; BFD_SKIP_ZERO=0
// switches it off. The map starts with the sub-tiles of the source voxels at step 0; when inputs are set again in the middle of a run every sub-tile
// counts as active from then on.
bool quiet_runs_wanted(const bfd_sim *s)          // tile lists built
{
    const bfd_dev &d = s->d;
    const bool whole = d.k0 == 0 && d.nk == d.N3;
    bool on = s->cfg.rmsFirstStep == 0 && class_kernels_in_place(s) &&
              (s->tiles.nSolid == 0 || d.cssRow != nullptr) && d.nk >= 3 * bfd_tile_subz();
    if (const char *ev = getenv("BFD_SKIP_ZERO_SLABS")) on = on && (whole || atoi(ev) != 0);      // 0: whole domains only (the first form of the round)
    if (const char *ev = getenv("BFD_SKIP_ZERO")) on = on && atoi(ev) != 0;
    return on;
}
int setup_activity_map(bfd_sim *s)
{
    bfd_dev &d = s->d;
    const bool whole = d.k0 == 0 && d.nk == d.N3;
    const bool on = s->tilesReady && quiet_runs_wanted(s);
    s->actReady = true;
    BFD_HIP(hipSetDevice(s->cfg.device));
    if (!on) { d.act = nullptr; drop_step_graph(s); return 0; }
    int tx, ty, nsub; bfd_tile_grid(d, &tx, &ty, &nsub);
    const size_t bytes = (size_t)(tx + 2) * (ty + 2) * (nsub + 2);
    if (!s->actBase || s->actBytes != bytes) {
        dev_release(s, &s->actBase);
        const int rc = dev_alloc(s, &s->actBase, bytes, false);
        if (rc) return rc;
        s->actBytes = bytes;
    }
    d.act = s->actBase; d.actX = tx + 2; d.actY = ty + 2;
    {   // a Z-slab: the runs of the sub-tiles that hold the planes next to a neighbour (the "boundary" runs of a split half-step) always work
        const int SUB = bfd_tile_subz(), lowPlanes = std::min(SUB, d.nk), hiStart = std::max(((d.nk - 2) / SUB) * SUB, lowPlanes);
        d.actLo = whole ? 0 : lowPlanes; d.actHi = whole ? 0x7fffffff : hiStart;
    }
    if (s->step == 0) {
        BFD_HIP(hipMemsetAsync(s->actBase, 0, bytes, s->stream));
        bfd_launch_mark_source_subtiles(d, s->stream, s->srcLin, (long)s->nSrcVox);
    } else {
        // the border stays clear (it stands for what lies outside the domain); every sub-tile inside is taken as active
        std::vector<unsigned char> h(bytes, 0);
        for (int q = 1; q <= nsub; q++) for (int y = 1; y <= ty; y++) memset(&h[((size_t)q * (ty + 2) + y) * (tx + 2) + 1], 1, (size_t)tx);
        BFD_HIP(hipStreamSynchronize(s->stream));                            // the engine's stream does not wait for the legacy stream this copy runs on
        BFD_HIP(hipMemcpy(s->actBase, h.data(), bytes, hipMemcpyHostToDevice));
    }
    BFD_HIP(hipGetLastError());
    BFD_HIP(hipStreamSynchronize(s->stream));        // a slab's half-steps may be queued on other streams than the engine's
    drop_step_graph(s);
    return 0;
}
