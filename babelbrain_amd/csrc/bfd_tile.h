// The 64 x 8 tile of the tiled kernels (bfd_kernels_dense / _fluid / _solid / _shear / _setup.hip) and the helpers of their launchers
// (bfd_kernels_tiled.hip orders the launches of a half-step). Helpers only: every kernel is in its own .hip file. gfx950 only.
//
// Design (DESIGN.md "Kernels"):
//  * x is the fastest axis; a wavefront is 64 consecutive x voxels of one row, so every state
//    load/store is a fully coalesced 256-B row segment.
//  * A workgroup owns a TX x TY = 64 x 8 tile (8 waves) and marches ZC planes along z. The z
//    stencil (k-2..k+2) lives in per-thread register queues, so each state value is fetched
//    from HBM once per half-step; the in-plane stencil (+-2 in x and y) is served from an LDS
//    tile of the current plane with its halo ring, double-buffered (one barrier per plane).
//  * Halo ring loads are distributed over the workgroup as two per-thread "tasks" fixed before
//    the loop; y-halo rows are full coalesced rows.
//  * Tiles are dealt to XCDs in contiguous runs (blockIdx -> tile remap) so neighbouring tiles
//    share one L2.
//  * Arithmetic is the canonical float32 sequence of oracle/fdtd_oracle.c (no contraction).
#pragma once
#include "bfd_internal.h"
#include <type_traits>

namespace {

constexpr int TX = BFD_TILE_X;
constexpr int TY = BFD_TILE_Y;
constexpr int LW = TX + 4;          // LDS row length (floats)
constexpr int LH = TY + 4;          // LDS rows
constexpr int NTHREADS = TX * TY;   // 512
constexpr int YT = 4 * TX;          // y-halo tasks per array (4 rows x 64)
constexpr int XT = 4 * TY;          // x-halo tasks per array (4 cols x TY)
constexpr int ZCHUNK = 32;        // longest z-run one workgroup marches
constexpr int SUBZ = BFD_SUBZ;     // z granularity of the fluid/solid classification (a run is a stretch of sub-tiles)

struct HaloTask {
    int lofs;       // offset inside one LDS tile (floats), -1 = no task
    int gofs;       // in-plane global offset j*N1+i (valid only if ok)
    int arr;        // which array of the kernel's LDS set
    bool ok;        // inside the domain (else the halo value is 0)
};

// y-type task u in [0,256): row r=u/64 -> ly = r<2 ? r : TY+r ; lx = u%64+2
__device__ __forceinline__ void ytask(int u, int arr, int i0, int j0, int N1, int N2, HaloTask &t)
{
    const int r = u >> 6, c = u & 63;
    const int ly = r < 2 ? r : TY + r, lx = c + 2;
    const int gi = i0 + c, gj = j0 - 2 + ly;
    t.arr = arr; t.lofs = ly * LW + lx; t.gofs = gj * N1 + gi;
    t.ok = (gi < N1) && (gj >= 0) && (gj < N2);
}
// x-type task u in [0,32): ly = u/4+2 ; c=u%4 -> lx = c<2 ? c : TX+c
__device__ __forceinline__ void xtask(int u, int arr, int i0, int j0, int N1, int N2, HaloTask &t)
{
    const int c = u & 3, ly = (u >> 2) + 2;
    const int lx = c < 2 ? c : TX + c;
    const int gi = i0 - 2 + lx, gj = j0 - 2 + ly;
    t.arr = arr; t.lofs = ly * LW + lx; t.gofs = gj * N1 + gi;
    t.ok = (gi >= 0) && (gi < N1) && (gj < N2);
}

// ------------------------------------------------------------------------------------------------
// QUIET runs (round 6, production calls only: bfd_dev::act != null). Ahead of the wave front every field is EXACTLY zero (float32 with
// denormals flushed: the numerical precursors of the front die out some 25 cells ahead of it), and a half-step maps an all-zero
// neighbourhood onto itself. bfd_dev::act holds one byte per 64 x 8 x SUBZ sub-tile (padded by one sub-tile on every side, border 0):
// 1 = a kernel has written a non-zero V or S value into the sub-tile at some time (set-only; the sub-tiles that hold source voxels carry
// it from the start). A run whose own sub-tiles and all their 26 neighbours are clear returns at entry: everything it would read is zero,
// everything it would write is the zero that is there already (memory variables and absorbing-layer variables included: they are driven
// by the same values). A run that does work ORs the bits of what it stores and sets the byte of its sub-tiles if anything was non-zero.
// Flags only ever get set, so reading a neighbour's byte while that neighbour sets it in the same launch errs on the side of working (the
// decision is taken once per workgroup: run_all_quiet).
// The sparse kernel has no part in this: a non-zero it writes lies within 2 cells of a non-zero V, whose sub-tile is flagged, and every run
// within reach of that cell is a neighbour of that sub-tile. In a Z-slab the runs next to a neighbour's planes always work (run_all_quiet). Bit-identical to running every run (the -0 a skipped update might have
// produced compares equal to the +0 that stays).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool run_all_quiet(const bfd_dev &d, int bx, int by, int kbeg, int kend)
{
    const int q0 = kbeg / SUBZ, q1 = (kend - 1) / SUBZ;
    const int nq = q1 - q0 + 3;                             // the run's sub-tiles, one more below and one above
    if (9 * nq > 64) return false;
    // Z-slab: the runs of the first and the last sub-tile read the ghost planes a neighbour fills: nothing here knows when those turn non-zero, so these runs
    // always work -- and set their bytes when they write a non-zero, which is how the rest of the slab learns that the wave has come in
    if (kbeg < d.actLo || kend > d.actHi) return false;
    const int l = threadIdx.x;                              // lane: a wave is one tile row
    const int dq = l / 9, r = l - 9 * dq, dy = r / 3, dx = r - 3 * dy;
    // padded coordinates: sub-tile (bx, by, q) sits at (bx + 1, by + 1, q + 1), so its lower neighbour is at (bx, by, q)
    const unsigned idx = (unsigned)(((q0 + dq) * d.actY + (by + dy)) * d.actX + (bx + dx));
    const unsigned f = (l < 9 * nq) ? (unsigned)d.act[idx] : 0u;
    // ONE answer per workgroup: every wave reads the bytes for itself, and a neighbour may set its byte between two of those reads -- a wave that
    // left while its siblings stayed would leave their LDS tile with rows nobody filled. If any wave saw a set byte, all of them work.
    return __syncthreads_or(f != 0u) == 0;
}
__device__ __forceinline__ void run_mark_active(const bfd_dev &d, int bx, int by, int kbeg, int kend, unsigned nzbits)
{
    if (__ballot((nzbits & 0x7fffffffu) != 0u) == 0ull) return;
    if (threadIdx.x == 0)
        for (int q = kbeg / SUBZ; q <= (kend - 1) / SUBZ; q++) d.act[((q + 1) * d.actY + by + 1) * d.actX + bx + 1] = 1;
}
__device__ __forceinline__ unsigned fbits(float v) { return __float_as_uint(v); }

}  // namespace

// ---- launch helpers (host): they use the caller's d, s, t and tilesX ----
#define BFD_LAUNCH(K, n, ...) hipLaunchKernelGGL(K, dim3(n), dim3(TX, TY, 1), 0, s, d, tilesX, n, __VA_ARGS__)
// launch over a range that has a cost-balanced map (bfd_tiles::xmap, index m): 8 x maxcnt blocks, those without a run return at once
#define BFD_LAUNCH_X(K, n, m, ...) do { const int *xm_ = t->xmap ? t->xmap + 10 * (m) : nullptr; \
        hipLaunchKernelGGL(K, dim3(xm_ ? 8 * t->xmapH[m][9] : (n)), dim3(TX, TY, 1), 0, s, d, tilesX, n, xm_, __VA_ARGS__); } while (0)
#define BFD_KT(cls, end) do { if (t->ktimer) bfd_kmark(t->ktimer, cls, end, s); } while (0)

// run-time flags into template arguments: lift(f, a, b, ...) calls f(std::bool_constant<a>(), std::bool_constant<b>(), ...). A kernel flavour is
// instantiated for every combination f's body names, so f guards the combinations that are never launched with if constexpr.
template <typename F> static inline void lift(F &&f) { f(); }
template <typename F, typename... B> static inline void lift(F &&f, bool b, B... rest)
{
    if (b) lift([&](auto... c) { f(std::true_type(), c...); }, rest...);
    else lift([&](auto... c) { f(std::false_type(), c...); }, rest...);
}

// run list layout: [fluid boundary | fluid interior | solid boundary | solid interior]; "boundary" = runs
// inside the first and the last ZCHUNK planes of the slab (the planes a Z-neighbour reads).
// part: 0 = every run, 1 = boundary runs, 2 = interior runs
static inline void part_range(int n, int nB, int part, int *off, int *cnt)
{
    if (part == 1) { *off = 0; *cnt = nB; }
    else if (part == 2) { *off = nB; *cnt = n - nB; }
    else { *off = 0; *cnt = n; }
}
