// Internal structures of libbabelfdtd_hip.so (gfx950 only). Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <future>
#include <string>
#include <vector>
#include "../../include/babelfdtd.h"

#define BFD_REFLECTOR_BIT 0x8000u   // bit 15 of the device material id marks a reflector voxel
#define BFD_MAT_MASK 0x7FFFu
// class byte of a cell (bfd_dev::cls)
#define BFD_CLS_FLUID 1u    // fluid centre (cS = 0), no reflector: Sxx == Syy == Szz, only Szz/Rzz is kept
#define BFD_CLS_NOMEM 2u    // BP == 0 and BS2 == 0: the normal stresses have no memory variable
#define BFD_CLS_EXY 4u      // the xy / xz / yz shear edge of this cell is updated (centre and the 3 other cells solid)
#define BFD_CLS_EXZ 8u
#define BFD_CLS_EYZ 16u
#define BFD_CLS_REFL 32u    // reflector voxel

// CA, CB of the O(4) staggered first derivative (Taylor coefficients) and the matching stability constant
// 1/(CA+CB) of dt <= BFD_STAB h / (sqrt(3) cmax). Overridable for scheme experiments (tests/rayleigh_study.py):
// make TAG=holberg EXTRA='-DBFD_CA=1.1382f -DBFD_CB=0.046414f -DBFD_STAB=(1.0/1.184614)'
#ifndef BFD_CA
#define BFD_CA 1.125f
#define BFD_CB (1.0f / 24.0f)
#endif
#ifndef BFD_STAB
#define BFD_STAB (6.0 / 7.0)
#endif

// tile geometry of the tiled kernels (bfd_tile.h, bfd_kernels_dense / _fluid / _solid / _shear / _setup.hip): 64 x 8 cells per workgroup plane,
// classification in sub-tiles of BFD_SUBZ planes
#define BFD_TILE_X 64
#define BFD_TILE_Y 8
#define BFD_SUBZ 8
// output rows of a workgroup of the fused time step (bfd_kernels_fused.hip): three tiles of the classification grid
#define BFD_FUSED_ROWS 24
// multi-material runs of the fused time step keep AP, BP, 1/rho of every material in LDS: media with more materials fuse only their one-material runs
#define BFD_FUSED_MAX_MATERIALS 1024

// device-side view of one slab; passed by value to kernels
struct bfd_dev {
    int N1, N2, N3;        // global dims
    int k0, nk;            // slab
    int ND, P;             // layer thickness, zone width P = ND+1
    int plane;             // N1*N2
    // state, each (nk+4) planes; pointer addresses local plane 0 (ghost planes at -2,-1,nk,nk+1)
    float *Vx, *Vy, *Vz, *Sxx, *Syy, *Szz, *Sxy, *Sxz, *Syz, *Rxx, *Ryy, *Rzz, *Rxy, *Rxz, *Ryz;
    const uint16_t *mat;   // same ghosting; bit 15 = reflector
    // per-cell class byte (same ghosting), computed at setup from ids, tables and the reflector mask (BFD_CLS_*).
    // Invariant of the tiled kernels (variants 0/3/4): at a cell with BFD_CLS_FLUID only Szz/Rzz of the three identical
    // normal stresses (and memory variables) is maintained -- every reader takes Szz there; a shear stress entry is
    // read only where its edge bit is set (elsewhere it is never updated and stays exactly 0).
    const uint8_t *cls;
    // per-material tables
    const float *AP, *BP, *AS2, *BS2, *invMu, *tauS, *invRho;
    float c1, k2;
    // CPML profiles: [axis][aI,bI,aH,bH]
    const float *axI, *bxI, *axH, *bxH, *ayI, *byI, *ayH, *byH, *azI, *bzI, *azH, *bzH;
    // CPML memory variables (compact zone storage)
    //   x zones: [nk][N2][2P]      y zones: [nk][2P][N1]      z zones: [2P][N2][N1] (global z zone index)
    // stress half-step: 0 dxVx 1 dyVy 2 dzVz 3 dyVx 4 dxVy 5 dzVx 6 dxVz 7 dzVy 8 dyVz
    // velocity half-step: 9 dxSxx 10 dySxy 11 dzSxz 12 dxSxy 13 dySyy 14 dzSyz 15 dxSxz 16 dySyz 17 dzSzz
    float *psi[18];
    int tilesX, tilesY;
    // write targets of the fields that variant 4 keeps in two copies (V, Szz, Rzz); equal to the read pointers in
    // every other variant (in-place update). Kernels read d.X and write d.XW.
    float *VxW, *VyW, *VzW, *SzzW, *RzzW;
    // Compact solid state (round 5; bfd_tiles::css). cssRow != null: the values that exist only at solid cells -- Sxx, Syy, the three
    // shear stresses and the memory variables Rxx, Ryy -- live in the order of the sparse shear list ("listed" cells: solid centre,
    // no reflector) instead of the full-volume arrays, which are then not maintained. cssRow[((kl + 2) * N2 + j) * cssStride + bx] =
    // list index of the first listed cell of row (kl, j) with i >= 64 bx (bx = tilesX: one past the row's last entry); a row of the
    // list is contiguous in x, so the entry of cell i is that base + the number of listed cells of the row in [64 bx, i).
    // 0xFFFFFFFF marks planes without compact values (ghost planes: every value there is 0).
    const unsigned *cssRow; int cssStride;
    float *cSxx, *cSyy, *cSxy, *cSxz, *cSyz, *cRxx, *cRyy, *cRxy, *cRxz, *cRyz;
    // Activity map (round 6; null = every run works in every half-step): one byte per 64 x 8 x BFD_SUBZ sub-tile, 1 = a non-zero V or S value has
    // been written there. Padded by one sub-tile on every side: sub-tile (bx, by, q) at ((q + 1) * actY + by + 1) * actX + bx + 1. A run whose
    // sub-tiles and all their neighbours are clear returns at entry (bfd_tile.h, "QUIET runs"). Production calls only (whole domains and Z-slabs).
    unsigned char *act; int actX, actY;
    int actLo, actHi;      // Z-slabs: runs that touch local planes below actLo or from actHi on (the sub-tiles a neighbour's planes reach) always work; whole domains: 0, INT_MAX
};
#define BFD_CSS_NONE 0xFFFFFFFFu
// a cell has compact values ("listed") when its class byte says solid centre, no reflector
static __device__ __forceinline__ bool css_listed(unsigned c) { return (c & (BFD_CLS_FLUID | BFD_CLS_REFL)) == 0u; }
// number of lanes below this one whose predicate is set (all lanes of the wave must get here)
static __device__ __forceinline__ unsigned css_rank(bool listed)
{
    const unsigned long long b = __ballot(listed);
    return __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
}
// list index of owned cell c (local linear index) or -1 when it has no compact values; for the readers outside the marching kernels
// (sensors, maps, sources): walks the class bytes of the row from the tile edge
static __device__ __forceinline__ long css_index(const bfd_dev &d, long c)
{
    if (!css_listed(d.cls[c])) return -1;
    const int kl = (int)(c / d.plane);
    const int r = (int)(c - (long)kl * d.plane);
    const int j = r / d.N1, i = r - j * d.N1;
    const unsigned rb = d.cssRow[((long)(kl + 2) * d.N2 + j) * d.cssStride + (i >> 6)];
    if (rb == BFD_CSS_NONE) return -1;
    unsigned n = 0;
    for (long q = c - (i & 63); q < c; q++) n += css_listed(d.cls[q]) ? 1u : 0u;
    return (long)rb + n;
}

// tile lists of the class-specialised path (variant 3): device array
// runs [fluid boundary | fluid interior | solid boundary | solid interior] (boundary = inside the first/last
// 32 planes); run = (bx + tilesX*by, kbeg | kend<<16, flags: bit0 solid, bit1 lossy, bit2 UNI, bit3 PML, bit4 LEAN, material
// id of UNI runs). n* counters after nSolidB are in 64x8x8 sub-tiles, for reporting.
// BFD_RUN_ADV_VZ in the flags of a run: stress_fluid stores the new Vz of the run's planes kbeg+1 .. kend-3 and velocity_fluid leaves Vz alone there
// (bfd_lists.hip, "advanced Vz"); both kernels read the same record. bfd_tiles::advVz = some run of the current lists carries it.
#define BFD_RUN_ADV_VZ 512
// kernel classes of the per-kernel timing / byte accounting (bfd_timing_kernels, bfd_algorithmic_bytes)
enum { BFD_K_STRESS_FLUID = 0, BFD_K_STRESS_SOLID = 1, BFD_K_STRESS_SHEAR = 2, BFD_K_VELOCITY_FLUID = 3, BFD_K_VELOCITY_SOLID = 4,
       BFD_K_FUSED = 5, BFD_K_COUNT = 6 };
struct bfd_sim;
// records an event before (end = 0) / after (end = 1) a launch of class cls (bfd_api.hip); t->ktimer != null while class timing is on
void bfd_kmark(bfd_sim *sim, int cls, int end, hipStream_t st);

// maps of bfd_tiles::xmap: fluid stress / fluid velocity / solid stress / solid velocity (plain runs) by part 0, 1, 2; the two pieces of solid
// runs in the absorbing layer; the fused runs
enum { BFD_XM_SF = 0, BFD_XM_VF = 3, BFD_XM_SS = 6, BFD_XM_VS = 9, BFD_XM_VSP_LO = 12, BFD_XM_VSP_HI = 13, BFD_XM_FUSED = 14, BFD_XMAP_COUNT = 15 };
struct bfd_tiles { bfd_sim *ktimer = nullptr; int nMat = 0; int4 *runs = nullptr;
                   unsigned *shearCells = nullptr; float *shearCoef = nullptr; long nShear = 0, shearLowEnd = 0, shearHighBeg = 0;   /* sparse shear list */
                   unsigned *shearCodes = nullptr; float *shearTab = nullptr; long nShearExplicit = 0;   /* per listed cell a byte per edge: 0 inactive, 1 + m = one material around the edge (coefficients from shearTab[8 m], [8 m + 1]; the cell's own AP, BP, AS2, BS2 at [8 m + 4 ..]), 255 = explicit coefficients in shearCoef; number of explicit edges */
                   int4 *runsAll = nullptr; int nAll = 0, nAllB = 0;   /* compact solid state: every run, fluid and solid, in list order [boundary | interior] -- the stress half-step's one launch of the fluid kernel */
                   /* compact solid state (bfd_dev::cssRow): the row table and where the ten compact arrays (Sxx Syy Sxy Sxz Syz Rxx Ryy Rxy Rxz Ryz, list order) live:
                      cssHosted = inside the full-volume buffers of their own fields (unused otherwise in this mode; the placement has spread those over the memory
                      regions, which the sparse kernel's ten streams need as much as the marching kernels' do: 0.253 against 0.266-0.29 ms), from allocation plane 4 on
                      (the planes a Z-neighbour exchanges stay free); else css = one block [10][cssCap] (solid cells too many for that) */
                   unsigned *cssRow = nullptr; float *css = nullptr; long cssCap = 0; bool cssHosted = false;
                   float *shearR = nullptr;   /* full-volume solid state (BFD_COMPACT_SOLID=0) only: memory variables Rxy, Rxz, Ryz of the listed cells, [3][nShear] in list order, beside the list (dense, coalesced); the full-volume arrays are filled from here on demand (bfd_get_field). Null when the state is compact */
                   int nFluid = 0, nFluidB = 0, nSolid = 0, nSolidB = 0, nSolidBP = 0 /* leading boundary runs that touch the absorbing layer */, nSolidIP = 0 /* trailing interior ones */, nFused = 0 /* runs of the fused kernel, after the solid runs */;
                   int nLossless = 0, nLossy = 0, nSolidSub = 0, nUni = 0, nPml = 0, nLean = 0, nFusedSub = 0;
                   bool advVz = false;
                   /* cost-balanced block -> run maps (round 4): block b of a launch runs on XCD slot b & 7 and takes run seg[slot] + (b >> 3) of
                      the launched range if that is below seg[slot + 1]; the launch has 8 x maxcnt blocks. One map of 10 ints (seg[0..8], maxcnt)
                      per launched range and kernel class, on the device in xmap, on the host in xmapH. */
                   int *xmap = nullptr; int xmapH[BFD_XMAP_COUNT][10] = {}; };

// Streamed source table (large PulseSource; bfd_sources.hip): the caller's float64 table stays on the host, time tiles of
// tileSteps steps are converted to float32 [step][source] by a packer job and uploaded double-buffered. pulseHost = null: no table is streamed.
struct bfd_source_tiles {
    const double *pulseHost = nullptr; int tileSteps = 0, nTiles = 0;
    float *tileDev[2] = {}, *tilePinned[2] = {}; int tileLoaded[2] = {-1, -1}, tilePacked[2] = {-1, -1};
    hipEvent_t evTile[2] = {}; bool evTileUsed[2] = {};
    hipEvent_t evRead[2][2] = {}; bool evReadUsed[2][2] = {};      // [buffer][0 = engine stream, 1 = a side stream]: behind the last kernels that read the tile the buffer holds
    std::future<void> packJob[2];
    // The two ends of what the table holds (device tiles, pinned buffers, packer jobs, events). release: back to "no table streamed"; the
    // events stay, the next table reuses them. destroy: release, and the events too (the engine is going away).
    void release(bfd_sim *s);
    void destroy(bfd_sim *s);
};

// Every member starts from its initialiser here; bfd_create sets what depends on the configuration or the environment. bfd_dev has none (it is passed
// to kernels by value and stays a plain aggregate): bfd_create clears it.
struct bfd_sim {
    bfd_config cfg = {};
    bfd_dev d;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    int step = 0;
    size_t nloc = 0, nalloc = 0;    // owned voxels, allocated voxels per state array
    float *stateBase[15] = {};      // allocation bases
    uint16_t *matBase = nullptr;
    uint8_t *clsBase = nullptr; bool classesReady = false;
    bool placementDone = false, haloHandedOut = false;   // bfd_prepare: the per-voxel arrays may be moved until a halo pointer has been given out
    std::string placementNote;           // what bfd_choose_placement found and did (bfd_placement_note; bfd_placement.hip)
    std::vector<void *> searched;        // state buffers that a search found in another memory region: kept for the next engine of this process when this one is destroyed
    int placementMode = 1; int64_t placementLimit = -1;   // bfd_set_placement: 0 = off; bytes the search may hold at a time (-1 = default rule)
    float *tables = nullptr;        // 7*nMat
    float *profiles = nullptr;      // 4*(N1+N2+N3)
    std::vector<void *> allocs;     // everything to free
    int64_t devBytes = 0;
    bool haveMaterials = false, haveMap = false;
    bfd_tiles tiles; bool tilesReady = false;   // variants 2, 3, 4
    bool pingpong = false;              // variant 4 on a whole domain: second copies of V, Szz, Rzz (ppBase), swapped every step
    float *ppBase[5] = {};
    int zchunk = 0;                     // planes of the longest z-run (8, 16 or 32), chosen per grid
    double cmax = 0;
    // sources (bfd_sources.hip)
    int64_t nSrcVox = 0, srcLowEnd = 0, srcHighBeg = 0;   // sources sorted by voxel: [0,lowEnd) first z-chunk, [highBeg,n) last z-chunk
    uint32_t *srcLin = nullptr, *srcRow = nullptr; float *srcW[3] = {}; float *pulseT = nullptr; int nSources = 0, lengthSource = 0;
    bfd_source_tiles srcTiles;      // the dense table streamed from the host instead of resident in pulseT
    // separable source (bfd_set_sources_separable; srcK = 0: the dense table above): row r at step n is
    // sum_k srcWeights[r*K + k] * srcSignals[n*K + k], in that order, in float32
    int srcK = 0; float *srcWeights = nullptr, *srcSignals = nullptr;
    // sensors
    unsigned char *actBase = nullptr; size_t actBytes = 0; bool actReady = false;   // storage of bfd_dev::act; actReady = the map matches the state (cleared by setters and bfd_reset)
    bool sensIsBox = false; int sensBox[5] = {};    // the sensor set is a dense box of voxels: extents in x, y and its first voxel (i0, j0, local k0); captures then need no index list
    int *sensEnt = nullptr; bool sensEntValid = false;   // compact solid state: list entry of every sensor voxel (-1 = none), valid for the current list
    int64_t nSensors = 0; uint32_t *sensLin = nullptr; float *sensOut = nullptr; int nTs = 0; int nSelS = 0; int selS[BFD_MAP_COUNT] = {};
    double *dftAcc = nullptr; float *dftPk = nullptr; int dftBin = 0;      // sensorMode 1: [nSelS][nSensors][2] running DFT sums, [nSelS][nSensors] running peaks
    // accumulators
    int nSelR = 0; int selR[BFD_MAP_COUNT] = {}; float *acc = nullptr, *pk = nullptr;
    int accStart = 0;
    // Paired Pressure accumulation (bfd_api.hip, "paired accumulation"): pairEnv = BFD_PAIR_ACC is not 0; pendingAcc = the Pressure of the current Szz
    // has not been added to the maps at the cells of the fluid runs yet (the next stress half-step adds it together with its own, or a flush does);
    // pairDone = the stress half-step of the current step took the pairing flavour (the maps hold this step already; cleared where the step counter
    // advances); pairedLaunches counts the launches of the pairing stress flavour (bfd_paired_launches)
    bool pairEnv = true, pendingAcc = false, pairDone = false; int64_t pairedLaunches = 0;
    // Advanced Vz (bfd_lists.hip, "advanced Vz"): advEnv = BFD_ADV_VZ is not 0; midStep = a stress half-step of the current step has been queued and its
    // velocity half-step has not ended (cleared where the step counter advances and in bfd_reset): Vz is then of mixed time level in the runs that
    // carry BFD_RUN_ADV_VZ, and the run lists must stay as they are
    bool advEnv = true, midStep = false;
    // timing
    bool timing = false, perKernel = false;
    hipEvent_t evBegin = nullptr, evEnd = nullptr;
    std::vector<hipEvent_t> evStress, evVelocity;  // pairs
    std::vector<hipEvent_t> evK[BFD_K_COUNT];      // pairs per kernel class (perKernel == 2)
    double algBytes[2][BFD_K_COUNT] = {};          // algorithmic bytes per launch and class: [0] no accumulation, [1] Pressure RMS accumulated
    std::vector<hipEvent_t> evPool;
    // optional hipGraph replay of "plain" time steps (no accumulation, no sensor sample, no per-kernel timing) in
    // bfd_run, BFD_USE_GRAPH=1; measured slower than direct launches on ROCm 7.2, so off by default (see bfd_run)
    int *stepDev = nullptr;         // device copy of the step counter (sources index their pulse with it inside a graph)
    hipGraphExec_t stepGraph = nullptr;       // BFD_GRAPH_STEPS time steps
    hipStream_t captureStream = nullptr;
    int graphState = 0;             // 0 not tried, 1 ready, -1 unavailable (direct launches are used)
    bool stepDevValid = false;
};
#define BFD_GRAPH_STEPS 8
// The class-specialised kernels (variants 0 / 3) updating the fields in place (no second copies of variant 4): the clause the three mode
// predicates share -- advanced Vz and quiet runs (bfd_lists.hip), paired accumulation (pair_engine, bfd_api.hip)
inline bool class_kernels_in_place(const bfd_sim *s) { return (s->cfg.kernelVariant == 0 || s->cfg.kernelVariant == 3) && !s->pingpong; }
// Advanced Vz: between the stress and the velocity half-step of a time step the runs that carry BFD_RUN_ADV_VZ hold the new Vz at their inner planes
// and the old one elsewhere; only the velocity half-step over the SAME lists completes it. What would rebuild the lists waits for the step to end.
inline bool lists_held_mid_step(const bfd_sim *s) { return s->midStep && s->tilesReady && s->tiles.advVz; }
#define BFD_REFUSE_MID_STEP(who) do { if (lists_held_mid_step(s)) BFD_FAIL(-6, who ": a stress half-step is outstanding: finish the time step first"); } while (0)

void bfd_set_error(const std::string &s);
#define BFD_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            bfd_set_error(std::string(#call) + ": " + hipGetErrorString(e_));                      \
            return -10;                                                                            \
        }                                                                                          \
    } while (0)
#define BFD_FAIL(code, msg) do { bfd_set_error(msg); return (code); } while (0)

// hipMalloc that gives idle buffers of the placement cache (bfd_placement.hip) back to the device before it reports that memory ran out
hipError_t malloc_or_release_cache(void **q, size_t bytes);
// A device block that lives as long as its scope: the temporaries of the setters and getters. cacheAware = the block is drawn through
// malloc_or_release_cache. Engine-lifetime memory goes through dev_alloc instead. It converts to T * wherever a pointer is expected; `.p` is written
// only where a template would deduce DevTemp itself (kernel launches, hipcub).
template <typename T>
struct DevTemp {
    T *p = nullptr; bool cacheAware;
    explicit DevTemp(bool cacheAware_ = false) : cacheAware(cacheAware_) {}
    DevTemp(const DevTemp &) = delete;
    DevTemp &operator=(const DevTemp &) = delete;
    ~DevTemp() { if (p) hipFree(p); }
    hipError_t alloc(size_t count) { return cacheAware ? malloc_or_release_cache((void **)&p, count * sizeof(T)) : hipMalloc((void **)&p, count * sizeof(T)); }
    operator T *() const { return p; }
};

inline int grid_for(long n, int block = 256) { return (int)std::min<long>((n + block - 1) / block, 256L * 32); }

template <typename T>
int dev_alloc(bfd_sim *s, T **p, size_t count, bool zero = true)
{
    void *q = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    BFD_HIP(malloc_or_release_cache(&q, bytes));
    if (zero) BFD_HIP(hipMemsetAsync(q, 0, bytes, s->stream));
    s->allocs.push_back(q);
    s->devBytes += (int64_t)bytes;
    *p = (T *)q;
    return 0;
}

// frees an array obtained from dev_alloc before the sim is destroyed (inputs that are set again)
template <typename T>
void dev_release(bfd_sim *s, T **p)
{
    if (!*p) return;
    auto it = std::find(s->allocs.begin(), s->allocs.end(), (void *)*p);
    if (it != s->allocs.end()) { hipFree(*it); s->allocs.erase(it); }
    *p = nullptr;
}

inline size_t span_elems(int N1, int N2, int nk, int64_t s1, int64_t s2, int64_t s3)
{
    return (size_t)((N1 - 1) * s1 + (N2 - 1) * s2 + (nk - 1) * s3 + 1);
}

// the selected maps of a bit mask, ascending; returns their number (bfd_api.hip)
int sel_list(uint32_t mask, int *sel);
// paired accumulation (bfd_api.hip): adds the outstanding Pressure to the maps before anything reads or clears them, or changes what lies behind them;
// st: the stream the following launches go to (default: the engine's)
int flush_pending(bfd_sim *s, hipStream_t st);
inline int flush_pending(bfd_sim *s) { return flush_pending(s, s->stream); }
// flags[v] = 1 where the strided device copy `in` of a caller's uint32 map of the slab is not 0, v in x-fastest order; on the engine's stream
// (bfd_api.hip: the layout kernel of the input setters)
void bfd_launch_gather_flags(const bfd_sim *s, const uint32_t *in, long s1, long s2, long s3, uint8_t *flags);
// ascending indices of the set flags among n, on the device: sel[0 .. *dcount). Queued on st; work = the select's scratch block, which the caller keeps
// until it has synchronised (bfd_api.hip)
hipError_t select_flagged(uint8_t *flags, uint32_t *sel, int *dcount, int n, hipStream_t st, DevTemp<char> &work);

// inputs changed (bfd_api.hip): a recorded step graph holds stale pointers; the run lists, the activity map and a recorded step graph are out of
// date, and (classes: materials, map, reflector) the cell classes
void drop_step_graph(bfd_sim *s);
void invalidate_lists(bfd_sim *s, bool classes = true);
// the accumulating steps of this engine pair (bfd_api.hip, "paired accumulation"); quiet = quiet runs are or will be in use, nFluid = the fluid run count
bool pair_engine(const bfd_sim *s, bool quiet, int nFluid);
// what feeds source values to a time step (bfd_sources.hip):
// the injection kernels of one part of a half-step (0 all, 1 = first + last z-chunk, 2 = the chunks between) at step s->step into the fields of `view`, on st
int bfd_inject_part(bfd_sim *s, int part, const bfd_dev &view, hipStream_t st);
// the injection node of a recorded plain step (hipGraph capture on cs): every source voxel, the step taken from the device's counter s->stepDev
void bfd_record_injection(bfd_sim *s, hipStream_t cs);
// everything the source path holds is released and the engine is back to "no sources"; final = the engine is being destroyed (the events go too)
void bfd_release_sources(bfd_sim *s, bool final);
// bfd_reset: the streamed table starts over (waits for the packer jobs; tiles are uploaded again on demand)
void bfd_rewind_sources(bfd_sim *s);
// the planner of the class-specialised path (bfd_lists.hip):
// builds the run lists, the sparse shear list and the compact solid state from the cell classes (rebuilt mid-run: the solid state is carried over)
int build_tile_lists(bfd_sim *s);
// quiet runs: sets up (or switches off) the activity map for the current lists and step
int setup_activity_map(bfd_sim *s);
// points the ten compact views of bfd_dev at where the compact arrays live; again whenever the state buffers change hands (after the placement)
void bind_compact_views(bfd_sim *s);
// this engine lets the runs ahead of the wave front return at entry (needs the run lists built)
bool quiet_runs_wanted(const bfd_sim *s);

// an event from the engine's pool or a new one; null when none can be made (bfd_api.hip)
hipEvent_t bfd_get_event(bfd_sim *s);
// the kernels' views of the state arrays (bfd_dev) from the allocation bases stateBase / ppBase (bfd_api.hip)
void bfd_bind_state_views(bfd_sim *s);
// placement of the per-voxel arrays by memory region and the cache of the buffers a search found (bfd_placement.hip): the chooser of bfd_prepare;
// a buffer of a destroyed engine offered to the cache (true: taken, the caller must not free it); cached buffers of another size freed; all freed,
// returns their bytes
int bfd_choose_placement(bfd_sim *s);
bool bfd_placement_cache_put(int device, size_t bytes, void *p);
void bfd_placement_cache_evict_other_sizes(int device, size_t bytes);
int64_t bfd_placement_cache_drop_all(void);
// what leaves the engine (bfd_outputs.hip): the end of a time step on stream st -- the maps the velocity kernels did not accumulate (qP = the slot
// they did, -1 = none) and the sensor sample; the output arrays cleared on the engine's stream (bfd_reset); the pinned pieces of the large
// device-to-host copies given back to the system (bfd_placement_cache_release)
int bfd_step_outputs(bfd_sim *s, hipStream_t st, int qP);
int bfd_clear_outputs(bfd_sim *s);
void bfd_release_pinned_pieces(void);
// madvise(MADV_HUGEPAGE) on a result buffer of the caller before a large device-to-host copy (bfd_outputs.hip)
void bfd_advise_result_buffer(void *p, size_t bytes);
// bfd_get_sensors with a row pitch: the series of selected map q at out + q * rowElems (bfd_outputs.hip; bfd_group.hip: a slab writes into its columns)
int bfd_sensors_into(bfd_sim *s, float *out, int64_t rowElems);
// kernel launchers (bfd_kernels_*.hip), by the file that defines them
// --- bfd_kernels_v1.hip
void bfd_launch_stress_v1(const bfd_dev &d, hipStream_t s);
void bfd_launch_velocity_v1(const bfd_dev &d, hipStream_t s);
// --- bfd_kernels_fused.hip: runs [off, off + n) of the fused list
void bfd_launch_fused(const bfd_dev &d, hipStream_t s, float *accP, float *pkP, const bfd_tiles *t, int off, int n);
int bfd_fused_rows(void);
int bfd_fused_max_materials(void);
// --- bfd_kernels_setup.hip: the tile grid's sizes and the kernels of the planner and of the placement
void bfd_tile_grid(const bfd_dev &d, int *tilesX, int *tilesY, int *subZ);
int bfd_tile_subz(void);
int bfd_tile_zchunk(void);
void bfd_launch_classify(const bfd_dev &d, hipStream_t s, int *flagsDev, int *tileMatDev);
void bfd_launch_mark_source_subtiles(const bfd_dev &d, hipStream_t s, const uint32_t *lin, long n);
void bfd_launch_cell_classes(const bfd_dev &d, hipStream_t s, uint8_t *clsBase, long nalloc);
// counts over the cells of the solid runs: [0] fluid no-memory, [1] fluid with memory, [2] solid no-memory, [3] solid with memory,
// [4] active shear edges, [5] reflector cells
void bfd_launch_count_solid_cells(const bfd_dev &d, hipStream_t s, const int4 *solidRuns, int nSolid, unsigned long long *counts6);
// placement probe: arrays a and b (pointers to local plane 0) updated in place along all runs of the slab, planes [0, kmax)
void bfd_launch_probe_pair(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, float *a, float *b, int kmax);
// --- bfd_kernels_shear.hip: the sparse shear kernel, its list and the compact solid state
// flags the cells of the sparse shear list: solid, non-reflector centre
void bfd_launch_mark_solid(const bfd_dev &d, hipStream_t s, unsigned char *flag, long n);
void bfd_launch_shear_order_keys(const bfd_dev &d, hipStream_t s, const unsigned *cells, unsigned long long *keys, long n, int lowPlanes, int hiStart);
void bfd_launch_shear_coefficients(const bfd_dev &d, hipStream_t s, const unsigned *cells, float *coef, unsigned *codes, float *tab, int nMat, long n);
// copies the list-ordered shear memory variables into the full-volume arrays Rxy, Rxz, Ryz (outputs only)
void bfd_launch_scatter_shear_memory(const bfd_dev &d, hipStream_t s, const bfd_tiles *t);
void bfd_launch_gather_shear_memory(const bfd_dev &d, hipStream_t s, const bfd_tiles *t);
// compact solid state: the row table of the ordered list (lowPlanes / hiStart as for bfd_launch_shear_order_keys)
void bfd_launch_css_row_table(const bfd_dev &d, hipStream_t s, const unsigned *cells, long n, unsigned *rowTable, int stride, int lowPlanes, int hiStart);
// dstFull (pointer to local plane 0 of a full-volume buffer) [cell] = compact array a [entry], a = 0..9 in the order Sxx Syy Sxy Sxz Syz Rxx Ryy Rxy Rxz Ryz;
// the reverse into dstCompact from a full-volume source. cells / n: the list the entries belong to.
void bfd_launch_css_scatter(hipStream_t s, const unsigned *cells, long n, const float *compact, float *dstFull);
void bfd_launch_css_gather(hipStream_t s, const unsigned *cells, long n, const float *srcFull, float *dstCompact);
// the sparse kernel over cells [b, e) of the list; R: their list-ordered memory variables (null with the compact solid state)
void bfd_launch_stress_shear(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, long b, long e, float *R);
// --- bfd_kernels_fluid.hip. runs / cnt: the range of the run list; m: index of its cost-balanced map (bfd_tiles::xmap), -1 = none
// pair: the plain fluid runs take the pairing flavour, which adds the Pressure of the previous and of this step to the maps accP / pkP
void bfd_launch_stress_fluid(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, const int4 *runs, int cnt, int m, bool pair, float *accP, float *pkP);
void bfd_launch_velocity_fluid(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, const int4 *runs, int cnt, int m, bool acc, float *accP, float *pkP);
// adds the Pressure of the current Szz to the maps at the accumulating cells of the fluid runs (paired accumulation with its partner step outstanding)
void bfd_launch_flush_paired(const bfd_dev &d, hipStream_t s, float *accP, float *pkP, const bfd_tiles *t);
// --- bfd_kernels_solid.hip. pml: the runs of the range touch the absorbing layer; part as below
void bfd_launch_stress_solid(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, const int4 *runs, int cnt, int m);
void bfd_launch_velocity_solid(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, int part, bool pml, const int4 *runs, int cnt, int m, float *accP, float *pkP);
// --- bfd_kernels_dense.hip (kernelVariant 2)
void bfd_launch_stress_dense(const bfd_dev &d, hipStream_t s, const int4 *runs, int n);
void bfd_launch_velocity_dense(const bfd_dev &d, hipStream_t s, const int4 *runs, int n, float *accP, float *pkP);
// --- bfd_kernels_tiled.hip: the launches of a half-step in their order
// part: 0 = every tile, 1 = boundary tiles, 2 = interior tiles (variant 2 lists every tile as solid)
// accP / pkP not null: the plain fluid runs take the pairing flavour, which adds the Pressure of the previous and of this step to the maps
void bfd_launch_stress_tiled(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, int part, float *accP = nullptr, float *pkP = nullptr);
// accP / pkP: Pressure RMS / peak accumulators of this step (slab-local, x-fastest) or nullptr; fluidAcc = false: only the solid runs
// accumulate (the fluid runs are paired in the stress half-step)
void bfd_launch_velocity_tiled(const bfd_dev &d, hipStream_t s, float *accP, float *pkP, const bfd_tiles *t, int part, bool fluidAcc = true);
