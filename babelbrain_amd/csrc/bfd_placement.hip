// Placement of the per-voxel arrays by memory region (bfd_prepare -> bfd_choose_placement) and the cache of buffers a search found.
// Host code only: the probe kernel is bfd_kernels_setup.hip's (bfd_launch_probe_pair). gfx950 only.
//
// The tiled kernels stream 6 to 20 arrays at the same cell offset. Round 2 found that the same kernels on the same data run
// 1.50 or 1.70 ms per step at C3 depending on nothing but where hipMalloc put those arrays, and chose among whole sets of
// allocations by timing the kernels (a lottery). Round 3 found the cause (scripts/ubench_layout.hip, ubench_pairmap.hip;
// profiles/r3/placement_*): the 288 GB of HBM fall into three contiguous physical regions of about 90 GiB (the ranks of the
// 12-high stacks, as far as can be told from outside), and streams that advance together are slow when they all lie in ONE
// region and fast as soon as they are spread over two: every array in one region 0.98 + 0.76 ms for the two fluid proxies,
// arrays alternating between two regions 0.86 + 0.68 ms, on every draw. A fresh process gets all its allocations from one
// region, a fragmented device gives a mix -- the lottery's "fast sets".
// What counts are the arrays a kernel WRITES (mixing experiment of the same benchmark: the stress proxy turns fast when Szz and
// Rzz lie apart, whatever V does; the velocity proxy when Vx, Vy, Vz and the accumulator are split two and two).
// So the arrays are placed, not drawn: a pair probe (two arrays updated in place at the same cell offset along the engine's
// own runs; zeros stay zeros, so it runs on the initial state) tells whether an array lies in the region of the reference
// array Vx (about 7 % slower) or in another one. The arrays of the stream order Vx Vy Vz Szz Rzz [Sxx ... Ryz] then alternate
// between "region of Vx" and "another region": first by exchanging buffers among the 15 state arrays (all the same size, all
// zero), then, if one kind is short, with freshly allocated candidates (misses are held until the search ends, so that the
// allocator moves on; bounded by the free memory). The Pressure accumulators are re-allocated likewise when they fall on
// the wrong side. A few dozen probes of well under a millisecond; results do not depend on it.
// BFD_PLACEMENT=0 switches it off; BFD_PLACEMENT_VERBOSE=1 prints what it does.
// Buffers that a search found in another memory region are kept when their engine is destroyed and offered to the next engine of this
// process that wants arrays of the same size on the same device (re-probed there: region classes are relative): the two or three solver calls
// of one RunCases (BASE:2338, 2374, 2401) pay the search once. Bounded (BABELFDTD_PLACEMENT_CACHE_GIB, default 48, 0 = off);
// bfd_placement_cache_release() frees it.
#include "bfd_internal.h"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <mutex>

// ---- the cache ----------------------------------------------------------------------------------------------------------
struct CachedBuf { int device; size_t bytes; void *p; };
static std::mutex g_cacheMutex;
static std::vector<CachedBuf> g_cache;
// at most BABELFDTD_PLACEMENT_CACHE_GIB (default 48) and never more than an eighth of the device's memory
static size_t placement_cache_cap()
{
    double gib = 48.0;
    if (const char *ev = getenv("BABELFDTD_PLACEMENT_CACHE_GIB")) gib = atof(ev);
    size_t cap = gib > 0 ? (size_t)(gib * 1073741824.0) : 0;
    size_t freeB = 0, totalB = 0;
    if (cap && hipMemGetInfo(&freeB, &totalB) == hipSuccess && totalB) cap = std::min(cap, totalB / 8);
    else (void)hipGetLastError();
    return cap;
}
// a new engine on `device` whose state arrays have `bytes` each: cached buffers of any other size are of no use to it and go back to the device
// before it allocates (they used to wait for the next bfd_destroy)
void bfd_placement_cache_evict_other_sizes(int device, size_t bytes)
{
    std::lock_guard<std::mutex> lk(g_cacheMutex);
    for (size_t q = 0; q < g_cache.size();) {
        if (g_cache[q].device == device && g_cache[q].bytes != bytes) { hipFree(g_cache[q].p); g_cache.erase(g_cache.begin() + q); }
        else q++;
    }
    (void)hipGetLastError();
}
static size_t placement_cache_bytes(int device)
{
    std::lock_guard<std::mutex> lk(g_cacheMutex);
    size_t held = 0;
    for (const CachedBuf &c : g_cache) if (c.device == device) held += c.bytes;
    return held;
}
static std::vector<void *> placement_cache_take(int device, size_t bytes)
{
    std::lock_guard<std::mutex> lk(g_cacheMutex);
    std::vector<void *> out;
    for (size_t q = 0; q < g_cache.size();) {
        if (g_cache[q].device == device && g_cache[q].bytes == bytes) { out.push_back(g_cache[q].p); g_cache.erase(g_cache.begin() + q); }
        else q++;
    }
    return out;
}
// true if the cache took the buffer (the caller must not free it)
bool bfd_placement_cache_put(int device, size_t bytes, void *p)
{
    std::lock_guard<std::mutex> lk(g_cacheMutex);
    hipSetDevice(device);
    const size_t cap = placement_cache_cap();
    // buffers of another size on this device are of no use to the caller that is coming: they make room first (kept as it was, although
    // bfd_create evicts them already: only an engine of another size that was created while this one lived can have left any)
    for (size_t q = 0; q < g_cache.size();) {
        if (g_cache[q].device == device && g_cache[q].bytes != bytes) { hipSetDevice(device); hipFree(g_cache[q].p); g_cache.erase(g_cache.begin() + q); }
        else q++;
    }
    size_t held = 0;
    for (const CachedBuf &c : g_cache) held += c.bytes;
    if (held + bytes > cap) return false;
    g_cache.push_back({device, bytes, p});
    return true;
}
// everything, on every device (bfd_placement_cache_release); the caller's current device stays current
int64_t bfd_placement_cache_drop_all(void)
{
    std::lock_guard<std::mutex> lk(g_cacheMutex);
    int64_t freed = 0;
    int cur = 0;
    const bool haveCur = hipGetDevice(&cur) == hipSuccess;
    for (const CachedBuf &c : g_cache) { hipSetDevice(c.device); hipFree(c.p); freed += (int64_t)c.bytes; }
    g_cache.clear();
    if (haveCur) hipSetDevice(cur);
    return freed;
}
// hipMalloc that gives the idle buffers of the cache back to the device before it reports that memory ran out
hipError_t malloc_or_release_cache(void **q, size_t bytes)
{
    hipError_t e = hipMalloc(q, bytes);
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
        (void)hipGetLastError();
        if (bfd_placement_cache_release() > 0) e = hipMalloc(q, bytes);
    }
    return e;
}

// ---- the pair probe -----------------------------------------------------------------------------------------------------
// device time of `reps` pair probes of the arrays at a and b (pointers to local plane 0), planes [0, kmax); < 0 on error
static float time_pair(bfd_sim *s, float *a, float *b, int kmax, int reps)
{
    (void)hipGetLastError();                    // a stale error of some earlier call is not this probe's
    hipEvent_t e0 = bfd_get_event(s), e1 = bfd_get_event(s);
    if (!e0 || !e1) { if (e0) s->evPool.push_back(e0); if (e1) s->evPool.push_back(e1); return -1.f; }
    for (int r = -1; r < reps; r++) {           // r = -1: untimed
        if (r == 0) hipEventRecord(e0, s->stream);
        bfd_launch_probe_pair(s->d, s->stream, &s->tiles, a, b, kmax);
    }
    hipEventRecord(e1, s->stream);
    float ms = -1.f;
    if (hipEventSynchronize(e1) == hipSuccess && hipGetLastError() == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ms /= reps;
    else ms = -1.f;
    s->evPool.push_back(e0); s->evPool.push_back(e1);
    return ms;
}

namespace {

// what every stage probes with. Buffers 0-14: the state arrays; 15-19 (variant 4 on a whole domain): the second copies of
// Vx Vy Vz Szz Rzz, written in the steps in which the first copies are read
struct Probe {
    bfd_sim *s;
    int nBuf;
    size_t g;              // elements from an allocation base to local plane 0
    int kmax;              // the probe runs over planes [0, kmax)
    size_t half;           // elements from plane 0 to the partner of a self-pair
    size_t bytes;          // of one state array
    int nProbes;
    bool verbose;
    std::string times;     // BFD_PLACEMENT_VERBOSE: every probe time
    explicit Probe(bfd_sim *sim)
        : s(sim), nBuf(sim->pingpong ? 20 : 15), g(2 * (size_t)sim->d.plane), kmax(sim->d.nk / 2), half((size_t)(sim->d.nk - kmax) * sim->d.plane),
          bytes(sim->nalloc * sizeof(float)), nProbes(0), verbose(getenv("BFD_PLACEMENT_VERBOSE") != nullptr) {}
    float pair(float *a, float *b) { nProbes++; return time_pair(s, a, b, kmax, 3); }
    float *&base(int a) const { return a < 15 ? s->stateBase[a] : s->ppBase[a - 15]; }
};

struct Levels { float tSame, thr, widest; std::vector<float> t0; };   // fastest self-pair, the threshold between the levels, the widest gap, Vx against buffer a
struct Buf { float *base; int cls; bool fresh; };
struct Classes {
    std::vector<Buf> pool;           // the nBuf originals, then the fresh buffers of the search
    std::vector<float *> repOf;      // class -> representative (pointer to local plane 0)
    int M;                           // the most populated class
    int sideOf(const Buf &b) const { return b.cls == M ? 0 : 1; }            // 0: region M, 1: elsewhere
};
struct Order { std::vector<int> order, side; };                              // array, and 0: region M, 1: elsewhere
struct Budget { size_t heldCap; bool defaultRule; double searchSeconds; bool probeTells; std::string capNote; size_t mine, others; };
struct Found { int need[2]; int nFresh, nCached; bool gaveUp; std::string ended; };   // ended: why the walk stopped, for the note

// The one owner of memory the search has taken and the engine does not own (yet). `ptrs`: candidates that missed and spacers, `bytes` of them,
// never more than `cap`. `fresh`: hits that an array is going to take -- the engine's from the commit stage on (commit()). The destructor gives
// everything back, so every early return does.
struct Held {
    hipStream_t stream; size_t cap;
    std::vector<void *> ptrs; size_t bytes = 0;
    std::vector<void *> fresh;
    Held(hipStream_t st, size_t cap_) : stream(st), cap(cap_) {}
    Held(const Held &) = delete;
    Held &operator=(const Held &) = delete;
    ~Held() { if (ptrs.empty() && fresh.empty()) return; release(); (void)hipGetLastError(); }
    void release()
    {
        for (void *h : ptrs) hipFree(h);
        for (void *f : fresh) hipFree(f);
        ptrs.clear(); fresh.clear();
    }
    // a candidate that is neither held nor taken: its probe failed, or no array wants it
    void discard(void *c) { hipFree(c); }
    // A zeroed candidate of n bytes, or null (no sticky error is left): memory short -- twice its size and an eighth of the device stay free --,
    // the cap reached, the caller's veto(freeB, totalB), asked between the memory check and the allocation, or hipMalloc / hipMemsetAsync failed.
    template <class Veto> float *draw(size_t n, Veto veto)
    {
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) != hipSuccess || freeB < 2 * n + totalB / 8 || bytes + n > cap) { (void)hipGetLastError(); return nullptr; }
        if (veto(freeB, totalB)) return nullptr;
        float *c = nullptr;
        if (hipMalloc((void **)&c, n) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (hipMemsetAsync(c, 0, n, stream) != hipSuccess) { hipFree(c); (void)hipGetLastError(); return nullptr; }
        return c;
    }
    float *draw(size_t n) { return draw(n, [](size_t, size_t) { return false; }); }
    // Holds candidate c of n bytes, so that the allocator moves on. A region is ~90 GiB wide: walk on in growing strides (an unprobed throw-away
    // block as large as everything held so far, 4 GiB at most: hipMalloc of 4 GiB takes 0.3 ms, of 16 GiB 650 ms -- scripts/r3/malloc_cost.hip)
    // instead of one array at a time
    void keep_miss(void *c, size_t n)
    {
        ptrs.push_back(c); bytes += n;
        const size_t stride = std::min(bytes, (size_t)4 << 30);
        size_t freeB = 0, totalB = 0;
        void *sp = nullptr;
        if (bytes + stride <= cap && hipMemGetInfo(&freeB, &totalB) == hipSuccess && freeB > stride + 2 * n + totalB / 8 && hipMalloc(&sp, stride) == hipSuccess) { ptrs.push_back(sp); bytes += stride; }
        else (void)hipGetLastError();
    }
};

// the switches; false = nothing to do, and the note says why
bool placement_wanted(bfd_sim *s)
{
    s->placementNote = "off";
    bool on = s->placementMode != 0;
    if (const char *ev = getenv("BFD_PLACEMENT")) on = atoi(ev) != 0;
    // below ~32 M voxels the arrays a kernel streams (5 x 4 B per voxel and up) fit the 256 MB memory-side cache, where they lie
    // in DRAM stops mattering, and the probe (0.02 ms at 256^3) cannot tell the regions apart any more
    size_t minVoxels = (size_t)32 << 20;
    if (const char *ev = getenv("BFD_PLACEMENT_MIN_VOXELS")) minVoxels = (size_t)atol(ev);      // tests: exercise it on small grids too
    if (!on) return false;
    if (s->step != 0 || s->haloHandedOut || s->cfg.kernelVariant == 1 || s->nloc < minVoxels || s->d.nk < 8 ||
        s->tiles.nFluid + s->tiles.nSolid == 0) { s->placementNote = "skipped (small grid or arrays already handed out)"; return false; }
    return true;
}

// Two levels of pair times: "same region" (an array against itself half a slab further on is always one of these) and,
// 7-15 % below, "different regions". Their absolute values move with the run lists of the medium, so the threshold is
// read off the samples: the five self-pairs and Vx against every other array, sorted; the widest gap below the fastest
// self-pair separates the levels if it is wider than 3.5 % (measured gaps: 7-10 %, scatter inside a level up to 5 %
// top to bottom but dense); without such a gap every array lies in the region of Vx.
int find_threshold(Probe &P, Levels &L)
{
    bfd_sim *s = P.s;
    const size_t g = P.g;
    float tSame = 0;
    std::vector<float> samples;
    for (int a : {0, 1, 2, 5, 11}) {
        const float t = P.pair(s->stateBase[a] + g, s->stateBase[a] + g + P.half);
        if (t <= 0) BFD_FAIL(-10, "placement: the pair probe failed on the zero state");
        if (tSame == 0 || t < tSame) tSame = t;
    }
    samples.push_back(tSame);
    std::vector<float> t0(P.nBuf, 0.f);
    for (int a = 1; a < P.nBuf; a++) {
        t0[a] = P.pair(s->stateBase[0] + g, P.base(a) + g);
        if (t0[a] <= 0) BFD_FAIL(-10, "placement: the pair probe failed");
        if (t0[a] <= tSame) samples.push_back(t0[a]);
        if (P.verbose) { char q[48]; snprintf(q, sizeof q, " %d:%.3f", a, t0[a]); P.times += q; }
    }
    std::sort(samples.begin(), samples.end());
    float thr = 0.95f * samples.front(), widest = 0.f;
    for (size_t q = 0; q + 1 < samples.size(); q++) {
        const float gap = samples[q + 1] / samples[q] - 1.0f;
        if (gap > widest) { widest = gap; if (gap >= 0.035f) thr = 0.5f * (samples[q] + samples[q + 1]); }
    }
    L.tSame = tSame; L.thr = thr; L.widest = widest; L.t0 = t0;
    return 0;
}

// region classes of the state-sized buffers, by comparison with one representative per class
int classify(Probe &P, const Levels &L, Classes &C)
{
    const size_t g = P.g;
    std::vector<Buf> &pool = C.pool;
    std::vector<float *> &repOf = C.repOf;
    for (int a = 0; a < P.nBuf; a++) {
        Buf b = {P.base(a), -1, false};
        for (size_t c = 0; c < repOf.size() && b.cls < 0; c++) {
            const float t = (c == 0 && a > 0) ? L.t0[a] : P.pair(repOf[c], b.base + g);
            if (t <= 0) BFD_FAIL(-10, "placement: the pair probe failed");
            if (P.verbose && c > 0) { char q[48]; snprintf(q, sizeof q, " %d/%zu:%.3f", a, c, t); P.times += q; }
            if (t >= L.thr) b.cls = (int)c;
        }
        if (b.cls < 0) { b.cls = (int)repOf.size(); repOf.push_back(b.base + g); }
        pool.push_back(b);
    }
    int M = 0;
    {
        std::vector<int> cnt(repOf.size(), 0);
        for (const Buf &b : pool) cnt[b.cls]++;
        for (size_t c = 0; c < cnt.size(); c++) if (cnt[c] > cnt[M]) M = (int)c;
    }
    C.M = M;
    return 0;
}

// stream order: arrays that a kernel WRITES together are neighbours in this list, and the list alternates between the
// most populated region M and "anywhere else":
//   velocity kernels write Vx Vy Vz (+ accumulator); stress_fluid Szz Rzz (+ Vz of the advancing runs, which already lies apart from Szz); stress_solid Sxx Syy Szz Rxx Ryy Rzz;
//   the sparse shear kernel Sxy Sxz Syz Rxy Rxz Ryz
Order stream_order(bool pingpong, bool solids)
{
    std::vector<int> order = {0, 1, 2, 5, 11};                               // Vx Vy Vz Szz Rzz
    std::vector<int> side = {0, 1, 0, 1, 0};                                 // 0: region M, 1: elsewhere
    if (pingpong) for (int a = 15; a < 20; a++) { order.push_back(a); side.push_back((a - 15) & 1); }   // the second copies like the first (the sums lie apart from Vz and from its copy)
    if (solids) { int q = 1; for (int a : {3, 9, 4, 10, 6, 12, 7, 13, 8, 14}) { order.push_back(a); side.push_back(q); q ^= 1; } }   // Sxx Rxx Syy Ryy Sxy Rxy Sxz Rxz Syz Ryz
    return {order, side};
}

// How much throw-away memory the search for another region may hold at a time (candidates that missed + spacers, all freed
// before bfd_choose_placement returns). A region is up to ~96 GiB wide and a fresh process may start at the beginning of one (boxes
// needed 92-160 GiB of candidates), but a solver call must not take the device away from whoever shares it: NOTHING is searched
// when other allocations than this engine's are present on the device (another process, the other slabs of a group, a GUI's
// bio-heat volumes): the buffers are then only exchanged among themselves. On a device the engine has to itself the search may
// hold up to 192 GiB while always leaving 48 GiB of what was free on entry untouched (round 4 had capped it at 64 GiB, which
// gives up on some boxes -- C3 85 instead of 91 Gvoxel-steps/s there; since round 5 a successful search is paid once per
// process: its buffers are kept for the next engine, the cache above).
// Precedence, later rules override earlier ones:
//   1. the default rule: 192 GiB, never more than two thirds of what was free on entry (an empty 288 GB device keeps 90 GiB for whoever comes),
//      always leaving 48 GiB; it walks by the clock (BABELFDTD_PLACEMENT_SEARCH_SECONDS, default 2) and watches the device's free memory:
//      allocations that are neither this engine's nor the search's own (another process that started at the same moment) end it at once and
//      everything held goes back;
//   2. the shared-device rule: more than 6 GiB of other allocations: no search (cap 0), and the note says so;
//   3. BABELFDTD_PLACEMENT_SEARCH_GIB replaces the 192 GiB (the owner of the device raises or lowers the default bound without code), still
//      leaving 48 GiB, and only on a device that is not shared; the clock and the watch of rule 1 stay on;
//   4. bfd_set_placement(sim, mode, limitBytes >= 0): that limit; the shared-device rule, the clock and the watch are off: the caller has decided;
//   5. BFD_PLACEMENT_SEARCH_MB (tests: walk a little on any grid): as 4, and the probe counts as telling whatever its duration.
// A cap of 0 from whichever rule means that the probe tells nothing: no candidate is drawn, for the accumulators either.
Budget search_budget(bfd_sim *s, float tSame)
{
    bool probeTells = tSame >= 0.05f;                                          // ms; shorter probes are launch overhead, not memory time
    size_t free0 = 0, total0 = 0;
    if (hipMemGetInfo(&free0, &total0) != hipSuccess) { free0 = total0 = 0; (void)hipGetLastError(); }
    // what this process keeps from an earlier engine's search (the cache) is the engine's to take, not somebody else's memory
    const size_t mine = (size_t)s->devBytes + placement_cache_bytes(s->cfg.device);
    const size_t others = total0 > free0 + mine ? total0 - free0 - mine : 0;
    size_t heldCap = free0 > ((size_t)48 << 30) ? std::min(std::min((size_t)192 << 30, free0 / 3 * 2), free0 - ((size_t)48 << 30)) : 0;
    bool defaultRule = true;
    double searchSeconds = 2.0;                                                // BABELFDTD_PLACEMENT_SEARCH_SECONDS
    if (const char *ev = getenv("BABELFDTD_PLACEMENT_SEARCH_SECONDS")) searchSeconds = atof(ev);
    std::string capNote;
    if (others > ((size_t)6 << 30)) { heldCap = 0; char q[96]; snprintf(q, sizeof q, "; device shared (%.0f GiB of other allocations): no search beyond the own buffers", others / 1073741824.0); capNote = q; }
    if (const char *ev = getenv("BABELFDTD_PLACEMENT_SEARCH_GIB")) {
        const double gib = atof(ev);
        if (gib >= 0 && others <= ((size_t)6 << 30)) heldCap = std::min((size_t)(gib * 1073741824.0), free0 > ((size_t)48 << 30) ? free0 - ((size_t)48 << 30) : 0);
    }
    if (s->placementLimit >= 0) { heldCap = (size_t)s->placementLimit; capNote.clear(); defaultRule = false; }
    if (const char *ev = getenv("BFD_PLACEMENT_SEARCH_MB")) { probeTells = true; heldCap = (size_t)atol(ev) << 20; capNote.clear(); defaultRule = false; }
    if (heldCap == 0) probeTells = false;
    return {heldCap, defaultRule, searchSeconds, probeTells, capNote, mine, others};
}

// a buffer on the side that is short joins the pool; `held` owns it until the commit stage
void take_fresh(Classes &C, Found &F, Held &held, float *c, int sd)
{
    C.pool.push_back({c, sd == 0 ? C.M : 100 + F.nFresh, true});
    held.fresh.push_back(c);
    F.need[sd]--; F.nFresh++;
}

// first what an earlier engine of this process found. Gated by the probe's duration itself, not by Budget::probeTells: with
// BFD_PLACEMENT_SEARCH_MB on a small grid the search below walks, but nothing is drawn from the cache (kept as it was).
void fill_from_cache(Probe &P, const Levels &L, Classes &C, Found &F, Held &held)
{
    bfd_sim *s = P.s;
    if (!((F.need[0] > 0 || F.need[1] > 0) && L.tSame >= 0.05f)) return;
    for (void *cp : placement_cache_take(s->cfg.device, P.bytes)) {
        float *c = (float *)cp;
        int sd = -1;
        if (hipMemsetAsync(c, 0, P.bytes, s->stream) == hipSuccess) { const float t = P.pair(C.repOf[C.M], c + P.g); if (t > 0) sd = t >= L.thr ? 0 : 1; }
        if (sd >= 0 && F.need[sd] > 0) { take_fresh(C, F, held, c, sd); F.nCached++; }
        else { hipStreamSynchronize(s->stream); held.discard(c); }
    }
}

// draw candidates until both sides have enough
void search(Probe &P, const Levels &L, Classes &C, const Budget &B, std::chrono::steady_clock::time_point tStart, Found &F, Held &held)
{
    size_t ownFreshBytes = 0;                                                  // fresh buffers drawn here (the cached ones are part of `mine`)
    while ((F.need[0] > 0 || F.need[1] > 0) && !F.gaveUp && B.probeTells) {
        // the default rule's clock and watch: the state arrays' search only
        float *c = held.draw(P.bytes, [&](size_t freeB, size_t totalB) {
            if (!B.defaultRule) return false;
            // ... and a clock: what the placement is worth to ONE solver call is a few per cent of its run time, so a search that has walked for longer than
            // that (seen once: ~6 s in a process that had built and destroyed many engines before) stops and keeps what exchanging gives
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - tStart).count() > B.searchSeconds) { F.ended += "; search ended by its time bound"; return true; }
            const size_t known = B.mine + held.bytes + ownFreshBytes + B.others;
            if (totalB > freeB + known && totalB - freeB - known > ((size_t)6 << 30)) { F.ended += "; somebody else began to allocate on the device: search ended"; return true; }
            return false;
        });
        if (!c) { F.gaveUp = true; break; }
        const float t = P.pair(C.repOf[C.M], c + P.g);
        if (t <= 0) { held.discard(c); F.gaveUp = true; break; }
        const int side = t >= L.thr ? 0 : 1;
        if (F.need[side] > 0) { take_fresh(C, F, held, c, side); ownFreshBytes += P.bytes; continue; }
        held.keep_miss(c, P.bytes);
    }
}

// which buffer every array gets: slotBuf[array] = index into the pool, taken[index]
void assign(const Probe &P, const Classes &C, const Order &O, std::vector<char> &taken, std::vector<int> &slotBuf)
{
    const std::vector<Buf> &pool = C.pool;
    taken.assign(pool.size(), 0);
    slotBuf.assign(P.nBuf, -1);
    auto pick = [&](int side, int prefer) -> int {
        if (!taken[prefer] && C.sideOf(pool[prefer]) == side) return prefer;
        for (int pass = 0; pass < 2; pass++)                                   // original buffers first, fresh ones after
            for (size_t q = 0; q < pool.size(); q++) if (!taken[q] && C.sideOf(pool[q]) == side && pool[q].fresh == (pass == 1)) return (int)q;
        return -1;
    };
    for (size_t q = 0; q < O.order.size(); q++) {
        const int a = O.order[q];
        int p = pick(O.side[q], a);
        if (p < 0) p = pick(1 - O.side[q], a);                                 // nothing on the wanted side
        taken[p] = 1; slotBuf[a] = p;
    }
    // the arrays outside the list take what is left of the original buffers; unused fresh ones and the held misses are released
    for (int a = 0; a < P.nBuf; a++) {
        if (slotBuf[a] >= 0) continue;
        int p = -1;
        for (size_t q = 0; q < pool.size() && p < 0; q++) if (!taken[q] && !pool[q].fresh) p = (int)q;
        for (size_t q = 0; q < pool.size() && p < 0; q++) if (!taken[q]) p = (int)q;
        taken[p] = 1; slotBuf[a] = p;
    }
}

int commit(const Probe &P, const Classes &C, const std::vector<char> &taken, const std::vector<int> &slotBuf, Held &held)
{
    bfd_sim *s = P.s;
    BFD_HIP(hipStreamSynchronize(s->stream));
    // From here on every pointer has exactly one owner. A fresh buffer that an array took is the engine's: s->allocs frees it at bfd_destroy,
    // unless the cache takes it there (s->searched). A fresh buffer nothing took goes back now. An original that a fresh one displaced leaves
    // s->allocs and is freed here. `held` keeps the misses and the spacers and nothing else.
    held.fresh.clear();
    for (size_t q = 0; q < C.pool.size(); q++) {
        const Buf &b = C.pool[q];
        if (taken[q]) { if (b.fresh) { s->allocs.push_back(b.base); s->searched.push_back(b.base); } continue; }
        if (b.fresh) { held.discard(b.base); continue; }
        auto it = std::find(s->allocs.begin(), s->allocs.end(), (void *)b.base);
        if (it != s->allocs.end()) s->allocs.erase(it);
        hipFree(b.base);
    }
    for (int a = 0; a < P.nBuf; a++) P.base(a) = C.pool[slotBuf[a]].base;
    bfd_bind_state_views(s);
    return 0;
}

// Pressure accumulators: written beside Vx Vy Vz by the velocity kernels: the RMS sums go to another region than Vz, a
// peak map beside them to another region than the sums
std::string place_accumulators(Probe &P, const Levels &L, const Budget &B)
{
    bfd_sim *s = P.s;
    std::string accNote;
    float *prevRep = s->stateBase[2] + P.g;
    for (int which = 0; which < 2; which++) {
        float **pp = which == 0 ? &s->acc : &s->pk;
        if (!*pp) continue;
        int qP = -1;
        for (int q = 0; q < s->nSelR; q++) if (s->selR[q] == BFD_MAP_PRESSURE) qP = q;
        if (qP < 0) continue;
        const size_t accBytes = (size_t)s->nSelR * s->nloc * sizeof(float);
        float *cur = *pp;
        float t = P.pair(prevRep, cur + (size_t)qP * s->nloc);
        // this accumulator's own misses: counted from zero against the same cap, at most 80 blocks, gone before the next accumulator is treated
        Held miss(s->stream, B.heldCap);
        while (t >= L.thr && miss.ptrs.size() < 80 && B.probeTells) {          // same region as its neighbour: look for another buffer
            float *c = miss.draw(accBytes);
            if (!c) break;
            const float tc = P.pair(prevRep, c + (size_t)qP * s->nloc);
            if (tc <= 0) { miss.discard(c); break; }
            if (tc < L.thr) {                                                  // the accumulator moves: its old buffer was the engine's, the new one is
                auto it = std::find(s->allocs.begin(), s->allocs.end(), (void *)cur);
                if (it != s->allocs.end()) s->allocs.erase(it);
                hipStreamSynchronize(s->stream);
                hipFree(cur);
                cur = c; s->allocs.push_back(c); t = tc;
            } else miss.keep_miss(c, accBytes);
        }
        hipStreamSynchronize(s->stream);
        miss.release();
        *pp = cur;
        accNote += std::string(which == 0 ? " sums " : " peaks ") + (t > 0 && t < L.thr ? "apart from" : "WITH") + (which == 0 ? " Vz," : " the sums,");
        prevRep = cur + (size_t)qP * s->nloc;
    }
    return accNote;
}

}  // namespace

int bfd_choose_placement(bfd_sim *s)
{
    if (!placement_wanted(s)) return 0;
    BFD_HIP(hipSetDevice(s->cfg.device));
    const auto tStart = std::chrono::steady_clock::now();
    Probe P(s);
    Levels L;
    Classes C;
    int rc = find_threshold(P, L);
    if (!rc) rc = classify(P, L, C);
    if (rc) return rc;
    const bool solids = s->tiles.nSolid > 0 || s->cfg.kernelVariant == 2;
    const Order O = stream_order(s->pingpong, solids);
    std::string before;
    for (int a : O.order) before += (char)('0' + std::min(C.pool[a].cls, 9));
    Found F = {{0, 0}, 0, 0, false, ""};
    for (int sd : O.side) F.need[sd]++;
    for (const Buf &b : C.pool) F.need[C.sideOf(b)]--;                        // spare arrays count: their buffers can be exchanged in
    const Budget B = search_budget(s, L.tSame);
    Held held(s->stream, B.heldCap);
    fill_from_cache(P, L, C, F, held);
    search(P, L, C, B, tStart, F, held);
    std::vector<char> taken;
    std::vector<int> slotBuf;
    assign(P, C, O, taken, slotBuf);
    rc = commit(P, C, taken, slotBuf, held);
    if (rc) return rc;
    const std::string accNote = place_accumulators(P, L, B);
    BFD_HIP(hipStreamSynchronize(s->stream));
    const size_t nHeld = held.ptrs.size(), heldBytes = held.bytes;
    held.release();
    std::string after;
    for (int a : O.order) { const Buf &b = C.pool[slotBuf[a]]; after += b.fresh ? (b.cls == C.M ? 'm' : 'n') : (char)('0' + std::min(b.cls, 9)); }
    char buf[1024];
    snprintf(buf, sizeof buf, "arrays placed by memory region (pair probe on the zero state: %d probes, within-region %.3f ms, threshold %.3f ms, gap between the levels %.0f %%; %zu regions seen): "
             "regions of %s %s -> %s (m / n = fresh allocation in / outside the most populated region),%s %d fresh, %zu candidates / spacers (%.1f GiB) released%s; %.2f s", P.nProbes, L.tSame, L.thr, 100.0 * L.widest, C.repOf.size(),
             (std::string("Vx Vy Vz Szz Rzz") + (s->pingpong ? " + their second copies" : "") + (solids ? " Sxx Rxx Syy Ryy Sxy Rxy Sxz Rxz Syz Ryz" : "")).c_str(), before.c_str(), after.c_str(), accNote.c_str(), F.nFresh, nHeld, heldBytes / 1073741824.0,
             (std::string(F.gaveUp ? "; search for another region given up (limit / memory)" : "") + B.capNote + F.ended + (F.nCached ? "; " + std::to_string(F.nCached) + " of the fresh buffers came from an earlier search of this process" : "")).c_str(), std::chrono::duration<double>(std::chrono::steady_clock::now() - tStart).count());
    s->placementNote = buf;
    if (P.verbose) fprintf(stderr, "placement: %s\nplacement: probe times, array:ms against Vx, array/class:ms against the other representatives:%s\n", buf, P.times.c_str());
    return 0;
}

extern "C" int bfd_set_placement(bfd_sim *s, int32_t mode, int64_t searchLimitBytes)
{
    if (!s) BFD_FAIL(-1, "null sim");
    if (s->placementDone) BFD_FAIL(-6, "bfd_set_placement: the arrays are placed already (call it before the first step / bfd_prepare)");
    s->placementMode = mode != 0; s->placementLimit = searchLimitBytes;
    return 0;
}

extern "C" const char *bfd_placement_note(bfd_sim *s)
{
    if (!s) return "";
    if (!s->placementDone) return "not prepared yet";
    return s->placementNote.c_str();
}
