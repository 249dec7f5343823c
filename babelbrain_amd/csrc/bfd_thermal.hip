// The whole-volume work of the Step-3 exposure analysis on MI355X, in the caller's numpy C order (k fastest).
//
// Replace, in ThermalModeling/CalculateTemperatureEffects.py,
//     the two copies of pAmp, SoS[MaterialMap], Density[MaterialMap], the masked stores, the two np.where(x == x.max())
//     and the five plane energies of AnalyzeLosses                                       :142-216     -> bfd_loss_survey3d
//     ResTemp * Sel.astype(np.float32) and np.argmax, three times                        :996-1001    -> bfd_class_extrema3d
//     X[Sel].max(), six times, and p_map[SelBrain].argmax() with the value read          :1126-1144   -> bfd_class_extrema3d
// The arithmetic per voxel is in bfd_thermal_core.h, which a plain C++ compiler accepts too.
//
//   extrema   quads of voxels (one 128-bit load per volume, the ids as one, two or four words) in a grid-stride loop. A thread keeps, for each of the
//             8 classes, the count, the first voxel outside the class and one (value, index) pair per volume as a 64-bit word (th_pair). Threads fold
//             into LDS and workgroups into global memory with integer atomics (max, min, add): the result does not depend on their order.
//   survey    lanes along k, ROWS rows of (i, j) per workgroup: a lane adds the terms of its k over the workgroup's rows, in ascending row order, into
//             three private float64 sums and writes them as partials [chunk][3][N3]. The two maxima are pairs, folded like those of the extrema.
//   fold      a tree over the chunks, 32 to a node, every node added in ascending order by one thread per (sum, k); the levels are launches.
//             ROWS and the 32 are constants, so the sums are the same bytes for any launch.
// No floating-point atomics. No kernel waits for another workgroup; every loop is bounded, see the comment at each.
#include <string.h>
#include "bfd_internal.h"
#include "bfd_call.h"
#include "bfd_thermal_core.h"
#include "bfd_thermal_stages.h"

namespace {

constexpr int THREADS = 256;
const char *const DATA_REFUSED = ": refused data: ";   // what every data refusal carries after the entry's name (ThermalAnalysis.py turns these into ValueError)
constexpr int64_t SWEEP_BLOCKS = 1024;                 // extrema: what lies beyond is taken by the grid-stride loop
constexpr int MAX_VOL = 4;                             // volumes one launch of the extrema kernel reads; more take further launches over the same map
constexpr int ROWS = 128;                              // rows of (i, j) one workgroup of the survey owns: a constant, never a function of the grid
constexpr int LDS_MATERIALS = 2048;                    // rows of the class table kept in LDS; a longer table is read from global memory
constexpr int LDS_PROPERTIES = 1280;                   // rows of rho and c kept in LDS by the survey (a CT-derived list has up to 1030): 20 KiB, so that
                                                       // six workgroups fit a CU; with 2048 rows four did: 1.085 against 1.005 ms at 448 x 448 x 384 (profiles/README.md, "Thermal analysis")
constexpr int FOLD = 32;                               // partial sums one node of the fold adds: a constant, like ROWS
constexpr uint32_t FLAG_ID = 1u, FLAG_VALUE = 2u;
constexpr uint32_t NO_INDEX = 0xFFFFFFFFu;

// the ids of quad q, widened
template <int IDB>
static __device__ __forceinline__ void th_load_ids(const void *map, int64_t q, uint32_t id[4])
{
    if (IDB == 1) {
        const uint32_t w = ((const uint32_t *)map)[q];
        id[0] = w & 0xFFu; id[1] = (w >> 8) & 0xFFu; id[2] = (w >> 16) & 0xFFu; id[3] = w >> 24;
    } else if (IDB == 2) {
        const uint2 w = ((const uint2 *)map)[q];
        id[0] = w.x & 0xFFFFu; id[1] = w.x >> 16; id[2] = w.y & 0xFFFFu; id[3] = w.y >> 16;
    } else {
        const uint4 w = ((const uint4 *)map)[q];
        id[0] = w.x; id[1] = w.y; id[2] = w.z; id[3] = w.w;
    }
}

template <int IDB>
static __device__ __forceinline__ uint32_t th_load_id(const void *map, int64_t i)
{
    if (IDB == 1) return ((const uint8_t *)map)[i];
    if (IDB == 2) return ((const uint16_t *)map)[i];
    return ((const uint32_t *)map)[i];
}

// ---------------------------------------------------------------- extrema ----------------------------------------------------------------

struct extrema_args { const float *vol[MAX_VOL]; };

// out: pairs [NV][8] (start TH_NO_PAIR), then counts [8] (start 0) as 64-bit words; firstOut: [8] (start NO_INDEX); flags: one word (start 0).
// The volumes and the map are padded to whole quads; n is the number of voxels.
template <int IDB, int NV>
__global__ __launch_bounds__(THREADS) void th_extrema(const extrema_args a, const void *__restrict__ map, int64_t n, int64_t quads, const uint8_t *__restrict__ classOf,
                                                      int nMat, unsigned long long *__restrict__ out, uint32_t *__restrict__ firstOut, uint32_t *__restrict__ flags)
{
    __shared__ uint8_t tab[LDS_MATERIALS];
    __shared__ unsigned long long sPair[NV * TH_CLASSES], sCount[TH_CLASSES];
    __shared__ uint32_t sFirst[TH_CLASSES], sFlags;
    const bool inLds = nMat <= LDS_MATERIALS;
    if (inLds) for (int w = threadIdx.x; w < nMat; w += THREADS) tab[w] = classOf[w];
    if (threadIdx.x < NV * TH_CLASSES) sPair[threadIdx.x] = TH_NO_PAIR;
    if (threadIdx.x < TH_CLASSES) { sCount[threadIdx.x] = 0; sFirst[threadIdx.x] = NO_INDEX; }
    if (threadIdx.x == 0) sFlags = 0;
    __syncthreads();

    unsigned long long pair[NV][TH_CLASSES];
    uint32_t cnt[TH_CLASSES], first[TH_CLASSES], bad = 0;
#pragma unroll
    for (int c = 0; c < TH_CLASSES; c++) {
        cnt[c] = 0; first[c] = NO_INDEX;
#pragma unroll
        for (int v = 0; v < NV; v++) pair[v][c] = TH_NO_PAIR;
    }
    for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * THREADS) {         // grid-stride: ends
        uint32_t id[4];
        th_load_ids<IDB>(map, q, id);
        uint4 x[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) x[v] = ((const uint4 *)a.vol[v])[q];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int64_t i = 4 * q + b;
            if (i >= n) continue;
            uint32_t m = 0;
            if (id[b] < (uint32_t)nMat) m = inLds ? tab[id[b]] : classOf[id[b]];          // never outside the table, whatever the map holds
            else bad |= FLAG_ID;
#pragma unroll
            for (int c = 0; c < TH_CLASSES; c++) {
                const bool in = (m >> c) & 1u;
                cnt[c] += in ? 1u : 0u;               // a thread sees fewer than 2^31 voxels
                if (!in && first[c] == NO_INDEX) first[c] = (uint32_t)i;                  // a thread's indices ascend
            }
#pragma unroll
            for (int v = 0; v < NV; v++) {
                const uint32_t bits = b == 0 ? x[v].x : b == 1 ? x[v].y : b == 2 ? x[v].z : x[v].w;
                if (!th_finite(bits)) bad |= FLAG_VALUE;
                const unsigned long long p = th_pair(th_key(bits), (uint32_t)i);
#pragma unroll
                for (int c = 0; c < TH_CLASSES; c++)
                    if ((m >> c) & 1u) pair[v][c] = th_pair_max(pair[v][c], p);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < TH_CLASSES; c++) {
        if (cnt[c]) atomicAdd(&sCount[c], (unsigned long long)cnt[c]);
        if (first[c] != NO_INDEX) atomicMin(&sFirst[c], first[c]);
#pragma unroll
        for (int v = 0; v < NV; v++)
            if (pair[v][c] != TH_NO_PAIR) atomicMax(&sPair[v * TH_CLASSES + c], pair[v][c]);
    }
    if (bad) atomicOr(&sFlags, bad);
    __syncthreads();
    if (threadIdx.x < NV * TH_CLASSES && sPair[threadIdx.x] != TH_NO_PAIR) atomicMax(out + threadIdx.x, sPair[threadIdx.x]);
    if (threadIdx.x < TH_CLASSES) {
        if (sCount[threadIdx.x]) atomicAdd(out + MAX_VOL * TH_CLASSES + threadIdx.x, sCount[threadIdx.x]);
        if (sFirst[threadIdx.x] != NO_INDEX) atomicMin(firstOut + threadIdx.x, sFirst[threadIdx.x]);
    }
    if (threadIdx.x == 0 && sFlags) atomicOr(flags, sFlags);
}

// ---------------------------------------------------------------- survey ----------------------------------------------------------------

struct survey_args {
    const float *p;
    float *pw;                                         // read, and written in place where writeWater is set
    const void *map;
    const uint8_t *brainMask;                          // or null: bit 0 of the class table
    const uint8_t *classOf;
    const double *rho, *c;
    int nMat, writeWater;
    int64_t rows, N3;                                  // rows = N1 * N2
    unsigned kBlocks;                                  // ceil(N3 / THREADS)
    double rhoWater, cWater, dx2;
};

// grid: chunks of ROWS rows x kBlocks blocks of THREADS values of k, as one dimension (workgroup = chunk * kBlocks + kBlock).
// partial: [chunk][3][N3] (raw water, water, tissue), every word written.
// pairs: [2] (tissue, water; start TH_NO_PAIR); flags: one word (start 0).
template <int IDB>
__global__ __launch_bounds__(THREADS) void th_survey(const survey_args a, double *__restrict__ partial, unsigned long long *__restrict__ pairs, uint32_t *__restrict__ flags)
{
    __shared__ uint8_t tab[LDS_PROPERTIES];
    __shared__ double sRho[LDS_PROPERTIES], sC[LDS_PROPERTIES];
    __shared__ unsigned long long sPair[2];
    __shared__ uint32_t sFlags;
    const bool inLds = a.nMat <= LDS_PROPERTIES;
    if (inLds) for (int w = threadIdx.x; w < a.nMat; w += THREADS) { tab[w] = a.classOf[w]; sRho[w] = a.rho[w]; sC[w] = a.c[w]; }
    if (threadIdx.x < 2) sPair[threadIdx.x] = TH_NO_PAIR;
    if (threadIdx.x == 0) sFlags = 0;
    __syncthreads();

    const int64_t chunk = blockIdx.x / a.kBlocks;
    const int64_t k = (int64_t)(blockIdx.x % a.kBlocks) * THREADS + threadIdx.x;
    const int64_t r0 = chunk * ROWS, r1 = r0 + ROWS < a.rows ? r0 + ROWS : a.rows;
    double eRaw = 0.0, eWater = 0.0, eTissue = 0.0;
    unsigned long long best[2] = {TH_NO_PAIR, TH_NO_PAIR};
    uint32_t bad = 0;
    if (k < a.N3) {
#pragma unroll 4
        for (int64_t r = r0; r < r1; r++) {            // at most ROWS trips
            const int64_t i = r * a.N3 + k;
            const uint32_t pb = __float_as_uint(a.p[i]), wb = __float_as_uint(a.pw[i]);
            const uint32_t id = th_load_id<IDB>(a.map, i);
            uint32_t m = 0;
            double R = 1.0, C = 1.0;
            if (id < (uint32_t)a.nMat) {               // never outside the tables, whatever the map holds
                m = inLds ? tab[id] : a.classOf[id];
                R = inLds ? sRho[id] : a.rho[id];
                C = inLds ? sC[id] : a.c[id];
            } else bad |= FLAG_ID;
            if (!th_finite(pb) || !th_finite(wb)) bad |= FLAG_VALUE;
            const bool brain = a.brainMask ? a.brainMask[i] != 0 : (m & 1u) != 0;
            const bool cleared = (m & 2u) != 0;
            const double tw = th_term(wb, a.rhoWater, a.cWater, a.dx2);
            eRaw += tw;
            // a cleared water voxel and a tissue voxel outside the brain are 0.0f: with rho, c > 0 and dx2 >= 0 their term is +0, which changes no sum
            if (!cleared) eWater += tw;
            if (brain) eTissue += th_term(pb, R, C, a.dx2);
            best[0] = th_pair_max(best[0], th_pair(th_masked_key(pb, brain), (uint32_t)i));
            best[1] = th_pair_max(best[1], th_pair(th_masked_key(wb, !cleared), (uint32_t)i));
            if (a.writeWater && cleared) a.pw[i] = 0.0f;
        }
        double *out = partial + chunk * 3 * a.N3 + k;
        out[0] = eRaw; out[a.N3] = eWater; out[2 * a.N3] = eTissue;
        atomicMax(&sPair[0], best[0]);
        atomicMax(&sPair[1], best[1]);
        if (bad) atomicOr(&sFlags, bad);
    }
    __syncthreads();
    if (threadIdx.x < 2 && sPair[threadIdx.x] != TH_NO_PAIR) atomicMax(pairs + threadIdx.x, sPair[threadIdx.x]);
    if (threadIdx.x == 0 && sFlags) atomicOr(flags, sFlags);
}

// out[g][t] = in[g * FOLD][t] + ... + in[g * FOLD + FOLD - 1][t] (as far as `count` goes), added in ascending order from +0: one node of the
// tree. FOLD loads are in flight before the first addition: a thread that adds 1568 partials one load at a time spends 0.5 ms waiting.
__global__ __launch_bounds__(THREADS) void th_fold(const double *__restrict__ in, int64_t count, int64_t width, double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x, g = blockIdx.y;
    if (t >= width) return;
    const int64_t first = g * FOLD;
    double v[FOLD];
#pragma unroll
    for (int j = 0; j < FOLD; j++) v[j] = first + j < count ? in[(first + j) * width + t] : 0.0;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < FOLD; j++)
        if (first + j < count) s += v[j];
    out[g * width + t] = s;
}

// ---------------------------------------------------------------- host ----------------------------------------------------------------

static const char *check_common(const void *map, int idBytes, int64_t N1, int64_t N2, int64_t N3, const uint8_t *classOf, int nMat)
{
    if (!map || !classOf) return ": null argument";
    if (N1 < 0 || N2 < 0 || N3 < 0) return ": negative dimension";
    if (!volume_fits(N1, N2, N3)) return ": the volume has 2^31 voxels or more (limit: fewer than 2^31)";
    if (idBytes != 1 && idBytes != 2 && idBytes != 4) return ": idBytes must be 1, 2 or 4";
    if (nMat < 1 || nMat > TH_MAX_MATERIALS) return ": nMat must be 1 .. 65536";
    return nullptr;
}

static bool positive_finite(double v) { return v > 0.0 && v - v == 0.0; }

// n items of `item` bytes on the device, padded with zeros to whole quads
struct Padded {
    DevTemp<uint8_t> d;
    size_t bytes = 0, padded = 0;
    hipError_t reserve(size_t n, size_t item)
    {
        bytes = n * item; padded = (n + 3) / 4 * 4 * item;
        hipError_t e = d.alloc(padded);
        if (e == hipSuccess && padded > bytes) e = hipMemset(d.p + bytes, 0, padded - bytes);
        return e;
    }
    hipError_t upload(const void *host) { return hipMemcpy(d.p, host, bytes, hipMemcpyHostToDevice); }
};

template <int IDB>
static void launch_extrema(int nv, unsigned blocks, const extrema_args &a, const void *map, int64_t n, int64_t quads, const uint8_t *classOf, int nMat,
                           unsigned long long *out, uint32_t *firstOut, uint32_t *flags)
{
#define TH_EXTREMA(NV) hipLaunchKernelGGL((th_extrema<IDB, NV>), dim3(blocks), dim3(THREADS), 0, 0, a, map, n, quads, classOf, nMat, out, firstOut, flags)
    if (nv == 1) TH_EXTREMA(1); else if (nv == 2) TH_EXTREMA(2); else if (nv == 3) TH_EXTREMA(3); else TH_EXTREMA(4);
#undef TH_EXTREMA
}

}  // namespace

extern "C" int bfd_class_extrema3d(int device, const float *const *volumes, int nVol, const void *map, int idBytes, int64_t N1, int64_t N2, int64_t N3,
                                   const uint8_t *classOf, int nMat, int64_t *count, float *maxIn, int64_t *argIn, float *maxKey, int64_t *argKey,
                                   float *kernelMs)
{
    static const char *who = "bfd_class_extrema3d";
    // every argument error is reported before a device is looked for
    if (!volumes || !count || !maxIn || !argIn || !maxKey || !argKey) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (const char *bad = check_common(map, idBytes, N1, N2, N3, classOf, nMat)) BFD_FAIL(-1, std::string(who) + bad);
    if (nVol < 1) BFD_FAIL(-1, std::string(who) + ": nVol must be at least 1");
    for (int v = 0; v < nVol; v++)
        if (!volumes[v]) BFD_FAIL(-1, std::string(who) + ": null argument");
    const size_t n = (size_t)(N1 * N2 * N3), slots = (size_t)nVol * TH_CLASSES;
    if (n) {
        const struct { const void *p; size_t b; } outs[5] = {{count, 8 * (size_t)TH_CLASSES}, {maxIn, 4 * slots}, {argIn, 8 * slots}, {maxKey, 4 * slots}, {argKey, 8 * slots}};
        for (int o = 0; o < 5; o++) {
            bool hit = overlap(map, n * (size_t)idBytes, outs[o].p, outs[o].b) || overlap(classOf, (size_t)nMat, outs[o].p, outs[o].b) ||
                       overlap(volumes, sizeof(void *) * (size_t)nVol, outs[o].p, outs[o].b);
            for (int v = 0; v < nVol; v++) hit = hit || overlap(volumes[v], 4 * n, outs[o].p, outs[o].b);
            for (int o2 = 0; o2 < o; o2++) hit = hit || overlap(outs[o2].p, outs[o2].b, outs[o].p, outs[o].b);
            if (hit) BFD_FAIL(-1, std::string(who) + ": an output may not alias an input or another output");
        }
    }

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    std::vector<unsigned long long> pairs(slots, TH_NO_PAIR);
    unsigned long long counts[TH_CLASSES] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t first[TH_CLASSES], flags = 0;
    for (int c = 0; c < TH_CLASSES; c++) first[c] = NO_INDEX;
    float total = 0.f;
    if (n) {
        std::vector<Padded> vols((size_t)nVol);
        std::vector<const float *> dvols((size_t)nVol);
        Padded dmap;
        DevTemp<uint8_t> dtab, dscratch;
        for (int v = 0; v < nVol; v++) BFD_STEP(vols[(size_t)v].reserve(n, 4));
        BFD_STEP(dmap.reserve(n, (size_t)idBytes));
        BFD_STEP(dtab.alloc((size_t)nMat));
        BFD_STEP(dscratch.alloc(bfd_class_extrema_scratch()));
        for (int v = 0; v < nVol; v++) { BFD_STEP(vols[(size_t)v].upload(volumes[v])); dvols[(size_t)v] = (const float *)vols[(size_t)v].d.p; }
        BFD_STEP(dmap.upload(map));
        BFD_STEP(hipMemcpy(dtab, classOf, (size_t)nMat, hipMemcpyHostToDevice));
        BFD_STEP(bfd_stage_class_extrema(dvols.data(), nVol, dmap.d.p, idBytes, (int64_t)n, dtab.p, nMat, dscratch.p, pairs.data(), counts, first, &flags, &total,
                                         nullptr, nullptr));
    }
    if (const int refused = bfd_class_extrema_finish(nVol, pairs.data(), counts, first, flags, count, maxIn, argIn, maxKey, argKey))
        BFD_FAIL(-1, std::string(who) + DATA_REFUSED + (refused == 1 ? "an id of the map is not below nMat" : "a value is not finite"));
    if (kernelMs) *kernelMs = total;
    return 0;
}

size_t bfd_class_extrema_scratch(void) { return (MAX_VOL + 1) * TH_CLASSES * sizeof(unsigned long long) + (TH_CLASSES + 1) * sizeof(uint32_t); }

hipError_t bfd_stage_class_extrema(const float *const *dVolumes, int nVol, const void *dMap, int idBytes, int64_t n, const uint8_t *dClassOf, int nMat,
                                   void *scratch, unsigned long long *pairs, unsigned long long *counts, uint32_t *first, uint32_t *flags, float *kernelMs,
                                   int64_t *bytesUp, int64_t *bytesDown)
{
#define TH_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)
    unsigned long long *dout = (unsigned long long *)scratch;
    uint32_t *dsmall = (uint32_t *)(dout + (MAX_VOL + 1) * TH_CLASSES);                      // firstOut [8], flags
    const int64_t quads = (n + 3) / 4;
    Events ev;
    TH_TRY(ev.create());
    const unsigned blocks = blocks_for(quads, THREADS, SWEEP_BLOCKS);
    for (int v0 = 0; v0 < nVol; v0 += MAX_VOL) {  // ceil(nVol / 4) launches over the same map
        const int nv = std::min(MAX_VOL, nVol - v0);
        unsigned long long init[(MAX_VOL + 1) * TH_CLASSES];
        uint32_t small[TH_CLASSES + 1];
        for (int q = 0; q < (MAX_VOL + 1) * TH_CLASSES; q++) init[q] = 0;
        for (int c = 0; c < TH_CLASSES; c++) small[c] = NO_INDEX;
        small[TH_CLASSES] = 0;
        extrema_args a;
        for (int v = 0; v < MAX_VOL; v++) a.vol[v] = dVolumes[v0 + std::min(v, nv - 1)];
        float ms = 0.f;
        TH_TRY(hipMemcpy(dout, init, sizeof init, hipMemcpyHostToDevice));
        TH_TRY(hipMemcpy(dsmall, small, sizeof small, hipMemcpyHostToDevice));
        TH_TRY(ev.record(0));
        if (idBytes == 1) launch_extrema<1>(nv, blocks, a, dMap, n, quads, dClassOf, nMat, dout, dsmall, dsmall + TH_CLASSES);
        else if (idBytes == 2) launch_extrema<2>(nv, blocks, a, dMap, n, quads, dClassOf, nMat, dout, dsmall, dsmall + TH_CLASSES);
        else launch_extrema<4>(nv, blocks, a, dMap, n, quads, dClassOf, nMat, dout, dsmall, dsmall + TH_CLASSES);
        TH_TRY(hipGetLastError());
        TH_TRY(ev.record(1));
        TH_TRY(ev.sync(1));
        TH_TRY(ev.elapsed(&ms, 0, 1));
        if (kernelMs) *kernelMs += ms;
        TH_TRY(hipMemcpy(init, dout, sizeof init, hipMemcpyDeviceToHost));
        TH_TRY(hipMemcpy(small, dsmall, sizeof small, hipMemcpyDeviceToHost));
        if (bytesUp) *bytesUp += (int64_t)(sizeof init + sizeof small);
        if (bytesDown) *bytesDown += (int64_t)(sizeof init + sizeof small);
        for (int v = 0; v < nv; v++)
            for (int c = 0; c < TH_CLASSES; c++) pairs[(size_t)(v0 + v) * TH_CLASSES + c] = init[v * TH_CLASSES + c];
        for (int c = 0; c < TH_CLASSES; c++) { counts[c] = init[MAX_VOL * TH_CLASSES + c]; first[c] = small[c]; }
        *flags |= small[TH_CLASSES];
    }
    return hipSuccess;
#undef TH_TRY
}

int bfd_class_extrema_finish(int nVol, const unsigned long long *pairs, const unsigned long long *counts, const uint32_t *first, uint32_t flags,
                             int64_t *count, float *maxIn, int64_t *argIn, float *maxKey, int64_t *argKey)
{
    if (flags & FLAG_ID) return 1;
    if (flags & FLAG_VALUE) return 2;
    const size_t slots = (size_t)nVol * TH_CLASSES;
    for (int c = 0; c < TH_CLASSES; c++) count[c] = (int64_t)counts[c];
    for (size_t s = 0; s < slots; s++) {
        const int c = (int)(s % TH_CLASSES);
        const unsigned long long in = pairs[s], keyed = th_keyed_pair(in, first[c] == NO_INDEX ? -1 : (int64_t)first[c]);
        maxIn[s] = in == TH_NO_PAIR ? 0.f : th_key_value(th_pair_key(in));
        argIn[s] = th_pair_index(in);
        maxKey[s] = keyed == TH_NO_PAIR ? 0.f : th_key_value(th_pair_key(keyed));
        argKey[s] = th_pair_index(keyed);
    }
    return 0;
}

void bfd_loss_survey_scratch(int64_t rows, int64_t N3, size_t *partialWords, size_t *sumWords)
{
    const int64_t chunks = (rows + ROWS - 1) / ROWS, width = 3 * N3;
    *partialWords = (size_t)(chunks * width);
    *sumWords = (size_t)(((chunks + FOLD - 1) / FOLD) * width);
}

hipError_t bfd_stage_loss_survey(const float *p, float *pw, const void *map, int idBytes, const uint8_t *brainMask, const uint8_t *classOf, const double *rho,
                                 const double *c, int nMat, int writeWater, int64_t rows, int64_t N3, double rhoWater, double cWater, double dx2, double *partial,
                                 double *sums, unsigned long long *pairs, uint32_t *flags, const double **result)
{
    const int64_t chunks = (rows + ROWS - 1) / ROWS, width = 3 * N3;
    const unsigned kBlocks = (unsigned)((N3 + THREADS - 1) / THREADS);
    const dim3 grid((unsigned)(chunks * kBlocks));  // below 2^31: chunks * kBlocks <= (rows / 128 + 1) * (N3 / 256 + 1)
    survey_args a = {p, pw, map, brainMask, classOf, rho, c, nMat, writeWater, rows, N3, kBlocks, rhoWater, cWater, dx2};
    if (idBytes == 1) hipLaunchKernelGGL(th_survey<1>, grid, dim3(THREADS), 0, 0, a, partial, pairs, flags);
    else if (idBytes == 2) hipLaunchKernelGGL(th_survey<2>, grid, dim3(THREADS), 0, 0, a, partial, pairs, flags);
    else hipLaunchKernelGGL(th_survey<4>, grid, dim3(THREADS), 0, 0, a, partial, pairs, flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the levels of the tree go to and fro between the two buffers until one row of sums is left: ceil(log32(chunks)) launches, at least one
    double *from = partial, *to = sums;
    int64_t count = chunks;
    do {
        const int64_t nodes = (count + FOLD - 1) / FOLD;
        for (int64_t g0 = 0; g0 < nodes; g0 += 65535) {      // gridDim.y is 65535 at the most
            const unsigned gy = (unsigned)std::min<int64_t>(65535, nodes - g0);
            hipLaunchKernelGGL(th_fold, dim3((unsigned)((width + THREADS - 1) / THREADS), gy), dim3(THREADS), 0, 0, (const double *)(from + g0 * FOLD * width),
                               count - g0 * FOLD, width, to + g0 * width);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        std::swap(from, to);
        count = nodes;
    } while (count > 1);
    *result = from;
    return hipSuccess;
}

extern "C" int bfd_loss_survey3d(int device, const float *p, const float *pw, int nFields, const void *map, int idBytes, int64_t N1, int64_t N2, int64_t N3,
                                 const uint8_t *classOf, int nMat, const uint8_t *brainMask, const double *rho, const double *c, double rhoWater, double cWater,
                                 double dx2, float *maxTissue, int64_t *argTissue, float *maxWater, int64_t *argWater, double *eWaterRaw, double *eWater,
                                 double *eTissue, float *waterOut, float *kernelMs)
{
    static const char *who = "bfd_loss_survey3d";
    // every argument error is reported before a device is looked for
    if (!p || !pw || !rho || !c || !maxTissue || !argTissue || !maxWater || !argWater || !eWaterRaw || !eWater || !eTissue)
        BFD_FAIL(-1, std::string(who) + ": null argument");
    if (const char *bad = check_common(map, idBytes, N1, N2, N3, classOf, nMat)) BFD_FAIL(-1, std::string(who) + bad);
    if (nFields < 1) BFD_FAIL(-1, std::string(who) + ": nFields must be at least 1");
    if (!positive_finite(rhoWater) || !positive_finite(cWater)) BFD_FAIL(-1, std::string(who) + ": rhoWater and cWater must be finite and positive");
    for (int q = 0; q < nMat; q++)
        if (!positive_finite(rho[q]) || !positive_finite(c[q])) BFD_FAIL(-1, std::string(who) + ": every rho and c must be finite and positive");
    if (!(dx2 >= 0.0) || dx2 - dx2 != 0.0) BFD_FAIL(-1, std::string(who) + ": dx2 must be finite and not negative");
    const size_t n = (size_t)(N1 * N2 * N3), F = (size_t)nFields;
    if (F > ((size_t)1 << 40) / std::max<size_t>(n, 1)) BFD_FAIL(-1, std::string(who) + ": nFields volumes hold 2^40 voxels or more");
    {
        const struct { const void *ptr; size_t b; } ins[7] = {{p, 4 * n * F}, {pw, 4 * n * F}, {map, n * (size_t)idBytes}, {classOf, (size_t)nMat},
                                                              {brainMask, brainMask ? n : 0}, {rho, 8 * (size_t)nMat}, {c, 8 * (size_t)nMat}};
        const struct { const void *ptr; size_t b; } outs[8] = {{maxTissue, 4 * F}, {argTissue, 8 * F}, {maxWater, 4 * F}, {argWater, 8 * F},
                                                               {eWaterRaw, 8 * F * (size_t)N3}, {eWater, 8 * F * (size_t)N3}, {eTissue, 8 * F * (size_t)N3},
                                                               {waterOut, waterOut ? 4 * n * F : 0}};
        for (int o = 0; o < 8; o++) {
            bool hit = false;
            if (!outs[o].b) continue;
            for (int i = 0; i < 7; i++) {
                if (!ins[i].b) continue;
                if (o == 7 && i == 1 && waterOut == pw) continue;         // the reference's in-place store
                hit = hit || overlap(ins[i].ptr, ins[i].b, outs[o].ptr, outs[o].b);
            }
            for (int o2 = 0; o2 < o; o2++) hit = hit || (outs[o2].b && overlap(outs[o2].ptr, outs[o2].b, outs[o].ptr, outs[o].b));
            if (hit) BFD_FAIL(-1, std::string(who) + ": an output may not alias an input or another output (waterOut may equal pw exactly)");
        }
    }

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    std::vector<double> sums(3 * F * (size_t)N3, 0.0);
    std::vector<unsigned long long> best(2 * F, TH_NO_PAIR);
    float total = 0.f;
    if (n) {
        const int64_t rows = N1 * N2, width = 3 * N3;
        size_t partialWords = 0, sumWords = 0;
        bfd_loss_survey_scratch(rows, N3, &partialWords, &sumWords);
        DevTemp<float> dp, dpw;                        // one tissue field; every water field where the cleared fields go back, else one
        DevTemp<uint8_t> dmap, dtab, dmask;
        DevTemp<double> drho, dc, dpartial, dsums;
        DevTemp<unsigned long long> dpairs;
        DevTemp<uint32_t> dflags;
        Events ev;
        BFD_STEP(dp.alloc(n));
        BFD_STEP(dpw.alloc(waterOut ? n * F : n));
        BFD_STEP(dmap.alloc(n * (size_t)idBytes));
        BFD_STEP(dtab.alloc((size_t)nMat));
        if (brainMask) BFD_STEP(dmask.alloc(n));
        BFD_STEP(drho.alloc((size_t)nMat));
        BFD_STEP(dc.alloc((size_t)nMat));
        BFD_STEP(dpartial.alloc(partialWords));
        BFD_STEP(dsums.alloc(sumWords));
        BFD_STEP(dpairs.alloc(2));
        BFD_STEP(dflags.alloc(1));
        BFD_STEP(hipMemcpy(dmap, map, n * (size_t)idBytes, hipMemcpyHostToDevice));
        BFD_STEP(hipMemcpy(dtab, classOf, (size_t)nMat, hipMemcpyHostToDevice));
        if (brainMask) BFD_STEP(hipMemcpy(dmask, brainMask, n, hipMemcpyHostToDevice));
        BFD_STEP(hipMemcpy(drho, rho, 8 * (size_t)nMat, hipMemcpyHostToDevice));
        BFD_STEP(hipMemcpy(dc, c, 8 * (size_t)nMat, hipMemcpyHostToDevice));
        BFD_STEP(hipMemset(dflags, 0, 4));
        BFD_STEP(ev.create());
        for (size_t f = 0; f < F; f++) {               // the fields are streamed through the same buffers
            float *w = dpw.p + (waterOut ? f * n : 0);
            float ms = 0.f;
            BFD_STEP(hipMemcpy(dp, p + f * n, 4 * n, hipMemcpyHostToDevice));
            BFD_STEP(hipMemcpy(w, pw + f * n, 4 * n, hipMemcpyHostToDevice));
            BFD_STEP(hipMemset(dpairs, 0, 16));
            const double *result = nullptr;
            BFD_STEP(ev.record(0));
            BFD_STEP(bfd_stage_loss_survey(dp.p, w, dmap.p, idBytes, brainMask ? dmask.p : nullptr, dtab.p, drho.p, dc.p, nMat, waterOut ? 1 : 0, rows, N3, rhoWater,
                                           cWater, dx2, dpartial.p, dsums.p, dpairs.p, dflags.p, &result));
            BFD_STEP(ev.record(1));
            BFD_STEP(ev.sync(1));
            BFD_STEP(ev.elapsed(&ms, 0, 1));
            total += ms;
            BFD_STEP(hipMemcpy(sums.data() + f * (size_t)width, result, 8 * (size_t)width, hipMemcpyDeviceToHost));
            BFD_STEP(hipMemcpy(best.data() + 2 * f, dpairs, 16, hipMemcpyDeviceToHost));
        }
        uint32_t flags = 0;
        BFD_STEP(hipMemcpy(&flags, dflags, 4, hipMemcpyDeviceToHost));
        if (flags & FLAG_ID) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "an id of the map is not below nMat");
        if (flags & FLAG_VALUE) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "a value is not finite");
        if (waterOut) BFD_STEP(hipMemcpy(waterOut, dpw, 4 * n * F, hipMemcpyDeviceToHost));
    }
    for (size_t f = 0; f < F; f++) {
        maxTissue[f] = best[2 * f] == TH_NO_PAIR ? 0.f : th_key_value(th_pair_key(best[2 * f]));
        argTissue[f] = th_pair_index(best[2 * f]);
        maxWater[f] = best[2 * f + 1] == TH_NO_PAIR ? 0.f : th_key_value(th_pair_key(best[2 * f + 1]));
        argWater[f] = th_pair_index(best[2 * f + 1]);
        for (int64_t k = 0; k < N3; k++) {
            eWaterRaw[f * (size_t)N3 + (size_t)k] = sums[f * 3 * (size_t)N3 + (size_t)k];
            eWater[f * (size_t)N3 + (size_t)k] = sums[f * 3 * (size_t)N3 + (size_t)N3 + (size_t)k];
            eTissue[f * (size_t)N3 + (size_t)k] = sums[f * 3 * (size_t)N3 + 2 * (size_t)N3 + (size_t)k];
        }
    }
    if (kernelMs) *kernelMs = total;
    return 0;
}
