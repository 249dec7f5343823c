// The domain setup between the mask file of Step 1 and the solver call of Step 2, on MI355X, in the caller's numpy C order (k fastest).
//
// Replace, in TranscranialModeling/BabelIntegrationBASE.py,
//     np.where(TempMaterialMap > 0), np.where(== 5), np.any(> 5) on the cropped and padded labels   :1163, :1903-1908, :2162   -> bfd_label_survey3d
//     the padded copies, the relabelling, the CT merge, the air mask and the water layer              :2111-2201                 -> bfd_assemble_material_map3d
//     the ray loop of the skull density ratio on the cropped CT index volume                          :816-854, :1384-1393       -> bfd_sdr_rays3d
// The driver flips the last axis of every volume it loads; the entries read the stored volume at M3 - 1 - k instead (flipK) and speak the driver's
// indices everywhere. The index arithmetic both sides share is in bfd_domain_core.h, which a plain C++ compiler accepts too.
//
// Survey: a wave per row of the whole volume, the row read as aligned 32-bit words (a row may begin and end inside a word). Counts go to a histogram
// in LDS, one atomic per word whose four voxels are equal and inside the box, zeros in a register; the six bounds and the first focal voxel stay in
// registers until the wave has taken its last row, then lanes -> wave -> workgroup and an integer atomic only where the bound in memory is not
// already as good. One 64-bit atomic per workgroup and bin.
// Assembly: one lane per output voxel, the 256-entry table in LDS, the statistics in registers until the end, then reduced the same way.
// Rays: a wave per ray, 64 voxels at a time. The rank of a skull voxel among those of its ray is the popcount of the ballot below its lane plus
// what the chunks before held. The first sweep gives the count and the maximum, the second the two positions and the minimum between them.
// 2048 workgroups stride over rows, voxels and rays. No kernel waits for another workgroup; every loop is bounded, see the comment at each.
#include <limits.h>
#include <math.h>
#include <cmath>
#include "bfd_internal.h"
#include "bfd_call.h"
#include "bfd_domain_core.h"
#include "bfd_domain_stages.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int64_t SWEEP_BLOCKS = 2048;            // what lies beyond is taken by a grid-stride loop
constexpr int HIST = 256;

// ---------------------------------------------------------------- survey ----------------------------------------------------------------

struct survey_args { int64_t rows; int M2, M3, lo0, hi0, lo1, hi1, lo2, hi2, flipK; };

// hist: 257 counters, zero before the launch; [256] counts the voxels equal to 5 in the whole volume. bnd: {min i, max i, min j, max j, min k, max k},
// box-relative, the minima INT_MAX and the maxima -1 before the launch. first: the smallest driver linear index of a 5, 0xFFFFFFFF before the launch.
// in: the volume, 4-byte aligned and padded to whole words.
__global__ __launch_bounds__(THREADS) void label_survey(const uint8_t *__restrict__ in, const survey_args a, unsigned long long *__restrict__ hist,
                                                        int *__restrict__ bnd, unsigned *__restrict__ first)
{
    __shared__ unsigned h[HIST + 1];
    for (int t = threadIdx.x; t <= HIST; t += THREADS) h[t] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t *words = (const uint32_t *)in;
    int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {-1, -1, -1};
    unsigned fmin = 0xFFFFFFFFu, zeros = 0;
    // grid-stride over rows, wave-uniform: ends after ceil(rows / (4 gridDim)) rounds
    for (int64_t row = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); row < a.rows; row += (int64_t)gridDim.x * WAVES) {
        const int i = (int)(row / a.M2), j = (int)(row % a.M2);
        const bool inIJ = i >= a.lo0 && i < a.hi0 && j >= a.lo1 && j < a.hi1;
        const int64_t start = row * a.M3, w0 = start >> 2;
        const int off = (int)(start & 3);                           // the row begins at byte `off` of word w0
        const int nW = (off + a.M3 + 3) >> 2;                       // words that hold a voxel of the row; the last lies inside the padded volume
        int kmn = INT_MAX, kmx = -1;
        for (int wi = lane; wi < nW; wi += 64) {                    // ends: wi grows
            const uint32_t w = words[w0 + wi];
            const int ks0 = 4 * wi - off;                           // the stored index of the word's byte 0 (may be negative: the row before)
            const int kdA = a.flipK ? a.M3 - 1 - ks0 : ks0, kdB = a.flipK ? kdA - 3 : kdA + 3;
            const int kLow = kdA < kdB ? kdA : kdB, kHigh = kdA < kdB ? kdB : kdA;
            const unsigned x0 = w & 0xFFu;
            if (ks0 >= 0 && ks0 + 3 < a.M3 && w == x0 * 0x01010101u && x0 != 5u && (!inIJ || (kLow >= a.lo2 && kHigh < a.hi2) || kHigh < a.lo2 || kLow >= a.hi2)) {
                // four equal voxels of this row, none the focal value, all inside the box or all outside it
                if (inIJ && kLow >= a.lo2 && kHigh < a.hi2) {
                    if (x0 == 0u) zeros += 4;
                    else {
                        atomicAdd(&h[x0], 4u);
                        kmn = kLow - a.lo2 < kmn ? kLow - a.lo2 : kmn;
                        kmx = kHigh - a.lo2 > kmx ? kHigh - a.lo2 : kmx;
                    }
                }
                continue;
            }
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int ks = ks0 + b;
                if (ks < 0 || ks >= a.M3) continue;
                const int kd = a.flipK ? a.M3 - 1 - ks : ks;
                const unsigned x = (w >> (8 * b)) & 0xFFu;
                if (x == 5u) {
                    atomicAdd(&h[HIST], 1u);
                    const unsigned lin = (unsigned)(start + kd);    // fewer than 2^31 voxels
                    fmin = lin < fmin ? lin : fmin;
                }
                if (inIJ && kd >= a.lo2 && kd < a.hi2) {
                    if (x == 0u) zeros++;
                    else {
                        atomicAdd(&h[x], 1u);
                        kmn = kd - a.lo2 < kmn ? kd - a.lo2 : kmn;
                        kmx = kd - a.lo2 > kmx ? kd - a.lo2 : kmx;
                    }
                }
            }
        }
        if (kmx >= 0) {                                             // this lane saw tissue of the row inside the box
            mn[0] = i - a.lo0 < mn[0] ? i - a.lo0 : mn[0]; mx[0] = i - a.lo0 > mx[0] ? i - a.lo0 : mx[0];
            mn[1] = j - a.lo1 < mn[1] ? j - a.lo1 : mn[1]; mx[1] = j - a.lo1 > mx[1] ? j - a.lo1 : mx[1];
            mn[2] = kmn < mn[2] ? kmn : mn[2];             mx[2] = kmx > mx[2] ? kmx : mx[2];
        }
    }
    // every wave arrives here: the loops above have no early exit from the kernel
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int l2 = __shfl_xor(mn[q], d), h2 = __shfl_xor(mx[q], d);
            mn[q] = l2 < mn[q] ? l2 : mn[q];
            mx[q] = h2 > mx[q] ? h2 : mx[q];
        }
        const unsigned f2 = __shfl_xor(fmin, d);
        fmin = f2 < fmin ? f2 : fmin;
        zeros += __shfl_xor(zeros, d);
    }
    // waves -> workgroup -> at most one atomic per bound, and none where the bound in memory is already as good: the bounds only ever move one way,
    // so a stale read can cost an atomic and never lose one (8192 waves on seven words took 0.5 ms at head size)
    __shared__ int red[6][WAVES];
    __shared__ unsigned redFirst[WAVES];
    if (lane == 0) {
        for (int q = 0; q < 3; q++) { red[2 * q][threadIdx.x >> 6] = mn[q]; red[2 * q + 1][threadIdx.x >> 6] = mx[q]; }
        redFirst[threadIdx.x >> 6] = fmin;
        if (zeros) atomicAdd(&h[0], zeros);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < WAVES; w++) {
            for (int q = 0; q < 3; q++) {
                mn[q] = red[2 * q][w] < mn[q] ? red[2 * q][w] : mn[q];
                mx[q] = red[2 * q + 1][w] > mx[q] ? red[2 * q + 1][w] : mx[q];
            }
            fmin = redFirst[w] < fmin ? redFirst[w] : fmin;
        }
        if (mx[0] >= 0)
            for (int q = 0; q < 3; q++) {
                if (mn[q] < __hip_atomic_load(bnd + 2 * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(bnd + 2 * q, mn[q]);
                if (mx[q] > __hip_atomic_load(bnd + 2 * q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(bnd + 2 * q + 1, mx[q]);
            }
        if (fmin < __hip_atomic_load(first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(first, fmin);
    }
    for (int t = threadIdx.x; t <= HIST; t += THREADS)
        if (h[t]) atomicAdd(hist + t, (unsigned long long)h[t]);
}

// ---------------------------------------------------------------- assembly ----------------------------------------------------------------

struct assemble_args {
    int64_t total;                                // voxels of the output
    int M2, M3, N2, N3;
    int lo[3], size[3], padLo[3];
    int flipK, focalI, focalJ;
    int64_t zWater;
    uint32_t ctOffset, nMaterials;
};

// acc64: {bone voxels, map > 0, map >= nMaterials}, zero before the launch. acc32: {min ct + ctOffset under bone (0xFFFFFFFF before the launch), max
// of it (0), max id of the map (0), the smallest k with map > 0 (0x7FFFFFFF), the same on the focal column (0x7FFFFFFF)}.
template <typename CT>
__global__ __launch_bounds__(THREADS) void assemble_map(const uint8_t *__restrict__ labels, const CT *__restrict__ ct, const uint8_t *__restrict__ air,
                                                        const uint32_t *__restrict__ lutG, const assemble_args a, uint32_t *__restrict__ map,
                                                        uint32_t *__restrict__ mapNoCT, uint32_t *__restrict__ airOut,
                                                        unsigned long long *__restrict__ acc64, unsigned *__restrict__ acc32)
{
    __shared__ uint32_t lut[HIST];
    for (int t = threadIdx.x; t < HIST; t += THREADS) lut[t] = lutG[t];
    __syncthreads();
    unsigned bone = 0, positive = 0, over = 0;
    unsigned ctMin = 0xFFFFFFFFu, ctMax = 0u, idMax = 0u, kMin = 0x7FFFFFFFu, kFocal = 0x7FFFFFFFu;
    // grid-stride over output voxels: ends after ceil(total / (THREADS gridDim)) rounds, at most 2^31 / THREADS: the 32-bit counts of a lane hold
    for (int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x; v < a.total; v += (int64_t)gridDim.x * THREADS) {
        const int k = (int)(v % a.N3);
        const int64_t row = v / a.N3;
        const int j = (int)(row % a.N2), i = (int)(row / a.N2);
        const int si = i - a.padLo[0], sj = j - a.padLo[1], sk = k - a.padLo[2];
        const bool inside = si >= 0 && si < a.size[0] && sj >= 0 && sj < a.size[1] && sk >= 0 && sk < a.size[2];
        uint32_t raw = 0, m = 0, ar = 0;
        if (inside) {
            // inside the source volume: the host checked 0 <= lo and lo + size <= M on every axis
            const int64_t src = ((int64_t)(a.lo[0] + si) * a.M2 + (a.lo[1] + sj)) * a.M3 + dm_source_k(a.lo[2] + sk, a.M3, a.flipK);
            raw = labels[src];
            const uint32_t e = lut[raw];
            if (e & DM_LUT_BONE) {                // never set where ct is null: the host refuses such a table
                m = (uint32_t)ct[src] + a.ctOffset;
                bone++;
                ctMin = m < ctMin ? m : ctMin;
                ctMax = m > ctMax ? m : ctMax;
            } else
                m = e;
            if (air) ar = air[src];
        }
        if (k <= a.zWater) m = 0;
        if (m) {
            positive++;
            idMax = m > idMax ? m : idMax;
            kMin = (unsigned)k < kMin ? (unsigned)k : kMin;
            if (i == a.focalI && j == a.focalJ) kFocal = (unsigned)k < kFocal ? (unsigned)k : kFocal;
        }
        if (m >= a.nMaterials) over++;
        map[v] = m;
        if (mapNoCT) mapNoCT[v] = raw;
        if (airOut) airOut[v] = ar;
    }
    // every lane arrives here: the loop above has no early exit from the kernel
    for (int d = 32; d >= 1; d >>= 1) {
        bone += __shfl_xor(bone, d);
        positive += __shfl_xor(positive, d);
        over += __shfl_xor(over, d);
        const unsigned c1 = __shfl_xor(ctMin, d), c2 = __shfl_xor(ctMax, d), c3 = __shfl_xor(idMax, d), c4 = __shfl_xor(kMin, d), c5 = __shfl_xor(kFocal, d);
        ctMin = c1 < ctMin ? c1 : ctMin;
        ctMax = c2 > ctMax ? c2 : ctMax;
        idMax = c3 > idMax ? c3 : idMax;
        kMin = c4 < kMin ? c4 : kMin;
        kFocal = c5 < kFocal ? c5 : kFocal;
    }
    // waves -> workgroup -> one atomic per count, and one per bound only where the bound in memory is not already as good (see label_survey)
    __shared__ unsigned part[8][WAVES];
    if ((threadIdx.x & 63) == 0) {
        const unsigned mine[8] = {bone, positive, over, ctMin, ctMax, idMax, kMin, kFocal};
        for (int q = 0; q < 8; q++) part[q][threadIdx.x >> 6] = mine[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < WAVES; w++) {
            bone += part[0][w]; positive += part[1][w]; over += part[2][w];
            ctMin = part[3][w] < ctMin ? part[3][w] : ctMin;
            ctMax = part[4][w] > ctMax ? part[4][w] : ctMax;
            idMax = part[5][w] > idMax ? part[5][w] : idMax;
            kMin = part[6][w] < kMin ? part[6][w] : kMin;
            kFocal = part[7][w] < kFocal ? part[7][w] : kFocal;
        }
        if (bone) atomicAdd(acc64, (unsigned long long)bone);
        if (positive) atomicAdd(acc64 + 1, (unsigned long long)positive);
        if (over) atomicAdd(acc64 + 2, (unsigned long long)over);
        if (ctMin < __hip_atomic_load(acc32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(acc32, ctMin);
        if (ctMax > __hip_atomic_load(acc32 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(acc32 + 1, ctMax);
        if (idMax > __hip_atomic_load(acc32 + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(acc32 + 2, idMax);
        if (kMin < __hip_atomic_load(acc32 + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(acc32 + 3, kMin);
        if (kFocal < __hip_atomic_load(acc32 + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(acc32 + 4, kFocal);
    }
}

// ---------------------------------------------------------------- rays ----------------------------------------------------------------

struct ray_args {
    int64_t rays;
    int cols, M2, M3, lo[3], size2, stepI, stepJ, flipK, minSkull;
    int64_t nHU;
    double centerRegion;
};

// the lanes below this one
static __device__ __forceinline__ unsigned long long lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

template <typename CT, typename T>
__global__ __launch_bounds__(THREADS) void sdr_rays(const CT *__restrict__ ct, const T *__restrict__ hu, const ray_args a, T *__restrict__ value,
                                                    int *__restrict__ count, uint8_t *__restrict__ state)
{
    const int lane = threadIdx.x & 63;
    // grid-stride over rays, wave-uniform: ends after ceil(rays / (4 gridDim)) rounds
    for (int64_t ray = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); ray < a.rays; ray += (int64_t)gridDim.x * WAVES) {
        const int r = (int)(ray / a.cols), c = (int)(ray % a.cols);
        // inside the volume: the host checked the box, and r * stepI < size[0], c * stepJ < size[1] by the lattice's size
        const int64_t base = ((int64_t)(a.lo[0] + r * a.stepI) * a.M2 + (a.lo[1] + c * a.stepJ)) * a.M3;
        // first sweep: the number of skull voxels, their maximum, an index beyond the table
        int n = 0;
        bool bad = false, haveMax = false;
        T huMax = 0;
        for (int p0 = 0; p0 < a.size2; p0 += 64) {                  // ends: p0 grows; the trip count is wave-uniform
            const int p = p0 + lane;
            int64_t idx = 0;
            if (p < a.size2) idx = (int64_t)ct[base + dm_source_k(a.lo[2] + p, a.M3, a.flipK)];
            if (idx >= a.nHU) bad = true;                           // counted as skull, never looked up
            else if (idx > 0) {
                const T x = hu[idx];
                huMax = haveMax ? (x > huMax ? x : huMax) : x;
                haveMax = true;
            }
            n += __popcll(__ballot(idx > 0));
        }
        bad = __any(bad);
        for (int d = 32; d >= 1; d >>= 1) {                         // the whole wave is here
            const T x = __shfl_xor(huMax, d);
            const bool hx = __shfl_xor((int)haveMax, d) != 0;
            if (hx) { huMax = haveMax ? (x > huMax ? x : huMax) : x; haveMax = true; }
        }
        int st = DM_RAY_COUNTED;
        T val = 0;
        if (bad) st = DM_RAY_BAD_INDEX;
        else if (n < a.minSkull) st = DM_RAY_FEW;
        else {
            int beg, end;
            dm_segment(n, a.centerRegion, &beg, &end);
            if (beg >= end) st = DM_RAY_EMPTY_CENTRE;
            else {
                // second sweep: the voxels from the skull voxel of rank beg up to, not including, the one of rank end
                int seen = 0;
                bool open = false, closed = false, have = false;
                T huMin = 0;
                for (int p0 = 0; p0 < a.size2 && !closed; p0 += 64) {          // ends: p0 grows; `closed` is wave-uniform
                    const int p = p0 + lane;
                    int64_t idx = 0;
                    if (p < a.size2) idx = (int64_t)ct[base + dm_source_k(a.lo[2] + p, a.M3, a.flipK)];
                    const unsigned long long skull = __ballot(idx > 0);
                    const int rank = seen + __popcll(skull & lanes_below(lane));
                    const unsigned long long atBeg = __ballot(idx > 0 && rank == beg), atEnd = __ballot(idx > 0 && rank == end);
                    const int from = open ? 0 : (atBeg ? __ffsll((long long)atBeg) - 1 : 64);
                    const int to = atEnd ? __ffsll((long long)atEnd) - 1 : 64;
                    if (p < a.size2 && lane >= from && lane < to) {
                        const T x = hu[idx];
                        huMin = have ? (x < huMin ? x : huMin) : x;
                        have = true;
                    }
                    open = open || atBeg != 0;
                    closed = atEnd != 0;
                    seen += __popcll(skull);
                }
                for (int d = 32; d >= 1; d >>= 1) {
                    const T x = __shfl_xor(huMin, d);
                    const bool hx = __shfl_xor((int)have, d) != 0;
                    if (hx) { huMin = have ? (x < huMin ? x : huMin) : x; have = true; }
                }
                if (!(huMax > (T)0)) st = DM_RAY_NOT_POSITIVE;
                else val = huMin / huMax;
            }
        }
        if (lane == 0) { value[ray] = val; count[ray] = n; state[ray] = (uint8_t)st; }
    }
}

static bool box_inside(const int64_t *lo, const int64_t *size, const int64_t *M)
{
    for (int q = 0; q < 3; q++)
        if (lo[q] < 0 || size[q] < 0 || lo[q] > M[q] || size[q] > M[q] - lo[q]) return false;
    return true;
}

}  // namespace

// ---------------------------------------------------------------- the stages (bfd_domain_stages.h) ----------------------------------------------------------------

hipError_t bfd_stage_label_survey(const uint8_t *dLabels, int64_t M1, int64_t M2, int64_t M3, const int64_t *lo, const int64_t *hi, int flipK,
                                  unsigned long long *dHist, int *dBnd, unsigned *dFirst)
{
    survey_args a;
    a.rows = M1 * M2; a.M2 = (int)M2; a.M3 = (int)M3;
    a.lo0 = (int)lo[0]; a.hi0 = (int)hi[0]; a.lo1 = (int)lo[1]; a.hi1 = (int)hi[1]; a.lo2 = (int)lo[2]; a.hi2 = (int)hi[2];
    a.flipK = flipK;
    hipLaunchKernelGGL(label_survey, dim3(blocks_for(a.rows, WAVES, SWEEP_BLOCKS)), dim3(THREADS), 0, 0, dLabels, a, dHist, dBnd, dFirst);
    return hipGetLastError();
}

void bfd_label_survey_finish(const unsigned long long *h, const int *bnd, unsigned first, int64_t *hist, int64_t *bounds, int64_t *focal)
{
    for (int q = 0; q < HIST; q++) hist[q] = (int64_t)h[q];
    for (int q = 0; q < 6; q++) bounds[q] = bnd[1] < 0 ? -1 : bnd[q];
    focal[0] = (int64_t)h[HIST];
    focal[1] = first == 0xFFFFFFFFu ? -1 : (int64_t)first;
}

hipError_t bfd_stage_assemble_map(const uint8_t *dLabels, const void *dCt, int ctBytes, const uint8_t *dAir, int64_t M2, int64_t M3, const int64_t *N,
                                  const int64_t *lo, const int64_t *size, const int64_t *padLo, int flipK, const uint32_t *dLut, uint32_t ctOffset, int64_t zWater,
                                  int64_t nMaterials, const int64_t *focalIJ, uint32_t *dMap, uint32_t *dMapNoCT, uint32_t *dAirOut, unsigned long long *d64,
                                  unsigned *d32)
{
    assemble_args a;
    a.total = N[0] * N[1] * N[2];
    a.M2 = (int)M2; a.M3 = (int)M3; a.N2 = (int)N[1]; a.N3 = (int)N[2];
    for (int q = 0; q < 3; q++) { a.lo[q] = (int)lo[q]; a.size[q] = (int)size[q]; a.padLo[q] = (int)padLo[q]; }
    a.flipK = flipK; a.focalI = (int)focalIJ[0]; a.focalJ = (int)focalIJ[1];
    a.zWater = zWater; a.ctOffset = ctOffset; a.nMaterials = (uint32_t)nMaterials;
    const unsigned blocks = blocks_for(a.total, THREADS, SWEEP_BLOCKS);
    if (ctBytes == 2)
        hipLaunchKernelGGL(assemble_map<uint16_t>, dim3(blocks), dim3(THREADS), 0, 0, dLabels, (const uint16_t *)dCt, dAir, dLut, a, dMap, dMapNoCT, dAirOut, d64, d32);
    else
        hipLaunchKernelGGL(assemble_map<uint32_t>, dim3(blocks), dim3(THREADS), 0, 0, dLabels, (const uint32_t *)dCt, dAir, dLut, a, dMap, dMapNoCT, dAirOut, d64, d32);
    return hipGetLastError();
}

void bfd_assemble_finish(const unsigned long long *c64, const unsigned *c32, int64_t *stats)
{
    stats[0] = (int64_t)c64[0];
    stats[1] = c64[0] ? (int64_t)c32[0] : -1;
    stats[2] = c64[0] ? (int64_t)c32[1] : -1;
    stats[3] = (int64_t)c64[1];
    stats[4] = (int64_t)c32[2];
    stats[5] = c64[1] ? (int64_t)c32[3] : -1;
    stats[6] = c32[4] == 0x7FFFFFFFu ? -1 : (int64_t)c32[4];
    stats[7] = (int64_t)c64[2];
}

int bfd_survey_arguments(const char *who, int64_t M1, int64_t M2, int64_t M3, const int64_t *lo, const int64_t *hi, int flipK)
{
    if (M1 < 0 || M2 < 0 || M3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (!volume_fits(M1, M2, M3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    const int64_t M[3] = {M1, M2, M3};
    for (int q = 0; q < 3; q++)
        if (lo[q] < 0 || lo[q] > hi[q] || hi[q] > M[q]) BFD_FAIL(-1, std::string(who) + ": the box must satisfy 0 <= lo <= hi <= M on every axis");
    if (flipK != 0 && flipK != 1) BFD_FAIL(-1, std::string(who) + ": flipK must be 0 or 1");
    return 0;
}

int bfd_assemble_arguments(const char *who, int64_t M1, int64_t M2, int64_t M3, bool haveCt, const int64_t *lo, const int64_t *size, const int64_t *padLo,
                           const int64_t *padHi, int flipK, const uint32_t *lut, int64_t zWater, int64_t nMaterials, const int64_t *focalIJ, int64_t *N)
{
    const int64_t M[3] = {M1, M2, M3};
    if (!box_inside(lo, size, M)) BFD_FAIL(-1, std::string(who) + ": the box must satisfy 0 <= lo and lo + size <= M on every axis");
    const int64_t LIMIT = (int64_t)1 << 31;
    for (int q = 0; q < 3; q++) {
        if (padLo[q] < 0 || padHi[q] < 0 || padLo[q] >= LIMIT || padHi[q] >= LIMIT) BFD_FAIL(-1, std::string(who) + ": the padding must be 0 .. 2^31 - 1");
        N[q] = size[q] + padLo[q] + padHi[q];
    }
    if (!volume_fits(N[0], N[1], N[2])) BFD_FAIL(-1, std::string(who) + ": the map has 2^31 voxels or more (limit: fewer than 2^31)");
    if (flipK != 0 && flipK != 1) BFD_FAIL(-1, std::string(who) + ": flipK must be 0 or 1");
    if (!haveCt)
        for (int q = 0; q < HIST; q++)
            if (lut[q] & DM_LUT_BONE) BFD_FAIL(-1, std::string(who) + ": the lut marks a label as bone and there is no ct");
    if (zWater < -1) BFD_FAIL(-1, std::string(who) + ": zWater must be -1 or a plane index");
    if (nMaterials < 0 || nMaterials > 0xFFFFFFFFll) BFD_FAIL(-1, std::string(who) + ": nMaterials must be 0 .. 2^32 - 1");
    if (N[0] * N[1] * N[2] && (focalIJ[0] < 0 || focalIJ[0] >= N[0] || focalIJ[1] < 0 || focalIJ[1] >= N[1]))
        BFD_FAIL(-1, std::string(who) + ": focalIJ must be a column of the map");
    return 0;
}

extern "C" int bfd_label_survey3d(int device, const uint8_t *labels, int64_t M1, int64_t M2, int64_t M3, const int64_t *lo, const int64_t *hi, int flipK,
                                  int64_t *hist, int64_t *bounds, int64_t *focal, float *kernelMs)
{
    static const char *who = "bfd_label_survey3d";
    // every argument error is reported before a device is looked for
    if (!labels || !lo || !hi || !hist || !bounds || !focal) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (int rc = bfd_survey_arguments(who, M1, M2, M3, lo, hi, flipK)) return rc;

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    const size_t n = (size_t)(M1 * M2 * M3);
    if (n == 0) {
        for (int q = 0; q < HIST; q++) hist[q] = 0;
        for (int q = 0; q < 6; q++) bounds[q] = -1;
        focal[0] = 0; focal[1] = -1;
        return 0;
    }

    const size_t np = (n + 3) / 4 * 4;                // whole words: a row's last word may reach past the volume's last voxel
    DevTemp<uint8_t> din;
    DevTemp<unsigned long long> dhist;
    DevTemp<int> dbnd;
    DevTemp<unsigned> dfirst;
    Events ev;
    unsigned long long h[HIST + 1];
    int bnd[6] = {INT_MAX, -1, INT_MAX, -1, INT_MAX, -1};
    unsigned first = 0xFFFFFFFFu;
    BFD_STEP(din.alloc(np));
    BFD_STEP(dhist.alloc(HIST + 1));
    BFD_STEP(dbnd.alloc(6));
    BFD_STEP(dfirst.alloc(1));
    BFD_STEP(hipMemset(dhist, 0, sizeof h));
    if (np > n) BFD_STEP(hipMemset(din.p + (np - 4), 0, 4));
    BFD_STEP(hipMemcpy(din, labels, n, hipMemcpyHostToDevice));
    BFD_STEP(hipMemcpy(dbnd, bnd, sizeof bnd, hipMemcpyHostToDevice));
    BFD_STEP(hipMemcpy(dfirst, &first, sizeof first, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    BFD_STEP(bfd_stage_label_survey(din, M1, M2, M3, lo, hi, flipK, dhist, dbnd, dfirst));
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    BFD_STEP(hipMemcpy(h, dhist, sizeof h, hipMemcpyDeviceToHost));
    BFD_STEP(hipMemcpy(bnd, dbnd, sizeof bnd, hipMemcpyDeviceToHost));
    BFD_STEP(hipMemcpy(&first, dfirst, sizeof first, hipMemcpyDeviceToHost));
    bfd_label_survey_finish(h, bnd, first, hist, bounds, focal);
    return 0;
}

extern "C" int bfd_assemble_material_map3d(int device, const uint8_t *labels, const void *ct, int ctBytes, const uint8_t *air, int64_t M1, int64_t M2, int64_t M3,
                                           const int64_t *lo, const int64_t *size, const int64_t *padLo, const int64_t *padHi, int flipK, const uint32_t *lut,
                                           uint32_t ctOffset, int64_t zWater, int64_t nMaterials, const int64_t *focalIJ, uint32_t *map, uint32_t *mapNoCT,
                                           uint32_t *airOut, int64_t *stats, float *kernelMs)
{
    static const char *who = "bfd_assemble_material_map3d";
    // every argument error is reported before a device is looked for
    if (!labels || !lo || !size || !padLo || !padHi || !lut || !focalIJ || !map || !stats) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (M1 < 0 || M2 < 0 || M3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (!volume_fits(M1, M2, M3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    if ((ctBytes != 0 && ctBytes != 2 && ctBytes != 4) || (ctBytes == 0) != (ct == nullptr))
        BFD_FAIL(-1, std::string(who) + ": ctBytes must be 0 with a null ct, or 2 or 4 with a ct");
    int64_t N[3];
    if (int rc = bfd_assemble_arguments(who, M1, M2, M3, ct != nullptr, lo, size, padLo, padHi, flipK, lut, zWater, nMaterials, focalIJ, N)) return rc;
    const size_t n = (size_t)(M1 * M2 * M3), nOut = (size_t)(N[0] * N[1] * N[2]);
    if (nOut) {
        const void *outs[3] = {map, mapNoCT, airOut};
        const void *ins[3] = {labels, ct, air};
        const size_t inBytes[3] = {n, n * (size_t)ctBytes, n};
        for (int p = 0; p < 3; p++) {
            if (!outs[p]) continue;
            for (int q = 0; q < 3; q++)
                if ((ins[q] && inBytes[q] && overlap(outs[p], 4 * nOut, ins[q], inBytes[q])) || (q > p && outs[q] && overlap(outs[p], 4 * nOut, outs[q], 4 * nOut)))
                    BFD_FAIL(-1, std::string(who) + ": an output may not alias an input or another output");
        }
    }

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (nOut == 0) {
        stats[0] = 0; stats[1] = stats[2] = -1; stats[3] = stats[4] = 0; stats[5] = stats[6] = -1; stats[7] = 0;
        return 0;
    }

    DevTemp<uint8_t> dlab, dct, dair;
    DevTemp<uint32_t> dlut, dmap, dno, dairOut;
    DevTemp<unsigned long long> d64;
    DevTemp<unsigned> d32;
    Events ev;
    unsigned long long c64[3] = {0, 0, 0};
    unsigned c32[5] = {0xFFFFFFFFu, 0u, 0u, 0x7FFFFFFFu, 0x7FFFFFFFu};
    BFD_STEP(dlab.alloc(std::max<size_t>(n, 1)));
    if (ct) BFD_STEP(dct.alloc(std::max<size_t>(n * (size_t)ctBytes, 1)));
    if (air) BFD_STEP(dair.alloc(std::max<size_t>(n, 1)));
    BFD_STEP(dlut.alloc(HIST));
    BFD_STEP(dmap.alloc(nOut));
    if (mapNoCT) BFD_STEP(dno.alloc(nOut));
    if (airOut) BFD_STEP(dairOut.alloc(nOut));
    BFD_STEP(d64.alloc(3));
    BFD_STEP(d32.alloc(5));
    if (n) {
        BFD_STEP(hipMemcpy(dlab, labels, n, hipMemcpyHostToDevice));
        if (ct) BFD_STEP(hipMemcpy(dct, ct, n * (size_t)ctBytes, hipMemcpyHostToDevice));
        if (air) BFD_STEP(hipMemcpy(dair, air, n, hipMemcpyHostToDevice));
    }
    BFD_STEP(hipMemcpy(dlut, lut, HIST * sizeof(uint32_t), hipMemcpyHostToDevice));
    BFD_STEP(hipMemcpy(d64, c64, sizeof c64, hipMemcpyHostToDevice));
    BFD_STEP(hipMemcpy(d32, c32, sizeof c32, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    BFD_STEP(bfd_stage_assemble_map(dlab, dct, ctBytes, dair, M2, M3, N, lo, size, padLo, flipK, dlut, ctOffset, zWater, nMaterials, focalIJ, dmap, dno, dairOut,
                                    d64, d32));
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    BFD_STEP(hipMemcpy(c64, d64, sizeof c64, hipMemcpyDeviceToHost));
    BFD_STEP(hipMemcpy(c32, d32, sizeof c32, hipMemcpyDeviceToHost));
    BFD_STEP(hipMemcpy(map, dmap, 4 * nOut, hipMemcpyDeviceToHost));
    if (mapNoCT) BFD_STEP(hipMemcpy(mapNoCT, dno, 4 * nOut, hipMemcpyDeviceToHost));
    if (airOut) BFD_STEP(hipMemcpy(airOut, dairOut, 4 * nOut, hipMemcpyDeviceToHost));
    bfd_assemble_finish(c64, c32, stats);
    return 0;
}

extern "C" int bfd_sdr_rays3d(int device, const void *ct, int ctBytes, int64_t M1, int64_t M2, int64_t M3, const int64_t *lo, const int64_t *size, int flipK,
                              const void *hu, int huBytes, int64_t nHU, int64_t stepI, int64_t stepJ, int64_t minSkullVoxels, double centerRegion, void *value,
                              int32_t *count, uint8_t *state, float *kernelMs)
{
    static const char *who = "bfd_sdr_rays3d";
    // every argument error is reported before a device is looked for
    if (!ct || !lo || !size || !hu || !value || !count || !state) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (M1 < 0 || M2 < 0 || M3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (!volume_fits(M1, M2, M3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    if (ctBytes != 2 && ctBytes != 4) BFD_FAIL(-1, std::string(who) + ": ctBytes must be 2 or 4");
    const int64_t M[3] = {M1, M2, M3};
    if (!box_inside(lo, size, M)) BFD_FAIL(-1, std::string(who) + ": the box must satisfy 0 <= lo and lo + size <= M on every axis");
    if (flipK != 0 && flipK != 1) BFD_FAIL(-1, std::string(who) + ": flipK must be 0 or 1");
    if (huBytes != 4 && huBytes != 8) BFD_FAIL(-1, std::string(who) + ": huBytes must be 4 or 8");
    if (nHU < 1 || nHU >= ((int64_t)1 << 31)) BFD_FAIL(-1, std::string(who) + ": nHU must be 1 .. 2^31 - 1");
    for (int64_t q = 0; q < nHU; q++)
        if (!std::isfinite(huBytes == 4 ? (double)((const float *)hu)[q] : ((const double *)hu)[q])) BFD_FAIL(-1, std::string(who) + ": every hu must be finite");
    if (stepI < 1 || stepJ < 1 || stepI >= ((int64_t)1 << 31) || stepJ >= ((int64_t)1 << 31)) BFD_FAIL(-1, std::string(who) + ": stepI and stepJ must be 1 .. 2^31 - 1");
    if (minSkullVoxels < 1 || minSkullVoxels >= ((int64_t)1 << 31)) BFD_FAIL(-1, std::string(who) + ": minSkullVoxels must be 1 .. 2^31 - 1");
    if (!(centerRegion >= 0.0) || !std::isfinite(centerRegion)) BFD_FAIL(-1, std::string(who) + ": centerRegion must be finite and not negative");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    const int64_t rowsR = (size[0] + stepI - 1) / stepI, colsR = (size[1] + stepJ - 1) / stepJ, rays = rowsR * colsR;
    if (rays == 0) return 0;

    const size_t n = (size_t)(M1 * M2 * M3);              // not 0: the box holds a ray
    ray_args a;
    a.rays = rays; a.cols = (int)colsR; a.M2 = (int)M2; a.M3 = (int)M3;
    for (int q = 0; q < 3; q++) a.lo[q] = (int)lo[q];
    a.size2 = (int)size[2]; a.stepI = (int)stepI; a.stepJ = (int)stepJ; a.flipK = flipK; a.minSkull = (int)minSkullVoxels;
    a.nHU = nHU; a.centerRegion = centerRegion;
    DevTemp<uint8_t> dct, dhu, dval, dstate;
    DevTemp<int> dcount;
    Events ev;
    BFD_STEP(dct.alloc(n * (size_t)ctBytes));
    BFD_STEP(dhu.alloc((size_t)nHU * (size_t)huBytes));
    BFD_STEP(dval.alloc((size_t)rays * (size_t)huBytes));
    BFD_STEP(dcount.alloc((size_t)rays));
    BFD_STEP(dstate.alloc((size_t)rays));
    BFD_STEP(hipMemcpy(dct, ct, n * (size_t)ctBytes, hipMemcpyHostToDevice));
    BFD_STEP(hipMemcpy(dhu, hu, (size_t)nHU * (size_t)huBytes, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    const dim3 grid(blocks_for(rays, WAVES, SWEEP_BLOCKS)), block(THREADS);
    BFD_STEP(ev.record(0));
    if (ctBytes == 2 && huBytes == 4)
        hipLaunchKernelGGL((sdr_rays<uint16_t, float>), grid, block, 0, 0, (const uint16_t *)dct.p, (const float *)dhu.p, a, (float *)dval.p, dcount.p, dstate.p);
    else if (ctBytes == 2)
        hipLaunchKernelGGL((sdr_rays<uint16_t, double>), grid, block, 0, 0, (const uint16_t *)dct.p, (const double *)dhu.p, a, (double *)dval.p, dcount.p, dstate.p);
    else if (huBytes == 4)
        hipLaunchKernelGGL((sdr_rays<uint32_t, float>), grid, block, 0, 0, (const uint32_t *)dct.p, (const float *)dhu.p, a, (float *)dval.p, dcount.p, dstate.p);
    else
        hipLaunchKernelGGL((sdr_rays<uint32_t, double>), grid, block, 0, 0, (const uint32_t *)dct.p, (const double *)dhu.p, a, (double *)dval.p, dcount.p, dstate.p);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    BFD_STEP(hipMemcpy(value, dval, (size_t)rays * (size_t)huBytes, hipMemcpyDeviceToHost));
    BFD_STEP(hipMemcpy(count, dcount, (size_t)rays * sizeof(int), hipMemcpyDeviceToHost));
    BFD_STEP(hipMemcpy(state, dstate, (size_t)rays, hipMemcpyDeviceToHost));
    return 0;
}
