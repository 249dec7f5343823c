// The bone-rim partial-volume correction of the CT on MI355X as one call, in the caller's numpy C order (k fastest).
//
// Replaces, in BabelBrain/BabelDatasetPreps.py (bMaximizeBoneRim, :935-1017), everything between the odd box of :942-946 and the store of :1010:
//     the clamp of the bone voxels                                  :931-933 (optional: `floor`)
//     interior_mask_val, binary_erosion, the global mean            :948-957
//     distance_transform_edt(1 - interior_mask)                     :964-967
//     edge_voxels, the weights                                      :970-976
//     interior_f, the two gaussian_filter calls, the local mean     :980-991
//     the blend, the clip and the store                             :994-1010
// The CT and the bone mask go up once, every intermediate stays on the device and the corrected CT comes down once. The erosion, the distance
// transform and the filter are the launch sequences of bfd_binary_morphology3d, bfd_distance_transform_edt3d and bfd_gaussian_filter3d themselves
// (bfd_step1_stages.h); the eroded words are the distance transform's background words as they stand, and the float64 distances never exist.
// The arithmetic per voxel is in bfd_bonerim_core.h, which a plain C++ compiler accepts too.
//
// Every kernel here takes one wave per 64-bit word of the packed masks, lane l at voxel 64 w + l of the row: a wave's loads and stores are one
// contiguous segment and the words of the masks are wave-uniform loads.
//   prepare   reads ct and bone once: the floor, the checks (finite; a dense value below 2^17), f = ct * dense and the float32 dense mask, the bone
//             mask as packed words (one ballot), the counts and the integer sum of the dense values x 2^14
//   count     the interior voxels: population count of the eroded words
//   edge      the largest squared distance over the edge voxels (bone and not interior) and their number; d2 is read at edge voxels alone.
//             Writes the interior as bytes where the caller asked for it
//   blend     at edge voxels alone: ct, d2, bi, bm, the weight from the table, bfd_bonerim_core.h's operations one at a time, the store, and the
//             last three statistics
// A lane keeps its counts in registers over its whole grid-stride loop; they are reduced lanes -> wave -> workgroup and end in one integer atomic
// per workgroup and count: integers, so every run gives the same. No kernel waits for another workgroup; every loop is bounded, see the comment at each.
// The weight table is formed on the HOST between the second and the third timed section (rim_weight_table): exp as numpy takes it on the CPU at
// hand, which is what makes the weights the reference's bit for bit.
#include <float.h>
#include <string.h>
#include "bfd_internal.h"
#include "bfd_call.h"
#include "bfd_bonerim_core.h"
#include "bfd_step1_stages.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int64_t RIM_BLOCKS = 2048;              // one sweep: 8192 words = 524288 voxels; what lies beyond is taken by the grid-stride loops
const char *const DATA_REFUSED = ": refused data: ";
constexpr int MAX_BOX = 31;

// the accumulators of a call, 64-bit words on the device
enum { ACC_BONE = 0, ACC_DENSE, ACC_SUM, ACC_BAD, ACC_INTERIOR, ACC_EDGE, ACC_MAXD2, ACC_GLOBAL, ACC_CLIPPED, ACC_CHANGED, ACC_COUNT };
constexpr unsigned BAD_NOT_FINITE = 1u, BAD_TOO_LARGE = 2u;

// The sum (MAX: the largest) of v over the workgroup, in every thread: lanes -> wave -> workgroup. The whole workgroup calls this together, after
// its loop. One atomic per workgroup and count follows: with one per wave, the 8192 waves of a sweep on the same few words took longer than the
// passes' bytes (the preparation pass at 448 x 448 x 384 went from 0.459 to 0.243 ms; profiles/README.md, "Bone rim").
template <bool MAX>
static __device__ __forceinline__ unsigned long long block_reduce(unsigned long long v)
{
    __shared__ unsigned long long part[WAVES];
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = MAX ? (o > v ? o : v) : v + o;
    }
    __syncthreads();                                  // the call before this one has read part
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    v = part[0];
    for (int w = 1; w < WAVES; w++) v = MAX ? (part[w] > v ? part[w] : v) : v + part[w];
    return v;
}

// ct is written where the floor raises it; f, m: float32 volumes; bits: rows * W words
__global__ __launch_bounds__(THREADS) void rim_prepare(float *__restrict__ ct, const uint8_t *__restrict__ bone, float *__restrict__ f, float *__restrict__ m,
                                                       uint64_t *__restrict__ bits, int64_t rows, int64_t N3, int64_t W, float threshold, int haveFloor,
                                                       float floorValue, unsigned long long *__restrict__ acc)
{
    const int lane = threadIdx.x & 63;
    const int64_t words = rows * W;
    unsigned long long nBone = 0, nDense = 0, sum = 0;            // this lane's
    unsigned bad = 0;
    // grid-stride over words, the same trip count for every lane of a wave (the word index is wave-uniform): ends
    for (int64_t item = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); item < words; item += (int64_t)gridDim.x * WAVES) {
        const int64_t row = item / W, k = (item - row * W) * 64 + lane;
        bool isBone = false;
        if (k < N3) {
            const int64_t v = row * N3 + k;
            isBone = bone[v] != 0;
            const float x = ct[v];
            const float y = rim_floor(x, isBone, haveFloor != 0, floorValue);
            if (y != x) ct[v] = y;
            if (!(fabsf(y) <= FLT_MAX)) bad |= BAD_NOT_FINITE;
            const bool dense = rim_dense(y, threshold);
            f[v] = rim_dense_product(y, dense);
            m[v] = dense ? 1.0f : 0.0f;
            if (dense) {
                nDense++;
                if (y < RIM_VALUE_LIMIT) sum += rim_fixed(y);
                else bad |= BAD_TOO_LARGE;
            }
        }
        const unsigned long long word = __ballot(isBone);
        if (lane == 0) { bits[item] = word; nBone += (unsigned long long)__popcll(word); }
    }
    // every thread arrives here: the loop above has no early exit from the kernel
    nBone = block_reduce<false>(nBone);
    nDense = block_reduce<false>(nDense);
    sum = block_reduce<false>(sum);
    const unsigned long long notFinite = block_reduce<false>(bad & BAD_NOT_FINITE ? 1 : 0), tooLarge = block_reduce<false>(bad & BAD_TOO_LARGE ? 1 : 0);
    if (threadIdx.x == 0) {
        if (nBone) atomicAdd(acc + ACC_BONE, nBone);
        if (nDense) { atomicAdd(acc + ACC_DENSE, nDense); atomicAdd(acc + ACC_SUM, sum); }
        if (notFinite || tooLarge) atomicOr(acc + ACC_BAD, (unsigned long long)((notFinite ? BAD_NOT_FINITE : 0u) | (tooLarge ? BAD_TOO_LARGE : 0u)));
    }
}

// the set bits of nWords words (padding bits 0)
__global__ __launch_bounds__(THREADS) void rim_count(const uint64_t *__restrict__ bits, int64_t nWords, unsigned long long *__restrict__ count)
{
    unsigned long long c = 0;
    for (int64_t w = (int64_t)blockIdx.x * THREADS + threadIdx.x; w < nWords; w += (int64_t)gridDim.x * THREADS) c += (unsigned long long)__popcll(bits[w]);   // grid-stride: ends
    c = block_reduce<false>(c);                       // every thread arrives here
    if (threadIdx.x == 0 && c) atomicAdd(count, c);
}

// interiorOut: null, or the interior as bytes
__global__ __launch_bounds__(THREADS) void rim_edge(const uint64_t *__restrict__ boneBits, const uint64_t *__restrict__ interiorBits, const int32_t *__restrict__ d2,
                                                    uint8_t *__restrict__ interiorOut, int64_t rows, int64_t N3, int64_t W, unsigned long long *__restrict__ acc)
{
    const int lane = threadIdx.x & 63;
    const int64_t words = rows * W;
    unsigned long long nEdge = 0, top = 0;            // nEdge: lane 0 counts for its wave
    for (int64_t item = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); item < words; item += (int64_t)gridDim.x * WAVES) {       // as in rim_prepare: ends
        const int64_t row = item / W, k = (item - row * W) * 64 + lane;
        const uint64_t in = interiorBits[item], edge = boneBits[item] & ~in;
        if (interiorOut && k < N3) interiorOut[row * N3 + k] = (uint8_t)((in >> lane) & 1u);
        if (!edge) continue;                          // wave-uniform
        if (lane == 0) nEdge += (unsigned long long)__popcll(edge);
        if ((edge >> lane) & 1u) {                    // an edge bit is a bone voxel: k < N3
            const unsigned long long d = (unsigned long long)d2[row * N3 + k];       // a squared distance: not negative
            top = d > top ? d : top;
        }
    }
    nEdge = block_reduce<false>(nEdge);               // every thread arrives here: `continue` is no exit from the kernel
    top = block_reduce<true>(top);
    if (threadIdx.x == 0 && nEdge) { atomicAdd(acc + ACC_EDGE, nEdge); atomicMax(acc + ACC_MAXD2, top); }
}

__global__ __launch_bounds__(THREADS) void rim_blend_pass(float *__restrict__ ct, const uint64_t *__restrict__ boneBits, const uint64_t *__restrict__ interiorBits,
                                                          const int32_t *__restrict__ d2, const float *__restrict__ bi, const float *__restrict__ bm,
                                                          const double *__restrict__ table, int64_t tableLength, float gmean, double maxBoost, int64_t rows,
                                                          int64_t N3, int64_t W, unsigned long long *__restrict__ acc)
{
    const int lane = threadIdx.x & 63;
    const int64_t words = rows * W;
    unsigned long long nGlobal = 0, nClipped = 0, nChanged = 0;   // this lane's
    for (int64_t item = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); item < words; item += (int64_t)gridDim.x * WAVES) {       // as in rim_prepare: ends
        const uint64_t edge = boneBits[item] & ~interiorBits[item];
        if (!edge) continue;                          // wave-uniform
        bool global = false, clipped = false, changed = false;
        if ((edge >> lane) & 1u) {
            const int64_t row = item / W, v = row * N3 + (item - row * W) * 64 + lane;
            const float o = ct[v];
            const float lm = rim_local_mean(bi[v], bm[v], gmean, &global);
            const float r = rim_blend(o, lm, rim_weight(table, tableLength, d2[v]), maxBoost, &clipped);
            changed = __float_as_uint(r) != __float_as_uint(o);
            if (changed) ct[v] = r;
        }
        nGlobal += global ? 1 : 0;
        nClipped += clipped ? 1 : 0;
        nChanged += changed ? 1 : 0;
    }
    nGlobal = block_reduce<false>(nGlobal);           // every thread arrives here
    nClipped = block_reduce<false>(nClipped);
    nChanged = block_reduce<false>(nChanged);
    if (threadIdx.x == 0) {
        if (nGlobal) atomicAdd(acc + ACC_GLOBAL, nGlobal);
        if (nClipped) atomicAdd(acc + ACC_CLIPPED, nClipped);
        if (nChanged) atomicAdd(acc + ACC_CHANGED, nChanged);
    }
}

}  // namespace

extern "C" int bfd_bone_rim_correct3d(int device, const float *ct, const uint8_t *bone, float *out, int64_t N1, int64_t N2, int64_t N3, const int32_t *box,
                                      float interiorThreshold, double maxBoost, double distanceScale, double sigma, const float *floorValue, float *globalMean,
                                      int globalMeanGiven, int64_t *stats, uint8_t *interior, int32_t *d2, float *bi, float *bm, float *kernelMs)
{
    static const char *who = "bfd_bone_rim_correct3d";
    // every argument error is reported before a device is looked for
    if (!ct || !bone || !out || !box || !globalMean || !stats) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (N1 < 0 || N2 < 0 || N3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (N1 > EDT_MAX_DIM || N2 > EDT_MAX_DIM || N3 > EDT_MAX_DIM)
        BFD_FAIL(-1, std::string(who) + ": every dimension must be at most 16384 (the squared distances are int32)");
    if (!volume_fits(N1, N2, N3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    for (int a = 0; a < 3; a++)
        if (box[a] < 3 || box[a] > MAX_BOX || !(box[a] & 1)) BFD_FAIL(-1, std::string(who) + ": every box size must be odd and 3 .. 31");
    if (!(interiorThreshold >= RIM_MIN_THRESHOLD) || !(interiorThreshold <= FLT_MAX))
        BFD_FAIL(-1, std::string(who) + ": interiorThreshold must be finite and at least 512 (the exact sum of the dense values rests on it)");
    if (maxBoost != maxBoost) BFD_FAIL(-1, std::string(who) + ": maxBoost is not a number");
    if (!(distanceScale > 0.0) || !std::isfinite(distanceScale)) BFD_FAIL(-1, std::string(who) + ": distanceScale must be finite and positive");
    if (!(sigma > 1e-15) || !std::isfinite(sigma)) BFD_FAIL(-1, std::string(who) + ": sigma must be finite and positive");
    const int radius = gauss_radius(sigma, 4.0);
    if (radius < 0) BFD_FAIL(-1, std::string(who) + ": the radius int(4 sigma + 0.5) is above " + std::to_string(GAUSS_MAX_RADIUS));
    if (floorValue && !(fabsf(*floorValue) <= FLT_MAX)) BFD_FAIL(-1, std::string(who) + ": the floor is not finite");
    if (globalMeanGiven != 0 && globalMeanGiven != 1) BFD_FAIL(-1, std::string(who) + ": globalMeanGiven must be 0 or 1");
    if (globalMeanGiven && !(fabsf(*globalMean) <= FLT_MAX)) BFD_FAIL(-1, std::string(who) + ": the given global mean is not finite");
    const size_t n = (size_t)(N1 * N2 * N3);
    if (n) {
        // out is ct itself or apart from it; every other output is apart from the inputs and from the other outputs
        const void *io[7] = {ct, bone, out, interior, d2, bi, bm};
        const size_t bytes[7] = {n * 4, n, n * 4, n, n * 4, n * 4, n * 4};
        for (int p = 0; p < 7; p++)
            for (int q = std::max(p + 1, 2); q < 7; q++) {
                if (!io[p] || !io[q] || (p == 0 && q == 2 && out == ct)) continue;
                if (overlap(io[p], bytes[p], io[q], bytes[q])) BFD_FAIL(-1, std::string(who) + ": an output may not overlap an input or another output (out may be ct itself)");
            }
    }

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "the volume is empty: there is no interior");

    const int64_t rows = N1 * N2, W = edt_row_words(N3), nWords = rows * W;
    DevTemp<float> dct, df, dm;
    DevTemp<uint8_t> dbone, dinterior;
    DevTemp<uint64_t> boneBits, bitsA, bitsB;
    DevTemp<int32_t> dd2;
    DevTemp<edt_site> scratch;                        // the stacks of the distance transform, then the second volume of each filter: 8 B per voxel
    DevTemp<unsigned long long> acc;
    DevTemp<double> dtable;
    Events ev;
    float ms1 = 0.f, ms2 = 0.f, ms3 = 0.f;
    unsigned long long r[ACC_COUNT];
    static_assert(sizeof(edt_site) == 2 * sizeof(float), "the scratch volume holds stack entries, then two float32 volumes");
    BFD_STEP(dct.alloc(n));
    BFD_STEP(dbone.alloc(n));
    BFD_STEP(df.alloc(n));
    BFD_STEP(dm.alloc(n));
    BFD_STEP(boneBits.alloc((size_t)nWords));
    BFD_STEP(bitsA.alloc((size_t)nWords));
    BFD_STEP(bitsB.alloc((size_t)nWords));
    BFD_STEP(dd2.alloc(n));
    BFD_STEP(scratch.alloc(n));
    BFD_STEP(acc.alloc(ACC_COUNT));
    if (interior) BFD_STEP(dinterior.alloc(n));
    BFD_STEP(hipMemset(acc, 0, sizeof r));
    BFD_STEP(hipMemcpy(dct, ct, n * 4, hipMemcpyHostToDevice));
    BFD_STEP(hipMemcpy(dbone, bone, n, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());

    // 1. the preparation pass and the erosion
    const unsigned wordBlocks = blocks_for(nWords, WAVES, RIM_BLOCKS);
    const int s[3] = {box[0], box[1], box[2]};
    uint64_t *interiorBits = nullptr;
    BFD_STEP(ev.record(0));
    hipLaunchKernelGGL(rim_prepare, dim3(wordBlocks), dim3(THREADS), 0, 0, dct.p, dbone.p, df.p, dm.p, boneBits.p, rows, N3, W, interiorThreshold,
                       floorValue ? 1 : 0, floorValue ? *floorValue : 0.f, acc.p);
    BFD_STEP(hipGetLastError());
    BFD_STEP(hipMemcpyAsync(bitsA, boneBits, (size_t)nWords * 8, hipMemcpyDeviceToDevice, 0));      // the erosion writes both of its buffers
    BFD_STEP(bfd_stage_box_morphology(bitsA, bitsB, (int)N1, (int)N2, (int)N3, s, 0, 0, &interiorBits));
    hipLaunchKernelGGL(rim_count, dim3(blocks_for(nWords, THREADS, RIM_BLOCKS)), dim3(THREADS), 0, 0, interiorBits, nWords, acc.p + ACC_INTERIOR);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(&ms1, 0, 1));
    // the refusals, the mean and the existence of an interior: what the host needs before the distance transform
    BFD_STEP(hipMemcpy(r, acc, sizeof r, hipMemcpyDeviceToHost));
    if (r[ACC_BAD] & BAD_NOT_FINITE) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "a CT value is not finite");
    if (r[ACC_BAD] & BAD_TOO_LARGE) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "a value at or above the interior threshold is at or above 2^17");
    if (!r[ACC_DENSE] && !globalMeanGiven) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "no voxel is at or above the interior threshold: there is no global mean");
    if (!r[ACC_INTERIOR]) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "the erosion leaves no interior voxel: there is no distance to take");
    const float gmean = globalMeanGiven ? *globalMean : rim_mean(r[ACC_SUM], r[ACC_DENSE]);

    // 2. the distance transform, the two filters and the largest squared distance of an edge voxel
    const double sig[3] = {sigma, sigma, sigma};
    const int rad[3] = {radius, radius, radius};
    float *half0 = (float *)scratch.p, *half1 = half0 + n;
    void *dbi = nullptr, *dbm = nullptr;
    BFD_STEP(ev.record(0));
    BFD_STEP(bfd_stage_edt_squared(interiorBits, dd2.p, scratch.p, N1, N2, N3));
    hipLaunchKernelGGL(rim_edge, dim3(wordBlocks), dim3(THREADS), 0, 0, boneBits.p, interiorBits, dd2.p, dinterior.p, rows, N3, W, acc.p);
    BFD_STEP(hipGetLastError());
    BFD_STEP(bfd_stage_gaussian3d(1, df.p, half0, N1, N2, N3, sig, rad, 0, 0.0, &dbi));
    BFD_STEP(bfd_stage_gaussian3d(1, dm.p, half1, N1, N2, N3, sig, rad, 0, 0.0, &dbm));
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(&ms2, 0, 1));
    // the largest squared distance sizes the weight table, which the host forms: exp as numpy takes it
    BFD_STEP(hipMemcpy(r, acc, sizeof r, hipMemcpyDeviceToHost));
    std::vector<double> table;
    rim_weight_table(distanceScale, (int64_t)r[ACC_MAXD2], gauss_numpy_vector_exp(), table);
    BFD_STEP(dtable.alloc(table.size()));
    BFD_STEP(hipMemcpy(dtable, table.data(), table.size() * 8, hipMemcpyHostToDevice));

    // 3. the blend, in place in the CT volume
    BFD_STEP(ev.record(0));
    hipLaunchKernelGGL(rim_blend_pass, dim3(wordBlocks), dim3(THREADS), 0, 0, dct.p, boneBits.p, interiorBits, dd2.p, (const float *)dbi, (const float *)dbm, dtable.p,
                       (int64_t)table.size(), gmean, maxBoost, rows, N3, W, acc.p);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(&ms3, 0, 1));
    BFD_STEP(hipMemcpy(r, acc, sizeof r, hipMemcpyDeviceToHost));
    BFD_STEP(hipMemcpy(out, dct, n * 4, hipMemcpyDeviceToHost));
    if (interior) BFD_STEP(hipMemcpy(interior, dinterior, n, hipMemcpyDeviceToHost));
    if (d2) BFD_STEP(hipMemcpy(d2, dd2, n * 4, hipMemcpyDeviceToHost));
    if (bi) BFD_STEP(hipMemcpy(bi, dbi, n * 4, hipMemcpyDeviceToHost));
    if (bm) BFD_STEP(hipMemcpy(bm, dbm, n * 4, hipMemcpyDeviceToHost));
    const int order[8] = {ACC_BONE, ACC_INTERIOR, ACC_DENSE, ACC_EDGE, ACC_GLOBAL, ACC_CLIPPED, ACC_CHANGED, ACC_MAXD2};
    for (int q = 0; q < 8; q++) stats[q] = (int64_t)r[order[q]];
    if (!globalMeanGiven) *globalMean = gmean;
    if (kernelMs) *kernelMs = ms1 + ms2 + ms3;
    return 0;
}
