// The whole-volume steps of the pseudo-CT from ZTE / PETRA on MI355X, in the caller's numpy C order (k fastest).
//
// Replace, in BabelBrain/CTZTEProcessing.py (ConvertZTE_PETRA_pCT) and its caller,
//     min, max, the 2^16 check and np.histogram of astype(int)                      :559-562                   -> bfd_integer_histogram3d
//     the masked copy and np.percentile                                             :588-591                   -> bfd_order_statistics3d
//     np.histogram(x[x > t], bins)                                                  :476-477, BabelDatasetPreps.py:828 -> bfd_uniform_histogram3d
//     the division, the head, np.max, the eroded head and the range test            :577, :592-597             -> bfd_pseudo_ct_candidates3d
//     the six masked stores of the HU values                                        :608-621                   -> bfd_pseudo_ct_convert3d
// (the largest component with this function's tie rule, :599-606, is bfd_select_component3d in bfd_morphology.hip, next to the labelling).
// The arithmetic per voxel is in bfd_pseudoct_core.h, which a plain C++ compiler accepts too.
//
// Every kernel takes quads of voxels (one 128-bit load of float32 values, two of float64; a byte mask as one 32-bit word) in a loop whose trip
// count is the same for every thread of the launch, because the counting below uses ballots of whole waves.
//   reduce    min and max as order-preserving 64-bit keys of the float64 value, and the count, of all voxels, of the voxels beyond a threshold, or
//             of the quotients; lanes -> wave -> workgroup -> one atomic triple per workgroup
//   counting  (pc_count) the lanes of a wave that hold the bin of the wave's first active lane add once; the others add for themselves. An MRI volume
//             is more than half one value, and 64 lanes on one LDS word are served one after another
//   integer   an LDS window of INT_WINDOW bins from the first bin on, flushed word by non-zero word; bins beyond the window (a range over 8192) go
//             to global memory through the same counting
//   select    radix select, 8 bits a pass from the top of the key (4 passes for float32, 8 for float64): one LDS histogram of 256 digits per rank,
//             counting the voxels whose key agrees with the rank's prefix so far. The host reads the histograms between the passes and extends the
//             prefixes; after the last pass a prefix is the key of the order statistic. Nothing is sorted and nothing is guessed
//   uniform   np.histogram's bin rule on the edges, staged in LDS with the counts
//   candidates, convert   element-wise
// No kernel waits for another workgroup; every loop is bounded, see the comment at each.
#include <float.h>
#include <string.h>
#include "bfd_internal.h"
#include "bfd_call.h"
#include "bfd_pseudoct_core.h"

namespace {

constexpr int THREADS = 256;
const char *const DATA_REFUSED = ": refused data: ";   // what every data refusal carries after the entry's name (PseudoCT.py turns these into ValueError)
constexpr int64_t SWEEP_BLOCKS = 2048;                 // select, candidates, convert: what lies beyond is taken by the grid-stride loop
constexpr int64_t REDUCE_BLOCKS = 1024;                // reduce: each workgroup ends in three atomics on the same three words
constexpr int HIST_THREADS = 512;
constexpr int64_t HIST_BLOCKS = 512;                   // the two histograms: fewer, larger workgroups, since each flushes its LDS counts
constexpr int INT_WINDOW = 8192;                       // bins of the integer histogram kept in LDS (32 KiB), from the first bin on
constexpr int DIGITS = 256;

// rounds of a launch: every thread makes the same number of trips
static __device__ __forceinline__ int64_t pc_rounds(int64_t quads) { return (quads + (int64_t)gridDim.x * blockDim.x - 1) / ((int64_t)gridDim.x * blockDim.x); }

// the raw bits of quad q
template <bool F64>
static __device__ __forceinline__ void pc_load(const void *values, int64_t q, uint64_t raw[4])
{
    if (F64) {
        const ulonglong2 a = ((const ulonglong2 *)values)[2 * q], b = ((const ulonglong2 *)values)[2 * q + 1];
        raw[0] = a.x; raw[1] = a.y; raw[2] = b.x; raw[3] = b.y;
    } else {
        const uint4 a = ((const uint4 *)values)[q];
        raw[0] = a.x; raw[1] = a.y; raw[2] = a.z; raw[3] = a.w;
    }
}

// hist[bin]++ for every lane with active set; the whole wave calls this together. The lanes that share the first active lane's bin add once.
template <typename H>
static __device__ __forceinline__ void pc_count(H *hist, int bin, bool active)
{
    const unsigned long long act = __ballot(active);
    if (!act) return;                                  // wave-uniform
    const int leader = __ffsll(act) - 1;
    const int lb = __shfl(bin, leader);
    const unsigned long long same = __ballot(active && bin == lb);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(hist + lb, (H)__popcll(same));
    else if (active && bin != lb) atomicAdd(hist + bin, (H)1);
}

// lanes -> wave -> workgroup -> one atomic per word and workgroup; the whole workgroup (THREADS) calls this together. minmax (may be null): [0] takes
// the smallest key, [1] the largest; count takes the sum. With an atomic triple per wave, the 8192 waves of a sweep on three words took 0.24 ms
// at any size, more than the pass over 256^3 itself: the integer histogram there went from 0.336 to 0.094 ms (profiles/README.md, "Pseudo-CT").
static __device__ __forceinline__ void pc_block_reduce(unsigned long long lo, unsigned long long hi, unsigned long long cnt,
                                                       unsigned long long *minmax, unsigned long long *count)
{
    __shared__ unsigned long long part[3][THREADS / 64];
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
        cnt += __shfl_xor(cnt, d);
    }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = lo; part[1][threadIdx.x >> 6] = hi; part[2][threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < THREADS / 64; w++) {
            lo = part[0][w] < lo ? part[0][w] : lo;
            hi = part[1][w] > hi ? part[1][w] : hi;
            cnt += part[2][w];
        }
        if (cnt) {
            if (minmax) { atomicMin(minmax, lo); atomicMax(minmax + 1, hi); }
            atomicAdd(count, cnt);
        }
    }
}

// ---------------------------------------------------------------- reduce ----------------------------------------------------------------

// what: 0 every voxel; 1 the voxels beyond `above`; 2 the quotients v / divisor (-0.5 outside the head)
struct reduce_args { int what, inclusive; double above, divisor; const uint32_t *head; };

// acc[0] = the smallest key (starts all ones), acc[1] = the largest (starts 0), acc[2] = the count
template <bool F64>
__global__ __launch_bounds__(THREADS) void pc_reduce(const void *__restrict__ values, int64_t n, int64_t quads, const reduce_args a, unsigned long long *__restrict__ acc)
{
    unsigned long long lo = ~0ull, hi = 0ull, cnt = 0ull;
    const int64_t rounds = pc_rounds(quads);
    for (int64_t it = 0; it < rounds; it++) {          // ends: the same trip count for every thread
        const int64_t q = (it * gridDim.x + blockIdx.x) * THREADS + threadIdx.x;
        if (q >= quads) continue;
        uint64_t raw[4];
        pc_load<F64>(values, q, raw);
        const uint32_t h = a.head ? a.head[q] : 0u;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            if (4 * q + b >= n) continue;
            double v = pc_value<F64>(raw[b]);
            if (a.what == 1 && !pc_selected(v, a.above, a.inclusive != 0)) continue;
            if (a.what == 2) v = pc_quotient(v, a.divisor, a.head != nullptr, ((h >> (8 * b)) & 0xFFu) != 0);
            const unsigned long long key = pc_key64(pc_bits64(v));
            lo = key < lo ? key : lo;
            hi = key > hi ? key : hi;
            cnt++;
        }
    }
    pc_block_reduce(lo, hi, cnt, acc, acc + 2);      // every thread arrives here: the loop above has no early exit from the kernel
}

// ---------------------------------------------------------------- integer histogram ----------------------------------------------------------------

// counts: `bins` words, zero before the launch; bin of v = trunc(v) - first, inside 0 .. bins - 1 for every voxel (first and bins come from the
// volume's own min and max)
template <bool F64>
__global__ __launch_bounds__(HIST_THREADS) void pc_integer_hist(const void *__restrict__ values, int64_t n, int64_t quads, int64_t first, int bins,
                                                                uint32_t *__restrict__ counts)
{
    __shared__ uint32_t win[INT_WINDOW];
    const int inWin = bins < INT_WINDOW ? bins : INT_WINDOW;
    for (int w = threadIdx.x; w < inWin; w += HIST_THREADS) win[w] = 0;
    __syncthreads();
    const int64_t rounds = pc_rounds(quads);
    for (int64_t it = 0; it < rounds; it++) {          // ends: the same trip count for every thread (pc_count needs whole waves)
        const int64_t q = (it * gridDim.x + blockIdx.x) * HIST_THREADS + threadIdx.x;
        uint64_t raw[4] = {0, 0, 0, 0};
        if (q < quads) pc_load<F64>(values, q, raw);
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const bool live = q < quads && 4 * q + b < n;
            int64_t bin = live ? pc_trunc(pc_value<F64>(raw[b])) - first : 0;
            bin = bin < 0 ? 0 : (bin >= bins ? bins - 1 : bin);         // never outside the counts, whatever the data
            pc_count(win, (int)bin, live && bin < INT_WINDOW);
            pc_count(counts, (int)bin, live && bin >= INT_WINDOW);
        }
    }
    __syncthreads();
    for (int w = threadIdx.x; w < inWin; w += HIST_THREADS)
        if (win[w]) atomicAdd(counts + w, win[w]);
}

// ---------------------------------------------------------------- radix select ----------------------------------------------------------------

struct select_args {
    const uint32_t *mask;                              // byte mask as words, or null
    double above;
    int inclusive, R, shift, keyBits;                  // this pass counts digit (key >> shift) & 255 of the keys with key >> (shift + 8) == prefix[r]
    uint64_t prefix[PC_MAX_RANKS];
};

// hist: R * 256 words, zero before the launch
template <bool F64>
__global__ __launch_bounds__(THREADS) void pc_select_pass(const void *__restrict__ values, int64_t n, int64_t quads, const select_args a, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t h[PC_MAX_RANKS * DIGITS];
    for (int w = threadIdx.x; w < a.R * DIGITS; w += THREADS) h[w] = 0;
    __syncthreads();
    const bool top = a.shift + 8 >= a.keyBits;         // the first pass: every key agrees with the empty prefix
    const int64_t rounds = pc_rounds(quads);
    for (int64_t it = 0; it < rounds; it++) {          // ends: the same trip count for every thread (pc_count needs whole waves)
        const int64_t q = (it * gridDim.x + blockIdx.x) * THREADS + threadIdx.x;
        uint64_t raw[4] = {0, 0, 0, 0};
        uint32_t m = 0;
        if (q < quads) {
            m = a.mask ? a.mask[q] : 0x01010101u;
            if (m) pc_load<F64>(values, q, raw);
        }
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const bool live = q < quads && 4 * q + b < n && ((m >> (8 * b)) & 0xFFu) && pc_selected(pc_value<F64>(raw[b]), a.above, a.inclusive != 0);
            const uint64_t key = pc_key<F64>(raw[b]);
            const int digit = (int)((key >> a.shift) & 0xFFu);
            const uint64_t high = top ? 0 : key >> (a.shift + 8);
            for (int r = 0; r < a.R; r++)              // wave-uniform bound
                pc_count(h + r * DIGITS, digit, live && (top || high == a.prefix[r]));
        }
    }
    __syncthreads();
    for (int w = threadIdx.x; w < a.R * DIGITS; w += THREADS)
        if (h[w]) atomicAdd(hist + w, h[w]);
}

// ---------------------------------------------------------------- uniform histogram ----------------------------------------------------------------

// counts: `bins` words, zero before the launch. The values beyond the threshold that lie inside edges[0] .. edges[bins] are counted
template <bool F64>
__global__ __launch_bounds__(HIST_THREADS) void pc_uniform_hist(const void *__restrict__ values, int64_t n, int64_t quads, double above, int inclusive, int bins,
                                                                const double *__restrict__ edges, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t h[PC_MAX_BINS];
    __shared__ double e[PC_MAX_BINS + 1];
    for (int w = threadIdx.x; w < bins; w += HIST_THREADS) h[w] = 0;
    for (int w = threadIdx.x; w <= bins; w += HIST_THREADS) e[w] = edges[w];
    __syncthreads();
    const double first = e[0], last = e[bins];
    const int64_t rounds = pc_rounds(quads);
    for (int64_t it = 0; it < rounds; it++) {          // ends: the same trip count for every thread (pc_count needs whole waves)
        const int64_t q = (it * gridDim.x + blockIdx.x) * HIST_THREADS + threadIdx.x;
        uint64_t raw[4] = {0, 0, 0, 0};
        if (q < quads) pc_load<F64>(values, q, raw);
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const double v = pc_value<F64>(raw[b]);
            const bool live = q < quads && 4 * q + b < n && pc_selected(v, above, inclusive != 0) && v >= first && v <= last;
            int bin = live ? pc_uniform_bin(v, first, last, bins, e) : 0;
            bin = bin < 0 ? 0 : (bin >= bins ? bins - 1 : bin);         // never outside the counts, whatever the edges
            pc_count(h, bin, live);
        }
    }
    __syncthreads();
    for (int w = threadIdx.x; w < bins; w += HIST_THREADS)
        if (h[w]) atomicAdd(counts + w, h[w]);
}

// ---------------------------------------------------------------- candidates and conversion ----------------------------------------------------------------

// mask = lo <= g <= hi, g = the quotient, or `maximum` where the eroded head is 0. acc[0] = voxels of the mask
template <bool F64>
__global__ __launch_bounds__(THREADS) void pc_candidates(const void *__restrict__ values, int64_t n, int64_t quads, double divisor, const uint32_t *__restrict__ head,
                                                         const uint32_t *__restrict__ eroded, double maximum, double lo, double hi, uint32_t *__restrict__ mask,
                                                         unsigned long long *__restrict__ acc)
{
    unsigned long long cnt = 0;
    for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * THREADS) {         // grid-stride: ends
        uint64_t raw[4];
        pc_load<F64>(values, q, raw);
        const uint32_t h = head ? head[q] : 0u, er = eroded[q];
        uint32_t o = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const double qv = pc_quotient(pc_value<F64>(raw[b]), divisor, head != nullptr, ((h >> (8 * b)) & 0xFFu) != 0);
            const double g = ((er >> (8 * b)) & 0xFFu) ? qv : maximum;
            if (4 * q + b < n && g >= lo && g <= hi) { o |= 1u << (8 * b); cnt++; }
        }
        mask[q] = o;
    }
    pc_block_reduce(~0ull, 0ull, cnt, nullptr, acc);  // every thread arrives here: the loop above has no early exit from the kernel
}

template <bool F64, bool OUT64>
__global__ __launch_bounds__(THREADS) void pc_convert(const void *__restrict__ values, int64_t quads, double divisor, const uint32_t *__restrict__ head,
                                                      const uint32_t *__restrict__ bone, const uint32_t *__restrict__ skin, const uint32_t *__restrict__ cavities,
                                                      double slope, double offset, void *__restrict__ out)
{
    for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * THREADS) {         // grid-stride: ends
        const uint32_t h = head ? head[q] : 0u, bn = bone[q], sk = skin[q], cv = cavities[q];
        uint64_t raw[4] = {0, 0, 0, 0};
        if (bn) pc_load<F64>(values, q, raw);          // the values matter under the bone region alone
        double ct[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int s = 8 * b;
            const bool isBone = ((bn >> s) & 0xFFu) != 0;
            const double qv = isBone ? pc_quotient(pc_value<F64>(raw[b]), divisor, head != nullptr, ((h >> s) & 0xFFu) != 0) : 0.0;
            ct[b] = pc_hu(qv, slope, offset, ((sk >> s) & 0xFFu) != 0, isBone, ((cv >> s) & 0xFFu) != 0);
        }
        if (OUT64) {
            ((double2 *)out)[2 * q] = make_double2(ct[0], ct[1]);
            ((double2 *)out)[2 * q + 1] = make_double2(ct[2], ct[3]);
        } else {
            ((float4 *)out)[q] = make_float4((float)ct[0], (float)ct[1], (float)ct[2], (float)ct[3]);
        }
    }
}

// ---------------------------------------------------------------- host ----------------------------------------------------------------

// the values of a call on the device, padded to whole quads
struct Volume {
    DevTemp<uint8_t> d;
    int64_t n = 0, quads = 0;
    size_t item = 4;
    hipError_t reserve(int dtype, size_t count)
    {
        n = (int64_t)count; quads = (n + 3) / 4; item = dtype == PC_F64 ? 8 : 4;
        return d.alloc((size_t)quads * 4 * item);
    }
    hipError_t upload(const void *host) { return hipMemcpy(d.p, host, (size_t)n * item, hipMemcpyHostToDevice); }
};

// a byte mask on the device, padded to whole words with zeros
struct Bytes {
    DevTemp<uint8_t> d;
    hipError_t reserve(size_t n) { return d.alloc((n + 3) / 4 * 4); }
    hipError_t upload(const uint8_t *host, size_t n)
    {
        const size_t np = (n + 3) / 4 * 4;
        if (np > n) { hipError_t e = hipMemset(d.p + (np - 4), 0, 4); if (e != hipSuccess) return e; }
        return hipMemcpy(d.p, host, n, hipMemcpyHostToDevice);
    }
    const uint32_t *words() const { return (const uint32_t *)d.p; }
};

static const char *check_volume(int dtype, const void *values, int64_t N1, int64_t N2, int64_t N3)
{
    if (dtype != PC_F32 && dtype != PC_F64) return ": dtype must be 1 (float32) or 3 (float64)";
    if (!values) return ": null argument";
    if (N1 < 0 || N2 < 0 || N3 < 0) return ": negative dimension";
    if (!volume_fits(N1, N2, N3)) return ": the volume has 2^31 voxels or more (limit: fewer than 2^31)";
    return nullptr;
}

static void launch_reduce(int dtype, const Volume &v, const reduce_args &a, unsigned long long *acc)
{
    const unsigned blocks = blocks_for(v.quads, THREADS, REDUCE_BLOCKS);
    if (dtype == PC_F64) hipLaunchKernelGGL(pc_reduce<true>, dim3(blocks), dim3(THREADS), 0, 0, (const void *)v.d.p, v.n, v.quads, a, acc);
    else hipLaunchKernelGGL(pc_reduce<false>, dim3(blocks), dim3(THREADS), 0, 0, (const void *)v.d.p, v.n, v.quads, a, acc);
}

static bool key_finite(unsigned long long k) { return k > PC_KEY64_NEG_INF && k < PC_KEY64_POS_INF; }

}  // namespace

extern "C" int bfd_integer_histogram3d(int device, int dtype, const void *values, int64_t N1, int64_t N2, int64_t N3, int64_t *counts, int64_t *first,
                                       int64_t *numBins, double *range, float *kernelMs)
{
    static const char *who = "bfd_integer_histogram3d";
    // every argument error is reported before a device is looked for
    if (const char *bad = check_volume(dtype, values, N1, N2, N3)) BFD_FAIL(-1, std::string(who) + bad);
    if (!counts || !first || !numBins || !range) BFD_FAIL(-1, std::string(who) + ": null argument");
    const size_t n = (size_t)(N1 * N2 * N3);
    if (n && overlap(values, n * (dtype == PC_F64 ? 8 : 4), counts, 8 * (size_t)PC_MAX_INT_BINS)) BFD_FAIL(-1, std::string(who) + ": counts may not alias values");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "the volume is empty: there is no range");

    Volume vol;
    DevTemp<unsigned long long> acc;
    DevTemp<uint32_t> dcounts;
    Events ev;
    float ms1 = 0.f, ms2 = 0.f;
    unsigned long long r[3] = {~0ull, 0ull, 0ull};
    BFD_STEP(vol.reserve(dtype, n));
    BFD_STEP(acc.alloc(3));
    BFD_STEP(dcounts.alloc(PC_MAX_INT_BINS));
    BFD_STEP(hipMemset(dcounts, 0, 4 * (size_t)PC_MAX_INT_BINS));
    BFD_STEP(vol.upload(values));
    BFD_STEP(hipMemcpy(acc, r, sizeof r, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    reduce_args ra = {0, 0, 0.0, 1.0, nullptr};
    launch_reduce(dtype, vol, ra, acc.p);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(&ms1, 0, 1));
    // the range sizes the histogram: the two keys are what the host needs between the kernels
    BFD_STEP(hipMemcpy(r, acc, sizeof r, hipMemcpyDeviceToHost));
    if (!key_finite(r[0]) || !key_finite(r[1])) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "a value is not finite");
    const double mn = pc_from_bits64(pc_unkey64(r[0])), mx = pc_from_bits64(pc_unkey64(r[1]));
    if (mx - mn > PC_MAX_RANGE) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "The range of values in the ZTE file exceeds 2^16");
    if (mn < -0x1p62 || mx > 0x1p62) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "a value is beyond +-2^62: it has no int64 truncation");
    const int64_t lowest = pc_trunc(mn);
    const int bins = (int)(pc_trunc(mx) - lowest + 1);  // 1 .. 65536: truncation moves min and max towards each other or by less than 1 each
    if (bins < 1 || bins > PC_MAX_INT_BINS) BFD_FAIL(-10, std::string(who) + ": the bin count left 1 .. 65536");

    BFD_STEP(ev.record(0));
    const unsigned blocks = blocks_for(vol.quads, HIST_THREADS, HIST_BLOCKS);
    if (dtype == PC_F64) hipLaunchKernelGGL(pc_integer_hist<true>, dim3(blocks), dim3(HIST_THREADS), 0, 0, (const void *)vol.d.p, vol.n, vol.quads, lowest, bins, dcounts.p);
    else hipLaunchKernelGGL(pc_integer_hist<false>, dim3(blocks), dim3(HIST_THREADS), 0, 0, (const void *)vol.d.p, vol.n, vol.quads, lowest, bins, dcounts.p);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(&ms2, 0, 1));
    std::vector<uint32_t> host((size_t)bins);
    BFD_STEP(hipMemcpy(host.data(), dcounts, 4 * (size_t)bins, hipMemcpyDeviceToHost));
    for (int q = 0; q < bins; q++) counts[q] = (int64_t)host[(size_t)q];
    *first = lowest; *numBins = bins;
    range[0] = mn; range[1] = mx;
    if (kernelMs) *kernelMs = ms1 + ms2;
    return 0;
}

extern "C" int bfd_order_statistics3d(int device, int dtype, const void *values, const uint8_t *mask, int64_t N1, int64_t N2, int64_t N3, double above,
                                      int inclusive, const int64_t *ranks, int R, double quantile, int64_t *count, int64_t *ranksUsed, double *statistics,
                                      float *kernelMs)
{
    static const char *who = "bfd_order_statistics3d";
    // every argument error is reported before a device is looked for
    if (const char *bad = check_volume(dtype, values, N1, N2, N3)) BFD_FAIL(-1, std::string(who) + bad);
    if (!count || !statistics) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (above != above) BFD_FAIL(-1, std::string(who) + ": the threshold is not a number");
    if (inclusive != 0 && inclusive != 1) BFD_FAIL(-1, std::string(who) + ": inclusive must be 0 or 1");
    if (ranks && (R < 1 || R > PC_MAX_RANKS)) BFD_FAIL(-1, std::string(who) + ": R must be 1 .. 4 where ranks are given");
    if (!ranks && !(quantile >= 0.0 && quantile <= 100.0)) BFD_FAIL(-1, std::string(who) + ": the quantile must be 0 .. 100 where no ranks are given");
    const size_t n = (size_t)(N1 * N2 * N3);

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "no voxel is selected: there is no order statistic");

    const bool f64 = dtype == PC_F64;
    Volume vol;
    Bytes dmask;
    DevTemp<uint32_t> dhist;
    Events ev;
    float total = 0.f;
    BFD_STEP(vol.reserve(dtype, n));
    if (mask) BFD_STEP(dmask.reserve(n));
    BFD_STEP(dhist.alloc(PC_MAX_RANKS * DIGITS));
    BFD_STEP(vol.upload(values));
    if (mask) BFD_STEP(dmask.upload(mask, n));
    BFD_STEP(ev.create());

    select_args a;
    a.mask = mask ? dmask.words() : nullptr;
    a.above = above; a.inclusive = inclusive;
    a.keyBits = f64 ? 64 : 32;
    a.R = ranks ? R : 2;
    int64_t left[PC_MAX_RANKS] = {0, 0, 0, 0}, used[PC_MAX_RANKS] = {0, 0, 0, 0}, selected = 0;
    for (int r = 0; r < PC_MAX_RANKS; r++) a.prefix[r] = 0;
    std::vector<uint32_t> hist(PC_MAX_RANKS * DIGITS);
    const unsigned blocks = blocks_for(vol.quads, THREADS, SWEEP_BLOCKS);
    for (a.shift = a.keyBits - 8; a.shift >= 0; a.shift -= 8) {         // 4 or 8 passes
        float ms = 0.f;
        BFD_STEP(hipMemset(dhist, 0, 4 * (size_t)(a.R * DIGITS)));
        BFD_STEP(ev.record(0));
        if (f64) hipLaunchKernelGGL(pc_select_pass<true>, dim3(blocks), dim3(THREADS), 0, 0, (const void *)vol.d.p, vol.n, vol.quads, a, dhist.p);
        else hipLaunchKernelGGL(pc_select_pass<false>, dim3(blocks), dim3(THREADS), 0, 0, (const void *)vol.d.p, vol.n, vol.quads, a, dhist.p);
        BFD_STEP(hipGetLastError());
        BFD_STEP(ev.record(1));
        BFD_STEP(ev.sync(1));
        BFD_STEP(ev.elapsed(&ms, 0, 1));
        total += ms;
        // the digit counts of each rank's prefix: what the host needs between the passes
        BFD_STEP(hipMemcpy(hist.data(), dhist, 4 * (size_t)(a.R * DIGITS), hipMemcpyDeviceToHost));
        if (a.shift == a.keyBits - 8) {
            // the first pass counts every selected voxel: the count, then the ranks
            for (int d = 0; d < DIGITS; d++) selected += hist[(size_t)d];
            if (selected == 0) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "no voxel is selected: there is no order statistic");
            if (ranks) {
                for (int r = 0; r < R; r++) {
                    if (ranks[r] < 0 || ranks[r] >= selected) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "a rank is outside 0 .. n - 1");
                    used[r] = ranks[r];
                }
            } else {
                double g;
                pc_quantile_ranks(selected, quantile, &used[0], &used[1], &g);
            }
            for (int r = 0; r < a.R; r++) left[r] = used[r];
        }
        for (int r = 0; r < a.R; r++) {
            int64_t below = 0;
            int d = 0;
            for (; d < DIGITS - 1; d++) {               // ends at 255 at the latest
                const int64_t c = hist[(size_t)(r * DIGITS + d)];
                if (left[r] < below + c) break;
                below += c;
            }
            left[r] -= below;
            a.prefix[r] = (a.prefix[r] << 8) | (uint64_t)d;
        }
    }
    *count = selected;
    for (int r = 0; r < a.R; r++) {
        statistics[r] = f64 ? pc_key_value<true>(a.prefix[r]) : pc_key_value<false>(a.prefix[r]);
        if (ranksUsed) ranksUsed[r] = used[r];
    }
    if (kernelMs) *kernelMs = total;
    return 0;
}

extern "C" int bfd_uniform_histogram3d(int device, int dtype, const void *values, int64_t N1, int64_t N2, int64_t N3, double above, int inclusive, int bins,
                                       const double *edges, int64_t *counts, double *range, int64_t *count, float *kernelMs)
{
    static const char *who = "bfd_uniform_histogram3d";
    // every argument error is reported before a device is looked for
    if (const char *bad = check_volume(dtype, values, N1, N2, N3)) BFD_FAIL(-1, std::string(who) + bad);
    if (edges ? !counts : (!range || !count)) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (above != above) BFD_FAIL(-1, std::string(who) + ": the threshold is not a number");
    if (inclusive != 0 && inclusive != 1) BFD_FAIL(-1, std::string(who) + ": inclusive must be 0 or 1");
    if (edges) {
        if (bins < 1 || bins > PC_MAX_BINS) BFD_FAIL(-1, std::string(who) + ": bins must be 1 .. 1024");
        for (int q = 0; q < bins; q++)
            if (!(edges[q] <= edges[q + 1]) || !(edges[q] - edges[q] == 0.0) || !(edges[q + 1] - edges[q + 1] == 0.0))
                BFD_FAIL(-1, std::string(who) + ": the edges must be finite and ascending");
        if (!(edges[0] < edges[bins])) BFD_FAIL(-1, std::string(who) + ": the edges must be finite and ascending");
    }
    const size_t n = (size_t)(N1 * N2 * N3);

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) {
        if (edges) for (int q = 0; q < bins; q++) counts[q] = 0;
        else { *count = 0; range[0] = range[1] = 0.0; }
        return 0;
    }

    Volume vol;
    DevTemp<unsigned long long> acc;
    DevTemp<uint32_t> dcounts;
    DevTemp<double> dedges;
    Events ev;
    unsigned long long r[3] = {~0ull, 0ull, 0ull};
    BFD_STEP(vol.reserve(dtype, n));
    if (edges) {
        BFD_STEP(dcounts.alloc((size_t)bins));
        BFD_STEP(dedges.alloc((size_t)bins + 1));
        BFD_STEP(hipMemset(dcounts, 0, 4 * (size_t)bins));
        BFD_STEP(hipMemcpy(dedges, edges, 8 * ((size_t)bins + 1), hipMemcpyHostToDevice));
    } else {
        BFD_STEP(acc.alloc(3));
        BFD_STEP(hipMemcpy(acc, r, sizeof r, hipMemcpyHostToDevice));
    }
    BFD_STEP(vol.upload(values));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    if (edges) {
        const unsigned blocks = blocks_for(vol.quads, HIST_THREADS, HIST_BLOCKS);
        if (dtype == PC_F64) hipLaunchKernelGGL(pc_uniform_hist<true>, dim3(blocks), dim3(HIST_THREADS), 0, 0, (const void *)vol.d.p, vol.n, vol.quads, above, inclusive, bins, dedges.p, dcounts.p);
        else hipLaunchKernelGGL(pc_uniform_hist<false>, dim3(blocks), dim3(HIST_THREADS), 0, 0, (const void *)vol.d.p, vol.n, vol.quads, above, inclusive, bins, dedges.p, dcounts.p);
    } else {
        reduce_args ra = {1, inclusive, above, 1.0, nullptr};
        launch_reduce(dtype, vol, ra, acc.p);
    }
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    float ms = 0.f;
    BFD_STEP(ev.elapsed(&ms, 0, 1));
    if (edges) {
        std::vector<uint32_t> host((size_t)bins);
        BFD_STEP(hipMemcpy(host.data(), dcounts, 4 * (size_t)bins, hipMemcpyDeviceToHost));
        for (int q = 0; q < bins; q++) counts[q] = (int64_t)host[(size_t)q];
    } else {
        BFD_STEP(hipMemcpy(r, acc, sizeof r, hipMemcpyDeviceToHost));
        if (r[2] && (!key_finite(r[0]) || !key_finite(r[1]))) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "a selected value is not finite");
        *count = (int64_t)r[2];
        range[0] = r[2] ? pc_from_bits64(pc_unkey64(r[0])) : 0.0;
        range[1] = r[2] ? pc_from_bits64(pc_unkey64(r[1])) : 0.0;
    }
    if (kernelMs) *kernelMs = ms;
    return 0;
}

extern "C" int bfd_pseudo_ct_candidates3d(int device, int dtype, const void *values, int64_t N1, int64_t N2, int64_t N3, double divisor, const uint8_t *head,
                                          const uint8_t *eroded, double lo, double hi, uint8_t *mask, double *maximum, int64_t *count, float *kernelMs)
{
    static const char *who = "bfd_pseudo_ct_candidates3d";
    // every argument error is reported before a device is looked for
    if (const char *bad = check_volume(dtype, values, N1, N2, N3)) BFD_FAIL(-1, std::string(who) + bad);
    if (!eroded || !mask || !maximum || !count) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (!(divisor - divisor == 0.0) || divisor == 0.0) BFD_FAIL(-1, std::string(who) + ": the divisor must be finite and not zero");
    if (lo != lo || hi != hi) BFD_FAIL(-1, std::string(who) + ": lo or hi is not a number");
    const size_t n = (size_t)(N1 * N2 * N3), vb = n * (dtype == PC_F64 ? 8 : 4);
    if (n && (overlap(values, vb, mask, n) || overlap(eroded, n, mask, n) || (head && overlap(head, n, mask, n))))
        BFD_FAIL(-1, std::string(who) + ": mask may not alias an input");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "the volume is empty: there is no maximum");

    Volume vol;
    Bytes dhead, deroded, dmask;
    DevTemp<unsigned long long> acc;
    Events ev;
    float ms1 = 0.f, ms2 = 0.f;
    unsigned long long r[3] = {~0ull, 0ull, 0ull}, zero = 0;
    BFD_STEP(vol.reserve(dtype, n));
    if (head) BFD_STEP(dhead.reserve(n));
    BFD_STEP(deroded.reserve(n));
    BFD_STEP(dmask.reserve(n));
    BFD_STEP(acc.alloc(3));
    BFD_STEP(vol.upload(values));
    if (head) BFD_STEP(dhead.upload(head, n));
    BFD_STEP(deroded.upload(eroded, n));
    BFD_STEP(hipMemcpy(acc, r, sizeof r, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    reduce_args ra = {2, 0, 0.0, divisor, head ? dhead.words() : nullptr};
    launch_reduce(dtype, vol, ra, acc.p);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(&ms1, 0, 1));
    // the maximum is an argument of the second pass and a refusal of the call: the host reads it between the kernels
    BFD_STEP(hipMemcpy(r, acc, sizeof r, hipMemcpyDeviceToHost));
    if (!key_finite(r[0]) || !key_finite(r[1])) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "a quotient is not finite");
    const double mx = pc_from_bits64(pc_unkey64(r[1]));
    BFD_STEP(hipMemcpy(acc, &zero, sizeof zero, hipMemcpyHostToDevice));
    BFD_STEP(ev.record(0));
    const unsigned blocks = blocks_for(vol.quads, THREADS, SWEEP_BLOCKS);
    if (dtype == PC_F64)
        hipLaunchKernelGGL(pc_candidates<true>, dim3(blocks), dim3(THREADS), 0, 0, (const void *)vol.d.p, vol.n, vol.quads, divisor, head ? dhead.words() : nullptr,
                           deroded.words(), mx, lo, hi, (uint32_t *)dmask.d.p, acc.p);
    else
        hipLaunchKernelGGL(pc_candidates<false>, dim3(blocks), dim3(THREADS), 0, 0, (const void *)vol.d.p, vol.n, vol.quads, divisor, head ? dhead.words() : nullptr,
                           deroded.words(), mx, lo, hi, (uint32_t *)dmask.d.p, acc.p);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(&ms2, 0, 1));
    BFD_STEP(hipMemcpy(&zero, acc, sizeof zero, hipMemcpyDeviceToHost));
    BFD_STEP(hipMemcpy(mask, dmask.d.p, n, hipMemcpyDeviceToHost));
    *maximum = mx;
    *count = (int64_t)zero;
    if (kernelMs) *kernelMs = ms1 + ms2;
    return 0;
}

extern "C" int bfd_pseudo_ct_convert3d(int device, int dtype, const void *values, int64_t N1, int64_t N2, int64_t N3, double divisor, const uint8_t *head,
                                       const uint8_t *bone, const uint8_t *skin, const uint8_t *cavities, double slope, double offset, int outDtype, void *out,
                                       float *kernelMs)
{
    static const char *who = "bfd_pseudo_ct_convert3d";
    // every argument error is reported before a device is looked for
    if (const char *bad = check_volume(dtype, values, N1, N2, N3)) BFD_FAIL(-1, std::string(who) + bad);
    if (!bone || !skin || !cavities || !out) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (outDtype != PC_F32 && outDtype != PC_F64) BFD_FAIL(-1, std::string(who) + ": outDtype must be 1 (float32) or 3 (float64)");
    if (!(divisor - divisor == 0.0) || divisor == 0.0) BFD_FAIL(-1, std::string(who) + ": the divisor must be finite and not zero");
    if (slope != slope || offset != offset) BFD_FAIL(-1, std::string(who) + ": slope or offset is not a number");
    const size_t n = (size_t)(N1 * N2 * N3), vb = n * (dtype == PC_F64 ? 8 : 4), ob = n * (outDtype == PC_F64 ? 8 : 4);
    if (n && (overlap(values, vb, out, ob) || overlap(bone, n, out, ob) || overlap(skin, n, out, ob) || overlap(cavities, n, out, ob) ||
              (head && overlap(head, n, out, ob))))
        BFD_FAIL(-1, std::string(who) + ": out may not alias an input");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) return 0;

    Volume vol, dout;
    Bytes dhead, dbone, dskin, dcav;
    Events ev;
    BFD_STEP(vol.reserve(dtype, n));
    BFD_STEP(dout.reserve(outDtype, n));
    if (head) BFD_STEP(dhead.reserve(n));
    BFD_STEP(dbone.reserve(n));
    BFD_STEP(dskin.reserve(n));
    BFD_STEP(dcav.reserve(n));
    BFD_STEP(vol.upload(values));
    if (head) BFD_STEP(dhead.upload(head, n));
    BFD_STEP(dbone.upload(bone, n));
    BFD_STEP(dskin.upload(skin, n));
    BFD_STEP(dcav.upload(cavities, n));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    const unsigned blocks = blocks_for(vol.quads, THREADS, SWEEP_BLOCKS);
    const uint32_t *hw = head ? dhead.words() : nullptr;
#define PC_CONVERT(F64, OUT64)                                                                                                                          \
    hipLaunchKernelGGL((pc_convert<F64, OUT64>), dim3(blocks), dim3(THREADS), 0, 0, (const void *)vol.d.p, vol.quads, divisor, hw, dbone.words(), dskin.words(), \
                       dcav.words(), slope, offset, (void *)dout.d.p)
    if (dtype == PC_F64) { if (outDtype == PC_F64) PC_CONVERT(true, true); else PC_CONVERT(true, false); }
    else { if (outDtype == PC_F64) PC_CONVERT(false, true); else PC_CONVERT(false, false); }
#undef PC_CONVERT
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    BFD_STEP(hipMemcpy(out, dout.d.p, ob, hipMemcpyDeviceToHost));
    return 0;
}
