// The whole-volume stages between the conformal masks and the file Step 2 reads, on MI355X, in the caller's numpy C order (k fastest).
//
// Replace, in BabelBrain/BabelDatasetPreps.py,
//     min, max, the quantisation to 2^CT_quantification levels, np.unique and MapFilter      :1019-1027, :1039   -> bfd_quantize_values3d
//     the Python double loop of the pre-focal cleanup                                         :1121-1133          -> bfd_clear_beyond_bone3d
// (the painting of components by size, :909-929, :1055-1061, :1077-1097, is bfd_paint_components3d in bfd_morphology.hip, next to the labelling).
// The arithmetic of the quantisation and the table builder are in bfd_tissue_core.h, which a plain C++ compiler accepts too.
//
// Quantisation, four kernels over quads of voxels (the mask is read as one 32-bit word, the values as one float4, and only where the word is not 0):
//   minmax    order-preserving integer keys of the values under the mask, reduced per wave, one atomicMin / atomicMax per wave. The host reads the
//             two keys, refuses what the definition does not cover and forms s and r once, in float32
//   presence  a bitmap of 2^bits bits per workgroup in LDS (8 KiB at 16 bits), OR-ed into global memory word by non-zero word at the end
//   table     one workgroup, one thread per chunk of 64 levels: the highest occurring level of the chunks below (max scan), the rows each chunk
//             opens (sum scan), then the rows and a uint16 rank per occurring level
//   apply     level -> rank -> map, v(level) -> quantized. The ranks are staged in LDS up to 12 bits (8 KiB); above, they are read from global
//             memory (at most 128 KiB, resident in L2): staging 64 KiB per workgroup at 15 bits was slower than the global reads at 16
// Cleanup: one wave per line. The line is read once as aligned 32-bit words, four per lane (1024 bytes: every line of up to 1021 voxels whatever
// its alignment), the highest bone index beyond kFocal is a wave reduction, the line is written once. A longer line is read a second time.
// 2048 workgroups stride over the lines, and the two counts go lanes -> wave -> workgroup -> one atomic pair: with a wave per line and a pair per
// wave, the 400,000 atomics on two addresses took 2.4 ms at head size, fifty times the copy.
// No kernel waits for another workgroup; every loop is bounded, see the comment at each.
#include <float.h>
#include <string.h>
#include "bfd_internal.h"
#include "bfd_call.h"
#include "bfd_tissue_core.h"

namespace {

constexpr int THREADS = 256;
// what the text of every data refusal of bfd_quantize_values3d carries after the entry's name (include/babelfdtd.h; TissueMask.py turns these into ValueError)
const char *const DATA_REFUSED = ": refused data: ";
constexpr int64_t SWEEP_BLOCKS = 2048;            // the passes over the volume: what lies beyond is taken by a grid-stride loop
constexpr int TABLE_THREADS = 1024;               // one per chunk of 64 levels at 16 bits
constexpr int RANK_LDS_BITS = 12;                 // ranks of up to 2^12 levels (8 KiB) are staged in LDS; measured: 64 KiB at 15 bits lost to global reads at 16
constexpr int LINE_WORDS = 4;                     // words of a line a lane keeps in registers: 64 * 4 * 4 - 3 = 1021 voxels fit at any alignment
constexpr int64_t LINE_BLOCKS = 2048;             // a wave takes many lines, so that the two counts cost one atomic pair per workgroup

static_assert((1 << TQ_MAX_BITS) / TQ_CHUNK <= TABLE_THREADS, "one thread per chunk");

// ---------------------------------------------------------------- quantisation ----------------------------------------------------------------

// keys[0] = the smallest key under the mask, keys[1] = the largest; they start as 0xFFFFFFFF and 0
__global__ __launch_bounds__(THREADS) void tq_minmax(const float4 *__restrict__ values, const uint32_t *__restrict__ mask, int64_t quads,
                                                     uint32_t *__restrict__ keys)
{
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * THREADS) {         // grid-stride: ends
        const uint32_t m = mask[q];
        if (!m) continue;
        const float4 x = values[q];
        const float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int b = 0; b < 4; b++)
            if ((m >> (8 * b)) & 0xFFu) {
                const uint32_t key = tq_key(__float_as_uint(e[b]));
                lo = key < lo ? key : lo;
                hi = key > hi ? key : hi;
            }
    }
    for (int d = 32; d >= 1; d >>= 1) {               // every lane arrives here: the loop above has no early exit from the kernel
        const uint32_t l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) { atomicMin(keys, lo); atomicMax(keys + 1, hi); }
}

// presence: tq_presence_words(bits) words, zero before the launch
__global__ __launch_bounds__(THREADS) void tq_presence(const float4 *__restrict__ values, const uint32_t *__restrict__ mask, int64_t quads,
                                                       const tq_params p, int words, uint32_t *__restrict__ presence)
{
    extern __shared__ uint32_t seen[];
    for (int w = threadIdx.x; w < words; w += THREADS) seen[w] = 0;
    __syncthreads();
    for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * THREADS) {         // grid-stride: ends
        const uint32_t m = mask[q];
        if (!m) continue;
        const float4 x = values[q];
        const float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int b = 0; b < 4; b++)
            if ((m >> (8 * b)) & 0xFFu) {
                const int l = tq_level(p, e[b]);      // 0 .. M: inside the bitmap
                const uint32_t bit = 1u << (l & 31);
                if (!(seen[l >> 5] & bit)) atomicOr(&seen[l >> 5], bit);
            }
    }
    __syncthreads();
    for (int w = threadIdx.x; w < words; w += THREADS)
        if (seen[w]) atomicOr(presence + w, seen[w]);
}

// inclusive scan of one int per thread over the workgroup: OP = max or +. Ends after log2(TABLE_THREADS) rounds.
template <bool MAX>
static __device__ int block_scan(int *sc, int mine)
{
    const int t = threadIdx.x;
    sc[t] = mine;
    __syncthreads();
    for (int d = 1; d < TABLE_THREADS; d <<= 1) {
        const int other = t >= d ? sc[t - d] : (MAX ? -1 : 0);
        __syncthreads();
        mine = MAX ? (other > mine ? other : mine) : mine + other;
        sc[t] = mine;
        __syncthreads();
    }
    return mine;
}

__global__ __launch_bounds__(TABLE_THREADS) void tq_table(const uint32_t *__restrict__ presence, const tq_params p, int chunks, float *__restrict__ table,
                                                          uint16_t *__restrict__ rank, int *__restrict__ rows)
{
    __shared__ int sc[TABLE_THREADS];
    const int t = threadIdx.x;
    const bool live = t < chunks;
    block_scan<true>(sc, live ? tq_chunk_last(presence, t) : -1);
    const int prev = t > 0 ? sc[t - 1] : -1;
    __syncthreads();
    block_scan<false>(sc, live ? tq_chunk_rows(p, presence, t, prev, 0, nullptr, nullptr) : 0);
    const int base = t > 0 ? sc[t - 1] : 0;
    if (live) tq_chunk_rows(p, presence, t, prev, base, table, rank);
    if (t == TABLE_THREADS - 1) rows[0] = sc[t];
}

// LDS: the ranks are copied to LDS first (levels * 2 bytes of dynamic shared memory)
template <bool LDS>
__global__ __launch_bounds__(THREADS) void tq_apply(const float4 *__restrict__ values, const uint32_t *__restrict__ mask, int64_t quads, const tq_params p,
                                                    const uint16_t *__restrict__ rank, int levels, float4 *__restrict__ quantized, uint4 *__restrict__ map)
{
    extern __shared__ uint16_t staged[];
    const uint16_t *rk = rank;
    if (LDS && map) {
        for (int l = threadIdx.x; l < levels; l += THREADS) staged[l] = rank[l];
        __syncthreads();
        rk = staged;
    }
    for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * THREADS) {         // grid-stride: ends
        const uint32_t m = mask[q];
        uint32_t r[4] = {0, 0, 0, 0};
        if (m || quantized) {
            const float4 x = values[q];
            float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int b = 0; b < 4; b++)
                if ((m >> (8 * b)) & 0xFFu) {
                    const int l = tq_level(p, e[b]);  // 0 .. M: inside the rank table
                    e[b] = tq_value(p, l);
                    if (map) r[b] = rk[l];
                }
            if (quantized) quantized[q] = make_float4(e[0], e[1], e[2], e[3]);
        }
        if (map) map[q] = make_uint4(r[0], r[1], r[2], r[3]);
    }
}

// ---------------------------------------------------------------- cleanup ----------------------------------------------------------------

struct line_args { int64_t lines; int N3, kFocal, boneA, boneB, from, to; };

// the highest k > kFocal of the word's four voxels that is bone, or -1. k0: the line index of the word's byte 0 (may be negative: the voxels of the
// line before, which share the word, are not looked at)
static __device__ __forceinline__ int line_bone(uint32_t w, int k0, const line_args &a)
{
    int hi = -1;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int k = k0 + b, x = (int)((w >> (8 * b)) & 0xFFu);
        if (k > a.kFocal && k < a.N3 && (x == a.boneA || x == a.boneB)) hi = k;
    }
    return hi;
}

// writes the voxels of the word that belong to the line: `from` beyond kb becomes `to` (kb < 0: none). Whole words where all four do, else bytes:
// the word is shared with a neighbouring line, which another wave writes
static __device__ __forceinline__ int line_store(uint32_t w, int k0, int kb, const line_args &a, uint8_t *dst)
{
    int changed = 0;
    uint32_t o = w;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int k = k0 + b, x = (int)((w >> (8 * b)) & 0xFFu);
        if (kb >= 0 && k > kb && k < a.N3 && x == a.from) {
            o = (o & ~(0xFFu << (8 * b))) | ((uint32_t)a.to << (8 * b));
            changed++;
        }
    }
    if (k0 >= 0 && k0 + 3 < a.N3) *(uint32_t *)dst = o;
    else {
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (k0 + b >= 0 && k0 + b < a.N3) dst[b] = (uint8_t)(o >> (8 * b));
    }
    return changed;
}

// in, out: the volumes, 4-byte aligned and padded to whole words. acc[0] = lines with bone beyond kFocal, acc[1] = voxels changed
__global__ __launch_bounds__(THREADS) void clear_beyond_bone(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const line_args a,
                                                             unsigned long long *__restrict__ acc)
{
    const int lane = threadIdx.x & 63;
    const uint32_t *words = (const uint32_t *)in;
    int withBone = 0, changed = 0;
    // grid-stride over lines, wave-uniform: ends after ceil(lines / (4 gridDim)) rounds
    for (int64_t line = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6); line < a.lines; line += (int64_t)gridDim.x * (THREADS / 64)) {
        const int64_t start = line * a.N3, w0 = start >> 2;
        const int off = (int)(start & 3);                           // the line begins at byte `off` of word w0
        const int nW = (off + a.N3 + 3) >> 2;                       // words that hold a voxel of the line; the last lies inside the padded volume
        uint32_t reg[LINE_WORDS];
        int hi = -1;
#pragma unroll
        for (int q = 0; q < LINE_WORDS; q++) {
            const int wi = q * 64 + lane;
            reg[q] = wi < nW ? words[w0 + wi] : 0u;
            if (wi < nW) { const int h = line_bone(reg[q], 4 * wi - off, a); hi = h > hi ? h : hi; }
        }
        for (int wi = LINE_WORDS * 64 + lane; wi < nW; wi += 64) {  // a line beyond the resident length: ends, wi grows
            const int h = line_bone(words[w0 + wi], 4 * wi - off, a);
            hi = h > hi ? h : hi;
        }
        for (int d = 32; d >= 1; d >>= 1) { const int h = __shfl_xor(hi, d); hi = h > hi ? h : hi; }      // the whole wave is here: the trip counts are wave-uniform
        if (lane == 0 && hi >= 0) withBone++;
#pragma unroll
        for (int q = 0; q < LINE_WORDS; q++) {
            const int wi = q * 64 + lane;
            if (wi < nW) changed += line_store(reg[q], 4 * wi - off, hi, a, out + 4 * (w0 + wi));
        }
        for (int wi = LINE_WORDS * 64 + lane; wi < nW; wi += 64)    // the second read
            changed += line_store(words[w0 + wi], 4 * wi - off, hi, a, out + 4 * (w0 + wi));
    }
    // the counts: lanes -> wave -> workgroup -> one atomic pair. Every wave arrives here: the loops above have no early exit from the kernel
    __shared__ int part[2][THREADS / 64];
    for (int d = 32; d >= 1; d >>= 1) changed += __shfl_xor(changed, d);
    if (lane == 0) { part[0][threadIdx.x >> 6] = withBone; part[1][threadIdx.x >> 6] = changed; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = 0, c = 0;
        for (int w = 0; w < THREADS / 64; w++) { b += (unsigned long long)part[0][w]; c += (unsigned long long)part[1][w]; }
        if (b || c) { atomicAdd(acc, b); atomicAdd(acc + 1, c); }
    }
}

}  // namespace

extern "C" int bfd_quantize_values3d(int device, const float *values, const uint8_t *mask, int64_t N1, int64_t N2, int64_t N3, int bits, float *quantized,
                                     uint32_t *map, float *table, int64_t *numValues, float *range, float *kernelMs)
{
    static const char *who = "bfd_quantize_values3d";
    // every argument error is reported before a device is looked for
    if (!values || !mask || !table || !numValues || !range) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (N1 < 0 || N2 < 0 || N3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (!volume_fits(N1, N2, N3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    if (bits < 1 || bits > TQ_MAX_BITS) BFD_FAIL(-1, std::string(who) + ": bits must be 1 .. 16");
    const size_t n = (size_t)(N1 * N2 * N3);
    if (n && ((quantized && (overlap(values, 4 * n, quantized, 4 * n) || overlap(mask, n, quantized, 4 * n))) ||
              (map && (overlap(values, 4 * n, map, 4 * n) || overlap(mask, n, map, 4 * n))) || (quantized && map && overlap(quantized, 4 * n, map, 4 * n))))
        BFD_FAIL(-1, std::string(who) + ": an output may not alias an input or another output");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "the mask is empty: there is no range to quantise");

    const int64_t quads = ((int64_t)n + 3) / 4;
    const size_t np = (size_t)quads * 4;              // the device volumes are padded to whole quads; the mask's padding is 0
    const int levels = 1 << bits, words = tq_presence_words(bits);
    DevTemp<float> dval, dq, dtable;
    DevTemp<uint8_t> dmask;
    DevTemp<uint32_t> dmap, dkeys, dpres;
    DevTemp<uint16_t> drank;
    DevTemp<int> drows;
    Events ev;
    float ms1 = 0.f, ms2 = 0.f;
    uint32_t keys[2] = {0xFFFFFFFFu, 0u};
    int rows = 0;
    BFD_STEP(dval.alloc(np));
    BFD_STEP(dmask.alloc(np));
    if (quantized) BFD_STEP(dq.alloc(np));
    if (map) BFD_STEP(dmap.alloc(np));
    BFD_STEP(dtable.alloc((size_t)levels));
    BFD_STEP(drank.alloc((size_t)levels));
    BFD_STEP(dkeys.alloc(2));
    BFD_STEP(dpres.alloc((size_t)words));
    BFD_STEP(drows.alloc(1));
    if (np > n) {
        BFD_STEP(hipMemset(dmask.p + (np - 4), 0, 4));
        BFD_STEP(hipMemset(dval.p + (np - 4), 0, 16));
    }
    BFD_STEP(hipMemset(dpres, 0, (size_t)words * 4));
    BFD_STEP(hipMemset(drank, 0, (size_t)levels * 2));
    BFD_STEP(hipMemcpy(dval, values, 4 * n, hipMemcpyHostToDevice));
    BFD_STEP(hipMemcpy(dmask, mask, n, hipMemcpyHostToDevice));
    BFD_STEP(hipMemcpy(dkeys, keys, sizeof keys, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    const unsigned blocks = blocks_for(quads, THREADS, SWEEP_BLOCKS);
    BFD_STEP(ev.record(0));
    hipLaunchKernelGGL(tq_minmax, dim3(blocks), dim3(THREADS), 0, 0, (const float4 *)dval.p, (const uint32_t *)dmask.p, quads, dkeys.p);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(&ms1, 0, 1));
    // the range decides whether there is anything to quantise: the two keys are what the host needs between the kernels
    BFD_STEP(hipMemcpy(keys, dkeys, sizeof keys, hipMemcpyDeviceToHost));
    if (keys[0] == 0xFFFFFFFFu && keys[1] == 0u) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "the mask is empty: there is no range to quantise");
    if (keys[0] <= TQ_KEY_NEG_INF || keys[1] >= TQ_KEY_POS_INF) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "a value under the mask is not finite");
    float mn, mx;
    const uint32_t bmn = tq_unkey(keys[0]), bmx = tq_unkey(keys[1]);
    memcpy(&mn, &bmn, 4);
    memcpy(&mx, &bmx, 4);
    const float A = mx - mn;
    if (!(A <= FLT_MAX)) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "max - min under the mask is not finite in float32");
    if (A < FLT_MIN) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "max - min under the mask is zero (or a denormal): there is one level only");
    const tq_params p = tq_make(mn, mx, bits);
    if (p.r < FLT_MIN) BFD_FAIL(-1, std::string(who) + DATA_REFUSED + "the step (max - min) / (2^bits - 1) is below 2^-126");

    BFD_STEP(ev.record(0));
    hipLaunchKernelGGL(tq_presence, dim3(blocks), dim3(THREADS), (size_t)words * 4, 0, (const float4 *)dval.p, (const uint32_t *)dmask.p, quads, p, words, dpres.p);
    hipLaunchKernelGGL(tq_table, dim3(1), dim3(TABLE_THREADS), 0, 0, dpres.p, p, tq_chunks(bits), dtable.p, drank.p, drows.p);
    if (quantized || map) {
        if (bits <= RANK_LDS_BITS)
            hipLaunchKernelGGL(tq_apply<true>, dim3(blocks), dim3(THREADS), map ? (size_t)levels * 2 : 0, 0, (const float4 *)dval.p, (const uint32_t *)dmask.p, quads, p,
                               drank.p, levels, (float4 *)dq.p, (uint4 *)dmap.p);
        else
            hipLaunchKernelGGL(tq_apply<false>, dim3(blocks), dim3(THREADS), 0, 0, (const float4 *)dval.p, (const uint32_t *)dmask.p, quads, p, drank.p, levels,
                               (float4 *)dq.p, (uint4 *)dmap.p);
    }
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(&ms2, 0, 1));
    BFD_STEP(hipMemcpy(&rows, drows, sizeof rows, hipMemcpyDeviceToHost));
    if (rows < 1 || rows > levels) BFD_FAIL(-10, std::string(who) + ": the table builder returned a row count outside 1 .. 2^bits");
    BFD_STEP(hipMemcpy(table, dtable, (size_t)rows * 4, hipMemcpyDeviceToHost));
    if (quantized) BFD_STEP(hipMemcpy(quantized, dq, 4 * n, hipMemcpyDeviceToHost));
    if (map) BFD_STEP(hipMemcpy(map, dmap, 4 * n, hipMemcpyDeviceToHost));
    *numValues = rows;
    range[0] = mn; range[1] = mx;
    if (kernelMs) *kernelMs = ms1 + ms2;
    return 0;
}

extern "C" int bfd_clear_beyond_bone3d(int device, const uint8_t *in, uint8_t *out, int64_t N1, int64_t N2, int64_t N3, int64_t kFocal, int boneA, int boneB,
                                       int from, int to, int64_t *counts, float *kernelMs)
{
    static const char *who = "bfd_clear_beyond_bone3d";
    // every argument error is reported before a device is looked for
    if (!in || !out || !counts) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (N1 < 0 || N2 < 0 || N3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (!volume_fits(N1, N2, N3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    if (kFocal < 0 || kFocal >= N3) BFD_FAIL(-1, std::string(who) + ": kFocal must be an index of the last axis (0 <= kFocal < N3)");
    for (int x : {boneA, boneB, from, to})
        if (x < 0 || x > 255) BFD_FAIL(-1, std::string(who) + ": boneA, boneB, from and to must be uint8 values (0 .. 255)");
    const size_t n = (size_t)(N1 * N2 * N3);
    if (n && overlap(in, n, out, n)) BFD_FAIL(-1, std::string(who) + ": out may not alias in");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) { counts[0] = counts[1] = 0; return 0; }

    const size_t np = (n + 3) / 4 * 4;                // whole words: a line's last word may reach past the volume's last voxel
    line_args a;
    a.lines = N1 * N2; a.N3 = (int)N3; a.kFocal = (int)kFocal; a.boneA = boneA; a.boneB = boneB; a.from = from; a.to = to;
    DevTemp<uint8_t> din, dout;
    DevTemp<unsigned long long> acc;
    Events ev;
    unsigned long long r[2] = {0, 0};
    BFD_STEP(din.alloc(np));
    BFD_STEP(dout.alloc(np));
    BFD_STEP(acc.alloc(2));
    BFD_STEP(hipMemset(acc, 0, sizeof r));
    if (np > n) BFD_STEP(hipMemset(din.p + (np - 4), 0, 4));
    BFD_STEP(hipMemcpy(din, in, n, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    hipLaunchKernelGGL(clear_beyond_bone, dim3(blocks_for(a.lines, THREADS / 64, LINE_BLOCKS)), dim3(THREADS), 0, 0, din.p, dout.p, a, acc.p);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    BFD_STEP(hipMemcpy(r, acc, sizeof r, hipMemcpyDeviceToHost));
    BFD_STEP(hipMemcpy(out, dout, n, hipMemcpyDeviceToHost));
    counts[0] = (int64_t)r[0]; counts[1] = (int64_t)r[1];
    return 0;
}
