// 3-D median filter on MI355X: uint8 masks and float32 pressure maps, in the caller's numpy C order (k fastest).
//
// Replaces, in the pipeline around the solver calls,
//     scipy.ndimage.median_filter(pAmp, 3)                      ThermalModeling/CalculateTemperatureEffects.py:908-918  (Step 3, float32)
//     MedianFilter.MedianFilter(data, size, GPUBackend=...)     BabelBrain/BabelDatasetPreps.py:870-876, 1050-1053, 1069-1072 (Step 1, uint8,
//                                                               sizes 7 and 3; callback installed at CalculateMaskProcess.py:42-70)
//
//     out[i,j,k] = the element of rank n/2 (0-based, ascending) of the s1 x s2 x s3 window centred on (i,j,k), n = s1 s2 s3, s in {1,3,5,7}
//
// Scheme: one workgroup per 4 x 4 x 64 output tile (lanes along k), the tile and its halo in LDS as ORDER-PRESERVING INTEGER KEYS, and a
// radix select per voxel: from the highest bit down, count the window's keys that agree with the bits chosen so far and have a 0 at this
// bit; the rank says whether the median is among them. No private array, no sort, no float comparison: the output is the key found, turned
// back into the input's bits -- one of the window's values, denormals included (a float min / max network would flush them in this build).
//   uint8: the key is the value. float32: bits ^ 0x80000000 for positive numbers, ~bits for negative ones (-0.0 sorts just below +0.0;
//   either may come out where both lie in a window). NaN: undefined (a NaN is ordered by its bits, beyond the infinities; numpy and scipy
//   do something else).
// Rounds: the OR and the AND over the tile INCLUDING ITS HALO (and the constant-mode fill) are workgroup-uniform; only the bits where
// they differ can differ between two keys of any window of the tile, so only those get a round: a 0/1 mask takes one round, labels 0-5
// three, a full-range uint8 volume eight, float32 as many bits as the tile's values differ in (at most 32).
// Bound: LDS read issue together with the vector ALU (one ds_read and three VALU operations per window element and round); HBM traffic
// (2-8 B per voxel) and the halo re-reads (through L2) are negligible beside 27-343 LDS reads per voxel and round. DESIGN.md, "Median filter".
#include "bfd_internal.h"
#include "bfd_call.h"
#include "bfd_thermal_stages.h"
#include <math.h>
#include <string.h>
#include <algorithm>

namespace {

constexpr int MT_I = 4, MT_J = 4, MT_K = 64;      // output tile: MT_J x MT_K threads, every thread MT_I voxels
constexpr int MT_THREADS = MT_J * MT_K;
constexpr int MR_MAX = 3;                         // largest radius (size 7)
constexpr long MAX_BLOCKS = 1L << 20;             // tiles beyond this are taken by a grid-stride loop

struct median_args {
    int N1, N2, N3;
    int r1, r2, r3;          // window radii per axis
    int mode;                // 0 reflect, 1 constant
    unsigned cvalKey;        // key of cval (constant mode)
    int nTk, nTj;            // tiles along k and j
    long nTiles;
};

// T = uint8_t: the value is its key. T = uint32_t: the bits of a float32; the key orders them as the numbers are ordered.
static __device__ __forceinline__ unsigned key_enc(uint8_t v) { return v; }
static __device__ __forceinline__ unsigned key_enc(uint32_t u) { return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
static __device__ __forceinline__ void key_dec(unsigned k, uint8_t *v) { *v = (uint8_t)k; }
static __device__ __forceinline__ void key_dec(unsigned k, uint32_t *u) { *u = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// scipy's 'reflect' (d c b a | a b c d | d c b a); every dimension is at least the radius, so one reflection reaches every cell a
// written output reads. Cells further out (only a partial tile's unwritten outputs read them) are clamped into the volume.
static __device__ __forceinline__ int reflect_index(int g, int N)
{
    if (g < 0) g = -1 - g;
    else if (g >= N) g = 2 * N - 1 - g;
    return min(max(g, 0), N - 1);
}

// R >= 0: cubic window of radius R, loops unrolled; R < 0: radii from the arguments (mixed sizes, size 1)
template <typename T, int R>
__global__ __launch_bounds__(MT_THREADS) void median3d(const T *__restrict__ in, T *__restrict__ out, const uint8_t *__restrict__ mask,
                                                       const median_args p)
{
    constexpr bool FIXED = R >= 0;
    constexpr int RM = FIXED ? R : MR_MAX;
    constexpr int UNROLL = FIXED ? 2 * R + 1 : 1;         // the two inner window loops: whole for a fixed radius
    __shared__ T tile[(MT_I + 2 * RM) * (MT_J + 2 * RM) * (MT_K + 2 * RM)];       // keys; uint8: 7,000 B, float32: 28,000 B at radius 3
    __shared__ unsigned red[2][MT_J];
    const int r1 = FIXED ? R : p.r1, r2 = FIXED ? R : p.r2, r3 = FIXED ? R : p.r3;
    const int W1 = MT_I + 2 * r1, W2 = MT_J + 2 * r2, W3 = MT_K + 2 * r3;
    const int lane = threadIdx.x & (MT_K - 1), tj = threadIdx.x / MT_K;
    const unsigned rank0 = (unsigned)((2 * r1 + 1) * (2 * r2 + 1) * (2 * r3 + 1)) / 2u;

    for (long t = blockIdx.x; t < p.nTiles; t += gridDim.x) {
        const int bk = (int)(t % p.nTk);
        const long q = t / p.nTk;
        const int bj = (int)(q % p.nTj), bi = (int)(q / p.nTj);
        const int i0 = bi * MT_I, j0 = bj * MT_J, k0 = bk * MT_K;
        const int j = j0 + tj, k = k0 + lane;
        const bool inJK = j < p.N2 && k < p.N3;

        // which of this thread's voxels exist (bits 0..3) and which of them are filtered (bits 4..7)
        unsigned sel = 0;
#pragma unroll
        for (int ii = 0; ii < MT_I; ii++) {
            const int i = i0 + ii;
            if (inJK && i < p.N1) {
                const long lin = ((long)i * p.N2 + j) * p.N3 + k;
                sel |= 1u << ii;
                if (!mask || mask[lin]) sel |= 16u << ii;
            }
        }
        // the barrier also keeps this tile's LDS stores behind the reads of the tile before it
        const int any = __syncthreads_or((int)(sel >> 4));
        if (!any) {                           // no voxel of the tile lies in the region: copy and leave
#pragma unroll
            for (int ii = 0; ii < MT_I; ii++)
                if (sel & (1u << ii)) {
                    const long lin = ((long)(i0 + ii) * p.N2 + j) * p.N3 + k;
                    out[lin] = in[lin];
                }
            continue;
        }

        // ---- tile and halo into LDS as keys; OR and AND of all of them ----
        unsigned vo = 0u, va = 0xFFFFFFFFu;
        for (int rr = tj; rr < W1 * W2; rr += MT_J) {
            const int a = rr / W2, b = rr - a * W2;
            int gi = i0 - r1 + a, gj = j0 - r2 + b;
            bool okRow = true;
            if (p.mode == 0) { gi = reflect_index(gi, p.N1); gj = reflect_index(gj, p.N2); }
            else {
                okRow = gi >= 0 && gi < p.N1 && gj >= 0 && gj < p.N2;
                gi = min(max(gi, 0), p.N1 - 1); gj = min(max(gj, 0), p.N2 - 1);
            }
            const T *src = in + ((long)gi * p.N2 + gj) * p.N3;
            for (int c = lane; c < W3; c += MT_K) {
                int gk = k0 - r3 + c;
                bool ok = okRow;
                if (p.mode == 0) gk = reflect_index(gk, p.N3);
                else { ok = ok && gk >= 0 && gk < p.N3; gk = min(max(gk, 0), p.N3 - 1); }
                const unsigned key = ok ? key_enc(src[gk]) : p.cvalKey;
                tile[rr * W3 + c] = (T)key;
                vo |= key; va &= key;
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) { vo |= __shfl_xor(vo, s); va &= __shfl_xor(va, s); }
        if (lane == 0) { red[0][tj] = vo; red[1][tj] = va; }
        __syncthreads();
        unsigned orAll = 0u, andAll = 0xFFFFFFFFu;
#pragma unroll
        for (int w = 0; w < MT_J; w++) { orAll |= red[0][w]; andAll &= red[1][w]; }
        const unsigned diff = orAll ^ andAll;                 // the bits in which two keys of this tile can differ
        const int top = diff ? 31 - __clz((int)diff) : -1;

        // ---- radix select per voxel ----
#pragma unroll 1
        for (int ii = 0; ii < MT_I; ii++) {
            if (!(sel & (1u << ii))) continue;
            const long lin = ((long)(i0 + ii) * p.N2 + j) * p.N3 + k;
            unsigned prefix;
            if (sel & (16u << ii)) {
                prefix = andAll;                              // the bits all keys share; the differing bits are decided below, highest first
                unsigned rank = rank0;
                const T *w0 = tile + (ii * W2 + tj) * W3 + lane;
#pragma unroll 1
                for (int b = top; b >= 0; b--) {
                    if (!((diff >> b) & 1u)) continue;        // workgroup-uniform
                    const unsigned low = (1u << b) - 1u;      // (key ^ prefix) <= low: agrees on the bits above b, 0 at b
                    unsigned cnt = 0;
#pragma unroll 1
                    for (int a = 0; a <= 2 * r1; a++) {
                        const T *wa = w0 + a * W2 * W3;
#pragma unroll UNROLL
                        for (int bb = 0; bb <= 2 * r2; bb++) {
#pragma unroll UNROLL
                            for (int c = 0; c <= 2 * r3; c++)
                                cnt += (((unsigned)wa[bb * W3 + c] ^ prefix) <= low) ? 1u : 0u;
                        }
                    }
                    if (rank >= cnt) { rank -= cnt; prefix |= 1u << b; }
                }
            } else {
                prefix = tile[((ii + r1) * W2 + tj + r2) * W3 + lane + r3];      // outside the region: the input
            }
            T v;
            key_dec(prefix, &v);
            out[lin] = v;
        }
    }
}

template <typename T>
void launch_median(const T *in, T *out, const uint8_t *mask, const median_args &p, unsigned blocks)
{
    const bool cubic = p.r1 == p.r2 && p.r2 == p.r3;
    if (cubic && p.r1 == 1) hipLaunchKernelGGL((median3d<T, 1>), dim3(blocks), dim3(MT_THREADS), 0, 0, in, out, mask, p);
    else if (cubic && p.r1 == 2) hipLaunchKernelGGL((median3d<T, 2>), dim3(blocks), dim3(MT_THREADS), 0, 0, in, out, mask, p);
    else if (cubic && p.r1 == 3) hipLaunchKernelGGL((median3d<T, 3>), dim3(blocks), dim3(MT_THREADS), 0, 0, in, out, mask, p);
    else hipLaunchKernelGGL((median3d<T, -1>), dim3(blocks), dim3(MT_THREADS), 0, 0, in, out, mask, p);
}

}  // namespace

// The launch of bfd_median_filter3d on device pointers (bfd_thermal_stages.h): in and out are distinct volumes, cvalKey the border value as a key
hipError_t bfd_stage_median3d(int dtype, const void *in, void *out, const uint8_t *regionMask, int64_t N1, int64_t N2, int64_t N3, int s1, int s2, int s3,
                              int mode, unsigned cvalKey)
{
    median_args p;
    p.N1 = (int)N1; p.N2 = (int)N2; p.N3 = (int)N3;
    p.r1 = s1 / 2; p.r2 = s2 / 2; p.r3 = s3 / 2;
    p.mode = mode;
    p.cvalKey = cvalKey;
    p.nTk = (int)((N3 + MT_K - 1) / MT_K);
    p.nTj = (int)((N2 + MT_J - 1) / MT_J);
    p.nTiles = (long)p.nTk * p.nTj * ((N1 + MT_I - 1) / MT_I);
    const unsigned blocks = blocks_for(p.nTiles, 1, MAX_BLOCKS);
    if (dtype == 0) launch_median<uint8_t>((const uint8_t *)in, (uint8_t *)out, regionMask, p, blocks);
    else launch_median<uint32_t>((const uint32_t *)in, (uint32_t *)out, regionMask, p, blocks);
    return hipGetLastError();
}

extern "C" int bfd_median_filter3d(int device, int dtype, const void *in, void *out, const uint8_t *regionMask,
                                   int64_t N1, int64_t N2, int64_t N3, int s1, int s2, int s3, int mode, double cval, float *kernelMs)
{
    static const char *who = "bfd_median_filter3d";
    // every argument error is reported before a device is looked for
    if (dtype != 0 && dtype != 1) BFD_FAIL(-1, std::string(who) + ": dtype must be 0 (uint8) or 1 (float32)");
    if (!in || !out) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (in == out) BFD_FAIL(-1, std::string(who) + ": out may not alias in");
    if (mode != 0 && mode != 1) BFD_FAIL(-1, std::string(who) + ": mode must be 0 (reflect) or 1 (constant)");
    if (N1 < 0 || N2 < 0 || N3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    const int s[3] = {s1, s2, s3};
    const int64_t N[3] = {N1, N2, N3};
    for (int a = 0; a < 3; a++) {
        if (s[a] != 1 && s[a] != 3 && s[a] != 5 && s[a] != 7)
            BFD_FAIL(-1, std::string(who) + ": every size must be 1, 3, 5 or 7");
        if (N[a] < s[a] / 2)
            BFD_FAIL(-1, std::string(who) + ": axis " + std::to_string(a) + " has " + std::to_string(N[a]) + " elements, fewer than size / 2 = " +
                         std::to_string(s[a] / 2) + ": one reflection would not reach");
    }
    if (!volume_fits(N1, N2, N3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    const size_t n = (size_t)(N1 * N2 * N3);
    const size_t esz = dtype == 0 ? 1 : 4;
    if (overlap(in, n * esz, out, n * esz)) BFD_FAIL(-1, std::string(who) + ": out may not alias in");      // partial overlap of the two buffers
    unsigned cvalKey;
    if (dtype == 0) {
        if (!(cval >= 0.0 && cval <= 255.0) || cval != floor(cval)) BFD_FAIL(-1, std::string(who) + ": cval is not a uint8 value");
        cvalKey = (unsigned)cval;
    } else {
        const float f = (float)cval;
        uint32_t u;
        memcpy(&u, &f, 4);
        cvalKey = u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    }

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) return 0;

    DevTemp<char> din, dout;
    DevTemp<uint8_t> dmask;
    Events ev;
    BFD_STEP(din.alloc(n * esz));
    BFD_STEP(dout.alloc(n * esz));
    if (regionMask) BFD_STEP(dmask.alloc(n));
    BFD_STEP(hipMemcpy(din, in, n * esz, hipMemcpyHostToDevice));
    if (regionMask) BFD_STEP(hipMemcpy(dmask, regionMask, n, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    BFD_STEP(bfd_stage_median3d(dtype, din.p, dout.p, dmask, N1, N2, N3, s1, s2, s3, mode, cvalKey));
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    BFD_STEP(hipMemcpy(out, dout, n * esz, hipMemcpyDeviceToHost));
    return 0;
}
