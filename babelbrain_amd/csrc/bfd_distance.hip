// Exact Euclidean distance transform and Gaussian filter of Step-1 volumes on MI355X, in the caller's numpy C order (k fastest).
//
// Replace, in the bone-rim partial-volume correction of BabelBrain/BabelDatasetPreps.py:936-1017 (bMaximizeBoneRim),
//     ndimage.distance_transform_edt(inv_interior)                 :967   -> bfd_distance_transform_edt3d (flag "invert" spares the 1 - mask pass of :964)
//     ndimage.gaussian_filter(volume, sigma=sigma_local)           :984, :986 (float32)   -> bfd_gaussian_filter3d
// The arithmetic of both is in bfd_distance_core.h, which a plain C++ compiler accepts too (tests/test_distance_host.py runs it serially on the CPU).
//
// Distance transform: exact and separable, integers throughout (squared distances int32, intersections of parabolas by integer division).
//   pack     one wave per 64 voxels of a row: a ballot turns them into one word of the bit-packed mask (bit set = background), rows padded to 64
//   rows     one lane per voxel: nearest background voxel of its own row from the leading / trailing zero counts of its word, the words beyond
//            walked where its half of the word is empty; squared, or EDT_NONE for a row without background (compared in the later passes, never added)
//   lines    along j, then along i: the lower envelope of the parabolas f(q) + (p - q)^2 of a line, Meijster's two scans. ONE LANE PER LINE, lanes
//            along k: every load and store of a wave is one contiguous 256-byte segment. The per-line stacks (site, start of its interval, value:
//            8 B an entry, as many entries as the line is long) do not fit in LDS; they live in a device scratch volume laid out
//            [position][line], so lanes of a wave that stand at the same depth read and write them coalesced. In place: a lane reads its whole line
//            before it writes any of it.
//   root     float64 square root of the int32, into the scratch volume (which the stacks no longer need)
// Device memory: the mask (1 B per voxel), its bits, 4 B per voxel for the squared distances and 8 B per voxel of scratch (stacks, then roots).
// Bound: the line passes are latency bound, not bandwidth bound -- a lane walks its line serially, twice.
//
// Gaussian filter: axes 0, 1, 2 in turn, each pass float64 sums rounded once to the volume's dtype, between two device volumes.
//   axis 2      a wave stages 64 outputs' row segment and its halo of r on either side in LDS as float64 (edge rule applied while staging, for any
//               ratio of r to the axis length) and every lane takes its 2 r + 1 taps from there
//   axes 0, 1   lanes along k (axis 0: along the flattened (j, k), which is contiguous); a workgroup stages a tile of (T + 2 r) x 64 samples in LDS in
//               the volume's dtype, the edge rule applied per tile row, and produces T x 64 outputs; T = what 48 KB of LDS leave beside the halo.
//               Where that is fewer than GAUSS_MIN_T rows (r above 88 for float32, above 40 for float64) the taps are read from global memory
//               instead (gauss_direct: the same sums, L2 takes the re-reads).
//   The weights are a kernel argument block (128 float64). No contraction (-ffp-contract=off); scipy's order of the sum (gauss_sum).
#include "bfd_internal.h"
#include "bfd_call.h"
#include "bfd_distance_core.h"
#include "bfd_step1_stages.h"
#include <math.h>
#include <string.h>
#include <algorithm>

namespace {

constexpr int THREADS = 256;
constexpr int64_t MAX_BLOCKS = 1 << 20;           // what lies beyond is taken by a grid-stride loop

// ------------------------------------------------------------ distance transform ------------------------------------------------------------

// bits[row * W + w]: bit b set where voxel 64 w + b of the row is background. One wave per word.
__global__ __launch_bounds__(THREADS) void edt_pack(const uint8_t *__restrict__ in, uint64_t *__restrict__ bits, int64_t rows, int64_t N3, int64_t W,
                                                    int invert)
{
    const int lane = threadIdx.x & 63;
    const int64_t words = rows * W;
    for (int64_t item = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6); item < words; item += (int64_t)gridDim.x * (THREADS / 64)) {
        const int64_t row = item / W, k = (item - row * W) * 64 + lane;
        const bool bg = k < N3 && ((in[row * N3 + k] != 0) == (invert != 0));
        const unsigned long long word = __ballot(bg);
        if (lane == 0) bits[item] = word;
    }
}

__global__ __launch_bounds__(THREADS) void edt_rows(const uint64_t *__restrict__ bits, int32_t *__restrict__ f, int64_t n, int64_t N3, int64_t W)
{
    for (int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x; v < n; v += (int64_t)gridDim.x * THREADS) {
        const uint32_t row = (uint32_t)v / (uint32_t)N3;          // fewer than 2^31 voxels: 32-bit division
        f[v] = edt_row_dist2(bits + row * W, W, v - (int64_t)row * N3);
    }
}

// line L = outer * N3 + k starts at outer * outerStride + k and steps by elemStride; its stack is column L of [m][nLines]
__global__ __launch_bounds__(THREADS) void edt_lines(int32_t *__restrict__ f, edt_site *__restrict__ stack, int64_t nLines, int64_t N3,
                                                     int64_t outerStride, int64_t elemStride, int m)
{
    for (int64_t L = (int64_t)blockIdx.x * THREADS + threadIdx.x; L < nLines; L += (int64_t)gridDim.x * THREADS) {
        const int64_t outer = L / N3;
        edt_line(f + outer * outerStride + (L - outer * N3), elemStride, m, stack + L, nLines);
    }
}

__global__ __launch_bounds__(THREADS) void edt_root(const int32_t *__restrict__ f, double *__restrict__ d, int64_t n)
{
    for (int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x; v < n; v += (int64_t)gridDim.x * THREADS) d[v] = sqrt((double)f[v]);
}

// -------------------------------------------------------------- Gaussian filter --------------------------------------------------------------

constexpr int GAUSS_LDS_BYTES = 48 * 1024;        // the tile of the passes along axes 0 and 1
constexpr int GAUSS_MIN_T = 16;                   // fewer output rows per tile than this: gauss_direct
constexpr int GAUSS_SEG = 64;                     // outputs of a wave along axis 2

struct gauss_args {
    int64_t outer, m, inner;      // the volume as [outer][m][inner], filtered along m
    int r, mode, T;
    double cval;
    double w[GAUSS_MAX_RADIUS + 1];
};

// axis 2 (inner == 1): item = (row, segment of 64)
template <typename T>
__global__ __launch_bounds__(THREADS) void gauss_last_axis(const T *__restrict__ in, T *__restrict__ out, const gauss_args p)
{
    __shared__ double seg[THREADS / 64][GAUSS_SEG + 2 * GAUSS_MAX_RADIUS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nSeg = (p.m + GAUSS_SEG - 1) / GAUSS_SEG, items = p.outer * nSeg;
    double *mine = seg[wave];
    for (int64_t base = (int64_t)blockIdx.x * (THREADS / 64); base < items; base += (int64_t)gridDim.x * (THREADS / 64)) {      // workgroup-uniform
        const int64_t item = base + wave;
        const bool live = item < items;
        const int64_t row = live ? item / nSeg : 0, k0 = live ? (item - row * nSeg) * GAUSS_SEG : 0;
        const T *line = in + row * p.m;
        if (live)
            for (int c = lane; c < GAUSS_SEG + 2 * p.r; c += 64) {
                const int64_t s = gauss_edge_index(k0 - p.r + c, p.m, p.mode);
                mine[c] = s < 0 ? p.cval : (double)line[s];
            }
        __syncthreads();
        if (live && k0 + lane < p.m) {
            const double *x0 = mine + p.r + lane;
            out[row * p.m + k0 + lane] = (T)gauss_sum([&](int d) { return x0[d]; }, p.w, p.r);
        }
        __syncthreads();          // the next item's stores stay behind these reads
    }
}

// axes 0 and 1: item = (outer, tile of T rows along m, 64 lanes along inner); 4 row groups of 64 lanes. CONSTANT = mode 1: a tile row may stand
// for cval (which need not be a value of the volume's dtype, so it is not stored in the tile)
template <typename T, bool CONSTANT>
__global__ __launch_bounds__(THREADS) void gauss_tiled(const T *__restrict__ in, T *__restrict__ out, const gauss_args p)
{
    constexpr int ROWS = GAUSS_LDS_BYTES / (64 * (int)sizeof(T));
    constexpr int GROUPS = THREADS / 64, BATCH = 12;      // rows a lane loads before it stores any: the loads of a batch are in flight together
    __shared__ T tile[ROWS][64];
    __shared__ int src[ROWS];                 // the row of the line that tile row t holds; -1: cval
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int64_t nX = (p.inner + 63) / 64, nU = (p.m + p.T - 1) / p.T, items = p.outer * nU * nX;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t bx = item % nX, q = item / nX, bu = q % nU, o = q / nU;
        const int64_t u0 = bu * p.T, x = bx * 64 + lane;
        const int nOut = p.m - u0 < p.T ? (int)(p.m - u0) : p.T, rows = nOut + 2 * p.r;
        const T *base = in + o * p.m * p.inner;
        for (int t = threadIdx.x; t < rows; t += THREADS) src[t] = (int)gauss_edge_index(u0 - p.r + t, p.m, p.mode);
        __syncthreads();
        if (x < p.inner)
            for (int t0 = grp; t0 < rows; t0 += GROUPS * BATCH) {
                T v[BATCH];
#pragma unroll
                for (int b = 0; b < BATCH; b++) {
                    const int t = t0 + GROUPS * b;
                    const int sr = t < rows ? src[t] : -1;
                    v[b] = sr >= 0 ? base[(int64_t)sr * p.inner + x] : (T)0;
                }
#pragma unroll
                for (int b = 0; b < BATCH; b++) {
                    const int t = t0 + GROUPS * b;
                    if (t < rows) tile[t][lane] = v[b];
                }
            }
        __syncthreads();
        if (x < p.inner)
            for (int t = grp; t < nOut; t += GROUPS) {
                const int c = t + p.r;
                const double s = CONSTANT ? gauss_sum([&](int d) { return src[c + d] < 0 ? p.cval : (double)tile[c + d][lane]; }, p.w, p.r)
                                          : gauss_sum([&](int d) { return (double)tile[c + d][lane]; }, p.w, p.r);
                out[(o * p.m + u0 + t) * p.inner + x] = (T)s;
            }
        __syncthreads();
    }
}

// any axis, any radius: one lane per output, taps from global memory
template <typename T>
__global__ __launch_bounds__(THREADS) void gauss_direct(const T *__restrict__ in, T *__restrict__ out, const gauss_args p)
{
    const int64_t n = p.outer * p.m * p.inner;
    for (int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x; v < n; v += (int64_t)gridDim.x * THREADS) {
        const int64_t x = v % p.inner, q = v / p.inner, u = q % p.m, o = q / p.m;
        const T *line = in + o * p.m * p.inner + x;
        out[v] = (T)gauss_sum([&](int d) {
            const int64_t s = gauss_edge_index(u + d, p.m, p.mode);
            return s < 0 ? p.cval : (double)line[s * p.inner];
        }, p.w, p.r);
    }
}

template <typename T>
void launch_gauss_axis(const T *in, T *out, gauss_args &p)
{
    if (p.inner == 1) {
        const int64_t items = p.outer * ((p.m + GAUSS_SEG - 1) / GAUSS_SEG);
        hipLaunchKernelGGL((gauss_last_axis<T>), dim3(blocks_for(items, THREADS / 64, MAX_BLOCKS)), dim3(THREADS), 0, 0, in, out, p);
        return;
    }
    const int rowsMax = GAUSS_LDS_BYTES / (64 * (int)sizeof(T));
    p.T = (int)std::min<int64_t>(rowsMax - 2 * p.r, (p.m + 3) / 4 * 4);
    if (rowsMax - 2 * p.r < GAUSS_MIN_T) {
        hipLaunchKernelGGL((gauss_direct<T>), dim3(blocks_for(p.outer * p.m * p.inner, THREADS, MAX_BLOCKS)), dim3(THREADS), 0, 0, in, out, p);
        return;
    }
    const int64_t items = p.outer * ((p.m + p.T - 1) / p.T) * ((p.inner + 63) / 64);
    if (p.mode == 1) hipLaunchKernelGGL((gauss_tiled<T, true>), dim3(blocks_for(items, 1, MAX_BLOCKS)), dim3(THREADS), 0, 0, in, out, p);
    else hipLaunchKernelGGL((gauss_tiled<T, false>), dim3(blocks_for(items, 1, MAX_BLOCKS)), dim3(THREADS), 0, 0, in, out, p);
}

}  // namespace

hipError_t bfd_stage_edt_squared(const uint64_t *background, int32_t *dist2, void *stack, int64_t N1, int64_t N2, int64_t N3)
{
    const int64_t n = N1 * N2 * N3, W = edt_row_words(N3);
    edt_site *st = (edt_site *)stack;
    hipLaunchKernelGGL(edt_rows, dim3(blocks_for(n, THREADS, MAX_BLOCKS)), dim3(THREADS), 0, 0, background, dist2, n, N3, W);
    hipLaunchKernelGGL(edt_lines, dim3(blocks_for(N1 * N3, THREADS, MAX_BLOCKS)), dim3(THREADS), 0, 0, dist2, st, N1 * N3, N3, N2 * N3, N3, (int)N2);
    hipLaunchKernelGGL(edt_lines, dim3(blocks_for(N2 * N3, THREADS, MAX_BLOCKS)), dim3(THREADS), 0, 0, dist2, st, N2 * N3, N3, N3, N2 * N3, (int)N1);
    return hipGetLastError();
}

hipError_t bfd_stage_gaussian3d(int dtype, void *a, void *b, int64_t N1, int64_t N2, int64_t N3, const double *sigma, const int *radius, int mode,
                                double cval, void **result)
{
    const int64_t N[3] = {N1, N2, N3};
    void *src = a, *dst = b;
    for (int ax = 0; ax < 3; ax++) {
        if (!(sigma[ax] > 1e-15)) continue;           // scipy skips the axis
        gauss_args p;
        p.outer = ax == 0 ? 1 : (ax == 1 ? N1 : N1 * N2);
        p.m = N[ax];
        p.inner = ax == 0 ? N2 * N3 : (ax == 1 ? N3 : 1);
        p.r = radius[ax]; p.mode = mode; p.T = 0; p.cval = cval;
        memset(p.w, 0, sizeof p.w);
        gauss_weights(sigma[ax], p.r, p.w);
        if (dtype == 1) launch_gauss_axis<float>((const float *)src, (float *)dst, p);
        else launch_gauss_axis<double>((const double *)src, (double *)dst, p);
        std::swap(src, dst);
    }
    *result = src;
    return hipGetLastError();
}

extern "C" int bfd_distance_transform_edt3d(int device, const uint8_t *in, int flags, int32_t *dist2, double *dist, int64_t N1, int64_t N2, int64_t N3,
                                            float *kernelMs)
{
    static const char *who = "bfd_distance_transform_edt3d";
    // every argument error is reported before a device is looked for
    if (!in) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (!dist2 && !dist) BFD_FAIL(-1, std::string(who) + ": at least one output (dist2, dist) must be asked for");
    if (flags & ~1) BFD_FAIL(-1, std::string(who) + ": unknown bits in flags (bit 0: invert)");
    if (N1 < 0 || N2 < 0 || N3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (N1 > EDT_MAX_DIM || N2 > EDT_MAX_DIM || N3 > EDT_MAX_DIM)
        BFD_FAIL(-1, std::string(who) + ": every dimension must be at most 16384 (the squared distances are int32)");
    if (!volume_fits(N1, N2, N3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    const size_t n = (size_t)(N1 * N2 * N3);
    if ((dist2 && overlap(in, n, dist2, n * 4)) || (dist && overlap(in, n, dist, n * 8)) || (dist2 && dist && overlap(dist2, n * 4, dist, n * 8)))
        BFD_FAIL(-1, std::string(who) + ": the outputs may not overlap the input or each other");
    const int invert = flags & 1;
    if (n) {
        bool any = false;
        if (invert) { for (size_t v = 0; v < n && !any; v++) any = in[v] != 0; }
        else any = memchr(in, 0, n) != nullptr;
        if (!any) BFD_FAIL(-1, std::string(who) + ": the volume has no background voxel: there is no distance to take");
    }

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) return 0;

    const int64_t rows = N1 * N2, W = edt_row_words(N3);
    DevTemp<uint8_t> din;
    DevTemp<uint64_t> dbits;
    DevTemp<int32_t> df;
    DevTemp<edt_site> dscratch;               // the stacks of the line passes, then the roots: 8 B per voxel either way
    Events ev;
    static_assert(sizeof(edt_site) == sizeof(double), "the scratch volume holds stack entries, then float64 roots");
    BFD_STEP(din.alloc(n));
    BFD_STEP(dbits.alloc((size_t)(rows * W)));
    BFD_STEP(df.alloc(n));
    BFD_STEP(dscratch.alloc(n));
    BFD_STEP(hipMemcpy(din, in, n, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    hipLaunchKernelGGL(edt_pack, dim3(blocks_for(rows * W, THREADS / 64, MAX_BLOCKS)), dim3(THREADS), 0, 0, din.p, dbits.p, rows, N3, W, invert);
    BFD_STEP(bfd_stage_edt_squared(dbits.p, df.p, dscratch.p, N1, N2, N3));
    if (dist) hipLaunchKernelGGL(edt_root, dim3(blocks_for((int64_t)n, THREADS, MAX_BLOCKS)), dim3(THREADS), 0, 0, df.p, (double *)dscratch.p, (int64_t)n);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    if (dist2) BFD_STEP(hipMemcpy(dist2, df, n * 4, hipMemcpyDeviceToHost));
    if (dist) BFD_STEP(hipMemcpy(dist, dscratch, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int bfd_gaussian_filter3d(int device, int dtype, const void *in, void *out, int64_t N1, int64_t N2, int64_t N3, const double *sigma,
                                     double truncate, int mode, double cval, float *kernelMs)
{
    static const char *who = "bfd_gaussian_filter3d";
    // every argument error is reported before a device is looked for
    if (dtype != 1 && dtype != 3) BFD_FAIL(-1, std::string(who) + ": dtype must be 1 (float32) or 3 (float64)");
    if (!in || !out || !sigma) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (mode < 0 || mode > 3) BFD_FAIL(-1, std::string(who) + ": mode must be 0 (reflect), 1 (constant), 2 (nearest) or 3 (mirror)");
    if (N1 < 0 || N2 < 0 || N3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (!volume_fits(N1, N2, N3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    if (!(truncate >= 0.0) || !std::isfinite(truncate)) BFD_FAIL(-1, std::string(who) + ": truncate must be finite and not negative");
    int radius[3];
    for (int a = 0; a < 3; a++) {
        if (!(sigma[a] >= 0.0) || !std::isfinite(sigma[a])) BFD_FAIL(-1, std::string(who) + ": every sigma must be finite and not negative");
        radius[a] = sigma[a] > 1e-15 ? gauss_radius(sigma[a], truncate) : 0;
        if (radius[a] < 0)
            BFD_FAIL(-1, std::string(who) + ": the radius int(truncate sigma + 0.5) of axis " + std::to_string(a) + " is above " + std::to_string(GAUSS_MAX_RADIUS));
    }
    const size_t n = (size_t)(N1 * N2 * N3);
    const size_t esz = dtype == 1 ? 4 : 8;
    if (overlap(in, n * esz, out, n * esz)) BFD_FAIL(-1, std::string(who) + ": out may not overlap in");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) return 0;

    DevTemp<char> da, db;
    Events ev;
    BFD_STEP(da.alloc(n * esz));
    BFD_STEP(db.alloc(n * esz));
    BFD_STEP(hipMemcpy(da, in, n * esz, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    void *src = da.p;
    BFD_STEP(bfd_stage_gaussian3d(dtype, da.p, db.p, N1, N2, N3, sigma, radius, mode, cval, &src));
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    BFD_STEP(hipMemcpy(out, src, n * esz, hipMemcpyDeviceToHost));      // all three axes skipped: the input
    return 0;
}
