// Spline resampling of 3-D volumes under an affine map on MI355X: scipy.ndimage.affine_transform / spline_filter for orders 0-3, modes
// constant, nearest and mirror, dtypes uint8, int16, float32, float64, in the caller's numpy C order (k fastest).
//
// Replaces, behind GPUFunctions/GPUResample/Resample.py::ResampleFromTo (callback installed at BabelBrain/CalculateMaskProcess.py:65-74),
//     nibabel.processing.resample_from_to(CT, mask grid, order=3, cval=min)     BabelDatasetPreps.py:859
//     ... (T1, mask grid, order=0)                                               BabelDatasetPreps.py:1168
//     ... fixed image of the CT co-registration                                  CTZTEProcessing.py:258
//
// Everything is float64 (coordinates, weights, sums, the coefficient volume) and rounded once, at the store, as scipy does; the arithmetic itself
// is bfd_resample_core.h, which a host program can call as well. The file is compiled with -ffp-contract=off like the rest of the library.
//   prefilter (orders 2, 3): input -> float64 (edge-padded by 12 per side for 'nearest'), then one recursive pass pair per axis in place.
//     axes 0 and 1: a lane per line, lanes along k, so every load and store of a wave is one contiguous run (prefilter_strided).
//     axis 2: the lines of a block are contiguous in memory (64 lines x N3); 64 x 32 tiles go through LDS, loaded and stored along k, and each
//     lane carries the recursion of its line from tile to tile, forwards for the causal pass and backwards for the anti-causal one (prefilter_k).
//   interpolation: one output voxel per lane, lanes along the output's k; the (order + 1)^3 coefficients are gathered from global memory
//     (interp3d). Order 3 (interp3d_staged): a workgroup takes a 4 x 8 x 32 output tile and, where the tile's source box holds at most ST_CAP
//     coefficients (every near-unit-scale map), stages the box in LDS once, boundary rule applied; 64 LDS reads per voxel replace 64 gathers.
//     Same arithmetic, same bits. Larger boxes, and voxels whose taps leave the box, gather.
// DESIGN.md, "Resampling".
#include "bfd_internal.h"
#include "bfd_call.h"
#include "bfd_resample_core.h"
#include <math.h>
#include <string.h>
#include <algorithm>

namespace {

constexpr long MAX_BLOCKS = 1L << 20;             // work beyond this is taken by grid-stride loops
constexpr int PK_LINES = 64, PK_COLS = 32;        // axis-2 prefilter: lines per block (one per lane) and columns per LDS tile
constexpr int IT_K = 64, IT_J = 4;                // interpolation: threads along k and j

// staged interpolation: output tile (i, j, k); a wave is 2 j x 32 k, so the 32 lanes of an LDS lane group read consecutive float64 of one
// box row (ds_read_b64: 64 banks of 4 B, conflict-free); every thread takes the tile's four i. ST_CAP float64 = 36 KiB: LDS leaves room for
// four workgroups per CU, one more than the three (3 waves per SIMD) that the kernel's 161-171 registers allow.
constexpr int ST_I = 4, ST_J = 8, ST_K = 32, ST_CAP = 4608;

// input of any dtype -> float64, edge-replicated by npad per side
template <typename T>
__global__ __launch_bounds__(256) void to_f64_padded(const T *__restrict__ in, double *__restrict__ out, long N1, long N2, long N3, int npad)
{
    const long P2 = N2 + 2 * npad, P3 = N3 + 2 * npad;
    const long total = (N1 + 2 * npad) * P2 * P3;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const long k = t % P3, q = t / P3, j = q % P2, i = q / P2;
        const long si = min(max(i - npad, 0L), N1 - 1), sj = min(max(j - npad, 0L), N2 - 1), sk = min(max(k - npad, 0L), N3 - 1);
        out[t] = (double)in[(si * N2 + sj) * N3 + sk];
    }
}

// lines along axis 0 or 1: line l = (o, r) starts at o * outerStride + r, r < inner (contiguous), its n elements are `stride` apart
__global__ __launch_bounds__(256) void prefilter_strided(double *c, long nLines, long inner, long outerStride, long n, long stride, const rs_filter f)
{
    for (long l = (long)blockIdx.x * blockDim.x + threadIdx.x; l < nLines; l += (long)gridDim.x * blockDim.x) {
        const long o = l / inner, r = l - o * inner;
        rs_filter_line(c + o * outerStride + r, n, stride, f);
    }
}

// lines along axis 2: line l occupies c[l n .. l n + n)
__global__ __launch_bounds__(PK_LINES) void prefilter_k(double *c, long nLines, long n, const rs_filter f)
{
    __shared__ double tile[PK_LINES][PK_COLS + 1];
    const int lane = threadIdx.x;
    const long nGroups = (nLines + PK_LINES - 1) / PK_LINES;
    for (long grp = blockIdx.x; grp < nGroups; grp += gridDim.x) {
        const long line0 = grp * PK_LINES;
        const int rows = (int)min((long)PK_LINES, nLines - line0);
        double *base = c + line0 * n;
        const bool have = lane < rows;
        // the start value reads the line's two ends as they are before any store of this group
        double prev = have ? rs_causal_init(base + (long)lane * n, n, 1, f) : 0.0, prev2 = 0.0;
        __syncthreads();                                  // also: the tile is free (the group before has stored it)
        for (long t0 = 0; t0 < n; t0 += PK_COLS) {        // ---- causal, tiles forwards ----
            const int cols = (int)min((long)PK_COLS, n - t0);
            for (int e = lane; e < PK_LINES * PK_COLS; e += PK_LINES) {
                const int r = e / PK_COLS, q = e % PK_COLS;
                if (r < rows && q < cols) tile[r][q] = base[(long)r * n + t0 + q];
            }
            __syncthreads();
            if (have)
                for (int q = 0; q < cols; q++) {
                    if (t0 + q > 0) { prev2 = prev; prev = f.gain * tile[lane][q] + f.z * prev; }
                    tile[lane][q] = prev;
                }
            __syncthreads();
            for (int e = lane; e < PK_LINES * PK_COLS; e += PK_LINES) {
                const int r = e / PK_COLS, q = e % PK_COLS;
                if (r < rows && q < cols) base[(long)r * n + t0 + q] = tile[r][q];
            }
            __syncthreads();
        }
        double next = rs_anticausal_init(prev2, prev, f);
        for (long t0 = ((n - 1) / PK_COLS) * PK_COLS; t0 >= 0; t0 -= PK_COLS) {      // ---- anti-causal, tiles backwards ----
            const int cols = (int)min((long)PK_COLS, n - t0);
            for (int e = lane; e < PK_LINES * PK_COLS; e += PK_LINES) {
                const int r = e / PK_COLS, q = e % PK_COLS;
                if (r < rows && q < cols) tile[r][q] = base[(long)r * n + t0 + q];
            }
            __syncthreads();
            if (have)
                for (int q = cols - 1; q >= 0; q--) {
                    if (t0 + q < n - 1) next = f.z * (next - tile[lane][q]);
                    tile[lane][q] = next;
                }
            __syncthreads();
            for (int e = lane; e < PK_LINES * PK_COLS; e += PK_LINES) {
                const int r = e / PK_COLS, q = e % PK_COLS;
                if (r < rows && q < cols) base[(long)r * n + t0 + q] = tile[r][q];
            }
            __syncthreads();
        }
    }
}

template <typename TIn, typename TOut, int ORDER>
__global__ __launch_bounds__(IT_K * IT_J) void interp3d(const TIn *__restrict__ coef, TOut *__restrict__ out, const rs_geom g, long nTk, long nTj, long nTiles)
{
    const int tk = threadIdx.x % IT_K, tj = threadIdx.x / IT_K;
    for (long t = blockIdx.x; t < nTiles; t += gridDim.x) {
        const long bk = t % nTk, q = t / nTk, bj = q % nTj, i = q / nTj;
        const long j = bj * IT_J + tj, k = bk * IT_K + tk;
        if (j >= g.O[1] || k >= g.O[2]) continue;
        rs_store(rs_voxel<TIn, ORDER>(coef, g, i, j, k), out + (i * g.O[1] + j) * g.O[2] + k);
    }
}

// order 3 with the tile's source box in LDS
template <typename TIn, typename TOut>
__global__ __launch_bounds__(ST_J * ST_K) void interp3d_staged(const TIn *__restrict__ coef, TOut *__restrict__ out, const rs_geom g, long nTk, long nTj, long nTiles)
{
    __shared__ double box[ST_CAP];
    const int tk = threadIdx.x % ST_K, tj = threadIdx.x / ST_K;
    for (long t = blockIdx.x; t < nTiles; t += gridDim.x) {
        const long bk = t % nTk, q = t / nTk, bj = q % nTj, bi = q / nTj;
        const long lo[3] = {bi * ST_I, bj * ST_J, bk * ST_K};
        const long hi[3] = {min(lo[0] + ST_I, g.O[0]) - 1, min(lo[1] + ST_J, g.O[1]) - 1, min(lo[2] + ST_K, g.O[2]) - 1};
        // workgroup-uniform: a function of the tile alone
        rs_box b = {{0, 0, 0}, {0, 0, 0}};
        const bool staged = rs_tile_box(g, lo, hi, b) && b.n[0] * b.n[1] * b.n[2] <= (long)ST_CAP;
        __syncthreads();                                  // the tile before has been read
        if (staged) {
            const int n12 = (int)(b.n[1] * b.n[2]), n2 = (int)b.n[2], cells = (int)b.n[0] * n12;
            for (int e = threadIdx.x; e < cells; e += ST_J * ST_K) {      // ends: cells <= ST_CAP
                const int e0 = e / n12, r = e - e0 * n12, e1 = r / n2, e2 = r - e1 * n2;
                const long s0 = rs_tap_index(b.lo[0] + e0, g.I[0], g.mode), s1 = rs_tap_index(b.lo[1] + e1, g.I[1], g.mode),
                           s2 = rs_tap_index(b.lo[2] + e2, g.I[2], g.mode);
                box[e] = (double)coef[(s0 * g.I[1] + s1) * g.I[2] + s2];
            }
        }
        __syncthreads();
        const long j = lo[1] + tj, k = lo[2] + tk;
        if (j > hi[1] || k > hi[2]) continue;
        for (long i = lo[0]; i <= hi[0]; i++) {
            rs_taps<3> tp;
            double v = g.cval;
            if (rs_make_taps<3>(g, i, j, k, tp)) {
                const long o0 = tp.start[0] - b.lo[0], o1 = tp.start[1] - b.lo[1], o2 = tp.start[2] - b.lo[2];
                const bool inside = staged && o0 >= 0 && o0 + 3 < b.n[0] && o1 >= 0 && o1 + 3 < b.n[1] && o2 >= 0 && o2 + 3 < b.n[2];
                if (inside) {
                    const double *base = box + (o0 * b.n[1] + o1) * b.n[2] + o2;
                    const int n12 = (int)(b.n[1] * b.n[2]), n2 = (int)b.n[2];
                    v = rs_sum<3>(tp, [&](int a, int bb, int c) { return base[a * n12 + bb * n2 + c]; });
                } else {
                    const long I1 = g.I[1], I2 = g.I[2];
                    v = rs_sum<3>(tp, [&](int a, int bb, int c) { return (double)coef[(tp.idx[0][a] * I1 + tp.idx[1][bb]) * I2 + tp.idx[2][c]]; });
                }
            }
            rs_store(v, out + (i * g.O[1] + j) * g.O[2] + k);
        }
    }
}

template <typename TIn, typename TOut>
void launch_interp(const void *coef, void *out, const rs_geom &g, int order, bool gathered)
{
    if (order == 3 && !gathered) {
        const long sTk = (g.O[2] + ST_K - 1) / ST_K, sTj = (g.O[1] + ST_J - 1) / ST_J, sTiles = sTk * sTj * ((g.O[0] + ST_I - 1) / ST_I);
        hipLaunchKernelGGL((interp3d_staged<TIn, TOut>), dim3(blocks_for(sTiles, 1, MAX_BLOCKS)), dim3(ST_J * ST_K), 0, 0,
                           (const TIn *)coef, (TOut *)out, g, sTk, sTj, sTiles);
        return;
    }
    const long nTk = (g.O[2] + IT_K - 1) / IT_K, nTj = (g.O[1] + IT_J - 1) / IT_J, nTiles = nTk * nTj * g.O[0];
    const dim3 grid(blocks_for(nTiles, 1, MAX_BLOCKS)), block(IT_K * IT_J);
    const TIn *c = (const TIn *)coef;
    TOut *o = (TOut *)out;
    if (order == 0) hipLaunchKernelGGL((interp3d<TIn, TOut, 0>), grid, block, 0, 0, c, o, g, nTk, nTj, nTiles);
    else if (order == 1) hipLaunchKernelGGL((interp3d<TIn, TOut, 1>), grid, block, 0, 0, c, o, g, nTk, nTj, nTiles);
    else if (order == 2) hipLaunchKernelGGL((interp3d<TIn, TOut, 2>), grid, block, 0, 0, c, o, g, nTk, nTj, nTiles);
    else hipLaunchKernelGGL((interp3d<TIn, TOut, 3>), grid, block, 0, 0, c, o, g, nTk, nTj, nTiles);
}

template <typename T>
void launch_dtype(bool fromCoef, const void *coef, void *out, const rs_geom &g, int order, bool gathered)
{
    if (fromCoef) launch_interp<double, T>(coef, out, g, order, gathered);
    else launch_interp<T, T>(coef, out, g, order, gathered);
}

// dtype codes of the two entries
constexpr int DT_U8 = 0, DT_F32 = 1, DT_I16 = 2;       // 3: float64
size_t dtype_size(int dtype) { return dtype == DT_U8 ? 1 : dtype == DT_I16 ? 2 : dtype == DT_F32 ? 4 : sizeof(double) /* DT_F64 */; }

// in (device, any dtype, [N]) -> out (float64, [N + 2 npad])
void launch_to_f64(int dtype, const void *in, double *out, const int64_t N[3], int npad)
{
    const long n1 = (long)N[0], n2 = (long)N[1], n3 = (long)N[2];
    const dim3 grid(blocks_for((n1 + 2 * npad) * (n2 + 2 * npad) * (n3 + 2 * npad), 256, MAX_BLOCKS)), block(256);
    if (dtype == DT_U8) hipLaunchKernelGGL(to_f64_padded<uint8_t>, grid, block, 0, 0, (const uint8_t *)in, out, n1, n2, n3, npad);
    else if (dtype == DT_I16) hipLaunchKernelGGL(to_f64_padded<int16_t>, grid, block, 0, 0, (const int16_t *)in, out, n1, n2, n3, npad);
    else if (dtype == DT_F32) hipLaunchKernelGGL(to_f64_padded<float>, grid, block, 0, 0, (const float *)in, out, n1, n2, n3, npad);
    else hipLaunchKernelGGL(to_f64_padded<double>, grid, block, 0, 0, (const double *)in, out, n1, n2, n3, npad);
}

// in (device, dtype, [N]) -> c (float64, [N + 2 npad]), filtered along the three axes
hipError_t prefilter_on_device(const void *in, double *c, int dtype, const int64_t N[3], int npad, int order, int mode)
{
    const long P[3] = {(long)N[0] + 2 * npad, (long)N[1] + 2 * npad, (long)N[2] + 2 * npad};
    launch_to_f64(dtype, in, c, N, npad);
    // axes of length 1 pass through, as in scipy
    if (P[0] > 1) {
        const long lines = P[1] * P[2];
        hipLaunchKernelGGL(prefilter_strided, dim3(blocks_for(lines, 256, MAX_BLOCKS)), dim3(256), 0, 0, c, lines, lines, 0L, P[0], P[1] * P[2], rs_make_filter(order, P[0], mode));
    }
    if (P[1] > 1) {
        const long lines = P[0] * P[2];
        hipLaunchKernelGGL(prefilter_strided, dim3(blocks_for(lines, 256, MAX_BLOCKS)), dim3(256), 0, 0, c, lines, P[2], P[1] * P[2], P[1], P[2], rs_make_filter(order, P[1], mode));
    }
    if (P[2] > 1) {
        const long lines = P[0] * P[1];
        hipLaunchKernelGGL(prefilter_k, dim3(blocks_for(lines, PK_LINES, MAX_BLOCKS)), dim3(PK_LINES), 0, 0, c, lines, P[2], rs_make_filter(order, P[2], mode));
    }
    return hipGetLastError();
}

}  // namespace

extern "C" int bfd_affine_transform3d(int device, int dtype, const void *in, void *out, int64_t N1, int64_t N2, int64_t N3,
                                      int64_t O1, int64_t O2, int64_t O3, const double *matrix, int order, int mode, double cval, int flags,
                                      float *kernelMs)
{
    static const char *who = "bfd_affine_transform3d";
    // every argument error is reported before a device is looked for
    if (dtype < 0 || dtype > 3) BFD_FAIL(-1, std::string(who) + ": dtype must be 0 (uint8), 1 (float32), 2 (int16) or 3 (float64)");
    if (!in || !out || !matrix) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (in == out) BFD_FAIL(-1, std::string(who) + ": out may not alias in");
    if (order < 0 || order > 3) BFD_FAIL(-1, std::string(who) + ": order must be 0, 1, 2 or 3");
    if (mode < 0 || mode > 2) BFD_FAIL(-1, std::string(who) + ": mode must be 0 (constant), 1 (nearest) or 2 (mirror)");
    if (N1 < 0 || N2 < 0 || N3 < 0 || O1 < 0 || O2 < 0 || O3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (!volume_fits(N1, N2, N3)) BFD_FAIL(-1, std::string(who) + ": the input has 2^31 voxels or more (limit: fewer than 2^31)");
    if (!volume_fits(O1, O2, O3)) BFD_FAIL(-1, std::string(who) + ": the output has 2^31 voxels or more (limit: fewer than 2^31)");
    for (int q = 0; q < 12; q++)
        if (!std::isfinite(matrix[q])) BFD_FAIL(-1, std::string(who) + ": the matrix has an element that is not finite");
    if ((dtype == DT_U8 || dtype == DT_I16) && !std::isfinite(cval)) BFD_FAIL(-1, std::string(who) + ": cval is not finite and the dtype is an integer");
    const size_t esz = dtype_size(dtype);
    const size_t nIn = (size_t)(N1 * N2 * N3), nOut = (size_t)(O1 * O2 * O3);
    if (overlap(in, nIn * esz, out, nOut * esz)) BFD_FAIL(-1, std::string(who) + ": out may not alias in");
    if (nOut && !nIn) BFD_FAIL(-1, std::string(who) + ": the input is empty");

    if (flags & ~3) BFD_FAIL(-1, std::string(who) + ": flags has bits other than 1 (prefilter) and 2 (gathered interpolation)");
    const bool filt = (flags & 1) && order > 1, gathered = (flags & 2) != 0;
    rs_geom g;
    g.npad = filt && mode == RS_NEAREST ? RS_NPAD : 0;
    const int64_t N[3] = {N1, N2, N3};
    for (int a = 0; a < 3; a++) g.I[a] = (long)N[a] + 2 * g.npad;
    g.O[0] = (long)O1; g.O[1] = (long)O2; g.O[2] = (long)O3;
    memcpy(g.m, matrix, sizeof g.m);
    g.mode = mode;
    g.cval = cval;

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) kernelMs[0] = kernelMs[1] = 0.f;
    if (nOut == 0) return 0;

    DevTemp<char> din, dout;
    DevTemp<double> dcoef;
    Events ev;
    BFD_STEP(din.alloc(nIn * esz));
    BFD_STEP(dout.alloc(nOut * esz));
    if (filt) BFD_STEP(dcoef.alloc((size_t)(g.I[0] * g.I[1] * g.I[2])));
    BFD_STEP(hipMemcpy(din, in, nIn * esz, hipMemcpyHostToDevice));
    BFD_STEP(ev.create(3));
    BFD_STEP(ev.record(0));
    if (filt) BFD_STEP(prefilter_on_device(din, dcoef, dtype, N, g.npad, order, mode));
    BFD_STEP(ev.record(1));
    const void *src = filt ? (const void *)dcoef.p : (const void *)din.p;
    if (dtype == DT_U8) launch_dtype<uint8_t>(filt, src, dout, g, order, gathered);
    else if (dtype == DT_I16) launch_dtype<int16_t>(filt, src, dout, g, order, gathered);
    else if (dtype == DT_F32) launch_dtype<float>(filt, src, dout, g, order, gathered);
    else launch_dtype<double>(filt, src, dout, g, order, gathered);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(2));
    BFD_STEP(ev.sync(2));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    BFD_STEP(ev.elapsed(kernelMs ? kernelMs + 1 : nullptr, 1, 2));
    BFD_STEP(hipMemcpy(out, dout, nOut * esz, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int bfd_spline_filter3d(int device, int dtype, const void *in, double *out, int64_t N1, int64_t N2, int64_t N3, int order, int mode,
                                   float *kernelMs)
{
    static const char *who = "bfd_spline_filter3d";
    if (dtype < 0 || dtype > 3) BFD_FAIL(-1, std::string(who) + ": dtype must be 0 (uint8), 1 (float32), 2 (int16) or 3 (float64)");
    if (!in || !out) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (in == (const void *)out) BFD_FAIL(-1, std::string(who) + ": out may not alias in");
    if (order < 0 || order > 3) BFD_FAIL(-1, std::string(who) + ": order must be 0, 1, 2 or 3");
    if (mode < 0 || mode > 2) BFD_FAIL(-1, std::string(who) + ": mode must be 0 (constant), 1 (nearest) or 2 (mirror)");
    if (N1 < 0 || N2 < 0 || N3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (!volume_fits(N1, N2, N3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    const size_t esz = dtype_size(dtype);
    const size_t n = (size_t)(N1 * N2 * N3);
    if (overlap(in, n * esz, out, n * sizeof(double))) BFD_FAIL(-1, std::string(who) + ": out may not alias in");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) return 0;

    DevTemp<char> din;
    DevTemp<double> dcoef;
    Events ev;
    const int64_t N[3] = {N1, N2, N3};
    BFD_STEP(din.alloc(n * esz));
    BFD_STEP(dcoef.alloc(n));
    BFD_STEP(hipMemcpy(din, in, n * esz, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    if (order > 1) BFD_STEP(prefilter_on_device(din, dcoef, dtype, N, 0, order, mode));
    else {                                                // orders 0 and 1 have no poles: the values themselves, as float64
        launch_to_f64(dtype, din, dcoef, N, 0);
        BFD_STEP(hipGetLastError());
    }
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    BFD_STEP(hipMemcpy(out, dcoef, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
