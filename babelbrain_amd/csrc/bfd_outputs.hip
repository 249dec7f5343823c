// What leaves the engine of libbabelfdtd_hip.so: sensor setup and capture, map accumulation, the single-bin DFT and the
// device-to-host paths of the result getters (include/babelfdtd.h). gfx950 only.
#include <functional>
#include <sys/mman.h>
#include "bfd_internal.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <thread>

// pinned 16 MB pieces of copy_out_large, kept from one readback of a call to the next (allocating and releasing eight of them costs 22 ms, as much as
// moving a 512^3 map); given back to the system with the placement cache (bfd_placement_cache_release: the drop-in call does that at its end; bfd_release_pinned_pieces)
static std::mutex g_pinMutex;
static std::vector<char *> g_pinFree;
static const size_t kPinPiece = (size_t)16 << 20;
static char *pin_take(size_t bytes)
{
    if (bytes == kPinPiece) {
        std::lock_guard<std::mutex> lk(g_pinMutex);
        if (!g_pinFree.empty()) { char *p = g_pinFree.back(); g_pinFree.pop_back(); return p; }
    }
    char *p = nullptr;
    if (hipHostMalloc((void **)&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
static void pin_give(char *p, size_t bytes)
{
    if (!p) return;
    if (bytes == kPinPiece) {
        std::lock_guard<std::mutex> lk(g_pinMutex);
        if (g_pinFree.size() < 32) { g_pinFree.push_back(p); return; }
    }
    hipHostFree(p);
}
void bfd_release_pinned_pieces(void)
{
    std::lock_guard<std::mutex> lk(g_pinMutex);
    for (char *p : g_pinFree) hipHostFree(p);
    g_pinFree.clear();
}

namespace {

// x-fastest device layout -> strided caller layout (through a dense device staging buffer)
__global__ void scatter_from_xfast(const float *__restrict__ in, float *__restrict__ out, long s1, long s2, long s3,
                                   int N1, int N2, int nk)
{
    const long n = (long)N1 * N2 * nk;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long)gridDim.x * blockDim.x) {
        const int i = (int)(v % N1), j = (int)((v / N1) % N2), k = (int)(v / ((long)N1 * N2));
        out[i * s1 + j * s2 + k * s3] = in[v];
    }
}
// does cell c (local linear index) hold only the Szz/Rzz copy of its normal stresses? (every fluid cell: bfd_dev::cls)
__device__ __forceinline__ bool normal_collapsed(const bfd_dev &d, long c)
{
    return (d.cls[c] & BFD_CLS_FLUID) != 0;
}

// a value that exists only at solid cells: from the compact arrays when the solid state is compact (0 where the cell is not listed:
// a reflector, or a fluid cell asked for a shear stress), else from the full-volume array. KNOWN: the caller has the cell's list entry
// already (e, -1 = not listed) -- the sensor kernels take it from a per-sensor table, accumulate_maps from the row table and a ballot --
// otherwise css_index walks the class bytes of the row
template <bool KNOWN>
__device__ __forceinline__ float solid_value(const bfd_dev &d, const float *full, const float *comp, long c, long e)
{
    if (!d.cssRow) return full[c];
    if (!KNOWN) e = css_index(d, c);
    return e >= 0 ? comp[e] : 0.0f;
}
template <bool KNOWN>
__device__ __forceinline__ float map_value_t(const bfd_dev &d, int sel, long c, long e)
{
    switch (sel) {
    case BFD_MAP_VX: return d.Vx[c];
    case BFD_MAP_VY: return d.Vy[c];
    case BFD_MAP_VZ: return d.Vz[c];
    case BFD_MAP_SIGMAXX: return normal_collapsed(d, c) ? d.Szz[c] : solid_value<KNOWN>(d, d.Sxx, d.cSxx, c, e);     // a fluid cell keeps one copy of its normal stresses
    case BFD_MAP_SIGMAYY: return normal_collapsed(d, c) ? d.Szz[c] : solid_value<KNOWN>(d, d.Syy, d.cSyy, c, e);
    case BFD_MAP_SIGMAZZ: return d.Szz[c];
    case BFD_MAP_SIGMAXY: return solid_value<KNOWN>(d, d.Sxy, d.cSxy, c, e);
    case BFD_MAP_SIGMAXZ: return solid_value<KNOWN>(d, d.Sxz, d.cSxz, c, e);
    case BFD_MAP_SIGMAYZ: return solid_value<KNOWN>(d, d.Syz, d.cSyz, c, e);
    case BFD_MAP_PRESSURE: {
        const float zz = d.Szz[c];
        if (normal_collapsed(d, c)) return -((zz + zz) + zz) * (1.0f / 3.0f);
        float xx, yy;
        if (d.cssRow) { if (!KNOWN) e = css_index(d, c); xx = e >= 0 ? d.cSxx[e] : 0.0f; yy = e >= 0 ? d.cSyy[e] : 0.0f; }
        else { xx = d.Sxx[c]; yy = d.Syy[c]; }
        const float s = (xx + yy) + zz;
        return -s * (1.0f / 3.0f);
    }
    default: return 0.0f;
    }
}
__device__ __forceinline__ float map_value(const bfd_dev &d, int sel, long c) { return map_value_t<false>(d, sel, c, -1); }
// value of map `sel` as the outputs define it (ALLV = |V|) with the cell's list entry known
__device__ __forceinline__ float output_value(const bfd_dev &d, int sel, long c, long e)
{
    if (sel == BFD_MAP_ALLV) { const float x = d.Vx[c], y = d.Vy[c], z = d.Vz[c]; return sqrtf((x * x + y * y) + z * z); }
    return map_value_t<true>(d, sel, c, e);
}
__device__ __forceinline__ bool map_needs_entry(int sel)
{
    return sel == BFD_MAP_SIGMAXX || sel == BFD_MAP_SIGMAYY || sel == BFD_MAP_SIGMAXY || sel == BFD_MAP_SIGMAXZ || sel == BFD_MAP_SIGMAYZ || sel == BFD_MAP_PRESSURE;
}
// list entries of the sensor voxels (compact solid state), resolved once per list: a capture is a plain gather again
__global__ void sensor_entries(bfd_dev d, const uint32_t *__restrict__ lin, long nSens, int *__restrict__ out)
{
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < nSens; s += (long)gridDim.x * blockDim.x)
        out[s] = (int)css_index(d, (long)lin[s]);
}
// fluid cells keep only Szz/Rzz of their identical normal stresses: restore the other copies
__global__ void expand_normal(bfd_dev d, long n)
{
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long)gridDim.x * blockDim.x) {
        if (!normal_collapsed(d, v)) continue;
        const float s = d.Szz[v], r = d.Rzz[v];
        d.Sxx[v] = s; d.Syy[v] = s; d.Rxx[v] = r; d.Ryy[v] = r;
    }
}
// output assembly (bfd_get_field, compact solid state): out = src at the cells that keep one copy of their normal stresses
__global__ void copy_at_fluid_cells(bfd_dev d, const float *__restrict__ src, float *__restrict__ out, long n)
{
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long)gridDim.x * blockDim.x)
        if (normal_collapsed(d, v)) out[v] = src[v];
}
__device__ __forceinline__ float map_sq(const bfd_dev &d, int sel, long c)
{
    if (sel == BFD_MAP_ALLV) {
        const float x = d.Vx[c], y = d.Vy[c], z = d.Vz[c];
        return (x * x + y * y) + z * z;
    }
    const float v = map_value(d, sel, c);
    return v * v;
}

struct SelList { int n; int sel[BFD_MAP_COUNT]; int skip[BFD_MAP_COUNT]; };

// RMS / peak accumulation outside the absorbing layer (generic path, any map selection). A wave = 64 consecutive x cells of one row: with a
// compact solid state the cell's list entry is the row-table base of this x tile + the listed lanes below (one ballot), once for all selections
__global__ __launch_bounds__(256) void accumulate_maps(bfd_dev d, SelList L, float *__restrict__ acc, float *__restrict__ pk, long nloc)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    const int kl = blockIdx.z;
    const int k = d.k0 + kl;
    const bool inDomain = i < d.N1 && j < d.N2;
    const long c = (long)kl * d.plane + (long)j * d.N1 + i;
    long e = -1;
    if (d.cssRow) {
        bool need = false;
        for (int q = 0; q < L.n; q++) need = need || (!L.skip[q] && map_needs_entry(L.sel[q]));
        if (need) {                                                      // block-uniform
            const bool listed = inDomain && css_listed(d.cls[c]);
            const unsigned rank = css_rank(listed);
            const unsigned rb = j < d.N2 ? d.cssRow[((long)(kl + 2) * d.N2 + j) * d.cssStride + blockIdx.x] : BFD_CSS_NONE;
            if (listed && rb != BFD_CSS_NONE) e = (long)rb + rank;
        }
    }
    if (i < d.ND || i >= d.N1 - d.ND || j < d.ND || j >= d.N2 - d.ND || k < d.ND || k >= d.N3 - d.ND) return;
    for (int q = 0; q < L.n; q++) {
        if (L.skip[q]) continue;    // accumulated inside the velocity kernel
        const float v = output_value(d, L.sel[q], c, e);
        if (acc) acc[q * nloc + c] = acc[q * nloc + c] + (L.sel[q] == BFD_MAP_ALLV ? map_sq(d, BFD_MAP_ALLV, c) : v * v);
        if (pk) {
            const float a = fabsf(v);
            if (a > pk[q * nloc + c]) pk[q * nloc + c] = a;
        }
    }
}
__global__ void finalize_rms(const float *__restrict__ acc, float *__restrict__ out, long n, float cnt)
{
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long)gridDim.x * blockDim.x)
        out[v] = sqrtf(acc[v] / cnt);
}
__global__ void last_map(bfd_dev d, int sel, float *__restrict__ out, long n)
{
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long)gridDim.x * blockDim.x)
        out[v] = (sel == BFD_MAP_ALLV) ? sqrtf(map_sq(d, BFD_MAP_ALLV, v)) : map_value(d, sel, v);
}

// Sensor sets that are a dense box of voxels (what the caller's CreateSensorMap makes: everything inside the absorbing layer past the source plane,
// BASE:2279-2290) need no index list: sensor s of the box is voxel (i0 + s % bx, j0 + (s / bx) % by, k0 + s / (bx by)) -- the order of the ascending
// x-fastest linear index the list is in. lin == null selects that form (4 of the 13 bytes a captured sample moved were the index).
struct SensorBox { unsigned bx, bxy, i0, j0, k0; };
__device__ __forceinline__ long sensor_cell(const bfd_dev &d, const uint32_t *__restrict__ lin, const SensorBox &B, long s)
{
    if (lin) return (long)lin[s];
    const unsigned u = (unsigned)s, kk = u / B.bxy, r = u - kk * B.bxy, jj = r / B.bx, ii = r - jj * B.bx;
    return (long)(B.k0 + kk) * d.plane + (long)(B.j0 + jj) * d.N1 + (B.i0 + ii);
}
// bounding box of a sensor list (min / max of i, j, k): six atomics per workgroup
__global__ __launch_bounds__(256) void sensor_bounds(bfd_dev d, const uint32_t *__restrict__ lin, long n, unsigned *__restrict__ mm)
{
    unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (long)gridDim.x * blockDim.x) {
        const unsigned c = lin[s], kl = c / (unsigned)d.plane, r = c - kl * (unsigned)d.plane, j = r / (unsigned)d.N1, i = r - j * (unsigned)d.N1;
        lo[0] = min(lo[0], i); hi[0] = max(hi[0], i); lo[1] = min(lo[1], j); hi[1] = max(hi[1], j); lo[2] = min(lo[2], kl); hi[2] = max(hi[2], kl);
    }
    for (int a = 0; a < 3; a++) {
        for (int o = 32; o > 0; o >>= 1) { lo[a] = min(lo[a], (unsigned)__shfl_down((int)lo[a], o)); hi[a] = max(hi[a], (unsigned)__shfl_down((int)hi[a], o)); }
        if ((threadIdx.x & 63) == 0) { atomicMin(mm + a, lo[a]); atomicMax(mm + 3 + a, hi[a]); }
    }
}
// sensors: out[q][col][s]; ent = the sensors' list entries (compact solid state) or null
__global__ void record_sensors(bfd_dev d, SelList L, const uint32_t *__restrict__ lin, SensorBox B, const int *__restrict__ ent, long nSens,
                               float *__restrict__ out, int col, int nTs)
{
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < nSens; s += (long)gridDim.x * blockDim.x) {
        const long c = sensor_cell(d, lin, B, s);
        const long e = (ent && !normal_collapsed(d, c)) ? (long)ent[s] : -1;
        for (int q = 0; q < L.n; q++)
            out[((long)q * nTs + col) * nSens + s] = output_value(d, L.sel[q], c, e);
    }
}
// sensorMode 1: the sample of this step goes straight into the running single-bin DFT sums and peaks of its sensor
// (same arithmetic, sample by sample, as dft_series applies to a stored series)
__global__ void accumulate_sensor_dft(bfd_dev d, SelList L, const uint32_t *__restrict__ lin, SensorBox B, const int *__restrict__ ent, long nSens,
                                      double *__restrict__ acc, float *__restrict__ pk, int col, int nTs, int bin)
{
    const int r = (int)(((long)bin * col) % nTs);                 // exact phase index
    double sn, cs;
    sincospi(2.0 * (double)r / (double)nTs, &sn, &cs);
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < nSens; s += (long)gridDim.x * blockDim.x) {
        const long c = sensor_cell(d, lin, B, s);
        const long e = (ent && !normal_collapsed(d, c)) ? (long)ent[s] : -1;
        for (int q = 0; q < L.n; q++) {
            const float x = output_value(d, L.sel[q], c, e);
            double *a = acc + 2 * ((long)q * nSens + s);
            a[0] += (double)x * cs; a[1] -= (double)x * sn;
            float *p = pk + (long)q * nSens + s;
            *p = fmaxf(*p, x);
        }
    }
}
__global__ void fill_float(float *__restrict__ p, long n, float v)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = v;
}
__global__ void finalize_sensor_dft(const double *__restrict__ acc, float *__restrict__ out, long n2, double sc)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x) out[i] = (float)(acc[i] * sc);
}

// [q][nTs][nSens] -> [q][nSens][nTs]
__global__ void transpose_sensors(const float *__restrict__ in, float *__restrict__ out, long nSens, int nTs, int nq)
{
    const long n = nSens * nTs * nq;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long)gridDim.x * blockDim.x) {
        const int t = (int)(v % nTs);
        const long s = (v / nTs) % nSens;
        const long q = v / ((long)nTs * nSens);
        out[v] = in[(q * nTs + t) * nSens + s];
    }
}

// the same for elements [v0, v0 + cnt) of the transposed block only (out = a piece buffer): the sensor series leave the device piece by piece
__global__ void transpose_sensors_range(const float *__restrict__ in, float *__restrict__ out, long nSens, int nTs, long v0, long cnt)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (long)gridDim.x * blockDim.x) {
        const long v = v0 + i;
        const int t = (int)(v % nTs);
        const long s = (v / nTs) % nSens;
        const long q = v / ((long)nTs * nSens);
        out[i] = in[(q * nTs + t) * nSens + s];
    }
}

// single-bin DFT + peak of sensor series. x(s,n) = in[s*sS + n*sN]; out[s] = (2/nTs) sum_n x exp(-2 pi i bin n/nTs)
__global__ void dft_series(const float *__restrict__ in, long sS, long sN, long nSens, int nTs, int bin,
                           float *__restrict__ outReIm, float *__restrict__ outPeak)
{
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < nSens; s += (long)gridDim.x * blockDim.x) {
        double re = 0.0, im = 0.0;
        float pk = -INFINITY;
        for (int n = 0; n < nTs; n++) {
            const float x = in[s * sS + n * sN];
            const int r = (int)(((long)bin * n) % nTs);                 // exact phase index
            double sn, cs;
            sincospi(2.0 * (double)r / (double)nTs, &sn, &cs);
            re += (double)x * cs; im -= (double)x * sn;
            pk = fmaxf(pk, x);
        }
        const double sc = 2.0 / (double)nTs;
        outReIm[2 * s] = (float)(re * sc); outReIm[2 * s + 1] = (float)(im * sc);
        if (outPeak) outPeak[s] = pk;
    }
}

}  // namespace

// numpy.fft.fftfreq(n, d) bin closest to freq (first minimum, like np.argmin; BASE:2498-2499)
static int dft_bin(int n, double d, double freq)
{
    int best = 0; double bd = INFINITY;
    for (int k = 0; k < n; k++) {
        const int kk = (k < (n + 1) / 2) ? k : k - n;
        const double f = (double)kk / ((double)n * d);
        const double e = fabs(f - freq);
        if (e < bd) { bd = e; best = k; }
    }
    return best;
}

// A large result block lands in host memory the caller has just allocated and never touched (a fresh numpy array): the copy then runs at the rate the
// kernel can fault 4 KB pages in. Transparent huge pages are in `madvise` mode on the ROCm images, so the range is advised first: one hipMemcpy of
// 4.3 GiB into untouched memory 0.46 -> 0.22 s on the MI355X box (profiles/r6/d2h_into_untouched_memory.txt). Advice only: a mapping that cannot
// take it (file-backed, already populated) is left as it is.
void bfd_advise_result_buffer(void *p, size_t bytes)
{
    if (!p || bytes < ((size_t)8 << 20)) return;
    const uintptr_t a = ((uintptr_t)p + 4095) & ~(uintptr_t)4095, b = ((uintptr_t)p + bytes) & ~(uintptr_t)4095;
    if (b > a) (void)madvise((void *)a, (size_t)(b - a), MADV_HUGEPAGE);
}

// Device -> pageable host for the large result blocks (sensor series, maps): T host threads, each moving its slice in 16 MB pieces through two pinned
// buffers of its own (the next piece in flight while the last one is copied out). One hipMemcpy is bound by the single thread that copies out of the
// runtime's staging buffers: 4.3 GiB into untouched huge-page memory 0.22 s, this way 0.11 s (profiles/r6/d2h_into_untouched_memory.txt). `after`: the
// stream whose work produces src (waited for here). Without a producer anything that fails on the way falls back to the plain copy.
// produce (optional): fills a device piece buffer with bytes [o, o + len) of the block on the given stream -- the block then never exists as a whole
// on the device (the sensor series: no 4.6 GB scratch allocation, which in a short call waited 5 s when a placement search had just released its
// candidates -- the runtime gives them back in the background). With a producer it returns hipErrorNotSupported
// when it declines (small block, threads off: the caller takes its old way) and any failure on the way as the error it is.
static hipError_t copy_out_large(int device, void *dst, const void *src, size_t bytes, hipStream_t after,
                                 const std::function<void(float *, size_t, size_t, hipStream_t)> *produce = nullptr)
{
    int T = 4;
    if (const char *ev = getenv("BFD_D2H_THREADS")) T = atoi(ev);
    size_t PIECE = (size_t)16 << 20, least = (size_t)256 << 20;
    if (const char *ev = getenv("BFD_D2H_PIECE_KB")) PIECE = std::max((size_t)4096, ((size_t)atol(ev) << 10) & ~(size_t)4095);      // tests: small grids through the same code
    if (const char *ev = getenv("BFD_D2H_MIN_MB")) least = (size_t)atol(ev) << 20;
    if (T < 2 || bytes < least || bytes < (size_t)T * 4096) {
        if (produce) return hipErrorNotSupported;
        const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, after);
        return e == hipSuccess ? hipStreamSynchronize(after) : e;
    }
    T = std::min(T, 16);
    hipError_t e = hipStreamSynchronize(after);
    if (e != hipSuccess) return e;
    std::vector<char *> pin(2 * (size_t)T, nullptr);
    for (auto &q : pin) if (e == hipSuccess && !(q = pin_take(PIECE))) e = hipErrorOutOfMemory;
    std::vector<DevTemp<float>> dpiece(produce ? 2 * (size_t)T : 0);
    for (auto &q : dpiece) if (e == hipSuccess && (e = q.alloc(PIECE / sizeof(float))) != hipSuccess) (void)hipGetLastError();
    if (e == hipSuccess) {
        std::vector<hipError_t> failed((size_t)T, hipSuccess);       // every worker's first error
        std::vector<std::thread> th;
        for (int t = 0; t < T; t++)
            th.emplace_back([&, t] {
                const size_t a = (bytes / T * t) & ~(size_t)4095, b = t + 1 == T ? bytes : (bytes / T * (t + 1)) & ~(size_t)4095;
                hipStream_t st = nullptr;
                hipEvent_t ev[2] = {nullptr, nullptr};
                hipError_t w = hipSetDevice(device);
                if (w == hipSuccess) w = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
                for (int q = 0; q < 2 && w == hipSuccess; q++) w = hipEventCreateWithFlags(&ev[q], hipEventDisableTiming);
                const size_t np = (b - a + PIECE - 1) / PIECE;
                auto issue = [&](size_t i) {
                    const size_t o = a + i * PIECE, len = std::min(PIECE, b - o);
                    const void *from = (const char *)src + o;
                    hipError_t x = hipSuccess;
                    if (produce) { float *piece = dpiece[2 * t + (i & 1)]; (*produce)(piece, o, len, st); from = piece; x = hipGetLastError(); }
                    if (x == hipSuccess) x = hipMemcpyAsync(pin[2 * t + (i & 1)], from, len, hipMemcpyDeviceToHost, st);
                    return x == hipSuccess ? hipEventRecord(ev[i & 1], st) : x;
                };
                if (w == hipSuccess && np) w = issue(0);                      // a worker without its stream or events goes straight to the clean-up
                for (size_t i = 0; i < np && w == hipSuccess; i++) {
                    if (i + 1 < np) w = issue(i + 1);
                    if (w == hipSuccess) w = hipEventSynchronize(ev[i & 1]);
                    if (w != hipSuccess) break;
                    const size_t o = a + i * PIECE, len = std::min(PIECE, b - o);
                    memcpy((char *)dst + o, pin[2 * t + (i & 1)], len);
                }
                if (st) { hipStreamSynchronize(st); hipStreamDestroy(st); }
                for (int q = 0; q < 2; q++) if (ev[q]) hipEventDestroy(ev[q]);
                failed[t] = w;
            });
        for (auto &x : th) x.join();
        for (int t = 0; t < T; t++) if (e == hipSuccess) e = failed[t];
    }
    for (auto &q : pin) pin_give(q, PIECE);
    if (e == hipSuccess) return hipSuccess;
    (void)hipGetLastError();
    if (produce) return e;      // a failure, not a refusal: the caller reports it
    return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);      // the plain way
}

int bfd_sensors_into(bfd_sim *s, float *out, int64_t rowElems)
{
    // the series of selected map q go to out + q * rowElems (rowElems >= nSensors * nTs): a slab of a group
    // writes straight into its columns of the caller's array
    if (!s) BFD_FAIL(-1, "null sim");
    const size_t row = (size_t)s->nTs * (size_t)s->nSensors, n = (size_t)s->nSelS * row;
    if (!n) return 0;
    if (s->cfg.sensorMode != 0) BFD_FAIL(-6, "bfd_get_sensors: the series are not stored with sensorMode 1 (use bfd_get_sensor_dft)");
    if (!out || !s->sensOut) BFD_FAIL(-1, "bfd_get_sensors: null argument");
    if (rowElems < (int64_t)row) BFD_FAIL(-2, "bfd_get_sensors: row shorter than nSensors * nSteps");
    BFD_HIP(hipSetDevice(s->cfg.device));
    {   // piece by piece through the host threads, no scratch block on the device
        hipError_t e = hipSuccess;
        for (int q = 0; q < s->nSelS; q++) bfd_advise_result_buffer(out + (size_t)q * rowElems, row * sizeof(float));
        const bool oneBlock = (size_t)rowElems == row;
        for (int q = 0; q < (oneBlock ? 1 : s->nSelS) && e == hipSuccess; q++) {
            const long v00 = oneBlock ? 0 : (long)q * (long)row;
            const std::function<void(float *, size_t, size_t, hipStream_t)> produce = [&, v00](float *piece, size_t o, size_t len, hipStream_t st) {
                const long cnt = (long)(len / sizeof(float));
                hipLaunchKernelGGL(transpose_sensors_range, dim3(grid_for(cnt)), dim3(256), 0, st, s->sensOut, piece, (long)s->nSensors, s->nTs, v00 + (long)(o / sizeof(float)), cnt);
            };
            e = copy_out_large(s->cfg.device, out + (size_t)q * rowElems, nullptr, (oneBlock ? n : row) * sizeof(float), s->stream, &produce);
        }
        if (e == hipSuccess) return 0;
        if (e != hipErrorNotSupported) BFD_FAIL(-10, std::string("bfd_get_sensors: ") + hipGetErrorString(e));
        (void)hipGetLastError();      // declined (small block, BFD_D2H_THREADS < 2): the whole block through a scratch copy
    }
    DevTemp<float> tmp;
    BFD_HIP(tmp.alloc(n));
    hipLaunchKernelGGL(transpose_sensors, dim3(grid_for((long)n)), dim3(256), 0, s->stream, s->sensOut, tmp.p, (long)s->nSensors, s->nTs, s->nSelS);
    hipError_t e = hipSuccess;
    for (int q = 0; q < s->nSelS; q++) bfd_advise_result_buffer(out + (size_t)q * rowElems, row * sizeof(float));
    if ((size_t)rowElems == row) e = copy_out_large(s->cfg.device, out, tmp, n * sizeof(float), s->stream);
    else
        for (int q = 0; q < s->nSelS && e == hipSuccess; q++)
            e = copy_out_large(s->cfg.device, out + (size_t)q * rowElems, tmp + (size_t)q * row, row * sizeof(float), s->stream);
    if (e != hipSuccess) BFD_FAIL(-10, std::string("bfd_get_sensors: ") + hipGetErrorString(e));
    return 0;
}

// End of a time step on stream st: the maps the velocity kernels did not accumulate themselves (qP = the slot they did, -1 = none) and the sensor sample
int bfd_step_outputs(bfd_sim *s, hipStream_t st, int qP)
{
    const bfd_dev &d = s->d;
    const int n = s->step;
    const bool accNow = (s->acc || s->pk) && n >= s->accStart;
    int rc = 0;
    if (accNow && !(qP >= 0 && s->nSelR == 1)) {
        SelList L; L.n = s->nSelR; memcpy(L.sel, s->selR, sizeof L.sel);
        for (int q = 0; q < BFD_MAP_COUNT; q++) L.skip[q] = (q == qP);
        dim3 block(64, 4, 1), grid((d.N1 + 63) / 64, (d.N2 + 3) / 4, d.nk);
        hipLaunchKernelGGL(accumulate_maps, grid, block, 0, st, d, L, s->acc, s->pk, (long)s->nloc);
    }
    if (s->nSensors && (s->sensOut || s->dftAcc) && n % s->cfg.sensorSub == 0 && n / s->cfg.sensorSub >= s->cfg.sensorStart) {
        const int col = n / s->cfg.sensorSub - s->cfg.sensorStart;
        if (col < s->nTs) {
            SelList L; L.n = s->nSelS; memcpy(L.sel, s->selS, sizeof L.sel); memset(L.skip, 0, sizeof L.skip);
            // compact solid state: the sensors' list entries, resolved when first needed after a list was built (round 6; every capture used to
            // walk the class bytes of the row for each solid sensor: 1.08 ms per capture on the shear medium at 512^3 against 0.42 ms at C3)
            const int *ent = nullptr;
            if (d.cssRow) {
                if (!s->sensEntValid) {
                    if (!s->sensEnt) { rc = dev_alloc(s, &s->sensEnt, (size_t)s->nSensors, false); if (rc) return rc; }
                    hipLaunchKernelGGL(sensor_entries, dim3(grid_for(s->nSensors)), dim3(256), 0, st, d, s->sensLin, (long)s->nSensors, s->sensEnt);
                    s->sensEntValid = true;
                }
                ent = s->sensEnt;
            }
            SensorBox B = {(unsigned)s->sensBox[0], (unsigned)s->sensBox[0] * (unsigned)s->sensBox[1], (unsigned)s->sensBox[2], (unsigned)s->sensBox[3], (unsigned)s->sensBox[4]};
            const uint32_t *lin = s->sensIsBox ? nullptr : s->sensLin;
            if (s->sensOut)
                hipLaunchKernelGGL(record_sensors, dim3(grid_for(s->nSensors)), dim3(256), 0, st, d, L, lin, B, ent,
                                   (long)s->nSensors, s->sensOut, col, s->nTs);
            else
                hipLaunchKernelGGL(accumulate_sensor_dft, dim3(grid_for(s->nSensors)), dim3(256), 0, st, d, L, lin, B, ent,
                                   (long)s->nSensors, s->dftAcc, s->dftPk, col, s->nTs, s->dftBin);
        }
    }
    return 0;
}

// the output arrays start over with the state (bfd_reset), on the engine's stream
int bfd_clear_outputs(bfd_sim *s)
{
    if (s->acc) BFD_HIP(hipMemsetAsync(s->acc, 0, (size_t)s->nSelR * s->nloc * sizeof(float), s->stream));
    if (s->pk) BFD_HIP(hipMemsetAsync(s->pk, 0, (size_t)s->nSelR * s->nloc * sizeof(float), s->stream));
    if (s->sensOut) BFD_HIP(hipMemsetAsync(s->sensOut, 0, (size_t)s->nSelS * s->nTs * (size_t)s->nSensors * sizeof(float), s->stream));
    if (s->dftAcc) {
        BFD_HIP(hipMemsetAsync(s->dftAcc, 0, 2 * (size_t)s->nSelS * (size_t)s->nSensors * sizeof(double), s->stream));
        if (s->nSensors > 0) hipLaunchKernelGGL(fill_float, dim3(grid_for((long)s->nSelS * s->nSensors)), dim3(256), 0, s->stream, s->dftPk, (long)s->nSelS * s->nSensors, -INFINITY);
    }
    return 0;
}

// A new sensor set of `count` voxels: what the old one held is released; the index list (unfilled), the series block or the running DFT sums and
// peaks and the DFT bin are set up; the set counts as a list until the caller says it is a box. Shared by bfd_set_sensor_map and bfd_set_sensor_box
static int sensor_storage(bfd_sim *s, int count)
{
    s->nSensors = count;
    dev_release(s, &s->sensLin); dev_release(s, &s->sensOut); dev_release(s, &s->dftAcc); dev_release(s, &s->dftPk);
    dev_release(s, &s->sensEnt); s->sensEntValid = false;
    s->sensIsBox = false;
    int rc = dev_alloc(s, &s->sensLin, (size_t)count, false);
    if (!rc && s->nSelS && s->nTs > 0) {
        if (s->cfg.sensorMode == 0) rc = dev_alloc(s, &s->sensOut, (size_t)s->nSelS * s->nTs * (size_t)count);
        else {
            rc = dev_alloc(s, &s->dftAcc, 2 * (size_t)s->nSelS * (size_t)count);
            if (!rc) rc = dev_alloc(s, &s->dftPk, (size_t)s->nSelS * (size_t)std::max(count, 1), false);
            if (!rc && count > 0) hipLaunchKernelGGL(fill_float, dim3(grid_for((long)s->nSelS * count)), dim3(256), 0, s->stream, s->dftPk, (long)s->nSelS * count, -INFINITY);
            s->dftBin = dft_bin(s->nTs, s->cfg.dt * s->cfg.sensorSub, s->cfg.freq);
        }
    }
    return rc;
}
// BFD_SENSOR_BOX=0 keeps the index list in use for the captures of a dense box
static bool sensor_box_form_allowed()
{
    const char *ev = getenv("BFD_SENSOR_BOX");
    return !ev || atoi(ev) != 0;
}
// the index list of a dense box, in the ascending x-fastest order bfd_set_sensor_map's select gives
__global__ void box_sensor_indices(bfd_dev d, SensorBox B, long n, uint32_t *__restrict__ lin)
{
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (long)gridDim.x * blockDim.x)
        lin[s] = (uint32_t)sensor_cell(d, nullptr, B, s);
}

extern "C" {

int bfd_set_sensor_map(bfd_sim *s, const uint32_t *map, int64_t s1, int64_t s2, int64_t s3, int64_t *nSensors)
{
    if (!s || !map) BFD_FAIL(-1, "bfd_set_sensor_map: null argument");
    BFD_HIP(hipSetDevice(s->cfg.device));
    { const int rc = flush_pending(s); if (rc) return rc; }
    const bfd_dev &d = s->d;
    const size_t span = span_elems(d.N1, d.N2, d.nk, s1, s2, s3);
    DevTemp<uint32_t> tmp, sel; DevTemp<uint8_t> flags; DevTemp<char> work;
    DevTemp<int> dcount;      // the count of the select, then the six bounds words of the box test
    hipError_t e = tmp.alloc(span);
    if (e == hipSuccess) e = flags.alloc(s->nloc);
    if (e == hipSuccess) e = sel.alloc(s->nloc);
    if (e == hipSuccess) e = dcount.alloc(6);
    if (e == hipSuccess) e = hipMemcpyAsync(tmp, map, span * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream);
    int count = 0;
    if (e == hipSuccess) {
        bfd_launch_gather_flags(s, tmp, (long)s1, (long)s2, (long)s3, flags);
        e = select_flagged(flags, sel, dcount, (int)s->nloc, s->stream, work);
        if (e == hipSuccess) e = hipMemcpyAsync(&count, dcount, sizeof(int), hipMemcpyDeviceToHost, s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    }
    int rc = 0;
    const unsigned init[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};      // both outlive the stream sync below
    unsigned mm[6] = {0, 0, 0, 0, 0, 0}; bool boxTried = false;
    if (e == hipSuccess) {
        rc = sensor_storage(s, count);
        if (!rc && count) e = hipMemcpyAsync(s->sensLin, sel, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToDevice, s->stream);
        // a dense box of voxels? (count == volume of the bounding box: every voxel of the box is a sensor)
        const bool tryBox = count > 0 && sensor_box_form_allowed();
        if (!rc && e == hipSuccess && tryBox) {
            unsigned *dbounds = (unsigned *)dcount.p;
            e = hipMemcpyAsync(dbounds, init, sizeof init, hipMemcpyHostToDevice, s->stream);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(sensor_bounds, dim3(std::min(grid_for((long)count), 1024)), dim3(256), 0, s->stream, d, s->sensLin, (long)count, dbounds);
                e = hipMemcpyAsync(mm, dbounds, sizeof mm, hipMemcpyDeviceToHost, s->stream);
            }
            boxTried = e == hipSuccess;
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        if (e == hipSuccess && boxTried) {
            const long bx = (long)mm[3] - mm[0] + 1, by = (long)mm[4] - mm[1] + 1, bz = (long)mm[5] - mm[2] + 1;
            if (bx * by * bz == (long)count) {
                s->sensIsBox = true;
                s->sensBox[0] = (int)bx; s->sensBox[1] = (int)by; s->sensBox[2] = (int)mm[0]; s->sensBox[3] = (int)mm[1]; s->sensBox[4] = (int)mm[2];
            }
        }
    }
    if (e != hipSuccess) BFD_FAIL(-10, std::string("bfd_set_sensor_map: ") + hipGetErrorString(e));
    if (rc) return rc;
    if (nSensors) *nSensors = s->nSensors;
    return 0;
}

int bfd_set_sensor_box(bfd_sim *s, const int32_t *lo, const int32_t *size, int64_t *nSensors)
{
    if (!s || !lo || !size) BFD_FAIL(-1, "bfd_set_sensor_box: null argument");
    const bfd_dev &d = s->d;
    const int dim[3] = {d.N1, d.N2, d.nk};
    for (int a = 0; a < 3; a++) {
        if (size[a] <= 0) BFD_FAIL(-1, "bfd_set_sensor_box: empty box");
        if (lo[a] < 0 || lo[a] >= dim[a] || size[a] > dim[a] - lo[a]) BFD_FAIL(-1, "bfd_set_sensor_box: the box leaves the slab");
    }
    if (s->nloc > (size_t)0x7FFFFFFF) BFD_FAIL(-2, "bfd_set_sensor_box: slab too large for 32-bit sensor counts");
    BFD_HIP(hipSetDevice(s->cfg.device));
    { const int rc = flush_pending(s); if (rc) return rc; }
    const long count = (long)size[0] * size[1] * size[2];
    const int rc = sensor_storage(s, (int)count);
    if (rc) return rc;
    s->sensBox[0] = size[0]; s->sensBox[1] = size[1]; s->sensBox[2] = lo[0]; s->sensBox[3] = lo[1]; s->sensBox[4] = lo[2];
    const SensorBox B = {(unsigned)size[0], (unsigned)size[0] * (unsigned)size[1], (unsigned)lo[0], (unsigned)lo[1], (unsigned)lo[2]};
    hipLaunchKernelGGL(box_sensor_indices, dim3(grid_for(count)), dim3(256), 0, s->stream, d, B, count, s->sensLin);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) BFD_FAIL(-10, std::string("bfd_set_sensor_box: ") + hipGetErrorString(e));
    s->sensIsBox = sensor_box_form_allowed();
    if (nSensors) *nSensors = s->nSensors;
    return 0;
}

int64_t bfd_num_sensors(bfd_sim *s) { return s ? s->nSensors : -1; }
int32_t bfd_num_sensor_steps(bfd_sim *s) { return s ? s->nTs : -1; }

int bfd_get_sensor_index(bfd_sim *s, uint32_t *index)
{
    if (!s || (!index && s->nSensors)) BFD_FAIL(-1, "bfd_get_sensor_index: null argument");
    if ((long)s->d.N1 * s->d.N2 * s->d.N3 >= (1L << 32) - 1) BFD_FAIL(-2, "domain too large for 32-bit sensor indices");
    if (!s->nSensors) return 0;
    BFD_HIP(hipSetDevice(s->cfg.device));
    bfd_advise_result_buffer(index, (size_t)s->nSensors * sizeof(uint32_t));
    BFD_HIP(hipMemcpy(index, s->sensLin, (size_t)s->nSensors * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const uint32_t off = (uint32_t)((size_t)s->d.k0 * s->d.plane + 1);
    for (int64_t v = 0; v < s->nSensors; v++) index[v] += off;
    return 0;
}

int bfd_get_sensors(bfd_sim *s, float *out)
{
    if (!s) BFD_FAIL(-1, "null sim");
    return bfd_sensors_into(s, out, (int64_t)s->nTs * (int64_t)s->nSensors);
}

static int download_volume(bfd_sim *s, const float *devXfast, float *out, int64_t s1, int64_t s2, int64_t s3)
{
    const bfd_dev &d = s->d;
    if (s1 < 0 || s2 < 0 || s3 < 0) BFD_FAIL(-2, "negative strides are not supported");
    const size_t span = span_elems(d.N1, d.N2, d.nk, s1, s2, s3);
    DevTemp<float> tmp;
    BFD_HIP(tmp.alloc(span));
    hipError_t e = hipSuccess;
    bfd_advise_result_buffer(out, span * sizeof(float));
    if (span != s->nloc) {   // non-dense view: keep what the caller has in the gaps
        e = hipMemcpyAsync(tmp, out, span * sizeof(float), hipMemcpyHostToDevice, s->stream);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(scatter_from_xfast, dim3(grid_for((long)s->nloc)), dim3(256), 0, s->stream, devXfast, tmp.p,
                           (long)s1, (long)s2, (long)s3, d.N1, d.N2, d.nk);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = copy_out_large(s->cfg.device, out, tmp, span * sizeof(float), s->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) BFD_FAIL(-10, std::string("download: ") + hipGetErrorString(e));
    return 0;
}

static void expand_if_collapsed(bfd_sim *s)
{
    if (s->d.cssRow) return;        // compact solid state: Sxx, Syy, Rxx, Ryy full-volume are not output scratch (they may host the compact arrays); bfd_get_field builds its outputs in a temporary
    if (s->classesReady)
        hipLaunchKernelGGL(expand_normal, dim3(grid_for((long)s->nloc)), dim3(256), 0, s->stream, s->d, (long)s->nloc);
}

int bfd_get_map(bfd_sim *s, int32_t kind, int32_t map, float *out, int64_t s1, int64_t s2, int64_t s3)
{
    if (!s || !out) BFD_FAIL(-1, "bfd_get_map: null argument");
    BFD_HIP(hipSetDevice(s->cfg.device));
    int q = -1;
    for (int a = 0; a < s->nSelR; a++) if (s->selR[a] == map) q = a;
    if (kind != BFD_KIND_LAST && q < 0) BFD_FAIL(-2, "bfd_get_map: map was not selected in selMapsRMS");
    if (kind != BFD_KIND_RMS && kind != BFD_KIND_PEAK && kind != BFD_KIND_LAST) BFD_FAIL(-2, "bfd_get_map: bad kind");
    if (kind == BFD_KIND_RMS && !s->acc) BFD_FAIL(-2, "bfd_get_map: RMS was not selected (SelRMSorPeak)");
    if (kind == BFD_KIND_PEAK && !s->pk) BFD_FAIL(-2, "bfd_get_map: peak was not selected (SelRMSorPeak)");
    if (kind == BFD_KIND_LAST && (map < 0 || map >= BFD_MAP_COUNT)) BFD_FAIL(-2, "bfd_get_map: bad map id");
    if (kind != BFD_KIND_LAST) { const int rf = flush_pending(s); if (rf) return rf; }
    if (kind == BFD_KIND_PEAK) return download_volume(s, s->pk + (size_t)q * s->nloc, out, s1, s2, s3);
    DevTemp<float> tmp;      // the finalised map
    BFD_HIP(tmp.alloc(s->nloc));
    if (kind == BFD_KIND_RMS) {
        const int nAcc = s->step - s->accStart;
        hipLaunchKernelGGL(finalize_rms, dim3(grid_for((long)s->nloc)), dim3(256), 0, s->stream, s->acc + (size_t)q * s->nloc, tmp.p,
                           (long)s->nloc, (float)(nAcc > 0 ? nAcc : 1));
    } else {
        if (map >= BFD_MAP_SIGMAXX && map <= BFD_MAP_SIGMAZZ) expand_if_collapsed(s);
        hipLaunchKernelGGL(last_map, dim3(grid_for((long)s->nloc)), dim3(256), 0, s->stream, s->d, map, tmp.p, (long)s->nloc);
    }
    return download_volume(s, tmp, out, s1, s2, s3);
}

int bfd_get_field(bfd_sim *s, int32_t a, float *out, int64_t s1, int64_t s2, int64_t s3)
{
    if (!s || !out || a < 0 || a > 14) BFD_FAIL(-1, "bfd_get_field: bad argument");
    BFD_HIP(hipSetDevice(s->cfg.device));
    expand_if_collapsed(s);
    const bfd_dev &d = s->d;
    static const int cssOf[15] = {-1, -1, -1, 0, 1, -1, 2, 3, 4, 5, 6, -1, 7, 8, 9};
    if (d.cssRow && cssOf[a] >= 0) {       // not on tilesReady: a setter at step > 0 clears that flag, but list, row table and compact arrays stay as they are until the next step rebuilds them
        // compact solid state: the field is assembled in a temporary -- zeros, the Szz / Rzz copy at the fluid cells (Sxx, Syy, Rxx, Ryy), the compact
        // values at the listed cells
        const float *comp[10] = {d.cSxx, d.cSyy, d.cSxy, d.cSxz, d.cSyz, d.cRxx, d.cRyy, d.cRxy, d.cRxz, d.cRyz};
        DevTemp<float> tmp(true);
        BFD_HIP(tmp.alloc(s->nloc));
        hipError_t e = hipMemsetAsync(tmp, 0, s->nloc * sizeof(float), s->stream);
        if (e == hipSuccess && (a == 3 || a == 4 || a == 9 || a == 10))
            hipLaunchKernelGGL(copy_at_fluid_cells, dim3(grid_for((long)s->nloc)), dim3(256), 0, s->stream, d, a >= 9 ? (const float *)d.Rzz : (const float *)d.Szz, tmp.p, (long)s->nloc);
        bfd_launch_css_scatter(s->stream, s->tiles.shearCells, s->tiles.nShear, comp[cssOf[a]], tmp);
        if (e != hipSuccess) BFD_FAIL(-10, std::string("bfd_get_field: ") + hipGetErrorString(e));
        return download_volume(s, tmp, out, s1, s2, s3);
    }
    if (a >= 12 && s->tilesReady && s->cfg.kernelVariant != 1) bfd_launch_scatter_shear_memory(s->d, s->stream, &s->tiles);   // Rxy, Rxz, Ryz live beside the sparse list
    float *cur[15] = {d.Vx, d.Vy, d.Vz, d.Sxx, d.Syy, d.Szz, d.Sxy, d.Sxz, d.Syz, d.Rxx, d.Ryy, d.Rzz, d.Rxy, d.Rxz, d.Ryz};
    return download_volume(s, cur[a], out, s1, s2, s3);
}


int bfd_get_sensor_dft(bfd_sim *s, double freq, float *outReIm, float *outPeak)
{
    if (!s) BFD_FAIL(-1, "null sim");
    const size_t n = (size_t)s->nSelS * (size_t)s->nSensors;
    if (!n || s->nTs <= 0) return 0;
    if (!outReIm || !(s->sensOut || s->dftAcc)) BFD_FAIL(-1, "bfd_get_sensor_dft: null argument");
    BFD_HIP(hipSetDevice(s->cfg.device));
    const int bin = dft_bin(s->nTs, s->cfg.dt * s->cfg.sensorSub, freq);
    bfd_advise_result_buffer(outReIm, 2 * n * sizeof(float));
    bfd_advise_result_buffer(outPeak, n * sizeof(float));
    if (s->dftAcc) {         // accumulated in the loop
        if (bin != s->dftBin) BFD_FAIL(-2, "bfd_get_sensor_dft: with sensorMode 1 the bin is the one of the sim's own frequency");
        DevTemp<float> dre;
        BFD_HIP(dre.alloc(2 * n));
        hipLaunchKernelGGL(finalize_sensor_dft, dim3(grid_for((long)(2 * n))), dim3(256), 0, s->stream, s->dftAcc, dre.p, (long)(2 * n), 2.0 / (double)s->nTs);
        hipError_t e = hipMemcpyAsync(outReIm, dre, 2 * n * sizeof(float), hipMemcpyDeviceToHost, s->stream);
        if (e == hipSuccess && outPeak) e = hipMemcpyAsync(outPeak, s->dftPk, n * sizeof(float), hipMemcpyDeviceToHost, s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) BFD_FAIL(-10, std::string("bfd_get_sensor_dft: ") + hipGetErrorString(e));
        return 0;
    }
    DevTemp<float> dre, dpk;
    BFD_HIP(dre.alloc(2 * n));
    hipError_t e = dpk.alloc(n);
    for (int q = 0; q < s->nSelS && e == hipSuccess; q++) {      // device block is [q][nTs][nSensors]
        hipLaunchKernelGGL(dft_series, dim3(grid_for(s->nSensors)), dim3(256), 0, s->stream,
                           s->sensOut + (size_t)q * s->nTs * s->nSensors, 1L, (long)s->nSensors, (long)s->nSensors, s->nTs, bin,
                           dre + 2 * (size_t)q * s->nSensors, dpk + (size_t)q * s->nSensors);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(outReIm, dre, 2 * n * sizeof(float), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && outPeak) e = hipMemcpyAsync(outPeak, dpk, n * sizeof(float), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) BFD_FAIL(-10, std::string("bfd_get_sensor_dft: ") + hipGetErrorString(e));
    return 0;
}

int bfd_dft_series(int32_t device, int64_t nSensors, int32_t nTs, const float *series, double dtSensor, double freq,
                   float *outReIm, float *outPeak)
{
    if (nSensors < 0 || nTs <= 0 || (nSensors && (!series || !outReIm))) BFD_FAIL(-1, "bfd_dft_series: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) BFD_FAIL(-3, "bfd_dft_series: no HIP device available (no CPU fallback)");
    if (device < 0 || device >= ndev) BFD_FAIL(-3, "bfd_dft_series: device ordinal out of range");
    if (!nSensors) return 0;
    BFD_HIP(hipSetDevice(device));
    const size_t n = (size_t)nSensors;
    DevTemp<float> din, dre, dpk;
    hipError_t e = din.alloc(n * nTs);
    if (e == hipSuccess) e = dre.alloc(2 * n);
    if (e == hipSuccess) e = dpk.alloc(n);
    if (e == hipSuccess) e = hipMemcpy(din, series, n * nTs * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(dft_series, dim3(grid_for((long)n)), dim3(256), 0, 0, din.p, (long)nTs, 1L, (long)n, nTs, dft_bin(nTs, dtSensor, freq), dre.p, dpk.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(outReIm, dre, 2 * n * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && outPeak) e = hipMemcpy(outPeak, dpk, n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) BFD_FAIL(-10, std::string("bfd_dft_series: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
