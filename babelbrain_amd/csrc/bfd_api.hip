// C ABI of libbabelfdtd_hip.so (include/babelfdtd.h): host logic, coefficient preparation, layout conversion,
// sources, tile lists, time stepping. gfx950 only. Sensors, maps and the result getters: bfd_outputs.hip.
//
// Mirrors what BabelIntegrationBASE.py:2338-2365 hands to the reference's solver
// (package BabelViscoFDTD==1.2.4, absent from /root/reference).
#include "bfd_internal.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <thread>
#include <hipcub/hipcub.hpp>

static thread_local std::string g_err;
void bfd_set_error(const std::string &s) { g_err = s; }

// ------------------------------------------------------------------------------------------------
// coefficient preparation (float64, rounded once to float32). DESIGN.md "Material model".
// ------------------------------------------------------------------------------------------------
namespace {

struct HostTables {
    std::vector<float> t;   // 7*nMat: AP,BP,AS2,BS2,invMu,tauS,invRho
    float c1, k2;
    double cmax;
};

// one standard-linear-solid mechanism, tau_sigma = 1/omega:  M(omega) = MR[(1+tau/2) + i tau/2]
void fit_sls(double rho, double c, double alpha, double q, double omega, bool exact, double &MR, double &tau)
{
    if (c <= 0.0) { MR = 0.0; tau = 0.0; return; }
    if (alpha <= 0.0) { MR = rho * c * c; tau = 0.0; return; }
    const double a = alpha / q;
    if (exact) {
        double x = a * c / omega;
        if (x > 0.4) x = 0.4;
        const double theta = 2.0 * atan(x);
        const double tt = tan(theta);
        const double t = 2.0 * tt / (1.0 - tt);
        const double re = 1.0 + 0.5 * t, im = 0.5 * t;
        const double mag = sqrt(re * re + im * im);
        const double ch = cos(0.5 * theta);
        tau = t;
        MR = rho * c * c * ch * ch / mag;
    } else {
        double Q = omega / (2.0 * c * a);
        if (Q < 1.5) Q = 1.5;
        tau = 2.0 / Q;
        MR = rho * c * c;
    }
}

void make_tables(int nMat, const double *matlist, const double *qcorr, double freq, bool exact,
                 double h, double dt, HostTables &T)
{
    const double omega = 2.0 * M_PI * freq;
    const double tauSigma = 1.0 / omega;
    const double dtoh = dt / h;
    const double half = dt / (2.0 * tauSigma);
    const double k2 = (dt / tauSigma) / (1.0 + half);
    T.c1 = (float)((1.0 - half) / (1.0 + half));
    T.k2 = (float)k2;
    T.t.assign(7 * (size_t)nMat, 0.0f);
    float *AP = T.t.data(), *BP = AP + nMat, *AS2 = BP + nMat, *BS2 = AS2 + nMat;
    float *invMu = BS2 + nMat, *tauS = invMu + nMat, *invRho = tauS + nMat;
    T.cmax = 0.0;
    for (int m = 0; m < nMat; m++) {
        const double *r = matlist + 5 * m;
        const double q = qcorr ? qcorr[m] : 1.0;
        double MRp, tauP, MRs, tauSh;
        fit_sls(r[0], r[1], r[3], q, omega, exact, MRp, tauP);
        fit_sls(r[0], r[2], r[4], q, omega, exact, MRs, tauSh);
        AP[m] = (float)(MRp * (1.0 + tauP) * dtoh);
        BP[m] = (float)(MRp * tauP * dtoh * k2);
        AS2[m] = (float)(2.0 * MRs * (1.0 + tauSh) * dtoh);
        BS2[m] = (float)(2.0 * MRs * tauSh * dtoh * k2);
        invMu[m] = (MRs > 0.0) ? (float)(1.0 / (MRs * dtoh)) : 0.0f;
        tauS[m] = (float)tauSh;
        invRho[m] = (float)(dtoh / r[0]);
        const double cu = sqrt(MRp * (1.0 + tauP) / r[0]);
        T.cmax = std::max(T.cmax, cu);
    }
}

void cpml_one(double depth, double d0, double amax, double dt, float &a, float &b)
{
    if (depth <= 0.0) { a = 0.0f; b = 0.0f; return; }
    if (depth > 1.0) depth = 1.0;
    const double d = d0 * depth * depth;
    const double al = amax * (1.0 - depth);
    const double bb = exp(-(d + al) * dt);
    b = (float)bb;
    a = (float)(d / (d + al) * (bb - 1.0));
}

// aI,bI at integer positions, aH,bH at half positions; see DESIGN.md "Absorbing layer"
void cpml_axis(int N, int ND, double cmax, double h, double dt, double freq, double R, float *out4N)
{
    const double d0 = -3.0 * cmax * log(R) / (2.0 * ND * h);
    const double amax = M_PI * freq;
    float *aI = out4N, *bI = aI + N, *aH = bI + N, *bH = aH + N;
    for (int i = 0; i < N; i++) {
        const double li = (double)(ND - i) / ND, lh = ((double)(ND - i) - 0.5) / ND;
        const double ri = (double)(i - (N - 1 - ND)) / ND, rh = ((double)(i - (N - 1 - ND)) + 0.5) / ND;
        cpml_one(std::max(li, ri), d0, amax, dt, aI[i], bI[i]);
        cpml_one(std::max(lh, rh), d0, amax, dt, aH[i], bH[i]);
    }
}

// ------------------------------------------------------------------------------------------------
// aux kernels
// ------------------------------------------------------------------------------------------------
// strided caller layout -> x-fastest device layout. One thread per destination voxel.
// MODE 0: material ids (value must be < limit, else *flag = 1); MODE 1: boolean (value != 0)
template <int MODE, typename TO>
__global__ void gather_to_xfast(const uint32_t *__restrict__ in, long s1, long s2, long s3, TO *__restrict__ out,
                                int N1, int N2, int nk, int kSrcOffset, int kSrcMin, int kSrcMax, uint32_t limit, int *flag)
{
    const long n = (long)N1 * N2 * nk;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long)gridDim.x * blockDim.x) {
        const int i = (int)(v % N1);
        const int j = (int)((v / N1) % N2);
        int k = (int)(v / ((long)N1 * N2)) + kSrcOffset;
        k = min(max(k, kSrcMin), kSrcMax);   // replicate missing ghost planes
        const uint32_t x = in[i * s1 + j * s2 + k * s3];
        if (MODE == 0) {
            if (x >= limit) *flag = 1;
            out[v] = (TO)x;
        } else {
            out[v] = (TO)(x != 0u);
        }
    }
}
__global__ void or_reflector(const uint32_t *__restrict__ in, long s1, long s2, long s3, uint16_t *__restrict__ mat,
                             int N1, int N2, int nk, int clear)
{
    const long n = (long)N1 * N2 * nk;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long)gridDim.x * blockDim.x) {
        uint16_t m = mat[v] & BFD_MAT_MASK;
        if (!clear) {
            const int i = (int)(v % N1), j = (int)((v / N1) % N2), k = (int)(v / ((long)N1 * N2));
            if (in[i * s1 + j * s2 + k * s3]) m |= BFD_REFLECTOR_BIT;
        }
        mat[v] = m;
    }
}
__global__ void transpose_pulse(const double *__restrict__ in, float *__restrict__ out, int nSrc, int L)
{   // in [nSrc][L] f64 -> out [L][nSrc] f32
    const long n = (long)nSrc * L;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long)gridDim.x * blockDim.x) {
        const int s = (int)(v % nSrc);
        const long t = v / nSrc;
        out[v] = (float)in[(long)s * L + t];
    }
}

// sources. typeSource 0/1: velocity (after the velocity half-step), 2/3: normal stresses (after the stress half-step).
// One body for both source forms; the value policy gives the float32 source value of a row at the current step.
struct DenseValue {            // the dense table: row `step` of the [step][source] float32 table
    const float *__restrict__ pulseAtStep;
    __device__ float operator()(uint32_t r) const { return pulseAtStep[r]; }
};
template <int K>
struct SeparableValue {        // sum_k w[r*K + k] * sig_k(step), in that order (no contraction: -ffp-contract=off)
    const float *__restrict__ w; float sig[K];
    __device__ float operator()(uint32_t r) const
    {
        const float *wr = w + (size_t)r * K;
        float acc = wr[0] * sig[0];
#pragma unroll
        for (int k = 1; k < K; k++) acc = acc + wr[k] * sig[k];
        return acc;
    }
};

template <class Value>
__device__ void inject_body(const bfd_dev &d, int typeSource, const uint32_t *__restrict__ lin, const uint32_t *__restrict__ row,
                            const float *__restrict__ wx, const float *__restrict__ wy, const float *__restrict__ wz,
                            const Value &value, long nVox)
{
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < nVox; s += (long)gridDim.x * blockDim.x) {
        const long c = lin[s];
        const float val = value(row[s]);
        const float x = wx ? wx[s] : 1.0f;
        if (typeSource >= 2) {
            const float v = val * x;
            float *pxx = d.Sxx + c, *pyy = d.Syy + c;
            if (d.cssRow) {         // compact solid state: a listed cell's Sxx, Syy live in the list; elsewhere nobody reads them (fluid cells keep Szz only) and
                const long e = css_index(d, c);      // the full-volume arrays are not to be written: they may host the compact ones
                pxx = e >= 0 ? d.cSxx + e : nullptr; pyy = e >= 0 ? d.cSyy + e : nullptr;
            }
            if (typeSource == 2) { if (pxx) { *pxx = *pxx + v; *pyy = *pyy + v; } d.Szz[c] = d.Szz[c] + v; }
            else { if (pxx) { *pxx = v; *pyy = v; } d.Szz[c] = v; }
        } else {
            const float y = wy ? wy[s] : 1.0f, z = wz ? wz[s] : 1.0f;
            if (typeSource == 0) { d.Vx[c] = d.Vx[c] + val * x; d.Vy[c] = d.Vy[c] + val * y; d.Vz[c] = d.Vz[c] + val * z; }
            else { d.Vx[c] = val * x; d.Vy[c] = val * y; d.Vz[c] = val * z; }
        }
    }
}

__global__ void inject_sources(bfd_dev d, int typeSource, const uint32_t *__restrict__ lin, const uint32_t *__restrict__ row,
                               const float *__restrict__ wx, const float *__restrict__ wy, const float *__restrict__ wz,
                               const float *__restrict__ pulseAtStep, long nVox)
{
    inject_body(d, typeSource, lin, row, wx, wy, wz, DenseValue{pulseAtStep}, nVox);
}

// graph replay: the step counter lives on the device
__global__ void inject_sources_at(bfd_dev d, int typeSource, const uint32_t *__restrict__ lin, const uint32_t *__restrict__ row,
                                  const float *__restrict__ wx, const float *__restrict__ wy, const float *__restrict__ wz,
                                  const float *__restrict__ pulseT, const int *__restrict__ stepDev, int nSources, int lengthSource, long nVox)
{
    const int step = *stepDev;
    if (step >= lengthSource) return;
    inject_body(d, typeSource, lin, row, wx, wy, wz, DenseValue{pulseT + (size_t)step * nSources}, nVox);
}

// separable source: sigAtStep = the K signal values of this step ([step][K] table); the same address for every lane
template <int K>
__global__ void inject_sources_sep(bfd_dev d, int typeSource, const uint32_t *__restrict__ lin, const uint32_t *__restrict__ row,
                                   const float *__restrict__ wx, const float *__restrict__ wy, const float *__restrict__ wz,
                                   const float *__restrict__ weights, const float *__restrict__ sigAtStep, long nVox)
{
    SeparableValue<K> v; v.w = weights;
#pragma unroll
    for (int k = 0; k < K; k++) v.sig[k] = sigAtStep[k];
    inject_body(d, typeSource, lin, row, wx, wy, wz, v, nVox);
}

template <int K>
__global__ void inject_sources_sep_at(bfd_dev d, int typeSource, const uint32_t *__restrict__ lin, const uint32_t *__restrict__ row,
                                      const float *__restrict__ wx, const float *__restrict__ wy, const float *__restrict__ wz,
                                      const float *__restrict__ weights, const float *__restrict__ signals, const int *__restrict__ stepDev,
                                      int lengthSource, long nVox)
{
    const int step = *stepDev;
    if (step >= lengthSource) return;
    SeparableValue<K> v; v.w = weights;
#pragma unroll
    for (int k = 0; k < K; k++) v.sig[k] = signals[(size_t)step * K + k];
    inject_body(d, typeSource, lin, row, wx, wy, wz, v, nVox);
}

__global__ void set_step(int *stepDev, int v) { *stepDev = v; }
__global__ void advance_step(int *stepDev) { *stepDev = *stepDev + 1; }


// separable injection with K terms: at host step `step`, or (stepDev != null, graph replay) at the device's step counter
template <int K>
void launch_inject_sep_k(hipStream_t st, const bfd_dev &view, int typeSource, const uint32_t *lin, const uint32_t *row, const float *wx,
                         const float *wy, const float *wz, const float *weights, const float *signals, int step, const int *stepDev,
                         int lengthSource, long n)
{
    if (stepDev)
        hipLaunchKernelGGL(inject_sources_sep_at<K>, dim3(grid_for(n)), dim3(256), 0, st, view, typeSource, lin, row, wx, wy, wz,
                           weights, signals, stepDev, lengthSource, n);
    else
        hipLaunchKernelGGL(inject_sources_sep<K>, dim3(grid_for(n)), dim3(256), 0, st, view, typeSource, lin, row, wx, wy, wz,
                           weights, signals + (size_t)step * K, n);
}
void launch_inject_separable(int K, hipStream_t st, const bfd_dev &view, int typeSource, const uint32_t *lin, const uint32_t *row,
                             const float *wx, const float *wy, const float *wz, const float *weights, const float *signals, int step,
                             const int *stepDev, int lengthSource, long n)
{
    switch (K) {
    case 1: launch_inject_sep_k<1>(st, view, typeSource, lin, row, wx, wy, wz, weights, signals, step, stepDev, lengthSource, n); break;
    case 2: launch_inject_sep_k<2>(st, view, typeSource, lin, row, wx, wy, wz, weights, signals, step, stepDev, lengthSource, n); break;
    case 3: launch_inject_sep_k<3>(st, view, typeSource, lin, row, wx, wy, wz, weights, signals, step, stepDev, lengthSource, n); break;
    default: launch_inject_sep_k<4>(st, view, typeSource, lin, row, wx, wy, wz, weights, signals, step, stepDev, lengthSource, n); break;
    }
}

// inputs changed: a recorded step graph holds stale pointers
static void drop_step_graph(bfd_sim *s)
{
    if (s->stepGraph) { hipGraphExecDestroy(s->stepGraph); s->stepGraph = nullptr; }
    if (s->graphState == 1) s->graphState = 0;
    s->stepDevValid = false;
}

// number of non-zero edge coefficients A (active shear updates) in the sparse shear list
__global__ void count_active_edges(const float *__restrict__ coef, const unsigned *__restrict__ codes, long n, unsigned long long *__restrict__ out)
{
    unsigned c = 0, x = 0;          // out[0] active edges, out[1] edges with explicit coefficients
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
        c += (coef[6 * t] != 0.f) + (coef[6 * t + 2] != 0.f) + (coef[6 * t + 4] != 0.f);
        const unsigned w = codes[t];
        x += ((w & 255u) == 255u) + (((w >> 8) & 255u) == 255u) + (((w >> 16) & 255u) == 255u);
    }
    if (c) atomicAdd(out, (unsigned long long)c);
    if (x) atomicAdd(out + 1, (unsigned long long)x);
}

// ---- streamed source table -------------------------------------------------------------------------------------------
// tile t = steps [t*TS, min((t+1)*TS, L)) of the caller's [nSources][L] float64 table -> pinned [steps][nSources] float32
// (the same float64 -> float32 rounding the resident path applies on the device). Row blocks keep reads and writes in cache.
void pack_tile_rows(const double *pulse, int nSources, int L, int t0, int len, float *out, int r0, int r1)
{
    const int RB = 64;
    for (int rb = r0; rb < r1; rb += RB) {
        const int re = std::min(rb + RB, r1);
        for (int q = 0; q < len; q++) {
            float *o = out + (size_t)q * nSources;
            for (int r = rb; r < re; r++) o[r] = (float)pulse[(size_t)r * L + t0 + q];
        }
    }
}
void pack_tile(const double *pulse, int nSources, int L, int TS, int t, float *out)
{
    const int t0 = t * TS, len = std::min(TS, L - t0);
    const int nth = (size_t)nSources * len > (1u << 20) ? 4 : 1;
    if (nth == 1) { pack_tile_rows(pulse, nSources, L, t0, len, out, 0, nSources); return; }
    std::vector<std::thread> th;
    for (int a = 0; a < nth; a++) {
        const int r0 = (int)((long)nSources * a / nth) / 64 * 64, r1 = a + 1 == nth ? nSources : (int)((long)nSources * (a + 1) / nth) / 64 * 64;
        th.emplace_back(pack_tile_rows, pulse, nSources, L, t0, len, out, r0, r1);
    }
    for (auto &x : th) x.join();
}

void drain_pack_jobs(bfd_sim *s)
{
    for (int b = 0; b < 2; b++) if (s->packJob[b].valid()) s->packJob[b].wait();
}

void release_streaming(bfd_sim *s)
{
    drain_pack_jobs(s);
    for (int b = 0; b < 2; b++) {
        if (s->packJob[b].valid()) s->packJob[b].get();
        dev_release(s, &s->tileDev[b]);
        if (s->tilePinned[b]) { hipHostFree(s->tilePinned[b]); s->tilePinned[b] = nullptr; }
        s->tileLoaded[b] = s->tilePacked[b] = -1; s->evTileUsed[b] = false; s->evReadUsed[b][0] = s->evReadUsed[b][1] = false;
    }
    s->pulseHost = nullptr; s->tileSteps = s->nTiles = 0;
}

// the float32 [nSources] row of source values for time step `step`, resident on the device when the kernels of stream st
// run: either a row of the resident table or of the time tile that holds the step (uploaded here when the run enters it)
int pulse_row(bfd_sim *s, int step, hipStream_t st, const float **row)
{
    if (!s->pulseHost) { *row = s->pulseT + (size_t)step * s->nSources; return 0; }
    const int TS = s->tileSteps, t = step / TS, b = t & 1;
    if (s->tileLoaded[b] != t) {
        if (s->tilePacked[b] == t && s->packJob[b].valid()) s->packJob[b].get();
        else {           // first tile, or the run jumped (bfd_reset): pack it here
            if (s->packJob[b].valid()) s->packJob[b].get();
            if (s->evTileUsed[b]) BFD_HIP(hipEventSynchronize(s->evTile[b]));
            pack_tile(s->pulseHost, s->nSources, s->lengthSource, TS, t, s->tilePinned[b]);
            s->tilePacked[b] = t;
        }
        const int len = std::min(TS, s->lengthSource - t * TS);
        // the kernels that read the tile this buffer held two tiles ago may have run on another stream (split half-steps):
        // the copy waits for the last of them
        for (int q = 0; q < 2; q++) if (s->evReadUsed[b][q]) BFD_HIP(hipStreamWaitEvent(st, s->evRead[b][q], 0));      // the readers on the engine's stream and on a caller's side stream
        BFD_HIP(hipMemcpyAsync(s->tileDev[b], s->tilePinned[b], (size_t)len * s->nSources * sizeof(float), hipMemcpyHostToDevice, st));
        BFD_HIP(hipEventRecord(s->evTile[b], st));
        s->evTileUsed[b] = true; s->tileLoaded[b] = t;
        // the next tile is packed beside the GPU's work on this one (the pinned buffer is free once its last upload is done)
        const int nb = b ^ 1, nt = t + 1;
        if (nt < s->nTiles && s->tilePacked[nb] != nt) {
            if (s->packJob[nb].valid()) s->packJob[nb].get();
            s->tilePacked[nb] = nt;
            const bool waitEv = s->evTileUsed[nb];
            hipEvent_t ev = s->evTile[nb];
            const int dev = s->cfg.device;
            const double *ph = s->pulseHost; const int nS = s->nSources, L = s->lengthSource; float *dst = s->tilePinned[nb];
            s->packJob[nb] = std::async(std::launch::async, [=]() {
                if (waitEv) { hipSetDevice(dev); hipEventSynchronize(ev); }
                pack_tile(ph, nS, L, TS, nt, dst);
            });
        }
    } else {
        BFD_HIP(hipStreamWaitEvent(st, s->evTile[b], 0));      // a part launched on another stream than the upload
    }
    *row = s->tileDev[b] + (size_t)(step - t * TS) * s->nSources;
    return 0;
}

// after the kernels of stream st that read the row pulse_row() returned: the tile buffer may be overwritten behind them
void pulse_row_read(bfd_sim *s, int step, hipStream_t st)
{
    if (!s->pulseHost) return;
    // one event per buffer and stream kind: the parts of a split half-step run on two streams at the same time, and a single
    // event recorded by both would keep only the later record
    const int b = (step / s->tileSteps) & 1, q = st == s->stream ? 0 : 1;
    if (s->evRead[b][q] && hipEventRecord(s->evRead[b][q], st) == hipSuccess) s->evReadUsed[b][q] = true;
}

}  // namespace

int sel_list(uint32_t mask, int *sel)
{
    int n = 0;
    for (int b = 0; b < BFD_MAP_COUNT; b++) if (mask & (1u << b)) sel[n++] = b;
    return n;
}

void bfd_launch_gather_flags(const bfd_sim *s, const uint32_t *in, long s1, long s2, long s3, uint8_t *flags)
{
    const bfd_dev &d = s->d;
    hipLaunchKernelGGL((gather_to_xfast<1, uint8_t>), dim3(grid_for((long)s->nloc)), dim3(256), 0, s->stream,
                       in, s1, s2, s3, flags, d.N1, d.N2, d.nk, 0, 0, d.nk - 1, 0u, (int *)nullptr);
}

hipError_t select_flagged(uint8_t *flags, uint32_t *sel, int *dcount, int n, hipStream_t st, DevTemp<char> &work)
{
    size_t wbytes = 0;
    hipcub::CountingInputIterator<uint32_t> ids(0);
    hipError_t e = hipcub::DeviceSelect::Flagged(nullptr, wbytes, ids, flags, sel, dcount, n, st);
    if (e == hipSuccess) e = work.alloc(std::max<size_t>(wbytes, 1));
    if (e == hipSuccess) e = hipcub::DeviceSelect::Flagged((void *)work.p, wbytes, ids, flags, sel, dcount, n, st);
    return e;
}

// inputs changed: the run lists, the activity map and a recorded step graph are out of date, and (classes: materials, map, reflector) the cell classes
static void invalidate_lists(bfd_sim *s, bool classes = true) { s->tilesReady = false; if (classes) s->classesReady = false; s->actReady = false; drop_step_graph(s); }
// Advanced Vz: between the stress and the velocity half-step of a time step the runs that carry BFD_RUN_ADV_VZ hold the new Vz at their inner planes
// and the old one elsewhere; only the velocity half-step over the SAME lists completes it. What would rebuild the lists waits for the step to end.
static bool lists_held_mid_step(const bfd_sim *s) { return s->midStep && s->tilesReady && s->tiles.advVz; }
#define BFD_REFUSE_MID_STEP(who) do { if (lists_held_mid_step(s)) BFD_FAIL(-6, who ": a stress half-step is outstanding: finish the time step first"); } while (0)

static int pressure_slot(const bfd_sim *s)
{
    int qP = -1;
    for (int q = 0; q < s->nSelR; q++) if (s->selR[q] == BFD_MAP_PRESSURE) qP = q;
    return qP;
}
// paired accumulation (see "paired accumulation" below): the slot of the Pressure map, and the flush of the outstanding step.
// st: the stream the following launches go to (default: the engine's); bfd_outputs.hip calls it too
int flush_pending(bfd_sim *s, hipStream_t st)
{
    if (!s->pendingAcc) return 0;        // also between the half-steps of the second step of a pair: its stress half-step has added both (pairDone)
    s->pendingAcc = false;
    const int qP = pressure_slot(s);
    if (qP < 0 || !s->tilesReady) return 0;
    BFD_HIP(hipSetDevice(s->cfg.device));
    bfd_launch_flush_paired(s->d, st, s->acc ? s->acc + (size_t)qP * s->nloc : nullptr, s->pk ? s->pk + (size_t)qP * s->nloc : nullptr, &s->tiles);
    BFD_HIP(hipGetLastError());
    return 0;
}

hipEvent_t bfd_get_event(bfd_sim *s)
{
    hipEvent_t e;
    if (!s->evPool.empty()) { e = s->evPool.back(); s->evPool.pop_back(); return e; }
    if (hipEventCreate(&e) != hipSuccess) return nullptr;      // callers skip the timing pair
    return e;
}

void bfd_bind_state_views(bfd_sim *s)
{
    bfd_dev &d = s->d;
    const size_t g = 2 * (size_t)d.plane;
    float **fp[15] = {&d.Vx, &d.Vy, &d.Vz, &d.Sxx, &d.Syy, &d.Szz, &d.Sxy, &d.Sxz, &d.Syz, &d.Rxx, &d.Ryy, &d.Rzz, &d.Rxy, &d.Rxz, &d.Ryz};
    for (int a = 0; a < 15; a++) *fp[a] = s->stateBase[a] + g;
    d.mat = s->matBase + g; d.cls = s->clsBase + g;
    d.VxW = d.Vx; d.VyW = d.Vy; d.VzW = d.Vz; d.SzzW = d.Szz; d.RzzW = d.Rzz;      // in-place variants: no second copies
    if (s->pingpong) { d.VxW = s->ppBase[0] + g; d.VyW = s->ppBase[1] + g; d.VzW = s->ppBase[2] + g; d.SzzW = s->ppBase[3] + g; d.RzzW = s->ppBase[4] + g; }
}

void bfd_kmark(bfd_sim *s, int cls, int end, hipStream_t st)
{
    hipEvent_t e = bfd_get_event(s);
    if (!e) return;
    if (!end && (s->evK[cls].size() & 1)) { s->evPool.push_back(e); return; }    // unmatched begin: keep pairs intact
    if (end && !(s->evK[cls].size() & 1)) { s->evPool.push_back(e); return; }
    hipEventRecord(e, st);
    s->evK[cls].push_back(e);
}

// ------------------------------------------------------------------------------------------------
extern "C" {

int bfd_abi_version(void) { return BFD_ABI_VERSION; }
const char *bfd_last_error(void) { return g_err.c_str(); }

int bfd_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int bfd_device_name(int device, char *buf, int buflen)
{
    hipDeviceProp_t p;
    BFD_HIP(hipGetDeviceProperties(&p, device));
    snprintf(buf, buflen, "%s (%s)", p.name, p.gcnArchName);
    return 0;
}

double bfd_stable_dt(int32_t nMat, const double *matlist, const double *qcorr, double freq,
                     int32_t qfactorCorrection, double h, double alphaCFL)
{
    if (nMat <= 0 || !matlist) { bfd_set_error("bfd_stable_dt: no materials"); return -1.0; }
    HostTables T;
    make_tables(nMat, matlist, qcorr, freq, qfactorCorrection != 0, h, 1.0, T);
    // O(2,4) staggered leapfrog: dt <= (6/7) h / (sqrt(3) cmax)
    return alphaCFL * BFD_STAB * h / (sqrt(3.0) * T.cmax);
}

int bfd_material_tables(int32_t nMat, const double *matlist, const double *qcorr, double freq,
                        int32_t qfactorCorrection, double h, double dt, float *tables7, float *c1k2, double *cmax)
{
    if (nMat <= 0 || !matlist) BFD_FAIL(-1, "bfd_material_tables: no materials");
    HostTables T;
    make_tables(nMat, matlist, qcorr, freq, qfactorCorrection != 0, h, dt, T);
    if (tables7) memcpy(tables7, T.t.data(), T.t.size() * sizeof(float));
    if (c1k2) { c1k2[0] = T.c1; c1k2[1] = T.k2; }
    if (cmax) *cmax = T.cmax;
    return 0;
}

int bfd_create(const bfd_config *cfg, bfd_sim **out)
{
    if (!cfg || !out) BFD_FAIL(-1, "bfd_create: null argument");
    const int P = cfg->NDelta + 1;
    if (cfg->N1 < 2 * P + 4 || cfg->N2 < 2 * P + 4 || cfg->N3 < 2 * P + 4)
        BFD_FAIL(-2, "bfd_create: every dimension must be at least 2*(NDelta+1)+4 voxels");
    if (cfg->k0 < 0 || cfg->nk < 0 || cfg->k0 + cfg->nk > cfg->N3) BFD_FAIL(-2, "bfd_create: slab [k0,k0+nk) outside the domain");
    // the rule of both splitters (slab.partition, partition() in bfd_group.hip): a slab owns the 2 + 2 planes its neighbours read
    if (cfg->nk < 4) BFD_FAIL(-2, "bfd_create: every slab needs at least 4 planes");
    if (cfg->nMat <= 0 || cfg->nMat > (int)BFD_MAT_MASK) BFD_FAIL(-2, "bfd_create: nMat must be in 1..32767");
    if (cfg->sensorSub <= 0 || cfg->sensorStart < 0 || cfg->nt < 0) BFD_FAIL(-2, "bfd_create: bad sensor sampling / nt");
    if (cfg->typeSource < 0 || cfg->typeSource > 3) BFD_FAIL(-2, "bfd_create: TypeSource must be 0..3");
    if (cfg->kernelVariant < 0 || cfg->kernelVariant > 4) BFD_FAIL(-2, "bfd_create: kernelVariant must be 0..4");
    if (cfg->rmsFirstStep < 0) BFD_FAIL(-2, "bfd_create: rmsFirstStep must be >= 0");
    if (cfg->selRMSorPeak < 0 || cfg->selRMSorPeak > 3) BFD_FAIL(-2, "bfd_create: SelRMSorPeak must be 0..3");
    if (cfg->sensorMode < 0 || cfg->sensorMode > 1) BFD_FAIL(-2, "bfd_create: sensorMode must be 0 or 1");
    if ((long)cfg->N1 * cfg->N2 * (cfg->nk + 4) >= (1L << 31)) BFD_FAIL(-2, "bfd_create: slab exceeds 2^31 voxels (split it into Z-slabs)");
    if (!(cfg->h > 0) || !(cfg->dt > 0) || !(cfg->freq > 0) || !(cfg->reflectionLimit > 0 && cfg->reflectionLimit < 1))
        BFD_FAIL(-2, "bfd_create: h, dt, freq must be > 0 and 0 < reflectionLimit < 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        BFD_FAIL(-3, "bfd_create: no HIP device available (this engine has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) BFD_FAIL(-3, "bfd_create: device ordinal out of range");
    BFD_HIP(hipSetDevice(cfg->device));

    bfd_sim *s = new bfd_sim();
    s->cfg = *cfg;
    s->step = 0; s->devBytes = 0; s->haveMaterials = s->haveMap = false; s->tilesReady = false;
    s->nSrcVox = 0; s->srcLin = s->srcRow = nullptr; s->srcW[0] = s->srcW[1] = s->srcW[2] = nullptr; s->pulseT = nullptr;
    s->nSources = s->lengthSource = 0;
    s->pulseHost = nullptr; s->tileSteps = s->nTiles = 0;
    s->srcK = 0; s->srcWeights = s->srcSignals = nullptr;
    for (int b = 0; b < 2; b++) { s->tileDev[b] = s->tilePinned[b] = nullptr; s->tileLoaded[b] = s->tilePacked[b] = -1; s->evTile[b] = nullptr; s->evTileUsed[b] = false; for (int q = 0; q < 2; q++) { s->evRead[b][q] = nullptr; s->evReadUsed[b][q] = false; } }
    s->sensEnt = nullptr; s->sensEntValid = false; s->sensIsBox = false; memset(s->sensBox, 0, sizeof s->sensBox);
    s->actBase = nullptr; s->actBytes = 0; s->actReady = false;
    s->nSensors = 0; s->sensLin = nullptr; s->sensOut = nullptr; s->dftAcc = nullptr; s->dftPk = nullptr; s->dftBin = 0;
    s->acc = s->pk = nullptr; s->timing = s->perKernel = false;
    s->pairEnv = true; s->pendingAcc = s->pairDone = false; s->pairedLaunches = 0;
    if (const char *ev = getenv("BFD_PAIR_ACC")) s->pairEnv = atoi(ev) != 0;      // 0: every step accumulates in the velocity kernels (A/B, tests)
    s->advEnv = true; s->midStep = false; s->tiles.advVz = false;
    if (const char *ev = getenv("BFD_ADV_VZ")) s->advEnv = atoi(ev) != 0;         // 0: velocity_fluid updates Vz of every plane (A/B, tests)
    s->tables = nullptr; s->profiles = nullptr; s->cmax = 0;
    memset(s->algBytes, 0, sizeof s->algBytes); s->tiles.ktimer = nullptr;
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) { delete s; BFD_FAIL(-10, "hipStreamCreate failed"); }
    s->ownStream = true;
    if (hipEventCreate(&s->evBegin) != hipSuccess) { hipStreamDestroy(s->stream); delete s; BFD_FAIL(-10, "hipEventCreate failed"); }
    if (hipEventCreate(&s->evEnd) != hipSuccess) { hipEventDestroy(s->evBegin); hipStreamDestroy(s->stream); delete s; BFD_FAIL(-10, "hipEventCreate failed"); }

    bfd_dev &d = s->d;
    memset(&d, 0, sizeof d);
    d.N1 = cfg->N1; d.N2 = cfg->N2; d.N3 = cfg->N3; d.k0 = cfg->k0; d.nk = cfg->nk;
    d.ND = cfg->NDelta; d.P = P; d.plane = cfg->N1 * cfg->N2;
    s->nloc = (size_t)d.plane * d.nk;
    s->nalloc = (size_t)d.plane * (d.nk + 4);
    bfd_placement_cache_evict_other_sizes(cfg->device, s->nalloc * sizeof(float));

    int rc = 0;
    float **fp[15] = {&d.Vx, &d.Vy, &d.Vz, &d.Sxx, &d.Syy, &d.Szz, &d.Sxy, &d.Sxz, &d.Syz,
                      &d.Rxx, &d.Ryy, &d.Rzz, &d.Rxy, &d.Rxz, &d.Ryz};
    for (int a = 0; a < 15 && !rc; a++) {
        rc = dev_alloc(s, &s->stateBase[a], s->nalloc);
        if (!rc) *fp[a] = s->stateBase[a] + 2 * (size_t)d.plane;
    }
    if (!rc) rc = dev_alloc(s, &s->matBase, s->nalloc);
    if (!rc) d.mat = s->matBase + 2 * (size_t)d.plane;
    if (!rc) rc = dev_alloc(s, &s->clsBase, s->nalloc);
    if (!rc) d.cls = s->clsBase + 2 * (size_t)d.plane;
    s->classesReady = false; s->placementDone = false; s->haloHandedOut = false;
    s->placementMode = 1; s->placementLimit = -1;
    d.VxW = d.Vx; d.VyW = d.Vy; d.VzW = d.Vz; d.SzzW = d.Szz; d.RzzW = d.Rzz;
    // variant 4 (fused fluid time step) needs the old fields to survive the step: second copies of V, Szz, Rzz. A
    // Z-slab keeps the in-place update (its neighbours alias the halo planes once), i.e. behaves like variant 3.
    s->pingpong = cfg->kernelVariant == 4 && cfg->k0 == 0 && cfg->nk == cfg->N3;
    if (s->pingpong) {
        float **wp[5] = {&d.VxW, &d.VyW, &d.VzW, &d.SzzW, &d.RzzW};
        for (int a = 0; a < 5 && !rc; a++) {
            rc = dev_alloc(s, &s->ppBase[a], s->nalloc);
            if (!rc) *wp[a] = s->ppBase[a] + 2 * (size_t)d.plane;
        }
    }
    // CPML memory variables
    const bool zTouch = (d.k0 < P) || (d.k0 + d.nk > d.N3 - P);
    static const int dirOf[18] = {0, 1, 2, 1, 0, 2, 0, 2, 1, 0, 1, 2, 0, 1, 2, 0, 1, 2};
    for (int a = 0; a < 18 && !rc; a++) {
        size_t n = 0;
        if (dirOf[a] == 0) n = (size_t)d.nk * d.N2 * 2 * P;
        else if (dirOf[a] == 1) n = (size_t)d.nk * 2 * P * d.N1;
        else n = zTouch ? (size_t)2 * P * d.plane : 0;
        rc = dev_alloc(s, &d.psi[a], n);
    }
    if (!rc) rc = dev_alloc(s, &s->tables, 7 * (size_t)cfg->nMat);
    if (!rc) rc = dev_alloc(s, &s->profiles, 4 * (size_t)(d.N1 + d.N2 + d.N3));
    s->nSelR = sel_list(cfg->selMapsRMS, s->selR);
    s->nSelS = sel_list(cfg->selMapsSensors, s->selS);
    if (!rc && (cfg->selRMSorPeak & 1) && s->nSelR) rc = dev_alloc(s, &s->acc, (size_t)s->nSelR * s->nloc);
    if (!rc && (cfg->selRMSorPeak & 2) && s->nSelR) rc = dev_alloc(s, &s->pk, (size_t)s->nSelR * s->nloc);
    s->accStart = cfg->rmsFirstStep > 0 ? cfg->rmsFirstStep - 1 : cfg->sensorStart * cfg->sensorSub;
    s->nTs = 0;
    for (int n = 0; n < cfg->nt; n++) if (n % cfg->sensorSub == 0 && n / cfg->sensorSub >= cfg->sensorStart) s->nTs++;
    if (rc) { bfd_destroy(s); return rc; }
    if (hipStreamSynchronize(s->stream) != hipSuccess) { bfd_destroy(s); BFD_FAIL(-10, "bfd_create: sync failed"); }
    *out = s;
    return 0;
}

void bfd_destroy(bfd_sim *s)
{
    if (!s) return;
    hipSetDevice(s->cfg.device);
    hipDeviceSynchronize();
    if (s->stepGraph) hipGraphExecDestroy(s->stepGraph);
    if (s->captureStream) hipStreamDestroy(s->captureStream);
    release_streaming(s);
    for (int b = 0; b < 2; b++) { if (s->evTile[b]) hipEventDestroy(s->evTile[b]); for (int q = 0; q < 2; q++) if (s->evRead[b][q]) hipEventDestroy(s->evRead[b][q]); }
    for (void *p : s->allocs) {
        const bool searched = std::find(s->searched.begin(), s->searched.end(), p) != s->searched.end();
        if (searched && bfd_placement_cache_put(s->cfg.device, s->nalloc * sizeof(float), p)) continue;
        hipFree(p);
    }
    for (hipEvent_t e : s->evPool) hipEventDestroy(e);
    for (hipEvent_t e : s->evStress) hipEventDestroy(e);
    for (hipEvent_t e : s->evVelocity) hipEventDestroy(e);
    for (auto &v : s->evK) for (hipEvent_t e : v) hipEventDestroy(e);
    hipEventDestroy(s->evBegin); hipEventDestroy(s->evEnd);
    if (s->ownStream) hipStreamDestroy(s->stream);
    delete s;
}

int bfd_set_stream(bfd_sim *s, void *hipStream)
{
    if (!s) BFD_FAIL(-1, "null sim");
    BFD_HIP(hipSetDevice(s->cfg.device));
    BFD_HIP(hipStreamSynchronize(s->stream));
    if (s->ownStream) { hipStreamDestroy(s->stream); s->ownStream = false; }
    s->stream = (hipStream_t)hipStream;      // NULL = the device's default (null) stream, which is torch's default too
    return 0;
}

int bfd_use_private_stream(bfd_sim *s)
{
    if (!s) BFD_FAIL(-1, "null sim");
    BFD_HIP(hipSetDevice(s->cfg.device));
    if (s->ownStream) return 0;
    BFD_HIP(hipStreamSynchronize(s->stream));
    BFD_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    s->ownStream = true;
    return 0;
}

int bfd_set_materials(bfd_sim *s, const double *matlist, const double *qcorr)
{
    if (!s || !matlist) BFD_FAIL(-1, "bfd_set_materials: null argument");
    BFD_REFUSE_MID_STEP("bfd_set_materials");
    BFD_HIP(hipSetDevice(s->cfg.device));
    { const int rc = flush_pending(s); if (rc) return rc; }      // inputs set again in the middle of a run: the maps take the outstanding Pressure first
    const bfd_config &c = s->cfg;
    for (int m = 0; m < c.nMat; m++) {
        const double *r = matlist + 5 * m;
        if (!(r[0] > 0) || !(r[1] > 0) || r[2] < 0 || r[3] < 0 || r[4] < 0)
            BFD_FAIL(-2, "bfd_set_materials: need rho>0, cL>0, cS>=0, alpha>=0 in every row");
        if (qcorr && !(qcorr[m] > 0)) BFD_FAIL(-2, "bfd_set_materials: QCorrection must be > 0");
    }
    HostTables T;
    make_tables(c.nMat, matlist, qcorr, c.freq, c.qfactorCorrection != 0, c.h, c.dt, T);
    const double cfl = T.cmax * c.dt / c.h;
    if (cfl > BFD_STAB / sqrt(3.0) * 1.0000001)
        BFD_FAIL(-4, "bfd_set_materials: DT violates the stability limit dt <= (6/7) h / (sqrt(3) cmax)");
    s->cmax = T.cmax;
    BFD_HIP(hipMemcpyAsync(s->tables, T.t.data(), T.t.size() * sizeof(float), hipMemcpyHostToDevice, s->stream));
    bfd_dev &d = s->d;
    const int n = c.nMat;
    d.AP = s->tables; d.BP = d.AP + n; d.AS2 = d.BP + n; d.BS2 = d.AS2 + n;
    d.invMu = d.BS2 + n; d.tauS = d.invMu + n; d.invRho = d.tauS + n;
    d.c1 = T.c1; d.k2 = T.k2;
    std::vector<float> prof(4 * (size_t)(d.N1 + d.N2 + d.N3));
    float *px = prof.data(), *py = px + 4 * d.N1, *pz = py + 4 * d.N2;
    cpml_axis(d.N1, d.ND, T.cmax, c.h, c.dt, c.freq, c.reflectionLimit, px);
    cpml_axis(d.N2, d.ND, T.cmax, c.h, c.dt, c.freq, c.reflectionLimit, py);
    cpml_axis(d.N3, d.ND, T.cmax, c.h, c.dt, c.freq, c.reflectionLimit, pz);
    BFD_HIP(hipMemcpyAsync(s->profiles, prof.data(), prof.size() * sizeof(float), hipMemcpyHostToDevice, s->stream));
    BFD_HIP(hipStreamSynchronize(s->stream));
    const float *bx = s->profiles, *by = bx + 4 * d.N1, *bz = by + 4 * d.N2;
    d.axI = bx; d.bxI = bx + d.N1; d.axH = bx + 2 * d.N1; d.bxH = bx + 3 * d.N1;
    d.ayI = by; d.byI = by + d.N2; d.ayH = by + 2 * d.N2; d.byH = by + 3 * d.N2;
    d.azI = bz; d.bzI = bz + d.N3; d.azH = bz + 2 * d.N3; d.bzH = bz + 3 * d.N3;
    s->haveMaterials = true; invalidate_lists(s);
    return 0;
}

int bfd_set_material_map(bfd_sim *s, const uint32_t *map, int64_t s1, int64_t s2, int64_t s3,
                         int32_t ghostLow, int32_t ghostHigh)
{
    if (!s || !map) BFD_FAIL(-1, "bfd_set_material_map: null argument");
    if (ghostLow < 0 || ghostLow > 2 || ghostHigh < 0 || ghostHigh > 2) BFD_FAIL(-2, "ghost plane counts must be 0..2");
    BFD_REFUSE_MID_STEP("bfd_set_material_map");
    BFD_HIP(hipSetDevice(s->cfg.device));
    { const int rc = flush_pending(s); if (rc) return rc; }
    const bfd_dev &d = s->d;
    // upload the readable span [k=-ghostLow .. nk-1+ghostHigh]
    const uint32_t *base = map - (int64_t)ghostLow * s3;
    const int nkSpan = d.nk + ghostLow + ghostHigh;
    if (s1 < 0 || s2 < 0 || s3 < 0) BFD_FAIL(-2, "negative strides are not supported");
    const size_t span = span_elems(d.N1, d.N2, nkSpan, s1, s2, s3);
    DevTemp<uint32_t> tmp; DevTemp<int> flag; int hflag = 0;
    BFD_HIP(tmp.alloc(span));
    hipError_t e = hipMemcpyAsync(tmp, base, span * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess) e = flag.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(flag, 0, sizeof(int), s->stream);
    if (e == hipSuccess) {
        // destination covers local planes -2..nk+1; source plane index = local k + ghostLow, clamped to the span
        hipLaunchKernelGGL((gather_to_xfast<0, uint16_t>), dim3(grid_for((long)s->nalloc)), dim3(256), 0, s->stream,
                           tmp.p, (long)s1, (long)s2, (long)s3, s->matBase, d.N1, d.N2, d.nk + 4, ghostLow - 2, 0, nkSpan - 1,
                           (uint32_t)s->cfg.nMat, flag.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&hflag, flag, sizeof(int), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) BFD_FAIL(-10, std::string("bfd_set_material_map: ") + hipGetErrorString(e));
    if (hflag) BFD_FAIL(-5, "bfd_set_material_map: MaterialMap holds an id >= number of MaterialList rows");
    s->haveMap = true; invalidate_lists(s);
    return 0;
}

int bfd_set_reflector(bfd_sim *s, const uint32_t *mask, int64_t s1, int64_t s2, int64_t s3)
{
    if (!s) BFD_FAIL(-1, "null sim");
    if (!s->haveMap) BFD_FAIL(-6, "bfd_set_reflector: set the material map first");
    BFD_REFUSE_MID_STEP("bfd_set_reflector");
    BFD_HIP(hipSetDevice(s->cfg.device));
    { const int rc = flush_pending(s); if (rc) return rc; }
    const bfd_dev &d = s->d;
    DevTemp<uint32_t> tmp;
    if (mask) {
        const size_t span = span_elems(d.N1, d.N2, d.nk, s1, s2, s3);
        BFD_HIP(tmp.alloc(span));
        BFD_HIP(hipMemcpyAsync(tmp, mask, span * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    }
    hipLaunchKernelGGL(or_reflector, dim3(grid_for((long)s->nloc)), dim3(256), 0, s->stream, tmp.p, (long)s1, (long)s2, (long)s3,
                       s->matBase + 2 * (size_t)d.plane, d.N1, d.N2, d.nk, mask ? 0 : 1);
    BFD_HIP(hipStreamSynchronize(s->stream));
    invalidate_lists(s);      // reflector cells end the UNI class of their tiles
    return 0;
}

// What both source forms share: checks the voxels, releases the previous sources of either form (device tables, streaming
// buffers, separable weights and signals) and uploads the voxel list sorted by voxel index with its Ox/Oy/Oz weights.
// who = the entry point, for the messages.
static int set_source_voxels(bfd_sim *s, const char *who, int64_t nVox, const uint32_t *localIndex, const uint32_t *row,
                             const float *wx, const float *wy, const float *wz, int32_t nSources, int32_t lengthSource)
{
    BFD_HIP(hipSetDevice(s->cfg.device));
    for (int64_t v = 0; v < nVox; v++) {
        if (localIndex[v] >= s->nloc) BFD_FAIL(-2, std::string(who) + ": voxel index outside the slab");
        if ((int)row[v] >= nSources) BFD_FAIL(-2, std::string(who) + ": SourceMap id exceeds PulseSource rows");
    }
    BFD_HIP(hipStreamSynchronize(s->stream));
    dev_release(s, &s->srcLin); dev_release(s, &s->srcRow); dev_release(s, &s->pulseT);
    release_streaming(s);
    dev_release(s, &s->srcWeights); dev_release(s, &s->srcSignals); s->srcK = 0;
    for (int a = 0; a < 3; a++) dev_release(s, &s->srcW[a]);
    s->nSrcVox = nVox; s->nSources = nSources; s->lengthSource = lengthSource;
    s->srcLowEnd = 0; s->srcHighBeg = nVox; invalidate_lists(s, false);
    if (nVox == 0) return 0;
    // keep the source voxels sorted by voxel index: the boundary/interior split of a half-step injects
    // the sources of the first and last z-chunk separately (build_tile_lists)
    std::vector<int64_t> order((size_t)nVox);
    for (int64_t v = 0; v < nVox; v++) order[v] = v;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return localIndex[a] < localIndex[b]; });
    std::vector<uint32_t> hl((size_t)nVox), hr((size_t)nVox);
    for (int64_t v = 0; v < nVox; v++) { hl[v] = localIndex[order[v]]; hr[v] = row[order[v]]; }
    int rc = 0;
    if ((rc = dev_alloc(s, &s->srcLin, nVox, false))) return rc;
    if ((rc = dev_alloc(s, &s->srcRow, nVox, false))) return rc;
    BFD_HIP(hipMemcpy(s->srcLin, hl.data(), nVox * sizeof(uint32_t), hipMemcpyHostToDevice));
    BFD_HIP(hipMemcpy(s->srcRow, hr.data(), nVox * sizeof(uint32_t), hipMemcpyHostToDevice));
    const float *w[3] = {wx, wy, wz};
    std::vector<float> hw((size_t)nVox);
    for (int a = 0; a < 3; a++) {
        s->srcW[a] = nullptr;
        if (w[a]) {
            if ((rc = dev_alloc(s, &s->srcW[a], nVox, false))) return rc;
            for (int64_t v = 0; v < nVox; v++) hw[v] = w[a][order[v]];
            BFD_HIP(hipMemcpy(s->srcW[a], hw.data(), nVox * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    return 0;
}

int bfd_set_sources(bfd_sim *s, int64_t nVox, const uint32_t *localIndex, const uint32_t *row,
                    const float *wx, const float *wy, const float *wz,
                    const double *pulse, int32_t nSources, int32_t lengthSource)
{
    if (!s) BFD_FAIL(-1, "null sim");
    if (nVox < 0 || (nVox > 0 && (!localIndex || !row || !pulse))) BFD_FAIL(-1, "bfd_set_sources: null argument");
    if (nSources < 0 || lengthSource < 0) BFD_FAIL(-2, "bfd_set_sources: bad PulseSource shape");
    BFD_REFUSE_MID_STEP("bfd_set_sources");
    { const int rc = flush_pending(s); if (rc) return rc; }
    int rc = set_source_voxels(s, "bfd_set_sources", nVox, localIndex, row, wx, wy, wz, nSources, lengthSource);
    if (rc || nVox == 0) return rc;
    const size_t np = (size_t)nSources * lengthSource;
    // Large tables are streamed: the float64 table stays where the caller built it (it must stay valid until the run is
    // over, as it does inside the solver call of the drop-in) and the device holds two time tiles. BFD_SOURCE_TILE=<steps>
    // forces streaming with that tile length (tests).
    int tile = 0;
    if (const char *ev = getenv("BFD_SOURCE_TILE")) tile = atoi(ev);
    if (tile <= 0 && np * sizeof(float) > ((size_t)1 << 30)) tile = 64;
    if (tile > 0 && lengthSource > 0 && nSources > 0) {
        tile = std::min(tile, (int)lengthSource);
        s->pulseHost = pulse; s->tileSteps = tile; s->nTiles = (lengthSource + tile - 1) / tile;
        for (int b = 0; b < 2; b++) {
            hipError_t e = hipSuccess;
            rc = dev_alloc(s, &s->tileDev[b], (size_t)tile * nSources, false);
            if (!rc) e = hipHostMalloc((void **)&s->tilePinned[b], (size_t)tile * nSources * sizeof(float), hipHostMallocDefault);
            if (!rc && e == hipSuccess && !s->evTile[b]) e = hipEventCreateWithFlags(&s->evTile[b], hipEventDisableTiming);
            for (int q = 0; q < 2; q++) if (!rc && e == hipSuccess && !s->evRead[b][q]) e = hipEventCreateWithFlags(&s->evRead[b][q], hipEventDisableTiming);
            if (rc || e != hipSuccess) {        // nothing half-built stays behind: the sim is back to "no sources"
                const std::string why = rc ? std::string(bfd_last_error()) : std::string("bfd_set_sources: ") + hipGetErrorString(e);
                release_streaming(s);
                s->nSrcVox = 0; s->srcHighBeg = 0;
                bfd_set_error(why);
                return rc ? rc : -10;
            }
        }
        s->graphState = -1;        // the recorded step graph indexes a resident table
        return 0;
    }
    if ((rc = dev_alloc(s, &s->pulseT, np, false))) return rc;
    DevTemp<double> tmp;
    BFD_HIP(tmp.alloc(std::max<size_t>(np, 1)));
    BFD_HIP(hipMemcpyAsync(tmp, pulse, np * sizeof(double), hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(transpose_pulse, dim3(grid_for((long)np)), dim3(256), 0, s->stream, tmp.p, s->pulseT, nSources, lengthSource);
    BFD_HIP(hipStreamSynchronize(s->stream));
    return 0;
}

int bfd_set_sources_separable(bfd_sim *s, int64_t nVox, const uint32_t *localIndex, const uint32_t *row,
                              const float *wx, const float *wy, const float *wz,
                              int32_t nSources, int32_t K, const float *weights, int32_t lengthSource, const float *signals)
{
    if (!s) BFD_FAIL(-1, "null sim");
    if (K < 1 || K > 4) BFD_FAIL(-2, "bfd_set_sources_separable: K must be 1..4");
    BFD_REFUSE_MID_STEP("bfd_set_sources_separable");
    { const int rc = flush_pending(s); if (rc) return rc; }
    if (nVox < 0 || (nVox > 0 && (!localIndex || !row || !weights || !signals))) BFD_FAIL(-1, "bfd_set_sources_separable: null argument");
    if (nSources < 0 || lengthSource < 0) BFD_FAIL(-2, "bfd_set_sources_separable: bad weights / signals shape");
    int rc = set_source_voxels(s, "bfd_set_sources_separable", nVox, localIndex, row, wx, wy, wz, nSources, lengthSource);
    if (rc || nVox == 0) return rc;
    // weights [nSources][K] as given; signals [K][lengthSource] -> [lengthSource][K]: the K values of a step side by side
    const size_t nw = (size_t)nSources * K, ns = (size_t)lengthSource * K;
    std::vector<float> sig(ns);
    for (int n = 0; n < lengthSource; n++)
        for (int k = 0; k < K; k++) sig[(size_t)n * K + k] = signals[(size_t)k * lengthSource + n];
    hipError_t e = hipSuccess;
    rc = dev_alloc(s, &s->srcWeights, nw, false);
    if (!rc) rc = dev_alloc(s, &s->srcSignals, ns, false);
    if (!rc && nw) e = hipMemcpy(s->srcWeights, weights, nw * sizeof(float), hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess && ns) e = hipMemcpy(s->srcSignals, sig.data(), ns * sizeof(float), hipMemcpyHostToDevice);
    if (rc || e != hipSuccess) {        // nothing half-built stays behind: the sim is back to "no sources"
        const std::string why = rc ? std::string(bfd_last_error()) : std::string("bfd_set_sources_separable: ") + hipGetErrorString(e);
        dev_release(s, &s->srcWeights); dev_release(s, &s->srcSignals);
        s->nSrcVox = 0; s->srcHighBeg = 0;
        bfd_set_error(why);
        return rc ? rc : -10;
    }
    s->srcK = K;
    return 0;
}

// where the ten compact arrays live (bfd_tiles::cssHosted); called when the list is built and again whenever the state buffers change hands
// (bfd_choose_placement exchanges them at step 0, when everything is still zero)
static void bind_compact_views(bfd_sim *s)
{
    bfd_dev &d = s->d;
    if (!d.cssRow) return;
    float **cp[10] = {&d.cSxx, &d.cSyy, &d.cSxy, &d.cSxz, &d.cSyz, &d.cRxx, &d.cRyy, &d.cRxy, &d.cRxz, &d.cRyz};
    static const int host[10] = {3, 4, 6, 7, 8, 9, 10, 12, 13, 14};      // Sxx Syy Sxy Sxz Syz Rxx Ryy Rxy Rxz Ryz among the 15 state arrays
    for (int a = 0; a < 10; a++)
        *cp[a] = s->tiles.cssHosted ? s->stateBase[host[a]] + 4 * (size_t)d.plane : s->tiles.css + (size_t)a * s->tiles.cssCap;
}
static bool quiet_runs_wanted(const bfd_sim *s);
static bool pair_engine(const bfd_sim *s, bool quiet, int nFluid);
static bool adv_vz_engine(const bfd_sim *s, int nSolid);

// The tile grid of one build: tx x ty columns of nsub sub-tiles (n in all) of SUB planes; a z-chunk, the longest run, is perChunk sub-tiles.
// "boundary" sub-tiles hold the 2 first / 2 last planes of the slab (what a Z-neighbour reads): they form the
// small part 1 of a split half-step; everything else is part 2. lowPlanes / hiStart delimit them in planes.
struct TileGrid {
    int tx, ty, nsub, n, SUB, perChunk, nChunks, nk, lowPlanes, hiStart;
    bool subBnd(int q) const { return q * SUB < lowPlanes || std::min((q + 1) * SUB, nk) > hiStart; }
};
// Not a getter: it chooses the run length of this build and stores it in s->zchunk (bfd_sim keeps the choice; perChunk is derived from it).
static TileGrid choose_tile_grid(bfd_sim *s)
{
    int tx, ty, nsub; bfd_tile_grid(s->d, &tx, &ty, &nsub);
    const int n = tx * ty * nsub;
    const int SUB = bfd_tile_subz();
    // longest run one workgroup marches: 16 planes; 8 on small grids so that the launch still has a few thousand
    // workgroups (measured: 256^3 49 -> 58, 128^3 29 -> 46 Gvoxel-steps/s). 32 was best at 512^3 while the z-chunks of
    // a column were consecutive in the list; under the banded order 16 is 2.5 % faster than 32 and 3 % faster than 8.
    const int t32 = tx * ty * ((s->d.nk + 31) / 32);
    // round 6: the switch point moved from 1500 to 3000 columns (320^3: 8 planes +4 % in water, +7 % with bone -- velocity_solid wants the workgroups; 352^3: +1.5 %;
    // 384^3: 16 planes +4 %; profiles/r6/pml_flavour_cost_and_run_length_mid_size.txt)
    s->zchunk = t32 >= 3000 ? 16 : 8;
    if (const char *ev = getenv("BFD_ZRUN")) { const int z = atoi(ev); if (z >= SUB && z % SUB == 0) s->zchunk = z; }   // tuning experiments
    if (s->zchunk > bfd_tile_zchunk()) s->zchunk = bfd_tile_zchunk();
    const int perChunk = s->zchunk / SUB;
    const int nChunks = (nsub + perChunk - 1) / perChunk;
    const int nkl = s->d.nk;
    const int lowPlanes = std::min(SUB, nkl);
    const int hiStart = std::max(((nkl - 2) / SUB) * SUB, lowPlanes);
    return {tx, ty, nsub, n, SUB, perChunk, nChunks, nkl, lowPlanes, hiStart};
}

// class flags and material of every sub-tile, from the device
static int fetch_tile_classes(bfd_sim *s, int n, std::vector<int> &flags, std::vector<int> &mats)
{
    DevTemp<int> dflags, dmats;
    BFD_HIP(dflags.alloc(n));
    hipError_t e = dmats.alloc(n);
    if (e == hipSuccess) {
        bfd_launch_classify(s->d, s->stream, dflags, dmats);
        e = hipMemcpyAsync(flags.data(), dflags, n * sizeof(int), hipMemcpyDeviceToHost, s->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(mats.data(), dmats, n * sizeof(int), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) BFD_FAIL(-10, std::string("classify tiles: ") + hipGetErrorString(e));
    return 0;
}

// Runs of the fused time step (variant 4, bfd_kernels_fused.hip): 64 x 24 cells = three tiles of this grid in y, a z-run of
// 2 .. fusedSub sub-tiles. A sub-tile qualifies (bit5) when it is fluid, has nothing of the absorbing layer or the domain
// edge within 2 cells (bit6), is not a boundary sub-tile of the slab, and the sources are of velocity type. Per column and
// z-chunk the rows are scanned upwards: where three consecutive tile rows qualify over a z-stretch they form a run and the
// scan moves on by three rows. A run is UNI when every sub-tile is (one material in the grown regions) and lossy when a
// cell of a grown region relaxes (bit7); stretches are cut where that class changes (a single sub-tile joins its neighbour).
static void form_fused_runs(bfd_sim *s, const TileGrid &G, std::vector<int> &flags, const std::vector<int> &mats, std::vector<char> &taken, std::vector<int4> &fused)
{
    const int tx = G.tx, ty = G.ty, nsub = G.nsub, SUB = G.SUB;
    const int fusedSub = 32 / SUB;
    struct FusedRun { int bx, by, q0, q1, cls, mat; };
    std::vector<FusedRun> fruns;
    if (s->pingpong && s->cfg.typeSource < 2) {
        const int FRW = bfd_fused_rows() / 8;
        const size_t layer = (size_t)tx * ty;
        for (int q = 0; q < nsub; q++)
            for (size_t txy = 0; txy < layer; txy++) { int &f = flags[(size_t)q * layer + txy]; if (!(f & 1) && !(f & 64) && !(f & 256) && !G.subBnd(q)) f |= 32; }
        for (int bx = 0; bx < tx; bx++)
            for (int qc = 0; qc < nsub; qc += fusedSub) {
                const int qe = std::min(qc + fusedSub, nsub), L = qe - qc;
                int by = 0;
                while (by + FRW <= ty) {
                    // class of the three rows at every q of the chunk: -1 = not available, else bit0 UNI, bit1 lossy
                    std::vector<int> cls(L, -1);
                    for (int q = qc; q < qe; q++) {
                        bool ok = true; int uni = 1, lossy = 0;
                        const int m0 = mats[(size_t)q * layer + (size_t)by * tx + bx];
                        for (int r = 0; r < FRW; r++) {
                            const size_t id = (size_t)q * layer + (size_t)(by + r) * tx + bx;
                            const int f = flags[id];
                            if (!(f & 32) || taken[id]) ok = false;
                            if (!(f & 4) || mats[id] != m0) uni = 0;
                            if (f & 128) lossy = 1;
                        }
                        if (!uni && s->cfg.nMat > bfd_fused_max_materials()) ok = false;
                        if (ok) cls[q - qc] = uni | (lossy << 1);
                    }
                    bool any = false;
                    int a = 0;
                    while (a < L) {
                        if (cls[a] < 0) { a++; continue; }
                        int b = a; while (b < L && cls[b] >= 0) b++;        // stretch [a, b)
                        if (b - a >= 2) {
                            any = true;
                            // segments of equal class (start, end, class); a segment of one sub-tile joins a neighbour
                            std::vector<std::array<int, 3>> seg;
                            for (int q = a; q < b; q++) {
                                if (seg.empty() || seg.back()[2] != cls[q]) seg.push_back({q, q + 1, cls[q]});
                                else seg.back()[1] = q + 1;
                            }
                            for (size_t u = 0; u < seg.size() && seg.size() > 1;) {
                                if (seg[u][1] - seg[u][0] >= 2) { u++; continue; }
                                const size_t v = u > 0 ? u - 1 : u + 1;      // UNI only if both are, lossy if either is
                                seg[v][0] = std::min(seg[v][0], seg[u][0]); seg[v][1] = std::max(seg[v][1], seg[u][1]);
                                seg[v][2] = (seg[v][2] & seg[u][2] & 1) | ((seg[v][2] | seg[u][2]) & 2);
                                seg.erase(seg.begin() + u);
                                u = 0;
                            }
                            for (const auto &rq : seg) {
                                fruns.push_back({bx, by, qc + rq[0], qc + rq[1], rq[2], mats[(size_t)(qc + rq[0]) * layer + (size_t)by * tx + bx]});
                                for (int q = qc + rq[0]; q < qc + rq[1]; q++)
                                    for (int r = 0; r < FRW; r++) { taken[(size_t)q * layer + (size_t)(by + r) * tx + bx] = 1; s->tiles.nFusedSub++; }
                            }
                        }
                        a = b;
                    }
                    by += any ? FRW : 1;
                }
            }
        // list order like the other runs: eight y-bands, inside a band z-chunk slowest, then row, bx fastest
        auto key = [&](const FusedRun &r) { const long band = (long)r.by * 8 / ty; return ((band * 4096 + r.q0 / fusedSub) * 4096 + r.by) * 4096 + r.bx; };
        std::stable_sort(fruns.begin(), fruns.end(), [&](const FusedRun &x, const FusedRun &y) { return key(x) < key(y); });
        for (const auto &r : fruns) {
            int4 run; run.x = r.by * tx + r.bx; run.y = (r.q0 * SUB) | (std::min(r.q1 * SUB, s->d.nk) << 16);
            run.z = 32 | 16 | ((r.cls & 2) ? 2 : 0) | ((r.cls & 1) ? 4 : 0); run.w = r.mat;
            fused.push_back(run);
        }
    }
}

// The runs of the two-kernel path: fluid boundary / interior (lists[0], [1]), solid boundary / interior (lists[2], [3]) and all of them in list
// order (listsAll: boundary, interior); sub-tiles the fused runs have taken are left out.
static void form_two_kernel_runs(bfd_sim *s, const TileGrid &G, const std::vector<int> &flags, const std::vector<int> &mats, std::vector<char> &taken, std::vector<int4> *lists, std::vector<int4> *listsAll)
{
    const int tx = G.tx, ty = G.ty, nsub = G.nsub, SUB = G.SUB, perChunk = G.perChunk, nChunks = G.nChunks;
    bfd_tiles &T = s->tiles;
    // List order = what is in flight together. The launch gives XCD e the e-th contiguous eighth of the list
    // (remap_block) and an XCD keeps ~100 workgroups in flight, all marching in z at the same pace; a halo line
    // (128 B for 2 or 3 floats of a neighbour tile's row) is an L2 hit only if that neighbour is in flight on the
    // same XCD. Default (2): eight y-bands, inside a band z-chunk slowest, then by, bx fastest -> x neighbours are
    // 1 apart, y neighbours tilesX apart. Measured at 512^3 (rocprofv3 FETCH/WRITE_SIZE, water): stress traffic
    // 3.55 -> 3.10 GB and 79 -> 88 Gvoxel-steps/s against (0) column order (z-chunks of a column consecutive);
    // (1) z-chunk slowest over the whole plane moves as few bytes but piles the absorbing-layer and lossy
    // z-levels onto single XCDs (C3: 75 -> 72). BFD_RUN_ORDER=0/1 select the other orders for experiments.
    std::vector<std::pair<int, int>> seq;       // (column, z-chunk) in list order
    {
        const char *ev = getenv("BFD_RUN_ORDER");
        const int mode = ev ? atoi(ev) : 2;
        if (mode == 1) {            // z-chunk slowest
            for (int c = 0; c < nChunks; c++) for (int txy = 0; txy < tx * ty; txy++) seq.push_back({txy, c});
        } else if (mode == 0) {     // column order
            for (int txy = 0; txy < tx * ty; txy++) for (int c = 0; c < nChunks; c++) seq.push_back({txy, c});
        } else {                    // 8 y-bands (one per XCD part), inside a band z-chunk slowest
            // (the two z-chunks of the absorbing layer first, so that the cheapest workgroups end every XCD's part of the list: no gain, removed;
            // profiles/r4/)
            for (int e = 0; e < 8; e++) {
                const int y0 = (int)((long)ty * e / 8), y1 = (int)((long)ty * (e + 1) / 8);
                for (int c = 0; c < nChunks; c++) for (int by = y0; by < y1; by++) for (int bx = 0; bx < tx; bx++) seq.push_back({by * tx + bx, c});
            }
        }
    }
    for (const auto &pc : seq) {
        const int txy = pc.first, c = pc.second;
        const int sb = c * perChunk, se0 = std::min(sb + perChunk, nsub);
        int q = sb;
        while (q < se0) {
            if (taken[(size_t)q * tx * ty + txy]) { q++; continue; }
            const int f = flags[(size_t)q * tx * ty + txy], m = mats[(size_t)q * tx * ty + txy];
            const bool solid = f & 1;
            const bool bnd = G.subBnd(q);
            int r = q + 1, pmlAny = f & 8;
            while (r < se0) {
                const int f2 = flags[(size_t)r * tx * ty + txy], m2 = mats[(size_t)r * tx * ty + txy];
                if (G.subBnd(r) != bnd || taken[(size_t)r * tx * ty + txy]) break;
                if (solid ? !(f2 & 1) : (((f2 ^ f) & ~(32 | 128 | 256)) != 0 || ((f & 4) && m2 != m))) break;
                pmlAny |= f2 & 8;
                r++;
            }
            const int kbeg = q * SUB, kend = std::min(r * SUB, s->d.nk);
            // solid runs: bit0 + bit3 (a sub-tile of the run touches the absorbing layer)
            int4 run; run.x = txy; run.y = kbeg | (kend << 16); run.z = solid ? (1 | pmlAny) : (f & ~(32 | 128 | 256)); run.w = m;
            lists[(solid ? 2 : 0) + (bnd ? 0 : 1)].push_back(run);
            listsAll[bnd ? 0 : 1].push_back(run);
            for (int u = q; u < r; u++) {
                taken[(size_t)u * tx * ty + txy] = 1;
                if (solid) T.nSolidSub++;
                else { if (f & 2) T.nLossy++; else T.nLossless++; if (f & 4) T.nUni++; if (f & 8) T.nPml++; if (f & 16) T.nLean++; }
            }
            q = r;
        }
    }
    // solid runs that touch the absorbing layer go to the two ends of the solid list: [boundary: PML | plain][interior: plain | PML]
    auto isPml = [](const int4 &r) { return (r.z & 8) != 0; };
    auto mid = std::stable_partition(lists[2].begin(), lists[2].end(), isPml);
    T.nSolidBP = (int)(mid - lists[2].begin());
    auto mid2 = std::stable_partition(lists[3].begin(), lists[3].end(), [&](const int4 &r) { return !isPml(r); });
    T.nSolidIP = (int)(lists[3].end() - mid2);
}

// Cost-balanced block -> run maps (experiment, BFD_XCD_BALANCE=1; default off). A launch's blocks go to the 8 XCDs round-robin and every
// XCD works through its own blocks at its own pace (-DBFD_EXP_XCD_CLOCK build: block b always runs on XCD (x0 + b) mod 8). With equal
// COUNTS per XCD (remap_block) the XCD that holds the short boundary runs is idle for the last fifth of every fluid launch and the bands
// with more tissue finish last. Here the contiguous parts of the list are cut by estimated cost instead (planes + prologue, weighted by
// the bytes per cell of the run's class), the launch gets 8 x (longest part) blocks and a block beyond its part returns at once.
// Measured: the ends of the XCDs move together (spread 19 % -> 13 % of a launch) and the step time does not -- C3 +1.2 %, shear medium
// -0.4 %, other weightings +-2 % either way: an XCD that runs dry leaves its share of the memory system to the others.
// profiles/r4/xcd_balance.txt.
static int build_balance_maps(bfd_sim *s, const std::vector<int4> &all)
{
    bfd_tiles &T = s->tiles;
    bool on = false;
    if (const char *ev = getenv("BFD_XCD_BALANCE")) on = atoi(ev) != 0 && s->cfg.kernelVariant != 2 && s->cfg.kernelVariant != 1;
    memset(s->tiles.xmapH, 0, sizeof s->tiles.xmapH);
    if (on) {
        const double wPml = 0.25, wLossy = 8, wMulti = 2, wRun = 2.0;
        // cost of run r for kernel class c: 0 fluid stress, 1 fluid velocity, 2 solid stress, 3 solid velocity
        auto cost = [&](const int4 &r, int c) {
            const double planes = (double)((r.y >> 16) - (r.y & 0xFFFF)) + wRun;
            const int f = r.z;
            double w;
            if (c == 0) w = 20 + ((f & 2) ? wLossy : 0) + ((f & 4) ? 0 : wMulti);
            else if (c == 1) w = 36 + ((f & 4) ? 0 : wMulti);
            else w = 40;
            if (f & 8) w *= 1.0 + wPml;
            return planes * w;
        };
        auto make = [&](int m, size_t a0, size_t a1, int c) {
            int *seg = s->tiles.xmapH[m];
            const size_t n = a1 > a0 ? a1 - a0 : 0;
            std::vector<double> cum(n + 1, 0.0);
            for (size_t i = 0; i < n; i++) cum[i + 1] = cum[i] + cost(all[a0 + i], c);
            int maxcnt = 0;
            seg[0] = 0;
            for (int x = 1; x <= 8; x++) {
                const double target = cum[n] * x / 8.0;
                size_t j = std::lower_bound(cum.begin(), cum.end(), target) - cum.begin();
                if (j > n || x == 8) j = n;
                if ((int)j < seg[x - 1]) j = seg[x - 1];
                seg[x] = (int)j;
                maxcnt = std::max(maxcnt, seg[x] - seg[x - 1]);
            }
            seg[9] = std::max(maxcnt, 1);
        };
        const size_t F = T.nFluid, FB = T.nFluidB, S0 = F, SB = T.nSolidB, SN = T.nSolid;
        for (int c = 0; c < 2; c++) {            // fluid stress (c = 0), fluid velocity (c = 1): parts 0, 1, 2
            const int m = c == 0 ? BFD_XM_SF : BFD_XM_VF;
            make(m + 0, 0, F, c); make(m + 1, 0, FB, c); make(m + 2, FB, F, c);
        }
        make(BFD_XM_SS + 0, S0, S0 + SN, 2); make(BFD_XM_SS + 1, S0, S0 + SB, 2); make(BFD_XM_SS + 2, S0 + SB, S0 + SN, 2);
        const size_t bp = T.nSolidBP, ip = T.nSolidIP;          // solid list = [boundary: PML | plain][interior: plain | PML]
        make(BFD_XM_VS + 0, S0 + bp, S0 + SN - ip, 3); make(BFD_XM_VS + 1, S0 + bp, S0 + SB, 3); make(BFD_XM_VS + 2, S0 + SB, S0 + SN - ip, 3);
        make(BFD_XM_VSP_LO, S0, S0 + bp, 3); make(BFD_XM_VSP_HI, S0 + SN - ip, S0 + SN, 3);
        make(BFD_XM_FUSED, S0 + SN, S0 + SN + T.nFused, 0);
        const int rc = dev_alloc(s, &s->tiles.xmap, (size_t)BFD_XMAP_COUNT * 10, false);
        if (rc) return rc;
        BFD_HIP(hipMemcpy(s->tiles.xmap, s->tiles.xmapH, sizeof s->tiles.xmapH, hipMemcpyHostToDevice));
    }
    return 0;
}

// sparse shear list: cells with a solid centre, ascending index (hostCells), in list order on the device, + their edge coefficients;
// decides whether the solid state is compact
static int build_shear_list(bfd_sim *s, const TileGrid &G, int *countOut, bool *compactOut, std::vector<unsigned> &hostCells)
{
    DevTemp<unsigned char> flag; DevTemp<unsigned> sel; DevTemp<int> dcount; DevTemp<char> work;
    hipError_t e = flag.alloc(s->nloc);
    if (e == hipSuccess) e = sel.alloc(s->nloc);
    if (e == hipSuccess) e = dcount.alloc(1);
    int count = 0, rc = 0;
    if (e == hipSuccess) {
        bfd_launch_mark_solid(s->d, s->stream, flag, (long)s->nloc);
        e = select_flagged(flag, sel, dcount, (int)s->nloc, s->stream, work);
        if (e == hipSuccess) e = hipMemcpyAsync(&count, dcount, sizeof(int), hipMemcpyDeviceToHost, s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    }
    hostCells.resize((size_t)count);
    if (e == hipSuccess && count) e = hipMemcpy(hostCells.data(), sel, (size_t)count * sizeof(unsigned), hipMemcpyDeviceToHost);
    // list order (bfd_kernels_v2.hip, shear_order_keys): by z-chunk and band of 8 rows, so that the z neighbours a cell gathers were
    // touched one band-plane earlier instead of one whole plane of the shell
    if (e == hipSuccess && count > 0) {
        DevTemp<unsigned long long> k0, k1; DevTemp<unsigned> v1; DevTemp<char> w2; size_t w2b = 0;
        e = k0.alloc((size_t)count);
        if (e == hipSuccess) e = k1.alloc((size_t)count);
        if (e == hipSuccess) e = v1.alloc((size_t)count);
        if (e == hipSuccess) {
            bfd_launch_shear_order_keys(s->d, s->stream, sel, k0, count, G.lowPlanes, G.hiStart);
            e = hipcub::DeviceRadixSort::SortPairs(nullptr, w2b, k0.p, k1.p, sel.p, v1.p, count, 0, 46, s->stream);
        }
        if (e == hipSuccess) e = w2.alloc(std::max<size_t>(w2b, 1));
        if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs((void *)w2.p, w2b, k0.p, k1.p, sel.p, v1.p, count, 0, 46, s->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(sel, v1, (size_t)count * 4, hipMemcpyDeviceToDevice, s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    }
    // Compact solid state (bfd_dev::cssRow): Sxx, Syy, the shear stresses and the five memory variables Rxx, Ryy, Rxy, Rxz, Ryz of the listed cells in
    // list order. Needs the row-contiguous list order. In a Z-slab the ghost planes of Sxz / Syz stay in the
    // full-volume arrays (the sparse kernel keeps full-volume copies of the planes a neighbour reads, the velocity kernel takes ghost planes from
    // there): the halo exchange is unchanged. BFD_COMPACT_SOLID=0 keeps the full-volume arrays.
    bool compact = count > 0 && s->d.N1 <= 4095;
    if (const char *ev = getenv("BFD_COMPACT_SOLID")) compact = compact && atoi(ev) != 0;
    if (e == hipSuccess) {
        rc = dev_alloc(s, &s->tiles.shearCells, (size_t)std::max(count, 1), false);
        if (!rc) rc = dev_alloc(s, &s->tiles.shearCoef, 6 * (size_t)std::max(count, 1), false);
        if (!rc && !compact) rc = dev_alloc(s, &s->tiles.shearR, 3 * (size_t)std::max(count, 1), true);      // lists are built at step 0: the memory variables start at zero (compact form: they are among the compact arrays)
        if (!rc && count) e = hipMemcpyAsync(s->tiles.shearCells, sel, (size_t)count * sizeof(unsigned), hipMemcpyDeviceToDevice, s->stream);
        if (!rc) rc = dev_alloc(s, &s->tiles.shearCodes, (size_t)std::max(count, 1), false);
        if (!rc) rc = dev_alloc(s, &s->tiles.shearTab, 8 * (size_t)s->cfg.nMat, false);
        if (!rc && e == hipSuccess) bfd_launch_shear_coefficients(s->d, s->stream, s->tiles.shearCells, s->tiles.shearCoef, s->tiles.shearCodes, s->tiles.shearTab, s->cfg.nMat, count);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    }
    if (e != hipSuccess) BFD_FAIL(-10, std::string("shear list: ") + hipGetErrorString(e));
    if (rc) return rc;
    s->tiles.nShear = count;
    if (s->step > 0 && s->tiles.shearR) { bfd_launch_gather_shear_memory(s->d, s->stream, &s->tiles); BFD_HIP(hipStreamSynchronize(s->stream)); }
    *countOut = count; *compactOut = compact;
    return 0;
}

// compact solid state: the row table, the ten arrays (hosted in the full-volume buffers or in a block of their own) and the combined run list
static int setup_compact_state(bfd_sim *s, const TileGrid &G, int count, const std::vector<int4> *listsAll)
{
    const int stride = G.tx + 1;
    int rc = dev_alloc(s, &s->tiles.cssRow, (size_t)(s->d.nk + 4) * s->d.N2 * stride, false);
    // the compact arrays live inside the full-volume buffers of their fields when the listed cells fit between the planes a Z-neighbour
    // exchanges (local planes 0, 1 and nk-2, nk-1 of Sxz / Syz travel: allocation planes 4 .. nk-1 are free); BFD_COMPACT_HOSTED=0 or
    // too many solid cells: one block of their own
    bool hosted = (size_t)count <= (size_t)std::max(s->d.nk - 4, 0) * s->d.plane;
    if (const char *ev = getenv("BFD_COMPACT_HOSTED")) hosted = hosted && atoi(ev) != 0;
    if (!rc && !hosted) rc = dev_alloc(s, &s->tiles.css, 10 * (size_t)count, true);
    if (rc) return rc;
    s->tiles.cssCap = count; s->tiles.cssHosted = hosted;
    bfd_launch_css_row_table(s->d, s->stream, s->tiles.shearCells, count, s->tiles.cssRow, stride, G.lowPlanes, G.hiStart);
    s->d.cssRow = s->tiles.cssRow; s->d.cssStride = stride;
    bind_compact_views(s);
    BFD_HIP(hipStreamSynchronize(s->stream));
    std::vector<int4> ra(listsAll[0]);
    ra.insert(ra.end(), listsAll[1].begin(), listsAll[1].end());
    rc = dev_alloc(s, &s->tiles.runsAll, ra.size(), false);
    if (rc) return rc;
    BFD_HIP(hipMemcpy(s->tiles.runsAll, ra.data(), ra.size() * sizeof(int4), hipMemcpyHostToDevice));
    s->tiles.nAllB = (int)listsAll[0].size(); s->tiles.nAll = (int)ra.size();
    return 0;
}

// a compact state set aside before a rebuild in the middle of a run: the values of the old list into the new one (or, should the new state not be compact -- the
// form was switched off, or no solid run is left and build_tile_lists calls with count 0 -- into the full-volume arrays)
static int carry_compact_in(bfd_sim *s, int count, const unsigned *oldCells, long oldN, const float *oldComp)
{
    DevTemp<float> tmp(true);
    const size_t g = 2 * (size_t)s->d.plane;
    float *newComp[10] = {s->d.cSxx, s->d.cSyy, s->d.cSxy, s->d.cSxz, s->d.cSyz, s->d.cRxx, s->d.cRyy, s->d.cRxy, s->d.cRxz, s->d.cRyz};
    float *full[10] = {s->d.Sxx, s->d.Syy, s->d.Sxy, s->d.Sxz, s->d.Syz, s->d.Rxx, s->d.Ryy, s->d.Rxy, s->d.Rxz, s->d.Ryz};
    hipError_t e2 = s->d.cssRow ? tmp.alloc(s->nalloc) : hipSuccess;
    // the new state is not compact (no solid cell left, or the form was switched off): the full-volume arrays take over, and the owned planes
    // of buffers that hosted compact arrays hold list-ordered values, not fields: cleared before the old values are scattered into them
    for (int a = 0; a < 10 && e2 == hipSuccess && !s->d.cssRow; a++) e2 = hipMemsetAsync(full[a], 0, s->nloc * sizeof(float), s->stream);
    for (int a = 0; a < 10 && e2 == hipSuccess; a++) {
        if (s->d.cssRow) {
            e2 = hipMemsetAsync(tmp, 0, s->nalloc * sizeof(float), s->stream);
            bfd_launch_css_scatter(s->stream, oldCells, oldN, oldComp + (size_t)a * oldN, tmp + g);
            bfd_launch_css_gather(s->stream, s->tiles.shearCells, count, tmp + g, newComp[a]);
        } else bfd_launch_css_scatter(s->stream, oldCells, oldN, oldComp + (size_t)a * oldN, full[a]);
    }
    if (e2 == hipSuccess) e2 = hipStreamSynchronize(s->stream);
    if (e2 != hipSuccess) BFD_FAIL(-10, std::string("compact solid state, list rebuilt in the middle of a run: ") + hipGetErrorString(e2));
    if (!s->d.cssRow && s->tiles.shearR) { bfd_launch_gather_shear_memory(s->d, s->stream, &s->tiles); BFD_HIP(hipStreamSynchronize(s->stream)); }
    return 0;
}

// algorithmic bytes per launch and kernel class (DESIGN.md "Kernels": per-cell byte tables of the tile classes):
// what each kernel has to move once per half-step if every value were fetched exactly once -- float32 fields 4 B,
// material ids 2 B; absorbing-layer memory variables, tables and halo re-reads excluded
static int account_algorithmic_bytes(bfd_sim *s, int tx, const std::vector<int4> &all)
{
    bfd_tiles &T = s->tiles;
    double (*B)[BFD_K_COUNT] = s->algBytes;
    memset(s->algBytes, 0, sizeof s->algBytes);
    const int N1 = s->d.N1, N2 = s->d.N2, N3 = s->d.N3, ND = s->d.ND, k0g = s->d.k0;
    // class counts over the cells of the solid runs (fluid / solid centre, with / without memory variables, active edges)
    unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
    if (T.nSolid && s->cfg.kernelVariant != 2) {
        DevTemp<unsigned long long> dc;
        BFD_HIP(dc.alloc(6));
        hipMemsetAsync(dc, 0, sizeof cnt, s->stream);
        bfd_launch_count_solid_cells(s->d, s->stream, s->tiles.runs + T.nFluid, T.nSolid, dc);
        hipMemcpyAsync(cnt, dc, sizeof cnt, hipMemcpyDeviceToHost, s->stream);
        const hipError_t e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) BFD_FAIL(-10, std::string("solid cell counts: ") + hipGetErrorString(e));
    }
    auto overlap = [](int a, int b, int lo, int hi) { return (double)std::max(0, std::min(b, hi) - std::max(a, lo)); };
    const bool pairAcc = pair_engine(s, quiet_runs_wanted(s), T.nFluid);      // the predicate the launches follow (pairing_step)
    for (size_t r = 0; r < all.size(); r++) {
        const int4 &run = all[r];
        const int bx = run.x % tx, by = run.x / tx, kb = run.y & 0xFFFF, ke = run.y >> 16, f = run.z;
        const int xa = bx * 64, xb = std::min(xa + 64, N1), ya = by * 8, yb = std::min(ya + 8, N2);
        const double cells = (double)(xb - xa) * (yb - ya) * (ke - kb);
        const double inner = overlap(xa, xb, ND, N1 - ND) * overlap(ya, yb, ND, N2 - ND) * overlap(k0g + kb, k0g + ke, ND, N3 - ND);
        const bool fusedRun = r >= (size_t)(T.nFluid + T.nSolid);
        if (fusedRun) {          // 64 x 24 cells per plane, all outside the absorbing layer: V, Szz (Rzz) read and written once per step (+ ids)
            const double fc = 64.0 * bfd_fused_rows() * (ke - kb);
            const double b = 32.0 + ((f & 2) ? 8.0 : 0.0) + ((f & 4) ? 0.0 : 2.0);
            B[0][BFD_K_FUSED] += b * fc; B[1][BFD_K_FUSED] += b * fc + 8.0 * fc;
        } else if (r < (size_t)T.nFluid) {
            const bool lossy = f & 2, uni = f & 4, single = (f & 16) != 0;
            double bs = 12.0 + 8.0 + (lossy ? 8.0 : 0.0) + (uni ? 0.0 : 2.0);
            if (!single) bs += 8.0 + (lossy ? 8.0 : 0.0);
            const double bv = 4.0 + 24.0 + (uni ? 0.0 : 2.0);
            for (int a = 0; a < 2; a++) { B[a][BFD_K_STRESS_FLUID] += bs * cells; B[a][BFD_K_VELOCITY_FLUID] += bv * cells; }
            // Pressure sum read and written: by velocity_fluid in every accumulating step, or (paired accumulation) by stress_fluid in
            // every second one: 4 B per launch averaged over a step pair
            if (pairAcc) B[1][BFD_K_STRESS_FLUID] += 4.0 * inner; else B[1][BFD_K_VELOCITY_FLUID] += 8.0 * inner;
            // advanced Vz: planes kbeg+1 .. kend-3 of the run get their new Vz from stress_fluid (a write; the read is in its 12 B of V already)
            // and velocity_fluid neither reads nor writes it there
            if (f & BFD_RUN_ADV_VZ) {
                const double advCells = (double)(xb - xa) * (yb - ya) * std::max(0, ke - kb - 3);
                for (int a = 0; a < 2; a++) { B[a][BFD_K_STRESS_FLUID] += 4.0 * advCells; B[a][BFD_K_VELOCITY_FLUID] -= 8.0 * advCells; }
            }
        } else if (s->cfg.kernelVariant == 2) {     // dense: V + 6 S + 6 R read, 6 S + 6 R written, id; 6 S + V read, V written, id
            for (int a = 0; a < 2; a++) { B[a][BFD_K_STRESS_SOLID] += 110.0 * cells; B[a][BFD_K_VELOCITY_SOLID] += 50.0 * cells + (a ? 8.0 * inner : 0.0); }
        } else {                                    // class-predicated solid kernels: per-cell terms come from the class counts below
            for (int a = 0; a < 2; a++) B[a][BFD_K_VELOCITY_SOLID] += (a ? 8.0 * inner : 0.0);
        }
    }
    if (T.nSolid && s->cfg.kernelVariant != 2) {
        // stress: V 12 + id 2 + class 1, + Szz r/w 8 (+ Rzz r/w 8) at a fluid cell, + 3 S r/w 24 + 3 R r/w 24 at a solid one
        // (a reflector cell: 48 B of zero stores); velocity: V r/w 24 + ids 2 + class 1 + Szz 4, + Sxx, Syy 8 at a solid cell,
        // + 4 per active shear edge
        const double nF0 = (double)cnt[0], nF1 = (double)cnt[1], nS = (double)cnt[2] + (double)cnt[3], nE = (double)cnt[4], nR = (double)cnt[5];
        const double all = nF0 + nF1 + nS + nR;
        const double bs = 15.0 * all + 8.0 * nF0 + 16.0 * nF1 + 48.0 * nS + 48.0 * nR;
        const double bv = 31.0 * all + 8.0 * (nS + nR) + 4.0 * nE;
        // compact solid state: the fluid kernel takes Szz / Rzz of the solid runs too (V 12 + id 2, + Szz r/w 8 (+ Rzz r/w 8); no class byte), the
        // sparse kernel Sxx, Syy, Rxx, Ryy of its cells (+ 32 + id 2 per listed cell, below)
        const double bsf = 14.0 * all + 8.0 * nF0 + 16.0 * nF1 + 16.0 * nS + 8.0 * nR;
        for (int a = 0; a < 2; a++) { if (s->d.cssRow) B[a][BFD_K_STRESS_FLUID] += bsf; else B[a][BFD_K_STRESS_SOLID] += bs; B[a][BFD_K_VELOCITY_SOLID] += bv; }
    }
    if (s->tiles.nShear) {       // sparse shear: cell index + 6 coefficients + V of the cell + read-modify-write of S and R per active edge
        DevTemp<unsigned long long> dc; unsigned long long hc[2] = {0, 0};
        BFD_HIP(dc.alloc(2));
        hipMemsetAsync(dc, 0, sizeof hc, s->stream);
        hipLaunchKernelGGL(count_active_edges, dim3(grid_for(s->tiles.nShear)), dim3(256), 0, s->stream, s->tiles.shearCoef, s->tiles.shearCodes, s->tiles.nShear, dc.p);
        hipMemcpyAsync(hc, dc, sizeof hc, hipMemcpyDeviceToHost, s->stream);
        const hipError_t e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) BFD_FAIL(-10, std::string("shear edge count: ") + hipGetErrorString(e));
        s->tiles.nShearExplicit = (long)hc[1];
        // per listed cell: index 4 + edge codes 4 + V 12; per edge with explicit coefficients 8; per active edge S and R r/w 16; compact solid
        // state: + Sxx, Syy, Rxx, Ryy r/w 32 (+ the cell's id 2 when it does not fit the code word's fourth byte)
        const double perCell = s->d.cssRow ? (s->cfg.nMat <= 255 ? 52.0 : 54.0) : 20.0;
        for (int a = 0; a < 2; a++) B[a][BFD_K_STRESS_SHEAR] = perCell * (double)s->tiles.nShear + 8.0 * (double)hc[1] + 16.0 * (double)hc[0];
    }
    return 0;
}

// Build the run lists of the tiled kernels (bfd_kernels_v2.hip). Sub-tiles of 64 x 8 x 8 cells are
// classified on the device; consecutive sub-tiles of one (bx,by) column with identical class merge into
// runs that never cross a 32-plane chunk boundary. Variant 2: every sub-tile counts as solid (dense kernels).
static int build_tile_lists(bfd_sim *s)
{
    // a list rebuilt in the middle of a run (inputs set again at step > 0): the shear memory variables travel through the
    // full-volume arrays
    const bool carryShearMemory = s->step > 0 && s->tilesReady == false && s->tiles.shearR && s->tiles.nShear > 0;
    if (carryShearMemory) { bfd_launch_scatter_shear_memory(s->d, s->stream, &s->tiles); BFD_HIP(hipStreamSynchronize(s->stream)); }
    // the same for a compact solid state: its ten arrays are set aside with their list (the full-volume buffers may host the compact arrays
    // themselves) and re-entered into the new list through one full-volume temporary, array by array, once that list exists
    const bool carryCompact = s->step > 0 && s->d.cssRow && s->tiles.nShear > 0;
    unsigned *oldCells = nullptr; DevTemp<float> oldComp; const long oldN = s->tiles.nShear;
    if (carryCompact) {
        float *src[10] = {s->d.cSxx, s->d.cSyy, s->d.cSxy, s->d.cSxz, s->d.cSyz, s->d.cRxx, s->d.cRyy, s->d.cRxy, s->d.cRxz, s->d.cRyz};
        BFD_HIP(oldComp.alloc(10 * (size_t)oldN));
        for (int a = 0; a < 10; a++) BFD_HIP(hipMemcpyAsync(oldComp + (size_t)a * oldN, src[a], (size_t)oldN * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
        BFD_HIP(hipStreamSynchronize(s->stream));
        oldCells = s->tiles.shearCells; s->tiles.shearCells = nullptr;       // released below, after the new list has taken the values over
    }
    s->sensEntValid = false;
    s->d.cssRow = nullptr; s->d.cSxx = s->d.cSyy = s->d.cSxy = s->d.cSxz = s->d.cSyz = s->d.cRxx = s->d.cRyy = s->d.cRxy = s->d.cRxz = s->d.cRyz = nullptr;
    dev_release(s, &s->tiles.cssRow); dev_release(s, &s->tiles.css); s->tiles.cssCap = 0; s->tiles.cssHosted = false;
    dev_release(s, &s->tiles.runsAll); s->tiles.nAll = s->tiles.nAllB = 0;
    dev_release(s, &s->tiles.runs); dev_release(s, &s->tiles.xmap); dev_release(s, &s->tiles.shearCells); dev_release(s, &s->tiles.shearCoef); dev_release(s, &s->tiles.shearR);    // lists of an earlier build
    dev_release(s, &s->tiles.shearCodes); dev_release(s, &s->tiles.shearTab);
    const TileGrid G = choose_tile_grid(s);
    std::vector<int> flags(G.n, 1), mats(G.n, 0);
    if (s->cfg.kernelVariant != 2) { const int rc = fetch_tile_classes(s, G.n, flags, mats); if (rc) return rc; }
    bfd_tiles &T = s->tiles;
    T.nMat = s->cfg.nMat;
    T.nFluid = T.nFluidB = T.nSolid = T.nSolidB = T.nSolidBP = T.nSolidIP = T.nFused = T.nLossless = T.nLossy = T.nSolidSub = T.nUni = T.nPml = T.nLean = T.nFusedSub = 0;
    s->d.tilesX = G.tx; s->d.tilesY = G.ty;
    // Every fluid sub-tile is LEAN (bit4): fluid cells keep a single copy of their identical normal stresses, whatever
    // tile they sit in and whatever reads them (bfd_dev::cls)
    if (s->cfg.kernelVariant != 2) for (int id = 0; id < G.n; id++) if (!(flags[id] & 1)) flags[id] |= 16;
    std::vector<int4> lists[5];      // fluid boundary, fluid interior, solid boundary, solid interior, fused fluid
    std::vector<int4> listsAll[2];   // every run of the two-kernel path in list order: boundary, interior (bfd_tiles::runsAll)
    std::vector<char> taken((size_t)G.n, 0);
    form_fused_runs(s, G, flags, mats, taken, lists[4]);
    form_two_kernel_runs(s, G, flags, mats, taken, lists, listsAll);
    T.nFluidB = (int)lists[0].size(); T.nFluid = T.nFluidB + (int)lists[1].size();
    T.nSolidB = (int)lists[2].size(); T.nSolid = T.nSolidB + (int)lists[3].size();
    T.nFused = (int)lists[4].size();
    T.advVz = false;
    if (adv_vz_engine(s, T.nSolid))
        for (int a = 0; a < 2; a++)
            for (int4 &run : lists[a])
                if (!(run.z & (1 | 8)) && (run.y >> 16) - (run.y & 0xFFFF) >= 4) { run.z |= BFD_RUN_ADV_VZ; T.advVz = true; }
    std::vector<int4> all;
    for (int a = 0; a < 5; a++) all.insert(all.end(), lists[a].begin(), lists[a].end());
    int rc = dev_alloc(s, &s->tiles.runs, all.size(), false);
    if (rc) return rc;
    BFD_HIP(hipMemcpy(s->tiles.runs, all.data(), all.size() * sizeof(int4), hipMemcpyHostToDevice));
    rc = build_balance_maps(s, all);
    if (rc) return rc;
    s->tiles.nShearExplicit = 0;
    s->tiles.nShear = s->tiles.shearLowEnd = s->tiles.shearHighBeg = 0;
    if (T.nSolid && s->cfg.kernelVariant != 2) {     // variant 2 stays monolithic and fully dense
        int count = 0; bool compact = false; std::vector<unsigned> hostCells;
        rc = build_shear_list(s, G, &count, &compact, hostCells);
        if (!rc && compact) rc = setup_compact_state(s, G, count, listsAll);
        if (!rc && carryCompact) rc = carry_compact_in(s, count, oldCells, oldN, oldComp);
        if (!rc && compact && s->step > 0 && !carryCompact) {
            // the first solid cells of a run in progress (they may only appear where every field is zero, include/babelfdtd.h): the compact arrays
            // start at zero. Hosted, they lie in full-volume buffers that an all-fluid engine uses as output scratch (expand_if_collapsed).
            float *comp[10] = {s->d.cSxx, s->d.cSyy, s->d.cSxy, s->d.cSxz, s->d.cSyz, s->d.cRxx, s->d.cRyy, s->d.cRxy, s->d.cRxz, s->d.cRyz};
            for (int a = 0; a < 10; a++) BFD_HIP(hipMemsetAsync(comp[a], 0, (size_t)count * sizeof(float), s->stream));
            BFD_HIP(hipStreamSynchronize(s->stream));
        }
        if (rc) return rc;
        s->tiles.shearLowEnd = std::lower_bound(hostCells.begin(), hostCells.end(), (unsigned)G.lowPlanes * (unsigned)s->d.plane) - hostCells.begin();
        s->tiles.shearHighBeg = std::lower_bound(hostCells.begin(), hostCells.end(), (unsigned)G.hiStart * (unsigned)s->d.plane) - hostCells.begin();
    } else if (carryCompact) {                       // no solid run is left: the full-volume arrays take the old compact values back
        rc = carry_compact_in(s, 0, oldCells, oldN, oldComp);
        if (rc) return rc;
    }
    {   // sources of the first / last z-chunk (bfd_set_sources sorted them by voxel)
        std::vector<uint32_t> lin((size_t)s->nSrcVox);
        if (s->nSrcVox) BFD_HIP(hipMemcpy(lin.data(), s->srcLin, lin.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        s->srcLowEnd = std::lower_bound(lin.begin(), lin.end(), (uint32_t)G.lowPlanes * (uint32_t)s->d.plane) - lin.begin();
        s->srcHighBeg = std::lower_bound(lin.begin(), lin.end(), (uint32_t)G.hiStart * (uint32_t)s->d.plane) - lin.begin();
    }
    rc = account_algorithmic_bytes(s, G.tx, all);
    if (rc) return rc;
    if (oldCells) dev_release(s, &oldCells);
    s->tilesReady = true;
    return 0;
}

// ---- advanced Vz -----------------------------------------------------------------------------------------------------------
// velocity_fluid reads and writes Vz (8 B per cell), yet its Vz update needs only the column's new Szz, which stress_fluid produces plane by plane
// while it holds the column's Vz in its z-queue. In a plain fluid run outside the absorbing layer stress_fluid therefore stores the new Vz of
// the planes whose stencil lies inside the run (kbeg+1 .. kend-3; the range proof is at stress_fluid_body) and velocity_fluid skips Vz there:
// + 4 B and - 8 B per advanced cell. The same expression in the same order (-ffp-contract=off): bit-identical. BFD_ADV_VZ=0 switches it off.
// ONE bit in the run record (BFD_RUN_ADV_VZ), set here when the lists are built, tells both kernels; they cannot disagree. An engine qualifies with
// the class-specialised kernels (variants 0 / 3) updating V in place, velocity-type sources (a stress-type source changes Szz between the two
// kernels), no solid run (velocity_solid and the sparse kernel read their fluid neighbours' Vz) and no quiet runs (those flavours ignore the bit).
// Z-slabs qualify: the planes a neighbour's stress half-step reads are a slab's first and last two, never inner planes of a run.
// Between the two half-steps of a step Vz is of mixed time level (bfd_sim::midStep): the setters that would rebuild the lists refuse until the step ends.
static bool adv_vz_engine(const bfd_sim *s, int nSolid)          // run lists just formed
{
    return s->advEnv && (s->cfg.kernelVariant == 0 || s->cfg.kernelVariant == 3) && !s->pingpong && s->d.VzW == s->d.Vz &&
           s->cfg.typeSource < 2 && nSolid == 0 && !quiet_runs_wanted(s);
}

// Quiet runs (bfd_dev::act; bfd_kernels_v2.hip): a production call lets the runs ahead of the wave front return at entry. On when the
// engine (a whole domain or a Z-slab of at least three sub-tiles: its boundary runs always work) accumulates its maps over the caller's own window (rmsFirstStep = 0: bench.py's timed windows, which accumulate from
// step 1, never see it), runs the class-specialised kernels (variants 0 / 3, in-place update) and keeps solid-only values compact; BFD_SKIP_ZERO=0
// switches it off. The map starts with the sub-tiles of the source voxels at step 0; when inputs are set again in the middle of a run every sub-tile
// counts as active from then on.
static bool quiet_runs_wanted(const bfd_sim *s)          // tile lists built
{
    const bfd_dev &d = s->d;
    const bool whole = d.k0 == 0 && d.nk == d.N3;
    bool on = s->cfg.rmsFirstStep == 0 && (s->cfg.kernelVariant == 0 || s->cfg.kernelVariant == 3) && !s->pingpong &&
              (s->tiles.nSolid == 0 || d.cssRow != nullptr) && d.nk >= 3 * bfd_tile_subz();
    if (const char *ev = getenv("BFD_SKIP_ZERO_SLABS")) on = on && (whole || atoi(ev) != 0);      // 0: whole domains only (the first form of the round)
    if (const char *ev = getenv("BFD_SKIP_ZERO")) on = on && atoi(ev) != 0;
    return on;
}
static int setup_activity_map(bfd_sim *s)
{
    bfd_dev &d = s->d;
    const bool whole = d.k0 == 0 && d.nk == d.N3;
    const bool on = s->tilesReady && quiet_runs_wanted(s);
    s->actReady = true;
    BFD_HIP(hipSetDevice(s->cfg.device));
    if (!on) { d.act = nullptr; drop_step_graph(s); return 0; }
    int tx, ty, nsub; bfd_tile_grid(d, &tx, &ty, &nsub);
    const size_t bytes = (size_t)(tx + 2) * (ty + 2) * (nsub + 2);
    if (!s->actBase || s->actBytes != bytes) {
        dev_release(s, &s->actBase);
        const int rc = dev_alloc(s, &s->actBase, bytes, false);
        if (rc) return rc;
        s->actBytes = bytes;
    }
    d.act = s->actBase; d.actX = tx + 2; d.actY = ty + 2;
    {   // a Z-slab: the runs of the sub-tiles that hold the planes next to a neighbour (the "boundary" runs of a split half-step) always work
        const int SUB = bfd_tile_subz(), lowPlanes = std::min(SUB, d.nk), hiStart = std::max(((d.nk - 2) / SUB) * SUB, lowPlanes);
        d.actLo = whole ? 0 : lowPlanes; d.actHi = whole ? 0x7fffffff : hiStart;
    }
    if (s->step == 0) {
        BFD_HIP(hipMemsetAsync(s->actBase, 0, bytes, s->stream));
        bfd_launch_mark_source_subtiles(d, s->stream, s->srcLin, (long)s->nSrcVox);
    } else {
        // the border stays clear (it stands for what lies outside the domain); every sub-tile inside is taken as active
        std::vector<unsigned char> h(bytes, 0);
        for (int q = 1; q <= nsub; q++) for (int y = 1; y <= ty; y++) memset(&h[((size_t)q * (ty + 2) + y) * (tx + 2) + 1], 1, (size_t)tx);
        BFD_HIP(hipStreamSynchronize(s->stream));                            // the engine's stream does not wait for the legacy stream this copy runs on
        BFD_HIP(hipMemcpy(s->actBase, h.data(), bytes, hipMemcpyHostToDevice));
    }
    BFD_HIP(hipGetLastError());
    BFD_HIP(hipStreamSynchronize(s->stream));        // a slab's half-steps may be queued on other streams than the engine's
    drop_step_graph(s);
    return 0;
}

static int check_ready(bfd_sim *s)
{
    if (!s) BFD_FAIL(-1, "null sim");
    if (!s->haveMaterials || !s->haveMap) BFD_FAIL(-6, "materials and material map must be set before stepping");
    if (!s->classesReady) {      // per-cell class bytes (every variant: the output kernels consult them too)
        BFD_HIP(hipSetDevice(s->cfg.device));
        bfd_launch_cell_classes(s->d, s->stream, s->clsBase, (long)s->nalloc);
        BFD_HIP(hipGetLastError());
        BFD_HIP(hipStreamSynchronize(s->stream));
        s->classesReady = true;
    }
    if (!s->tilesReady && s->cfg.kernelVariant != 1) {
        BFD_HIP(hipSetDevice(s->cfg.device));
        const int rc = build_tile_lists(s);
        if (rc) return rc;
    }
    if (!s->placementDone) {
        s->placementDone = true;
        const int rc = bfd_choose_placement(s);
        if (rc) return rc;
        bind_compact_views(s);        // the state buffers may have changed hands
    }
    if (!s->actReady) { const int rc = setup_activity_map(s); if (rc) return rc; }
    return 0;
}

// ---- paired accumulation -------------------------------------------------------------------------------------------------
// The Pressure sum / peak of the fluid runs costs velocity_fluid a read and a write of the map in every accumulating step. stress_fluid
// holds, for every cell, the old Szz (the final pressure of the step before: velocity-type sources never touch Szz) and the new one in
// registers, so accumulating steps go in pairs: in the first velocity_fluid runs its non-accumulating flavour and the engine remembers
// that the maps lack this step (pendingAcc); in the second the pairing flavour of stress_fluid adds both steps in one read-modify-write,
// in the order they are added otherwise. Whatever reads or clears the maps, or changes what lies behind them, flushes first
// (flush_pending: one small kernel adds the Pressure of the current Szz); the next accumulating step then opens a new pair. The solid
// runs are not paired (their pressure needs Sxx / Syy, which the sparse kernel writes after stress_fluid): velocity_solid accumulates in
// every step; a cell belongs to one run class, so the two schemes do not meet. Both parts of a split half-step take the same flavour, the
// state flips where the step counter advances. Bit-identical to accumulating in every step; BFD_PAIR_ACC=0 selects that path.
// Off with stress-type sources (they change Szz between the two kernels), outside variants 0 / 3, with the second copies of variant 4,
// and with quiet runs (those flavours accumulate in 2 % of a call's steps). Graph replay covers non-accumulating steps only.
// The accumulating steps of this engine pair: ONE predicate for the byte tables (build_tile_lists: quiet = quiet_runs_wanted, the run count just
// built) and for the launches (pairing_step: quiet = the activity map is in use, the current run count)
static bool pair_engine(const bfd_sim *s, bool quiet, int nFluid)
{
    return s->pairEnv && s->cfg.typeSource < 2 && (s->cfg.kernelVariant == 0 || s->cfg.kernelVariant == 3) && !s->pingpong && !quiet &&
           nFluid > 0 && (s->acc || s->pk) && pressure_slot(s) >= 0;
}
// this step's accumulation of the fluid runs is paired (constant over the parts of a time step; pairDone: its stress half-step has already
// taken the pairing flavour, so the step stays paired whatever a setter did in between)
static bool pairing_step(const bfd_sim *s)
{
    return s->pairDone || (s->step >= s->accStart && s->tilesReady && pair_engine(s, s->d.act != nullptr, s->tiles.nFluid));
}

// sources of one part of a half-step: part 0 all, 1 = first+last z-chunk, 2 = the chunks between
// Views of the fields for the launches of one time step when V, Szz, Rzz are kept in two copies (variant 4): kernels
// read d.X and write d.XW. After the stress half-step the new Szz/Rzz are the W copies; after the velocity half-step
// so are the new V; swap_fields() then makes the W copies current. In-place variants: W == X, all views equal d.
static bfd_dev new_stress_view(const bfd_dev &d) { bfd_dev v = d; v.Szz = d.SzzW; v.Rzz = d.RzzW; return v; }
static bfd_dev new_velocity_view(const bfd_dev &d) { bfd_dev v = d; v.Vx = d.VxW; v.Vy = d.VyW; v.Vz = d.VzW; return v; }
static void swap_fields(bfd_dev &d)
{
    std::swap(d.Vx, d.VxW); std::swap(d.Vy, d.VyW); std::swap(d.Vz, d.VzW); std::swap(d.Szz, d.SzzW); std::swap(d.Rzz, d.RzzW);
}

static int inject_part(bfd_sim *s, int part, const bfd_dev &view, hipStream_t st)
{
    const int64_t n = s->nSrcVox;
    int64_t beg[2] = {0, 0}, end[2] = {0, 0};
    if (part == 0 || s->cfg.kernelVariant == 1) { if (part == 1) return 0; end[0] = n; }
    else if (part == 1) { end[0] = s->srcLowEnd; beg[1] = s->srcHighBeg; end[1] = n; }
    else { beg[0] = s->srcLowEnd; end[0] = s->srcHighBeg; }
    if (s->srcK) {          // separable: weights and signals are resident, nothing to stream
        for (int r = 0; r < 2; r++) {
            const int64_t c = end[r] - beg[r];
            if (c <= 0) continue;
            launch_inject_separable(s->srcK, st, view, s->cfg.typeSource, s->srcLin + beg[r], s->srcRow + beg[r],
                                    s->srcW[0] ? s->srcW[0] + beg[r] : nullptr, s->srcW[1] ? s->srcW[1] + beg[r] : nullptr,
                                    s->srcW[2] ? s->srcW[2] + beg[r] : nullptr, s->srcWeights, s->srcSignals, s->step, nullptr,
                                    s->lengthSource, (long)c);
        }
        return 0;
    }
    const float *pulse = nullptr;
    { const int rc = pulse_row(s, s->step, st, &pulse); if (rc) return rc; }
    for (int r = 0; r < 2; r++) {
        const int64_t c = end[r] - beg[r];
        if (c <= 0) continue;
        hipLaunchKernelGGL(inject_sources, dim3(grid_for(c)), dim3(256), 0, st, view, s->cfg.typeSource,
                           s->srcLin + beg[r], s->srcRow + beg[r], s->srcW[0] ? s->srcW[0] + beg[r] : nullptr,
                           s->srcW[1] ? s->srcW[1] + beg[r] : nullptr, s->srcW[2] ? s->srcW[2] + beg[r] : nullptr, pulse, (long)c);
    }
    pulse_row_read(s, s->step, st);
    return 0;
}

// part 0 = whole half-step; 1 = boundary tiles (first/last z-chunk: what a Z-neighbour reads) with their
// sources; 2 = interior tiles with theirs. Variant 1 has no tiles: part 1 is empty, part 2 is everything.
static int stress_part(bfd_sim *s, int part, hipStream_t st)
{
    int rc = check_ready(s); if (rc) return rc;
    if (part < 0 || part > 2) BFD_FAIL(-2, "half-step part must be 0, 1 or 2");
    BFD_HIP(hipSetDevice(s->cfg.device));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (s->timing && s->perKernel) {
        e0 = bfd_get_event(s); e1 = bfd_get_event(s);
        if (!e0 || !e1) { if (e0) s->evPool.push_back(e0); if (e1) s->evPool.push_back(e1); e0 = e1 = nullptr; }
        else hipEventRecord(e0, st);
    }
    if (s->pingpong && part != 0) BFD_FAIL(-2, "split half-steps are not available with kernelVariant 4 on a whole domain");
    if (s->cfg.kernelVariant == 1) { if (part != 1) bfd_launch_stress_v1(s->d, st); }
    else {
        float *accP = nullptr, *pkP = nullptr;
        if (s->pendingAcc && !pairing_step(s)) { rc = flush_pending(s, st); if (rc) return rc; }
        if (s->pendingAcc || s->pairDone) {          // second step of a pair: the maps take the previous step's Pressure and this one's
            const int qP = pressure_slot(s);
            accP = s->acc ? s->acc + (size_t)qP * s->nloc : nullptr; pkP = s->pk ? s->pk + (size_t)qP * s->nloc : nullptr;
            s->pairedLaunches++;
            // from here on the maps hold this step: a flush between the half-steps must add nothing (the other part of a split half-step
            // still takes the pairing flavour for its own cells)
            s->pendingAcc = false; s->pairDone = true;
        }
        bfd_launch_stress_v2(s->d, st, &s->tiles, part, accP, pkP);
        s->midStep = true;
    }
    if (e0) { hipEventRecord(e1, st); s->evStress.push_back(e0); s->evStress.push_back(e1); }
    if (s->nSrcVox && s->cfg.typeSource >= 2 && s->step < s->lengthSource) { rc = inject_part(s, part, new_stress_view(s->d), st); if (rc) return rc; }
    BFD_HIP(hipGetLastError());
    return 0;
}

static int velocity_part(bfd_sim *s, int part, hipStream_t st)
{
    int rc = check_ready(s); if (rc) return rc;
    if (part < 0 || part > 2) BFD_FAIL(-2, "half-step part must be 0, 1 or 2");
    BFD_HIP(hipSetDevice(s->cfg.device));
    const bfd_dev &d = s->d;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (s->timing && s->perKernel) {
        e0 = bfd_get_event(s); e1 = bfd_get_event(s);
        if (!e0 || !e1) { if (e0) s->evPool.push_back(e0); if (e1) s->evPool.push_back(e1); e0 = e1 = nullptr; }
        else hipEventRecord(e0, st);
    }
    const int n = s->step;
    const bool accNow = (s->acc || s->pk) && n >= s->accStart;
    const bool paired = pairing_step(s);      // the fluid runs' Pressure goes through stress_fluid (paired accumulation)
    int qP = -1;   // Pressure is accumulated inside the tiled velocity kernels
    if (accNow && s->cfg.kernelVariant != 1)
        for (int q = 0; q < s->nSelR; q++) if (s->selR[q] == BFD_MAP_PRESSURE) qP = q;
    if (s->cfg.kernelVariant == 1) { if (part != 1) bfd_launch_velocity_v1(d, st); }
    else {
        float *accP = (qP >= 0 && s->acc) ? s->acc + (size_t)qP * s->nloc : nullptr;
        float *pkP = (qP >= 0 && s->pk) ? s->pk + (size_t)qP * s->nloc : nullptr;
        if (s->pingpong) {
            if (part != 0) BFD_FAIL(-2, "split half-steps are not available with kernelVariant 4 on a whole domain");
            bfd_launch_fused(d, st, accP, pkP, &s->tiles, 0, s->tiles.nFused);        // both half-steps of its runs: old fields -> W copies
        }
        bfd_launch_velocity_v2(new_stress_view(d), st, accP, pkP, &s->tiles, part, !paired);
    }
    if (e0) { hipEventRecord(e1, st); s->evVelocity.push_back(e0); s->evVelocity.push_back(e1); }
    if (s->nSrcVox && s->cfg.typeSource < 2 && s->step < s->lengthSource) { rc = inject_part(s, part, new_velocity_view(d), st); if (rc) return rc; }
    if (part == 1) { BFD_HIP(hipGetLastError()); return 0; }
    if (s->pingpong) swap_fields(s->d);
    rc = bfd_step_outputs(s, st, qP); if (rc) return rc;      // end of the time step: remaining accumulators, sensors
    BFD_HIP(hipGetLastError());
    if (paired) { s->pendingAcc = !s->pairDone; s->pairDone = false; }      // first step of a pair: the maps lack it; second: settled in its stress half-step
    s->step++;
    s->midStep = false;
    s->stepDevValid = false;
    return 0;
}

int bfd_half_step_stress(bfd_sim *s) { return s ? stress_part(s, 0, s->stream) : check_ready(s); }
int bfd_half_step_velocity(bfd_sim *s) { return s ? velocity_part(s, 0, s->stream) : check_ready(s); }
int bfd_half_step_stress_part(bfd_sim *s, int32_t part) { return s ? stress_part(s, part, s->stream) : check_ready(s); }
int bfd_half_step_velocity_part(bfd_sim *s, int32_t part) { return s ? velocity_part(s, part, s->stream) : check_ready(s); }
// the same on a caller-chosen stream (no synchronisation here: the caller orders the streams with events); the
// engine's own stream is left untouched, so parts may be queued on different streams back to back
int bfd_half_step_stress_part_on(bfd_sim *s, int32_t part, void *hipStream)
{
    if (!s) BFD_FAIL(-1, "null sim");
    return stress_part(s, part, (hipStream_t)hipStream);
}
int bfd_half_step_velocity_part_on(bfd_sim *s, int32_t part, void *hipStream)
{
    if (!s) BFD_FAIL(-1, "null sim");
    return velocity_part(s, part, (hipStream_t)hipStream);
}

// One plain time step recorded into the capture stream: same launches as stress_part / velocity_part (part 0),
// sources indexed by the device step counter, which the last node advances.
static void record_plain_step(bfd_sim *s, hipStream_t cs)
{
    const bfd_dev &d = s->d;
    auto inject = [&]() {
        if (!s->nSrcVox) return;
        if (s->srcK) {
            launch_inject_separable(s->srcK, cs, d, s->cfg.typeSource, s->srcLin, s->srcRow, s->srcW[0], s->srcW[1], s->srcW[2],
                                    s->srcWeights, s->srcSignals, 0, s->stepDev, s->lengthSource, (long)s->nSrcVox);
            return;
        }
        hipLaunchKernelGGL(inject_sources_at, dim3(grid_for(s->nSrcVox)), dim3(256), 0, cs, d, s->cfg.typeSource, s->srcLin, s->srcRow,
                           s->srcW[0], s->srcW[1], s->srcW[2], s->pulseT, s->stepDev, s->nSources, s->lengthSource, (long)s->nSrcVox);
    };
    if (s->cfg.kernelVariant == 1) bfd_launch_stress_v1(d, cs); else bfd_launch_stress_v2(d, cs, &s->tiles, 0);
    if (s->cfg.typeSource >= 2) inject();
    if (s->cfg.kernelVariant == 1) bfd_launch_velocity_v1(d, cs); else bfd_launch_velocity_v2(d, cs, nullptr, nullptr, &s->tiles, 0);
    if (s->cfg.typeSource < 2) inject();
    hipLaunchKernelGGL(advance_step, dim3(1), dim3(1), 0, cs, s->stepDev);
}

static void build_step_graph(bfd_sim *s)
{
    s->graphState = -1;
    if (!s->stepDev && dev_alloc(s, &s->stepDev, 1, true)) return;
    if (!s->captureStream && hipStreamCreateWithFlags(&s->captureStream, hipStreamNonBlocking) != hipSuccess) { s->captureStream = nullptr; return; }
    hipGraph_t g = nullptr;
    if (hipStreamBeginCapture(s->captureStream, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); return; }
    for (int q = 0; q < BFD_GRAPH_STEPS; q++) record_plain_step(s, s->captureStream);
    if (hipStreamEndCapture(s->captureStream, &g) != hipSuccess || !g) { (void)hipGetLastError(); return; }
    const hipError_t e = hipGraphInstantiate(&s->stepGraph, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    if (e != hipSuccess) { s->stepGraph = nullptr; (void)hipGetLastError(); return; }
    s->graphState = 1;
}

// steps [n, n+G) neither accumulate nor sample sensors
static bool plain_steps(const bfd_sim *s, int n, int G)
{
    if ((s->timing && s->perKernel) || s->pingpong) return false;
    if ((s->acc || s->pk) && n + G > s->accStart) return false;
    if (s->nSensors && (s->sensOut || s->dftAcc)) {
        const int sub = s->cfg.sensorSub;
        const int last = n + G - 1;
        // a sample is taken at step m when m % sub == 0 and m / sub in [sensorStart, sensorStart + nTs)
        const int firstCol = (n + sub - 1) / sub, lastCol = last / sub;
        if (lastCol >= firstCol && lastCol >= s->cfg.sensorStart && firstCol < s->cfg.sensorStart + s->nTs) return false;
    }
    return true;
}

int bfd_run(bfd_sim *s, int32_t nSteps)
{
    int rc = check_ready(s); if (rc) return rc;
    // Graph replay is opt-in (BFD_USE_GRAPH=1): on ROCm 7.2 / MI355X replaying the 8-step graph is SLOWER than the same
    // launches issued directly (water, no accumulation: 128^3 38.8 vs 31.3 us/step, 256^3 210 vs 196 us/step), the
    // in-order stream already keeps the GPU fed from one host thread. Kept for runtimes where that changes.
    const char *ug = getenv("BFD_USE_GRAPH");
    const bool useGraph = ug && atoi(ug) != 0;
    int n = 0;
    while (n < nSteps) {
        if (useGraph && nSteps - n >= BFD_GRAPH_STEPS && s->graphState >= 0 && plain_steps(s, s->step, BFD_GRAPH_STEPS)) {
            BFD_HIP(hipSetDevice(s->cfg.device));
            if (s->graphState == 0) build_step_graph(s);
            if (s->graphState == 1) {
                if (!s->stepDevValid) { hipLaunchKernelGGL(set_step, dim3(1), dim3(1), 0, s->stream, s->stepDev, s->step); s->stepDevValid = true; }
                if (hipGraphLaunch(s->stepGraph, s->stream) == hipSuccess) { s->step += BFD_GRAPH_STEPS; n += BFD_GRAPH_STEPS; continue; }
                (void)hipGetLastError();
                s->graphState = -1;          // this runtime cannot replay into the engine's stream: direct launches from here on
            }
        }
        s->stepDevValid = false;
        rc = bfd_half_step_stress(s); if (rc) return rc;
        rc = bfd_half_step_velocity(s); if (rc) return rc;
        n++;
    }
    return 0;
}

int bfd_sync(bfd_sim *s)
{
    if (!s) BFD_FAIL(-1, "null sim");
    BFD_HIP(hipSetDevice(s->cfg.device));
    BFD_HIP(hipStreamSynchronize(s->stream));
    return 0;
}
int bfd_current_step(bfd_sim *s) { return s ? s->step : -1; }
int bfd_prepare(bfd_sim *s) { return check_ready(s); }

int bfd_halo_region(bfd_sim *s, int32_t group, int32_t f, int32_t side, int32_t send, void **devPtr, size_t *bytes)
{
    if (!s || !devPtr || !bytes) BFD_FAIL(-1, "bfd_halo_region: null argument");
    if (group < 0 || group > 1 || f < 0 || f > 2 || side < 0 || side > 1) BFD_FAIL(-2, "bfd_halo_region: bad selector");
    s->haloHandedOut = true;              // from here on the arrays stay where they are (bfd_prepare)
    const bfd_dev &d = s->d;
    float *arr[2][3] = {{d.Vx, d.Vy, d.Vz}, {d.Sxz, d.Syz, d.Szz}};
    float *a = arr[group][f];
    long kl;
    if (side == 0) kl = send ? 0 : -2; else kl = send ? d.nk - 2 : d.nk;
    *devPtr = a + kl * (long)d.plane;
    *bytes = 2 * (size_t)d.plane * sizeof(float);
    return 0;
}

int64_t bfd_placement_cache_release(void)
{
    const int64_t freed = bfd_placement_cache_drop_all();
    bfd_release_pinned_pieces();          // host memory: not part of the count
    (void)hipGetLastError();
    return freed;
}

int bfd_halo_fields(bfd_sim *s, int32_t group, uint32_t *mask)
{
    if (!mask || group < 0 || group > 1) BFD_FAIL(-1, "bfd_halo_fields: bad argument");
    int rc = check_ready(s); if (rc) return rc;
    // an all-fluid slab of the tiled kernels keeps a single normal stress and no shear: its stencils reach across a Z face
    // only through Vz (stress half-step) and Szz (velocity half-step) -- field 2 of either group
    const bool tiled = s->cfg.kernelVariant != 1 && s->cfg.kernelVariant != 2;
    *mask = (tiled && s->tilesReady && s->tiles.nSolid == 0) ? 4u : 7u;
    return 0;
}

int bfd_timing_begin(bfd_sim *s, int32_t perKernel)
{
    if (!s) BFD_FAIL(-1, "null sim");
    BFD_HIP(hipSetDevice(s->cfg.device));
    for (hipEvent_t e : s->evStress) s->evPool.push_back(e);
    for (hipEvent_t e : s->evVelocity) s->evPool.push_back(e);
    s->evStress.clear(); s->evVelocity.clear();
    for (auto &v : s->evK) { for (hipEvent_t e : v) s->evPool.push_back(e); v.clear(); }
    s->timing = true; s->perKernel = perKernel != 0;
    s->tiles.ktimer = perKernel == 2 ? s : nullptr;      // 2: additionally one event pair around every kernel launch
    BFD_HIP(hipEventRecord(s->evBegin, s->stream));
    return 0;
}

int bfd_timing_end(bfd_sim *s, double *totalMs, double *stressMs, double *velocityMs, double *otherMs,
                   int64_t *nStress, int64_t *nVelocity)
{
    if (!s) BFD_FAIL(-1, "null sim");
    if (!s->timing) BFD_FAIL(-6, "bfd_timing_end without bfd_timing_begin");
    BFD_HIP(hipSetDevice(s->cfg.device));
    BFD_HIP(hipEventRecord(s->evEnd, s->stream));
    BFD_HIP(hipEventSynchronize(s->evEnd));
    float ms = 0;
    BFD_HIP(hipEventElapsedTime(&ms, s->evBegin, s->evEnd));
    double st = 0, ve = 0;
    for (size_t a = 0; a + 1 < s->evStress.size(); a += 2) { float t; BFD_HIP(hipEventElapsedTime(&t, s->evStress[a], s->evStress[a + 1])); st += t; }
    for (size_t a = 0; a + 1 < s->evVelocity.size(); a += 2) { float t; BFD_HIP(hipEventElapsedTime(&t, s->evVelocity[a], s->evVelocity[a + 1])); ve += t; }
    if (totalMs) *totalMs = ms;
    if (stressMs) *stressMs = st;
    if (velocityMs) *velocityMs = ve;
    if (otherMs) *otherMs = ms - st - ve;
    if (nStress) *nStress = (int64_t)s->evStress.size() / 2;
    if (nVelocity) *nVelocity = (int64_t)s->evVelocity.size() / 2;
    s->timing = false;
    s->tiles.ktimer = nullptr;
    return 0;
}

int bfd_timing_kernels(bfd_sim *s, double *msPerClass, int64_t *launchesPerClass)
{
    if (!s || !msPerClass) BFD_FAIL(-1, "bfd_timing_kernels: null argument");
    BFD_HIP(hipSetDevice(s->cfg.device));
    for (int c = 0; c < BFD_K_COUNT; c++) {
        double sum = 0;
        const std::vector<hipEvent_t> &v = s->evK[c];
        for (size_t a = 0; a + 1 < v.size(); a += 2) {
            BFD_HIP(hipEventSynchronize(v[a + 1]));
            float t; BFD_HIP(hipEventElapsedTime(&t, v[a], v[a + 1])); sum += t;
        }
        msPerClass[c] = sum;
        if (launchesPerClass) launchesPerClass[c] = (int64_t)v.size() / 2;
    }
    return 0;
}

int bfd_algorithmic_bytes(bfd_sim *s, int32_t accumulating, double *bytesPerClass)
{
    int rc = check_ready(s); if (rc) return rc;
    if (!bytesPerClass) BFD_FAIL(-1, "bfd_algorithmic_bytes: null argument");
    if (s->cfg.kernelVariant == 1) BFD_FAIL(-2, "bfd_algorithmic_bytes: kernelVariant 1 has no tile classes");
    for (int c = 0; c < BFD_K_COUNT; c++) bytesPerClass[c] = s->algBytes[accumulating ? 1 : 0][c];
    return 0;
}

int64_t bfd_paired_launches(bfd_sim *s) { return s ? s->pairedLaunches : -1; }

int bfd_reset(bfd_sim *s)
{
    if (!s) BFD_FAIL(-1, "null sim");
    BFD_HIP(hipSetDevice(s->cfg.device));
    const bfd_dev &d = s->d;
    for (int a = 0; a < 15; a++) BFD_HIP(hipMemsetAsync(s->stateBase[a], 0, s->nalloc * sizeof(float), s->stream));
    if (s->pingpong) for (int a = 0; a < 5; a++) BFD_HIP(hipMemsetAsync(s->ppBase[a], 0, s->nalloc * sizeof(float), s->stream));
    const int P = d.P;
    const bool zTouch = (d.k0 < P) || (d.k0 + d.nk > d.N3 - P);
    static const int dirOf[18] = {0, 1, 2, 1, 0, 2, 0, 2, 1, 0, 1, 2, 0, 1, 2, 0, 1, 2};
    for (int a = 0; a < 18; a++) {
        size_t n = dirOf[a] == 0 ? (size_t)d.nk * d.N2 * 2 * P : (dirOf[a] == 1 ? (size_t)d.nk * 2 * P * d.N1 : (zTouch ? (size_t)2 * P * d.plane : 0));
        if (n) BFD_HIP(hipMemsetAsync(d.psi[a], 0, n * sizeof(float), s->stream));
    }
    if (s->tiles.shearR && s->tiles.nShear) BFD_HIP(hipMemsetAsync(s->tiles.shearR, 0, 3 * (size_t)s->tiles.nShear * sizeof(float), s->stream));
    if (s->tiles.css && s->tiles.cssCap) BFD_HIP(hipMemsetAsync(s->tiles.css, 0, 10 * (size_t)s->tiles.cssCap * sizeof(float), s->stream));      // hosted compact arrays were zeroed with their buffers
    { const int rc = bfd_clear_outputs(s); if (rc) return rc; }
    s->step = 0; s->stepDevValid = false; s->actReady = false;         // the activity map starts over with the state
    s->pendingAcc = s->pairDone = false;                               // the maps were cleared: nothing is outstanding
    s->midStep = false;
    BFD_HIP(hipStreamSynchronize(s->stream));
    drain_pack_jobs(s);
    for (int b = 0; b < 2; b++) s->tileLoaded[b] = -1;        // the streamed source table starts over (tiles are re-packed on demand)
    return 0;
}

int bfd_tile_counts(bfd_sim *s, int32_t *nLossless, int32_t *nLossy, int32_t *nSolid, int32_t *nUni, int32_t *nPml)
{
    int rc = check_ready(s); if (rc) return rc;
    if (nLossless) *nLossless = s->tilesReady ? s->tiles.nLossless : 0;
    if (nLossy) *nLossy = s->tilesReady ? s->tiles.nLossy : 0;
    if (nSolid) *nSolid = s->tilesReady ? s->tiles.nSolidSub : 0;
    if (nUni) *nUni = s->tilesReady ? s->tiles.nUni : 0;
    if (nPml) *nPml = s->tilesReady ? s->tiles.nPml : 0;
    return 0;
}

int bfd_activity_counts(bfd_sim *s, int64_t *active, int64_t *total)
{
    if (!s || !active || !total) BFD_FAIL(-1, "bfd_activity_counts: null argument");
    *active = 0; *total = 0;
    if (!s->d.act || !s->actReady) return 0;
    BFD_HIP(hipSetDevice(s->cfg.device));
    std::vector<unsigned char> h(s->actBytes);
    BFD_HIP(hipStreamSynchronize(s->stream));
    BFD_HIP(hipMemcpy(h.data(), s->actBase, s->actBytes, hipMemcpyDeviceToHost));
    int tx, ty, nsub; bfd_tile_grid(s->d, &tx, &ty, &nsub);
    for (unsigned char v : h) *active += v ? 1 : 0;
    *total = (int64_t)tx * ty * nsub;
    return 0;
}

int bfd_tile_count_lean(bfd_sim *s, int32_t *nLean)
{
    int rc = check_ready(s); if (rc) return rc;
    if (nLean) *nLean = !s->tilesReady ? 0 : s->tiles.nLean;
    return 0;
}

int bfd_tile_count_fused(bfd_sim *s, int32_t *nFused)
{
    int rc = check_ready(s); if (rc) return rc;
    if (nFused) *nFused = s->tilesReady ? s->tiles.nFusedSub : 0;
    return 0;
}

int64_t bfd_device_bytes(bfd_sim *s) { return s ? s->devBytes : -1; }

}  // extern "C"
