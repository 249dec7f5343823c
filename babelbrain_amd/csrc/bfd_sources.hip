// Everything that feeds source values to a time step of libbabelfdtd_hip.so: the setters of the dense and the separable source form, the resident
// and the streamed source table, the injection kernels and their launches (direct and inside a recorded step). gfx950 only.
// bfd_api.hip reaches it through bfd_inject_part, bfd_record_injection, bfd_release_sources and bfd_rewind_sources (bfd_internal.h).
#include "bfd_internal.h"

#include <stdlib.h>

#include <algorithm>
#include <thread>

namespace {

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

void drain_pack_jobs(bfd_source_tiles &T)
{
    for (int b = 0; b < 2; b++) if (T.packJob[b].valid()) T.packJob[b].wait();
}

// the float32 [nSources] row of source values for time step `step`, resident on the device when the kernels of stream st
// run: either a row of the resident table or of the time tile that holds the step (uploaded here when the run enters it)
int pulse_row(bfd_sim *s, int step, hipStream_t st, const float **row)
{
    bfd_source_tiles &T = s->srcTiles;
    if (!T.pulseHost) { *row = s->pulseT + (size_t)step * s->nSources; return 0; }
    const int TS = T.tileSteps, t = step / TS, b = t & 1;
    if (T.tileLoaded[b] != t) {
        if (T.tilePacked[b] == t && T.packJob[b].valid()) T.packJob[b].get();
        else {           // first tile, or the run jumped (bfd_reset): pack it here
            if (T.packJob[b].valid()) T.packJob[b].get();
            if (T.evTileUsed[b]) BFD_HIP(hipEventSynchronize(T.evTile[b]));
            pack_tile(T.pulseHost, s->nSources, s->lengthSource, TS, t, T.tilePinned[b]);
            T.tilePacked[b] = t;
        }
        const int len = std::min(TS, s->lengthSource - t * TS);
        // the kernels that read the tile this buffer held two tiles ago may have run on another stream (split half-steps):
        // the copy waits for the last of them
        for (int q = 0; q < 2; q++) if (T.evReadUsed[b][q]) BFD_HIP(hipStreamWaitEvent(st, T.evRead[b][q], 0));      // the readers on the engine's stream and on a caller's side stream
        BFD_HIP(hipMemcpyAsync(T.tileDev[b], T.tilePinned[b], (size_t)len * s->nSources * sizeof(float), hipMemcpyHostToDevice, st));
        BFD_HIP(hipEventRecord(T.evTile[b], st));
        T.evTileUsed[b] = true; T.tileLoaded[b] = t;
        // the next tile is packed beside the GPU's work on this one (the pinned buffer is free once its last upload is done)
        const int nb = b ^ 1, nt = t + 1;
        if (nt < T.nTiles && T.tilePacked[nb] != nt) {
            if (T.packJob[nb].valid()) T.packJob[nb].get();
            T.tilePacked[nb] = nt;
            const bool waitEv = T.evTileUsed[nb];
            hipEvent_t ev = T.evTile[nb];
            const int dev = s->cfg.device;
            const double *ph = T.pulseHost; const int nS = s->nSources, L = s->lengthSource; float *dst = T.tilePinned[nb];
            T.packJob[nb] = std::async(std::launch::async, [=]() {
                if (waitEv) { hipSetDevice(dev); hipEventSynchronize(ev); }
                pack_tile(ph, nS, L, TS, nt, dst);
            });
        }
    } else {
        BFD_HIP(hipStreamWaitEvent(st, T.evTile[b], 0));      // a part launched on another stream than the upload
    }
    *row = T.tileDev[b] + (size_t)(step - t * TS) * s->nSources;
    return 0;
}

// after the kernels of stream st that read the row pulse_row() returned: the tile buffer may be overwritten behind them
void pulse_row_read(bfd_sim *s, int step, hipStream_t st)
{
    bfd_source_tiles &T = s->srcTiles;
    if (!T.pulseHost) return;
    // one event per buffer and stream kind: the parts of a split half-step run on two streams at the same time, and a single
    // event recorded by both would keep only the later record
    const int b = (step / T.tileSteps) & 1, q = st == s->stream ? 0 : 1;
    if (T.evRead[b][q] && hipEventRecord(T.evRead[b][q], st) == hipSuccess) T.evReadUsed[b][q] = true;
}

}  // namespace

void bfd_source_tiles::release(bfd_sim *s)
{
    bfd_source_tiles &T = *this;
    drain_pack_jobs(T);
    for (int b = 0; b < 2; b++) {
        if (T.packJob[b].valid()) T.packJob[b].get();
        dev_release(s, &T.tileDev[b]);
        if (T.tilePinned[b]) { hipHostFree(T.tilePinned[b]); T.tilePinned[b] = nullptr; }
        T.tileLoaded[b] = T.tilePacked[b] = -1; T.evTileUsed[b] = false; T.evReadUsed[b][0] = T.evReadUsed[b][1] = false;
    }
    T.pulseHost = nullptr; T.tileSteps = T.nTiles = 0;
}

void bfd_source_tiles::destroy(bfd_sim *s)
{
    release(s);
    for (int b = 0; b < 2; b++) {
        if (evTile[b]) { hipEventDestroy(evTile[b]); evTile[b] = nullptr; }
        for (int q = 0; q < 2; q++) if (evRead[b][q]) { hipEventDestroy(evRead[b][q]); evRead[b][q] = nullptr; }
    }
}

// The previous sources of either form go: the voxel list and the resident table, the streamed table, the separable weights and signals, the
// Ox/Oy/Oz weights. The counts are the caller's to set (a setter enters the new ones).
void bfd_release_sources(bfd_sim *s, bool final)
{
    dev_release(s, &s->srcLin); dev_release(s, &s->srcRow); dev_release(s, &s->pulseT);
    if (final) s->srcTiles.destroy(s); else s->srcTiles.release(s);
    dev_release(s, &s->srcWeights); dev_release(s, &s->srcSignals); s->srcK = 0;
    for (int a = 0; a < 3; a++) dev_release(s, &s->srcW[a]);
}

void bfd_rewind_sources(bfd_sim *s)
{
    drain_pack_jobs(s->srcTiles);
    for (int b = 0; b < 2; b++) s->srcTiles.tileLoaded[b] = -1;
}

// sources of one part of a half-step: part 0 all, 1 = first+last z-chunk, 2 = the chunks between
int bfd_inject_part(bfd_sim *s, int part, const bfd_dev &view, hipStream_t st)
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

// the same choice of kernel for a recorded step: all voxels in one launch, the step read from the device's counter
void bfd_record_injection(bfd_sim *s, hipStream_t cs)
{
    const bfd_dev &d = s->d;
    if (!s->nSrcVox) return;
    if (s->srcK) {
        launch_inject_separable(s->srcK, cs, d, s->cfg.typeSource, s->srcLin, s->srcRow, s->srcW[0], s->srcW[1], s->srcW[2],
                                s->srcWeights, s->srcSignals, 0, s->stepDev, s->lengthSource, (long)s->nSrcVox);
        return;
    }
    hipLaunchKernelGGL(inject_sources_at, dim3(grid_for(s->nSrcVox)), dim3(256), 0, cs, d, s->cfg.typeSource, s->srcLin, s->srcRow,
                       s->srcW[0], s->srcW[1], s->srcW[2], s->pulseT, s->stepDev, s->nSources, s->lengthSource, (long)s->nSrcVox);
}

extern "C" {

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
    bfd_release_sources(s, false);
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
        bfd_source_tiles &T = s->srcTiles;
        T.pulseHost = pulse; T.tileSteps = tile; T.nTiles = (lengthSource + tile - 1) / tile;
        for (int b = 0; b < 2; b++) {
            hipError_t e = hipSuccess;
            rc = dev_alloc(s, &T.tileDev[b], (size_t)tile * nSources, false);
            if (!rc) e = hipHostMalloc((void **)&T.tilePinned[b], (size_t)tile * nSources * sizeof(float), hipHostMallocDefault);
            if (!rc && e == hipSuccess && !T.evTile[b]) e = hipEventCreateWithFlags(&T.evTile[b], hipEventDisableTiming);
            for (int q = 0; q < 2; q++) if (!rc && e == hipSuccess && !T.evRead[b][q]) e = hipEventCreateWithFlags(&T.evRead[b][q], hipEventDisableTiming);
            if (rc || e != hipSuccess) {        // nothing half-built stays behind: the sim is back to "no sources"
                const std::string why = rc ? std::string(bfd_last_error()) : std::string("bfd_set_sources: ") + hipGetErrorString(e);
                T.release(s);
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

}  // extern "C"
