// C ABI of libbabelfdtd_hip.so (include/babelfdtd.h): host logic, coefficient preparation, layout conversion,
// time stepping. gfx950 only. Sources: bfd_sources.hip. Run lists of the tiled kernels: bfd_lists.hip. Sensors, maps and
// the result getters: bfd_outputs.hip.
//
// Mirrors what BabelIntegrationBASE.py:2338-2365 hands to the reference's solver
// (package BabelViscoFDTD==1.2.4, absent from /root/reference).
#include "bfd_internal.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
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
__global__ void set_step(int *stepDev, int v) { *stepDev = v; }
__global__ void advance_step(int *stepDev) { *stepDev = *stepDev + 1; }

}  // namespace

// inputs changed: a recorded step graph holds stale pointers
void drop_step_graph(bfd_sim *s)
{
    if (s->stepGraph) { hipGraphExecDestroy(s->stepGraph); s->stepGraph = nullptr; }
    if (s->graphState == 1) s->graphState = 0;
    s->stepDevValid = false;
}

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
void invalidate_lists(bfd_sim *s, bool classes) { s->tilesReady = false; if (classes) s->classesReady = false; s->actReady = false; drop_step_graph(s); }

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

// The event pair around the kernels of a half-step (per-kernel timing): the opening event recorded on st, or no pair when an event cannot be made
// (the one obtained goes back to the pool); the closing event recorded behind the kernels and the pair kept in `pairs` (evStress / evVelocity).
static void open_timing_pair(bfd_sim *s, hipStream_t st, hipEvent_t &e0, hipEvent_t &e1)
{
    e0 = e1 = nullptr;
    if (!(s->timing && s->perKernel)) return;
    e0 = bfd_get_event(s); e1 = bfd_get_event(s);
    if (!e0 || !e1) { if (e0) s->evPool.push_back(e0); if (e1) s->evPool.push_back(e1); e0 = e1 = nullptr; }
    else hipEventRecord(e0, st);
}
static void close_timing_pair(hipStream_t st, hipEvent_t e0, hipEvent_t e1, std::vector<hipEvent_t> &pairs)
{
    if (e0) { hipEventRecord(e1, st); pairs.push_back(e0); pairs.push_back(e1); }
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
    if (const char *ev = getenv("BFD_PAIR_ACC")) s->pairEnv = atoi(ev) != 0;      // 0: every step accumulates in the velocity kernels (A/B, tests)
    if (const char *ev = getenv("BFD_ADV_VZ")) s->advEnv = atoi(ev) != 0;         // 0: velocity_fluid updates Vz of every plane (A/B, tests)
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
    bfd_release_sources(s, true);
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

}  // extern "C"

// The material ids of the readable span [k = -ghostLow .. nk-1+ghostHigh] that starts at devBase (device memory), into the engine's x-fastest ids:
// the tail the host form and the device form of the setter share. who = the entry's name for the messages
static int material_map_from_device(bfd_sim *s, const char *who, const uint32_t *devBase, int64_t s1, int64_t s2, int64_t s3, int32_t ghostLow, int nkSpan)
{
    const bfd_dev &d = s->d;
    DevTemp<int> flag; int hflag = 0;
    hipError_t e = flag.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(flag, 0, sizeof(int), s->stream);
    if (e == hipSuccess) {
        // destination covers local planes -2..nk+1; source plane index = local k + ghostLow, clamped to the span
        hipLaunchKernelGGL((gather_to_xfast<0, uint16_t>), dim3(grid_for((long)s->nalloc)), dim3(256), 0, s->stream,
                           devBase, (long)s1, (long)s2, (long)s3, s->matBase, d.N1, d.N2, d.nk + 4, ghostLow - 2, 0, nkSpan - 1,
                           (uint32_t)s->cfg.nMat, flag.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&hflag, flag, sizeof(int), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) BFD_FAIL(-10, std::string(who) + ": " + hipGetErrorString(e));
    if (hflag) BFD_FAIL(-5, std::string(who) + ": MaterialMap holds an id >= number of MaterialList rows");
    s->haveMap = true; invalidate_lists(s);
    return 0;
}

// The span [p, p + elems) of uint32 is device memory of the sim's own device, inside one allocation: what the device forms of the setters ask of
// their pointer before a kernel reads through it. A host pointer, managed memory, another device's memory or a span that runs past its
// allocation: false
static bool device_span_of(const bfd_sim *s, const uint32_t *p, size_t elems)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (at.type != hipMemoryTypeDevice || at.device != s->cfg.device) return false;
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return false; }
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)base;
    return a >= b && elems * sizeof(uint32_t) <= size - (a - b);
}

extern "C" {

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
    DevTemp<uint32_t> tmp;
    BFD_HIP(tmp.alloc(span));
    const hipError_t e = hipMemcpyAsync(tmp, base, span * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream);
    if (e != hipSuccess) BFD_FAIL(-10, std::string("bfd_set_material_map: ") + hipGetErrorString(e));
    return material_map_from_device(s, "bfd_set_material_map", tmp, s1, s2, s3, ghostLow, nkSpan);
}

int bfd_set_material_map_device(bfd_sim *s, const uint32_t *devMap, int64_t s1, int64_t s2, int64_t s3,
                                int32_t ghostLow, int32_t ghostHigh)
{
    if (!s || !devMap) BFD_FAIL(-1, "bfd_set_material_map_device: null argument");
    if (ghostLow < 0 || ghostLow > 2 || ghostHigh < 0 || ghostHigh > 2) BFD_FAIL(-2, "ghost plane counts must be 0..2");
    if (s1 < 0 || s2 < 0 || s3 < 0) BFD_FAIL(-2, "negative strides are not supported");
    BFD_REFUSE_MID_STEP("bfd_set_material_map_device");
    const bfd_dev &d = s->d;
    const uint32_t *base = devMap - (int64_t)ghostLow * s3;
    const int nkSpan = d.nk + ghostLow + ghostHigh;
    BFD_HIP(hipSetDevice(s->cfg.device));
    if (!device_span_of(s, base, span_elems(d.N1, d.N2, nkSpan, s1, s2, s3)))
        BFD_FAIL(-1, "bfd_set_material_map_device: devMap is not device memory of the sim's device that holds the whole view");
    { const int rc = flush_pending(s); if (rc) return rc; }
    return material_map_from_device(s, "bfd_set_material_map_device", base, s1, s2, s3, ghostLow, nkSpan);      // read in place
}

// mask (device memory, or null with clear) into the reflector bit of the ids
static int reflector_from_device(bfd_sim *s, const uint32_t *devMask, int64_t s1, int64_t s2, int64_t s3)
{
    const bfd_dev &d = s->d;
    hipLaunchKernelGGL(or_reflector, dim3(grid_for((long)s->nloc)), dim3(256), 0, s->stream, devMask, (long)s1, (long)s2, (long)s3,
                       s->matBase + 2 * (size_t)d.plane, d.N1, d.N2, d.nk, devMask ? 0 : 1);
    BFD_HIP(hipStreamSynchronize(s->stream));
    invalidate_lists(s);      // reflector cells end the UNI class of their tiles
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
    return reflector_from_device(s, tmp, s1, s2, s3);
}

int bfd_set_reflector_device(bfd_sim *s, const uint32_t *devMask, int64_t s1, int64_t s2, int64_t s3)
{
    if (!s) BFD_FAIL(-1, "bfd_set_reflector_device: null sim");
    if (devMask && (s1 < 0 || s2 < 0 || s3 < 0)) BFD_FAIL(-2, "negative strides are not supported");
    if (!s->haveMap) BFD_FAIL(-6, "bfd_set_reflector_device: set the material map first");
    BFD_REFUSE_MID_STEP("bfd_set_reflector_device");
    const bfd_dev &d = s->d;
    BFD_HIP(hipSetDevice(s->cfg.device));
    if (devMask && !device_span_of(s, devMask, span_elems(d.N1, d.N2, d.nk, s1, s2, s3)))
        BFD_FAIL(-1, "bfd_set_reflector_device: devMask is not device memory of the sim's device that holds the whole view");
    { const int rc = flush_pending(s); if (rc) return rc; }
    return reflector_from_device(s, devMask, s1, s2, s3);      // read in place
}

}  // extern "C"

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
bool pair_engine(const bfd_sim *s, bool quiet, int nFluid)
{
    return s->pairEnv && s->cfg.typeSource < 2 && class_kernels_in_place(s) && !quiet &&
           nFluid > 0 && (s->acc || s->pk) && pressure_slot(s) >= 0;
}
// this step's accumulation of the fluid runs is paired (constant over the parts of a time step; pairDone: its stress half-step has already
// taken the pairing flavour, so the step stays paired whatever a setter did in between)
static bool pairing_step(const bfd_sim *s)
{
    return s->pairDone || (s->step >= s->accStart && s->tilesReady && pair_engine(s, s->d.act != nullptr, s->tiles.nFluid));
}

// Views of the fields for the launches of one time step when V, Szz, Rzz are kept in two copies (variant 4): kernels
// read d.X and write d.XW. After the stress half-step the new Szz/Rzz are the W copies; after the velocity half-step
// so are the new V; swap_fields() then makes the W copies current. In-place variants: W == X, all views equal d.
static bfd_dev new_stress_view(const bfd_dev &d) { bfd_dev v = d; v.Szz = d.SzzW; v.Rzz = d.RzzW; return v; }
static bfd_dev new_velocity_view(const bfd_dev &d) { bfd_dev v = d; v.Vx = d.VxW; v.Vy = d.VyW; v.Vz = d.VzW; return v; }
static void swap_fields(bfd_dev &d)
{
    std::swap(d.Vx, d.VxW); std::swap(d.Vy, d.VyW); std::swap(d.Vz, d.VzW); std::swap(d.Szz, d.SzzW); std::swap(d.Rzz, d.RzzW);
}

// part 0 = whole half-step; 1 = boundary tiles (first/last z-chunk: what a Z-neighbour reads) with their
// sources; 2 = interior tiles with theirs. Variant 1 has no tiles: part 1 is empty, part 2 is everything.
static int stress_part(bfd_sim *s, int part, hipStream_t st)
{
    int rc = check_ready(s); if (rc) return rc;
    if (part < 0 || part > 2) BFD_FAIL(-2, "half-step part must be 0, 1 or 2");
    BFD_HIP(hipSetDevice(s->cfg.device));
    hipEvent_t e0, e1;
    open_timing_pair(s, st, e0, e1);
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
        bfd_launch_stress_tiled(s->d, st, &s->tiles, part, accP, pkP);
        s->midStep = true;
    }
    close_timing_pair(st, e0, e1, s->evStress);
    if (s->nSrcVox && s->cfg.typeSource >= 2 && s->step < s->lengthSource) { rc = bfd_inject_part(s, part, new_stress_view(s->d), st); if (rc) return rc; }
    BFD_HIP(hipGetLastError());
    return 0;
}

static int velocity_part(bfd_sim *s, int part, hipStream_t st)
{
    int rc = check_ready(s); if (rc) return rc;
    if (part < 0 || part > 2) BFD_FAIL(-2, "half-step part must be 0, 1 or 2");
    BFD_HIP(hipSetDevice(s->cfg.device));
    const bfd_dev &d = s->d;
    hipEvent_t e0, e1;
    open_timing_pair(s, st, e0, e1);
    const int n = s->step;
    const bool accNow = (s->acc || s->pk) && n >= s->accStart;
    const bool paired = pairing_step(s);      // the fluid runs' Pressure goes through stress_fluid (paired accumulation)
    int qP = -1;   // Pressure is accumulated inside the tiled velocity kernels
    if (accNow && s->cfg.kernelVariant != 1) qP = pressure_slot(s);
    if (s->cfg.kernelVariant == 1) { if (part != 1) bfd_launch_velocity_v1(d, st); }
    else {
        float *accP = (qP >= 0 && s->acc) ? s->acc + (size_t)qP * s->nloc : nullptr;
        float *pkP = (qP >= 0 && s->pk) ? s->pk + (size_t)qP * s->nloc : nullptr;
        if (s->pingpong) {
            if (part != 0) BFD_FAIL(-2, "split half-steps are not available with kernelVariant 4 on a whole domain");
            bfd_launch_fused(d, st, accP, pkP, &s->tiles, 0, s->tiles.nFused);        // both half-steps of its runs: old fields -> W copies
        }
        bfd_launch_velocity_tiled(new_stress_view(d), st, accP, pkP, &s->tiles, part, !paired);
    }
    close_timing_pair(st, e0, e1, s->evVelocity);
    if (s->nSrcVox && s->cfg.typeSource < 2 && s->step < s->lengthSource) { rc = bfd_inject_part(s, part, new_velocity_view(d), st); if (rc) return rc; }
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

extern "C" {

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
    if (s->cfg.kernelVariant == 1) bfd_launch_stress_v1(d, cs); else bfd_launch_stress_tiled(d, cs, &s->tiles, 0);
    if (s->cfg.typeSource >= 2) bfd_record_injection(s, cs);
    if (s->cfg.kernelVariant == 1) bfd_launch_velocity_v1(d, cs); else bfd_launch_velocity_tiled(d, cs, nullptr, nullptr, &s->tiles, 0);
    if (s->cfg.typeSource < 2) bfd_record_injection(s, cs);
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
    bfd_rewind_sources(s);        // the streamed source table starts over (tiles are re-packed on demand)
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
