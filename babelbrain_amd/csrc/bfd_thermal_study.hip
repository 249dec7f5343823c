// A thermal study on MI355X: the volumes of one Step-3 calculation (ThermalModeling/CalculateTemperatureEffects.py:908-1193) held on the device from
// their first upload to the last result the caller asks for. The arithmetic is the existing entries': the median in a region (bfd_median.hip), the
// loss survey and the class extrema (bfd_thermal.hip) and the bio-heat step loop (bfd_bhte.hip) run here through their device-pointer stages
// (bfd_thermal_stages.h), the same launch sequences their public entries run between their own copies. What this file adds is the glue that used to be
// host passes over a volume, per element in bfd_thermal_study_core.h:
//   narrow_ids     the map as passed (1, 2 or 4-byte ids) -> resident 8- or 16-bit ids, with the range check
//   region_mask    class table and ids -> the byte mask the median takes
//   heat_source    q = ((s s) qf[m]), s = the scaled pressure, from the UNSCALED resident p (no scaled copy of p exists)
//   field_max      the scaled p (one field) or the maximum over the scaled fields, float32; the float64 product of mode 0
//   merge_max      np.maximum(resident, uploaded volume)
//   table_lookup   T = initT[m]
//   plane gathers  [:, j, :] of a float32 volume and of the ids
// All are streaming kernels: quads of voxels (16 B per lane and float32 array) in grid-stride loops of 2048 x 256 threads, like the helpers of
// bfd_bhte.hip. Every resident float32 volume starts on a 16-byte boundary and is padded to whole quads (field stride ns = n rounded up to 4), so the
// last quad of a volume reads and writes inside the volume's own allocation. No atomics of any kind here; no kernel waits for another workgroup; every
// loop is a grid-stride loop over a fixed count. The same bytes come out in every run.
// Layout: the caller's numpy C order [N1][N2][N3], last axis fastest. T, dose, q, Tmax, doseAtCapture and the ids carry the front and back pads of
// bhte_run_core (bfd_bhte_pads); the whole id allocation is zeroed at creation, so an id read from a pad indexes every table.
#include <string.h>
#include <type_traits>
#include <vector>
#include "bfd_internal.h"
#include "bfd_call.h"
#include "bfd_thermal_stages.h"
#include "bfd_thermal_core.h"
#include "bfd_thermal_study_core.h"
#include "../../include/babelfdtd.h"

struct bfd_thermal_s {
    int device = 0, N1 = 0, N2 = 0, N3 = 0, nFields = 0, nMat = 0, idBytes = 1;
    size_t n = 0, ns = 0, padF = 0, padB = 0;        // voxels; voxels rounded up to whole quads; pads in elements
    float *p = nullptr, *pw = nullptr;                // [nFields] volumes, ns apart
    float *q = nullptr;                               // [nFields] volumes, ns apart, padded as a whole
    float *T[2] = {nullptr, nullptr}, *dose = nullptr, *Tmax = nullptr, *doseCap = nullptr;
    float *scratch = nullptr;                         // one volume: the output of the median, an uploaded volume, p_map
    float *prevT = nullptr, *prevDose = nullptr, *prevTend = nullptr;      // PreviousData's volumes, allocated by bfd_thermal_set_previous alone
    void *ids = nullptr;
    uint8_t *mask = nullptr;                          // one byte per voxel: the region of the median, the brain mask of the survey
    int cur = 0;                                      // which of T holds the temperature
    bool inputs = false, scaled = false, ran = false, pmapHeld = false;
    int mode = 0;
    std::vector<double> ratio;
    double *dRatio = nullptr;                         // [nFields] on the device
    int64_t up = 0, down = 0;
    std::vector<void *> allocs;
};

namespace {

constexpr int THREADS = 256, BLOCKS = 2048;
enum { V_TMAX = BFD_THERMAL_TMAX, V_DOSECAP = BFD_THERMAL_DOSE_AT_CAPTURE, V_T = BFD_THERMAL_T, V_DOSE = BFD_THERMAL_DOSE, V_Q = BFD_THERMAL_Q,
       V_PMAP = BFD_THERMAL_P_MAP, V_PW = BFD_THERMAL_PW, V_P = BFD_THERMAL_P, V_MAP = BFD_THERMAL_MAP };

#define TS_GRID_STRIDE(v, count) for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < (count); v += (size_t)gridDim.x * blockDim.x)

// ids of quad v of a resident map, widened
template <typename ID> __device__ __forceinline__ void load_ids(const ID *ids, size_t v, uint32_t id[4]);
template <> __device__ __forceinline__ void load_ids<uint8_t>(const uint8_t *ids, size_t v, uint32_t id[4])
{
    const uint32_t w = ((const uint32_t *)ids)[v];
    id[0] = w & 0xFFu; id[1] = (w >> 8) & 0xFFu; id[2] = (w >> 16) & 0xFFu; id[3] = w >> 24;
}
template <> __device__ __forceinline__ void load_ids<uint16_t>(const uint16_t *ids, size_t v, uint32_t id[4])
{
    const uint2 w = ((const uint2 *)ids)[v];
    id[0] = w.x & 0xFFFFu; id[1] = w.x >> 16; id[2] = w.y & 0xFFFFu; id[3] = w.y >> 16;
}
template <typename ID> __device__ __forceinline__ void store_ids(ID *ids, size_t v, const uint32_t id[4]);
template <> __device__ __forceinline__ void store_ids<uint8_t>(uint8_t *ids, size_t v, const uint32_t id[4])
{
    ((uint32_t *)ids)[v] = id[0] | (id[1] << 8) | (id[2] << 16) | (id[3] << 24);
}
template <> __device__ __forceinline__ void store_ids<uint16_t>(uint16_t *ids, size_t v, const uint32_t id[4])
{
    ((uint2 *)ids)[v] = make_uint2(id[0] | (id[1] << 16), id[2] | (id[3] << 16));
}

// the map as passed (IDB bytes per id, padded with zeros to whole quads) -> resident ids; *flag set where an id is not below nMat
template <int IDB, typename ID>
__global__ __launch_bounds__(THREADS) void narrow_ids(const void *__restrict__ in, ID *__restrict__ out, size_t quads, uint32_t nMat, uint32_t *__restrict__ flag)
{
    uint32_t bad = 0;
    TS_GRID_STRIDE(v, quads) {
        uint32_t id[4];
        if (IDB == 1) load_ids<uint8_t>((const uint8_t *)in, v, id);
        else if (IDB == 2) load_ids<uint16_t>((const uint16_t *)in, v, id);
        else { const uint4 w = ((const uint4 *)in)[v]; id[0] = w.x; id[1] = w.y; id[2] = w.z; id[3] = w.w; }
#pragma unroll
        for (int b = 0; b < 4; b++) id[b] = ts_narrow_id(id[b], nMat, &bad);
        store_ids<ID>(out, v, id);
    }
    if (bad) *flag = 1u;                              // every writer stores the same word
}

template <typename ID>
__global__ __launch_bounds__(THREADS) void region_mask(const ID *__restrict__ ids, const uint8_t *__restrict__ classOf, int bit, uint8_t *__restrict__ mask, size_t quads)
{
    TS_GRID_STRIDE(v, quads) {
        uint32_t id[4];
        load_ids<ID>(ids, v, id);                     // resident ids index the table, pads included (zeros)
        ((uint32_t *)mask)[v] = (uint32_t)ts_region(id[0], classOf, bit) | ((uint32_t)ts_region(id[1], classOf, bit) << 8) |
                                ((uint32_t)ts_region(id[2], classOf, bit) << 16) | ((uint32_t)ts_region(id[3], classOf, bit) << 24);
    }
}

template <typename ID>
__global__ __launch_bounds__(THREADS) void study_table_lookup(const ID *__restrict__ ids, const float *__restrict__ tab, float4 *__restrict__ out, size_t quads)
{
    TS_GRID_STRIDE(v, quads) {
        uint32_t id[4];
        load_ids<ID>(ids, v, id);
        out[v] = make_float4(tab[id[0]], tab[id[1]], tab[id[2]], tab[id[3]]);
    }
}

template <typename ID>
__global__ __launch_bounds__(THREADS) void study_heat_source(const float4 *__restrict__ p, const ID *__restrict__ ids, const float *__restrict__ qf, float4 *__restrict__ q,
                                                             size_t quads, double ratio, int mode)
{
    TS_GRID_STRIDE(v, quads) {
        uint32_t id[4];
        load_ids<ID>(ids, v, id);
        const float4 a = p[v];
        q[v] = make_float4(ts_heat(ts_scaled(a.x, ratio, mode), qf[id[0]]), ts_heat(ts_scaled(a.y, ratio, mode), qf[id[1]]),
                           ts_heat(ts_scaled(a.z, ratio, mode), qf[id[2]]), ts_heat(ts_scaled(a.w, ratio, mode), qf[id[3]]));
    }
}

// out = the scaled field (nFields == 1) or the maximum over the scaled fields
__global__ __launch_bounds__(THREADS) void field_max(const float4 *__restrict__ p, size_t strideQuads, int nFields, const double *__restrict__ ratio, int mode,
                                                     float4 *__restrict__ out, size_t quads)
{
    TS_GRID_STRIDE(v, quads) {
        const float4 a = p[v];
        const double r0 = ratio[0];
        float4 m = make_float4(ts_scaled(a.x, r0, mode), ts_scaled(a.y, r0, mode), ts_scaled(a.z, r0, mode), ts_scaled(a.w, r0, mode));
        for (int f = 1; f < nFields; f++) {           // nFields trips
            const float4 b = p[v + (size_t)f * strideQuads];
            const double r = ratio[f];
            m.x = ts_nan_max(m.x, ts_scaled(b.x, r, mode)); m.y = ts_nan_max(m.y, ts_scaled(b.y, r, mode));
            m.z = ts_nan_max(m.z, ts_scaled(b.z, r, mode)); m.w = ts_nan_max(m.w, ts_scaled(b.w, r, mode));
        }
        out[v] = m;
    }
}

// out[v] = (double)p[first + v] * ratio for v < count: a piece of the float64 p_map of mode 0
__global__ __launch_bounds__(THREADS) void scaled64(const float *__restrict__ p, size_t first, size_t count, double ratio, double *__restrict__ out)
{
    TS_GRID_STRIDE(v, count) out[v] = ts_scaled64(p[first + v], ratio);
}

__global__ __launch_bounds__(THREADS) void merge_max(float4 *__restrict__ held, const float4 *__restrict__ other, size_t quads)
{
    TS_GRID_STRIDE(v, quads) {
        float4 m = held[v];
        const float4 t = other[v];
        m.x = ts_nan_max(m.x, t.x); m.y = ts_nan_max(m.y, t.y); m.z = ts_nan_max(m.z, t.z); m.w = ts_nan_max(m.w, t.w);
        held[v] = m;
    }
}

// out[i][k] = vol[i][j][k]
__global__ __launch_bounds__(THREADS) void plane_f32(const float *__restrict__ vol, float *__restrict__ out, size_t N1, size_t N2, size_t N3, size_t j)
{
    TS_GRID_STRIDE(v, N1 * N3) out[v] = vol[((v / N3) * N2 + j) * N3 + v % N3];
}
template <typename ID>
__global__ __launch_bounds__(THREADS) void plane_ids(const ID *__restrict__ ids, uint32_t *__restrict__ out, size_t N1, size_t N2, size_t N3, size_t j)
{
    TS_GRID_STRIDE(v, N1 * N3) out[v] = ids[((v / N3) * N2 + j) * N3 + v % N3];
}

unsigned grid_of(size_t items) { return blocks_for((int64_t)items, THREADS, BLOCKS); }

hipError_t copy_up(bfd_thermal_s *s, void *dst, const void *src, size_t bytes)
{
    s->up += (int64_t)bytes;
    return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
}
hipError_t copy_down(bfd_thermal_s *s, void *dst, const void *src, size_t bytes)
{
    s->down += (int64_t)bytes;
    return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
}

// p_map into the scratch volume unless it is there already
hipError_t hold_pmap(bfd_thermal_s *s)
{
    if (s->pmapHeld) return hipSuccess;
    hipLaunchKernelGGL(field_max, dim3(grid_of(s->ns / 4)), dim3(THREADS), 0, 0, (const float4 *)s->p, s->ns / 4, s->nFields, (const double *)s->dRatio, s->mode,
                       (float4 *)s->scratch, s->ns / 4);
    const hipError_t e = hipGetLastError();
    s->pmapHeld = e == hipSuccess;
    return e;
}

// the resident float32 volume of a name (one volume: p is its first field): null where the name has none
float *volume_of(bfd_thermal_s *s, int which)
{
    switch (which) {
    case V_TMAX: return s->Tmax;
    case V_DOSECAP: return s->doseCap;
    case V_T: return s->T[s->cur];
    case V_DOSE: return s->dose;
    case V_PMAP: return s->scratch;
    case V_P: return s->p;
    default: return nullptr;
    }
}

// -6 where the stage that produces `which` has not run
int stage_missing(const bfd_thermal_s *s, const char *who, int which)
{
    if (!s->inputs) BFD_FAIL(-6, std::string(who) + ": bfd_thermal_set_inputs comes first");
    if ((which == V_PMAP || which == V_Q) && !s->scaled) BFD_FAIL(-6, std::string(who) + ": bfd_thermal_set_scale comes first");
    if ((which == V_TMAX || which == V_DOSECAP || which == V_T || which == V_DOSE || which == V_Q) && !s->ran)
        BFD_FAIL(-6, std::string(who) + ": bfd_thermal_run comes first");
    return 0;
}

template <typename F> void by_id_width(const bfd_thermal_s *s, F f)
{
    if (s->idBytes == 2) f((uint16_t *)s->ids); else f((uint8_t *)s->ids);
}

}  // namespace

extern "C" int bfd_thermal_create(int device, int64_t N1, int64_t N2, int64_t N3, int nFields, int nMat, bfd_thermal *handle)
{
    static const char *who = "bfd_thermal_create";
    if (!handle) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (N1 < 3 || N2 < 3 || N3 < 3) BFD_FAIL(-1, std::string(who) + ": every dimension must be at least 3");
    if (!volume_fits(N1, N2, N3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    if (nFields < 1 || nFields > 4096) BFD_FAIL(-1, std::string(who) + ": nFields must be 1 .. 4096");
    if (nMat < 1 || nMat > bfd_bhte_max_materials())
        BFD_FAIL(-1, std::string(who) + ": nMat must be 1 .. " + std::to_string(bfd_bhte_max_materials()));
    if (int rc = pick_device(who, device)) return rc;
    bfd_thermal_s *s = new bfd_thermal_s;
    s->device = device; s->N1 = (int)N1; s->N2 = (int)N2; s->N3 = (int)N3; s->nFields = nFields; s->nMat = nMat;
    s->idBytes = nMat > 256 ? 2 : 1;                  // the rule of _bhte_inputs (RayleighAndBHTE.py)
    s->n = (size_t)(N1 * N2 * N3); s->ns = (s->n + 3) / 4 * 4;
    bfd_bhte_pads((int)N3, &s->padF, &s->padB);       // the fastest axis of the kernels is the caller's last
    s->ratio.assign((size_t)nFields, 1.0);
    const size_t F = (size_t)nFields;
    hipError_t e = hipSuccess;
    // everything zeroed once: no byte of a resident volume, pads included, is ever read before it is defined
    auto A = [&](void **ptr, size_t front, size_t elems, size_t back, size_t elemBytes) {
        if (e != hipSuccess) return;
        void *raw = nullptr;
        const size_t bytes = (front + elems + back) * elemBytes;
        e = hipMalloc(&raw, bytes);
        if (e != hipSuccess) return;
        s->allocs.push_back(raw);
        e = hipMemset(raw, 0, bytes);
        *ptr = (char *)raw + front * elemBytes;
    };
    A((void **)&s->p, 0, F * s->ns, 0, 4);
    A((void **)&s->pw, 0, F * s->ns, 0, 4);
    A((void **)&s->q, s->padF, F * s->ns, s->padB, 4);
    A((void **)&s->T[0], s->padF, s->ns, s->padB, 4);
    A((void **)&s->T[1], s->padF, s->ns, s->padB, 4);
    A((void **)&s->dose, s->padF, s->ns, s->padB, 4);
    A((void **)&s->Tmax, s->padF, s->ns, s->padB, 4);
    A((void **)&s->doseCap, s->padF, s->ns, s->padB, 4);
    A((void **)&s->scratch, 0, s->ns, 0, 4);
    A((void **)&s->ids, s->padF, s->ns, s->padB, (size_t)s->idBytes);
    A((void **)&s->mask, 0, s->ns, 0, 1);
    A((void **)&s->dRatio, 0, F, 0, 8);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        for (void *q : s->allocs) hipFree(q);
        delete s;
        BFD_FAIL(-10, std::string(who) + ": " + hipGetErrorString(e));
    }
    *handle = s;
    return 0;
}

extern "C" void bfd_thermal_destroy(bfd_thermal s)
{
    if (!s) return;
    if (hipSetDevice(s->device) == hipSuccess) hipDeviceSynchronize();
    for (void *q : s->allocs) hipFree(q);
    delete s;
}

extern "C" int bfd_thermal_set_inputs(bfd_thermal s, const float *p, const float *pw, const void *map, int idBytes)
{
    static const char *who = "bfd_thermal_set_inputs";
    if (!s || !p || !pw || !map) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (idBytes != 1 && idBytes != 2 && idBytes != 4) BFD_FAIL(-1, std::string(who) + ": idBytes must be 1, 2 or 4");
    if (int rc = pick_device(who, s->device)) return rc;
    s->inputs = s->scaled = s->ran = s->pmapHeld = false;
    const size_t quads = s->ns / 4;
    DevTemp<uint8_t> staged;
    DevTemp<uint32_t> flag;
    uint32_t bad = 0;
    BFD_STEP(staged.alloc(s->ns * (size_t)idBytes));
    BFD_STEP(flag.alloc(1));
    BFD_STEP(hipMemset(staged, 0, s->ns * (size_t)idBytes));
    BFD_STEP(hipMemset(flag, 0, 4));
    BFD_STEP(copy_up(s, staged, map, s->n * (size_t)idBytes));
    by_id_width(s, [&](auto *ids) {
        typedef typename std::remove_pointer<decltype(ids)>::type ID;
        if (idBytes == 1) hipLaunchKernelGGL((narrow_ids<1, ID>), dim3(grid_of(quads)), dim3(THREADS), 0, 0, (const void *)staged.p, ids, quads, (uint32_t)s->nMat, flag.p);
        else if (idBytes == 2) hipLaunchKernelGGL((narrow_ids<2, ID>), dim3(grid_of(quads)), dim3(THREADS), 0, 0, (const void *)staged.p, ids, quads, (uint32_t)s->nMat, flag.p);
        else hipLaunchKernelGGL((narrow_ids<4, ID>), dim3(grid_of(quads)), dim3(THREADS), 0, 0, (const void *)staged.p, ids, quads, (uint32_t)s->nMat, flag.p);
    });
    BFD_STEP(hipGetLastError());
    BFD_STEP(copy_down(s, &bad, flag, 4));
    if (bad) BFD_FAIL(-5, std::string(who) + ": an id of the map is not below nMat (" + std::to_string(s->nMat) + "); nothing is kept");
    for (int f = 0; f < s->nFields; f++) {
        BFD_STEP(copy_up(s, s->p + (size_t)f * s->ns, p + (size_t)f * s->n, 4 * s->n));
        BFD_STEP(copy_up(s, s->pw + (size_t)f * s->ns, pw + (size_t)f * s->n, 4 * s->n));
    }
    s->inputs = true;
    return 0;
}

extern "C" int bfd_thermal_median_region(bfd_thermal s, const uint8_t *classOf, int bit, int which, float *kernelMs)
{
    static const char *who = "bfd_thermal_median_region";
    if (!s || !classOf) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (bit < 0 || bit > 7) BFD_FAIL(-1, std::string(who) + ": bit must be 0 .. 7");
    if (which != V_P && which != V_PW) BFD_FAIL(-1, std::string(who) + ": which must be BFD_THERMAL_P or BFD_THERMAL_PW");
    if (int rc = stage_missing(s, who, which)) return rc;
    if (int rc = pick_device(who, s->device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    DevTemp<uint8_t> dtab;
    Events ev;
    BFD_STEP(dtab.alloc((size_t)s->nMat));
    BFD_STEP(copy_up(s, dtab, classOf, (size_t)s->nMat));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    s->pmapHeld = false;                              // the scratch volume takes the filtered field
    by_id_width(s, [&](auto *ids) { hipLaunchKernelGGL(region_mask, dim3(grid_of(s->ns / 4)), dim3(THREADS), 0, 0, ids, (const uint8_t *)dtab.p, bit, s->mask, s->ns / 4); });
    BFD_STEP(hipGetLastError());
    float *fields = which == V_P ? s->p : s->pw;
    for (int f = 0; f < s->nFields; f++) {
        float *field = fields + (size_t)f * s->ns;
        BFD_STEP(bfd_stage_median3d(1, field, s->scratch, s->mask, s->N1, s->N2, s->N3, 3, 3, 3, 0, 0u));
        BFD_STEP(hipMemcpyAsync(field, s->scratch, 4 * s->n, hipMemcpyDeviceToDevice, 0));
    }
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    return 0;
}

extern "C" int bfd_thermal_loss_survey(bfd_thermal s, const uint8_t *classOf, const uint8_t *brainMask, const double *rho, const double *c, double rhoWater,
                                       double cWater, double dx2, float *maxTissue, int64_t *argTissue, float *maxWater, int64_t *argWater, double *eWaterRaw,
                                       double *eWater, double *eTissue, float *kernelMs)
{
    static const char *who = "bfd_thermal_loss_survey";
    if (!s || !classOf || !rho || !c || !maxTissue || !argTissue || !maxWater || !argWater || !eWaterRaw || !eWater || !eTissue)
        BFD_FAIL(-1, std::string(who) + ": null argument");
    auto positive_finite = [](double v) { return v > 0.0 && v - v == 0.0; };
    if (!positive_finite(rhoWater) || !positive_finite(cWater)) BFD_FAIL(-1, std::string(who) + ": rhoWater and cWater must be finite and positive");
    for (int q = 0; q < s->nMat; q++)
        if (!positive_finite(rho[q]) || !positive_finite(c[q])) BFD_FAIL(-1, std::string(who) + ": every rho and c must be finite and positive");
    if (!(dx2 >= 0.0) || dx2 - dx2 != 0.0) BFD_FAIL(-1, std::string(who) + ": dx2 must be finite and not negative");
    if (int rc = stage_missing(s, who, V_P)) return rc;
    if (int rc = pick_device(who, s->device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    const size_t F = (size_t)s->nFields, N3 = (size_t)s->N3, width = 3 * N3;
    const int64_t rows = (int64_t)s->N1 * s->N2;
    size_t partialWords = 0, sumWords = 0;
    bfd_loss_survey_scratch(rows, s->N3, &partialWords, &sumWords);
    std::vector<double> sums(F * width, 0.0);
    std::vector<unsigned long long> best(2 * F, 0);
    DevTemp<uint8_t> dtab;
    DevTemp<double> drho, dc, dpartial, dsums;
    DevTemp<unsigned long long> dpairs;
    DevTemp<uint32_t> dflags;
    Events ev;
    float total = 0.f;
    BFD_STEP(dtab.alloc((size_t)s->nMat));
    BFD_STEP(drho.alloc((size_t)s->nMat));
    BFD_STEP(dc.alloc((size_t)s->nMat));
    BFD_STEP(dpartial.alloc(partialWords));
    BFD_STEP(dsums.alloc(sumWords));
    BFD_STEP(dpairs.alloc(2));
    BFD_STEP(dflags.alloc(1));
    BFD_STEP(copy_up(s, dtab, classOf, (size_t)s->nMat));
    BFD_STEP(copy_up(s, drho, rho, 8 * (size_t)s->nMat));
    BFD_STEP(copy_up(s, dc, c, 8 * (size_t)s->nMat));
    if (brainMask) BFD_STEP(copy_up(s, s->mask, brainMask, s->n));
    BFD_STEP(hipMemset(dflags, 0, 4));
    BFD_STEP(ev.create());
    for (size_t f = 0; f < F; f++) {
        const double *result = nullptr;
        float ms = 0.f;
        BFD_STEP(hipMemset(dpairs, 0, 16));
        BFD_STEP(ev.record(0));
        BFD_STEP(bfd_stage_loss_survey(s->p + f * s->ns, s->pw + f * s->ns, s->ids, s->idBytes, brainMask ? s->mask : nullptr, dtab.p, drho.p, dc.p, s->nMat, 1, rows,
                                       s->N3, rhoWater, cWater, dx2, dpartial.p, dsums.p, dpairs.p, dflags.p, &result));
        BFD_STEP(ev.record(1));
        BFD_STEP(ev.sync(1));
        BFD_STEP(ev.elapsed(&ms, 0, 1));
        total += ms;
        BFD_STEP(copy_down(s, sums.data() + f * width, result, 8 * width));
        BFD_STEP(copy_down(s, best.data() + 2 * f, dpairs, 16));
    }
    uint32_t flags = 0;
    BFD_STEP(copy_down(s, &flags, dflags, 4));
    if (flags & 2u) BFD_FAIL(-1, std::string(who) + ": refused data: a value is not finite");      // FLAG_VALUE of bfd_thermal.hip; the resident ids index the tables
    for (size_t f = 0; f < F; f++) {
        // the (value, index) words of bfd_thermal.hip, decoded as bfd_loss_survey3d does
        maxTissue[f] = best[2 * f] == TH_NO_PAIR ? 0.f : th_key_value(th_pair_key(best[2 * f]));
        argTissue[f] = th_pair_index(best[2 * f]);
        maxWater[f] = best[2 * f + 1] == TH_NO_PAIR ? 0.f : th_key_value(th_pair_key(best[2 * f + 1]));
        argWater[f] = th_pair_index(best[2 * f + 1]);
        for (size_t k = 0; k < N3; k++) {
            eWaterRaw[f * N3 + k] = sums[f * width + k];
            eWater[f * N3 + k] = sums[f * width + N3 + k];
            eTissue[f * N3 + k] = sums[f * width + 2 * N3 + k];
        }
    }
    if (kernelMs) *kernelMs = total;
    return 0;
}

extern "C" int bfd_thermal_set_scale(bfd_thermal s, const double *ratio, int mode)
{
    static const char *who = "bfd_thermal_set_scale";
    if (!s || !ratio) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (mode != TS_MODE_DOUBLE_RATIO && mode != TS_MODE_FLOAT_RATIO) BFD_FAIL(-1, std::string(who) + ": mode must be 0 or 1");
    if (mode == TS_MODE_DOUBLE_RATIO && s->nFields != 1) BFD_FAIL(-1, std::string(who) + ": mode 0 is the scaling of one field");
    for (int f = 0; f < s->nFields; f++)
        if (ratio[f] - ratio[f] != 0.0) BFD_FAIL(-1, std::string(who) + ": every ratio must be finite");
    if (int rc = stage_missing(s, who, V_P)) return rc;
    if (int rc = pick_device(who, s->device)) return rc;
    BFD_STEP(copy_up(s, s->dRatio, ratio, 8 * (size_t)s->nFields));
    s->ratio.assign(ratio, ratio + s->nFields);
    s->mode = mode;
    s->scaled = true;
    s->pmapHeld = false;
    return 0;
}

extern "C" int bfd_thermal_run(bfd_thermal s, const float *cd, const float *cp, const float *qf, const float *initT, int flags, const float *T0,
                               const float *dose0, float Tcore, double dt, int nSteps, const int32_t *fieldOfStep, int nFactorMonitoring, int64_t nPoints,
                               const uint32_t *pointIndex, float *points, int nCaptures, const int32_t *captureStep, double *kernelMs)
{
    static const char *who = "bfd_thermal_run";
    (void)nFactorMonitoring;                          // the study keeps no monitored plane (the flow passes -1 for it, :966, :984, :1055)
    if (!s || !cd || !cp || !qf) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (flags < 0 || flags > 31 || ((flags & 16) && (flags & 3))) BFD_FAIL(-1, std::string(who) + ": flags must be 0 .. 31, bit 4 without bits 0 and 1");
    if (((flags & 1) && !T0) || ((flags & 2) && !dose0)) BFD_FAIL(-1, std::string(who) + ": flags announce a volume that is null");
    const bool fresh = (flags & 4) || !s->ran;
    if (fresh && !(flags & 17) && !initT) BFD_FAIL(-1, std::string(who) + ": a fresh start needs T0 or initT");
    if (nSteps < 0 || (nSteps > 0 && !fieldOfStep)) BFD_FAIL(-1, std::string(who) + ": nSteps is negative or fieldOfStep is null");
    for (int t = 0; t < nSteps; t++)
        if (fieldOfStep[t] < -1 || fieldOfStep[t] >= s->nFields) BFD_FAIL(-1, std::string(who) + ": fieldOfStep entry out of range");
    if (nPoints < 0 || nPoints > 0x7fffffff || (nPoints > 0 && (!pointIndex || !points))) BFD_FAIL(-1, std::string(who) + ": bad point list");
    for (int64_t t = 0; t < nPoints; t++)
        if (pointIndex[t] >= s->n) BFD_FAIL(-1, std::string(who) + ": monitored point outside the volume");
    if (nCaptures < 0 || (nCaptures > 0 && !captureStep)) BFD_FAIL(-1, std::string(who) + ": bad capture list");
    for (int q = 0; q < nCaptures; q++)
        if (captureStep[q] < 0 || captureStep[q] > nSteps || (q > 0 && captureStep[q] < captureStep[q - 1]))
            BFD_FAIL(-1, std::string(who) + ": captureStep must ascend within [0, nSteps]");
    if (!s->inputs) BFD_FAIL(-6, std::string(who) + ": bfd_thermal_set_inputs comes first");
    if (!s->scaled) BFD_FAIL(-6, std::string(who) + ": bfd_thermal_set_scale comes first");
    if ((flags & 16) && !(s->prevT && s->prevDose)) BFD_FAIL(-6, std::string(who) + ": bfd_thermal_set_previous comes first");
    if (int rc = pick_device(who, s->device)) return rc;
    if (kernelMs) *kernelMs = 0.0;
    const size_t quads = s->ns / 4, M = (size_t)s->nMat;
    const bool series = nPoints > 0 && nSteps > 0;
    DevTemp<float> tables, dPts;                      // cd, cp, qf, initT
    DevTemp<unsigned> dIdx;
    BFD_STEP(tables.alloc(4 * M));
    if (series) { BFD_STEP(dIdx.alloc((size_t)nPoints)); BFD_STEP(dPts.alloc((size_t)nPoints * (size_t)nSteps)); }
    BFD_STEP(copy_up(s, tables.p, cd, 4 * M));
    BFD_STEP(copy_up(s, tables.p + M, cp, 4 * M));
    BFD_STEP(copy_up(s, tables.p + 2 * M, qf, 4 * M));
    if (series) BFD_STEP(copy_up(s, dIdx, pointIndex, 4 * (size_t)nPoints));
    s->ran = false;                                   // until this run has ended
    float *Tin = s->T[s->cur];
    if (flags & 1) BFD_STEP(copy_up(s, Tin, T0, 4 * s->n));
    else if (flags & 16) BFD_STEP(hipMemcpyAsync(Tin, s->prevT, 4 * s->ns, hipMemcpyDeviceToDevice, 0));
    else if (fresh) {
        BFD_STEP(copy_up(s, tables.p + 3 * M, initT, 4 * M));
        by_id_width(s, [&](auto *ids) { hipLaunchKernelGGL(study_table_lookup, dim3(grid_of(quads)), dim3(THREADS), 0, 0, ids, (const float *)(tables.p + 3 * M), (float4 *)Tin, quads); });
        BFD_STEP(hipGetLastError());
    }
    if (flags & 2) BFD_STEP(copy_up(s, s->dose, dose0, 4 * s->n));
    else if (flags & 16) BFD_STEP(hipMemcpyAsync(s->dose, s->prevDose, 4 * s->ns, hipMemcpyDeviceToDevice, 0));
    else if (fresh) BFD_STEP(hipMemsetAsync(s->dose, 0, 4 * s->ns, 0));
    for (int f = 0; f < s->nFields; f++) {
        by_id_width(s, [&](auto *ids) {
            hipLaunchKernelGGL(study_heat_source, dim3(grid_of(quads)), dim3(THREADS), 0, 0, (const float4 *)(s->p + (size_t)f * s->ns), ids, (const float *)(tables.p + 2 * M),
                               (float4 *)(s->q + (size_t)f * s->ns), quads, s->ratio[(size_t)f], s->mode);
        });
        BFD_STEP(hipGetLastError());
    }
    const bfd_bhte_device_run r = {1, s->idBytes, s->N3, s->N2, s->N1, s->nMat, {Tin, s->T[1 - s->cur]}, s->dose, s->q, s->ns, s->ids, tables.p, tables.p + M, Tcore, dt,
                                   nSteps, fieldOfStep, -1, 1, nullptr, 0, series ? nPoints : 0, series ? dIdx.p : nullptr, series ? dPts.p : nullptr, nCaptures, captureStep,
                                   s->Tmax, s->doseCap, ((flags & 8) && !fresh) ? 1 : 0};
    int cur = 0;
    BFD_STEP(bfd_stage_bhte_run(r, &cur, kernelMs));
    if (cur) s->cur = 1 - s->cur;
    if (nCaptures == 0) {                             // no capture list: Tmax is T at the end, the dose at capture the dose
        BFD_STEP(hipMemcpyAsync(s->Tmax, s->T[s->cur], 4 * s->ns, hipMemcpyDeviceToDevice, 0));
        BFD_STEP(hipMemcpyAsync(s->doseCap, s->dose, 4 * s->ns, hipMemcpyDeviceToDevice, 0));
    }
    if (series) BFD_STEP(copy_down(s, points, dPts, 4 * (size_t)nPoints * (size_t)nSteps));
    BFD_STEP(hipDeviceSynchronize());
    s->ran = true;
    return 0;
}

extern "C" int bfd_thermal_set_previous(bfd_thermal s, const float *finalTemp, const float *finalDose, const float *tempEndFUS)
{
    static const char *who = "bfd_thermal_set_previous";
    if (!s || !finalTemp || !finalDose || !tempEndFUS) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (int rc = pick_device(who, s->device)) return rc;
    float **held[3] = {&s->prevT, &s->prevDose, &s->prevTend};
    const float *from[3] = {finalTemp, finalDose, tempEndFUS};
    for (int v = 0; v < 3; v++) {
        if (!*held[v]) {
            void *raw = nullptr;
            BFD_STEP(hipMalloc(&raw, 4 * s->ns));
            s->allocs.push_back(raw);
            BFD_STEP(hipMemset(raw, 0, 4 * s->ns));
            *held[v] = (float *)raw;
        }
        BFD_STEP(copy_up(s, *held[v], from[v], 4 * s->n));
    }
    return 0;
}

extern "C" int bfd_thermal_merge_max(bfd_thermal s, int which, const float *hostVolume)
{
    static const char *who = "bfd_thermal_merge_max";
    if (!s) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (which != V_TMAX && which != V_DOSECAP && which != V_T && which != V_DOSE) BFD_FAIL(-1, std::string(who) + ": which must name Tmax, doseAtCapture, T or dose");
    if (int rc = stage_missing(s, who, which)) return rc;
    if (!hostVolume && !s->prevTend) BFD_FAIL(-6, std::string(who) + ": bfd_thermal_set_previous comes first");
    if (int rc = pick_device(who, s->device)) return rc;
    const float *other = s->prevTend;
    if (hostVolume) {
        s->pmapHeld = false;                          // the scratch volume takes the uploaded one
        BFD_STEP(copy_up(s, s->scratch, hostVolume, 4 * s->n));
        other = s->scratch;
    }
    hipLaunchKernelGGL(merge_max, dim3(grid_of(s->ns / 4)), dim3(THREADS), 0, 0, (float4 *)volume_of(s, which), (const float4 *)other, s->ns / 4);
    BFD_STEP(hipGetLastError());
    BFD_STEP(hipDeviceSynchronize());
    return 0;
}

extern "C" int bfd_thermal_extrema(bfd_thermal s, const int *which, int nVol, const uint8_t *classOf, int64_t *count, float *maxIn, int64_t *argIn, float *maxKey,
                                   int64_t *argKey, float *kernelMs)
{
    static const char *who = "bfd_thermal_extrema";
    if (!s || !which || !classOf || !count || !maxIn || !argIn || !maxKey || !argKey) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (nVol < 1 || nVol > 64) BFD_FAIL(-1, std::string(who) + ": nVol must be 1 .. 64");
    for (int v = 0; v < nVol; v++)
        if (which[v] != V_TMAX && which[v] != V_DOSECAP && which[v] != V_T && which[v] != V_DOSE && which[v] != V_PMAP && !(which[v] == V_P && s->nFields == 1))
            BFD_FAIL(-1, std::string(who) + ": a volume must be Tmax, doseAtCapture, T, dose, p_map or, with one field, p");
    for (int v = 0; v < nVol; v++)
        if (int rc = stage_missing(s, who, which[v])) return rc;
    if (int rc = pick_device(who, s->device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    std::vector<const float *> vols((size_t)nVol);
    for (int v = 0; v < nVol; v++) {
        if (which[v] == V_PMAP) BFD_STEP(hold_pmap(s));
        vols[(size_t)v] = volume_of(s, which[v]);
    }
    std::vector<unsigned long long> pairs((size_t)nVol * 8, 0);
    unsigned long long counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t first[8], flags = 0;
    for (int q = 0; q < 8; q++) first[q] = 0xFFFFFFFFu;
    float total = 0.f;
    DevTemp<uint8_t> dtab, dscratch;
    BFD_STEP(dtab.alloc((size_t)s->nMat));
    BFD_STEP(dscratch.alloc(bfd_class_extrema_scratch()));
    BFD_STEP(copy_up(s, dtab, classOf, (size_t)s->nMat));
    BFD_STEP(bfd_stage_class_extrema(vols.data(), nVol, s->ids, s->idBytes, (int64_t)s->n, dtab.p, s->nMat, dscratch.p, pairs.data(), counts, first, &flags, &total,
                                     &s->up, &s->down));
    if (bfd_class_extrema_finish(nVol, pairs.data(), counts, first, flags, count, maxIn, argIn, maxKey, argKey))
        BFD_FAIL(-1, std::string(who) + ": refused data: a value is not finite");
    if (kernelMs) *kernelMs = total;
    return 0;
}

extern "C" int bfd_thermal_get(bfd_thermal s, int which, void *out, int dtype)
{
    static const char *who = "bfd_thermal_get";
    if (!s || !out) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (which < V_TMAX || which > V_P) BFD_FAIL(-1, std::string(who) + ": which names no volume");
    if (dtype != 0 && dtype != 1) BFD_FAIL(-1, std::string(who) + ": dtype must be 0 (float32) or 1 (float64)");
    if (dtype == 1 && !(which == V_PMAP && s->mode == TS_MODE_DOUBLE_RATIO && s->nFields == 1))
        BFD_FAIL(-1, std::string(who) + ": float64 is the type of p_map for one field in mode 0 alone");
    if (int rc = stage_missing(s, who, which)) return rc;
    if (int rc = pick_device(who, s->device)) return rc;
    if (which == V_Q || which == V_PW || which == V_P) {
        const float *src = which == V_Q ? s->q : which == V_PW ? s->pw : s->p;
        for (int f = 0; f < s->nFields; f++) BFD_STEP(copy_down(s, (float *)out + (size_t)f * s->n, src + (size_t)f * s->ns, 4 * s->n));
        return 0;
    }
    if (dtype == 1) {                                 // in pieces through the scratch volume: ns / 2 float64 at a time
        s->pmapHeld = false;
        const size_t piece = s->ns / 2;
        for (size_t first = 0; first < s->n; first += piece) {
            const size_t cnt = std::min(piece, s->n - first);
            hipLaunchKernelGGL(scaled64, dim3(grid_of(cnt)), dim3(THREADS), 0, 0, (const float *)s->p, first, cnt, s->ratio[0], (double *)s->scratch);
            BFD_STEP(hipGetLastError());
            BFD_STEP(copy_down(s, (double *)out + first, s->scratch, 8 * cnt));
        }
        return 0;
    }
    if (which == V_PMAP) BFD_STEP(hold_pmap(s));
    BFD_STEP(copy_down(s, out, volume_of(s, which), 4 * s->n));
    return 0;
}

extern "C" int bfd_thermal_get_plane(bfd_thermal s, int which, int64_t j, void *out)
{
    static const char *who = "bfd_thermal_get_plane";
    if (!s || !out) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (which != V_PMAP && which != V_MAP && !(which == V_P && s->nFields == 1))
        BFD_FAIL(-1, std::string(who) + ": which must be BFD_THERMAL_P_MAP, BFD_THERMAL_MAP or, with one field, BFD_THERMAL_P");
    if (j < 0 || j >= s->N2) BFD_FAIL(-1, std::string(who) + ": the plane lies outside the volume");
    if (int rc = stage_missing(s, who, which)) return rc;
    if (int rc = pick_device(who, s->device)) return rc;
    const size_t cells = (size_t)s->N1 * (size_t)s->N3;
    DevTemp<uint32_t> plane;
    BFD_STEP(plane.alloc(cells));
    if (which != V_MAP) {
        if (which == V_PMAP) BFD_STEP(hold_pmap(s));
        hipLaunchKernelGGL(plane_f32, dim3(grid_of(cells)), dim3(THREADS), 0, 0, (const float *)volume_of(s, which), (float *)plane.p, (size_t)s->N1, (size_t)s->N2, (size_t)s->N3, (size_t)j);
    } else
        by_id_width(s, [&](auto *ids) { hipLaunchKernelGGL(plane_ids, dim3(grid_of(cells)), dim3(THREADS), 0, 0, ids, plane.p, (size_t)s->N1, (size_t)s->N2, (size_t)s->N3, (size_t)j); });
    BFD_STEP(hipGetLastError());
    BFD_STEP(copy_down(s, out, plane, 4 * cells));
    return 0;
}

extern "C" int bfd_thermal_traffic(bfd_thermal s, int64_t *bytesUp, int64_t *bytesDown)
{
    if (!s || !bytesUp || !bytesDown) BFD_FAIL(-1, "bfd_thermal_traffic: null argument");
    *bytesUp = s->up; *bytesDown = s->down;
    return 0;
}
