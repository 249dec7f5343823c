// Result packing of libbabelfdtd_hip.so (bfd_pack_results, include/babelfdtd.h): the Pressure RMS map and the per-sensor DFT sums and peaks of the
// engine, which live in x-fastest order, become the cropped, zeroed, scaled and flipped volumes the caller saves, which are k-fastest. gfx950 only.
//
// One kernel class, pack_tile<KIND>: a workgroup owns a 64 (i) x 64 (k) tile of one output row j. Its lanes first run along i and read the engine's
// arrays in full lines (4 B of the accumulator, 16 B of the DFT sums or 4 B of the peaks per lane), then, through an LDS tile, run along k and write
// the output in full lines (4 B, or 8 B for the complex map). The tile rows are padded by one element of the access width (4 B / 8 B): the
// transposed read then has stride 65 (130) dwords and meets no bank twice within a 32-lane half. Every output voxel is written exactly once, the
// zeros included, so there is no fill pass, no scatter and no atomic. Sensor sets that are not a dense box take pack_list instead: one zero fill, then
// one lane per sensor stores its value where the voxel lands (pack_output_index); same values. pack_map carries the study's maps along: both sides
// are k-fastest there, so it is a plain copy with the last axis reversed. The stages at the end are what bfd_pack_results and the acoustic study
// (bfd_acoustic.hip) both run.
#include "bfd_internal.h"
#include "bfd_pack_core.h"
#include "bfd_domain_stages.h"

#include <math.h>

namespace {

enum { PACK_AMP = 0, PACK_COMPLEX = 1, PACK_PEAK = 2 };
#define PACK_TILE 64

struct PackArgs {
    PackGeom g;
    PackBox box;
    int N1, plane;
    const float *acc; float cnt;                    // Pressure accumulator of the slab (x-fastest), number of accumulated steps
    const double *dft; const float *pk; double sc;  // DFT sums [nSensors][2] and peaks [nSensors] of Pressure, 2 / nTs
    int scale; double ampScale; float correction;
};

template <int KIND> struct PackElem { typedef float type; };
template <> struct PackElem<PACK_COMPLEX> { typedef float2 type; };

__device__ __forceinline__ float2 dft_value(const PackArgs &A, long s)
{
    const double2 a = reinterpret_cast<const double2 *>(A.dft)[s];
    float re = (float)(a.x * A.sc), im = (float)(a.y * A.sc);            // finalize_sensor_dft (bfd_outputs.hip)
    if (A.scale) { re = pack_scale_f32(re, A.correction); im = pack_scale_f32(im, A.correction); }
    return make_float2(re, im);
}
__device__ __forceinline__ float peak_value(const PackArgs &A, long s)
{
    const float p = A.pk[s];
    return A.scale ? pack_scale_f32(p, A.correction) : p;
}

template <int KIND>
__global__ __launch_bounds__(256) void pack_tile(PackArgs A, typename PackElem<KIND>::type *__restrict__ out)
{
    typedef typename PackElem<KIND>::type T;
    __shared__ T tile[PACK_TILE][PACK_TILE + 1];
    const PackGeom &g = A.g;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int c0 = blockIdx.x * PACK_TILE, a0 = blockIdx.y * PACK_TILE;
    for (int b = blockIdx.z; b < g.O[1]; b += gridDim.z) {
        for (int r = ty; r < PACK_TILE; r += 4) {                       // lanes along i: row r of the tile is output column c0 + r
            const int a = a0 + tx, c = c0 + r;
            T v;
            if (KIND == PACK_COMPLEX) *reinterpret_cast<float2 *>(&v) = make_float2(0.0f, 0.0f); else *reinterpret_cast<float *>(&v) = 0.0f;
            int i, j, k;
            if (a < g.O[0] && c < g.O[2] && pack_source_voxel(g, a, b, c, i, j, k)) {
                if (KIND == PACK_AMP) {
                    float x = sqrtf(A.acc[(long)k * A.plane + (long)j * A.N1 + i] / A.cnt);      // finalize_rms (bfd_outputs.hip)
                    if (A.scale) x = pack_scale_amp(x, A.ampScale);
                    *reinterpret_cast<float *>(&v) = x;
                } else {
                    const long s = pack_box_sensor(A.box, i, j, k);
                    if (s >= 0) {
                        if (KIND == PACK_COMPLEX) *reinterpret_cast<float2 *>(&v) = dft_value(A, s);
                        else *reinterpret_cast<float *>(&v) = peak_value(A, s);
                    }
                }
            }
            tile[r][tx] = v;
        }
        __syncthreads();
        for (int r = ty; r < PACK_TILE; r += 4) {                       // lanes along k: row r is output row a0 + r
            const int a = a0 + r, c = c0 + tx;
            if (a < g.O[0] && c < g.O[2]) out[((long)a * g.O[1] + b) * g.O[2] + c] = tile[tx][r];
        }
        __syncthreads();
    }
}

// any sensor list: the outputs were zeroed; sensor s stores where its voxel lands, if it lands
__global__ void pack_list(PackArgs A, const uint32_t *__restrict__ lin, long nSens, float2 *__restrict__ outC, float *__restrict__ outP)
{
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < nSens; s += (long)gridDim.x * blockDim.x) {
        const unsigned cell = lin[s], kl = cell / (unsigned)A.plane, r = cell - kl * (unsigned)A.plane, j = r / (unsigned)A.N1, i = r - j * (unsigned)A.N1;
        const long o = pack_output_index(A.g, (int)i, (int)j, (int)kl);
        if (o < 0) continue;
        if (outC) outC[o] = dft_value(A, s);
        if (outP) outP[o] = peak_value(A, s);
    }
}

// A volume in the caller's C order (k fastest) cropped, pasted and flipped: both sides are k-fastest, so lanes along the output's last axis read a
// contiguous run of the source, ascending or (flipped) descending; TO = uint32 or, for a mask, uint8
template <typename TO>
__global__ __launch_bounds__(256) void pack_map(PackGeom g, int N2, int N3, const uint32_t *__restrict__ in, TO *__restrict__ out, unsigned total)
{
    // 32-bit index arithmetic: the output has fewer than 2^31 voxels (bfd_pack_arguments), and the grid-stride sum stays below 2^32
    for (unsigned v = blockIdx.x * blockDim.x + threadIdx.x; v < total; v += gridDim.x * blockDim.x) {
        const unsigned row = v / (unsigned)g.O[2];
        const int c = (int)(v - row * (unsigned)g.O[2]);
        const int a = (int)(row / (unsigned)g.O[1]), b = (int)(row - (unsigned)a * (unsigned)g.O[1]);
        const int cc = g.flipK ? g.O[2] - 1 - c : c;
        const int u = a - g.at[0], w1 = b - g.at[1], w = cc - g.at[2];
        uint32_t x = 0;
        if (u >= 0 && u < g.keep[0] && w1 >= 0 && w1 < g.keep[1] && w >= 0 && w < g.keep[2])
            x = in[((long)(g.lo[0] + u) * N2 + (g.lo[1] + w1)) * N3 + (g.lo[2] + w)];
        out[v] = (TO)x;
    }
}

template <int KIND>
void launch_tile(const PackArgs &A, typename PackElem<KIND>::type *out, hipStream_t st)
{
    const PackGeom &g = A.g;
    const dim3 grid((g.O[2] + PACK_TILE - 1) / PACK_TILE, (g.O[0] + PACK_TILE - 1) / PACK_TILE, std::min(g.O[1], 65535));
    hipLaunchKernelGGL((pack_tile<KIND>), grid, dim3(PACK_TILE, 4), 0, st, A, out);
}

int slot_of(const int *sel, int n, int map)
{
    for (int q = 0; q < n; q++) if (sel[q] == map) return q;
    return -1;
}

}  // namespace

static PackGeom geometry_of(const bfd_sim *s, const bfd_pack_spec &sp)
{
    const int dim[3] = {s->d.N1, s->d.N2, s->d.nk};
    PackGeom g;
    for (int a = 0; a < 3; a++) { g.lo[a] = sp.lo[a]; g.keep[a] = dim[a] - sp.hi[a] - sp.lo[a]; g.O[a] = sp.O[a]; g.at[a] = sp.at[a]; }
    g.zSource = sp.zSource; g.k0 = s->d.k0; g.flipK = sp.flipK;
    return g;
}

// The launch sequence into device volumes (each may be null) on the sim's stream; the caller has checked the spec and what the sim holds
static hipError_t pack_into(bfd_sim *s, const bfd_pack_spec &sp, float *dAmp, float2 *dComplex, float *dPeak)
{
    const bfd_dev &d = s->d;
    PackArgs A = {};
    A.g = geometry_of(s, sp);
    A.N1 = d.N1; A.plane = d.plane;
    A.scale = sp.applyScale; A.ampScale = sp.ampScale; A.correction = (float)sp.correction;
    const size_t nOut = (size_t)sp.O[0] * sp.O[1] * sp.O[2];
    if (dAmp) {
        const int nAcc = s->step - s->accStart;
        A.acc = s->acc + (size_t)slot_of(s->selR, s->nSelR, BFD_MAP_PRESSURE) * s->nloc; A.cnt = (float)(nAcc > 0 ? nAcc : 1);
        launch_tile<PACK_AMP>(A, dAmp, s->stream);
    }
    if (!dComplex && !dPeak) return hipGetLastError();
    const size_t q = (size_t)slot_of(s->selS, s->nSelS, BFD_MAP_PRESSURE);
    A.dft = s->dftAcc + 2 * q * (size_t)s->nSensors; A.pk = s->dftPk + q * (size_t)s->nSensors; A.sc = 2.0 / (double)s->nTs;
    if (s->sensIsBox || !s->nSensors) {
        const int bx = s->sensBox[0], by = s->sensBox[1];
        if (s->nSensors) A.box = PackBox{bx, by, (int)(s->nSensors / ((int64_t)bx * by)), s->sensBox[2], s->sensBox[3], s->sensBox[4]};     // else an empty box: zeros
        if (dComplex) launch_tile<PACK_COMPLEX>(A, dComplex, s->stream);
        if (dPeak) launch_tile<PACK_PEAK>(A, dPeak, s->stream);
        return hipGetLastError();
    }
    hipError_t e = hipSuccess;
    if (dComplex) e = hipMemsetAsync(dComplex, 0, nOut * sizeof(float2), s->stream);
    if (e == hipSuccess && dPeak) e = hipMemsetAsync(dPeak, 0, nOut * sizeof(float), s->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pack_list, dim3(grid_for((long)s->nSensors)), dim3(256), 0, s->stream, A, s->sensLin, (long)s->nSensors, dComplex, dPeak);
    return hipGetLastError();
}

int bfd_pack_arguments(const char *who_, const bfd_sim *s, const bfd_pack_spec *spec, bool wantAmp, bool wantSensors)
{
    const std::string who = std::string(who_) + ": ";
    if (!s || !spec) BFD_FAIL(-1, who + "null argument");
    const bfd_pack_spec &sp = *spec;
    if ((sp.flipK != 0 && sp.flipK != 1) || (sp.applyScale != 0 && sp.applyScale != 1)) BFD_FAIL(-1, who + "flipK and applyScale are 0 or 1");
    if (sp.applyScale && (!std::isfinite(sp.ampScale) || !std::isfinite(sp.correction))) BFD_FAIL(-1, who + "a scale is not finite");
    const int dim[3] = {s->d.N1, s->d.N2, s->d.nk};
    for (int a = 0; a < 3; a++)
        if (sp.lo[a] < 0 || sp.hi[a] < 0 || (int64_t)sp.lo[a] + sp.hi[a] >= dim[a]) BFD_FAIL(-1, who + "lo / hi leave no kept region inside the slab");
    if (sp.O[0] <= 0 || sp.O[1] <= 0 || sp.O[2] <= 0 || (int64_t)sp.O[0] * sp.O[1] > 0x7FFFFFFF / (int64_t)sp.O[2])
        BFD_FAIL(-1, who + "the output shape must be positive and below 2^31 voxels");
    for (int a = 0; a < 3; a++)
        if (sp.at[a] < 0 || (int64_t)sp.at[a] + (dim[a] - sp.hi[a] - sp.lo[a]) > sp.O[a]) BFD_FAIL(-1, who + "the kept region does not lie inside the output at this offset");
    if (wantAmp && (!s->acc || slot_of(s->selR, s->nSelR, BFD_MAP_PRESSURE) < 0)) BFD_FAIL(-2, who + "pAmp needs the Pressure RMS map (selMapsRMS, SelRMSorPeak)");
    if (wantSensors && s->nSensors && (!s->dftAcc || slot_of(s->selS, s->nSelS, BFD_MAP_PRESSURE) < 0))
        BFD_FAIL(-2, who + "pComplex and pPeak need sensorMode 1 with Pressure among the sensor maps");
    return 0;
}

int bfd_stage_pack_results(bfd_sim *s, const bfd_pack_spec *spec, float *dAmp, float *dComplex, float *dPeak)
{
    BFD_HIP(hipSetDevice(s->cfg.device));
    { const int rc = flush_pending(s); if (rc) return rc; }
    BFD_HIP(pack_into(s, *spec, dAmp, (float2 *)dComplex, dPeak));
    return 0;
}

hipError_t bfd_stage_pack_map(bfd_sim *s, const bfd_pack_spec *spec, const uint32_t *dVolume, void *dOut, int outBytes)
{
    const PackGeom g = geometry_of(s, *spec);
    const long total = (long)g.O[0] * g.O[1] * g.O[2];
    if (outBytes == 1) hipLaunchKernelGGL(pack_map<uint8_t>, dim3(grid_for(total)), dim3(256), 0, s->stream, g, s->d.N2, s->d.nk, dVolume, (uint8_t *)dOut, (unsigned)total);
    else hipLaunchKernelGGL(pack_map<uint32_t>, dim3(grid_for(total)), dim3(256), 0, s->stream, g, s->d.N2, s->d.nk, dVolume, (uint32_t *)dOut, (unsigned)total);
    return hipGetLastError();
}

extern "C" int bfd_pack_results(bfd_sim *s, const bfd_pack_spec *spec, float *pAmp, float *pComplex, float *pPeak, float *kernelMs)
{
    if (int rc = bfd_pack_arguments("bfd_pack_results", s, spec, pAmp != nullptr, pComplex || pPeak)) return rc;
    const bfd_pack_spec &sp = *spec;
    if (kernelMs) *kernelMs = 0.0f;
    if (!pAmp && !pComplex && !pPeak) return 0;
    BFD_HIP(hipSetDevice(s->cfg.device));
    { const int rc = flush_pending(s); if (rc) return rc; }
    const size_t nOut = (size_t)sp.O[0] * sp.O[1] * sp.O[2];
    DevTemp<float> dAmp(true), dPeak(true); DevTemp<float2> dComplex(true);
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t e = hipSuccess;
    if (pAmp) e = dAmp.alloc(nOut);
    if (e == hipSuccess && pComplex) e = dComplex.alloc(nOut);
    if (e == hipSuccess && pPeak) e = dPeak.alloc(nOut);
    for (int q = 0; q < 2 && e == hipSuccess; q++) e = hipEventCreate(&ev[q]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], s->stream);
    if (e == hipSuccess) e = pack_into(s, sp, dAmp, dComplex, dPeak);
    if (e == hipSuccess) e = hipEventRecord(ev[1], s->stream);
    if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    if (e == hipSuccess && pAmp) e = hipMemcpy(pAmp, dAmp, nOut * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && pComplex) e = hipMemcpy(pComplex, dComplex, nOut * sizeof(float2), hipMemcpyDeviceToHost);
    if (e == hipSuccess && pPeak) e = hipMemcpy(pPeak, dPeak, nOut * sizeof(float), hipMemcpyDeviceToHost);
    for (hipEvent_t x : ev) if (x) hipEventDestroy(x);
    if (e != hipSuccess) { (void)hipGetLastError(); BFD_FAIL(-10, std::string("bfd_pack_results: ") + hipGetErrorString(e)); }
    if (kernelMs) *kernelMs = ms;
    return 0;
}
