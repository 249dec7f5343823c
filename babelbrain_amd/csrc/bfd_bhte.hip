// Pennes bio-heat equation on MI355X: explicit 7-point FDTD + CEM43 thermal dose.
//
// Replaces `BabelViscoFDTD.tools.RayleighAndBHTE.BHTE` (package absent from /root/reference), which
// BabelBrain's Step 3 calls with the Step-2 pressure amplitude map:
//     ResTemp,ResDose,MonitorSlice,Qarr,TemperaturePoints = BHTE(PMaps, MaterialMap, MaterialList, dx,
//            TotalDurationSteps, nStepsOn, cy, nFactorMonitoring=, dt=, DutyCycle=, Backend=, initT0=, initDose=,
//            MonitoringPointsMap=, stableTemp=)            ThermalModeling/CalculateTemperatureEffects.py:365-456, 960
// Scheme (documented restatement; parity with the package unpinned):
//   T' = T + cd[m] * (((((Txm+Txp)+Tym)+Typ)+Tzm)+Tzp - 6 T) + cp[m] * (Tcore - T) + (n < nStepsOn ? q : 0)
//   cd = dt k/(rho c dx^2),  cp = dt rho_b c_b w / (6e7 c)  (w in mL/min/kg),  q = dt * duty * a_abs p^2/(rho c_s) / (rho c)
//   dose += dt/60 * R^(43 - T'),  R = 0.5 for T' >= 43 else 0.25 (evaluated as exp2).   Faces of the volume keep their temperature.
// Bound: HBM. One step moves T read + write, q read, dose RMW, uint8 ids (uint16 for lists of more than 256 materials, below): ~21 B per voxel; the default path takes FOUR steps per
// launch (round 6: bhte_stepNg; stretches it cannot take go to the two-step kernel bhte_step2g and the one-step kernel) and moves those bytes
// once for all of them. x-fastest layout.
// This file is the host side: the entry points, the run behind them and the step loop. The kernels and their launchers are in bfd_bhte_kernels.hip
// (bfd_bhte_launch.h); what a run decides before it launches anything -- regions, pads, grids, switches, passes -- is in bfd_bhte_plan_core.h.
#include "bfd_internal.h"
#include "bfd_bhte_launch.h"
#include <math.h>
#include <vector>

void bfd_bhte_pads(int N1, size_t *front, size_t *back) { bhte_pads(N1, front, back); }

// The step loop of a run on device pointers (bfd_thermal_stages.h): what bhte_run_core does between its uploads and its downloads, and what the
// thermal study (bfd_thermal_study.hip) runs on its resident volumes. Geometry, then the plan, then the plan's launches between two events.
// Steps per pass: FOUR by default (BFD_BHTE_STEPS=2 / 3 / 4 forces one length). Gvoxel-steps/s at 320^3 / 512^3 (scripts/r6/bhte_phases.sh, bhte_nc_ab.sh,
// profiles/r6/bhte_steps_per_pass.txt): nothing heats -- two steps 470 / 515, three 568 / 679, four 710-728 / 795-810 (four cells per thread: 99-128 registers,
// 2 spilled); a field heats -- two 374 / 395, three 487 / 568, four with four cells per thread 382-397 / 380-403 (its heat-source queue spills 18 registers
// to scratch), four with TWO cells per thread 564 / 642 (82 registers, none spilled: GNCells).
hipError_t bfd_stage_bhte_run(const bfd_bhte_device_run &r, int *curOut, double *kernelMs)
{
    const bhte_knobs knobs = bhte_knobs_from_env();
    bhte_geom geom[BHTE_SMAX + 1] = {};
    bool fits[BHTE_SMAX + 1] = {};
    for (int S = BHTE_SMIN; S <= BHTE_SMAX; S++) { geom[S] = bhte_pass_geom(r.N1, r.N2, r.N3, S, knobs.zrun); fits[S] = bhte_geom_fits(geom[S]); }
    const std::vector<bhte_pass> plan = bhte_plan_passes(r.fieldOfStep, r.nSteps, r.captureStep, r.nCaptures, knobs, fits);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipEventCreate(&e0); hipEventCreate(&e1); hipEventRecord(e0, 0);
    int cur = 0, nextCap = 0;
    for (const bhte_pass &p : plan) {
        nextCap = bhte_launch_captures(r, cur, p.first, nextCap);
        bhte_launch_inner_monitors(r, cur, p);
        bhte_launch_pass(r, cur, p, geom[p.length >= BHTE_SMIN ? p.length : BHTE_SMIN]);
        cur = 1 - cur;
        bhte_launch_monitors(r, cur, p.first + p.length - 1);
    }
    bhte_launch_captures(r, cur, r.nSteps, nextCap);
    hipEventRecord(e1, 0);
    hipError_t e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess && kernelMs) { float ms = 0; hipEventElapsedTime(&ms, e0, e1); *kernelMs = ms; }
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    *curOut = cur;
    return e;
}

// The run behind all entry points. F, M, S: extents of the fastest, middle and slowest axis of the volumes as they lie in memory.
// q (host, nFields volumes) or, if null, pressure + qf: the heat increments are then computed on the device (and copied to qOut).
// initT (per material) replaces the upload of T when flags bit 0 is clear; the dose starts from zero when bit 1 is clear.
// Captures (bfd_bhte_run_protocol; the other entry points pass none): at step boundary captureStep[c] (after step captureStep[c] - 1)
// Tmax = max(Tmax, T) (the first copies T) and doseCap = dose; no pass crosses a capture boundary.
// ID: the width of the material ids (unsigned char: nMat <= 256; uint16_t: nMat <= BFD_BHTE_MAX_MATERIALS); the launchers select the kernels' overloads by it.
template <bool REV, typename ID>
static int bhte_run_core(int32_t device, int32_t F, int32_t M, int32_t S, int32_t nMat, const ID *mat, const float *cd, const float *cp,
                         const float *qf, const float *initT, int32_t nFields, const float *q, const float *pressure, float *qOut, float *T, float *dose,
                         int32_t flags, float Tcore, double dt, int32_t nSteps, const int32_t *fieldOfStep, int32_t sliceJ, int32_t nFactorMonitoring,
                         float *monitorSlice, int64_t nPoints, const uint32_t *pointIndex, float *points, double *kernelMs,
                         int32_t nCaptures = 0, const int32_t *captureStep = nullptr, float *Tmax = nullptr, float *doseCap = nullptr)
{
    const int maxMat = sizeof(ID) == 1 ? 256 : BFD_BHTE_MAX_MATERIALS, idBits = 8 * (int)sizeof(ID);
    if (nMat > maxMat) {
        bfd_set_error("bfd_bhte_run: " + std::to_string(nMat) + " materials, at most " + std::to_string(maxMat) + " with " + std::to_string(idBits) + "-bit ids" +
                      (sizeof(ID) == 1 ? " (bfd_bhte_run_volumes16 / bfd_bhte_run_protocol16 take up to " + std::to_string(BFD_BHTE_MAX_MATERIALS) + ")" : std::string()));
        return -1;
    }
    if (F < 3 || M < 3 || S < 3 || nMat < 1 || nFields < 1 || !mat || !cd || !cp || (!q && !(pressure && qf)) || !T || !dose || nSteps < 0 ||
        (nSteps > 0 && !fieldOfStep) || (!(flags & 1) && !initT) || nCaptures < 0 || (nCaptures > 0 && !(captureStep && Tmax && doseCap))) {
        bfd_set_error("bfd_bhte_run: bad argument"); return -1;
    }
    for (int s = 0; s < nSteps; s++)
        if (fieldOfStep[s] < -1 || fieldOfStep[s] >= nFields) { bfd_set_error("bfd_bhte_run: fieldOfStep entry out of range"); return -1; }
    for (int c = 0; c < nCaptures; c++)
        if (captureStep[c] < 0 || captureStep[c] > nSteps || (c > 0 && captureStep[c] < captureStep[c - 1])) {
            bfd_set_error("bfd_bhte_run: captureStep must ascend within [0, nSteps]"); return -1;
        }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { bfd_set_error("bfd_bhte_run: no HIP device available (no CPU fallback)"); return -3; }
    if (device < 0 || device >= ndev) { bfd_set_error("bfd_bhte_run: device ordinal out of range"); return -3; }
    BFD_HIP(hipSetDevice(device));
    const int N1 = F, N2 = M, N3 = S;                            // the kernels' names: x fastest
    const size_t n = (size_t)N1 * N2 * N3;
    if (sliceJ >= N2) { bfd_set_error("bfd_bhte_run: monitored plane outside the volume"); return -1; }
    for (int64_t t = 0; t < nPoints && pointIndex && points; t++)
        if (pointIndex[t] >= n) { bfd_set_error("bfd_bhte_run: monitored point outside the volume"); return -1; }
    const int fm = nFactorMonitoring > 0 ? nFactorMonitoring : 1;
    const long nSamples = (monitorSlice && sliceJ >= 0) ? (nSteps + fm - 1) / fm : 0;
    float *dT[2] = {nullptr, nullptr}, *dDose = nullptr, *dq = nullptr, *dcd = nullptr, *dcp = nullptr, *dqf = nullptr, *dSlice = nullptr, *dPts = nullptr;
    float *dTmax = nullptr, *dDoseCap = nullptr;
    ID *dmat = nullptr; unsigned *dIdx = nullptr;
    std::vector<void *> allocs;
    auto A = [&](void **p, size_t bytes) { hipError_t e = hipMalloc(p, bytes ? bytes : 1); if (e == hipSuccess) allocs.push_back(*p); return e; };
    // the volumes carry pads (elements): the multi-step kernels address every cell of their regions, also those that hang over the faces (bhte_pads)
    size_t padF = 0, padB = 0;
    bfd_bhte_pads(N1, &padF, &padB);
    auto AP = [&](void **p, size_t elems, size_t elemBytes) {
        void *raw = nullptr; const hipError_t e = A(&raw, (padF + elems + padB) * elemBytes);
        if (e == hipSuccess) *p = (char *)raw + padF * elemBytes;
        return e;
    };
    hipError_t e = AP((void **)&dT[0], n, 4);
    if (e == hipSuccess) e = AP((void **)&dT[1], n, 4);
    if (e == hipSuccess) e = AP((void **)&dDose, n, 4);
    if (e == hipSuccess) e = AP((void **)&dq, n * (size_t)nFields, 4);
    if (e == hipSuccess) e = AP((void **)&dmat, n, sizeof(ID));
    if (e == hipSuccess && nCaptures) e = AP((void **)&dTmax, n, 4);
    if (e == hipSuccess && nCaptures) e = AP((void **)&dDoseCap, n, 4);
    if (e == hipSuccess) e = A((void **)&dcd, nMat * 4);
    if (e == hipSuccess) e = A((void **)&dcp, nMat * 4);
    if (e == hipSuccess) e = A((void **)&dqf, nMat * 4);
    if (e == hipSuccess && nSamples) e = A((void **)&dSlice, (size_t)N1 * N3 * nSamples * 4);
    if (e == hipSuccess && nPoints && points) { e = A((void **)&dIdx, nPoints * 4); if (e == hipSuccess) e = A((void **)&dPts, (size_t)nPoints * nSteps * 4); }
    // 16-bit ids index the LDS table of the multi-step kernels: the ring cells that lie in the pads must read an id inside it too (any byte is inside the 8-bit table)
    if (e == hipSuccess && sizeof(ID) > 1) e = hipMemset(dmat - padF, 0, (padF + n + padB) * sizeof(ID));
    if (e == hipSuccess) e = hipMemcpy(dmat, mat, n * sizeof(ID), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dcd, cd, nMat * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dcp, cp, nMat * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (flags & 1) e = hipMemcpy(dT[0], T, n * 4, hipMemcpyHostToDevice);
        else {                                                                   // T = initT[material], via the table slot of qf
            e = hipMemcpy(dqf, initT, nMat * 4, hipMemcpyHostToDevice);
            if (e == hipSuccess) { bhte_launch_table_lookup((int)sizeof(ID), dmat, dqf, dT[0], n); e = hipDeviceSynchronize(); }
        }
    }
    if (e == hipSuccess) e = (flags & 2) ? hipMemcpy(dDose, dose, n * 4, hipMemcpyHostToDevice) : hipMemset(dDose, 0, n * 4);
    if (e == hipSuccess) {
        if (q) e = hipMemcpy(dq, q, n * 4 * (size_t)nFields, hipMemcpyHostToDevice);
        else {                                                                   // q = (p p) qf[material], in place
            e = hipMemcpy(dqf, qf, nMat * 4, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(dq, pressure, n * 4 * (size_t)nFields, hipMemcpyHostToDevice);
            for (int f = 0; f < nFields && e == hipSuccess; f++) bhte_launch_heat_source((int)sizeof(ID), dq + (size_t)f * n, dmat, dqf, dq + (size_t)f * n, n);
            if (e == hipSuccess && qOut) e = hipMemcpy(qOut, dq, n * 4 * (size_t)nFields, hipMemcpyDeviceToHost);
        }
    }
    if (e == hipSuccess && dIdx) e = hipMemcpy(dIdx, pointIndex, nPoints * 4, hipMemcpyHostToDevice);
    int cur = 0;
    if (e == hipSuccess) {
        const bfd_bhte_device_run r = {REV ? 1 : 0, (int)sizeof(ID), N1, N2, N3, nMat, {dT[0], dT[1]}, dDose, dq, n, dmat, dcd, dcp, Tcore, dt, nSteps, fieldOfStep,
                                       sliceJ, fm, dSlice, nSamples, nPoints, dIdx, dPts, nCaptures, captureStep, dTmax, dDoseCap, 0};
        e = bfd_stage_bhte_run(r, &cur, kernelMs);
    }
    if (e == hipSuccess) e = hipMemcpy(T, dT[cur], n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(dose, dDose, n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && dSlice) e = hipMemcpy(monitorSlice, dSlice, (size_t)N1 * N3 * nSamples * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && dPts) e = hipMemcpy(points, dPts, (size_t)nPoints * nSteps * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && dTmax) e = hipMemcpy(Tmax, dTmax, n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && dDoseCap) e = hipMemcpy(doseCap, dDoseCap, n * 4, hipMemcpyDeviceToHost);
    for (void *p : allocs) hipFree(p);
    if (e != hipSuccess) { bfd_set_error(std::string("bfd_bhte_run: ") + hipGetErrorString(e)); return -10; }
    return 0;
}

// All volumes x-fastest (i + N1*(j + N2*k)), float32; mat uint8 ids into cd/cp (nMat <= 256).
// T, dose: in/out (initial -> final). q: heat increment per ON step (already multiplied by dt*duty/(rho c)).
// monitorSlice (may be NULL): [N1][N3][nSliceSamples], plane j = sliceJ sampled every nFactorMonitoring steps.
// points (may be NULL): [nPoints][nSteps], temperature after every step at the listed voxels.
// q: nFields volumes, one per pressure field (BHTEMultiplePressureFields: steered multi-point sonications,
// CalculateTemperatureEffects.py:381, 978). fieldOfStep[s] = which of them heats during step s, -1 = none.
extern "C" int bfd_bhte_run_fields(int32_t device, int32_t N1, int32_t N2, int32_t N3, int32_t nMat, const unsigned char *mat,
                                   const float *cd, const float *cp, int32_t nFields, const float *q, float *T, float *dose,
                                   float Tcore, double dt, int32_t nSteps, const int32_t *fieldOfStep, int32_t sliceJ,
                                   int32_t nFactorMonitoring, float *monitorSlice, int64_t nPoints, const uint32_t *pointIndex,
                                   float *points, double *kernelMs)
{
    if (!q) { bfd_set_error("bfd_bhte_run: bad argument"); return -1; }
    return bhte_run_core<false, unsigned char>(device, N1, N2, N3, nMat, mat, cd, cp, nullptr, nullptr, nFields, q, nullptr, nullptr, T, dose, 3, Tcore, dt, nSteps, fieldOfStep,
                                sliceJ, nFactorMonitoring, monitorSlice, nPoints, pointIndex, points, kernelMs);
}

// The same run on volumes in the CALLER'S numpy C order -- [N1][N2][N3], the last axis fastest -- so that the host transposes
// nothing (at 384^3 the transposes and the float32 products of the heat source were 2 s of a 2.3 s call whose kernels take
// 0.03 s), and with the heat source computed on the device: q = (p p) qf[material] from the pressure amplitude(s) `pressure`
// (nFields volumes, float32 Pa) and the per-material factor qf; qOut (may be NULL) receives it. The neighbours are summed
// axis 0 first, like the oracle does on such arrays. flags bit 0: T holds the initial temperature (else initT[material]);
// bit 1: dose holds the initial dose (else zero). monitorSlice: [N1][N3][nSamples] = T[:, sliceJ, :]; pointIndex: C-order
// linear indices (i*N2 + j)*N3 + k.
extern "C" int bfd_bhte_run_volumes(int32_t device, int32_t N1, int32_t N2, int32_t N3, int32_t nMat, const unsigned char *mat,
                                    const float *cd, const float *cp, const float *qf, const float *initT, int32_t nFields,
                                    const float *pressure, float *qOut, float *T, float *dose, int32_t flags, float Tcore, double dt,
                                    int32_t nSteps, const int32_t *fieldOfStep, int32_t sliceJ, int32_t nFactorMonitoring,
                                    float *monitorSlice, int64_t nPoints, const uint32_t *pointIndex, float *points, double *kernelMs)
{
    if (!pressure || !qf) { bfd_set_error("bfd_bhte_run_volumes: bad argument"); return -1; }
    return bhte_run_core<true, unsigned char>(device, N3, N2, N1, nMat, mat, cd, cp, qf, initT, nFields, nullptr, pressure, qOut, T, dose, flags, Tcore, dt, nSteps, fieldOfStep,
                               sliceJ, nFactorMonitoring, monitorSlice, nPoints, pointIndex, points, kernelMs);
}

// A whole repeated-sonication protocol (the caller's RunBHTECycles loop, CalculateTemperatureEffects.py:259-460) as one run of
// bfd_bhte_run_volumes: fieldOfStep spans every ON call, OFF call and group pause back to back, the volumes are uploaded once and
// downloaded once, and at each captureStep boundary (the end of an ON call) Tmax = max(Tmax, T) and doseAtCapture = dose on the
// device. The reference discards the monitored plane of these calls: sliceJ must be -1.
extern "C" int bfd_bhte_run_protocol(int32_t device, int32_t N1, int32_t N2, int32_t N3, int32_t nMat, const unsigned char *mat,
                                     const float *cd, const float *cp, const float *qf, const float *initT, int32_t nFields,
                                     const float *pressure, float *qOut, float *T, float *dose, int32_t flags, float Tcore, double dt,
                                     int32_t nSteps, const int32_t *fieldOfStep, int32_t sliceJ, int32_t nFactorMonitoring,
                                     float *monitorSlice, int64_t nPoints, const uint32_t *pointIndex, float *points, double *kernelMs,
                                     int32_t nCaptures, const int32_t *captureStep, float *Tmax, float *doseAtCapture)
{
    if (!pressure || !qf || sliceJ != -1 || nCaptures < 1) { bfd_set_error("bfd_bhte_run_protocol: bad argument"); return -1; }
    return bhte_run_core<true, unsigned char>(device, N3, N2, N1, nMat, mat, cd, cp, qf, initT, nFields, nullptr, pressure, qOut, T, dose, flags, Tcore, dt, nSteps, fieldOfStep,
                               -1, nFactorMonitoring, nullptr, nPoints, pointIndex, points, kernelMs, nCaptures, captureStep, Tmax, doseAtCapture);
}

// The two calls above for material lists of more than 256 rows (a CT-derived list: up to 1030): 16-bit ids, nMat <= bfd_bhte_max_materials().
// Same arithmetic in the same order; a list that fits 8 bits gives the same bits through either entry.
extern "C" int bfd_bhte_max_materials(void) { return BFD_BHTE_MAX_MATERIALS; }
extern "C" int bfd_bhte_run_volumes16(int32_t device, int32_t N1, int32_t N2, int32_t N3, int32_t nMat, const uint16_t *mat,
                                      const float *cd, const float *cp, const float *qf, const float *initT, int32_t nFields,
                                      const float *pressure, float *qOut, float *T, float *dose, int32_t flags, float Tcore, double dt,
                                      int32_t nSteps, const int32_t *fieldOfStep, int32_t sliceJ, int32_t nFactorMonitoring,
                                      float *monitorSlice, int64_t nPoints, const uint32_t *pointIndex, float *points, double *kernelMs)
{
    if (!pressure || !qf) { bfd_set_error("bfd_bhte_run_volumes16: bad argument"); return -1; }
    return bhte_run_core<true, uint16_t>(device, N3, N2, N1, nMat, mat, cd, cp, qf, initT, nFields, nullptr, pressure, qOut, T, dose, flags, Tcore, dt, nSteps, fieldOfStep,
                                         sliceJ, nFactorMonitoring, monitorSlice, nPoints, pointIndex, points, kernelMs);
}
extern "C" int bfd_bhte_run_protocol16(int32_t device, int32_t N1, int32_t N2, int32_t N3, int32_t nMat, const uint16_t *mat,
                                       const float *cd, const float *cp, const float *qf, const float *initT, int32_t nFields,
                                       const float *pressure, float *qOut, float *T, float *dose, int32_t flags, float Tcore, double dt,
                                       int32_t nSteps, const int32_t *fieldOfStep, int32_t sliceJ, int32_t nFactorMonitoring,
                                       float *monitorSlice, int64_t nPoints, const uint32_t *pointIndex, float *points, double *kernelMs,
                                       int32_t nCaptures, const int32_t *captureStep, float *Tmax, float *doseAtCapture)
{
    if (!pressure || !qf || sliceJ != -1 || nCaptures < 1) { bfd_set_error("bfd_bhte_run_protocol16: bad argument"); return -1; }
    return bhte_run_core<true, uint16_t>(device, N3, N2, N1, nMat, mat, cd, cp, qf, initT, nFields, nullptr, pressure, qOut, T, dose, flags, Tcore, dt, nSteps, fieldOfStep,
                                         -1, nFactorMonitoring, nullptr, nPoints, pointIndex, points, kernelMs, nCaptures, captureStep, Tmax, doseAtCapture);
}

// One pressure field heating during the first nStepsOn steps (the reference's BHTE call).
extern "C" int bfd_bhte_run(int32_t device, int32_t N1, int32_t N2, int32_t N3, int32_t nMat, const unsigned char *mat,
                            const float *cd, const float *cp, const float *q, float *T, float *dose, float Tcore, double dt,
                            int32_t nSteps, int32_t nStepsOn, int32_t sliceJ, int32_t nFactorMonitoring, float *monitorSlice,
                            int64_t nPoints, const uint32_t *pointIndex, float *points, double *kernelMs)
{
    if (nSteps < 0) { bfd_set_error("bfd_bhte_run: bad argument"); return -1; }
    std::vector<int32_t> sched((size_t)nSteps + 1, -1);
    for (int s = 0; s < nSteps && s < nStepsOn; s++) sched[s] = 0;
    return bfd_bhte_run_fields(device, N1, N2, N3, nMat, mat, cd, cp, 1, q, T, dose, Tcore, dt, nSteps, sched.data(), sliceJ,
                               nFactorMonitoring, monitorSlice, nPoints, pointIndex, points, kernelMs);
}
