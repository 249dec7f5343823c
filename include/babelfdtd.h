/*
 * babelfdtd.h -- C ABI of the MI355X-native viscoelastic FDTD engine (libbabelfdtd_hip.so).
 *
 * This is the drop-in boundary for BabelBrain's Step-2 hot path. The reference reaches its
 * solver through two Python methods of a module-global object
 *     PModel = PropagationModel()                                   BabelIntegrationBASE.py:43
 *     PModel.CalculateMatricesForPropagation(...)                   BabelIntegrationBASE.py:1799,1801
 *     PModel.StaggeredFDTD_3D_with_relaxation(...)                  BabelIntegrationBASE.py:2338,2374,2401
 * whose implementation (package BabelViscoFDTD==1.2.4, environment_linux.yml:44) binds a
 * per-backend native module selected by the integer COMPUTING_BACKEND (BabelBrain.py:429-439,
 * SelFiles/SelFiles.py:245-262). The functions below are what such a backend module binds:
 * plain pointers and sizes, int return codes (0 = ok, <0 = error, text via bfd_last_error()),
 * no exceptions, no torch types. babelbrain_amd/PropagationModel.py is the ctypes binding.
 *
 * Conventions
 *  - Volumes handed in by the caller are described by a base pointer and three ELEMENT strides
 *    (s1,s2,s3) for the axes (i,j,k) of an (N1,N2,nk) view, so a C-order numpy array is passed
 *    without a host transpose: element (i,j,k) is base[i*s1 + j*s2 + k*s3]. The byte span
 *    base[0 .. (N1-1)*s1+(N2-1)*s2+(nk-1)*s3] must be readable/writable. Inputs are never modified.
 *  - On the device every volume is "x-fastest": linear index i + N1*(j + N2*k), the order the
 *    reference decodes IndexSensorMap with (BabelIntegrationBASE.py:2508-2511).
 *  - One bfd_sim owns the Z-slab [k0, k0+nk) of the global N1 x N2 x N3 domain (single GPU:
 *    k0=0, nk=N3). Slabs are advanced half-step by half-step; the two ghost planes on each side
 *    are exchanged by the caller between half-steps (bfd_halo_region gives device pointers), or
 *    are zero at the ends of the domain. A slab has at least 4 planes, the 2 + 2 its neighbours
 *    read: bfd_create refuses a thinner one, as bfd_group_create refuses a split that gives one.
 *  - Selectable maps are a bitmask of BFD_MAP_* (names follow the reference's SelMapsRMSPeakList /
 *    SelMapsSensorsList strings, BabelIntegrationBASE.py:1413-1417, 2355-2356).
 */
#ifndef BABELFDTD_H
#define BABELFDTD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BFD_ABI_VERSION 7

enum {
    BFD_MAP_VX = 0, BFD_MAP_VY = 1, BFD_MAP_VZ = 2,
    BFD_MAP_SIGMAXX = 3, BFD_MAP_SIGMAYY = 4, BFD_MAP_SIGMAZZ = 5,
    BFD_MAP_SIGMAXY = 6, BFD_MAP_SIGMAXZ = 7, BFD_MAP_SIGMAYZ = 8,
    BFD_MAP_PRESSURE = 9, BFD_MAP_ALLV = 10, BFD_MAP_COUNT = 11
};

/* which accumulated volume bfd_get_map returns */
enum { BFD_KIND_RMS = 0, BFD_KIND_PEAK = 1, BFD_KIND_LAST = 2 };

/* halo groups exchanged between Z-neighbours */
enum { BFD_HALO_VELOCITY = 0 /* Vx,Vy,Vz: before the stress half-step   */,
       BFD_HALO_STRESS = 1   /* Sxz,Syz,Szz: before the velocity half-step */ };

typedef struct bfd_sim bfd_sim;

typedef struct bfd_config {
    int32_t N1, N2, N3;        /* global domain, voxels, absorbing layer included (BASE:1876-1878) */
    int32_t k0, nk;            /* this slab owns global planes [k0, k0+nk)                        */
    int32_t nMat;              /* rows of MaterialList                                            */
    int32_t NDelta;            /* absorbing-layer thickness in cells (NDelta=12, BASE:2350)       */
    int32_t typeSource;        /* TypeSource: 0 add velocity, 1 set velocity, 2 add stress, 3 set stress (BASE:2327,2332,2393) */
    int32_t sensorSub;         /* SensorSubSampling (BASE:2363)                                   */
    int32_t sensorStart;       /* SensorStart, in sub-sampled steps (BASE:2109,2364)              */
    int32_t nt;                /* total number of time steps of the run (sizes the sensor block)  */
    int32_t selRMSorPeak;      /* SelRMSorPeak: 1 RMS, 2 peak, 3 both (BASE:2357)                 */
    uint32_t selMapsRMS;       /* SelMapsRMSPeakList as BFD_MAP_* bits (BASE:2355)                */
    uint32_t selMapsSensors;   /* SelMapsSensorsList as BFD_MAP_* bits (BASE:2356)                */
    int32_t qfactorCorrection; /* QfactorCorrection (BASE:2361)                                   */
    int32_t device;            /* HIP device ordinal                                              */
    int32_t kernelVariant;     /* 0 = default (= 3), 1 = simple one-thread-per-voxel kernels, 2 = LDS-tiled dense, 3 = LDS-tiled with fluid/solid tile classes, 4 = 3 + fused stress/velocity pass over eligible fluid tiles (whole domains only: keeps two copies of V, Szz, Rzz; on a Z-slab it is 3) */
    int32_t rmsFirstStep;      /* 0 = RMS/peak accumulation starts at step SensorStart*SensorSubSampling (the reference's last-cycles
                                * window, BASE:2108-2109); n > 0 = it starts at step n-1 (bench: every timed step accumulates) */
    int32_t sensorMode;        /* 0 = the sensor series are stored ([nSensors][nTs] per selected map, what the reference returns);
                                * 1 = only their single-frequency content is kept: re/im of the DFT bin nearest to `freq` and the peak
                                * are accumulated per sensor while the samples are taken (what CalculatePhaseData extracts from the
                                * series, BASE:2498-2520) -- 20 B per sensor instead of 4*nTs; bfd_get_sensors is then unavailable */
    double h;                  /* SpatialStep, m (BASE:2344)                                      */
    double dt;                 /* DT, s (BASE:2351)                                               */
    double freq;               /* Frequency, Hz (BASE:2341)                                       */
    double reflectionLimit;    /* ReflectionLimit (BASE:2352)                                     */
} bfd_config;

/* ---- library / device ---- */
int bfd_abi_version(void);
const char *bfd_last_error(void);
int bfd_device_count(void);                                   /* replaces <backend>.ListDevices, SelFiles.py:245-262 */
int bfd_device_name(int device, char *buf, int buflen);

/* ---- CalculateMatricesForPropagation (BASE:1799,1801): stable dt and per-material tables ----
 * matlist: nMat x 5 float64 rows [rho, cL, cS, alphaL, alphaS] (BASE:1712-1729); qcorr: nMat
 * float64 QCorrection factors or NULL (BASE:1290). tables7 (may be NULL) receives 7*nMat
 * float32: AP,BP,AS2,BS2,invMu,tauS,invRho for the given dt. */
double bfd_stable_dt(int32_t nMat, const double *matlist, const double *qcorr, double freq,
                     int32_t qfactorCorrection, double h, double alphaCFL);
int bfd_material_tables(int32_t nMat, const double *matlist, const double *qcorr, double freq,
                        int32_t qfactorCorrection, double h, double dt, float *tables7,
                        float *c1k2, double *cmax);

/* ---- StaggeredFDTD_3D_with_relaxation (BASE:2338-2365), decomposed ---- */
int bfd_create(const bfd_config *cfg, bfd_sim **out);
void bfd_destroy(bfd_sim *sim);

/* launch every kernel of this sim on an existing HIP stream (hipStream_t as void*), e.g. torch's
 * current stream, so the caller's halo exchange orders against it; NULL = the device's default
 * (null) stream. A new sim runs on a private non-blocking stream; bfd_use_private_stream returns to one. */
int bfd_set_stream(bfd_sim *sim, void *hipStream);
int bfd_use_private_stream(bfd_sim *sim);

/* MaterialList + QCorrection (BASE:2340,2362) */
int bfd_set_materials(bfd_sim *sim, const double *matlist, const double *qcorr);
/* Replacing inputs on a live sim. Every setter may be called again: after bfd_reset, and between two time steps of a run (from then on
 * the run uses the new input; sources index their table by the absolute step). Between time steps the material of a cell may change only
 * where the cell's 15 fields and those of its neighbours within 4 cells are all exactly zero (ahead of the wave front): such a cell does
 * not know its material, and the run equals one that had the new map from step 0. What becomes of non-zero stresses in a cell whose
 * material changes is undefined (a solid cell that turns fluid loses its shear stresses and memory variables). The same holds for the
 * cells a reflector mask adds or releases. */
/* MaterialMap slab (BASE:2339). ghostLow/ghostHigh (0..2): planes readable below k=0 / above
 * k=nk-1 of the view (neighbour slab's cells); missing ghost planes replicate the edge plane.
 * A new map CLEARS THE REFLECTOR: the mask lives in the ids this call rewrites, so bfd_set_reflector must be called again after it. */
int bfd_set_material_map(bfd_sim *sim, const uint32_t *map, int64_t s1, int64_t s2, int64_t s3,
                         int32_t ghostLow, int32_t ghostHigh);
/* ReflectorMask slab (BASE:2365); NULL clears it. A mask REPLACES the previous one (it is not added to it). Set it after the material map. */
int bfd_set_reflector(bfd_sim *sim, const uint32_t *mask, int64_t s1, int64_t s2, int64_t s3);
/* SourceMap/PulseSource/Ox,Oy,Oz (BASE:2342-2349) in compact form: nVox source voxels of this
 * slab, local x-fastest linear index, 0-based PulseSource row, per-voxel weights (NULL = 1),
 * pulse = [nSources][lengthSource] float64 exactly as the caller built it (Single:335-346).
 * A table whose float32 form exceeds 1 GiB (238 k sources x 6.8 k steps at 512^3: 6.4 GB; 1 M x 7 k at 1024^3: 28 GB) is
 * STREAMED: it stays in the caller's memory -- which must then remain valid and unchanged until the last time step has
 * been issued, as it does inside the solver call -- and reaches the device in double-buffered time tiles of 64 steps
 * (float64 -> float32 by a host packer that runs beside the GPU); the device holds 2 tiles instead of 12 bytes per
 * table entry. Smaller tables are converted once and kept resident. Results are identical either way. */
int bfd_set_sources(bfd_sim *sim, int64_t nVox, const uint32_t *localIndex, const uint32_t *row,
                    const float *wx, const float *wy, const float *wz,
                    const double *pulse, int32_t nSources, int32_t lengthSource);
/* The same sources with a separable (low-rank) table instead of the dense one (ABI 7, additive): row r at step n is
 *   acc = weights[r*K + 0] * signals[0*lengthSource + n]; acc = acc + weights[r*K + 1] * signals[1*lengthSource + n]; ...
 * in float32, in this order, without FMA contraction and with float32 denormals flushed -- bit for bit what the dense path
 * computes from the float64 table of those float32 values. weights = [nSources][K], signals = [K][lengthSource], 1 <= K <= 4.
 * A CW transducer row |u| sin(2 pi f t + arg u) ramp(t) has K = 2 (weights |u| cos arg u, |u| sin arg u; signals
 * sin(2 pi f t) ramp(t), cos(2 pi f t) ramp(t)). Both arrays are copied to the device (nSources*K + lengthSource*K floats):
 * nothing is streamed and the caller's arrays may go at once. Setting either form of source releases the other. */
int bfd_set_sources_separable(bfd_sim *sim, int64_t nVox, const uint32_t *localIndex, const uint32_t *row,
                              const float *wx, const float *wy, const float *wz,
                              int32_t nSources, int32_t K, const float *weights, int32_t lengthSource, const float *signals);
/* SensorMap slab (BASE:2346); returns the number of sensors of this slab in *nSensors */
int bfd_set_sensor_map(bfd_sim *sim, const uint32_t *map, int64_t s1, int64_t s2, int64_t s3,
                       int64_t *nSensors);
/* The three setters above for callers whose volumes are on the device already (ABI 7, additive).
 * bfd_set_material_map_device / bfd_set_reflector_device: the same view (element strides >= 0, ghost planes), the same meaning, return codes
 * (-2 ghost counts or strides, -6 mid-step or no map yet, -5 an id >= nMat) and side effects as the host forms (a new map clears the reflector;
 * the run lists are rebuilt), but devMap / devMask is DEVICE memory of the sim's own device: the layout kernel reads it in place, no temporary
 * is allocated and nothing is copied. The pointer is looked up first (hipPointerGetAttributes, hipMemGetAddressRange): a host pointer, managed
 * memory, memory of another device, or a view that does not lie inside one allocation is refused with -1 and the sim is unchanged. The work that
 * wrote the volume must have finished: the sim's stream waits for no other stream. The call returns when the kernel has read the volume.
 * devMask = NULL clears the reflector, as in the host form. */
int bfd_set_material_map_device(bfd_sim *sim, const uint32_t *devMap, int64_t s1, int64_t s2, int64_t s3,
                                int32_t ghostLow, int32_t ghostHigh);
int bfd_set_reflector_device(bfd_sim *sim, const uint32_t *devMask, int64_t s1, int64_t s2, int64_t s3);
/* The sensors of a dense box of voxels without a volume: voxels lo[a] <= index < lo[a] + size[a] of the slab's (N1, N2, nk) volume (k local to
 * the slab). The index list is written on the device in ascending x-fastest order; afterwards the sim is in the state bfd_set_sensor_map reaches
 * from a volume that is 1 inside the box and 0 outside: same count, same bfd_get_sensor_index, same DFT bin, series block or DFT sums, and
 * the captures take the box form (BFD_SENSOR_BOX=0 keeps the list form, as there). -1: sim, lo or size NULL, an empty box (a size <= 0), a box
 * that leaves the slab; nothing is changed then. nSensors may be NULL. */
int bfd_set_sensor_box(bfd_sim *sim, const int32_t *lo /*[3]*/, const int32_t *size /*[3]*/, int64_t *nSensors);

/* time stepping. bfd_run = nSteps x (stress half-step, velocity half-step, accumulate, sensors)
 * for a slab without neighbours. With neighbours the caller alternates:
 *   exchange VELOCITY halos -> bfd_half_step_stress -> exchange STRESS halos -> bfd_half_step_velocity */
int bfd_run(bfd_sim *sim, int32_t nSteps);
int bfd_half_step_stress(bfd_sim *sim);
int bfd_half_step_velocity(bfd_sim *sim);   /* also accumulates, records sensors, advances the step counter */
/* the same half-steps in two parts, so a halo exchange can overlap the bulk of the work:
 * part 1 = the tiles of the first and last z-chunk (8-32 planes) of the slab (everything a Z-neighbour reads),
 * part 2 = all other tiles plus the end-of-step work; part 0 = both (the calls above). Per half-step call
 * part 1 then part 2. (kernelVariant 1: part 1 is empty.) */
int bfd_half_step_stress_part(bfd_sim *sim, int32_t part);
int bfd_half_step_velocity_part(bfd_sim *sim, int32_t part);
/* The same launched on a stream of the caller (NULL = the default stream) without any synchronisation: the boundary part
 * can run on a side stream that a halo exchange waits on while the interior part keeps the main stream busy. The caller
 * orders the two streams (events); parts of one half-step are independent of each other, the end-of-step work of
 * velocity part 2 (sensors, non-Pressure accumulators) reads the whole slab. */
int bfd_half_step_stress_part_on(bfd_sim *sim, int32_t part, void *hipStream);
int bfd_half_step_velocity_part_on(bfd_sim *sim, int32_t part, void *hipStream);
int bfd_sync(bfd_sim *sim);
int bfd_current_step(bfd_sim *sim);
/* Everything the first step would otherwise do on entry: per-cell classes, run lists, and the placement of the per-voxel
 * arrays: streams that advance together are 12 % slower when all of them lie in one of the three physical regions of the
 * HBM than when they are spread over two, so a pair probe on the (all-zero) initial state finds the
 * region of every array relative to Vx and the arrays a kernel reads together are made to alternate -- by exchanging
 * buffers, and with fresh allocations where one side is short. BFD_PLACEMENT=0 switches it off. Results do not depend on
 * it. bfd_run and the half-step calls do this by themselves at step 0; call it explicitly BEFORE bfd_halo_region when halo
 * pointers are taken ahead of the first step (pointers handed out pin the arrays). */
int bfd_prepare(bfd_sim *sim);
/* one line on what the placement found and did (valid until the sim is destroyed) */
const char *bfd_placement_note(bfd_sim *sim);
/* Placement policy, before the first step / bfd_prepare. mode 0 = leave the arrays where hipMalloc put them. searchLimitBytes =
 * how much throw-away device memory the search for a buffer in another region may hold at a time (all of it is released
 * before bfd_prepare returns); < 0 = the default rule: nothing at all when the device carries other allocations than this
 * engine's (another process, the other slabs of a group): the engine's own buffers are then only exchanged among themselves;
 * on a device the engine has to itself up to 192 GiB, at most two thirds of what was free on entry and always leaving 48 GiB of it
 * untouched; the search ends at once when allocations that are neither the engine's nor its own appear on the device while it walks, and
 * after 2 s (BABELFDTD_PLACEMENT_SEARCH_SECONDS): the placement is worth a few per cent of one call's run time.
 * bfd_prepare never fails for lack of memory where mode 0 succeeds. */
int bfd_set_placement(bfd_sim *sim, int32_t mode, int64_t searchLimitBytes);
/* The default rule can be moved without code by whoever owns the device: BABELFDTD_PLACEMENT_SEARCH_GIB=<GiB> replaces the 192 GiB
 * (the shared-device rule stays). Buffers a search found in another region are kept when their engine is destroyed and
 * offered to the next engine of this process with arrays of the same size on the same device, so that the two or three solver calls of
 * one RUN_SIMULATION (BabelIntegrationBASE.py:2338, 2374, 2401) pay the search once; at most BABELFDTD_PLACEMENT_CACHE_GIB (default
 * 48, never more than an eighth of the device's memory, 0 = keep nothing) are held between engines; bfd_create evicts buffers of another
 * array size, and any allocation of the library that runs out of memory frees the cache and tries once more.
 * bfd_placement_cache_release frees them now and returns the bytes freed (the Python drop-in calls it when a solver call returns,
 * unless it was built with keepPlacementCache=True / BABELFDTD_PLACEMENT_CACHE_KEEP=1). It also gives back the pinned host pieces
 * (16 MB each, at most 32) the result readbacks keep between them; those are not part of the count. */
int64_t bfd_placement_cache_release(void);

/* device pointer/bytes of a halo region: field f (0..2 within the group), side 0 = low-k face,
 * 1 = high-k face; send = 1: the 2 owned boundary planes, send = 0: the 2 ghost planes.
 * Each region is 2*N1*N2 contiguous float32. */
int bfd_halo_region(bfd_sim *sim, int32_t group, int32_t f, int32_t side, int32_t send,
                    void **devPtr, size_t *bytes);

/* which fields of a halo group this slab READS from its Z-neighbours' planes, as a bit mask (bit f = field f of
 * bfd_halo_region): 7 in general; 4 (Vz / Szz only) for a slab without solid runs under the tiled kernels, whose
 * stencils cross a Z face through those two fields alone. Across an interface each side sends what the other reads. */
int bfd_halo_fields(bfd_sim *sim, int32_t group, uint32_t *mask);

/* timing of the step loop, device time from HIP events on the sim's stream */
int bfd_timing_begin(bfd_sim *sim, int32_t perKernel);
int bfd_timing_end(bfd_sim *sim, double *totalMs, double *stressMs, double *velocityMs,
                   double *otherMs, int64_t *nStressLaunches, int64_t *nVelocityLaunches);

/* Finer timing (bfd_timing_begin(sim, 2)): device ms and launch count per kernel class over the timed window, classes
 * 0 stress fluid tiles, 1 normal stresses of solid tiles, 2 sparse shear stresses, 3 velocity fluid tiles,
 * 4 velocity solid tiles, 5 fused fluid time step. Call after bfd_timing_end. Arrays of 6. */
int bfd_timing_kernels(bfd_sim *sim, double *msPerClass, int64_t *launchesPerClass);
/* ALGORITHMIC bytes one launch of each kernel class has to move (same class order), from the tile-class counts: every
 * field value of the class's per-cell byte table fetched / stored exactly once (float32 4 B, material id 2 B; absorbing-
 * layer memory variables, coefficient tables and halo re-reads excluded). accumulating != 0 adds the
 * Pressure RMS accumulator (8 B per cell outside the absorbing layer) to the velocity classes; where the accumulation of the
 * fluid runs is paired (bfd_paired_launches) it is 4 B per launch of the fluid stress class instead: the average over a step
 * pair. Where Vz is advanced (below) the fluid stress class moves 4 B more and the fluid velocity class 8 B less per advanced
 * cell, with or without accumulation. DESIGN.md section 6. */
int bfd_algorithmic_bytes(bfd_sim *sim, int32_t accumulating, double *bytesPerClass);
/* Paired Pressure accumulation (all-fluid runs, velocity-type sources, rmsFirstStep >= 1 or quiet runs off): accumulating steps go in
 * pairs, the stress half-step of the second adds the Pressure of both to the RMS / peak maps; bfd_get_map, bfd_reset and the
 * setters settle an open pair first, so results equal accumulating in every step bit for bit. BFD_PAIR_ACC=0 switches it off.
 * Between the two half-steps of a time step the RMS / peak maps of the fluid runs may already hold that step (second step of a pair;
 * otherwise they hold the steps before it, as without pairing); after bfd_half_step_velocity they are the same either way.
 * Returns the number of launches of the pairing stress flavour so far (0: every step accumulated in the velocity kernels). */
int64_t bfd_paired_launches(bfd_sim *sim);
/* Advanced Vz (no entry point of its own): in an engine of the class-specialised kernels (variants 0 / 3, in-place update) with velocity-type
 * sources, no solid run and no quiet runs (rmsFirstStep >= 1 or BFD_SKIP_ZERO=0), the stress half-step also stores the new Vz of the inner planes
 * of every fluid run outside the absorbing layer and the velocity half-step leaves Vz alone there; results are bit-identical, BFD_ADV_VZ=0
 * switches it off. The two half-steps of a time step are then one unit: between them bfd_set_materials, bfd_set_material_map,
 * bfd_set_reflector, bfd_set_sources and bfd_set_sources_separable return -6 ("finish the time step first") and change nothing;
 * bfd_set_sensor_map and the getters stay available (see bfd_get_field for "Vz"). */
/* back to step 0: fields, absorbing-layer memory, accumulators and the sensor block zeroed; inputs are kept */
int bfd_reset(bfd_sim *sim);

/* results */
int64_t bfd_num_sensors(bfd_sim *sim);
int32_t bfd_num_sensor_steps(bfd_sim *sim);
/* 1-based GLOBAL x-fastest linear index of every sensor of this slab, ascending (BASE:2369,2503) */
int bfd_get_sensor_index(bfd_sim *sim, uint32_t *index);
/* out[nSelSensors][nSensors][nTs] float32, maps in ascending BFD_MAP_* order (BASE:2507: FFT along axis 1). Blocks of 256 MB and
 * more (this one, the maps below) are carried by four host threads of the library through pinned pieces (BFD_D2H_THREADS; the
 * call returns when all of it has arrived); the destination is advised to use huge pages. */
int bfd_get_sensors(bfd_sim *sim, float *out);
/* Single-frequency content of the recorded sensor series, computed on the device: replaces the host
 * FFT + bin pick of CalculatePhaseData (BASE:2498-2520) without moving the (nSensor x nTs) block.
 *   F[q][s] = (2/nTs) sum_n x[q][s][n] exp(-2 pi i bin n / nTs),  bin = argmin |fftfreq(nTs, DT*SensorSubSampling) - freq|
 *   peak[q][s] = max_n x[q][s][n]                                                   (BASE:2518)
 * outReIm: [nSelSensors][nSensors][2] float32, outPeak (may be NULL): [nSelSensors][nSensors].
 * With sensorMode 1 the values come from the in-loop accumulators (same arithmetic, sample by sample; freq must be the
 * sim's own frequency). */
int bfd_get_sensor_dft(bfd_sim *sim, double freq, float *outReIm, float *outPeak);
/* the same transform for a host series [nSensors][nTs] (row-major), sampling period dtSensor */
int bfd_dft_series(int32_t device, int64_t nSensors, int32_t nTs, const float *series, double dtSensor, double freq,
                   float *outReIm, float *outPeak);

/* Result packing (ABI 7, additive): the Pressure results of a run with sensorMode 1 as the volumes the caller saves, formed on the device --
 * what CalculatePhaseData's scatter (BASE:2503-2520), the dispersion scaling (BASE:2433-2456) and ReturnResults' zero / crop / paste / flip
 * (BASE:2729-2885) make of them on the host. Coordinates are voxels of the slab's (N1, N2, nk) volume, k local to the slab.
 *   kept region: lo[a] <= index < dim[a] - hi[a] (the Crop offsets; hi counts planes dropped at the high end)
 *   output: numpy C order [O[0]][O[1]][O[2]]; the kept region lands at offset at[a], the rest is 0; with flipK = 1 the output is then
 *           reversed along its last axis. O = kept size and at = 0 gives DataForSim; O = the mask's shape and at = the shrinks gives
 *           paste_and_flip.
 *   zero where the voxel's global k <= zSource, and (pComplex, pPeak) where the voxel is not a sensor.
 *   applyScale = 0: no scaling at all. applyScale = 1, per voxel:
 *     pAmp     = (float)((double)rms * ampScale), rms = the Pressure RMS map as bfd_get_map gives it; ampScale = Correction * sqrt(2) in float64
 *     pComplex = re, im of bfd_get_sensor_dft, each times (float)correction in float32
 *     pPeak    = the peak of bfd_get_sensor_dft times (float)correction in float32
 *   (denormal operands and products are kept, as numpy on a CPU keeps them: these products are the one place where the library does not flush.)
 * Each output may be NULL. pAmp needs the Pressure RMS map selected, pComplex / pPeak need sensorMode 1 with Pressure among the sensor maps
 * (-2 otherwise). A sensor set that is a dense box (bfd_set_sensor_box, or a map recognised as one) is packed by index arithmetic; any other
 * list by one zero fill and one lane per sensor; same values, no atomics, the same bytes in every run.
 * -1, before the device is touched and in this order: sim or spec NULL; flipK or applyScale not 0 / 1; a scale that is not finite (with
 * applyScale); lo or hi negative or an empty kept region; O not positive or beyond 2^31 - 1 voxels; at negative or the kept region not inside O.
 * kernelMs (may be NULL): the kernels alone. */
typedef struct bfd_pack_spec {
    int32_t lo[3], hi[3];
    int32_t zSource;
    int32_t O[3], at[3];
    int32_t flipK, applyScale;
    double ampScale, correction;
} bfd_pack_spec;
int bfd_pack_results(bfd_sim *sim, const bfd_pack_spec *spec, float *pAmp, float *pComplex /*[..][2]*/, float *pPeak, float *kernelMs);
/* one accumulated volume of this slab into a strided (N1,N2,nk) float32 view */
int bfd_get_map(bfd_sim *sim, int32_t kind, int32_t map, float *out, int64_t s1, int64_t s2, int64_t s3);
/* raw state array a (0..14: Vx Vy Vz Sxx Syy Szz Sxy Sxz Syz Rxx Ryy Rzz Rxy Rxz Ryz), for tests.
 * Between bfd_half_step_stress* and the matching velocity half-step, "Vz" (a = 2) is of mixed time level where Vz is advanced (below):
 * the inner planes of the advancing runs hold the new Vz already, every other cell the old one; after the velocity half-step it is the new Vz everywhere. */
int bfd_get_field(bfd_sim *sim, int32_t a, float *out, int64_t s1, int64_t s2, int64_t s3);
/* number of 64x8x8-voxel sub-tiles per class of the class-specialised kernels (variant 0/3):
 * lossless fluid, lossy fluid, solid, and among the fluid ones how many hold one material only (UNI)
 * and how many touch the absorbing layer (PML) (DESIGN.md "Tile classes"); zeros for variants 1, 2 */
int bfd_tile_counts(bfd_sim *sim, int32_t *nLossless, int32_t *nLossy, int32_t *nSolid, int32_t *nUni, int32_t *nPml);
/* fluid sub-tiles that keep a single copy of their three identical normal stresses: all of them in an all-fluid
 * slab, those without a solid sub-tile beside them in x or y otherwise; 0 when a Sigma** output is selected */
int bfd_tile_count_lean(bfd_sim *sim, int32_t *nLean);
/* fluid sub-tiles advanced by the fused time-step kernel (kernelVariant 4 on a whole domain; 0 otherwise) */
int bfd_tile_count_fused(bfd_sim *sim, int32_t *nFused);
/* Quiet runs (ABI 7). A production call of a whole domain -- the caller's own accumulation window (rmsFirstStep = 0), class-specialised
 * kernels, solid-only values compact; BFD_SKIP_ZERO=0 switches it off -- keeps one activity byte per 64x8x8-voxel sub-tile: set once a kernel
 * has written a non-zero velocity or stress there (the sub-tiles of the source voxels from the start). Ahead of the wave front every field
 * is exactly zero (float32, denormals flushed), and a tile run whose sub-tiles and all their neighbours are clear returns at entry: results
 * are bit-identical, the steps before the front has crossed the domain cost less (the time plan BabelIntegrationBASE.py:2082-2109 gives a
 * call about 1.8 transits of the domain's diagonal). *active = sub-tiles marked so far, *total = sub-tiles of the domain; both 0 when the
 * engine runs every tile in every half-step (Z-slabs, bench.py's timed windows, the other kernel variants). */
int bfd_activity_counts(bfd_sim *sim, int64_t *active, int64_t *total);
/* device memory this sim holds, bytes */
int64_t bfd_device_bytes(bfd_sim *sim);

/* ---- One solver call on several devices of THIS process: Z-slab decomposition behind the drop-in ----
 * The reference's caller is one process making one call (Babel_SingleTx.py:258 spawns a single Process;
 * BabelIntegrationBASE.py:2338-2365 calls PModel.StaggeredFDTD_3D_with_relaxation once, device chosen by
 * DefaultGPUDeviceName :2358). A group owns one slab engine per entry of `devices` (slab r = balanced r-th share of the
 * N3 planes, on HIP device devices[r]; an ordinal may repeat), takes the WHOLE-domain inputs exactly as bfd_set_* take a
 * slab's, runs the step loop in C and moves the 2+2 halo planes per half-step and interface with peer copies ordered by
 * events (hipMemcpyPeerAsync; boundary runs first, interior beside the copies). No second process, no collective.
 * cfg: k0 = 0, nk = N3; cfg->device is ignored. Results equal the single-device run bit for bit. */
typedef struct bfd_group bfd_group;
int bfd_group_create(const bfd_config *cfg, int32_t nSlabs, const int32_t *devices, bfd_group **out);
void bfd_group_destroy(bfd_group *g);
int32_t bfd_group_size(bfd_group *g);
/* slab r: its planes [k0, k0+nk), device and engine (for the per-slab queries above: tile counts, timing, fields) */
int bfd_group_slab(bfd_group *g, int32_t r, int32_t *k0, int32_t *nk, int32_t *device, bfd_sim **sim);
int bfd_group_set_materials(bfd_group *g, const double *matlist, const double *qcorr);
/* whole-domain (N1,N2,N3) views with element strides, as bfd_set_material_map / _reflector / _sensor_map */
int bfd_group_set_material_map(bfd_group *g, const uint32_t *map, int64_t s1, int64_t s2, int64_t s3);
int bfd_group_set_reflector(bfd_group *g, const uint32_t *mask, int64_t s1, int64_t s2, int64_t s3);
/* as bfd_set_sources with GLOBAL x-fastest voxel indices i + N1*(j + N2*k); the pulse table is shared by the slabs */
int bfd_group_set_sources(bfd_group *g, int64_t nVox, const int64_t *globalIndex, const uint32_t *row,
                          const float *wx, const float *wy, const float *wz,
                          const double *pulse, int32_t nSources, int32_t lengthSource);
/* as bfd_set_sources_separable with GLOBAL voxel indices; every slab holds the whole weights and signals */
int bfd_group_set_sources_separable(bfd_group *g, int64_t nVox, const int64_t *globalIndex, const uint32_t *row,
                                    const float *wx, const float *wy, const float *wz,
                                    int32_t nSources, int32_t K, const float *weights, int32_t lengthSource, const float *signals);
int bfd_group_set_sensor_map(bfd_group *g, const uint32_t *map, int64_t s1, int64_t s2, int64_t s3, int64_t *nSensors);
int bfd_group_set_placement(bfd_group *g, int32_t mode, int64_t searchLimitBytes);   /* bfd_set_placement of every slab */
int bfd_group_prepare(bfd_group *g);                     /* bfd_prepare of every slab + the halo plan; bfd_group_run does it by itself */
int bfd_group_run(bfd_group *g, int32_t nSteps);         /* queues nSteps time steps on every slab; returns without waiting */
int bfd_group_sync(bfd_group *g);
int bfd_group_reset(bfd_group *g);
/* wall time of the window, the largest device time of a slab (HIP events on its main stream), the host time spent
 * queueing work inside bfd_group_run (exposed launch overhead when it approaches the wall time), halo bytes moved per
 * time step over all interfaces, and whether the overlapped order was used (slabs of >= 64 planes) */
int bfd_group_timing_begin(bfd_group *g);
int bfd_group_timing_end(bfd_group *g, double *wallMs, double *maxDeviceMs, double *hostIssueMs, double *haloBytesPerStep,
                         int32_t *overlapped);
/* How the halo planes travel across each interface (slab r | slab r+1), decided in bfd_group_create -- the reference has no counterpart
 * (one device per call, BabelIntegrationBASE.py:2358); here a silently missing peer path (IOMMU, HIP_VISIBLE_DEVICES, topology) would
 * only show as a bad scaling curve. status[r] & 15 = BFD_PEER_SAME_DEVICE (both slabs on one device: a device copy), BFD_PEER_DIRECT
 * (peer access enabled both ways: hipMemcpyPeerAsync moves the planes device to device) or BFD_PEER_STAGED (not available in at least
 * one direction: the runtime stages the copies through the host). Detail bits: 16 / 32 = can access / enabled from slab r's device to
 * slab r+1's, 64 / 128 = the other way. Returns the number of interfaces (nSlabs - 1); status needs room for that many. */
#define BFD_PEER_SAME_DEVICE 0
#define BFD_PEER_DIRECT 1
#define BFD_PEER_STAGED 2
int bfd_group_peer_status(bfd_group *g, int32_t *status, int32_t n);
/* results over the whole domain: sensors of all slabs in ascending GLOBAL index (BASE:2369, 2503), volumes into a
 * strided (N1,N2,N3) view */
int64_t bfd_group_num_sensors(bfd_group *g);
int32_t bfd_group_num_sensor_steps(bfd_group *g);
int bfd_group_get_sensor_index(bfd_group *g, uint32_t *index);
int bfd_group_get_sensors(bfd_group *g, float *out);                  /* [nSelSensors][nSensors][nTs] */
int bfd_group_get_sensor_dft(bfd_group *g, double freq, float *outReIm, float *outPeak);
int bfd_group_get_map(bfd_group *g, int32_t kind, int32_t map, float *out, int64_t s1, int64_t s2, int64_t s3);
int64_t bfd_group_device_bytes(bfd_group *g);

/* ---- Rayleigh-Sommerfeld integral: replaces BabelViscoFDTD.tools.RayleighAndBHTE.ForwardSimple ----
 * (call sites BabelIntegrationSingle.py:295, BabelIntegrationANNULAR_ARRAY.py:383,411,
 * BabelIntegrationCONCAVE_PHASEDARRAY.py:307,328,425,446).
 *   out[n] = (i k / 2pi) sum_m u0[m] ds[m] exp(-i k R_nm) / R_nm,  k = kReal + i kImag
 * center: nSrc x 3 float32 (m), ds: nSrc float32 (m^2), u0: nSrc x 2 float32 (re,im),
 * rf: nPts x 3 float32 (m), out: nPts x 2 float32 (re,im). kernelMs (may be NULL): device time. */
int bfd_rayleigh_forward(int32_t device, int64_t nSrc, const float *center, const float *ds, const float *u0,
                         double kReal, double kImag, int64_t nPts, const float *rf, float *out, double *kernelMs);

/* ---- The same integral resolved by transducer element: many steerings, or every element's own field, in one pass ----
 * Replaces the repeated ForwardSimple calls of the phased-array drivers over one geometry:
 *   per steering: BabelIntegrationCONCAVE_PHASEDARRAY.py:91-107 (each MultiPoint entry calls ForwardSimple at :328 and, refocused,
 *   at :446, and once more for the water-only pass; H317, I12378, ATAC, R15148, R15646, IGT64_500, H301, DomeTx and REMOPD reach
 *   it through CalculateFieldProcess.py:75-120) -- between those calls only exp(i phi_e) per element changes (:308-314);
 *   per element: BabelIntegrationH246.py:333-339, BabelIntegrationANNULAR_ARRAY.py:379-384, TxCalibration.py:323-328, 1021-1026
 *   (one ForwardSimple call per element on that element's sub-sources).
 * The records of element e are elemStart[e] .. elemStart[e+1]-1 (nBase += elemdims in the reference).
 *   G[e][n]   = (i k / 2pi) sum_{m in e} sub[m] ds[m] exp(-i k R_nm) / R_nm,  k = kReal + i kImag
 *   out[s][n] = sum_e weights[e][s] G[e][n]
 * sub: nSrc x 2 float32 (re,im) per-sub-source factor (AdjustWeightAmplitudes / OptimizedWeights, BabelIntegrationBASE.py:2224-2234),
 * NULL = 1. elemStart: nElem + 1 values, elemStart[0] = 0, elemStart[nElem] = nSrc, non-decreasing; an empty element contributes
 * nothing. weights: [nElem][nSteer][2] float32; out: [nSteer][nPts][2]. Any nSteer >= 1: geometry and points go up once, the
 * columns run 8 to a launch, kernelMs (may be NULL) is the device time of all launches.
 * Element mode, weights = NULL and nSteer = 0: out is G itself, [nElem][nPts][2] (zeros for an empty element).
 * A column's value depends only on the records, that column of the weights, k and the point -- not on nSteer, the column's
 * position, nPts or the point's position.
 * Device memory held during the call: 24 nSrc + 8 (nElem + 1) + 64 nElem ceil(nSteer / 8) + 12 nPts + 8 nPts nSteer bytes
 * (element mode: 8 nPts nElem for the result). Returns 0; -1 bad argument, -3 no such device, -10 device error (a failed
 * allocation included); bfd_last_error() has the text. nPts = 0 returns 0. */
int bfd_rayleigh_forward_elements(int32_t device, int64_t nSrc, const float *center, const float *ds, const float *sub,
                                  int32_t nElem, const int64_t *elemStart, int32_t nSteer, const float *weights,
                                  double kReal, double kImag, int64_t nPts, const float *rf, float *out, double *kernelMs);

/* ---- Pennes bio-heat equation + CEM43 dose: replaces BabelViscoFDTD.tools.RayleighAndBHTE.BHTE ----
 * (call sites ThermalModeling/CalculateTemperatureEffects.py:365-456, 960). Volumes x-fastest float32, mat = uint8
 * ids into cd/cp (per material: dt k/(rho c dx^2) and dt rho_b c_b w/(6e7 c)); q = temperature increment of one ON
 * step; T and dose are updated in place; faces of the volume keep their temperature. monitorSlice (may be NULL):
 * [N1][N3][ceil(nSteps/nFactorMonitoring)] of plane j = sliceJ; points (may be NULL): [nPoints][nSteps]. */
int bfd_bhte_run(int32_t device, int32_t N1, int32_t N2, int32_t N3, int32_t nMat, const unsigned char *mat,
                 const float *cd, const float *cp, const float *q, float *T, float *dose, float Tcore, double dt,
                 int32_t nSteps, int32_t nStepsOn, int32_t sliceJ, int32_t nFactorMonitoring, float *monitorSlice,
                 int64_t nPoints, const uint32_t *pointIndex, float *points, double *kernelMs);

/* Several pressure fields heating in turn: replaces BabelViscoFDTD.tools.RayleighAndBHTE.BHTEMultiplePressureFields
 * (call sites ThermalModeling/CalculateTemperatureEffects.py:381, 978; schedule built at :715-736). q holds nFields
 * volumes back to back; fieldOfStep[s] in [-1, nFields) names the field that heats during step s (-1 = none). */
int bfd_bhte_run_fields(int32_t device, int32_t N1, int32_t N2, int32_t N3, int32_t nMat, const unsigned char *mat,
                        const float *cd, const float *cp, int32_t nFields, const float *q, float *T, float *dose,
                        float Tcore, double dt, int32_t nSteps, const int32_t *fieldOfStep, int32_t sliceJ,
                        int32_t nFactorMonitoring, float *monitorSlice, int64_t nPoints, const uint32_t *pointIndex,
                        float *points, double *kernelMs);

/* The same run on volumes in the CALLER'S numpy C order, [N1][N2][N3] with the LAST axis fastest (what BHTE() receives at
 * CalculateTemperatureEffects.py:960: no host transposes), and with the heat source computed on the device from the
 * pressure amplitude(s): q = (p p) qf[material], float32; `pressure` holds nFields volumes (Pa), qOut (may be NULL) receives
 * q (the reference returns it as Qarr). The six neighbours are summed axis 0 first. flags bit 0: T holds the initial
 * temperature (else T starts from initT[material] and is output only); bit 1: dose holds the initial dose (else zero).
 * monitorSlice (may be NULL): [N1][N3][ceil(nSteps/nFactorMonitoring)] = T[:, sliceJ, :]; pointIndex: C-order linear
 * indices (i N2 + j) N3 + k. Steps are taken two per launch (one kernel pass moves the 21 B per voxel of a step once for
 * both); the monitors of the intermediate step are computed at the monitored voxels. */
int bfd_bhte_run_volumes(int32_t device, int32_t N1, int32_t N2, int32_t N3, int32_t nMat, const unsigned char *mat,
                         const float *cd, const float *cp, const float *qf, const float *initT, int32_t nFields,
                         const float *pressure, float *qOut, float *T, float *dose, int32_t flags, float Tcore, double dt,
                         int32_t nSteps, const int32_t *fieldOfStep, int32_t sliceJ, int32_t nFactorMonitoring,
                         float *monitorSlice, int64_t nPoints, const uint32_t *pointIndex, float *points, double *kernelMs);

/* A whole repeated-sonication protocol in one call: replaces the caller's RunBHTECycles loop
 * (ThermalModeling/CalculateTemperatureEffects.py:259-460), which makes one BHTE call per ON period, one per OFF period and one
 * per group pause and moves T and the dose through the host between them. Arguments as bfd_bhte_run_volumes, with fieldOfStep
 * covering the whole protocol back to back and points [nPoints][nSteps] over all of it; sliceJ must be -1 (no monitored plane)
 * and monitorSlice is ignored. captureStep: nCaptures >= 1 ascending step boundaries in [0, nSteps] (boundary c = after step
 * c - 1, the end of an ON call): there Tmax = max(Tmax, T) (the first capture copies T) and doseAtCapture = dose. Tmax and
 * doseAtCapture are [N1][N2][N3] outputs. No multi-step pass crosses a capture, so every output equals what the chain of
 * bfd_bhte_run_volumes calls gives. */
int bfd_bhte_run_protocol(int32_t device, int32_t N1, int32_t N2, int32_t N3, int32_t nMat, const unsigned char *mat,
                          const float *cd, const float *cp, const float *qf, const float *initT, int32_t nFields,
                          const float *pressure, float *qOut, float *T, float *dose, int32_t flags, float Tcore, double dt,
                          int32_t nSteps, const int32_t *fieldOfStep, int32_t sliceJ, int32_t nFactorMonitoring,
                          float *monitorSlice, int64_t nPoints, const uint32_t *pointIndex, float *points, double *kernelMs,
                          int32_t nCaptures, const int32_t *captureStep, float *Tmax, float *doseAtCapture);

/* Material lists of more than 256 rows. A CT-derived plan quantises bone HU to 2^10 bins behind 3 or 6 soft tissues
 * (BabelDatasetPreps.py:1019-1037, BabelIntegrationBASE.py:1242-1244): MaterialMapCT indexes up to 1030 rows, one thermal row per
 * bin (CalculateTemperatureEffects.py:804-841). bfd_bhte_run_volumes16 / bfd_bhte_run_protocol16 are bfd_bhte_run_volumes /
 * bfd_bhte_run_protocol with 16-bit ids: mat = uint16 ids into cd / cp / qf / initT, 1 <= nMat <= bfd_bhte_max_materials()
 * (1536, the coefficient table the multi-step kernels keep in LDS; more gives -1 and an error text that names the limit);
 * every other argument, the return codes and the arithmetic are those of the 8-bit twin, which stays the entry for nMat <= 256.
 * The same problem gives the same bits through either. (The x-fastest entries bfd_bhte_run / bfd_bhte_run_fields are 8-bit only.) */
int bfd_bhte_max_materials(void);
int bfd_bhte_run_volumes16(int32_t device, int32_t N1, int32_t N2, int32_t N3, int32_t nMat, const uint16_t *mat,
                           const float *cd, const float *cp, const float *qf, const float *initT, int32_t nFields,
                           const float *pressure, float *qOut, float *T, float *dose, int32_t flags, float Tcore, double dt,
                           int32_t nSteps, const int32_t *fieldOfStep, int32_t sliceJ, int32_t nFactorMonitoring,
                           float *monitorSlice, int64_t nPoints, const uint32_t *pointIndex, float *points, double *kernelMs);
int bfd_bhte_run_protocol16(int32_t device, int32_t N1, int32_t N2, int32_t N3, int32_t nMat, const uint16_t *mat,
                            const float *cd, const float *cp, const float *qf, const float *initT, int32_t nFields,
                            const float *pressure, float *qOut, float *T, float *dose, int32_t flags, float Tcore, double dt,
                            int32_t nSteps, const int32_t *fieldOfStep, int32_t sliceJ, int32_t nFactorMonitoring,
                            float *monitorSlice, int64_t nPoints, const uint32_t *pointIndex, float *points, double *kernelMs,
                            int32_t nCaptures, const int32_t *captureStep, float *Tmax, float *doseAtCapture);

/* ---- 3-D median filter: replaces scipy.ndimage.median_filter / GPUFunctions.GPUMedianFilter.MedianFilter around the solver calls ----
 * (ThermalModeling/CalculateTemperatureEffects.py:908-918: float32 pressure amplitude, size 3; BabelBrain/BabelDatasetPreps.py:870-876,
 * 1050-1053, 1069-1072: uint8 masks, sizes 7 and 3, through the callback CalculateMaskProcess.py:42-70 installs).
 *   out[i][j][k] = the element of rank n/2 (0-based, ascending) of the s1 x s2 x s3 window centred on (i,j,k), n = s1 s2 s3
 * in and out: HOST pointers to [N1][N2][N3] volumes in numpy C order (k fastest), dtype 0 = uint8, 1 = float32; in is never written and out
 * may not overlap it. Each s is 1, 3, 5 or 7 (the reference's limit is 7 per axis). mode 0 = scipy's 'reflect' (the default there; the
 * reference kernel's -1-ix / 2 dim-1-ix), 1 = 'constant' with cval (for uint8 an integer in 0..255; for float32 rounded to float32).
 * Every dimension must be at least s/2 on its axis (one reflection suffices), and the volume must have fewer than 2^31 voxels: otherwise -1,
 * nothing is truncated. The output is one of the window's input values with its bits unchanged: nothing is flushed or rounded, float32
 * denormals included; where a window holds both -0.0 and +0.0 either may come out. Behaviour on NaN is undefined.
 * regionMask (may be NULL): uint8 [N1][N2][N3]; out = regionMask != 0 ? median : in, bit for bit (4 x 4 x 64 tiles without a masked voxel
 * are copied). kernelMs (may be NULL): device time of the kernel alone, HIP events. Device memory during the call: two volumes and the mask.
 * Returns 0; -1 bad argument (reported before a device is looked for), -3 no such device, -10 device error; text in bfd_last_error.
 * There is no CPU fallback. */
int bfd_median_filter3d(int device, int dtype /*0 u8, 1 f32*/, const void *in, void *out,
                        const uint8_t *regionMask /*may be NULL*/,
                        int64_t N1, int64_t N2, int64_t N3, int s1, int s2, int s3,
                        int mode /*0 reflect, 1 constant*/, double cval, float *kernelMs /*may be NULL*/);

/* ---- binary morphology and component labelling of Step-1 masks: what follows the median in BabelDatasetPreps.py ----
 * (:881-883 BinaryClosingFilter = scipy.ndimage.binary_closing with an all-ones structure of round(5 mm / voxel) per axis; :901, :953, :1106
 * binary_dilation / binary_erosion with the default cross and iterations; :888-894, :910-929, :1055-1058, :1078-1081 LabelImage, the largest region.)
 * Conventions of bfd_median_filter3d: HOST pointers to [N1][N2][N3] volumes in numpy C order (k fastest), fewer than 2^31 voxels; the input is never
 * written and no output may overlap it; returns 0; -1 bad argument (reported before a device is looked for), -3 no such device, -10 device error;
 * text in bfd_last_error; kernelMs (may be NULL): device time of the kernels alone, HIP events; device memory lives for the call; no CPU fallback.
 *
 * bfd_binary_morphology3d: op 0 erosion, 1 dilation, 2 closing, 3 opening of the uint8 mask `in` (non-zero = true) into `out` (exactly 0 or 1), equal
 * voxel for voxel to scipy.ndimage.binary_erosion / binary_dilation / binary_closing / binary_opening(in, structure, iterations, border_value=...)
 * with origin 0, scipy's mirrored window for even sizes included. structure: uint8 [s1][s2][s3] (non-zero = true), or NULL for the 3 x 3 x 3 cross
 * generate_binary_structure(3, 1) (s1, s2, s3 are then ignored). An all-ones structure may have 1..31 elements per axis and is applied as three
 * 1-D passes per erosion / dilation; any other structure at most 7 per axis and at least one true element (otherwise -1). iterations >= 1.
 * borderValue (what lies outside the volume): 0 or 1 for erosion and dilation, 0 for closing and opening. Device memory during the call: the
 * volume (1 B per voxel) and two bit-packed copies (1 bit per voxel each, rows padded to 64 voxels). */
int bfd_binary_morphology3d(int device, int op /*0 erode, 1 dilate, 2 close, 3 open*/, const uint8_t *in, uint8_t *out,
                            int64_t N1, int64_t N2, int64_t N3, const uint8_t *structure /*may be NULL: the cross*/, int s1, int s2, int s3,
                            int iterations, int borderValue, float *kernelMs /*may be NULL*/);

/* bfd_label3d: connected components of the uint8 mask `in` (non-zero = foreground). connectivity 1, 2, 3 = 6, 18, 26 neighbours, scipy's
 * generate_binary_structure(3, connectivity). labels (int32 [N1][N2][N3], may be NULL): 0 = background, components numbered 1..n in the order of their
 * first voxel in C-order raster scan -- equal element for element to scipy.ndimage.label(in, generate_binary_structure(3, connectivity))[0].
 * numLabels (may be NULL) receives n. sizes (int64, may be NULL) receives the voxel counts of labels 1..n when sizesCapacity >= n, and is left alone
 * otherwise. largest (uint8 [N1][N2][N3], may be NULL) receives the mask (0 / 1) of the component with the most voxels, among equals the one with
 * the highest label; all zero when there is no component. At least one output must be asked for. Device memory during the call: 9 B per voxel
 * (the mask, parents / labels, root ranks), the prefix sum's scratch block and 8 B per component. */
int bfd_label3d(int device, const uint8_t *in, int32_t *labels /*may be NULL*/, int64_t N1, int64_t N2, int64_t N3, int connectivity,
                int64_t *numLabels /*may be NULL*/, int64_t *sizes /*may be NULL*/, int64_t sizesCapacity, uint8_t *largest /*may be NULL*/,
                float *kernelMs /*may be NULL*/);

/* ---- spline resampling of Step-1 volumes: scipy.ndimage.affine_transform / spline_filter behind GPUFunctions/GPUResample/Resample.py::ResampleFromTo ----
 * (callback installed at CalculateMaskProcess.py:65-74; callers BabelDatasetPreps.py:859 CT, order 3; :1168 T1, order 0; CTZTEProcessing.py:258.)
 * Conventions of bfd_median_filter3d: HOST pointers to C-order volumes (k fastest), input and output each fewer than 2^31 voxels, the input is
 * never written and out may not overlap it; returns 0; -1 bad argument (reported before a device is looked for), -3 no such device, -10 device
 * error; text in bfd_last_error; kernelMs (may be NULL): device time of the kernels alone, HIP events; device memory lives for the call and is
 * freed on every path; no CPU fallback.
 * dtype: 0 uint8, 1 float32, 2 int16, 3 float64, of in and of out alike. matrix: twelve doubles, row a = (m_a0, m_a1, m_a2, offset_a); output
 * voxel (i, j, k) takes the input at coordinate_a = offset_a + m_a0 i + m_a1 j + m_a2 k. order 0..3; mode 0 constant (cval outside
 * [0, N - 1]), 1 nearest, 2 mirror, with scipy's meaning, scipy's 12-sample edge padding before the prefilter of `nearest` included.
 * flags: bit 0 (1) = prefilter: with order >= 2, in holds samples and the B-spline coefficients are computed first (float64, on the device);
 * otherwise in is interpolated as it is. Bit 1 (2) = gathered interpolation also at order 3, where the default stages the source box of each
 * 4 x 8 x 32 output tile in LDS; the two give the same bits (for checks and timing). kernelMs here points to TWO floats: device time of the
 * prefilter and of the interpolation. All arithmetic is float64, rounded once at the store: to float32 by the conversion, to the integer dtypes by scipy's
 * rule, trunc(t + 0.5) for t > 0 and trunc(t - 0.5) otherwise (half away from zero), saturating; uint8 gives 0 for every t <= 0. cval takes the
 * same conversion and must be finite for integer dtypes; the matrix must be finite. Device memory: in, out and, with the prefilter,
 * 8 B per (padded) input voxel. */
int bfd_affine_transform3d(int device, int dtype, const void *in, void *out, int64_t N1, int64_t N2, int64_t N3,
                           int64_t O1, int64_t O2, int64_t O3, const double *matrix /*[12]*/, int order, int mode, double cval, int flags,
                           float *kernelMs /*[2], may be NULL*/);

/* bfd_spline_filter3d: the prefilter alone, scipy.ndimage.spline_filter(in, order, output=float64, mode): out is float64 [N1][N2][N3]. Modes
 * constant and mirror filter with mirror boundaries, nearest with reflect boundaries (no padding here, as in scipy); orders 0 and 1 and axes of
 * length 1 pass through. */
int bfd_spline_filter3d(int device, int dtype, const void *in, double *out, int64_t N1, int64_t N2, int64_t N3, int order, int mode,
                        float *kernelMs /*may be NULL*/);

/* ---- mesh voxelisation: GPUFunctions.GPUVoxelize.Voxelize (BabelDatasetPreps.py:570, :667, :670, :673; callback installed at CalculateMaskProcess.py) ----
 * Conventions of bfd_median_filter3d: HOST pointers; returns 0; -1 bad argument (reported before a device is looked for), -3 no such device, -10
 * device error; text in bfd_last_error; kernelMs (may be NULL): device time of the kernels alone, HIP events; device memory lives for the call and
 * is freed on every path; no CPU fallback.
 *
 * bfd_voxelize_mesh: solid voxelisation of a surface mesh by parity along x. triangles: float32 [n][3][3]; box min[3], max[3]; grid (gx, gy, gz);
 * u_a = (max_a - min_a) / g_a. All arithmetic is float64, one operation per rounding (no fused multiply-add, no sqrt: the normal is not normalised),
 * on coordinates relative to min. Voxel (i, j, k) is set iff an ODD number of triangles satisfy (a) and (b):
 *   (a) the triangle's projection onto (y, z) contains the column centre p = ((j + 1/2) u_y, (k + 1/2) u_z). The projection is made counter-clockwise
 *       by exchanging its second and third vertex when its signed area (b - a) x (c - a) is negative; a triangle of signed area exactly 0 is skipped.
 *       The edge function of edge a->b is t = (p_y - a_y)(p_z - b_z) - (p_z - a_z)(p_y - b_y), evaluated in that form: the neighbouring triangle, which
 *       sees the edge as b->a, then gets exactly -t, which keeps a closed mesh watertight. The test passes for t > 0 on all three edges, and for
 *       t == 0 on an edge that is top-left: b_z < a_z, or b_z == a_z and a_y > b_y (the reference's TopLeftEdge).
 *   (b) the surface lies at or beyond the voxel centre: floor(xs / u_x - 1/2) >= i, with xs = v0_x - (n_y (p_y - v0_y) + n_z (p_z - v0_z)) / n_x and
 *       n = (v1 - v0) x (v2 - v1) of the vertices as given. A surface beyond the last voxel counts for every i; one below the first voxel centre,
 *       or a NaN (n_x == 0 under a zero numerator), for none.
 *   Only columns inside the triangle's box ceil(min / u - 1/2) .. floor(max / u - 1/2), clamped to the grid, are looked at.
 * Differences from the reference's voxelize.cpp, on purpose: it truncates toward zero where (b) floors (a surface within half a voxel of the box's low
 * x face empties voxel 0 there); it takes |t| < 1e-6, an absolute threshold, as "on the edge"; it drops triangles with |n_x| / |n| < 1e-6; it computes
 * in float32. Outputs, each may be NULL but not all:
 *   table  uint32 [ceil(gx gy gz / 32)]: one bit per voxel, bit 31 - (index % 32) of word index / 32 with index = i + gx (j + gy k) (the reference's
 *          packing); the padding bits of the last word are 0
 *   mask   uint8 [gz][gy][gx] (0 / 1), only below 2^31 voxels
 *   count  the number of set voxels
 * The result does not depend on the order of the triangles, nor on which vertex of a triangle comes first (a cyclic rotation), and is the same bits
 * from run to run: every crossing is one atomic XOR of one bit, and XOR commutes. One atomic per (triangle, column) that passes (a), where the
 * reference issues one per voxel below the surface. -1: n < 1, g_a < 1 or >= 2^31, more than 2^40 voxels, a non-finite vertex or box, max_a <= min_a,
 * a voxel size that is not positive and finite, a mask at 2^31 voxels or more, outputs that overlap. float32 denormals among the vertices may be read
 * as 0. Device memory during the call: 36 + 128 B per triangle, 2 bits per voxel in rows of gx + 1 bits padded to 64 (crossings, occupancy), the table,
 * the mask when asked for. */
int bfd_voxelize_mesh(int device, const float *triangles, int64_t nTriangles, const double *min /*[3]*/, const double *max /*[3]*/,
                      int64_t gx, int64_t gy, int64_t gz, uint32_t *table /*may be NULL*/, uint8_t *mask /*may be NULL*/,
                      int64_t *count /*may be NULL*/, float *kernelMs /*may be NULL*/);

/* bfd_voxel_points: the centres of the set voxels of a table in bfd_voxelize_mesh's packing (padding bits are ignored), in ascending index
 * i + gx (j + gy k) -- the same order in every run, where the reference's atomic counter gives another each time. points: float32 [count][3];
 * coordinate a = (float)(min_a + (idx_a + 0.5) unit_a), formed in float64 and rounded once. count (may be NULL) receives the table's population, which
 * is taken on the host before a device is looked for: with capacity below it the call returns -1 and count is still written (call with capacity 0 and
 * points NULL to size the array). Stateless: the table need not come from bfd_voxelize_mesh. Device memory: the table, 8 B per table word, the points. */
int bfd_voxel_points(int device, const uint32_t *table, int64_t gx, int64_t gy, int64_t gz, const double *min /*[3]*/, const double *unit /*[3]*/,
                     float *points /*may be NULL when capacity is 0*/, int64_t capacity, int64_t *count /*may be NULL*/, float *kernelMs /*may be NULL*/);

/* ---- conformal masks: the scatter of the voxel centres through the rotated affine, BabelDatasetPreps.py:710-759 ----
 * (per mesh: hstack, np.round(np.dot(InVAffineRot, XYZ)).astype(np.int64), the filter of the upper side :740-743, the fancy-index store.)
 * Same conventions as bfd_voxelize_mesh. The points never exist on the host: only the mask (1 B per voxel of the simulation grid), the index bounds
 * and four counts come back.
 *
 * Points. The points of a table are those of bfd_voxel_points: one per set voxel, index = i + gx (j + gy k), padding bits ignored; coordinate a of
 * a point is (float)(min_a + (idx_a + 0.5) unit_a), formed in float64 and rounded once.
 * Transform. matrix: float32 [3][4], the first three rows of InVAffineRot. Row a of a point (x, y, z) is
 *     t_a = ((m_a0 x + m_a1 y) + m_a2 z) + m_a3
 * with every product and every sum rounded to float32 on its own, in exactly this order, no fused multiply-add; n_a = rint(t_a), half to even, as
 * np.round has it. The build flushes float32 denormals: a flushed operand changes a t_a by less than 2^-126 and cannot move it across a
 * half-integer. A t_a that is not finite or is at least 2^31 in magnitude saturates: n_a = INT32_MAX for t_a >= 2^31, INT32_MIN for t_a <= -2^31 and
 * for NaN.
 * Output. out: uint8 [M1][M2][M3], last axis fastest, written whole with 0 or 1. A point sets voxel (n_0, n_1, n_2) with numpy's index rules behind
 * the reference's filter:
 *     a point with any n_a >= M_a is dropped ("above"; the filter comes first, whatever the point's other indices are);
 *     otherwise a point with any n_a < -M_a is dropped ("below": numpy raises IndexError there; a saturated index is always on its side);
 *     otherwise an index in [-M_a, 0) wraps by +M_a ("wrapped": the reference filters only the upper side).
 *   counts  int64 [4] = {points, above, wrapped, below}, each point counted once beside `points`
 *   lo, hi  int64 [3] each: the minimum and maximum of n_a over all points before any dropping, saturated to the int32 range as above; left
 *           alone when the table has no point. They come together.
 * With out == NULL the call is the bounds pass: M1..M3 are ignored and counts[1..3] are 0. At least one of out, lo/hi, counts must be asked for.
 * An empty table is not an error: out all zero, counts all zero, lo and hi untouched. The result is a set: the same bytes in every run.
 * tests/conformal_oracle.py restates all of this in numpy with elementwise float32 operations; the device equals it voxel for voxel and number
 * for number.
 * -1, in this order: the grid errors of bfd_voxel_points (min and unit finite); a non-finite matrix; M_a < 1 where out is given; an out of 2^31 voxels
 * or more; an out that overlaps an input; lo without hi; no output asked for. kernelMs brackets the memset of out and the kernel, never a copy.
 * Device memory: the table, out. */
int bfd_voxel_scatter3d(int device, const uint32_t *table, int64_t gx, int64_t gy, int64_t gz, const double *min /*[3]*/, const double *unit /*[3]*/,
                        const float *matrix /*[12]*/, int64_t M1, int64_t M2, int64_t M3, uint8_t *out /*may be NULL*/, int64_t *lo /*may be NULL*/,
                        int64_t *hi /*may be NULL*/, int64_t *counts /*may be NULL*/, float *kernelMs /*may be NULL*/);

/* bfd_voxelize_scatter3d: bfd_voxelize_mesh's table of the mesh, made on the device and scattered there (unit_a = (max_a - min_a) / g_a): what
 * bfd_voxelize_mesh -> bfd_voxel_scatter3d gives, without the table or any point leaving the device. -1: the triangle, grid, box and vertex errors
 * of bfd_voxelize_mesh, then the errors above from the matrix on. kernelMs brackets the voxelisation too. */
int bfd_voxelize_scatter3d(int device, const float *triangles, int64_t nTriangles, const double *min /*[3]*/, const double *max /*[3]*/,
                           int64_t gx, int64_t gy, int64_t gz, const float *matrix /*[12]*/, int64_t M1, int64_t M2, int64_t M3,
                           uint8_t *out /*may be NULL*/, int64_t *lo /*may be NULL*/, int64_t *hi /*may be NULL*/, int64_t *counts /*may be NULL*/,
                           float *kernelMs /*may be NULL*/);

/* ---- CT value mapping: GPUFunctions.GPUMapping.MappingFilter.MapFilter (BabelDatasetPreps.py:1039; host loop :1034-1037) ----
 * Same conventions. out[v] (uint32) = the row m with unique[m] == hu[v] where sel[v] != 0 and such a row exists, 0 everywhere else -- what the
 * reference's kernel leaves in its zero-initialised output. == is float32 equality: -0.0 matches +0.0, a NaN in hu matches nothing. unique: float32
 * [nU], 1 <= nU <= 65536, STRICTLY INCREASING (np.unique output is; checked, a NaN included: -1), searched by bisection; staged in LDS up to 4096 rows.
 * hu float32 [N], sel uint8 [N], N >= 0 elements in any shape; out may not overlap an input. One pass: 5 B read and 4 B written per element. */
int bfd_map_values3d(int device, const float *hu, const uint8_t *sel, const float *unique, int64_t nU, uint32_t *out, int64_t N,
                     float *kernelMs /*may be NULL*/);

/* ---- exact Euclidean distance transform and Gaussian filter: the scipy.ndimage calls of the bone-rim correction, BabelDatasetPreps.py:936-1017 ----
 * (:967 ndimage.distance_transform_edt(inv_interior); :984, :986 ndimage.gaussian_filter(volume, sigma=sigma_local) on float32 volumes; the erosion
 * of :953 is bfd_binary_morphology3d with an all-ones structure.)
 * Conventions of bfd_median_filter3d: HOST pointers to [N1][N2][N3] volumes in numpy C order (k fastest), fewer than 2^31 voxels; the input is never
 * written and no output may overlap it; returns 0; -1 bad argument (reported before a device is looked for), -3 no such device, -10 device error;
 * text in bfd_last_error; kernelMs (may be NULL): device time of the kernels alone, HIP events; on a refusal (-1, -3) the outputs and kernelMs are
 * untouched; device memory lives for the call and is freed on every path; an empty volume returns 0 after the device pick; no CPU fallback.
 *
 * bfd_distance_transform_edt3d: a voxel is BACKGROUND where in == 0, with bit 0 of flags ("invert") where in != 0 (other bits of flags: -1).
 * dist2[v] (int32, may be NULL) = the smallest squared Euclidean distance, in voxels, from v to a background voxel, as an exact integer (0 at a
 * background voxel); dist[v] (float64, may be NULL) = its square root, taken on the device: correctly rounded, so dist equals
 * scipy.ndimage.distance_transform_edt(in) element for element (scipy forms the same integer in float64 and takes one square root). At least one
 * output must be asked for. Every dimension is at most 16384, so that 3 (N - 1)^2 stays within int32; a volume without any background voxel is
 * refused (scipy's result there is not a distance): both -1, the second after a host pass over the input. The scheme is separable and works in
 * integers throughout: nearest background voxel per row from the bit-packed mask, then the lower envelope of parabolas along j and along i with
 * intersections by integer division. The same bits from run to run. Device memory during the call: the mask (1 B per voxel), its bits (rows padded to 64
 * voxels), 4 B per voxel for the squared distances and 8 B per voxel of scratch (the stacks of the envelope passes, then the roots). */
int bfd_distance_transform_edt3d(int device, const uint8_t *in, int flags /*bit 0: invert*/, int32_t *dist2 /*may be NULL*/, double *dist /*may be NULL*/,
                                 int64_t N1, int64_t N2, int64_t N3, float *kernelMs /*may be NULL*/);

/* bfd_gaussian_filter3d: scipy.ndimage.gaussian_filter(in, sigma, order=0, mode=..., cval=..., truncate=...) with out of in's dtype: 1 float32,
 * 3 float64 (the codes of bfd_affine_transform3d). sigma: three float64, one per axis. Per axis the host forms scipy's weights in float64: radius
 * r = int(truncate sigma + 0.5), w(x) = exp(-0.5 / sigma^2 * x^2) for x = -r .. r over their sum (numpy's pairwise sum; exp as numpy takes it on the CPU at hand, so that the
 * weights are those of scipy on the same machine bit for bit: bfd_distance_core.h, gauss_exp). An axis with sigma <= 1e-15 is
 * skipped, as scipy skips it; with all three skipped out is a copy of in. r <= 127 per axis; sigma and truncate finite and not negative: otherwise
 * -1. mode 0 reflect (d c b a | a b c d | d c b a, scipy's default), 1 constant (cval, as float64), 2 nearest, 3 mirror (d c b | a b c d | c b a),
 * each for any ratio of radius to axis length (an axis of length 1 under radius 12 takes as many reflections as it needs). The axes are filtered in the
 * order 0, 1, 2; every sum is float64, formed in scipy's order for a symmetric kernel (the centre term, then (x[p - d] + x[p + d]) w[d] from d = r
 * down to 1) without contraction, and rounded to dtype once per axis, as scipy rounds when it writes its intermediate into the output array.
 * Device memory during the call: two volumes. */
int bfd_gaussian_filter3d(int device, int dtype /*1 f32, 3 f64*/, const void *in, void *out, int64_t N1, int64_t N2, int64_t N3,
                          const double *sigma /*[3]*/, double truncate, int mode /*0 reflect, 1 constant, 2 nearest, 3 mirror*/, double cval,
                          float *kernelMs /*may be NULL*/);

/* ---- the final tissue mask: the whole-volume stages of BabelDatasetPreps.py between the conformal masks and the file Step 2 reads ----
 * Conventions of bfd_median_filter3d and of the section above: HOST pointers, numpy C order, fewer than 2^31 voxels, inputs never written, 0 / -1 (before
 * a device is looked for) / -3 / -10, text in bfd_last_error, kernelMs the kernels alone, outputs untouched on an argument refusal, nothing held
 * on the device after the call.
 *
 * bfd_paint_components3d: the components of the foreground in == value, chosen by size, set to `fill`; the labels never leave the device.
 * Replaces label -> regionprops -> sorted(key=area) -> np.isin -> masked store (:909-929, :1077-1097; :1055-1061 for select 2).
 * Components and their labels are bfd_label3d's (raster order of the first voxel; connectivity 1, 2, 3). The LARGEST component has the most voxels,
 * among equals the HIGHEST label: what sorted(regionprops(...), key=area)[-1] selects, Python's sort being stable and regionprops listing by label.
 *   select 0  every component except the largest                                                    (:922-924)
 *   select 1  every component except the largest whose size a satisfies (double)a < 0.1 * (double)L, L the size of the largest; the product is
 *             formed once in float64, as Python forms 0.1*regions[-1].area                          (:926, bApplyBOXFOV)
 *   select 2  the largest alone                                                                     (:1061)
 * out = in with the selected voxels set to fill; every other voxel is copied, whatever its value. counts int64 [4] = {components, size of the
 * largest, components painted, voxels painted}. Without foreground out = in and the counts are 0 (the reference raises at regions[-1]). An empty
 * volume returns 0 after the device pick with the counts zeroed.
 * -1, in this order: a null pointer (in, out, counts); a negative dimension; 2^31 voxels or more; value or fill outside 0 .. 255; connectivity outside
 * 1 .. 3; select outside 0 .. 2; out overlapping in. kernelMs is the sum of the timed sections (labelling, sizes, flags and painting).
 * Device memory: bfd_label3d's 9 B per voxel and 8 B per component, and 1 B per voxel for out. */
int bfd_paint_components3d(int device, const uint8_t *in, uint8_t *out, int64_t N1, int64_t N2, int64_t N3, int value, int connectivity,
                           int select /*0 all but the largest, 1 the small ones, 2 the largest*/, int fill, int64_t *counts /*[4]*/,
                           float *kernelMs /*may be NULL*/);

/* bfd_quantize_values3d: min and max of `values` under the mask, the quantisation to 2^bits levels, the table of distinct quantised values and the
 * index map, :1019-1027 and :1039 in one call. All float32, one rounding per operation, no fused multiply-add:
 *     mn, mx = min, max of values where mask != 0          A = mx - mn          M = 2^bits - 1
 *     s = fl32(M / A)        r = fl32(A / M)
 *     level(x) = rint(fl32(s * fl32(x - mn)))              half to even, as np.round
 *     v(l)     = fl32(fl32(r * l) + mn)
 *   quantized  float32 [N1][N2][N3], may be NULL: v(level(x)) under the mask, values elsewhere
 *   table      float32, room for 2^bits: the distinct v(l) of the levels that occur, ascending (np.unique(ndataCT[nfct]) after :1026). v is
 *              non-decreasing in l; levels whose values are equal share a row
 *   numValues  the number of rows written
 *   map        uint32 [N1][N2][N3], may be NULL: the row of v(level(x)) under the mask, 0 elsewhere (what MapFilter returns at :1039)
 *   range      float32 [2] = {mn, mx}
 * This equals the reference's expression under numpy 1.x (float64 scalars A/M, M/A demoted against the float32 array) and 2.x (float32 divisions): a
 * float64 quotient of two float32 values rounded to float32 is the correctly rounded float32 quotient. The build flushes float32 denormals and numpy
 * does not: the definition covers inputs whose intermediates are normal or zero. tests/tissue_oracle.py restates it in numpy.
 * -1 before a device is looked for, in this order: a null pointer (values, mask, table, numValues, range); a negative dimension; 2^31 voxels or
 * more; bits outside 1 .. 16; an output overlapping an input or the other output. -1 AFTER the device pick and the min / max reduction, before any
 * output is written, in this order: an empty mask (an empty volume included); a value under the mask that is not finite; A not finite in float32;
 * A == 0 (a denormal A is zero to the device); r < 2^-126. The text of each of these, and of no other error, reads "bfd_quantize_values3d: refused data: ...".
 * kernelMs is zero after such a refusal, the other outputs are untouched.
 * Device memory: 5 B per voxel, 4 B per voxel for each of quantized and map, 6 B per level. */
int bfd_quantize_values3d(int device, const float *values, const uint8_t *mask, int64_t N1, int64_t N2, int64_t N3, int bits /*1 .. 16*/,
                          float *quantized /*may be NULL*/, uint32_t *map /*may be NULL*/, float *table /*2^bits floats*/, int64_t *numValues,
                          float *range /*[2]*/, float *kernelMs /*may be NULL*/);

/* bfd_clear_beyond_bone3d: the pre-focal cleanup, :1122-1133 without the two flips. Per line (i, j): let kb be the largest k > kFocal with
 * in[i][j][k] equal to boneA or boneB; if there is one, every k > kb with in == from becomes `to`. Everything else is copied: a line without such
 * bone, any bone at k <= kFocal, `from` voxels at or below kb. counts int64 [2] = {lines with such bone, voxels changed}. An empty volume (with
 * N3 > kFocal) returns 0 after the device pick with the counts zeroed.
 * -1, in this order: a null pointer (in, out, counts); a negative dimension; 2^31 voxels or more; kFocal outside 0 .. N3 - 1; boneA, boneB, from or
 * to outside 0 .. 255; out overlapping in. Device memory: two volumes. */
int bfd_clear_beyond_bone3d(int device, const uint8_t *in, uint8_t *out, int64_t N1, int64_t N2, int64_t N3, int64_t kFocal, int boneA, int boneB,
                            int from, int to, int64_t *counts /*[2]*/, float *kernelMs /*may be NULL*/);

/* ---- the domain setup of Step 2: what TranscranialModeling/BabelIntegrationBASE.py does between the mask file and the solver call ----
 * Conventions of the section above: HOST pointers, numpy C order (k fastest), fewer than 2^31 voxels per volume, inputs never written, 0 / -1 (before
 * a device is looked for) / -3 / -10, text in bfd_last_error, kernelMs the kernels alone, outputs untouched on a refusal, nothing held on the
 * device after the call. The driver flips axis 2 of every volume it loads (:1161, :1176, :1179, :1844). With flipK = 1 the entries read the stored
 * volume at M3 - 1 - k, and every index they take or report is in the driver's (flipped) coordinates; the flipped copy never exists.
 * tests/domain_oracle.py restates the three definitions in numpy.
 *
 * bfd_label_survey3d: what the driver asks of the label volume (:1163, :1903-1908, :2162), in one pass. The box lo, hi is half-open, in driver
 * coordinates.
 *   hist    int64 [256]: the number of voxels of each label inside the box
 *   bounds  int64 [6] = {min i, max i, min j, max j, min k, max k} of the voxels inside the box with label > 0, relative to lo; all -1 where none.
 *           bounds[4] is FirstVoxelTissueZ - ZLOffset of :1903-1904 for the crop the box stands for
 *   focal   int64 [2] = {voxels equal to 5 in the WHOLE volume, the smallest C-order linear index of one in driver coordinates or -1}
 * An empty volume returns 0 after the device pick with hist zeroed, bounds -1 and focal {0, -1}.
 * -1, in this order: a null pointer (labels, lo, hi, hist, bounds, focal); a negative dimension; 2^31 voxels or more; a box that is not
 * 0 <= lo <= hi <= M on every axis; flipK outside 0 .. 1. Device memory: one volume. */
int bfd_label_survey3d(int device, const uint8_t *labels, int64_t M1, int64_t M2, int64_t M3, const int64_t *lo /*[3]*/, const int64_t *hi /*[3]*/,
                       int flipK, int64_t *hist /*[256]*/, int64_t *bounds /*[6]*/, int64_t *focal /*[2]*/, float *kernelMs /*may be NULL*/);

/* bfd_assemble_material_map3d: :2111-2201 (the path that is neither water only nor a test hook). The source box lo, size of the volumes [M1][M2][M3]
 * (driver coordinates) lands at padLo in outputs of N = size + padLo + padHi per axis; outside it every output is 0. With raw the label at a voxel:
 *   mapNoCT  uint32 [N], may be NULL: raw (:2166, before the relabelling and before the water layer)
 *   airOut   uint32 [N], may be NULL: air at the voxel, 0 where air is NULL (:2183-2190; no water layer)
 *   map      uint32 [N]: lut[raw] where bit 31 of lut[raw] is clear, ct + ctOffset (uint32 arithmetic) where it is set; then 0 on the planes
 *            k <= zWater (:2201; -1: none). The sequential relabels of :2169-2173 and :2196-2198 are functions of raw: the caller runs them on
 *            0 .. 255 and hands the result as lut. ct is the index map as stored (uint16 or uint32 by ctBytes), ctOffset 3 or 6 (:1241-1244)
 *   stats    int64 [8] = {voxels taken from ct (bone); the min and the max of ct + ctOffset over them, before the water layer, as the asserts of
 *            :2191-2192 see them, -1 without bone; voxels with map > 0; the max of map; the smallest k with map > 0, -1 if none; the same on the
 *            column focalIJ (what CalculateDomainZReference reads, :2609-2614; the reference aliases _MaterialMap and _MaterialMapRef at :2161, so
 *            that method sees the final map); voxels with map >= nMaterials}
 * An empty map (a zero in N) returns 0 after the device pick with stats {0, -1, -1, 0, 0, -1, -1, 0}.
 * -1, in this order: a null pointer (labels, lo, size, padLo, padHi, lut, focalIJ, map, stats); a negative dimension; 2^31 voxels or more in the
 * source; ctBytes outside {0, 2, 4} or not 0 exactly where ct is NULL; a box that is not 0 <= lo, 0 <= size, lo + size <= M; a padding outside
 * 0 .. 2^31 - 1; a map of 2^31 voxels or more; flipK outside 0 .. 1; a lut entry with bit 31 while ct is NULL; zWater < -1; nMaterials outside
 * 0 .. 2^32 - 1; focalIJ outside the map (a non-empty map only); an output overlapping an input or another output.
 * Device memory: the inputs handed, and 4 B per voxel of N for each output. */
int bfd_assemble_material_map3d(int device, const uint8_t *labels, const void *ct /*may be NULL*/, int ctBytes /*0, 2, 4*/, const uint8_t *air /*may be NULL*/,
                                int64_t M1, int64_t M2, int64_t M3, const int64_t *lo /*[3]*/, const int64_t *size /*[3]*/, const int64_t *padLo /*[3]*/,
                                const int64_t *padHi /*[3]*/, int flipK, const uint32_t *lut /*[256]*/, uint32_t ctOffset, int64_t zWater, int64_t nMaterials,
                                const int64_t *focalIJ /*[2]*/, uint32_t *map, uint32_t *mapNoCT /*may be NULL*/, uint32_t *airOut /*may be NULL*/,
                                int64_t *stats /*[8]*/, float *kernelMs /*may be NULL*/);

/* bfd_sdr_rays3d: compute_sdr_from_rays, :816-854, on the box lo, size of the CT index volume (uint16 or uint32 by ctBytes, as stored, WITHOUT the
 * offset of :1241-1244), with HU = hu[index] and skull = index > 0 as :1385-1392 form them. hu is float32 or float64 (huBytes 4 or 8) and `value` has
 * its type. One ray per (r, c) of the lattice ceil(size[0] / stepI) x ceil(size[1] / stepJ), r outer and c inner, along k at
 * (lo[0] + r stepI, lo[1] + c stepJ). With n the skull voxels of the ray (count) and p(q) the position of the one of rank q:
 *   state 4  an index >= nHU on the ray (numpy raises IndexError at :1389; only the rays of the lattice are looked at)
 *   state 0  n < minSkullVoxels
 *   else     mid = n // 2, l_half = n centerRegion, beg = max(0, rint(mid - l_half / 2)), end = min(n - 1, 1 + rint(mid + l_half / 2)), in float64,
 *            one rounding per operation, rint half to even as np.round (dm_segment of csrc/bfd_domain_core.h)
 *   state 3  beg >= end: the centre slice is empty (numpy's .min() raises ValueError)
 *   state 2  the maximum of hu over the skull voxels is <= 0
 *   state 1  value = min(hu[index] for every voxel p(beg) <= p < p(end), skull or not: a voxel of index 0 contributes hu[0]) / that maximum, one
 *            division in the table's type
 * value is 0 unless the state is 1. A lattice without rays returns 0 after the device pick and writes nothing.
 * -1, in this order: a null pointer (ct, lo, size, hu, value, count, state); a negative dimension; 2^31 voxels or more; ctBytes outside {2, 4}; a box
 * that is not 0 <= lo, 0 <= size, lo + size <= M; flipK outside 0 .. 1; huBytes outside {4, 8}; nHU outside 1 .. 2^31 - 1; a hu that is not
 * finite; stepI or stepJ outside 1 .. 2^31 - 1; minSkullVoxels outside 1 .. 2^31 - 1; centerRegion negative or not finite.
 * Device memory: the index volume, the table and 5 B + huBytes per ray. */
int bfd_sdr_rays3d(int device, const void *ct, int ctBytes /*2, 4*/, int64_t M1, int64_t M2, int64_t M3, const int64_t *lo /*[3]*/, const int64_t *size /*[3]*/,
                   int flipK, const void *hu, int huBytes /*4, 8*/, int64_t nHU, int64_t stepI, int64_t stepJ, int64_t minSkullVoxels, double centerRegion,
                   void *value, int32_t *count, uint8_t *state, float *kernelMs /*may be NULL*/);

/* ---- the pseudo-CT from ZTE / PETRA: the whole-volume steps of BabelBrain/CTZTEProcessing.py, ConvertZTE_PETRA_pCT (:501-628) ----
 * Conventions of the sections above: HOST pointers, numpy C order (k fastest), fewer than 2^31 voxels, inputs never written, 0 / -1 (before a device
 * is looked for) / -3 / -10, text in bfd_last_error, kernelMs the kernels alone (the sum of the timed sections where the host reads a few words
 * between them), outputs untouched on a refusal, nothing held on the device after the call. `values` is float32 or float64 by dtype (1 or 3, the
 * codes of bfd_gaussian_filter3d). All arithmetic is float64, one rounding per operation; a float32 voxel is widened exactly first, denormals
 * included, as nibabel's get_fdata hands the reference float64. Byte masks are read as != 0. Four of the entries refuse DATA as well: -1 AFTER the
 * device pick and their first reduction, with kernelMs zeroed and nothing else written; the text of each of these, and of no other error, reads
 * "<entry>: refused data: ...". tests/pseudoct_oracle.py restates the definitions in numpy and scipy.
 *
 * bfd_integer_histogram3d: :559-562. range = {min, max} of the volume; first = (int64)min and last = (int64)max, truncated toward zero as
 * astype(int) truncates; numBins = last - first + 1 (at most 65536); counts[b] = the voxels v with (int64)v == first + b, so the bin of 0 collects
 * (-1, 1). counts has room for 65536; only numBins are written. Counts are integers: every run gives the same.
 * -1, in this order: dtype outside {1, 3}; values null; a negative dimension; 2^31 voxels or more; a null pointer (counts, first, numBins, range);
 * counts overlapping values. Refused data, in this order: an empty volume; a value that is not finite; max - min > 65535 ("The range of values in
 * the ZTE file exceeds 2^16", the reference's text); a value beyond +-2^62.
 * Device memory: the volume and 256 KiB. */
int bfd_integer_histogram3d(int device, int dtype /*1 f32, 3 f64*/, const void *values, int64_t N1, int64_t N2, int64_t N3, int64_t *counts /*[65536]*/,
                            int64_t *first, int64_t *numBins, double *range /*[2]*/, float *kernelMs /*may be NULL*/);

/* bfd_order_statistics3d: exact order statistics of the SELECTED voxels: mask != 0 (mask NULL: all) and v > above (v >= above with inclusive; a NaN
 * is never selected; above = -inf with inclusive selects every voxel that is not a NaN). count = their number n. With ranks (R of them, 1 .. 4, each
 * 0 .. n - 1): statistics[r] = the value at rank ranks[r] of the ascending order. Without (ranks NULL; R is not looked at): the two ranks
 * np.percentile(x, quantile) reads, lo = floor((n - 1) * (quantile / 100)) and min(lo + 1, n - 1), in float64; statistics[0 .. 1] their values.
 * ranksUsed (may be NULL) receives the ranks. The values are found by a radix select on order-preserving integer keys of the voxels' own format (32
 * bits for float32, 64 for float64; -0.0 orders below +0.0), 8 bits a pass: no sort and no approximation; the host reads 256 counts per rank
 * between the passes. np.percentile's interpolation between the two is the caller's (pc_lerp of csrc/bfd_pseudoct_core.h restates it).
 * -1, in this order: dtype outside {1, 3}; values null; a negative dimension; 2^31 voxels or more; a null pointer (count, statistics); above a NaN;
 * inclusive outside 0 .. 1; R outside 1 .. 4 where ranks are given; quantile outside 0 .. 100 where they are not. Refused data, in this order:
 * nothing selected (an empty volume included); a rank outside 0 .. n - 1.
 * Device memory: the volume, 1 B per voxel with a mask, 4 KiB. */
int bfd_order_statistics3d(int device, int dtype /*1 f32, 3 f64*/, const void *values, const uint8_t *mask /*may be NULL*/, int64_t N1, int64_t N2, int64_t N3,
                           double above, int inclusive, const int64_t *ranks /*[R], may be NULL*/, int R, double quantile, int64_t *count,
                           int64_t *ranksUsed /*[R] or [2], may be NULL*/, double *statistics /*[R] or [2]*/, float *kernelMs /*may be NULL*/);

/* bfd_uniform_histogram3d: np.histogram(x[x > above], bins) in two calls (x >= above with inclusive; :476-477 and BabelDatasetPreps.py:828).
 *   edges NULL   range = {min, max} and count of the selected voxels (0, 0 and 0 where there are none). bins and counts are not looked at. The caller
 *                forms edges = np.linspace(min, max, bins + 1), min - 0.5 .. max + 0.5 where they are equal
 *   edges given  float64 [bins + 1], finite, ascending, edges[0] < edges[bins]; bins 1 .. 1024. counts[b] = the selected voxels in bin b by numpy's
 *                rule for equal bins: i = (int)(((a - first) / (last - first)) * bins), first = edges[0], last = edges[bins]; i == bins goes down by
 *                one; i -= 1 where a < edges[i]; then i += 1 where a >= edges[i + 1] and i != bins - 1. A selected voxel outside first .. last is
 *                not counted. range and count are not looked at
 * An empty volume returns 0 after the device pick with the outputs of the form zeroed.
 * -1, in this order: dtype outside {1, 3}; values null; a negative dimension; 2^31 voxels or more; a null pointer (counts with edges; range, count
 * without); above a NaN; inclusive outside 0 .. 1; bins outside 1 .. 1024; edges not finite or not ascending. Refused data (first form): a selected
 * value that is not finite.
 * Device memory: the volume and 12 KiB. */
int bfd_uniform_histogram3d(int device, int dtype /*1 f32, 3 f64*/, const void *values, int64_t N1, int64_t N2, int64_t N3, double above, int inclusive,
                            int bins, const double *edges /*[bins + 1] or NULL*/, int64_t *counts /*[bins]*/, double *range /*[2]*/, int64_t *count,
                            float *kernelMs /*may be NULL*/);

/* bfd_pseudo_ct_candidates3d: :577 / :592-597. q = values / divisor, one float64 division per voxel; with a head, q = -0.5 where head == 0 (ZTE;
 * PETRA hands NULL). maximum = max q over all voxels. g = q where eroded != 0, maximum elsewhere (eroded: the head after binary_erosion,
 * iterations 3). mask = 1 where lo <= g <= hi, else 0; count = the voxels of the mask. Two passes: the maximum, then the mask from the same quotients.
 * -1, in this order: dtype outside {1, 3}; values null; a negative dimension; 2^31 voxels or more; a null pointer (eroded, mask, maximum, count); a
 * divisor that is zero or not finite; lo or hi a NaN; mask overlapping an input. Refused data, in this order: an empty volume; a quotient that is not
 * finite. Device memory: the volume and 1 B per voxel for each mask. */
int bfd_pseudo_ct_candidates3d(int device, int dtype /*1 f32, 3 f64*/, const void *values, int64_t N1, int64_t N2, int64_t N3, double divisor,
                               const uint8_t *head /*may be NULL*/, const uint8_t *eroded, double lo, double hi, uint8_t *mask, double *maximum,
                               int64_t *count, float *kernelMs /*may be NULL*/);

/* bfd_pseudo_ct_convert3d: :608-621 for every voxel, in the reference's order of statements (pc_hu of csrc/bfd_pseudoct_core.h):
 *     ct = skin != 0 ? 42 : -1000
 *     bone != 0:  ct = fl(fl(slope * q) + offset)          q as in bfd_pseudo_ct_candidates3d; no fused multiply-add
 *     ct < -1000: ct = -1000          ct > 3300: ct = -1000          cavities != 0: ct = -1000
 * out is float64 (outDtype 3) or that value rounded once to float32 (1). A NaN under the bone region stays a NaN, as in numpy. An empty volume
 * returns 0 after the device pick. This entry refuses no data.
 * -1, in this order: dtype outside {1, 3}; values null; a negative dimension; 2^31 voxels or more; a null pointer (bone, skin, cavities, out);
 * outDtype outside {1, 3}; a divisor that is zero or not finite; slope or offset a NaN; out overlapping an input.
 * Device memory: the two volumes and 1 B per voxel for each mask. */
int bfd_pseudo_ct_convert3d(int device, int dtype /*1 f32, 3 f64*/, const void *values, int64_t N1, int64_t N2, int64_t N3, double divisor,
                            const uint8_t *head /*may be NULL*/, const uint8_t *bone, const uint8_t *skin, const uint8_t *cavities, double slope,
                            double offset, int outDtype /*1 f32, 3 f64*/, void *out, float *kernelMs /*may be NULL*/);

/* bfd_select_component3d (csrc/bfd_morphology.hip): the component of in != 0 with the most voxels, as a 0 / 1 mask; components and labels are
 * bfd_label3d's. Among components of equal size, tie 0 keeps the HIGHEST label (bfd_label3d's `largest`, sorted(regionprops, key=area)[-1]) and
 * tie 1 the LOWEST: sorted(props, key=pixelcount, reverse=True)[0] of :604-606, Python's sort being stable. info int64 [2] = {components, voxels
 * of the chosen one}. Without foreground out is all 0 and info is 0 (the reference raises at props[0]). An empty volume returns 0 after the
 * device pick with info zeroed.
 * -1, in this order: a null pointer (in, out, info); a negative dimension; 2^31 voxels or more; connectivity outside 1 .. 3; tie outside 0 .. 1; out
 * overlapping in. kernelMs is the sum of the timed sections (labelling, sizes, reduction and mask). Device memory: bfd_label3d's. */
int bfd_select_component3d(int device, const uint8_t *in, uint8_t *out, int64_t N1, int64_t N2, int64_t N3, int connectivity, int tie /*0 highest, 1 lowest*/,
                           int64_t *info /*[2]*/, float *kernelMs /*may be NULL*/);

/* ---- the bone-rim partial-volume correction of the CT: BabelBrain/BabelDatasetPreps.py, bMaximizeBoneRim (:935-1017), as one call ----
 * Conventions of the sections above: HOST pointers, numpy C order (k fastest), fewer than 2^31 voxels, inputs never written (out may be ct itself),
 * 0 / -1 / -3 / -10, text in bfd_last_error, kernelMs the sum of the timed sections, outputs untouched on a refusal, nothing held on the device
 * after the call. tests/bonerim_oracle.py restates the definition in numpy and scipy.
 *
 * bfd_bone_rim_correct3d (csrc/bfd_bonerim.hip). ct float32, bone read as != 0, box = RatioCTVoxels already made odd and at least 3 (:942-946):
 *     floor given:  ct = floor where bone and ct < floor                                   (:931-933; out carries these values too)
 *     dense    = ct >= interiorThreshold                                                   (:951)
 *     interior = binary_erosion(bone, ones(box)), border value 0, one iteration            (:953)
 *     gmean    = the given mean, or the exact mean of ct over dense (below)                (:957)
 *     d2       = the exact squared Euclidean distance to the nearest interior voxel        (:964-967)
 *     edge     = bone and not interior                                                     (:970)
 *     w        = exp(-sqrt(d2) / distanceScale), float64, exp as numpy takes it on the CPU at hand: a table over d2 formed on the host (:974-976)
 *     bi, bm   = gaussian_filter(ct * dense), gaussian_filter(float32(dense)), float32, sigma on the three axes, reflect, truncate 4 (:980-986)
 *     lm       = bm > float32(1e-6) ? bi / bm : gmean, float32                             (:988)
 *     at edge voxels: c = o + w * (lm - o), the subtraction float32, the rest float64; delta = min(c - o, maxBoost); out = float32(o + delta),
 *     rounded to nearest even (:994-1010). Every other voxel keeps its bits.
 *   globalMean   float32, in and out. globalMeanGiven 1: the value is used as it is (numpy's own .mean() gives the reference's bits). 0: the
 *                entry computes gmean = float32(double(S) / (16384.0 * count)), S = the sum of ct * 2^14 over dense as 64-bit integers, which is
 *                exact and the same in every run, and writes it back. numpy's pairwise float32 sum may differ from it by an ulp or so; it reaches
 *                the edge voxels with bm <= 1e-6 alone, which stats counts
 *   stats        int64 [8] = {bone, interior, dense, edge voxels; edge voxels that took gmean; edge voxels whose delta the clip lowered; voxels
 *                whose stored bits the blend changed; the largest d2 over edge voxels}
 *   interior (uint8), d2 (int32), bi, bm (float32): [N1][N2][N3], each may be NULL: the fields, for tests
 * -1 before a device is looked for, in this order: a null pointer (ct, bone, out, box, globalMean, stats); a negative dimension; a dimension above
 * 16384; 2^31 voxels or more; a box size that is even or outside 3 .. 31; interiorThreshold not finite or below 512 (every float32 from 512 up is a
 * multiple of 2^-14: the exact sum rests on it); maxBoost a NaN; distanceScale not finite or not positive; sigma not finite or not positive; the
 * radius int(4 sigma + 0.5) above 127; a floor that is not finite; globalMeanGiven outside 0 .. 1; a given mean that is not finite; an output
 * overlapping an input or another output (out == ct is no overlap). -1 AFTER the device pick, the preparation pass and the erosion, with kernelMs
 * zeroed and nothing else written, in this order: an empty volume; a CT value that is not finite; a dense value at or above 2^17; no dense voxel
 * (unless a mean is given); an erosion that leaves no interior voxel. The text of each of these, and of no other error, reads
 * "bfd_bone_rim_correct3d: refused data: ...". Device memory: 25 B per voxel, 3 bits per voxel of packed masks, 1 B per voxel with interior, the table. */
int bfd_bone_rim_correct3d(int device, const float *ct, const uint8_t *bone, float *out, int64_t N1, int64_t N2, int64_t N3, const int32_t *box /*[3]*/,
                           float interiorThreshold, double maxBoost, double distanceScale, double sigma, const float *floorValue /*may be NULL*/,
                           float *globalMean, int globalMeanGiven, int64_t *stats /*[8]*/, uint8_t *interior /*may be NULL*/, int32_t *d2 /*may be NULL*/,
                           float *bi /*may be NULL*/, float *bm /*may be NULL*/, float *kernelMs /*may be NULL*/);

/* ---- the Step-3 exposure analysis: ThermalModeling/CalculateTemperatureEffects.py, AnalyzeLosses (:94-256) and the extrema lines (:996-1001,
 * :1126-1144) ----
 * Conventions of the sections above: HOST pointers, numpy C order (k fastest, as bfd_bhte_run_volumes takes its volumes), fewer than 2^31 voxels,
 * inputs never written (waterOut may be pw itself), 0 / -1 / -3 / -10, text in bfd_last_error, kernelMs the sum of the timed sections, outputs
 * untouched on a refusal, nothing held on the device after the call. tests/thermal_oracle.py restates both definitions in numpy.
 *   map       material ids of idBytes 1, 2 or 4 (uint8, uint16, uint32), [N1][N2][N3]
 *   classOf   uint8 [nMat], 1 <= nMat <= 65536: bit c set = the id belongs to class c, 8 classes. Every selection of :864-906 and :165-179
 *             (isin, ==, !=, >, ranges, complements) is such a table
 * Results are the same bytes in every run: maxima travel as (value, index) words through integer atomics, sums are added in one fixed order; no
 * floating-point atomics. Values are compared as IEEE does, -0 == +0; float32 denormals are values like any other.
 * Refused data (-1 AFTER the device pick and the pass over the volumes, kernelMs zeroed, nothing else written), in this order: an id that is not
 * below nMat; a value of any volume that is not finite. The text of each, and of no other error, reads "<entry>: refused data: ...".
 *
 * bfd_class_extrema3d (csrc/bfd_thermal.hip): nVol float32 volumes (volumes[v] -> [N1][N2][N3]) over one map in one pass.
 *   count  [8]        voxels of class c
 *   maxIn  [nVol][8]  the maximum of x over the class, argIn the lowest linear index that attains it: X[Sel].max() of :1126-1138 and
 *                     p_map[SelBrain].argmax() with the value read (:1142-1144). An empty class: maxIn 0, argIn -1
 *   maxKey [nVol][8]  the maximum over ALL voxels of key = in ? x : x * 0.0f, argKey the lowest linear index whose key equals it: exactly
 *                     np.argmax(X * Sel.astype(np.float32)) of :996-1001. A class of negative values loses to the first +-0 outside it; an
 *                     all-zero product gives index 0. maxKey is +0 where the key is a zero of either sign
 * More than 4 volumes take one pass over the map for every 4. An empty volume returns 0 after the device pick: count 0, maxima 0, indices -1.
 * -1, in this order: a null pointer (volumes, count, maxIn, argIn, maxKey, argKey, map, classOf); a negative dimension; 2^31 voxels or more;
 * idBytes outside {1, 2, 4}; nMat outside 1 .. 65536; nVol below 1; a null volume; an output overlapping an input or another output.
 * Device memory: the volumes and the map. */
int bfd_class_extrema3d(int device, const float *const *volumes /*[nVol]*/, int nVol, const void *map, int idBytes, int64_t N1, int64_t N2, int64_t N3,
                        const uint8_t *classOf /*[nMat]*/, int nMat, int64_t *count /*[8]*/, float *maxIn, int64_t *argIn, float *maxKey,
                        int64_t *argKey, float *kernelMs /*may be NULL*/);

/* bfd_loss_survey3d (csrc/bfd_thermal.hip): the volume work of AnalyzeLosses for nFields focal spots. p, pw float32 [nFields][N1][N2][N3]: the
 * pressure amplitude in tissue and in water. Class bit 0 = brain (SelBrain), bit 1 = selregion (:165-179); brainMask, uint8 [N1][N2][N3] read as
 * != 0, replaces bit 0 where given. rho, c float64 [nMat] (Density, SoS); rhoWater, cWater = row 0 of the reference's tables; dx2 = (xf[1] - xf[0])^2.
 * Per field f:
 *   maxTissue, argTissue   the maximum of p with everything outside the brain set to 0.0f, and the first linear index that attains it (:189-195)
 *   maxWater, argWater     the same for pw with selregion set to 0.0f (:181-185)
 *   eWaterRaw [f][N3]      for every k, the sum over (i, j) of the terms of pw BEFORE the zeroing (:162-163 read plane 2 before :181)
 *   eWater    [f][N3]      of the terms of the zeroed water field (:203-204, :211-212)
 *   eTissue   [f][N3]      of the terms of the brain-masked p (:152, :207-208, :215-216)
 * A term is (((double)(float)((x * x) / 2.0f) / R) / C) * dx2: the square and the halving in float32 (denormals kept), then three float64
 * operations, each rounded once; (R, C) = (rhoWater, cWater) for water and (rho[id], c[id]) for tissue. These are the reference's types under
 * NumPy >= 2 promotion (under numpy 1.x its water energies are float32 sums). A plane's terms are added in a fixed order: rows (i, j) in ascending
 * order inside chunks of 128 rows, the chunks by a tree of 32 to a node, every node in ascending order; within (n - 1) u / (1 - (n - 1) u) of the
 * exact sum, n = N1 N2, u = 2^-53.
 * All N3 planes come from the one pass; the caller picks planes 2, cz, czw and czr.
 *   waterOut  may be NULL, or [nFields][N1][N2][N3]: the zeroed water field (the in-place store of :181); it may equal pw exactly
 * An empty volume returns 0 after the device pick: maxima 0, indices -1, sums 0.
 * -1, in this order: a null pointer (p, pw, rho, c, the four maxima and indices, the three sums, map, classOf); a negative dimension; 2^31 voxels or
 * more; idBytes outside {1, 2, 4}; nMat outside 1 .. 65536; nFields below 1; rhoWater or cWater not finite or not positive; a rho or c not finite or
 * not positive (a voxel set to 0.0f then has the term +0 and is left out of the sum); dx2 not finite or negative; nFields volumes of 2^40 voxels or
 * more; an output overlapping an input or another output other than waterOut == pw.
 * Device memory: one tissue field, one water field (nFields of them with waterOut), the map, the mask, 24 B per 128 rows and k of partial sums. */
int bfd_loss_survey3d(int device, const float *p, const float *pw, int nFields, const void *map, int idBytes, int64_t N1, int64_t N2, int64_t N3,
                      const uint8_t *classOf /*[nMat]*/, int nMat, const uint8_t *brainMask /*may be NULL*/, const double *rho, const double *c,
                      double rhoWater, double cWater, double dx2, float *maxTissue, int64_t *argTissue, float *maxWater, int64_t *argWater,
                      double *eWaterRaw, double *eWater, double *eTissue, float *waterOut /*may be NULL*/, float *kernelMs /*may be NULL*/);

/* ---- Thermal study: the volumes of one Step-3 calculation resident on the device (csrc/bfd_thermal_study.hip) ----
 * The flow of CalculateTemperatureEffects.py:908-1193 makes some ten calls over the same volumes; through the entries above every one of them
 * uploads the pressure amplitude and the map again and brings whole volumes back. A bfd_thermal handle holds them on one device from the single
 * upload of bfd_thermal_set_inputs to the results the caller asks for by name. The arithmetic is that of the entries above: the study runs the
 * same launch sequences (csrc/bfd_thermal_stages.h), so every result equals what the separate calls give, element by element.
 * Volumes are HOST pointers in numpy C order [N1][N2][N3] (last axis fastest), as bfd_bhte_run_volumes takes them; fields are
 * [nFields][N1][N2][N3].
 * The contract is that of the Step-1 entries: argument errors (-1) are reported before the device is touched, in the order each entry lists them;
 * -3 for no device or a bad ordinal; -5 for a map id that is not below nMat; -6, with a text naming the missing stage, for a stage asked for
 * before the stage it needs (set_inputs -> set_scale -> run; results of a stage exist after it); -10 for a HIP error. Outputs are untouched on a
 * refusal; kernelMs may be NULL and brackets kernels only.
 * Names of resident volumes (`which`): */
enum {
    BFD_THERMAL_TMAX = 0,             /* maximum of T over the captures of the last run; T at its end where it had none */
    BFD_THERMAL_DOSE_AT_CAPTURE = 1,  /* the dose at the last capture; the dose at the end where the run had none */
    BFD_THERMAL_T = 2,                /* temperature after the last run */
    BFD_THERMAL_DOSE = 3,             /* thermal dose after the last run */
    BFD_THERMAL_Q = 4,                /* heat increment of one ON step, [nFields] volumes, of the last run */
    BFD_THERMAL_P_MAP = 5,            /* the scaled pressure (one field) or the maximum over the scaled fields (:1115, :1118) */
    BFD_THERMAL_PW = 6,               /* the water fields, [nFields] volumes, as the median and the survey have left them */
    BFD_THERMAL_P = 7,                /* the UNSCALED tissue fields, [nFields] volumes */
    BFD_THERMAL_MAP = 8               /* the material ids (plane getter only) */
};
typedef struct bfd_thermal_s *bfd_thermal;

/* N1, N2, N3 >= 3, fewer than 2^31 voxels; 1 <= nFields <= 4096; 1 <= nMat <= bfd_bhte_max_materials(): up to 256 rows give 8-bit resident ids, more
 * 16-bit ones. Device memory, all of it taken here: 6 + 3 nFields float32 volumes (p, pw, q per field; two of T, dose, Tmax, doseAtCapture, one
 * scratch volume), the ids and one byte per voxel, with the pads of the bio-heat kernels. -1: handle null; a dimension below 3; 2^31 voxels or
 * more; nFields; nMat. */
int bfd_thermal_create(int device, int64_t N1, int64_t N2, int64_t N3, int nFields, int nMat, bfd_thermal *handle);
void bfd_thermal_destroy(bfd_thermal handle);            /* NULL is accepted */

/* ONE upload each of p and pw (float32 [nFields][N1][N2][N3]) and of the map (ids of idBytes 1, 2 or 4, narrowed on the device). An id that is not
 * below nMat: -5, nothing is kept and set_inputs has to be called again. Any earlier scale and run are forgotten. -1: a null pointer; idBytes. */
int bfd_thermal_set_inputs(bfd_thermal handle, const float *p, const float *pw, const void *map, int idBytes);

/* The 3 x 3 x 3 median (reflect) of :908-918 merged under class bit `bit` of classOf (uint8 [nMat]), in place on every resident field of `which`
 * (BFD_THERMAL_P or BFD_THERMAL_PW): what bfd_median_filter3d gives with the region mask formed from map and table. -1: a null pointer; bit outside
 * 0 .. 7; which. */
int bfd_thermal_median_region(bfd_thermal handle, const uint8_t *classOf, int bit, int which, float *kernelMs /*may be NULL*/);

/* bfd_loss_survey3d on the resident fields: same arguments from classOf on, same outputs ([nFields], sums [nFields][N3]); the resident water fields
 * are cleared over class bit 1, as waterOut == pw does. brainMask (uint8 [N1][N2][N3], may be NULL) is uploaded where given. -1: a null pointer;
 * rhoWater, cWater; a rho or c; dx2; after the pass, a value that is not finite ("refused data"). */
int bfd_thermal_loss_survey(bfd_thermal handle, const uint8_t *classOf, const uint8_t *brainMask /*may be NULL*/, const double *rho, const double *c,
                            double rhoWater, double cWater, double dx2, float *maxTissue, int64_t *argTissue, float *maxWater, int64_t *argWater,
                            double *eWaterRaw, double *eWater, double *eTissue, float *kernelMs /*may be NULL*/);

/* The pressure ratio of every field. No pass over a volume: p stays unscaled on the device, and the scaled value of a voxel, defined once in
 * csrc/bfd_thermal_study_core.h, is formed wherever it is used (heat source, p_map, its extrema and planes):
 *   mode 0  one field, pAmp * PressureRatio (:960, :1029): (float)((double)p * ratio[0]), the float64 product NumPy >= 2 forms, rounded once
 *   mode 1  InputsBHTE[n] *= PressureRatio[n] (:975-977): the float32 product p * (float)ratio[n]
 * -1: a null pointer; mode; mode 0 with several fields; a ratio that is not finite. */
int bfd_thermal_set_scale(bfd_thermal handle, const double *ratio /*[nFields]*/, int mode);

/* The step loop of bfd_bhte_run_protocol on the resident volumes: cd, cp, qf, initT float32 [nMat]; q = ((s s) qf[m]) from the scaled pressure s.
 * flags bit 0: T0 holds the initial temperature; bit 1: dose0 the initial dose; bit 2: start over; bit 3: the first capture of a run that continues
 * merges into the Tmax held, so that Tmax spans the runs (np.maximum over the chunks of :1094-1098); bit 4 (without bits 0 and 1): start from the
 * temperature and dose of bfd_thermal_set_previous, copied on the device. A run without bit 0 (bit 1) continues from the
 * resident temperature (dose) of the run before; the first run, or one with bit 2, starts from initT[material] (a dose of zero). points
 * [nPoints][nSteps] of pointIndex (C-order linear indices) come back; T, dose, q, Tmax and the dose at the last capture stay. Without captures Tmax
 * is T at the end. nSteps == 0 sets the start state and returns. nFactorMonitoring is accepted and unused: the study keeps no monitored plane.
 * -1: a null pointer (handle, cd, cp, qf); flags; a volume the flags announce; a fresh start without T0 and initT; nSteps; a schedule entry; the
 * point list; a point outside the volume; the capture list. */
int bfd_thermal_run(bfd_thermal handle, const float *cd, const float *cp, const float *qf, const float *initT /*may be NULL*/, int flags,
                    const float *T0 /*may be NULL*/, const float *dose0 /*may be NULL*/, float Tcore, double dt, int nSteps, const int32_t *fieldOfStep,
                    int nFactorMonitoring, int64_t nPoints, const uint32_t *pointIndex, float *points, int nCaptures, const int32_t *captureStep,
                    double *kernelMs /*may be NULL*/);

/* PreviousData's volumes (:948-956), uploaded ONCE: FinalTemp and FinalDose start the first bio-heat call (:972) and the protocol (:1065), TempEndFUS is
 * merged twice (:994, :1108). Three more float32 volumes of device memory, taken here. -1: a null pointer. */
int bfd_thermal_set_previous(bfd_thermal handle, const float *finalTemp, const float *finalDose, const float *tempEndFUS);

/* resident = np.maximum(resident, hostVolume) (:994, :1108) for Tmax, doseAtCapture, T or dose; a NaN on either side wins. hostVolume NULL: the
 * TempEndFUS of bfd_thermal_set_previous (-6 without it). */
int bfd_thermal_merge_max(bfd_thermal handle, int which, const float *hostVolume);

/* bfd_class_extrema3d over resident volumes named in which[nVol] (Tmax, doseAtCapture, T, dose, p_map and, with one field, the unscaled p;
 * 1 <= nVol <= 64), same outputs. */
int bfd_thermal_extrema(bfd_thermal handle, const int *which, int nVol, const uint8_t *classOf /*[nMat]*/, int64_t *count /*[8]*/, float *maxIn,
                        int64_t *argIn, float *maxKey, int64_t *argKey, float *kernelMs /*may be NULL*/);

/* One named result to the host, float32 (dtype 0); q, pw and p come as [nFields] volumes. dtype 1: float64, for p_map of one field in mode 0 alone,
 * (double)p * ratio, the type SaveDict['p_map'] has at :1115. */
int bfd_thermal_get(bfd_thermal handle, int which, void *out, int dtype);
/* [:, j, :] of p_map (float32 [N1][N3]), of the map (uint32 [N1][N3]) or, with one field, of the unscaled p: p_map_central (for one field the
 * caller forms pAmp[:, cy, :] * PressureRatio in float64, as :1116 does) and MaterialMap_central of :1116-1120 */
int bfd_thermal_get_plane(bfd_thermal handle, int which, int64_t j, void *out);

/* Bytes the study has copied host -> device and device -> host since its creation, counted where each copy is issued */
int bfd_thermal_traffic(bfd_thermal handle, int64_t *bytesUp, int64_t *bytesDown);

/* Acoustic study (ABI 7, additive): the volumes of one Step-2 calculation held on one device from their upload to the results the caller asks for.
 * Every stage is the launch sequence of the public entry it names, in device-pointer form, so its results equal that entry's element by element:
 *   bfd_acoustic_set_volumes  labels (uint8 [M1][M2][M3], as stored), the ct index volume (ctBytes 2 or 4) and the air mask (uint8): one upload each
 *   bfd_acoustic_survey       bfd_label_survey3d on the resident labels
 *   bfd_acoustic_assemble     bfd_assemble_material_map3d from `lo` on, without output pointers: map, mapNoCT (with a ct) and airOut (with an air
 *                             mask) stay resident, stats [8] comes back. waterOnly = 1: the map is zeros, formed on the device, and nothing else exists
 *   bfd_acoustic_attach       bfd_set_material_map_device of the resident map on `sim`, then bfd_set_reflector_device where airOut exists
 *   bfd_acoustic_pack         bfd_pack_results of `sim` (all three outputs) into resident volumes of slot 0 (tissue), 1 (water) or 2 (refocus), and
 *                             the resident maps cropped, pasted and flipped the same way (not zeroed at the source plane), the air mask as uint8
 *   bfd_acoustic_get          one packed volume of a slot, or (slot ignored) a whole assembled map, to the host
 *   bfd_acoustic_traffic      bytes the study has copied host -> device and device -> host since its creation, counted where each copy is issued
 * Contract (csrc/bfd_call.h): argument errors are -1 with a text, before a device is looked for, in the order of the entry each stage names (then
 * what the stage adds: waterOnly, slot, which); -3: no device or a bad ordinal; -6: a stage was asked for before the stage it needs, which the text
 * names (set_volumes before survey and assemble, assemble before attach, pack and the whole maps, a run before pack, pack before get), or a volume
 * the study does not hold (no ct, no air mask, a water-only map); -10: a HIP error. Outputs are untouched on a refusal. The sim of attach and pack is
 * a whole domain (k0 = 0) of the assembled map's shape on the study's device, else -1; the shape is compared with the assembled map, so this -1
 * alone follows the -6 of a missing assembly (and precedes the -6 of a missing run). */
typedef struct bfd_acoustic_s *bfd_acoustic;
enum {
    BFD_ACOUSTIC_P_AMP = 0,             /* float32 [O]: pAmp of bfd_pack_results */
    BFD_ACOUSTIC_P_COMPLEX = 1,         /* float32 [O][2] */
    BFD_ACOUSTIC_PEAK = 2,              /* float32 [O] */
    BFD_ACOUSTIC_MATERIAL_MAP = 3,      /* uint32 [O]: the map the sim ran on */
    BFD_ACOUSTIC_MATERIAL_MAP_NOCT = 4, /* uint32 [O]: the raw labels of the domain (with a ct) */
    BFD_ACOUSTIC_AIR_MASK = 5,          /* uint8 [O] (with an air mask) */
    BFD_ACOUSTIC_FULL_MAP = 6,          /* uint32 [N1][N2][N3]: map, mapNoCT, airOut as bfd_assemble_material_map3d writes them */
    BFD_ACOUSTIC_FULL_MAP_NOCT = 7,
    BFD_ACOUSTIC_FULL_AIR = 8
};
int bfd_acoustic_create(int device, int64_t M1, int64_t M2, int64_t M3, int ctBytes, int hasAir, bfd_acoustic *handle);
void bfd_acoustic_destroy(bfd_acoustic handle);           /* NULL is accepted */
int bfd_acoustic_set_volumes(bfd_acoustic handle, const uint8_t *labels, const void *ct, const uint8_t *air);
int bfd_acoustic_survey(bfd_acoustic handle, const int64_t *lo, const int64_t *hi, int flipK, int64_t *hist, int64_t *bounds, int64_t *focal);
int bfd_acoustic_assemble(bfd_acoustic handle, const int64_t *lo, const int64_t *size, const int64_t *padLo, const int64_t *padHi, int flipK,
                          const uint32_t *lut, uint32_t ctOffset, int64_t zWater, int64_t nMaterials, const int64_t *focalIJ, int waterOnly,
                          int64_t *stats);
int bfd_acoustic_attach(bfd_acoustic handle, bfd_sim *sim);
int bfd_acoustic_pack(bfd_acoustic handle, bfd_sim *sim, const bfd_pack_spec *spec, int slot);
int bfd_acoustic_get(bfd_acoustic handle, int which, int slot, void *out);
int bfd_acoustic_traffic(bfd_acoustic handle, int64_t *bytesUp, int64_t *bytesDown);

#ifdef __cplusplus
}
#endif
#endif /* BABELFDTD_H */
