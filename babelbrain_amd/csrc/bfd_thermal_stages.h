// Launch sequences of Step-3 entries in their device-pointer form, for the thermal study (bfd_thermal_study.hip), which chains them on volumes that
// stay on the device. Each is defined beside its kernels and is what the public entry of the same stage runs between its own copies, so a stage has
// one set of kernels and one set of grids: the public entries and the study cannot drift. Host code only. Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The step loop of bhte_run_core (bfd_bhte.hip) on device pointers. The volumes carry the pads bhte_run_core gives them (bfd_bhte_pads); ids of 16
// bits have zeroed pads. N1 is the FASTEST axis here, as in the kernels. rev: the volumes are in the caller's C order (neighbours summed slowest
// axis first).
struct bfd_bhte_device_run {
    int rev, idBytes;                      // idBytes 1 (nMat <= 256) or 2
    int N1, N2, N3, nMat;
    float *T[2];                           // T[0] holds the initial temperature; *cur says which holds the result
    float *dose;
    const float *q;                        // heat increment of field f at q + f * qStride
    size_t qStride;
    const void *mat;
    const float *cd, *cp;
    float Tcore;
    double dt;
    int nSteps;
    const int32_t *fieldOfStep;            // HOST: it steers the launches
    int sliceJ, fm;                        // monitored plane (slice == null: none) sampled every fm steps
    float *slice;
    long nSamples;
    int64_t nPoints;                       // pts == null: no point series
    const unsigned *idx;
    float *pts;                            // [nPoints][nSteps]
    int nCaptures;
    const int32_t *captureStep;            // HOST
    float *Tmax, *doseCap;
    int mergeFirstCapture;                 // 0: the first capture copies T into Tmax; 1: it merges into the Tmax held, like the later ones
};
// pads of a volume of bhte_run_core, in elements, for a fastest axis of N1 cells
void bfd_bhte_pads(int N1, size_t *front, size_t *back);
// Queues the whole run on the null stream between two events and waits for the second. kernelMs may be null.
hipError_t bfd_stage_bhte_run(const bfd_bhte_device_run &r, int *cur, double *kernelMs);

// The passes of bfd_class_extrema3d (bfd_thermal.hip) over nVol device volumes (padded to whole quads of voxels, 16-byte aligned) and a device map
// of idBytes 1, 2 or 4: one launch for every 4 volumes, each between the small copies that start and read its (value, index) words. scratch: what
// bfd_class_extrema_scratch() says, in bytes. pairs [nVol][8], counts [8], first [8] and *flags are HOST words in the kernel's own form, which
// bfd_class_extrema_finish turns into the entry's outputs (return 1: an id beyond the table, 2: a value that is not finite, 0 otherwise: the
// entry's data refusals in their order). bytesUp / bytesDown (may be null) are advanced by the small copies issued.
size_t bfd_class_extrema_scratch(void);
hipError_t bfd_stage_class_extrema(const float *const *dVolumes, int nVol, const void *dMap, int idBytes, int64_t n, const uint8_t *dClassOf, int nMat,
                                   void *scratch, unsigned long long *pairs, unsigned long long *counts, uint32_t *first, uint32_t *flags, float *kernelMs,
                                   int64_t *bytesUp, int64_t *bytesDown);
int bfd_class_extrema_finish(int nVol, const unsigned long long *pairs, const unsigned long long *counts, const uint32_t *first, uint32_t flags,
                             int64_t *count, float *maxIn, int64_t *argIn, float *maxKey, int64_t *argKey);

// The launch of bfd_median_filter3d (bfd_median.hip; dtype 0 uint8, 1 float32) from the volume `in` to the distinct volume `out`; regionMask (may be
// null): filtered where it is non-zero, copied elsewhere. cvalKey: the border value of mode 1 as the kernel's key (unused in mode 0, reflect).
hipError_t bfd_stage_median3d(int dtype, const void *in, void *out, const uint8_t *regionMask, int64_t N1, int64_t N2, int64_t N3, int s1, int s2, int s3,
                              int mode, unsigned cvalKey);

// The launches of bfd_loss_survey3d (bfd_thermal.hip) for one field: the survey and the levels of its fold. rows = N1 N2. pairs [2] start as zeros,
// flags [1] accumulates over the fields; partial and sums: bfd_loss_survey_scratch() words of float64. *result = the row [3][N3] of sums (raw water,
// water, tissue), in one of the two. writeWater: the water field is cleared in place where class bit 1 is set.
void bfd_loss_survey_scratch(int64_t rows, int64_t N3, size_t *partialWords, size_t *sumWords);
hipError_t bfd_stage_loss_survey(const float *p, float *pw, const void *map, int idBytes, const uint8_t *brainMask, const uint8_t *classOf, const double *rho,
                                 const double *c, int nMat, int writeWater, int64_t rows, int64_t N3, double rhoWater, double cWater, double dx2, double *partial,
                                 double *sums, unsigned long long *pairs, uint32_t *flags, const double **result);
