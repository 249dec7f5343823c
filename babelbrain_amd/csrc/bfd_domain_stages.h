// Launch sequences of Step-2 entries in their device-pointer form, for the acoustic study (bfd_acoustic.hip), which chains them on volumes that stay
// on the device. Each is defined beside its kernels and is what the public entry of the same stage runs between its own copies, so a stage has one
// set of kernels and one set of grids: the public entries and the study cannot drift. Host code only. Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/babelfdtd.h"

// --- bfd_domain.hip
// The argument checks bfd_label_survey3d and bfd_assemble_material_map3d make on what follows their volumes, in the header's order (-1 and a text, or
// 0); N: the shape of the assembled map.
int bfd_survey_arguments(const char *who, int64_t M1, int64_t M2, int64_t M3, const int64_t *lo, const int64_t *hi, int flipK);
int bfd_assemble_arguments(const char *who, int64_t M1, int64_t M2, int64_t M3, bool haveCt, const int64_t *lo, const int64_t *size, const int64_t *padLo,
                           const int64_t *padHi, int flipK, const uint32_t *lut, int64_t zWater, int64_t nMaterials, const int64_t *focalIJ, int64_t *N);
// The launch of bfd_label_survey3d on the null stream. dLabels: the volume padded to whole 32-bit words. Before the launch dHist [257] is zero, dBnd [6]
// is {INT_MAX, -1} x 3 and *dFirst is 0xFFFFFFFF. bfd_label_survey_finish turns the three as read back into the entry's outputs.
hipError_t bfd_stage_label_survey(const uint8_t *dLabels, int64_t M1, int64_t M2, int64_t M3, const int64_t *lo, const int64_t *hi, int flipK,
                                  unsigned long long *dHist, int *dBnd, unsigned *dFirst);
void bfd_label_survey_finish(const unsigned long long *h /*[257]*/, const int *bnd /*[6]*/, unsigned first, int64_t *hist, int64_t *bounds, int64_t *focal);
// The launch of bfd_assemble_material_map3d on the null stream (a map of at least one voxel). dCt, dAir, dMapNoCT, dAirOut may be null. Before the
// launch d64 [3] is zero and d32 [5] is {0xFFFFFFFF, 0, 0, 0x7FFFFFFF, 0x7FFFFFFF}; bfd_assemble_finish turns the two as read back into stats [8].
hipError_t bfd_stage_assemble_map(const uint8_t *dLabels, const void *dCt, int ctBytes, const uint8_t *dAir, int64_t M2, int64_t M3, const int64_t *N,
                                  const int64_t *lo, const int64_t *size, const int64_t *padLo, int flipK, const uint32_t *dLut, uint32_t ctOffset, int64_t zWater,
                                  int64_t nMaterials, const int64_t *focalIJ, uint32_t *dMap, uint32_t *dMapNoCT, uint32_t *dAirOut, unsigned long long *d64,
                                  unsigned *d32);
void bfd_assemble_finish(const unsigned long long *c64, const unsigned *c32, int64_t *stats);

// --- bfd_pack.hip
// What bfd_pack_results checks before the device is touched (-1), and what the sim must hold for the outputs wanted (-2); 0 where the pack can run
int bfd_pack_arguments(const char *who, const bfd_sim *sim, const bfd_pack_spec *spec, bool wantAmp, bool wantSensors);
// The launch sequence of bfd_pack_results into device volumes of spec->O voxels (each may be null), on the sim's stream, after the outstanding Pressure
// has been added to the maps
int bfd_stage_pack_results(bfd_sim *sim, const bfd_pack_spec *spec, float *dAmp, float *dComplex /*[..][2]*/, float *dPeak);
// A volume of the sim's shape in C order (k fastest; 4-byte elements) cropped, pasted and flipped as the spec says, without the zeroing at the source
// plane: out [O[0]][O[1]][O[2]] of 4-byte elements (outBytes 4) or of bytes holding the low byte of each element (outBytes 1). On the sim's stream.
hipError_t bfd_stage_pack_map(bfd_sim *sim, const bfd_pack_spec *spec, const uint32_t *dVolume, void *dOut, int outBytes);
