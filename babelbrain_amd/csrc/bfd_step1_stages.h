// Launch sequences of Step-1 entries in their device-pointer form, for entries that chain them without the host in between (bfd_bonerim.hip is the
// first). Each is defined beside its kernels and is what the public entry of the same stage runs between its own copies, so a stage has one set of
// kernels and one set of grids, and the public entry's result and kernelMs mean what they did. Host code only. Not part of the ABI.
//
// Every function queues its kernels on the null stream and returns: it allocates nothing, copies nothing between host and device and waits for
// nothing. Scratch is the caller's. The value returned is hipGetLastError() after the last launch.
//
// The packed masks of the morphology and of the distance transform share one layout: (N3 + 63) / 64 words of 64 bits per row (i, j), bit k & 63 of
// word k >> 6 is voxel k. The morphology does not maintain the bits of a row's last word past N3 in general; after an EROSION with border value 0
// they are 0 (every pass takes them as the border value and ANDs them in), which is what the distance transform asks of its background words.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One erosion (dilate = 0) or dilation (dilate = 1) by an all-ones structure of s[0] x s[1] x s[2] elements, each 1 .. 31, scipy's origin 0: one
// pass per axis with s > 1, along k, then j, then i, between the two packed buffers a (the input) and b. *result = the buffer that holds the result
// (a where no axis has s > 1); the other one holds an intermediate.
hipError_t bfd_stage_box_morphology(uint64_t *a, uint64_t *b, int N1, int N2, int N3, const int *s, int dilate, int borderValue, uint64_t **result);

// Exact squared Euclidean distance of every voxel to the nearest voxel whose bit is set in `background` (padding bits 0, at least one bit set), int32
// into dist2: the row pass and the two envelope passes of bfd_distance_transform_edt3d, without its packing and without its square root. stack: 8 B
// per voxel.
hipError_t bfd_stage_edt_squared(const uint64_t *background, int32_t *dist2, void *stack, int64_t N1, int64_t N2, int64_t N3);

// The three axis passes of bfd_gaussian_filter3d (dtype 1 float32, 3 float64) between the volumes a (the input) and b; an axis with sigma <= 1e-15
// is skipped. radius[a] = gauss_radius(sigma[a], truncate), at most 127. *result = the volume that holds the result (a where every axis is skipped).
hipError_t bfd_stage_gaussian3d(int dtype, void *a, void *b, int64_t N1, int64_t N2, int64_t N3, const double *sigma, const int *radius, int mode,
                                double cval, void **result);
