// Index arithmetic of bfd_domain.hip, as host-and-device functions: the kernels call these per voxel and per ray, and a plain C++ program can call the
// same functions serially on the CPU to check them (no HIP needed; tests/test_domain_host.py does). Not part of the ABI.
//
// The segment of a ray, BabelIntegrationBASE.py:841-844, in float64 with ONE OPERATION PER ROUNDING in the order written here (the library is built
// with -ffp-contract=off, and so must every user of this file be):
//     mid = count // 2,  l_half = fl(count * center_region)
//     beg = max(0, int(rint(fl(mid - fl(l_half / 2)))))                  half to even, as np.round
//     end = min(count - 1, 1 + int(rint(fl(mid + fl(l_half / 2)))))
#pragma once
#include <math.h>
#include <stdint.h>
#ifndef BFD_HD
#if defined(__HIPCC__)
#define BFD_HD __host__ __device__ __forceinline__
#else
#define BFD_HD inline
#endif
#endif

// bit 31 of a LUT entry of bfd_assemble_material_map3d: the raw label is bone, the map takes ct + ctOffset there
#define DM_LUT_BONE 0x80000000u
// ray states of bfd_sdr_rays3d
#define DM_RAY_FEW 0
#define DM_RAY_COUNTED 1
#define DM_RAY_NOT_POSITIVE 2
#define DM_RAY_EMPTY_CENTRE 3
#define DM_RAY_BAD_INDEX 4

// the index of the last axis at which driver index k is stored
BFD_HD int64_t dm_source_k(int64_t k, int64_t M3, int flipK) { return flipK ? M3 - 1 - k : k; }

// a double that is a whole number, as an int within 0 .. limit (what lies outside is cut to the nearer end: the callers clamp to that range anyway)
BFD_HD int dm_int_within(double x, int limit) { return x <= 0.0 ? 0 : (x >= (double)limit ? limit : (int)x); }

// The ranks (among the `count` >= 1 skull voxels of a ray) of the two voxels between which the centre minimum is taken; center_region >= 0.
// The centre is empty where *beg >= *end.
BFD_HD void dm_segment(int count, double center_region, int *beg, int *end)
{
    const double mid = (double)(count / 2);
    const double l_half = (double)count * center_region;
    const double h = l_half / 2.0;
    const double b = rint(mid - h);
    const double e = rint(mid + h);
    *beg = dm_int_within(b, count);
    const int e1 = dm_int_within(e, count - 1) + 1;              // e >= 0 here; cut before the + 1, so that count = INT_MAX does not overflow
    *end = e1 < count - 1 ? e1 : count - 1;
}
