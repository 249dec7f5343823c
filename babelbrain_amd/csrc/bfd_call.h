// The host side of a Step-1 device call, shared by bfd_median.hip, bfd_morphology.hip, bfd_resample.hip, bfd_voxelize.hip, bfd_distance.hip, bfd_tissue.hip, bfd_domain.hip, bfd_pseudoct.hip, bfd_bonerim.hip, bfd_thermal.hip, bfd_thermal_study.hip and bfd_acoustic.hip (and by no other
// source: the solver's translation units do not see this file). Host code only.
//
// The contract of the stand-alone device calls (bfd_median_filter3d, bfd_binary_morphology3d, bfd_label3d, bfd_affine_transform3d, bfd_spline_filter3d,
// bfd_voxelize_mesh, bfd_voxel_points, bfd_map_values3d, bfd_distance_transform_edt3d, bfd_gaussian_filter3d, bfd_voxel_scatter3d,
// bfd_voxelize_scatter3d, bfd_paint_components3d, bfd_quantize_values3d, bfd_clear_beyond_bone3d,
// bfd_label_survey3d, bfd_assemble_material_map3d, bfd_sdr_rays3d, bfd_integer_histogram3d, bfd_order_statistics3d, bfd_uniform_histogram3d,
// bfd_pseudo_ct_candidates3d, bfd_pseudo_ct_convert3d, bfd_select_component3d, bfd_bone_rim_correct3d,
// bfd_class_extrema3d, bfd_loss_survey3d). Every entry takes these steps in this order:
//    1. argument errors: -1 and a text, each before a device is looked for, in the entry's own order
//    2. pick_device: -3 where no device is visible or the ordinal is out of range
//    3. kernelMs zeroed (after the device pick)
//    4. an empty problem returns 0 here, after the device pick
//    5. temporaries (DevTemp; the scan's scratch is sized here, outside the timed section)
//    6. host-to-device copies
//    7. Events::record(0)
//    8. the kernels, on the null stream like everything else
//    9. Events::record and Events::sync
//   10. Events::elapsed into kernelMs: it brackets the kernels (and the hipMemsetAsync calls of bfd_voxelize_mesh and the two scatter entries), never a copy between host and
//       device; bfd_label3d, bfd_paint_components3d, bfd_select_component3d, bfd_quantize_values3d, bfd_integer_histogram3d, bfd_order_statistics3d,
//       bfd_pseudo_ct_candidates3d and bfd_bone_rim_correct3d report the sum of their timed sections (the host reads the number of components, the keys
//       of a range or of a maximum, the digit counts of a radix pass, or the counts and the largest squared distance of the bone rim between them), bfd_affine_transform3d prefilter and interpolation separately
//   11. device-to-host copies
//   12. the first hipError_t of steps 5-11 ends the call (BFD_STEP): "<entry>: <hipGetErrorString>" and -10; no later step runs
// bfd_quantize_values3d refuses data as well (-1: an empty mask, a value that is not finite, a range of zero, a step below 2^-126): after its
// first reduction, with kernelMs zeroed and nothing else written. So do bfd_integer_histogram3d (an empty volume, a value that is not finite, a
// range over 65535), bfd_order_statistics3d (nothing selected, a rank beyond the count), bfd_uniform_histogram3d (a selected value that is not
// finite), bfd_pseudo_ct_candidates3d (an empty volume, a quotient that is not finite) and bfd_bone_rim_correct3d (an empty volume, a value that is not
// finite, a dense value at or above 2^17, no dense voxel, no interior voxel), and bfd_class_extrema3d and bfd_loss_survey3d (an id that is not below
// nMat, a value that is not finite; their kernelMs is the sum over the launches, one for every 4 volumes or for every field); include/babelfdtd.h lists
// each in its order.
// On any other refusal (-1, -3) the outputs and kernelMs are untouched. Everything a call holds on the device, events included, is released on every way
// out: the next call of the process starts from nothing.
#pragma once
#include "bfd_internal.h"

// BFD_HIP with the entry's name in front of the message, as the argument errors have it: needs `who` in scope
#define BFD_STEP(call)                                                                             \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            bfd_set_error(std::string(who) + ": " + hipGetErrorString(e_));                        \
            return -10;                                                                            \
        }                                                                                          \
    } while (0)

static inline int pick_device(const char *who, int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) BFD_FAIL(-3, std::string(who) + ": no HIP device available (no CPU fallback)");
    if (device < 0 || device >= ndev) BFD_FAIL(-3, std::string(who) + ": device ordinal out of range");
    BFD_HIP(hipSetDevice(device));
    return 0;
}

// the two byte ranges share a byte
static inline bool overlap(const void *p, size_t pb, const void *q, size_t qb)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qb && b < a + pb;
}

// fewer than 2^31 voxels; the product is formed without overflow: each factor is checked against what is left of the limit
static inline bool volume_fits(int64_t N1, int64_t N2, int64_t N3)
{
    const int64_t LIMIT = (int64_t)1 << 31;
    return !(N1 >= LIMIT || N2 >= LIMIT || N3 >= LIMIT || (N2 && N1 > (LIMIT - 1) / N2) || (N3 && N1 * N2 > (LIMIT - 1) / N3));
}

// workgroups of a launch whose kernel takes what lies beyond cap * perBlock items in a grid-stride loop; at least one. The cap belongs to the
// call site: the grids are the ones each kernel was measured with.
static inline unsigned blocks_for(int64_t items, int perBlock, int64_t cap)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + perBlock - 1) / perBlock, cap));
}

// The events around the timed sections of a call, on the null stream: two, or three where two sections are reported separately.
struct Events {
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
    hipError_t create(int count = 2)
    {
        hipError_t e = hipSuccess;
        for (int q = 0; q < count && e == hipSuccess; q++) e = hipEventCreate(&ev[q]);
        return e;
    }
    hipError_t record(int q) { return hipEventRecord(ev[q], 0); }
    hipError_t sync(int q) { return hipEventSynchronize(ev[q]); }
    // milliseconds between two recorded events, the later one waited for; ms == null (the caller did not ask): nothing
    hipError_t elapsed(float *ms, int from, int to) { return ms ? hipEventElapsedTime(ms, ev[from], ev[to]) : hipSuccess; }
};
