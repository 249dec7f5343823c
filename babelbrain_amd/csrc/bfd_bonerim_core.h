// Arithmetic of bfd_bonerim.hip, the bone-rim partial-volume correction of BabelBrain/BabelDatasetPreps.py:935-1017 (bMaximizeBoneRim), as
// host-and-device functions: the kernels call these per voxel, and a plain C++ program can call the same functions serially on the CPU to check
// them against numpy (no HIP needed; tests/test_bonerim_host.py does). Not part of the ABI.
//
// ONE OPERATION PER ROUNDING, in the reference's types (the library is built with -ffp-contract=off): float32 where numpy computes in float32,
// float64 where a float64 operand has widened the expression.
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>
#include "bfd_distance_core.h"

// ---- the exact mean of the dense voxels ----
// A dense value is at least RIM_MIN_THRESHOLD = 512, so it is a multiple of 2^-14 (24 significant bits from 2^9 up), and it is below
// RIM_VALUE_LIMIT = 2^17: x 2^14 is an integer below 2^31, and fewer than 2^31 of them sum to less than 2^62. The sum is exact, whatever the order.
#define RIM_MIN_THRESHOLD 512.0f
#define RIM_VALUE_LIMIT 131072.0f
#define RIM_FIXED_ONE 16384.0

// x 2^14 as an integer; x a dense value (512 <= x < 2^17): the product is exact and so is the conversion
BFD_HD uint64_t rim_fixed(float x) { return (uint64_t)(x * 16384.0f); }

// float32(double(S) / (16384.0 * count)); count > 0
BFD_HD float rim_mean(uint64_t S, uint64_t count) { return (float)((double)S / (RIM_FIXED_ONE * (double)count)); }

// ---- per voxel ----
// :951
BFD_HD bool rim_dense(float ct, float threshold) { return ct >= threshold; }

// :980, ndataCT * interior_mask_val: a float32 product with 1 or 0, so a negative value outside the dense mask gives -0.0
BFD_HD float rim_dense_product(float ct, bool dense) { return ct * (dense ? 1.0f : 0.0f); }

// :931-933, the clamp of the bone voxels
BFD_HD float rim_floor(float ct, bool bone, bool haveFloor, float floorValue) { return haveFloor && bone && ct < floorValue ? floorValue : ct; }

// :988, np.where(blur_mask > 1e-6, blur_interior / blur_mask, global_interior_mean) in float32: the comparison is against float32(1e-6), the
// quotient is the correctly rounded float32 quotient (formed in float64 and rounded once: a float64 quotient of two float32 values rounds to the
// same float32 as the float32 division). *global = the voxel took the global mean.
BFD_HD float rim_local_mean(float bi, float bm, float gmean, bool *global)
{
    const bool local = bm > 1e-6f;
    *global = !local;
    return local ? (float)((double)bi / (double)bm) : gmean;
}

// :994-1000 and the store of :1010 for one edge voxel. o: the CT value, lm: its local mean, w: its weight (float64), maxBoost: max_boost.
//     correct = o + w * (lm - o)      the subtraction in float32, the product and the sum in float64
//     delta   = correct - o           float64
//     delta   = min(delta, maxBoost)  np.clip with an upper bound alone
//     correct = o + delta             float64, rounded to float32 (nearest even) by the store
// *clipped = the clip lowered delta.
BFD_HD float rim_blend(float o, float lm, double w, double maxBoost, bool *clipped)
{
    const float diff = lm - o;
    const double prod = w * (double)diff;
    const double c = (double)o + prod;
    double delta = c - (double)o;
    *clipped = delta > maxBoost;
    if (delta > maxBoost) delta = maxBoost;
    const double c2 = (double)o + delta;
    return (float)c2;
}

// the weight of squared distance d2: the table's entry, 0 beyond the table
BFD_HD double rim_weight(const double *table, int64_t length, int64_t d2) { return d2 < length ? table[d2] : 0.0; }

// ---- the weight table (host only) ----
// :974-976, weights = np.exp(-dist / distance_scale) with dist = sqrt of the exact integer squared distance: w[d2] for d2 = 0 .. maxD2, exp as numpy
// takes it on the CPU at hand (gauss_exp of bfd_distance_core.h). The expression is exactly 0 from -dist / scale = -750 on (exp underflows to 0 below
// -745.14), so the table is not formed beyond (750 scale)^2, and trailing zeros are dropped: the reader takes 0 beyond the table (rim_weight).
inline void rim_weight_table(double scale, int64_t maxD2, bool vectorExp, std::vector<double> &w)
{
    const double reach = 750.0 * scale;
    const double cut = reach * reach;
    int64_t last = maxD2;
    if ((double)last > cut) last = (int64_t)cut + 1;
    w.resize((size_t)(last + 1));
    for (int64_t d2 = 0; d2 <= last; d2++) {
        const double dist = sqrt((double)d2);
        w[(size_t)d2] = gauss_exp(-dist / scale, vectorExp);
    }
    while (w.size() > 1 && w.back() == 0.0) w.pop_back();
}
