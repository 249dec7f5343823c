// Arithmetic of bfd_pseudoct.hip, as host-and-device functions: the kernels call these per voxel, and a plain C++ program can call the same
// functions serially on the CPU to check them (no HIP needed; tests/test_pseudoct_host.py does). Not part of the ABI.
//
// Everything is float64, ONE OPERATION PER ROUNDING, in the order written here (the library is built with -ffp-contract=off, and so must every user
// of this file be). A float32 voxel is widened first, exactly: the widening is done on the bits where the value is a denormal, because the build
// flushes float32 denormals in float32 instructions and numpy does not.
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

#define PC_F32 1
#define PC_F64 3
#define PC_MAX_RANGE 65535.0                           // max - min of bfd_integer_histogram3d: 2^16 - 1, CTZTEProcessing.py:559
#define PC_MAX_INT_BINS 65536
#define PC_MAX_BINS 1024
#define PC_MAX_RANKS 4

BFD_HD double pc_from_bits64(uint64_t b) { double d; __builtin_memcpy(&d, &b, 8); return d; }
BFD_HD uint64_t pc_bits64(double d) { uint64_t b; __builtin_memcpy(&b, &d, 8); return b; }

// the float32 with these bits as a float64, exactly; denormals without a float32 instruction: m * 2^-149
BFD_HD double pc_widen32(uint32_t b)
{
    if (((b >> 23) & 0xFFu) == 0) {
        const double d = (double)(int32_t)(b & 0x7FFFFFu) * 0x1p-149;
        return (b >> 31) ? -d : d;
    }
    float f;
    __builtin_memcpy(&f, &b, 4);
    return (double)f;
}

// the voxel whose bits are `raw` (float32 in the low word, or float64) as float64
template <bool F64>
BFD_HD double pc_value(uint64_t raw) { return F64 ? pc_from_bits64(raw) : pc_widen32((uint32_t)raw); }

// Order-preserving keys: a < b as floats <=> key(a) < key(b) as unsigned (-0.0 below +0.0; NaNs beyond the infinities on either side)
BFD_HD uint32_t pc_key32(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
BFD_HD uint32_t pc_unkey32(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
BFD_HD uint64_t pc_key64(uint64_t bits) { return bits ^ ((bits >> 63) ? ~(uint64_t)0 : (uint64_t)1 << 63); }
BFD_HD uint64_t pc_unkey64(uint64_t key) { return key ^ ((key >> 63) ? (uint64_t)1 << 63 : ~(uint64_t)0); }
#define PC_KEY64_NEG_INF 0x000FFFFFFFFFFFFFull
#define PC_KEY64_POS_INF 0xFFF0000000000000ull

// the key of the voxel's own format (32 significant bits for float32) and the value it stands for
template <bool F64>
BFD_HD uint64_t pc_key(uint64_t raw) { return F64 ? pc_key64(raw) : (uint64_t)pc_key32((uint32_t)raw); }
template <bool F64>
BFD_HD double pc_key_value(uint64_t key) { return F64 ? pc_from_bits64(pc_unkey64(key)) : pc_widen32(pc_unkey32((uint32_t)key)); }

// v > above, or v >= above: false for a NaN
BFD_HD bool pc_selected(double v, double above, bool inclusive) { return inclusive ? v >= above : v > above; }

// astype(int) of a finite value within +-2^62: toward zero, so (-1, 1) is 0
BFD_HD int64_t pc_trunc(double v) { return (int64_t)v; }

// np.histogram's bin of a value first <= a <= last among `bins` equal bins: edges = np.linspace(first, last, bins + 1)
BFD_HD int pc_uniform_bin(double a, double first, double last, int bins, const double *edges)
{
    const double d = a - first;
    const double w = last - first;
    const double f = d / w;
    const double t = f * (double)bins;
    int i = (int)t;
    if (i == bins) i--;
    if (a < edges[i]) i--;
    if (a >= edges[i + 1] && i != bins - 1) i++;
    return i;
}

// The quotient the HU line reads (arrZTE after :577 / :592-593): v / divisor, -0.5 outside the head where there is a head
BFD_HD double pc_quotient(double v, double divisor, bool hasHead, bool inHead) { return hasHead && !inHead ? -0.5 : v / divisor; }

// CTZTEProcessing.py:608-621 for one voxel, in the reference's order of statements
BFD_HD double pc_hu(double q, double slope, double offset, bool skin, bool bone, bool cavity)
{
    double ct = skin ? 42.0 : -1000.0;
    if (bone) {
        const double t = slope * q;
        ct = t + offset;
    }
    if (ct < -1000.0) ct = -1000.0;
    if (ct > 3300.0) ct = -1000.0;
    if (cavity) ct = -1000.0;
    return ct;
}

// np.percentile's position: lo = floor((n - 1) * (q / 100)), hi = min(lo + 1, n - 1), g = (n - 1) * (q / 100) - lo
BFD_HD void pc_quantile_ranks(int64_t n, double q, int64_t *lo, int64_t *hi, double *g)
{
    const double f = q / 100.0;
    const double pos = (double)(n - 1) * f;
    double fl = floor(pos);
    if (fl > (double)(n - 1)) fl = (double)(n - 1);
    if (fl < 0.0) fl = 0.0;
    *lo = (int64_t)fl;
    *hi = *lo + 1 < n ? *lo + 1 : n - 1;
    *g = pos - fl;
}

// numpy's linear interpolation between the two order statistics (function_base._lerp)
BFD_HD double pc_lerp(double A, double B, double g)
{
    const double d = B - A;
    if (g >= 0.5) {
        const double s = 1.0 - g;
        const double t = d * s;
        return B - t;
    }
    const double t = d * g;
    return A + t;
}
