// The per-element arithmetic the thermal study (bfd_thermal_study.hip) adds, in a form a plain C++ compiler accepts too (tests/test_thermal_study_host.py
// compiles it for the host and holds it to numpy). No device memory, no launch: values in, values out.
//
// The scaled pressure of a voxel is defined HERE and nowhere else: the heat source, the field maximum, the metrics and the getters all call ts_scaled.
//   mode 0 (one field; pAmp * PressureRatio of CalculateTemperatureEffects.py:960, :1029): under NumPy >= 2 the product of a float32 array and a
//          float64 scalar is float64, and BHTE takes it as float32: ONE rounding of the exact float64 product, (float)((double)p * ratio)
//   mode 1 (several fields; InputsBHTE[n] *= PressureRatio[n] of :975-977, the ratio already float32): the float32 product p * (float)ratio
// Compile with -ffp-contract=off (csrc/Makefile does); on the device float32 results below 2^-126 flush to zero like everywhere in the library.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TS_HD __host__ __device__ __forceinline__
#else
#define TS_HD static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define TS_FMUL(a, b) __fmul_rn((a), (b))
#define TS_DMUL(a, b) __dmul_rn((a), (b))
#else
#define TS_FMUL(a, b) ((a) * (b))
#define TS_DMUL(a, b) ((a) * (b))
#endif

enum { TS_MODE_DOUBLE_RATIO = 0, TS_MODE_FLOAT_RATIO = 1 };

// the float64 product of mode 0 before its rounding: what SaveDict['p_map'] holds at :1115
TS_HD double ts_scaled64(float p, double ratio) { return TS_DMUL((double)p, ratio); }

TS_HD float ts_scaled(float p, double ratio, int mode)
{
    return mode == TS_MODE_DOUBLE_RATIO ? (float)ts_scaled64(p, ratio) : TS_FMUL(p, (float)ratio);
}

// heat increment of one ON step, q = ((s s) qf[m]): the two float32 products of heat_source_body (bfd_bhte.hip), s the scaled pressure
TS_HD float ts_heat(float s, float qf) { return TS_FMUL(TS_FMUL(s, s), qf); }

// np.maximum of one element: a NaN on either side wins (and stays)
TS_HD float ts_nan_max(float m, float t) { return (t > m || t != t) ? t : m; }

// the element of InputsBHTE.max(axis=0) (:1118): the scaled fields p[f * stride] folded in field order
TS_HD float ts_field_max(const float *p, int64_t stride, int nFields, const double *ratio, int mode)
{
    float m = ts_scaled(p[0], ratio[0], mode);
    for (int f = 1; f < nFields; f++) m = ts_nan_max(m, ts_scaled(p[(int64_t)f * stride], ratio[f], mode));
    return m;
}

// a material id narrowed to the resident width: 0 and *bad set where it does not index the table
TS_HD uint32_t ts_narrow_id(uint32_t id, uint32_t nMat, uint32_t *bad)
{
    if (id < nMat) return id;
    *bad = 1u;
    return 0u;
}

// one voxel of the region byte mask: bit `bit` of the id's class
TS_HD uint8_t ts_region(uint32_t id, const uint8_t *classOf, int bit) { return (uint8_t)((classOf[id] >> bit) & 1u); }
