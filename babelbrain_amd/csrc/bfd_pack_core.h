// Result packing (bfd_pack.hip): the index arithmetic between an output voxel and the slab's voxel it shows, and the three scale definitions. Plain
// C++ for host and device, so that the tests compile this file for the host and hold it to the numpy restatement (tests/test_acoustic_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BFD_PACK_HD __host__ __device__ __forceinline__
#else
#define BFD_PACK_HD inline
#endif

// bfd_pack_spec resolved against the slab: keep = extents of the kept region, k0 = the slab's first global plane
struct PackGeom {
    int lo[3], keep[3], O[3], at[3];
    int zSource, k0, flipK;
};
// a dense box of sensors: extents in x and y, first voxel (local k); sensor s of the box is its voxel in ascending x-fastest order
struct PackBox { int bx, by, bz, i0, j0, k0; };

// The slab voxel (i, j, k) that output voxel (a, b, c) shows; false where the output is 0 whatever the results are: outside the pasted region, or
// at or before the source plane
BFD_PACK_HD bool pack_source_voxel(const PackGeom &g, int a, int b, int c, int &i, int &j, int &k)
{
    const int cc = g.flipK ? g.O[2] - 1 - c : c;
    const int u = a - g.at[0], v = b - g.at[1], w = cc - g.at[2];
    if (u < 0 || u >= g.keep[0] || v < 0 || v >= g.keep[1] || w < 0 || w >= g.keep[2]) return false;
    i = g.lo[0] + u; j = g.lo[1] + v; k = g.lo[2] + w;
    return g.k0 + k > g.zSource;
}
// The reverse: linear index of the output voxel that shows slab voxel (i, j, k), -1 where none does
BFD_PACK_HD long pack_output_index(const PackGeom &g, int i, int j, int k)
{
    const int u = i - g.lo[0], v = j - g.lo[1], w = k - g.lo[2];
    if (u < 0 || u >= g.keep[0] || v < 0 || v >= g.keep[1] || w < 0 || w >= g.keep[2] || g.k0 + k <= g.zSource) return -1;
    const int cc = g.at[2] + w, c = g.flipK ? g.O[2] - 1 - cc : cc;
    return ((long)(g.at[0] + u) * g.O[1] + (g.at[1] + v)) * g.O[2] + c;
}
// sensor number of voxel (i, j, k) in a box, -1 outside it
BFD_PACK_HD long pack_box_sensor(const PackBox &B, int i, int j, int k)
{
    const int u = i - B.i0, v = j - B.j0, w = k - B.k0;
    if (u < 0 || u >= B.bx || v < 0 || v >= B.by || w < 0 || w >= B.bz) return -1;
    return ((long)w * B.by + v) * B.bx + u;
}

// The library is built with float32 denormals flushed: a float32 instruction takes a denormal operand as zero, and the float64 -> float32 conversion
// returns zero for a denormal result. numpy on a CPU keeps both, so the scaling below touches float32 values through integer and float64 instructions
// only, which the mode leaves alone.
// A float32 as the float64 of the same value
BFD_PACK_HD double pack_exact_double(float v)
{
    uint32_t u;
    __builtin_memcpy(&u, &v, sizeof u);
    if ((u & 0x7F800000u) != 0u) return (double)v;                  // normal, infinite or NaN
    const double m = (double)(int32_t)(u & 0x007FFFFFu) * 0x1p-149;
    return (u >> 31) ? -m : m;
}
// A float64 rounded to float32, half to even, as the conversion rounds it: below the smallest normal the result is a multiple of 2^-149, formed as an
// integer (2^23 of them are the smallest normal itself, which is what the bit pattern says)
BFD_PACK_HD float pack_round_float(double d)
{
    const double a = d < 0 ? -d : d;
    if (!(a < 0x1p-126)) return (float)d;                           // normal range, infinite or NaN
    const uint32_t u = (uint32_t)__builtin_rint(a * 0x1p149) | (__builtin_signbit(d) ? 0x80000000u : 0u);
    float f;
    __builtin_memcpy(&f, &u, sizeof f);
    return f;
}

// a *= Correction*np.sqrt(2) on a float32 array (BASE:2440): the factor is a float64 scalar, the product is formed in float64 and rounded once
BFD_PACK_HD float pack_scale_amp(float rms, double ampScale) { return pack_round_float(pack_exact_double(rms) * ampScale); }
// c64 *= python float, f32 *= python float (BASE:2517-2520): the factor becomes float32 first, the product is a float32 product. Formed in float64,
// where the product of two float32 is exact, and rounded once: the IEEE float32 product bit for bit
BFD_PACK_HD float pack_scale_f32(float v, float correction) { return pack_round_float(pack_exact_double(v) * pack_exact_double(correction)); }
