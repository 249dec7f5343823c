// Arithmetic of bfd_thermal.hip, as host-and-device functions: the kernels call these per voxel, and a plain C++ program can call the same
// functions serially on the CPU to check them (no HIP needed; tests/test_thermal_host.py does). Not part of the ABI.
//
// ONE OPERATION PER ROUNDING, in the order written here (the library is built with -ffp-contract=off, and so must every user of this file be).
// The build flushes float32 denormals in float32 instructions and numpy does not, so no float32 instruction touches a voxel: a float32 value is
// carried as the float64 that equals it, float32 roundings are made on float64 values (th_round32), and comparisons are made on integer keys.
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

#define TH_CLASSES 8
#define TH_MAX_MATERIALS 65536

BFD_HD uint32_t th_bits32(float f) { uint32_t b; __builtin_memcpy(&b, &f, 4); return b; }
BFD_HD float th_from_bits32(uint32_t b) { float f; __builtin_memcpy(&f, &b, 4); return f; }

BFD_HD bool th_finite(uint32_t bits) { return ((bits >> 23) & 0xFFu) != 0xFFu; }

// the float32 with these bits as a float64, exactly; denormals without a float32 instruction: m * 2^-149
BFD_HD double th_widen32(uint32_t b)
{
    if (((b >> 23) & 0xFFu) == 0) {
        const double d = (double)(int32_t)(b & 0x7FFFFFu) * 0x1p-149;
        return (b >> 31) ? -d : d;
    }
    return (double)th_from_bits32(b);
}

// the float32 nearest to d >= 0 (ties to even), as a float64. Below 2^-126 the float32 grid is the multiples of 2^-149: adding and taking away
// 1.5 * 2^-97, whose last place is 2^-149 and whose significand is even, rounds to that grid in float64 arithmetic.
BFD_HD double th_round32(double d)
{
    if (d < 0x1p-126) return (d + 0x1.8p-97) - 0x1.8p-97;
    return (double)(float)d;
}

// (x * x) / 2.0f as numpy forms it in float32: the product of two float32 is exact in float64, so rounding it once is the float32 product; the
// halving is exact in float64 and rounds again where the half is a float32 denormal
BFD_HD double th_half_square(uint32_t xbits)
{
    const double x = th_widen32(xbits);
    const double sq = th_round32(x * x);
    return th_round32(sq * 0.5);
}

// One term of a plane energy: (((double)(float)((x * x) / 2.0f) / R) / C) * dx2, each of the three float64 operations rounded once
BFD_HD double th_term(uint32_t xbits, double R, double C, double dx2)
{
    const double h = th_half_square(xbits);
    const double a = h / R;
    const double b = a / C;
    return b * dx2;
}

// Order-preserving key of a float32 that is not a NaN: a < b as floats <=> key(a) < key(b) as signed integers, and -0 has the key of +0, so equal
// keys are IEEE-equal values. Finite values have keys inside +-0x7F7FFFFF.
BFD_HD int32_t th_key(uint32_t bits) { return (bits >> 31) ? -(int32_t)(bits & 0x7FFFFFFFu) : (int32_t)bits; }
BFD_HD float th_key_value(int32_t key) { return th_from_bits32(key < 0 ? (0x80000000u | (uint32_t)(-key)) : (uint32_t)key); }

// the key of x * Sel.astype(np.float32) for finite x: x inside the class, +-0 outside
BFD_HD int32_t th_masked_key(uint32_t bits, bool in) { return in ? th_key(bits) : 0; }

// A (value, index) pair as one unsigned word whose order is: the larger value first, among equal values (-0 == +0) the lower index. index < 2^31.
// 0 is below every pair: "nothing yet".
#define TH_NO_PAIR 0ull
BFD_HD uint64_t th_pair(int32_t key, uint32_t index) { return ((uint64_t)((uint32_t)key + 0x80000000u) << 32) | (uint64_t)(0xFFFFFFFFu - index); }
BFD_HD int32_t th_pair_key(uint64_t pair) { return (int32_t)((uint32_t)(pair >> 32) - 0x80000000u); }
BFD_HD int64_t th_pair_index(uint64_t pair) { return pair == TH_NO_PAIR ? -1 : (int64_t)(0xFFFFFFFFu - (uint32_t)pair); }
BFD_HD uint64_t th_pair_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// np.argmax(x * Sel.astype(np.float32)) from the class's own maximum and the first voxel outside the class (firstOut, or -1 where every voxel is
// inside): every outside voxel has the key 0, so the first of them stands for all.
BFD_HD uint64_t th_keyed_pair(uint64_t inPair, int64_t firstOut)
{
    return firstOut < 0 ? inPair : th_pair_max(inPair, th_pair(0, (uint32_t)firstOut));
}
