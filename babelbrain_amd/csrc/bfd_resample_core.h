// Index, weight and recursion arithmetic of bfd_resample.hip, as host-and-device functions: the kernels call these per voxel / per line, and a
// plain C++ program can call the same functions serially on the CPU to check them (no HIP needed: compile with a C++ compiler).
// Everything is float64 and follows scipy.ndimage (ni_interpolation.c, ni_splines.c) operation by operation where the order of the
// operations is scipy's to choose; the one deliberate difference is the bounded horizon of the causal start value (RS_HORIZON). Not part of the ABI.
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

#define RS_CONSTANT 0
#define RS_NEAREST 1
#define RS_MIRROR 2
#define RS_NPAD 12          // scipy's _prepad_for_spline_filter: edge-replicated samples per side before the prefilter of 'nearest'
#define RS_HORIZON 64       // terms of the causal start sum; |pole|^64 < 3e-37 (order 3), 1e-49 (order 2)

// ---- prefilter: one pole per order (2: sqrt(8) - 3, 3: sqrt(3) - 2), the host computes pole, gain and pole^n ----
struct rs_filter {
    double z;               // the pole
    double gain;            // (1 - z)(1 - 1/z), applied to every sample as it is first read
    double zn;              // mirror: z^(n-1); reflect: z^n  (n: length of the line)
    int reflect;            // 0: mirror boundary (modes constant and mirror); 1: reflect (mode nearest, whose lines are padded first)
};

BFD_HD double rs_pole(int order) { return order == 2 ? sqrt(8.0) - 3.0 : sqrt(3.0) - 2.0; }

inline rs_filter rs_make_filter(int order, long n, int mode)
{
    rs_filter f;
    f.z = rs_pole(order);
    f.gain = (1.0 - f.z) * (1.0 - 1.0 / f.z);
    f.reflect = mode == RS_NEAREST;
    f.zn = pow(f.z, (double)(f.reflect ? n : n - 1));
    return f;
}

// c+[0] of a line of n >= 2 raw samples c[0], c[s], ...: scipy's _init_causal_mirror / _init_causal_reflect with the sum cut after RS_HORIZON
// terms from either end (scipy runs over the whole line; the terms left out are below 3e-37 of the line's largest sample).
BFD_HD double rs_causal_init(const double *c, long n, long s, const rs_filter &f)
{
    const double g = f.gain, z = f.z, zn = f.zn;
    double zi = z;
    if (!f.reflect) {
        const long m = n - 1 < RS_HORIZON + 1 ? n - 1 : RS_HORIZON + 1;
        double c0 = g * c[0] + zn * (g * c[(n - 1) * s]);
        for (long i = 1; i < m; i++) {                       // ends: m <= RS_HORIZON + 1
            c0 += zi * (g * c[i * s] + zn * (g * c[(n - 1 - i) * s]));
            zi *= z;
        }
        return c0 / (1.0 - zn * zn);
    }
    const long m = n < RS_HORIZON + 1 ? n : RS_HORIZON + 1;
    const double first = g * c[0];
    double c0 = first + zn * (g * c[(n - 1) * s]);
    for (long i = 1; i < m; i++) {                           // ends: m <= RS_HORIZON + 1
        // scipy sums in place in c[0], so the last term of a short line (i = n - 1) reads the running sum where the formula has c[0]
        c0 += zi * (g * c[i * s] + zn * (i == n - 1 ? c0 : g * c[(n - 1 - i) * s]));
        zi *= z;
    }
    c0 *= z / (1.0 - zn * zn);
    return c0 + first;
}

// c-[n-1] from the last two causal values
BFD_HD double rs_anticausal_init(double cm2 /*c+[n-2]*/, double cm1 /*c+[n-1]*/, const rs_filter &f)
{
    if (!f.reflect) return (f.z * cm2 + cm1) * f.z / (f.z * f.z - 1.0);
    return cm1 * (f.z / (f.z - 1.0));
}

// the whole filter of one line in place: n >= 2 samples, s elements apart
BFD_HD void rs_filter_line(double *c, long n, long s, const rs_filter &f)
{
    double prev = rs_causal_init(c, n, s, f), prev2 = 0.0;
    c[0] = prev;
    for (long i = 1; i < n; i++) {                           // ends: n is the line's length
        const double v = f.gain * c[i * s] + f.z * prev;
        c[i * s] = v;
        prev2 = prev; prev = v;
    }
    double next = rs_anticausal_init(prev2, prev, f);
    c[(n - 1) * s] = next;
    for (long i = n - 2; i >= 0; i--) {
        const double v = f.z * (next - c[i * s]);
        c[i * s] = v;
        next = v;
    }
}

// ---- coordinates ----
// scipy's map_coordinate for the three modes. constant: -1 outside [0, len - 1]; mirror: (d c b | a b c d | c b a), any distance. nearest: scipy
// leaves the coordinate as it is and clamps the taps (rs_tap_index), so beyond the last sample the result runs into the edge COEFFICIENT; here
// the coordinate is also held within 4 samples of the volume, where all taps are the edge one already, so that it fits an integer.
BFD_HD double rs_map_coordinate(double in, long len, int mode)
{
    if (mode == RS_CONSTANT) return (in < 0.0 || in > (double)(len - 1)) ? -1.0 : in;
    if (mode == RS_NEAREST) return in < -4.0 ? -4.0 : (in > (double)(len + 3) ? (double)(len + 3) : in);
    if (in < 0.0) {
        if (len <= 1) return 0.0;
        const long sz2 = 2 * len - 2;
        in = (double)sz2 * (double)(long)(-in / (double)sz2) + in;
        return in <= (double)(1 - len) ? in + (double)sz2 : -in;
    }
    if (in > (double)(len - 1)) {
        if (len <= 1) return 0.0;
        const long sz2 = 2 * len - 2;
        in -= (double)sz2 * (double)(long)(in / (double)sz2);
        if (in >= (double)len) in = (double)sz2 - in;
    }
    return in;
}

// a tap's index: clamped for nearest, mirrored (any distance) for constant and mirror
BFD_HD long rs_tap_index(long idx, long len, int mode)
{
    if (mode == RS_NEAREST) return idx < 0 ? 0 : (idx > len - 1 ? len - 1 : idx);
    if (len <= 1) return 0;
    const long sz2 = 2 * len - 2;
    if (idx < 0) {
        idx = sz2 * (-idx / sz2) + idx;
        return idx <= 1 - len ? idx + sz2 : -idx;
    }
    if (idx > len - 1) {
        idx -= sz2 * (idx / sz2);
        if (idx >= len) idx = sz2 - idx;
    }
    return idx;
}

// first tap of a mapped coordinate
BFD_HD long rs_first_tap(double cc, int order)
{
    return (long)floor((order & 1) ? cc : cc + 0.5) - order / 2;
}

// the order + 1 B-spline weights of the taps rs_first_tap(cc) ...; orders 1, 2, 3 (order 0 has the single weight 1)
BFD_HD void rs_weights(double cc, int order, double *w)
{
    if (order == 1) {
        const double x = cc - floor(cc);
        w[0] = 1.0 - x; w[1] = x;
    } else if (order == 2) {
        const double x = cc - floor(cc + 0.5);           // -0.5 <= x < 0.5, distance to the middle tap
        const double y = 0.5 - x;
        w[0] = 0.5 * y * y;
        w[1] = 0.75 - x * x;
        w[2] = 1.0 - w[0] - w[1];
    } else if (order == 3) {
        const double x = cc - floor(cc), z = 1.0 - x;
        w[0] = z * z * z / 6.0;
        w[1] = (x * x * (x - 2.0) * 3.0 + 4.0) / 6.0;
        w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
        w[3] = 1.0 - w[0] - w[1] - w[2];
    } else {
        w[0] = 1.0;
    }
}

// ---- the one rounding, at the store: scipy's conversion (round half away from zero, saturating) ----
BFD_HD void rs_store(double t, float *o) { *o = (float)t; }
BFD_HD void rs_store(double t, double *o) { *o = t; }
BFD_HD void rs_store(double t, int16_t *o)
{
    t = t > 0.0 ? t + 0.5 : t - 0.5;
    if (!(t > -32768.0)) t = -32768.0;                  // NaN goes here as well
    if (t > 32767.0) t = 32767.0;
    *o = (int16_t)t;
}
BFD_HD void rs_store(double t, uint8_t *o)
{
    t = t > 0.0 ? t + 0.5 : 0.0;
    if (t > 255.0) t = 255.0;
    *o = (uint8_t)t;
}

// ---- one output voxel ----
struct rs_geom {
    long I[3];              // the coefficient volume (padded by npad per side where the prefilter of 'nearest' ran)
    long O[3];              // the output
    double m[12];           // row a: coordinate a = m[4a+3] + i m[4a] + j m[4a+1] + k m[4a+2], summed in this order (scipy's)
    int mode, npad;
    double cval;
};

// The taps of output voxel (i, j, k): first raw tap per axis (before the boundary rule), the mapped indices and the weights.
template <int ORDER>
struct rs_taps {
    long start[3];
    long idx[3][ORDER + 1];
    double w[3][ORDER + 1];
};

// false: the voxel lies outside (mode constant) and takes cval
template <int ORDER>
BFD_HD bool rs_make_taps(const rs_geom &g, long i, long j, long k, rs_taps<ORDER> &t)
{
    for (int a = 0; a < 3; a++) {
        double cc = g.m[4 * a + 3];
        cc += (double)i * g.m[4 * a];
        cc += (double)j * g.m[4 * a + 1];
        cc += (double)k * g.m[4 * a + 2];
        cc = rs_map_coordinate(cc + (double)g.npad, g.I[a], g.mode);
        if (g.mode == RS_CONSTANT && !(cc > -1.0)) return false;
        t.start[a] = rs_first_tap(cc, ORDER);
        for (int q = 0; q <= ORDER; q++) t.idx[a][q] = rs_tap_index(t.start[a] + q, g.I[a], g.mode);
        rs_weights(cc, ORDER, t.w[a]);
    }
    return true;
}

// Taps are multiplied by their three weights one after the other and summed in raster order, as scipy does. fetch(a, b, c): coefficient of tap
// (a, b, c) as float64, from wherever the caller keeps it; the arithmetic does not depend on that.
template <int ORDER, typename F>
BFD_HD double rs_sum(const rs_taps<ORDER> &t, F fetch)
{
    double sum = 0.0;
    for (int a = 0; a <= ORDER; a++)
        for (int b = 0; b <= ORDER; b++)
            for (int c = 0; c <= ORDER; c++) {
                double v = fetch(a, b, c);
                if (ORDER > 0) { v *= t.w[0][a]; v *= t.w[1][b]; v *= t.w[2][c]; }
                sum += v;
            }
    return sum;
}

// The value of output voxel (i, j, k) before the rounding to the output's dtype. coef: [I0][I1][I2] in C order; for ORDER < 2 and with
// prefilter off it is the input itself.
template <typename TIn, int ORDER>
BFD_HD double rs_voxel(const TIn *coef, const rs_geom &g, long i, long j, long k)
{
    rs_taps<ORDER> t;
    if (!rs_make_taps<ORDER>(g, i, j, k, t)) return g.cval;
    const long I1 = g.I[1], I2 = g.I[2];
    return rs_sum<ORDER>(t, [&](int a, int b, int c) { return (double)coef[(t.idx[0][a] * I1 + t.idx[1][b]) * I2 + t.idx[2][c]]; });
}

// ---- the source box of an output tile (order 3) ----
// Raw tap indices [lo, lo + n) per axis that the voxels i0 <= i <= i1, ... of a tile can read: the coordinate is affine, so each of its three
// terms is extreme at an end of the tile; the map of the mode is applied to the two ends where it is monotone. false: no box (mirror mode
// with coordinates outside [0, len - 1], where the fold is not monotone, or a tile that lies outside under mode constant).
struct rs_box { long lo[3], n[3]; };

BFD_HD bool rs_tile_box(const rs_geom &g, const long lo[3], const long hi[3], rs_box &b)
{
    for (int a = 0; a < 3; a++) {
        double cmin = g.m[4 * a + 3] + (double)g.npad, cmax = cmin;
        for (int d = 0; d < 3; d++) {
            const double p = (double)lo[d] * g.m[4 * a + d], q = (double)hi[d] * g.m[4 * a + d];
            cmin += p < q ? p : q; cmax += p < q ? q : p;
        }
        const double slack = 1e-9 * (1.0 + fabs(cmin) + fabs(cmax));      // the voxels' own sums round differently
        cmin -= slack; cmax += slack;
        const double last = (double)(g.I[a] - 1);
        if (g.mode == RS_MIRROR) {
            if (cmin < 0.0 || cmax > last) return false;
        } else if (g.mode == RS_CONSTANT) {
            if (cmax < 0.0 || cmin > last) return false;
            cmin = cmin < 0.0 ? 0.0 : cmin; cmax = cmax > last ? last : cmax;
        } else {
            cmin = rs_map_coordinate(cmin, g.I[a], RS_NEAREST); cmax = rs_map_coordinate(cmax, g.I[a], RS_NEAREST);
        }
        b.lo[a] = (long)floor(cmin) - 1;
        b.n[a] = (long)floor(cmax) + 2 - b.lo[a] + 1;
    }
    return true;
}
