// Arithmetic and index logic of bfd_distance.hip, as host-and-device functions: the kernels call these per voxel, per line and per tap, and a plain
// C++ program can call the same functions serially on the CPU to check them (no HIP needed; tests/test_distance_host.py does). Not part of the ABI.
//
// Distance transform: integers throughout. Squared distances are int32 (every dimension is at most EDT_MAX_DIM, so 3 (N - 1)^2 < 2^31); the
// intersections of the parabolas of the envelope passes are integer divisions, never floating point: that is what makes the result exact.
// Gaussian filter: float64, ONE OPERATION PER ROUNDING, in the order written here (the library is built with -ffp-contract=off): the order is the one
// scipy.ndimage's correlate1d takes for a symmetric kernel, the weights are formed as scipy.ndimage's _gaussian_kernel1d forms them with numpy.
#pragma once
#include <fenv.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#ifndef BFD_HD
#if defined(__HIPCC__)
#define BFD_HD __host__ __device__ __forceinline__
#else
#define BFD_HD inline
#endif
#endif

// ------------------------------------------------------------ distance transform ------------------------------------------------------------

#define EDT_MAX_DIM 16384
// "no background voxel in this row / on this line so far": compared, never added to
#define EDT_NONE INT32_MAX
// samples of a line that the first scan of an envelope pass loads at a time
#define EDT_AHEAD 8

// 64-bit words of one bit-packed row of n voxels
BFD_HD int64_t edt_row_words(int64_t n) { return (n + 63) / 64; }

// Squared distance from voxel k of a row to the nearest background voxel of the same row, or EDT_NONE. row: W words, bit (k & 63) of word k >> 6 is set
// where voxel k is background; the padding bits of the last word are 0. The nearest set bit at or below k and at or above k come from the leading /
// trailing zero counts of the voxel's own word; where that half of the word is empty the words beyond are walked to the first that is not.
BFD_HD int32_t edt_row_dist2(const uint64_t *row, int64_t W, int64_t k)
{
    const int64_t w = k >> 6;
    const int b = (int)(k & 63);
    int64_t dl = -1, dr = -1;
    const uint64_t lo = row[w] & (~(uint64_t)0 >> (63 - b));      // bits 0 .. b
    if (lo) dl = b - (63 - __builtin_clzll(lo));
    else
        for (int64_t q = w - 1; q >= 0; q--)
            if (row[q]) { dl = k - (q * 64 + 63 - __builtin_clzll(row[q])); break; }
    const uint64_t hi = row[w] >> b;                              // bits b .. 63
    if (hi) dr = __builtin_ctzll(hi);
    else
        for (int64_t q = w + 1; q < W; q++)
            if (row[q]) { dr = q * 64 + __builtin_ctzll(row[q]) - k; break; }
    const int64_t d = dl < 0 ? dr : (dr < 0 ? dl : (dl < dr ? dl : dr));
    return d < 0 ? EDT_NONE : (int32_t)(d * d);
}

// One entry of a line's stack: the site (position s on the line, value g there) and the first position t from which it is the lowest parabola.
// s and t are below EDT_MAX_DIM = 2^14 and share a word.
struct edt_site {
    int32_t st;      // s | t << 16
    int32_t g;
};

// The envelope passes work in int32. Positions are below EDT_MAX_DIM = 2^14, so a squared offset is at most 16383^2; a value that enters the pass
// along j is at most 16383^2 and one that enters the pass along i at most 2 * 16383^2. Every parabola value and every numerator below is therefore at
// most 3 * 16383^2 = 805,208,067 < 2^31: nothing overflows, and a 32-bit division is as exact as a wider one.
// the parabola of site s with value g, at x
BFD_HD int32_t edt_parabola(int32_t x, int32_t s, int32_t g) { return (x - s) * (x - s) + g; }

// the last x at which the parabola of site i (value gi) is not above that of site u > i (value gu): floor of the intersection, by integer division
// (never floating point: that is what makes the transform exact). Called only where parabola i is not above parabola u at some x >= 0, so the
// numerator is not negative and the division is an unsigned one.
BFD_HD int32_t edt_sep(int32_t i, int32_t gi, int32_t u, int32_t gu) { return (int32_t)((uint32_t)(u * u - i * i + gu - gi) / (uint32_t)(2 * (u - i))); }

// One line of an envelope pass (Meijster's two scans), in place: f[u * stride], u = 0 .. m - 1, holds the squared distances of the passes before
// (EDT_NONE: none) and receives min over q of f[q] + (u - q)^2. Sites with EDT_NONE are not sites; a line without any stays EDT_NONE. stack: m entries
// at stack[q * stackStride]. A line of length 1 and a line without sites are ordinary cases.
// The two highest entries of the stack are held in registers (top: s, t, g; below: bs, bt, bg, valid while q >= 1): a pop makes `below` the top at
// once and only then loads the entry under it, which nothing needs before the next pop.
BFD_HD void edt_line(int32_t *f, int64_t stride, int m, edt_site *stack, int64_t stackStride)
{
    int q = -1;
    int32_t s = 0, t = 0, g = 0, bs = 0, bt = 0, bg = 0;
#define EDT_POP()                                                                                          \
    do {                                                                                                   \
        q--;                                                                                               \
        if (q >= 0) {                                                                                      \
            s = bs; t = bt; g = bg;                                                                        \
            if (q >= 1) { const edt_site e_ = stack[(q - 1) * stackStride]; bs = e_.st & 0xFFFF; bt = e_.st >> 16; bg = e_.g; } \
        }                                                                                                  \
    } while (0)
    for (int u0 = 0; u0 < m; u0 += EDT_AHEAD) {
        int32_t ahead[EDT_AHEAD];         // the loads of a batch are issued together: they do not depend on the stack
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < EDT_AHEAD; j++) ahead[j] = u0 + j < m ? f[(int64_t)(u0 + j) * stride] : EDT_NONE;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < EDT_AHEAD; j++) {
            const int32_t gu = ahead[j];
            const int u = u0 + j;
            if (gu == EDT_NONE) continue;
            while (q >= 0 && edt_parabola(t, s, g) > edt_parabola(t, u, gu)) EDT_POP();
            if (q < 0) { q = 0; s = u; t = 0; g = gu; }
            else {
                const int32_t w = 1 + edt_sep(s, g, u, gu);
                if (w >= m) continue;
                q++; bs = s; bt = t; bg = g; s = u; t = w; g = gu;
            }
            edt_site e;
            e.st = s | (t << 16); e.g = g;
            stack[q * stackStride] = e;
        }
    }
    if (q < 0) return;
    for (int u = m - 1; u >= 0; u--) {
        f[u * stride] = edt_parabola(u, s, g);
        if (u == t) EDT_POP();
    }
#undef EDT_POP
}

// -------------------------------------------------------------- Gaussian filter --------------------------------------------------------------

#define GAUSS_MAX_RADIUS 127

// The weights are formed on the host (plain inline functions: host only under hipcc).
// numpy's pairwise sum of n float64 (the inner loop of np.add.reduce): plain below 8, eight partial sums up to 128, halves beyond
inline double gauss_pairwise_sum(const double *a, int n)
{
    if (n < 8) {
        double res = 0.;
        for (int i = 0; i < n; i++) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; j++) r[j] = a[j];
        int i;
        for (i = 8; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; j++) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res += a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return gauss_pairwise_sum(a, n2) + gauss_pairwise_sum(a + n2, n - n2);
}

// exp as numpy takes it. numpy's float64 exp loop is the C library's exp, except on a CPU with the AVX-512 feature set of Skylake-X (F, CD, BW, DQ,
// VL), where numpy's Linux builds call the high-accuracy exp of Intel's short vector math library, which numpy carries in its sources
// (numpy/_core/src/umath/svml, BSD-3-Clause). That routine is within one unit in the last place but not correctly rounded, and scipy's weights are
// what it gives. gauss_exp_svml restates its main path for one element, operation by operation (every operation is IEEE, so one lane of the vector
// code and this scalar code give the same bits): n = x log2(e) in sixteenths by a fused multiply-add onto a shifter, ROUNDED TOWARD ZERO; the
// reduced argument r = x - n ln2 in two fused steps; a degree-5 polynomial in r; 2^(j/16) from a table of 16 with its low part; the scaling by 2^floor(n).
// Held to np.exp on 5.9 million arguments of |x| < 707.7 on such a CPU: no difference. Beyond that the routine takes a slow path that is not restated:
// gauss_exp gives the C library's value there (exp(x) < 5e-308: a weight that small needs truncate above 37).
inline double gauss_exp_svml(double x)
{
    static const uint64_t TH[16] = {0x3ff0000000000000, 0x3ff0b5586cf9890f, 0x3ff172b83c7d517b, 0x3ff2387a6e756238, 0x3ff306fe0a31b715, 0x3ff3dea64c123422,
                                    0x3ff4bfdad5362a27, 0x3ff5ab07dd485429, 0x3ff6a09e667f3bcd, 0x3ff7a11473eb0187, 0x3ff8ace5422aa0db, 0x3ff9c49182a3f090,
                                    0x3ffae89f995ad3ad, 0x3ffc199bdd85529c, 0x3ffd5818dcfba487, 0x3ffea4afa2a490da};      // 2^(j/16)
    static const uint64_t TL[16] = {0x0000000000000000, 0x3c979aa65d837b6d, 0xbc801b15eaa59348, 0x3c968efde3a8a894, 0x3c834d754db0abb6, 0x3c859f48a72a4c6d,
                                    0x3c7690cebb7aafb0, 0x3c9063e1e21c5409, 0xbc93b3efbf5e2228, 0xbc7b32dcb94da51d, 0x3c8db72fc1f0eab4, 0x3c71affc2b91ce27,
                                    0x3c8c1a7792cb3387, 0x3c736eae30af0cb3, 0x3c74a385a63d07a7, 0xbc8ff7128fd391f0};      // its low part, relative
    // log2(e), the shifter 1.5 * 2^48 + 1023, ln2 high and low, the polynomial's coefficients from degree 5 down to 0
    static const uint64_t K[10] = {0x3ff71547652b82fe, 0x42f8000000003ff0, 0x3fe62e42fefa39ef, 0x3c7abc9e3b39803f, 0x3f57411836940c04, 0x3f81101cbbc265c0,
                                   0x3fa55557242d68fe, 0x3fc5555553939732, 0x3fe000000000d008, 0x3fefffffffffff70};
    double k[10], th, tl;
    memcpy(k, K, sizeof k);
    const int mode = fegetround();
    volatile double vx = x;               // read after the rounding mode is set, stored before it is put back
    fesetround(FE_TOWARDZERO);
    volatile double vm = fma(vx, k[0], k[1]);
    fesetround(mode);
    const double m = vm, n = m - k[1];
    uint64_t mb, rb;
    memcpy(&mb, &m, 8);
    memcpy(&th, &TH[mb & 15], 8);
    memcpy(&tl, &TL[mb & 15], 8);
    double r = fma(-n, k[2], x);
    r = fma(-k[3], n, r);
    memcpy(&rb, &r, 8);
    rb &= 0xbfffffffffffffffull;          // the routine's own mask
    memcpy(&r, &rb, 8);
    const double r2 = r * r;
    double p = fma(k[4], r, k[5]);
    const double p1 = fma(k[6], r, k[7]), p0 = fma(k[8], r, k[9]);
    p = fma(r2, p, p1);
    p = fma(r2, p, p0);
    double t = fma(p, r, tl);
    t = fma(th, t, th);
    return ldexp(t, (int)floor(n));
}

// the CPU has what numpy asks for before it takes the vector library's exp
inline bool gauss_numpy_vector_exp(void)
{
#if defined(__x86_64__) && (defined(__GNUC__) || defined(__clang__))
    return __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512cd") && __builtin_cpu_supports("avx512bw") &&
           __builtin_cpu_supports("avx512dq") && __builtin_cpu_supports("avx512vl");
#else
    return false;
#endif
}

inline double gauss_exp(double x, bool vectorExp) { return vectorExp && fabs(x) < 707.7032713517042 ? gauss_exp_svml(x) : exp(x); }

// scipy's radius for sigma and truncate, int(truncate sigma + 0.5), or -1 where it exceeds GAUSS_MAX_RADIUS
inline int gauss_radius(double sigma, double truncate)
{
    const double t = truncate * sigma + 0.5;
    return t < (double)(GAUSS_MAX_RADIUS + 1) ? (int)t : -1;
}

// w[d], d = 0 .. r: exp(-0.5 / sigma^2 * d^2) over the sum of all 2 r + 1 of them: the sum as numpy forms it (pairwise), exp as numpy takes it on
// this CPU (gauss_exp), so that the weights are scipy.ndimage's _gaussian_kernel1d of the same machine, bit for bit
inline void gauss_weights(double sigma, int r, double *w)
{
    double phi[2 * GAUSS_MAX_RADIUS + 1];
    const double sigma2 = sigma * sigma;
    const double c = -0.5 / sigma2;
    const bool vectorExp = gauss_numpy_vector_exp();
    for (int i = 0; i <= 2 * r; i++) {
        const int x = i - r;
        phi[i] = gauss_exp(c * (double)(x * x), vectorExp);
    }
    const double sum = gauss_pairwise_sum(phi, 2 * r + 1);
    for (int d = 0; d <= r; d++) w[d] = phi[r + d] / sum;
}

// Where sample g of a line of n comes from, for any g (as many reflections as it takes); -1: cval. mode 0 reflect (d c b a | a b c d | d c b a),
// 1 constant, 2 nearest, 3 mirror (d c b | a b c d | c b a).
BFD_HD int64_t gauss_edge_index(int64_t g, int64_t n, int mode)
{
    if (g >= 0 && g < n) return g;
    if (mode == 1) return -1;
    if (mode == 2) return g < 0 ? 0 : n - 1;
    if (mode == 0) {
        const int64_t p = 2 * n;
        int64_t q = g % p;
        if (q < 0) q += p;
        return q < n ? q : p - 1 - q;
    }
    if (n == 1) return 0;
    const int64_t p = 2 * n - 2;
    int64_t q = g % p;
    if (q < 0) q += p;
    return q < n ? q : p - q;
}

// One output: the centre term first, then the pairs from d = r down to 1. x(d) gives the extended line's sample at offset d as float64.
template <typename X>
BFD_HD double gauss_sum(X x, const double *w, int r)
{
    double s = x(0) * w[0];
    for (int d = r; d >= 1; d--) s += (x(-d) + x(d)) * w[d];
    return s;
}
