// Index, window and neighbour logic of bfd_morphology.hip, as host-and-device functions: the kernels call these per word / per voxel, and a
// plain C++ program can call the same functions serially on the CPU to check them (no HIP needed: compile with a C++ compiler).
// Not part of the ABI.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define BFD_HD __host__ __device__ __forceinline__
#else
#define BFD_HD inline
#endif

// ---- bit-packed masks ----
// One bit per voxel along k: bit b of word [(i N2 + j) nW + w] is voxel (i, j, 64 w + b), nW = ceil(N3 / 64). The bits of a row's last word past N3
// are NOT maintained: every reader takes them, like everything else outside the volume, as the border value (morph_word).
struct morph_dims {
    int N1, N2, N3, nW;
    uint64_t tail;          // the bits of a row's last word that are voxels
};

BFD_HD morph_dims morph_make_dims(int N1, int N2, int N3)
{
    morph_dims g;
    g.N1 = N1; g.N2 = N2; g.N3 = N3; g.nW = (N3 + 63) / 64;
    g.tail = (N3 & 63) ? ((uint64_t)1 << (N3 & 63)) - 1 : ~(uint64_t)0;
    return g;
}

// word w of row (i, j) as a pass sees it; fill = 0 or ~0, the border value in every bit
BFD_HD uint64_t morph_word(const uint64_t *bits, const morph_dims &g, int i, int j, int w, uint64_t fill)
{
    if (i < 0 || i >= g.N1 || j < 0 || j >= g.N2 || w < 0 || w >= g.nW) return fill;
    uint64_t v = bits[((long)i * g.N2 + j) * g.nW + w];
    if (w == g.nW - 1) v = (v & g.tail) | (fill & ~g.tail);
    return v;
}

// the 64 voxels k = 64 w + d ... 64 w + d + 63 of a row from its words w - 1, w, w + 1; -63 <= d <= 63
BFD_HD uint64_t morph_shift(uint64_t prev, uint64_t cur, uint64_t next, int d)
{
    if (d == 0) return cur;
    if (d > 0) return (cur >> d) | (next << (64 - d));
    return (cur << (-d)) | (prev >> (64 + d));
}

// taps of one axis of an all-ones structure of size s (scipy, origin 0): out[x] = AND / OR of in[x + d], lo <= d <= hi. Dilation mirrors the window.
BFD_HD void morph_box_taps(int s, bool dilate, int *lo, int *hi)
{
    if (dilate) { *lo = -(s - 1 - s / 2); *hi = s / 2; }
    else { *lo = -(s / 2); *hi = s - 1 - s / 2; }
}

// 1-D pass along k of word w of row (i, j); |lo|, |hi| <= 63
BFD_HD uint64_t morph_pass_k(const uint64_t *bits, const morph_dims &g, int i, int j, int w, int lo, int hi, bool dilate, uint64_t fill)
{
    const uint64_t p = morph_word(bits, g, i, j, w - 1, fill), c = morph_word(bits, g, i, j, w, fill), n = morph_word(bits, g, i, j, w + 1, fill);
    uint64_t acc = dilate ? 0 : ~(uint64_t)0;
    for (int d = lo; d <= hi; d++) {                 // ends: hi - lo + 1 <= 31 taps
        const uint64_t v = morph_shift(p, c, n, d);
        acc = dilate ? (acc | v) : (acc & v);
    }
    return acc;
}

// 1-D pass along i (axis 0) or j (axis 1): whole words
BFD_HD uint64_t morph_pass_ij(const uint64_t *bits, const morph_dims &g, int i, int j, int w, int axis, int lo, int hi, bool dilate, uint64_t fill)
{
    uint64_t acc = dilate ? 0 : ~(uint64_t)0;
    for (int d = lo; d <= hi; d++) {                 // ends: hi - lo + 1 <= 31 taps
        const uint64_t v = axis == 0 ? morph_word(bits, g, i + d, j, w, fill) : morph_word(bits, g, i, j + d, w, fill);
        acc = dilate ? (acc | v) : (acc & v);
    }
    return acc;
}

// General structure up to 7 x 7 x 7: the true elements grouped by (di, dj); bit (dk + 3) of km says that (di, dj, dk) is a tap:
// out[x] = AND / OR of in[x + tap]. Erosion taps are (a - s1/2, b - s2/2, c - s3/2) of every true structure[a][b][c]; dilation taps their negatives.
#define MORPH_GEN_MAX 7
struct morph_taps {
    int n;
    signed char di[MORPH_GEN_MAX * MORPH_GEN_MAX], dj[MORPH_GEN_MAX * MORPH_GEN_MAX];
    unsigned char km[MORPH_GEN_MAX * MORPH_GEN_MAX];
};

// structure: uint8 [s1][s2][s3], every s <= 7. Returns the number of true elements.
inline int morph_make_taps(const uint8_t *structure, int s1, int s2, int s3, bool dilate, morph_taps *t)
{
    int count = 0;
    t->n = 0;
    for (int a = 0; a < s1; a++)
        for (int b = 0; b < s2; b++) {
            unsigned km = 0;
            for (int c = 0; c < s3; c++)
                if (structure[(a * s2 + b) * s3 + c]) {
                    const int dk = dilate ? -(c - s3 / 2) : c - s3 / 2;
                    km |= 1u << (dk + 3);
                    count++;
                }
            if (!km) continue;
            t->di[t->n] = (signed char)(dilate ? -(a - s1 / 2) : a - s1 / 2);
            t->dj[t->n] = (signed char)(dilate ? -(b - s2 / 2) : b - s2 / 2);
            t->km[t->n] = (unsigned char)km;
            t->n++;
        }
    return count;
}

BFD_HD uint64_t morph_general(const uint64_t *bits, const morph_dims &g, int i, int j, int w, const morph_taps &t, bool dilate, uint64_t fill)
{
    uint64_t acc = dilate ? 0 : ~(uint64_t)0;
    for (int q = 0; q < t.n; q++) {                  // ends: n <= 49 rows of at most 7 taps
        const int ri = i + t.di[q], rj = j + t.dj[q];
        const uint64_t p = morph_word(bits, g, ri, rj, w - 1, fill), c = morph_word(bits, g, ri, rj, w, fill), n = morph_word(bits, g, ri, rj, w + 1, fill);
        const unsigned km = t.km[q];
        for (int b = 0; b < 7; b++)
            if ((km >> b) & 1u) {
                const uint64_t v = morph_shift(p, c, n, b - 3);
                acc = dilate ? (acc | v) : (acc & v);
            }
    }
    return acc;
}

// ---- component labelling ----
// Tile of the workgroup-local union-find: LT_I x LT_J x LT_K voxels (i, j, k); local id t = (ii LT_J + jj) LT_K + kk grows with the raster index.
#define LT_I 8
#define LT_J 8
#define LT_K 64
#define LT_VOX (LT_I * LT_J * LT_K)

// The 13 neighbours that precede a voxel in raster order, q = 0..12; false when connectivity c (1, 2, 3: 6, 18, 26 neighbours, scipy's
// generate_binary_structure(3, c)) does not include it. Unions with these alone connect every adjacent pair, each from its later voxel.
BFD_HD bool label_backward_neighbour(int q, int c, int *di, int *dj, int *dk)
{
    if (q < 9) { *di = -1; *dj = q / 3 - 1; *dk = q % 3 - 1; }
    else if (q < 12) { *di = 0; *dj = -1; *dk = q - 10; }
    else { *di = 0; *dj = 0; *dk = -1; }
    const int m = (*di != 0) + (*dj != 0) + (*dk != 0);
    return m <= c;
}
