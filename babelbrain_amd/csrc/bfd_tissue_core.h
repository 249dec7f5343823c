// Arithmetic of bfd_tissue.hip's quantisation, as host-and-device functions: the kernels call these per voxel and per chunk of levels, and a plain C++
// program can call the same functions serially on the CPU to check them (no HIP needed; tests/test_tissue_host.py does). Not part of the ABI.
//
// All float32, ONE OPERATION PER ROUNDING, in the order written here (the library is built with -ffp-contract=off, and so must every user of this
// file be): BabelDatasetPreps.py:1019-1027 as numpy evaluates it,
//     A = mx - mn,  M = 2^bits - 1,  s = fl(M / A),  r = fl(A / M)
//     level(x) = rint(fl(s * fl(x - mn)))           half to even, as np.round
//     v(l)     = fl(fl(r * l) + mn)
// v is non-decreasing in l, so the distinct values of a set of levels are the v(l) of the set in ascending l with equal neighbours merged.
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

#define TQ_MAX_BITS 16
// levels a chunk of the table builder covers: two words of the presence bitmap
#define TQ_CHUNK 64

struct tq_params {
    float mn, s, r;
    int M;
};

BFD_HD tq_params tq_make(float mn, float mx, int bits)
{
    tq_params p;
    const float A = mx - mn;
    p.M = (1 << bits) - 1;
    p.mn = mn;
    p.s = (float)p.M / A;
    p.r = A / (float)p.M;
    return p;
}

// 0 .. M for every x in [mn, mx]; the clamp only keeps an x outside that range (there is none under the mask) inside the bitmap and the rank table
BFD_HD int tq_level(const tq_params &p, float x)
{
    const float d = x - p.mn;
    const float t = p.s * d;
    const float l = rintf(t);
    return l >= (float)p.M ? p.M : (l > 0.f ? (int)l : 0);
}

BFD_HD float tq_value(const tq_params &p, int l)
{
    const float t = p.r * (float)l;
    return t + p.mn;
}

// Presence bitmap: bit (l & 31) of word l >> 5 is set where level l occurs; at least one chunk long.
BFD_HD int tq_presence_words(int bits) { return (1 << bits) < TQ_CHUNK ? TQ_CHUNK / 32 : (1 << bits) / 32; }
BFD_HD int tq_chunks(int bits) { return tq_presence_words(bits) / (TQ_CHUNK / 32); }

// the highest level of chunk c that occurs, or -1
BFD_HD int tq_chunk_last(const uint32_t *presence, int c)
{
    const uint32_t lo = presence[2 * c], hi = presence[2 * c + 1];
    if (hi) return c * TQ_CHUNK + 63 - __builtin_clz(hi);
    if (lo) return c * TQ_CHUNK + 31 - __builtin_clz(lo);
    return -1;
}

// The levels of chunk c that occur, ascending. prev: the highest occurring level below the chunk (-1: none). A level opens a new table row where its
// value differs from that of the occurring level before it. Returns the number of rows the chunk opens; with table != NULL it also writes them from
// row `base` on and writes rank[l] = row of v(l) for every occurring level l of the chunk (base = rows opened below the chunk).
BFD_HD int tq_chunk_rows(const tq_params &p, const uint32_t *presence, int c, int prev, int base, float *table, uint16_t *rank)
{
    int rows = 0;
    bool have = prev >= 0;
    float last = have ? tq_value(p, prev) : 0.f;
    for (int w = 0; w < 2; w++) {
        uint32_t bits = presence[2 * c + w];
        while (bits) {                                // ends: every round clears the lowest set bit
            const int l = c * TQ_CHUNK + 32 * w + __builtin_ctz(bits);
            bits &= bits - 1;
            const float v = tq_value(p, l);
            if (!have || v != last) {
                if (table) table[base + rows] = v;
                rows++;
                have = true;
                last = v;
            }
            if (table) rank[l] = (uint16_t)(base + rows - 1);
        }
    }
    return rows;
}

// The whole table, serially, chunk by chunk as the kernel's threads take them: returns the number of rows (at most 2^bits)
BFD_HD int tq_build_table(const tq_params &p, const uint32_t *presence, int bits, float *table, uint16_t *rank)
{
    int prev = -1, base = 0;
    for (int c = 0; c < tq_chunks(bits); c++) {
        base += tq_chunk_rows(p, presence, c, prev, base, table, rank);
        const int last = tq_chunk_last(presence, c);
        if (last >= 0) prev = last;
    }
    return base;
}

// Order-preserving key of a float32: a < b as floats <=> key(a) < key(b) as unsigned (-0.0 below +0.0; NaNs beyond the infinities on either side)
BFD_HD uint32_t tq_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
BFD_HD uint32_t tq_unkey(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
#define TQ_KEY_NEG_INF 0x007FFFFFu
#define TQ_KEY_POS_INF 0xFF800000u
