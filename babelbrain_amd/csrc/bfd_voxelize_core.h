// Arithmetic, index and word logic of bfd_voxelize.hip, as host-and-device functions: the kernels call these per triangle, per (triangle, column)
// pair and per word, and a plain C++ program can call the same functions serially on the CPU to check them (no HIP needed). Not part of the ABI.
//
// The definition (include/babelfdtd.h, bfd_voxelize_mesh) is evaluated in float64, ONE OPERATION PER ROUNDING, in exactly the order written here:
// the library is built with -ffp-contract=off, and tests/voxelize_oracle.py performs the same operations in numpy. Do not reassociate.
// The conformal-mask scatter (bfd_voxel_scatter3d) is float32 under the same rule; its pieces are further down (conf_*), restated in
// tests/conformal_oracle.py.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define BFD_HD __host__ __device__ __forceinline__
#else
#define BFD_HD inline
#endif

struct vox_grid {
    int64_t gx, gy, gz;
    double min[3], u[3];     // u_a = (max_a - min_a) / g_a
    int64_t rowWords;        // 64-bit words of one column of the crossing table: gx + 1 bits, padded
    int64_t nColumns;        // gy gz
    int64_t nVoxels;         // gx gy gz
};

BFD_HD vox_grid vox_make_grid(const double *bmin, const double *bmax, int64_t gx, int64_t gy, int64_t gz)
{
    vox_grid g;
    g.gx = gx; g.gy = gy; g.gz = gz;
    const int64_t n[3] = {gx, gy, gz};
    for (int a = 0; a < 3; a++) { g.min[a] = bmin[a]; g.u[a] = (bmax[a] - bmin[a]) / (double)n[a]; }
    g.rowWords = (gx + 1 + 63) / 64;
    g.nColumns = gy * gz;
    g.nVoxels = gx * gy * gz;
    return g;
}

// What the crossing kernel needs of a triangle; written once per triangle by the setup kernel. Coordinates are relative to the box's min.
struct vox_tri {
    double ay, az, by, bz, cy, cz;   // the projection onto (y, z), counter-clockwise
    double v0x, v0y, v0z;            // the first vertex as given
    double nx, ny, nz;               // (v1 - v0) x (v2 - v1) of the vertices as given, not normalised
    int32_t jl, kl, nj, nk;          // clamped column box [jl, jl + nj) x [kl, kl + nk); nj = 0: the triangle meets no column
    int32_t topleft;                 // bit e: edge e (a->b, b->c, c->a) is a top-left edge
    int32_t pad;
};

// b_z < a_z, or b_z == a_z and a_y > b_y
BFD_HD bool vox_top_left(double ay, double az, double by, double bz) { return bz < az || (bz == az && ay > by); }

// tri: nine float32 (three vertices). Returns the number of columns of the triangle's clamped box (0: skipped).
BFD_HD int64_t vox_setup_triangle(const float *tri, const vox_grid &g, vox_tri *o)
{
    double v[3][3];
    for (int p = 0; p < 3; p++)
        for (int a = 0; a < 3; a++) v[p][a] = (double)tri[3 * p + a] - g.min[a];
    double ay = v[0][1], az = v[0][2], by = v[1][1], bz = v[1][2], cy = v[2][1], cz = v[2][2];
    const double area = (by - ay) * (cz - az) - (cy - ay) * (bz - az);
    o->nj = 0; o->nk = 0; o->jl = 0; o->kl = 0; o->pad = 0;
    if (area < 0) { double t = by; by = cy; cy = t; t = bz; bz = cz; cz = t; }
    o->ay = ay; o->az = az; o->by = by; o->bz = bz; o->cy = cy; o->cz = cz;
    o->topleft = (vox_top_left(ay, az, by, bz) ? 1 : 0) | (vox_top_left(by, bz, cy, cz) ? 2 : 0) | (vox_top_left(cy, cz, ay, az) ? 4 : 0);
    const double e0x = v[1][0] - v[0][0], e0y = v[1][1] - v[0][1], e0z = v[1][2] - v[0][2];
    const double e1x = v[2][0] - v[1][0], e1y = v[2][1] - v[1][1], e1z = v[2][2] - v[1][2];
    o->nx = e0y * e1z - e0z * e1y;
    o->ny = e0z * e1x - e0x * e1z;
    o->nz = e0x * e1y - e0y * e1x;
    o->v0x = v[0][0]; o->v0y = v[0][1]; o->v0z = v[0][2];
    if (area == 0) return 0;
    // the comparisons are made in float64 before anything is converted: a bound far outside the grid never reaches an integer
    const double jl = fmax(ceil(fmin(ay, fmin(by, cy)) / g.u[1] - 0.5), 0.0), jh = fmin(floor(fmax(ay, fmax(by, cy)) / g.u[1] - 0.5), (double)(g.gy - 1));
    const double kl = fmax(ceil(fmin(az, fmin(bz, cz)) / g.u[2] - 0.5), 0.0), kh = fmin(floor(fmax(az, fmax(bz, cz)) / g.u[2] - 0.5), (double)(g.gz - 1));
    if (!(jl <= jh && kl <= kh)) return 0;
    o->jl = (int32_t)jl; o->kl = (int32_t)kl;
    o->nj = (int32_t)(jh - jl) + 1; o->nk = (int32_t)(kh - kl) + 1;
    return (int64_t)o->nj * o->nk;
}

// edge function of a->b at p, in the one form whose value is exactly negated when the neighbouring triangle sees the edge as b->a
BFD_HD bool vox_edge_pass(double py, double pz, double ay, double az, double by, double bz, bool topLeft)
{
    const double t = (py - ay) * (pz - bz) - (pz - az) * (py - by);
    return t > 0 || (t == 0 && topLeft);
}

// Test (a) and the crossing position of triangle t in column (j, k): returns the bit position c = min(floor(q), gx - 1) + 1 in 1 .. gx of the
// column's row of the crossing table, or 0 when nothing is issued (the centre is outside the projection, or the surface lies below the first
// voxel centre, q < 0, or q is NaN: n_x == 0 with a zero numerator).
BFD_HD int64_t vox_crossing(const vox_tri &t, const vox_grid &g, int64_t j, int64_t k)
{
    const double py = ((double)j + 0.5) * g.u[1], pz = ((double)k + 0.5) * g.u[2];
    if (!vox_edge_pass(py, pz, t.ay, t.az, t.by, t.bz, (t.topleft & 1) != 0)) return 0;
    if (!vox_edge_pass(py, pz, t.by, t.bz, t.cy, t.cz, (t.topleft & 2) != 0)) return 0;
    if (!vox_edge_pass(py, pz, t.cy, t.cz, t.ay, t.az, (t.topleft & 4) != 0)) return 0;
    const double xs = t.v0x - (t.ny * (py - t.v0y) + t.nz * (pz - t.v0z)) / t.nx;
    const double q = floor(xs / g.u[0] - 0.5);
    if (!(q >= 0)) return 0;
    return (int64_t)fmin(q, (double)(g.gx - 1)) + 1;
}

// Suffix parity inside a word: bit b of the result = XOR of the bits of x at positions > b.
BFD_HD uint64_t vox_suffix_parity(uint64_t x)
{
    uint64_t s = x >> 1;
    s ^= s >> 1; s ^= s >> 2; s ^= s >> 4; s ^= s >> 8; s ^= s >> 16; s ^= s >> 32;
    return s;
}

BFD_HD int vox_popcount64(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}

// Word w of a column's occupancy row from the column's crossing row (rowWords words): bit b = voxel 64 w + b, the bits from gx on are 0.
BFD_HD uint64_t vox_scan_word(const uint64_t *row, int64_t w, const vox_grid &g)
{
    int parityAbove = 0;
    for (int64_t q = w + 1; q < g.rowWords; q++) parityAbove ^= vox_popcount64(row[q]) & 1;
    uint64_t occ = vox_suffix_parity(row[w]);
    if (parityAbove) occ = ~occ;
    const int64_t left = g.gx - 64 * w;                  // voxels from this word on
    if (left <= 0) return 0;
    if (left < 64) occ &= ((uint64_t)1 << left) - 1;
    return occ;
}

// bits [i, i + n) of an occupancy row as the low n bits, 1 <= n <= 32
BFD_HD uint32_t vox_row_bits(const uint64_t *row, int64_t i, int n)
{
    const int64_t w = i >> 6;
    const int s = (int)(i & 63);
    uint64_t v = row[w] >> s;
    if (s + n > 64) v |= row[w + 1] << (64 - s);
    return (uint32_t)(v & (((uint64_t)1 << n) - 1));
}

BFD_HD uint32_t vox_reverse32(uint32_t x)
{
    x = (x >> 16) | (x << 16);
    x = ((x & 0xFF00FF00u) >> 8) | ((x & 0x00FF00FFu) << 8);
    x = ((x & 0xF0F0F0F0u) >> 4) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x & 0xCCCCCCCCu) >> 2) | ((x & 0x33333333u) << 2);
    return ((x & 0xAAAAAAAAu) >> 1) | ((x & 0x55555555u) << 1);
}

// Word o of the voxel table (bit 31 - (index % 32) of word index / 32, index = i + gx (j + gy k)) from the occupancy rows: a table word takes up
// to 32 consecutive indices, which lie in one column's row or, for a short gx, in several.
BFD_HD uint32_t vox_table_word(const uint64_t *occ, int64_t o, const vox_grid &g)
{
    int64_t idx = 32 * o;
    const int64_t end = idx + 32 < g.nVoxels ? idx + 32 : g.nVoxels;
    uint32_t lsb = 0;                                    // bit b = index 32 o + b
    int at = 0;
    while (idx < end) {                                  // ends: n >= 1 in every round
        const int64_t col = idx / g.gx, i = idx - col * g.gx;
        int64_t n = g.gx - i;
        if (n > end - idx) n = end - idx;
        lsb |= vox_row_bits(occ + col * g.rowWords, i, (int)n) << at;
        at += (int)n; idx += n;
    }
    return vox_reverse32(lsb);
}

// the bits of table word o that are voxels, in the table's packing (all 32 except in a partial last word)
BFD_HD uint32_t vox_table_valid(int64_t o, int64_t nVoxels)
{
    const int64_t left = nVoxels - 32 * o;
    return left >= 32 ? 0xFFFFFFFFu : (left <= 0 ? 0u : ~(0xFFFFFFFFu >> left));
}

// coordinate of voxel index idx along one axis: float64, rounded once to float32
BFD_HD float vox_centre(double min, double unit, int64_t idx) { return (float)(min + ((double)idx + 0.5) * unit); }

// Conformal masks (include/babelfdtd.h, bfd_voxel_scatter3d): a point through a float32 [3][4] matrix to a voxel index. Every product and every
// sum is rounded to float32 on its own, in the order written; tests/conformal_oracle.py performs the same operations in numpy. On the device the
// intrinsics keep the statement independent of -ffp-contract; a host build needs -ffp-contract=off (x86-64 without -mfma contracts nothing anyway).
// This build flushes float32 denormals: a flushed operand changes a t by less than 2^-126 and cannot move it across a half-integer.
BFD_HD float conf_mul(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}
BFD_HD float conf_add(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}

// t = ((m0 x + py) + pz) + m3 of one matrix row m, with py = conf_mul(m1, y) and pz = conf_mul(m2, z) formed by the caller: they are the same for
// every point of a source row, and a product rounded on its own is the same wherever it is formed
BFD_HD float conf_row(const float *m, float x, float py, float pz) { return conf_add(conf_add(conf_add(conf_mul(m[0], x), py), pz), m[3]); }

// n = rint(t), half to even (np.round), saturated to the int32 range: t >= 2^31 and +inf give INT32_MAX, t <= -2^31, -inf and NaN give INT32_MIN
BFD_HD int32_t conf_round(float t)
{
    if (!(t > -2147483648.f)) return INT32_MIN;
    if (t >= 2147483648.f) return INT32_MAX;
    return (int32_t)rintf(t);
}

// the index of the three coordinates of a point, in one call
BFD_HD void conf_point(const float m[3][4], float x, float y, float z, int32_t n[3])
{
    for (int a = 0; a < 3; a++) n[a] = conf_round(conf_row(m[a], x, conf_mul(m[a][1], y), conf_mul(m[a][2], z)));
}

// What becomes of a point with index n in an output volume [M0][M1][M2], numpy's index rules behind the reference's filter of the upper side: the
// value is the slot of counts[] the point is counted in beside counts[0] (0: none).
enum { CONF_INSIDE = 0, CONF_ABOVE = 1, CONF_WRAPPED = 2, CONF_BELOW = 3 };
//   CONF_ABOVE    some n_a >= M_a: dropped (the filter comes first: such a point is dropped whatever its other indices are)
//   CONF_BELOW    otherwise, some n_a < -M_a: dropped (numpy raises IndexError here)
//   CONF_WRAPPED  otherwise, some n_a in [-M_a, 0): that index wraps by +M_a
// *at receives the voxel (i0 M1 + i1) M2 + i2 of a point that is not dropped; the saturated indices of conf_round are dropped on their side for
// every 1 <= M_a < 2^31.
BFD_HD int conf_target(const int32_t n[3], const int64_t M[3], int64_t *at)
{
    bool above = false, below = false, wrapped = false;
    for (int a = 0; a < 3; a++) {
        above |= n[a] >= M[a];
        below |= n[a] < -M[a];
        wrapped |= n[a] < 0;
    }
    if (above) return CONF_ABOVE;
    if (below) return CONF_BELOW;
    int64_t v = 0;
    for (int a = 0; a < 3; a++) v = v * M[a] + (n[a] < 0 ? n[a] + M[a] : n[a]);
    *at = v;
    return wrapped ? CONF_WRAPPED : CONF_INSIDE;
}

// bit of voxel index idx in a table in bfd_voxelize_mesh's packing
BFD_HD bool vox_table_bit(const uint32_t *table, int64_t idx) { return (table[idx >> 5] >> (31 - (int)(idx & 31))) & 1u; }

// CT value mapping. Values are compared as order-preserving integer keys of their float32 bits, never as floats: this build flushes float32
// denormals, and a float comparison might take a denormal for 0. The key keeps float order and float equality: -0.0 gets the key of +0.0.
BFD_HD bool map_is_nan(uint32_t bits) { return (bits & 0x7FFFFFFFu) > 0x7F800000u; }
BFD_HD uint32_t map_key(uint32_t bits)
{
    if (bits == 0x80000000u) bits = 0u;
    return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// the index m with keys[m] == key(v) in a strictly increasing table of keys, or 0 when there is none or v is a NaN (which equals nothing)
BFD_HD uint32_t map_lookup(const uint32_t *keys, int n, uint32_t vbits)
{
    if (map_is_nan(vbits)) return 0u;
    const uint32_t v = map_key(vbits);
    int lo = 0, hi = n;                                  // first index with keys[index] >= v; ends: hi - lo halves
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return (lo < n && keys[lo] == v) ? (uint32_t)lo : 0u;
}
