// Sparse shear kernel of the tiled path and the kernels that build and serve its list: stress_shear_sparse works one thread per listed cell
// (solid centre); mark_solid_cells, shear_order_keys, shear_coefficients and shear_material_table make the list; scatter / gather_shear_memory
// carry its memory variables to and from the full-volume arrays; css_row_table, css_scatter and css_gather serve the compact solid state.
// The kernels defined behind the anonymous namespace have external names: they keep the symbols they have always had. gfx950 only.
#include "bfd_internal.h"
#include "bfd_device.h"
#include <algorithm>

namespace {

// sparse shear update: one thread per listed cell (solid centre). coef[6*t..] = A,B of the xy, xz, yz edges
// (0,0 where the 4-cell condition fails), computed once at setup with the canonical arithmetic.
__device__ __forceinline__ float ldv(const float *__restrict__ a, int N1, int N2, int i, int j, long kofs)
{
    return (i >= 0 && i < N1 && j >= 0 && j < N2) ? a[kofs + (long)j * N1 + i] : 0.0f;
}

// x / d for x < 2^31 and d >= 2 as a multiply-high and a shift (M = ceil(2^(31+L) / d), L = ceil(log2 d)): the three run-time integer
// divisions of the cell index cost ~100 of this kernel's ~310 VALU instructions per thread
struct FastDiv { unsigned M, s; };
__device__ __forceinline__ unsigned fdiv(unsigned x, FastDiv f) { return __umulhi(x, f.M) >> f.s; }

constexpr int SPARSE_WAVES_PER_SIMD = 5;
// NORMAL (compact solid state): the kernel also updates Sxx, Syy and their memory variables of its cell (compact arrays, entry t of this launch's
// part of the list) -- Szz / Rzz of the cell were written by the fluid stress kernel, which ran before and has advanced the absorbing-layer
// memory variables of dxVx, dyVy, dzVz: they are read here, not advanced.
template <bool NORMAL>
__global__ __launch_bounds__(256, SPARSE_WAVES_PER_SIMD) void stress_shear_sparse(bfd_dev d, const unsigned *__restrict__ cells, const unsigned *__restrict__ codes,
                                                           const float *__restrict__ tab, const float *__restrict__ coef,
                                                           float *__restrict__ Rc, long nTotal, long n, FastDiv divN1, FastDiv divPlane,
                                                           float *__restrict__ cSxy, float *__restrict__ cSxz, float *__restrict__ cSyz,
                                                           float *__restrict__ cSxx, float *__restrict__ cSyy, float *__restrict__ cRxx, float *__restrict__ cRyy,
                                                           float *__restrict__ cRxy, float *__restrict__ cRxz, float *__restrict__ cRyz)
{
    // XCD e works through the e-th contiguous eighth of the list (order: shear_order_keys): the V values a cell gathers from its
    // row / plane neighbours were fetched by blocks just before it on the SAME XCD (its own L2)
    const long t = (long)remap_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    if (t >= n) return;
    const int N1 = d.N1, N2 = d.N2, P = d.P;
    const long pl = d.plane;
    const unsigned c = LDNT(cells + t);
    // compact solid state: the ten values of the cell are dense streams in list order and depend on nothing -- in flight before the gathers start
    float oSxx = 0.f, oSyy = 0.f, oRxx = 0.f, oRyy = 0.f, oSxy = 0.f, oSxz = 0.f, oSyz = 0.f, oRxy = 0.f, oRxz = 0.f, oRyz = 0.f;
    if (NORMAL) {
        oSxx = LDNT(cSxx + t); oSyy = LDNT(cSyy + t); oRxx = LDNT(cRxx + t); oRyy = LDNT(cRyy + t);
        oSxy = LDNT(cSxy + t); oSxz = LDNT(cSxz + t); oSyz = LDNT(cSyz + t);
        oRxy = LDNT(cRxy + t); oRxz = LDNT(cRxz + t); oRyz = LDNT(cRyz + t);
    }
    const unsigned ukl = fdiv(c, divPlane), rem = c - ukl * (unsigned)d.plane, uj = fdiv(rem, divN1);
    const int i = (int)(rem - uj * (unsigned)N1), j = (int)uj, kl = (int)ukl;
    const long ko = (long)kl * pl;
    const int k = d.k0 + kl;
    // edge coefficients: from the per-material table where the four cells of the edge hold one material (most of a bone's
    // interior), explicit otherwise (24 B per cell less to stream)
    const unsigned cw = LDNT(codes + t);
    float AP = 0.f, BP = 0.f, AS2 = 0.f, BS2 = 0.f;
    if (NORMAL) {       // material of the cell: from the code word (its fourth byte), else from the id array
        const unsigned mb = cw >> 24;
        const int m = mb ? (int)mb - 1 : (int)(d.mat[c] & BFD_MAT_MASK);
        const float4 cm = *(const float4 *)(tab + 8 * m + 4);
        AP = cm.x; BP = cm.y; AS2 = cm.z; BS2 = cm.w;
    }
    float Axy = 0.f, Bxy = 0.f, Axz = 0.f, Bxz = 0.f, Ayz = 0.f, Byz = 0.f;
    {
        const unsigned q = cw & 255u;
        if (q == 255u) { Axy = LDNT(coef + 6 * t); Bxy = LDNT(coef + 6 * t + 1); } else if (q) { const float2 ab = *(const float2 *)(tab + 8 * (q - 1)); Axy = ab.x; Bxy = ab.y; }
    }
    {
        const unsigned q = (cw >> 8) & 255u;
        if (q == 255u) { Axz = LDNT(coef + 6 * t + 2); Bxz = LDNT(coef + 6 * t + 3); } else if (q) { const float2 ab = *(const float2 *)(tab + 8 * (q - 1)); Axz = ab.x; Bxz = ab.y; }
    }
    {
        const unsigned q = (cw >> 16) & 255u;
        if (q == 255u) { Ayz = LDNT(coef + 6 * t + 4); Byz = LDNT(coef + 6 * t + 5); } else if (q) { const float2 ab = *(const float2 *)(tab + 8 * (q - 1)); Ayz = ab.x; Byz = ab.y; }
    }
    // the 21 velocities: wave-uniform bases + one 32-bit byte offset (c < 2^30); a cell whose stencil stays inside the domain in x and y
    // (all but the cells on the outermost two rows / columns) takes them without a test per value
    const unsigned c4 = c * 4u, r4 = (unsigned)N1 * 4u;
    float vx0, vy0, vz0;
    float dyVx, dxVy, dxVz, dyVz, dxVx = 0.f, dyVy = 0.f, dzVz = 0.f;
    const bool inside = i >= 2 && i + 2 < N1 && j >= 2 && j + 2 < N2;
    if (inside) {
        // round 6: the four x-taps of a component as ONE unaligned 16-byte load: 12 of the 30 gathers become 3 (0.245 -> 0.232 ms at the shear medium 512^3)
        typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
        const f4u qx = *(const f4u *)((const char *)uni(d.Vx) + (c4 - 8u));        // Vx at i-2 .. i+1
        const f4u qy = *(const f4u *)((const char *)uni(d.Vy) + (c4 - 4u));        // Vy at i-1 .. i+2
        const f4u qz = *(const f4u *)((const char *)uni(d.Vz) + (c4 - 4u));        // Vz at i-1 .. i+2
        vx0 = qx.z; vy0 = qy.y; vz0 = qz.y;
        dyVx = dplus4(F4(d.Vx, c4 - r4), vx0, F4(d.Vx, c4 + r4), F4(d.Vx, c4 + 2 * r4));
        dxVy = dplus4(qy.x, vy0, qy.z, qy.w);
        dxVz = dplus4(qz.x, vz0, qz.z, qz.w);
        dyVz = dplus4(F4(d.Vz, c4 - r4), vz0, F4(d.Vz, c4 + r4), F4(d.Vz, c4 + 2 * r4));
        if (NORMAL) { dxVx = dminus4(qx.x, qx.y, vx0, qx.w); dyVy = dminus4(F4(d.Vy, c4 - 2 * r4), F4(d.Vy, c4 - r4), vy0, F4(d.Vy, c4 + r4)); }
    } else {
        vx0 = F4(d.Vx, c4); vy0 = F4(d.Vy, c4); vz0 = F4(d.Vz, c4);
        dyVx = dplus4(ldv(d.Vx, N1, N2, i, j - 1, ko), vx0, ldv(d.Vx, N1, N2, i, j + 1, ko), ldv(d.Vx, N1, N2, i, j + 2, ko));
        dxVy = dplus4(ldv(d.Vy, N1, N2, i - 1, j, ko), vy0, ldv(d.Vy, N1, N2, i + 1, j, ko), ldv(d.Vy, N1, N2, i + 2, j, ko));
        dxVz = dplus4(ldv(d.Vz, N1, N2, i - 1, j, ko), vz0, ldv(d.Vz, N1, N2, i + 1, j, ko), ldv(d.Vz, N1, N2, i + 2, j, ko));
        dyVz = dplus4(ldv(d.Vz, N1, N2, i, j - 1, ko), vz0, ldv(d.Vz, N1, N2, i, j + 1, ko), ldv(d.Vz, N1, N2, i, j + 2, ko));
        if (NORMAL) {
            dxVx = dminus4(ldv(d.Vx, N1, N2, i - 2, j, ko), ldv(d.Vx, N1, N2, i - 1, j, ko), vx0, ldv(d.Vx, N1, N2, i + 1, j, ko));
            dyVy = dminus4(ldv(d.Vy, N1, N2, i, j - 2, ko), ldv(d.Vy, N1, N2, i, j - 1, ko), vy0, ldv(d.Vy, N1, N2, i, j + 1, ko));
        }
    }
    float dzVx = dplus4(F4(d.Vx - pl, c4), vx0, F4(d.Vx + pl, c4), F4(d.Vx + 2 * pl, c4));
    float dzVy = dplus4(F4(d.Vy - pl, c4), vy0, F4(d.Vy + pl, c4), F4(d.Vy + 2 * pl, c4));
    if (NORMAL) dzVz = dminus4(F4(d.Vz - 2 * pl, c4), F4(d.Vz - pl, c4), vz0, F4(d.Vz + pl, c4));
    if (i < P || i >= N1 - P) {
        const int xi = i < P ? i : i - (N1 - 2 * P);
        const unsigned q = (unsigned)((kl * N2 + j) * (2 * P) + xi);
        dxVy = cpml(d.psi[4], q, d.axH[i], d.bxH[i], dxVy);
        dxVz = cpml(d.psi[6], q, d.axH[i], d.bxH[i], dxVz);
        if (NORMAL) dxVx = dxVx + d.psi[0][q];          // advanced by the fluid stress kernel in this half-step
    }
    if (j < P || j >= N2 - P) {
        const int yj = j < P ? j : j - (N2 - 2 * P);
        const unsigned q = (unsigned)((kl * (2 * P) + yj) * N1 + i);
        dyVx = cpml(d.psi[3], q, d.ayH[j], d.byH[j], dyVx);
        dyVz = cpml(d.psi[8], q, d.ayH[j], d.byH[j], dyVz);
        if (NORMAL) dyVy = dyVy + d.psi[1][q];
    }
    if (k < P || k >= d.N3 - P) {
        const int zk = k < P ? k : k - (d.N3 - 2 * P);
        const unsigned q = (unsigned)(zk * d.plane) + (unsigned)(j * N1 + i);
        dzVx = cpml(d.psi[5], q, d.azH[k], d.bzH[k], dzVx);
        dzVy = cpml(d.psi[7], q, d.azH[k], d.bzH[k], dzVy);
        if (NORMAL) dzVz = dzVz + d.psi[2][q];
    }
    const float c1 = d.c1;
    if (NORMAL) {       // Sxx, Syy of the cell: the canonical expressions of stress_v2 / stress_solid
        const float sXY = dxVx + dyVy;
        const float div = sXY + dzVz;
        const float sYZ = dyVy + dzVz, sXZ = dxVx + dzVz;
        float rn = c1 * oRxx - (BP * div - BS2 * sYZ);
        __builtin_nontemporal_store(oSxx + ((AP * div - AS2 * sYZ) + 0.5f * (oRxx + rn)), cSxx + t); __builtin_nontemporal_store(rn, cRxx + t);
        rn = c1 * oRyy - (BP * div - BS2 * sXZ);
        __builtin_nontemporal_store(oSyy + ((AP * div - AS2 * sXZ) + 0.5f * (oRyy + rn)), cSyy + t); __builtin_nontemporal_store(rn, cRyy + t);
    }
    // memory variables: with the other compact arrays or beside the list (Rc, list order)
    float *pRxy = NORMAL ? cRxy + t : Rc + t, *pRxz = NORMAL ? cRxz + t : Rc + nTotal + t, *pRyz = NORMAL ? cRyz + t : Rc + 2 * nTotal + t;
    // shear stresses: in list order too when the solid state is compact (cSxy .. = the entries of this launch's part of the list)
    float *pSxy = cSxy ? cSxy + t : d.Sxy + c, *pSxz = cSxz ? cSxz + t : d.Sxz + c, *pSyz = cSyz ? cSyz + t : d.Syz + c;
    if (Axy != 0.f) {
        const float e = dyVx + dxVy;
        const float r = NORMAL ? oRxy : LDNT(pRxy), rn = c1 * r - Bxy * e;
        *pSxy = (NORMAL ? oSxy : LDNT(pSxy)) + (Axy * e + 0.5f * (r + rn)); *pRxy = rn;
    }
    // compact solid state in a Z-slab: the planes a neighbour reads (its ghost planes: my plane 0 and my last two) also go to the full-volume
    // Sxz / Syz, which is where the halo exchange takes them from
    const bool shared = NORMAL && (kl == 0 || kl >= d.nk - 2);
    if (Axz != 0.f) {
        const float e = dzVx + dxVz;
        const float r = NORMAL ? oRxz : LDNT(pRxz), rn = c1 * r - Bxz * e;
        const float v = (NORMAL ? oSxz : LDNT(pSxz)) + (Axz * e + 0.5f * (r + rn));
        *pSxz = v; *pRxz = rn;
        if (shared) d.Sxz[c] = v;
    }
    if (Ayz != 0.f) {
        const float e = dzVy + dyVz;
        const float r = NORMAL ? oRyz : LDNT(pRyz), rn = c1 * r - Byz * e;
        const float v = (NORMAL ? oSyz : LDNT(pSyz)) + (Ayz * e + 0.5f * (r + rn));
        *pSyz = v; *pRyz = rn;
        if (shared) d.Syz[c] = v;
    }
}

// outputs: the list-ordered memory variables of the shear stresses into the full-volume arrays
__global__ void scatter_shear_memory(bfd_dev d, const unsigned *__restrict__ cells, const float *__restrict__ Rc, long n)
{
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
        const unsigned c = cells[t];
        d.Rxy[c] = Rc[t]; d.Rxz[c] = Rc[n + t]; d.Ryz[c] = Rc[2 * n + t];
    }
}

// the reverse, after a list has been rebuilt in the middle of a run
__global__ void gather_shear_memory(bfd_dev d, const unsigned *__restrict__ cells, float *__restrict__ Rc, long n)
{
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
        const unsigned c = cells[t];
        Rc[t] = d.Rxy[c]; Rc[n + t] = d.Rxz[c]; Rc[2 * n + t] = d.Ryz[c];
    }
}

// setup: flag cells with a solid, non-reflector centre; then the edge coefficients of the listed cells
__global__ void mark_solid_cells(bfd_dev d, unsigned char *__restrict__ flag, long n)
{
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long)gridDim.x * blockDim.x) {
        const unsigned raw = d.mat[v];
        const bool solid = !(raw & BFD_REFLECTOR_BIT) && d.invMu[raw & BFD_MAT_MASK] > 0.f;
        flag[v] = solid ? 1 : 0;
    }
}
// codes (may be null): one word per listed cell, a byte per edge (xy, xz, yz): 0 = the edge is never updated, 1 + m = its four
// cells hold material m < 254 (coefficients from the per-material table shear_material_table builds with the very same
// expression), 255 = mixed materials: the explicit coefficients in coef are read; the fourth byte: 1 + material of the cell itself (0 when
// it does not fit: the kernel reads the id array then) -- the sparse kernel's Sxx / Syy coefficients start from this word, which arrives
// with the cell index, instead of from the id behind the index (one dependent memory round trip less)
__global__ void shear_coefficients(bfd_dev d, const unsigned *__restrict__ cells, float *__restrict__ coef, unsigned *__restrict__ codes, long n)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int N1 = d.N1, N2 = d.N2;
    const long pl = d.plane;
    const unsigned c = cells[t];
    const int i = (int)(c % (unsigned)N1), j = (int)((c / (unsigned)N1) % (unsigned)N2);
    const long ko = (long)(c / (unsigned)d.plane) * pl;
    const int i1 = min(i + 1, N1 - 1), j1 = min(j + 1, N2 - 1);
    const long r0 = ko + (long)j * N1, r1 = ko + (long)j1 * N1;
    const int m = d.mat[c] & BFD_MAT_MASK;
    const int mx = d.mat[r0 + i1] & BFD_MAT_MASK, my = d.mat[r1 + i] & BFD_MAT_MASK, mz = d.mat[r0 + pl + i] & BFD_MAT_MASK;
    const int mxy = d.mat[r1 + i1] & BFD_MAT_MASK, mxz = d.mat[r0 + pl + i1] & BFD_MAT_MASK, myz = d.mat[r1 + pl + i] & BFD_MAT_MASK;
    const float iv0 = d.invMu[m], t0 = d.tauS[m], k2 = d.k2;
    const float ivx = d.invMu[mx], ivy = d.invMu[my], ivz = d.invMu[mz];
    float o[6] = {0, 0, 0, 0, 0, 0};
    {
        const float e4 = d.invMu[mxy];
        if (ivx > 0.f && ivy > 0.f && e4 > 0.f) {
            const float muH = 4.0f / ((iv0 + ivx) + (ivy + e4));
            const float tau = 0.25f * ((t0 + d.tauS[mx]) + (d.tauS[my] + d.tauS[mxy]));
            o[0] = muH * (1.0f + tau); o[1] = (muH * tau) * k2;
        }
    }
    {
        const float e4 = d.invMu[mxz];
        if (ivx > 0.f && ivz > 0.f && e4 > 0.f) {
            const float muH = 4.0f / ((iv0 + ivx) + (ivz + e4));
            const float tau = 0.25f * ((t0 + d.tauS[mx]) + (d.tauS[mz] + d.tauS[mxz]));
            o[2] = muH * (1.0f + tau); o[3] = (muH * tau) * k2;
        }
    }
    {
        const float e4 = d.invMu[myz];
        if (ivy > 0.f && ivz > 0.f && e4 > 0.f) {
            const float muH = 4.0f / ((iv0 + ivy) + (ivz + e4));
            const float tau = 0.25f * ((t0 + d.tauS[my]) + (d.tauS[mz] + d.tauS[myz]));
            o[4] = muH * (1.0f + tau); o[5] = (muH * tau) * k2;
        }
    }
    for (int q = 0; q < 6; q++) coef[6 * t + q] = o[q];
    if (codes) {
        auto code = [&](float A, int ma, int mb, int mc) { return A == 0.f ? 0u : ((m == ma && m == mb && m == mc && m < 254) ? (unsigned)(1 + m) : 255u); };
        codes[t] = code(o[0], mx, my, mxy) | (code(o[2], mx, mz, mxz) << 8) | (code(o[4], my, mz, myz) << 16) | (m < 255 ? (unsigned)(1 + m) << 24 : 0u);
    }
}
// A, B of an edge whose four cells hold material m: tab[2 m], tab[2 m + 1]
__global__ void shear_material_table(bfd_dev d, float *__restrict__ tab, int nMat)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nMat) return;
    const float iv0 = d.invMu[m], t0 = d.tauS[m], k2 = d.k2;
    float A = 0.f, B = 0.f;
    if (iv0 > 0.f) {
        const float muH = 4.0f / ((iv0 + iv0) + (iv0 + iv0));
        const float tau = 0.25f * ((t0 + t0) + (t0 + t0));
        A = muH * (1.0f + tau); B = (muH * tau) * k2;
    }
    // 32 bytes per material: (A, B) of a one-material edge as one 8-byte load, the cell's own AP, BP, AS2, BS2 as one 16-byte load (round 6: the sparse
    // kernel takes its per-material coefficients with 1 + 3 loads instead of 4 + 6)
    tab[8 * m] = A; tab[8 * m + 1] = B; tab[8 * m + 2] = 0.f; tab[8 * m + 3] = 0.f;
    tab[8 * m + 4] = d.AP[m]; tab[8 * m + 5] = d.BP[m]; tab[8 * m + 6] = d.AS2[m]; tab[8 * m + 7] = d.BS2[m];
}

}  // namespace

// cells [b, e) of the list; R = their part of the list-ordered memory variables (full-volume stresses), unused with the compact solid state
void bfd_launch_stress_shear(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, long b, long e, float *R)
{
    if (e <= b) return;
    auto magic = [](unsigned dv) { FastDiv f; unsigned L = 0; while ((1ull << L) < dv) L++; if (L == 0) L = 1;
                                   f.M = (unsigned)(((1ull << (31 + L)) + dv - 1) / dv); f.s = L - 1; return f; };
    const FastDiv dN1 = magic((unsigned)d.N1), dPl = magic((unsigned)d.plane);
    const dim3 g((unsigned)((e - b + 255) / 256));
    if (d.cssRow) hipLaunchKernelGGL(stress_shear_sparse<true>, g, dim3(256), 0, s, d, t->shearCells + b, t->shearCodes + b, t->shearTab, t->shearCoef + 6 * b, (float *)nullptr, t->nShear, e - b, dN1, dPl,
                                     d.cSxy + b, d.cSxz + b, d.cSyz + b, d.cSxx + b, d.cSyy + b, d.cRxx + b, d.cRyy + b, d.cRxy + b, d.cRxz + b, d.cRyz + b);
    else hipLaunchKernelGGL(stress_shear_sparse<false>, g, dim3(256), 0, s, d, t->shearCells + b, t->shearCodes + b, t->shearTab, t->shearCoef + 6 * b, R, t->nShear, e - b, dN1, dPl,
                            (float *)nullptr, (float *)nullptr, (float *)nullptr, (float *)nullptr, (float *)nullptr, (float *)nullptr, (float *)nullptr, (float *)nullptr, (float *)nullptr, (float *)nullptr);
}

// Order of the sparse shear list. Ascending in the cell index (k, j, i), a cell's z neighbours (planes k-2 .. k+2, 9 of its 21
// gathered V values) were touched a whole plane of listed cells earlier: 1 MB of traffic at 512^2 planes, 3.8 MB at 1024^2, five
// planes of that beyond the 4 MB L2 of an XCD -- at 1024^3 the kernel moved 1.68 x its algorithmic bytes (8.58 GB per launch).
// The order kept: (z-chunk of 16 planes, band of 8 rows, plane, row, i): rows keep their whole length in x, the z neighbours are
// one band-plane away: 6.21 GB = 1.21 x at 1024^3, unchanged at 512^3 (0.89 GB, where the planes fitted), kernel time unchanged:
// it follows neither the bytes nor the number of gathers (the six x neighbours taken from the neighbouring lanes by shuffles: 4-9 %
// slower). Cutting the rows at the 64-wide tiles as well: same bytes, 3 % slower (removed, like the ascending order).
// The three plane ranges the split half-steps launch separately (first / middle / last planes of a slab) stay contiguous: their
// number leads the key. profiles/r3/shear_list_order.txt
// rows keep their whole length in x: (part of the slab, z-chunk, band of 8 rows, plane, row, i)
__device__ __forceinline__ unsigned long long shear_key2(unsigned i, unsigned j, unsigned k, int lowPlanes, int hiStart)
{
    const unsigned long long seg = (int)k < lowPlanes ? 0ull : ((int)k >= hiStart ? 2ull : 1ull);
    return (seg << 44) | ((unsigned long long)(k >> 4) << 32) | ((unsigned long long)(j >> 3) << 19) |
           ((unsigned long long)(k & 15u) << 15) | ((unsigned long long)(j & 7u) << 12) | (unsigned long long)(i & 4095u);
}
__global__ void shear_order_keys(bfd_dev d, const unsigned *__restrict__ cells, unsigned long long *__restrict__ keys, long n, int lowPlanes, int hiStart)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const unsigned c = cells[t];
    const unsigned i = c % (unsigned)d.N1, j = (c / (unsigned)d.N1) % (unsigned)d.N2, k = c / (unsigned)d.plane;
    keys[t] = shear_key2(i, j, k, lowPlanes, hiStart);
}
// Row table of the compact solid state (bfd_dev::cssRow) for a list in order mode 2: entry (plane kk = kl + 2, row j, tile bx) = number of listed
// cells that precede cell (64 bx, j, kl) in list order = lower bound of its key in the sorted list (the keys are recomputed from the cells). A
// row of the list is contiguous and ascending in i, so this is the entry of the row's first listed cell at or after x = 64 bx; bx = tilesX
// (the key's i field carries into the row bits: still the next key in order) gives one past the row. Ghost planes: BFD_CSS_NONE.
__global__ void css_row_table(bfd_dev d, const unsigned *__restrict__ cells, long n, unsigned *__restrict__ table, int stride, int lowPlanes, int hiStart)
{
    const long total = (long)(d.nk + 4) * d.N2 * stride;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int bx = (int)(e % stride);
        const long r = e / stride;
        const int j = (int)(r % d.N2), kl = (int)(r / d.N2) - 2;
        if (kl < 0 || kl >= d.nk) { table[e] = BFD_CSS_NONE; continue; }
        const unsigned long long probe = shear_key2(0u, (unsigned)j, (unsigned)kl, lowPlanes, hiStart) + (unsigned long long)(64 * bx);
        long lo = 0, hi = n;
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            const unsigned c = cells[mid];
            const unsigned ci = c % (unsigned)d.N1, cj = (c / (unsigned)d.N1) % (unsigned)d.N2, ck = c / (unsigned)d.plane;
            if (shear_key2(ci, cj, ck, lowPlanes, hiStart) < probe) lo = mid + 1; else hi = mid;
        }
        table[e] = (unsigned)lo;
    }
}
void bfd_launch_css_row_table(const bfd_dev &d, hipStream_t s, const unsigned *cells, long n, unsigned *rowTable, int stride, int lowPlanes, int hiStart)
{
    const long total = (long)(d.nk + 4) * d.N2 * stride;
    hipLaunchKernelGGL(css_row_table, dim3((unsigned)std::min<long>((total + 255) / 256, 65536)), dim3(256), 0, s, d, cells, n, rowTable, stride, lowPlanes, hiStart);
}
// one compact array <-> a full-volume buffer at the listed cells (outputs; a list rebuilt in the middle of a run)
__global__ void css_scatter(const unsigned *__restrict__ cells, long n, const float *__restrict__ compact, float *__restrict__ dstFull)
{
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) dstFull[cells[t]] = compact[t];
}
__global__ void css_gather(const unsigned *__restrict__ cells, long n, const float *__restrict__ srcFull, float *__restrict__ dstCompact)
{
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) dstCompact[t] = srcFull[cells[t]];
}
void bfd_launch_css_scatter(hipStream_t s, const unsigned *cells, long n, const float *compact, float *dstFull)
{
    if (n > 0) hipLaunchKernelGGL(css_scatter, dim3((unsigned)std::min<long>((n + 255) / 256, 8192)), dim3(256), 0, s, cells, n, compact, dstFull);
}
void bfd_launch_css_gather(hipStream_t s, const unsigned *cells, long n, const float *srcFull, float *dstCompact)
{
    if (n > 0) hipLaunchKernelGGL(css_gather, dim3((unsigned)std::min<long>((n + 255) / 256, 8192)), dim3(256), 0, s, cells, n, srcFull, dstCompact);
}

void bfd_launch_shear_order_keys(const bfd_dev &d, hipStream_t s, const unsigned *cells, unsigned long long *keys, long n, int lowPlanes, int hiStart)
{
    if (n) hipLaunchKernelGGL(shear_order_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, cells, keys, n, lowPlanes, hiStart);
}

void bfd_launch_mark_solid(const bfd_dev &d, hipStream_t s, unsigned char *flag, long n)
{
    hipLaunchKernelGGL(mark_solid_cells, dim3((unsigned)std::min<long>((n + 255) / 256, 8192)), dim3(256), 0, s, d, flag, n);
}
void bfd_launch_scatter_shear_memory(const bfd_dev &d, hipStream_t s, const bfd_tiles *t)
{
    if (t->shearCells && t->shearR && t->nShear)
        hipLaunchKernelGGL(scatter_shear_memory, dim3((unsigned)std::min<long>((t->nShear + 255) / 256, 8192)), dim3(256), 0, s, d, t->shearCells, t->shearR, t->nShear);
}
void bfd_launch_gather_shear_memory(const bfd_dev &d, hipStream_t s, const bfd_tiles *t)
{
    if (t->shearCells && t->shearR && t->nShear)
        hipLaunchKernelGGL(gather_shear_memory, dim3((unsigned)std::min<long>((t->nShear + 255) / 256, 8192)), dim3(256), 0, s, d, t->shearCells, t->shearR, t->nShear);
}
void bfd_launch_shear_coefficients(const bfd_dev &d, hipStream_t s, const unsigned *cells, float *coef, unsigned *codes, float *tab, int nMat, long n)
{
    if (n) hipLaunchKernelGGL(shear_coefficients, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, cells, coef, codes, n);
    if (tab) hipLaunchKernelGGL(shear_material_table, dim3((unsigned)((nMat + 255) / 256)), dim3(256), 0, s, d, tab, nMat);
}
