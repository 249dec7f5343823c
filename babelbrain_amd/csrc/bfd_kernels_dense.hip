// Dense kernels of the tiled path (kernelVariant 2): every cell of a run takes the full solid arithmetic, stress_v2 for the stress half-step and
// velocity_v2 for the velocity half-step. They run the solid runs of an engine that has no sparse shear list: bench.py's dense reference and
// the variant tests. Tile, z-march and LDS staging: bfd_tile.h. gfx950 only.
#include "bfd_tile.h"
#include "bfd_device.h"

namespace {

constexpr int STRESS_WAVES_PER_SIMD = 4;     // 2 workgroups of 8 waves per CU (<= 128 VGPRs); 6 or 8 spill and run 1.4-2.4x slower (measured)
constexpr int VELOCITY_WAVES_PER_SIMD = 4;

// ------------------------------------------------------------------------------------------------
// stress half-step
// ------------------------------------------------------------------------------------------------
// rowFlags (may be null): per run and plane, 2 bits per tile row (wave): bit0 = every cell of the row has a
// fluid centre and no reflector -> the row takes the fluid arithmetic (one normal stress read, identical
// result written to all three, no shear work); bit1 = additionally every cell has BP == 0 (no memory variable).
__global__ __launch_bounds__(NTHREADS, STRESS_WAVES_PER_SIMD) void stress_v2(bfd_dev d, int tilesX, int nblocks,
                                                                             const int4 *__restrict__ runs,
                                                                             const unsigned short *__restrict__ rowFlags)
{
    __shared__ float sV[2][3][LH * LW];
    const int N1 = d.N1, N2 = d.N2;
    const int pos = remap_block(blockIdx.x, nblocks);
    const int4 run = runs[pos];
    const int bx = run.x % tilesX, by = run.x / tilesX;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * TX + tx;
    const int i0 = bx * TX, j0 = by * TY;
    const int i = i0 + tx, j = j0 + ty;
    const bool valid = (i < N1) && (j < N2);
    const long pl = d.plane;
    const int kbeg = run.y & 0xFFFF, kend = run.y >> 16;
    const int P = d.P;
    const int own = (ty + 2) * LW + tx + 2;
    const unsigned cij = valid ? (unsigned)(j * N1 + i) : 0u;    // in-plane offset shared by every array

    // halo tasks: [Vx-y, Vy-y, Vz-y] 3*256, then [Vx-x, Vy-x, Vz-x] 3*32
    HaloTask ta, tb;
    ytask(tid & 255, tid >> 8, i0, j0, N1, N2, ta);
    {
        const int t2 = tid + NTHREADS;
        if (t2 < 3 * YT) ytask(t2 - 2 * YT, 2, i0, j0, N1, N2, tb);
        else if (t2 < 3 * YT + 3 * XT) { const int u = t2 - 3 * YT; xtask(u % XT, u / XT, i0, j0, N1, N2, tb); }
        else { tb.lofs = -1; tb.ok = false; tb.arr = 0; tb.gofs = 0; }
    }
    const float *pa = (ta.arr == 0 ? d.Vx : (ta.arr == 1 ? d.Vy : d.Vz)) + (ta.ok ? ta.gofs : 0);
    const float *pb = (tb.arr == 0 ? d.Vx : (tb.arr == 1 ? d.Vy : d.Vz)) + (tb.ok ? tb.gofs : 0);
    float *la = &sV[0][ta.arr][ta.lofs];
    float *lb = &sV[0][tb.arr][tb.lofs < 0 ? 0 : tb.lofs];
    const bool hasB = tb.lofs >= 0;

    const bool zi = valid && (i < P || i >= N1 - P);
    const bool zj = valid && (j < P || j >= N2 - P);
    const float c1 = d.c1, k2 = d.k2;

    // z register queues, primed for plane kbeg (ghost planes make kbeg-2 .. always addressable)
    float vxm1 = 0, vx0 = 0, vxp1 = 0, vxp2 = 0, vym1 = 0, vy0 = 0, vyp1 = 0, vyp2 = 0, vzm2 = 0, vzm1 = 0, vz0 = 0, vzp1 = 0;
    {
        const float *bVx = d.Vx + kbeg * pl, *bVy = d.Vy + kbeg * pl, *bVz = d.Vz + kbeg * pl;
        if (valid) {
            vxm1 = F4((bVx - pl), cij * 4u); vx0 = F4(bVx, cij * 4u); vxp1 = F4((bVx + pl), cij * 4u); vxp2 = F4((bVx + 2 * pl), cij * 4u);
            vym1 = F4((bVy - pl), cij * 4u); vy0 = F4(bVy, cij * 4u); vyp1 = F4((bVy + pl), cij * 4u); vyp2 = F4((bVy + 2 * pl), cij * 4u);
            vzm2 = F4((bVz - 2 * pl), cij * 4u); vzm1 = F4((bVz - pl), cij * 4u); vz0 = F4(bVz, cij * 4u); vzp1 = F4((bVz + pl), cij * 4u);
        }
    }
    float ha = ta.ok ? pa[kbeg * pl] : 0.0f;
    float hb = tb.ok ? pb[kbeg * pl] : 0.0f;

    for (int kl = kbeg; kl < kend; kl++) {
        const int b = kl & 1;
        const long ko = (long)kl * pl;          // uniform: plane bases stay in SGPRs
        const int k = d.k0 + kl;
        const int bo = b * (3 * LH * LW);
        // stage plane kl in LDS
        sV[b][0][own] = vx0; sV[b][1][own] = vy0; sV[b][2][own] = vz0;
        la[bo] = ha;
        if (hasB) lb[bo] = hb;
        __syncthreads();

        // this plane's state first (needed soonest), then the prefetches for plane kl+1
        float *pSxx = d.Sxx + ko, *pSyy = d.Syy + ko, *pSzz = d.Szz + ko;
        float *pRxx = d.Rxx + ko, *pRyy = d.Ryy + ko, *pRzz = d.Rzz + ko;
        const uint16_t *pM = d.mat + ko;
        const unsigned rf = rowFlags ? (rowFlags[pos * ZCHUNK + (kl - kbeg)] >> (2 * __builtin_amdgcn_readfirstlane(ty))) & 3u : 0u;
        const bool rowFluid = rf & 1u, rowLossless = rf & 2u;       // wave-uniform
        unsigned mraw = 0;
        float sxx = 0, syy = 0, szz = 0, rxx = 0, ryy = 0, rzz = 0;
        if (valid) {
            mraw = U2(pM, cij * 2u);
            szz = F4(pSzz, cij * 4u);
            if (!rowLossless) rzz = F4(pRzz, cij * 4u);
            if (!rowFluid) { sxx = F4(pSxx, cij * 4u); syy = F4(pSyy, cij * 4u); rxx = F4(pRxx, cij * 4u); ryy = F4(pRyy, cij * 4u); }
        }
        float nvx = 0, nvy = 0, nvz = 0, nha = 0, nhb = 0;
        if (kl + 1 < kend) {
            if (valid) { nvx = F4((d.Vx + ko + 3 * pl), cij * 4u); nvy = F4((d.Vy + ko + 3 * pl), cij * 4u); nvz = F4((d.Vz + ko + 2 * pl), cij * 4u); }
            if (ta.ok) nha = pa[ko + pl];
            if (tb.ok) nhb = pb[ko + pl];
        }

        if (valid && rowFluid) {
            // fluid row inside a solid tile: same arithmetic as stress_fluid_body, all three copies written
            const float *sx = &sV[b][0][own], *sy = &sV[b][1][own];
            float dxVx = dminus4(sx[-2], sx[-1], vx0, sx[1]);
            float dyVy = dminus4(sy[-2 * LW], sy[-LW], vy0, sy[LW]);
            float dzVz = dminus4(vzm2, vzm1, vz0, vzp1);
            if (zi) {
                const int xi = i < P ? i : i - (N1 - 2 * P);
                dxVx = cpml(d.psi[0], (unsigned)((kl * N2 + j) * (2 * P) + xi), d.axI[i], d.bxI[i], dxVx);
            }
            if (zj) {
                const int yj = j < P ? j : j - (N2 - 2 * P);
                dyVy = cpml(d.psi[1], (unsigned)((kl * (2 * P) + yj) * N1 + i), d.ayI[j], d.byI[j], dyVy);
            }
            if (k < P || k >= d.N3 - P) {
                const int zk = k < P ? k : k - (d.N3 - 2 * P);
                dzVz = cpml(d.psi[2], (unsigned)(zk * d.plane) + cij, d.azI[k], d.bzI[k], dzVz);
            }
            const int m = mraw & BFD_MAT_MASK;
            const float div = (dxVx + dyVy) + dzVz;
            const float AP = d.AP[m];
            float val;
            if (rowLossless) {
                val = szz + AP * div;
            } else {
                const float rn = c1 * rzz - d.BP[m] * div;
                val = szz + (AP * div + 0.5f * (rzz + rn));
                F4(pRxx, cij * 4u) = rn; F4(pRyy, cij * 4u) = rn; F4(pRzz, cij * 4u) = rn;
            }
            F4(pSxx, cij * 4u) = val; F4(pSyy, cij * 4u) = val; F4(pSzz, cij * 4u) = val;
        } else if (valid) {
            const float *sx = &sV[b][0][own], *sy = &sV[b][1][own], *sz = &sV[b][2][own];
            float dxVx = dminus4(sx[-2], sx[-1], vx0, sx[1]);
            float dyVy = dminus4(sy[-2 * LW], sy[-LW], vy0, sy[LW]);
            float dzVz = dminus4(vzm2, vzm1, vz0, vzp1);
            float dyVx = dplus4(sx[-LW], vx0, sx[LW], sx[2 * LW]);
            float dxVy = dplus4(sy[-1], vy0, sy[1], sy[2]);
            float dzVx = dplus4(vxm1, vx0, vxp1, vxp2);
            float dxVz = dplus4(sz[-1], vz0, sz[1], sz[2]);
            float dzVy = dplus4(vym1, vy0, vyp1, vyp2);
            float dyVz = dplus4(sz[-LW], vz0, sz[LW], sz[2 * LW]);

            if (mraw & BFD_REFLECTOR_BIT) {
                F4(pSxx, cij * 4u) = 0.f; F4(pSyy, cij * 4u) = 0.f; F4(pSzz, cij * 4u) = 0.f; F4((d.Sxy + ko), cij * 4u) = 0.f; F4((d.Sxz + ko), cij * 4u) = 0.f; F4((d.Syz + ko), cij * 4u) = 0.f;
                F4(pRxx, cij * 4u) = 0.f; F4(pRyy, cij * 4u) = 0.f; F4(pRzz, cij * 4u) = 0.f; F4((d.Rxy + ko), cij * 4u) = 0.f; F4((d.Rxz + ko), cij * 4u) = 0.f; F4((d.Ryz + ko), cij * 4u) = 0.f;
            } else {
                const int m = mraw & BFD_MAT_MASK;
                if (zi) {
                    const int xi = i < P ? i : i - (N1 - 2 * P);
                    const unsigned q = (unsigned)((kl * N2 + j) * (2 * P) + xi);
                    dxVx = cpml(d.psi[0], q, d.axI[i], d.bxI[i], dxVx);
                    dxVy = cpml(d.psi[4], q, d.axH[i], d.bxH[i], dxVy);
                    dxVz = cpml(d.psi[6], q, d.axH[i], d.bxH[i], dxVz);
                }
                if (zj) {
                    const int yj = j < P ? j : j - (N2 - 2 * P);
                    const unsigned q = (unsigned)((kl * (2 * P) + yj) * N1 + i);
                    dyVy = cpml(d.psi[1], q, d.ayI[j], d.byI[j], dyVy);
                    dyVx = cpml(d.psi[3], q, d.ayH[j], d.byH[j], dyVx);
                    dyVz = cpml(d.psi[8], q, d.ayH[j], d.byH[j], dyVz);
                }
                if (k < P || k >= d.N3 - P) {
                    const int zk = k < P ? k : k - (d.N3 - 2 * P);
                    const unsigned q = (unsigned)(zk * d.plane) + cij;
                    dzVz = cpml(d.psi[2], q, d.azI[k], d.bzI[k], dzVz);
                    dzVx = cpml(d.psi[5], q, d.azH[k], d.bzH[k], dzVx);
                    dzVy = cpml(d.psi[7], q, d.azH[k], d.bzH[k], dzVy);
                }
                {
                    const float AP = d.AP[m], BP = d.BP[m], AS2 = d.AS2[m], BS2 = d.BS2[m];
                    const float sXY = dxVx + dyVy;
                    const float div = sXY + dzVz;
                    const float sYZ = dyVy + dzVz, sXZ = dxVx + dzVz;
                    float rn;
                    rn = c1 * rxx - (BP * div - BS2 * sYZ);
                    F4(pSxx, cij * 4u) = sxx + ((AP * div - AS2 * sYZ) + 0.5f * (rxx + rn)); F4(pRxx, cij * 4u) = rn;
                    rn = c1 * ryy - (BP * div - BS2 * sXZ);
                    F4(pSyy, cij * 4u) = syy + ((AP * div - AS2 * sXZ) + 0.5f * (ryy + rn)); F4(pRyy, cij * 4u) = rn;
                    rn = c1 * rzz - (BP * div - BS2 * sXY);
                    F4(pSzz, cij * 4u) = szz + ((AP * div - AS2 * sXY) + 0.5f * (rzz + rn)); F4(pRzz, cij * 4u) = rn;
                }
                const float iv0 = d.invMu[m];
                if (iv0 > 0.f) {    // shear only where the centre cell is solid
                    const float t0 = d.tauS[m];
                    const int i1 = min(i + 1, N1 - 1), j1 = min(j + 1, N2 - 1);
                    const unsigned r0 = (unsigned)(j * N1), r1 = (unsigned)(j1 * N1);
                    const uint16_t *pM1 = pM + pl;
                    const int mx = pM[r0 + i1] & BFD_MAT_MASK, my = pM[r1 + i] & BFD_MAT_MASK;
                    const int mz = pM1[r0 + i] & BFD_MAT_MASK, mxy = pM[r1 + i1] & BFD_MAT_MASK;
                    const int mxz = pM1[r0 + i1] & BFD_MAT_MASK, myz = pM1[r1 + i] & BFD_MAT_MASK;
                    const float ivx = d.invMu[mx], ivy = d.invMu[my], ivz = d.invMu[mz];
                    {
                        const float e4 = d.invMu[mxy];
                        if (ivx > 0.f && ivy > 0.f && e4 > 0.f) {
                            float *pS = d.Sxy + ko, *pR = d.Rxy + ko;
                            const float muH = 4.0f / ((iv0 + ivx) + (ivy + e4));
                            const float tau = 0.25f * ((t0 + d.tauS[mx]) + (d.tauS[my] + d.tauS[mxy]));
                            const float A = muH * (1.0f + tau), B = (muH * tau) * k2;
                            const float e = dyVx + dxVy;
                            const float r = F4(pR, cij * 4u), rn = c1 * r - B * e;
                            F4(pS, cij * 4u) = F4(pS, cij * 4u) + (A * e + 0.5f * (r + rn)); F4(pR, cij * 4u) = rn;
                        }
                    }
                    {
                        const float e4 = d.invMu[mxz];
                        if (ivx > 0.f && ivz > 0.f && e4 > 0.f) {
                            float *pS = d.Sxz + ko, *pR = d.Rxz + ko;
                            const float muH = 4.0f / ((iv0 + ivx) + (ivz + e4));
                            const float tau = 0.25f * ((t0 + d.tauS[mx]) + (d.tauS[mz] + d.tauS[mxz]));
                            const float A = muH * (1.0f + tau), B = (muH * tau) * k2;
                            const float e = dzVx + dxVz;
                            const float r = F4(pR, cij * 4u), rn = c1 * r - B * e;
                            F4(pS, cij * 4u) = F4(pS, cij * 4u) + (A * e + 0.5f * (r + rn)); F4(pR, cij * 4u) = rn;
                        }
                    }
                    {
                        const float e4 = d.invMu[myz];
                        if (ivy > 0.f && ivz > 0.f && e4 > 0.f) {
                            float *pS = d.Syz + ko, *pR = d.Ryz + ko;
                            const float muH = 4.0f / ((iv0 + ivy) + (ivz + e4));
                            const float tau = 0.25f * ((t0 + d.tauS[my]) + (d.tauS[mz] + d.tauS[myz]));
                            const float A = muH * (1.0f + tau), B = (muH * tau) * k2;
                            const float e = dzVy + dyVz;
                            const float r = F4(pR, cij * 4u), rn = c1 * r - B * e;
                            F4(pS, cij * 4u) = F4(pS, cij * 4u) + (A * e + 0.5f * (r + rn)); F4(pR, cij * 4u) = rn;
                        }
                    }
                }
            }
        }
        // rotate the z queues
        vxm1 = vx0; vx0 = vxp1; vxp1 = vxp2; vxp2 = nvx;
        vym1 = vy0; vy0 = vyp1; vyp1 = vyp2; vyp2 = nvy;
        vzm2 = vzm1; vzm1 = vz0; vz0 = vzp1; vzp1 = nvz;
        ha = nha; hb = nhb;
    }
}

// ------------------------------------------------------------------------------------------------
// velocity half-step (+ fused Pressure RMS / peak accumulation)
// ------------------------------------------------------------------------------------------------
// LDS set: 0 Sxx (x halo), 1 Syy (y halo), 2 Sxy (x and y halo), 3 Sxz (x halo), 4 Syz (y halo)
template <bool ACC>
__global__ __launch_bounds__(NTHREADS, VELOCITY_WAVES_PER_SIMD) void velocity_v2(bfd_dev d, int tilesX, int nblocks,
                                                        float *__restrict__ accP, float *__restrict__ pkP,
                                                        const int4 *__restrict__ runs)
{
    __shared__ float sS[2][5][LH * LW];
    const int N1 = d.N1, N2 = d.N2;
    const int4 run = runs[remap_block(blockIdx.x, nblocks)];
    const int bx = run.x % tilesX, by = run.x / tilesX;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * TX + tx;
    const int i0 = bx * TX, j0 = by * TY;
    const int i = i0 + tx, j = j0 + ty;
    const bool valid = (i < N1) && (j < N2);
    const long pl = d.plane;
    const int kbeg = run.y & 0xFFFF, kend = run.y >> 16;
    const int P = d.P;
    const int own = (ty + 2) * LW + tx + 2;
    const unsigned cij = valid ? (unsigned)(j * N1 + i) : 0u;
    const unsigned cx = valid ? (unsigned)(j * N1 + min(i + 1, N1 - 1)) : 0u;      // (i+1, j)
    const unsigned cy = valid ? (unsigned)(min(j + 1, N2 - 1) * N1 + i) : 0u;      // (i, j+1)
    const bool accA = ACC && accP != nullptr, accK = ACC && pkP != nullptr;

    // halo tasks: [Syy-y, Sxy-y] 2*256 (task A: every thread), then [Syz-y] 256, [Sxx-x, Sxy-x, Sxz-x] 3*32
    HaloTask ta, tb;
    ytask(tid & 255, (tid >> 8) ? 2 : 1, i0, j0, N1, N2, ta);
    {
        const int t2 = tid;     // second task index in [0, 256+96)
        if (t2 < YT) ytask(t2, 4, i0, j0, N1, N2, tb);
        else if (t2 < YT + 3 * XT) {
            const int u = t2 - YT;
            const int a = u / XT;
            xtask(u % XT, a == 0 ? 0 : (a == 1 ? 2 : 3), i0, j0, N1, N2, tb);
        } else { tb.lofs = -1; tb.ok = false; tb.arr = 0; tb.gofs = 0; }
    }
    const float *pa = (ta.arr == 1 ? d.Syy : d.Sxy) + (ta.ok ? ta.gofs : 0);
    const float *pb = (tb.arr == 4 ? d.Syz : (tb.arr == 0 ? d.Sxx : (tb.arr == 2 ? d.Sxy : d.Sxz))) + (tb.ok ? tb.gofs : 0);
    float *la = &sS[0][ta.arr][ta.lofs];
    float *lb = &sS[0][tb.arr][tb.lofs < 0 ? 0 : tb.lofs];
    const bool hasB = tb.lofs >= 0;

    const bool zi = valid && (i < P || i >= N1 - P);
    const bool zj = valid && (j < P || j >= N2 - P);
    const bool inner = valid && i >= d.ND && i < N1 - d.ND && j >= d.ND && j < N2 - d.ND;

    // z queues: Szz k-1..k+2 ; Sxz, Syz k-2..k+1 ; in-plane arrays one plane ahead
    float zzm1 = 0, zz0 = 0, zzp1 = 0, zzp2 = 0, xzm2 = 0, xzm1 = 0, xz0 = 0, xzp1 = 0, yzm2 = 0, yzm1 = 0, yz0 = 0, yzp1 = 0;
    float sxx = 0, syy = 0, sxy = 0;
    if (valid) {
        const float *bzz = d.Szz + kbeg * pl, *bxz = d.Sxz + kbeg * pl, *byz = d.Syz + kbeg * pl;
        zzm1 = F4((bzz - pl), cij * 4u); zz0 = F4(bzz, cij * 4u); zzp1 = F4((bzz + pl), cij * 4u); zzp2 = F4((bzz + 2 * pl), cij * 4u);
        xzm2 = F4((bxz - 2 * pl), cij * 4u); xzm1 = F4((bxz - pl), cij * 4u); xz0 = F4(bxz, cij * 4u); xzp1 = F4((bxz + pl), cij * 4u);
        yzm2 = F4((byz - 2 * pl), cij * 4u); yzm1 = F4((byz - pl), cij * 4u); yz0 = F4(byz, cij * 4u); yzp1 = F4((byz + pl), cij * 4u);
        sxx = F4((d.Sxx + kbeg * pl), cij * 4u); syy = F4((d.Syy + kbeg * pl), cij * 4u); sxy = F4((d.Sxy + kbeg * pl), cij * 4u);
    }
    // pipelined like the fluid bodies: V, accumulators and material ids of plane kl are in registers when its
    // iteration starts (own id two planes ahead: the z face needs 1/rho of plane kl+1)
    float vx = 0, vy = 0, vz = 0, av = 0, pv = 0, r0 = 0;
    unsigned mraw = 0, mraw1 = 0, mx = 0, my = 0;
    if (valid) {
        const uint16_t *bM = d.mat + kbeg * pl;
        vx = F4((d.Vx + kbeg * pl), cij * 4u); vy = F4((d.Vy + kbeg * pl), cij * 4u); vz = F4((d.Vz + kbeg * pl), cij * 4u);
        mraw = U2(bM, cij * 2u); mraw1 = U2((bM + pl), cij * 2u); mx = U2(bM, cx * 2u); my = U2(bM, cy * 2u);
        if (accA) av = F4((accP + kbeg * pl), cij * 4u);
        if (accK) pv = F4((pkP + kbeg * pl), cij * 4u);
        r0 = d.invRho[mraw & BFD_MAT_MASK];
    }
    float ha = ta.ok ? pa[kbeg * pl] : 0.0f;
    float hb = tb.ok ? pb[kbeg * pl] : 0.0f;

    for (int kl = kbeg; kl < kend; kl++) {
        const int b = kl & 1;
        const long ko = (long)kl * pl;
        const int k = d.k0 + kl;
        const int bo = b * (5 * LH * LW);
        sS[b][0][own] = sxx; sS[b][1][own] = syy; sS[b][2][own] = sxy; sS[b][3][own] = xz0; sS[b][4][own] = yz0;
        la[bo] = ha;
        if (hasB) lb[bo] = hb;
        float r1 = 0, rx = 0, ry = 0;
        if (valid) {
            r1 = d.invRho[mraw1 & BFD_MAT_MASK];       // plane kl+1, becomes r0 of the next iteration
            rx = d.invRho[mx & BFD_MAT_MASK];
            ry = d.invRho[my & BFD_MAT_MASK];
        }
        __syncthreads();

        const float *pVx = d.Vx + ko, *pVy = d.Vy + ko, *pVz = d.Vz + ko;
        float *wVx = d.VxW + ko, *wVy = d.VyW + ko, *wVz = d.VzW + ko;
        float nzz = 0, nxz = 0, nyz = 0, nxx = 0, nyy = 0, nxy = 0, nha = 0, nhb = 0;
        float nvx = 0, nvy = 0, nvz = 0, nav = 0, npv = 0;
        unsigned nm2 = 0, nmx = 0, nmy = 0;
        if (valid) nm2 = U2((d.mat + ko + 2 * pl), cij * 2u);              // ghost planes make kl+2 addressable
        if (kl + 1 < kend) {
            if (valid) {
                nzz = F4((d.Szz + ko + 3 * pl), cij * 4u); nxz = F4((d.Sxz + ko + 2 * pl), cij * 4u); nyz = F4((d.Syz + ko + 2 * pl), cij * 4u);
                nxx = F4((d.Sxx + ko + pl), cij * 4u); nyy = F4((d.Syy + ko + pl), cij * 4u); nxy = F4((d.Sxy + ko + pl), cij * 4u);
                nvx = F4((pVx + pl), cij * 4u); nvy = F4((pVy + pl), cij * 4u); nvz = F4((pVz + pl), cij * 4u);
                nmx = U2((d.mat + ko + pl), cx * 2u); nmy = U2((d.mat + ko + pl), cy * 2u);
                if (accA) nav = F4((accP + ko + pl), cij * 4u);
                if (accK) npv = F4((pkP + ko + pl), cij * 4u);
            }
            if (ta.ok) nha = pa[ko + pl];
            if (tb.ok) nhb = pb[ko + pl];
        }

        if (valid) {
            if (ACC) {
                // Pressure RMS / peak of this step's final stresses (stress sources were injected
                // before this kernel), outside the absorbing layer only
                if (inner && k >= d.ND && k < d.N3 - d.ND) {
                    const float s = (sxx + syy) + zz0;
                    const float p = -s * (1.0f / 3.0f);
                    if (accA) F4((accP + ko), cij * 4u) = av + p * p;
                    if (accK) { const float ap = fabsf(p); if (ap > pv) F4((pkP + ko), cij * 4u) = ap; }
                }
            }
            if (mraw & BFD_REFLECTOR_BIT) {
                F4(wVx, cij * 4u) = 0.f; F4(wVy, cij * 4u) = 0.f; F4(wVz, cij * 4u) = 0.f;
            } else {
                const float *pxx = &sS[b][0][own], *pyy = &sS[b][1][own], *pxy = &sS[b][2][own];
                const float *pxz = &sS[b][3][own], *pyz = &sS[b][4][own];
                float dxSxx = dplus4(pxx[-1], sxx, pxx[1], pxx[2]);
                float dySxy = dminus4(pxy[-2 * LW], pxy[-LW], sxy, pxy[LW]);
                float dzSxz = dminus4(xzm2, xzm1, xz0, xzp1);
                float dxSxy = dminus4(pxy[-2], pxy[-1], sxy, pxy[1]);
                float dySyy = dplus4(pyy[-LW], syy, pyy[LW], pyy[2 * LW]);
                float dzSyz = dminus4(yzm2, yzm1, yz0, yzp1);
                float dxSxz = dminus4(pxz[-2], pxz[-1], xz0, pxz[1]);
                float dySyz = dminus4(pyz[-2 * LW], pyz[-LW], yz0, pyz[LW]);
                float dzSzz = dplus4(zzm1, zz0, zzp1, zzp2);
                if (zi) {
                    const int xi = i < P ? i : i - (N1 - 2 * P);
                    const unsigned q = (unsigned)((kl * N2 + j) * (2 * P) + xi);
                    dxSxx = cpml(d.psi[9], q, d.axH[i], d.bxH[i], dxSxx);
                    dxSxy = cpml(d.psi[12], q, d.axI[i], d.bxI[i], dxSxy);
                    dxSxz = cpml(d.psi[15], q, d.axI[i], d.bxI[i], dxSxz);
                }
                if (zj) {
                    const int yj = j < P ? j : j - (N2 - 2 * P);
                    const unsigned q = (unsigned)((kl * (2 * P) + yj) * N1 + i);
                    dySxy = cpml(d.psi[10], q, d.ayI[j], d.byI[j], dySxy);
                    dySyy = cpml(d.psi[13], q, d.ayH[j], d.byH[j], dySyy);
                    dySyz = cpml(d.psi[16], q, d.ayI[j], d.byI[j], dySyz);
                }
                if (k < P || k >= d.N3 - P) {
                    const int zk = k < P ? k : k - (d.N3 - 2 * P);
                    const unsigned q = (unsigned)(zk * d.plane) + cij;
                    dzSxz = cpml(d.psi[11], q, d.azI[k], d.bzI[k], dzSxz);
                    dzSyz = cpml(d.psi[14], q, d.azI[k], d.bzI[k], dzSyz);
                    dzSzz = cpml(d.psi[17], q, d.azH[k], d.bzH[k], dzSzz);
                }
                const float bxv = 0.5f * (r0 + rx), byv = 0.5f * (r0 + ry), bzv = 0.5f * (r0 + r1);
                ST4(wVx, cij * 4u, vx + bxv * ((dxSxx + dySxy) + dzSxz));
                ST4(wVy, cij * 4u, vy + byv * ((dxSxy + dySyy) + dzSyz));
                ST4(wVz, cij * 4u, vz + bzv * ((dxSxz + dySyz) + dzSzz));
            }
        }
        zzm1 = zz0; zz0 = zzp1; zzp1 = zzp2; zzp2 = nzz;
        xzm2 = xzm1; xzm1 = xz0; xz0 = xzp1; xzp1 = nxz;
        yzm2 = yzm1; yzm1 = yz0; yz0 = yzp1; yzp1 = nyz;
        sxx = nxx; syy = nyy; sxy = nxy;
        ha = nha; hb = nhb;
        vx = nvx; vy = nvy; vz = nvz; av = nav; pv = npv;
        r0 = r1; mraw = mraw1; mraw1 = nm2; mx = nmx; my = nmy;
    }
}

}  // namespace

void bfd_launch_stress_dense(const bfd_dev &d, hipStream_t s, const int4 *runs, int n)
{
    const int tilesX = (d.N1 + TX - 1) / TX;
    BFD_LAUNCH(stress_v2, n, runs, (const unsigned short *)nullptr);
}

void bfd_launch_velocity_dense(const bfd_dev &d, hipStream_t s, const int4 *runs, int n, float *accP, float *pkP)
{
    const int tilesX = (d.N1 + TX - 1) / TX;
    lift([&](auto ACC) { BFD_LAUNCH((velocity_v2<decltype(ACC)::value>), n, accP, pkP, runs); }, accP || pkP);
}
