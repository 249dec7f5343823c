// Solid-run kernels of the tiled path: the runs that hold a solid cell within 2 cells. stress_solid updates the normal stresses (the sparse kernel
// of bfd_kernels_shear.hip has the shear stresses), velocity_solid the velocities; both work cell by cell from the class byte bfd_dev::cls.
// Tile, z-march, LDS staging and the quiet-run helpers: bfd_tile.h; GLOBAL accessors: bfd_device.h. gfx950 only.
#include "bfd_tile.h"
#include "bfd_device.h"

namespace {

// ------------------------------------------------------------------------------------------------
// SOLID runs in the tiled path (variant 3): normal stresses by a pipelined marching kernel (stress_solid), shear
// stresses by a sparse per-cell kernel (stress_shear_sparse) over the list of cells with a solid centre. Each
// kernel is lean (no long dependent chains behind a workgroup barrier), which the monolithic stress_v2 is not.
// Values equal stress_v2's; CPML memory variables of the cross derivatives are advanced only at listed cells
// (they feed nothing else).
// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// SOLID runs, class-predicated kernels (variants 0/3/4). A solid run is a 64 x 8 x (8..16) block that has a solid cell
// within 2 cells, but typically two thirds of its cells are fluid (a thin curved shell cuts through it). Every lane
// therefore works by the class byte of ITS cell (bfd_dev::cls, computed at setup):
//   * fluid cell: the three normal stresses are identical -> only Szz/Rzz is read and written (nobody reads Sxx/Syy of a
//     fluid cell: every reader substitutes Szz there, also across tile borders);
//   * a shear stress entry is loaded only where its edge bit says it is ever updated (elsewhere it is exactly 0).
// Loads are per-lane predicated, so only the lines of the cells that need an array are fetched; the arithmetic is the
// canonical sequence for every lane (zeros / substituted values make it equal to the dense kernels' bit for bit, up
// to the sign of an exact zero). Class bytes run two planes ahead of the state loads they steer.
// ------------------------------------------------------------------------------------------------
template <bool PML>
__device__ __forceinline__ void stress_solid_body(const bfd_dev &d, const int4 &run, int tilesX, float (*sV)[2][LH * LW])
{
    const int N1 = d.N1, N2 = d.N2;
    const int bx = run.x % tilesX, by = run.x / tilesX, kbeg = run.y & 0xFFFF, kend = run.y >> 16;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * TX + tx;
    const int i0 = bx * TX, j0 = by * TY;
    const int i = i0 + tx, j = j0 + ty;
    const bool valid = (i < N1) && (j < N2);
    const long pl = d.plane;
    const int P = d.P;
    const int own = (ty + 2) * LW + tx + 2;
    const unsigned cij = valid ? (unsigned)(j * N1 + i) : 0u;

    HaloTask t; t.lofs = -1; t.ok = false; t.arr = 0; t.gofs = 0;
    if (tid < YT) ytask(tid, 1, i0, j0, N1, N2, t);
    else if (tid < YT + XT) xtask(tid - YT, 0, i0, j0, N1, N2, t);
    const bool has = t.lofs >= 0;
    // the array of the task is uniform per wave (waves 0-3: Vy rows, wave 4: Vx columns): SGPR base + 32-bit byte offset
    const float *ph = __builtin_amdgcn_readfirstlane(t.arr) == 0 ? d.Vx : d.Vy;
    const unsigned hofs = t.ok ? (unsigned)t.gofs * 4u : 0u;
    float *lh = &sV[0][t.arr][has ? t.lofs : 0];
    const float c1 = d.c1;

    const bool zi = PML && valid && (i < P || i >= N1 - P);
    const bool zj = PML && valid && (j < P || j >= N2 - P);
    float ax = 0, bxc = 0, ay = 0, byc = 0, px = 0, py = 0, pz = 0;
    unsigned qx = 0, qy = 0;
    const unsigned dqx = (unsigned)(N2 * 2 * P), dqy = (unsigned)(2 * P * N1);
    if (zi) { ax = d.axI[i]; bxc = d.bxI[i]; qx = (unsigned)((kbeg * N2 + j) * (2 * P) + (i < P ? i : i - (N1 - 2 * P))); px = F4(d.psi[0], (unsigned)(qx) * 4u); }
    if (zj) { ay = d.ayI[j]; byc = d.byI[j]; qy = (unsigned)((kbeg * (2 * P) + (j < P ? j : j - (N2 - 2 * P))) * N1 + i); py = F4(d.psi[1], (unsigned)(qy) * 4u); }
    if (PML) {
        const int kg = d.k0 + kbeg;
        if (valid && (kg < P || kg >= d.N3 - P)) pz = F4(d.psi[2], (unsigned)((unsigned)((kg < P ? kg : kg - (d.N3 - 2 * P)) * d.plane) + cij) * 4u);
    }

    float vx0 = 0, vy0 = 0, vzm2 = 0, vzm1 = 0, vz0 = 0, vzp1 = 0;
    float sxx = 0, syy = 0, szz = 0, rxx = 0, ryy = 0, rzz = 0;
    unsigned mraw = 0, cl = BFD_CLS_FLUID | BFD_CLS_NOMEM, cl1 = BFD_CLS_FLUID | BFD_CLS_NOMEM;
    if (valid) {
        const float *bVz = d.Vz + kbeg * pl;
        cl = U1((d.cls + kbeg * pl), cij); cl1 = U1((d.cls + kbeg * pl + pl), cij);
        vx0 = F4((d.Vx + kbeg * pl), cij * 4u); vy0 = F4((d.Vy + kbeg * pl), cij * 4u);
        vzm2 = F4((bVz - 2 * pl), cij * 4u); vzm1 = F4((bVz - pl), cij * 4u); vz0 = F4(bVz, cij * 4u); vzp1 = F4((bVz + pl), cij * 4u);
        mraw = U2((d.mat + kbeg * pl), cij * 2u);
        szz = F4((d.Szz + kbeg * pl), cij * 4u);
        const bool fl = cl & BFD_CLS_FLUID, mem = !(cl & BFD_CLS_NOMEM) || !fl;
        if (mem) rzz = F4((d.Rzz + kbeg * pl), cij * 4u);
        if (!fl) {
            sxx = F4((d.Sxx + kbeg * pl), cij * 4u); syy = F4((d.Syy + kbeg * pl), cij * 4u);
            rxx = F4((d.Rxx + kbeg * pl), cij * 4u); ryy = F4((d.Ryy + kbeg * pl), cij * 4u);
        }
    }
    float hv = t.ok ? F4(ph + kbeg * pl, hofs) : 0.0f;

    for (int kl = kbeg; kl < kend; kl++) {
        const int b = kl & 1;
        // opaque to loop strength reduction: otherwise every array gets a 64-bit per-lane pointer that is bumped each plane
        // (a VGPR pair per array); this way the plane bases are recomputed on the scalar unit and stay in SGPRs
        const long ko = (long)__builtin_amdgcn_readfirstlane(kl) * pl;
        const int k = d.k0 + kl;
        float nvx = 0, nvy = 0, nvz = 0, nh = 0, nsxx = 0, nsyy = 0, nszz = 0, nrxx = 0, nryy = 0, nrzz = 0, npx = 0, npy = 0, npz = 0;
        unsigned nmraw = 0, ncl2 = BFD_CLS_FLUID | BFD_CLS_NOMEM;
        auto prefetch_next = [&]() {
        if (valid) ncl2 = U1((d.cls + ko + 2 * pl), cij);           // ghost planes make kl+2 addressable
            if (kl + 1 < kend) {
                if (valid) {
                    const bool nfl = cl1 & BFD_CLS_FLUID, nmem = !(cl1 & BFD_CLS_NOMEM) || !nfl;
                    nvx = F4((d.Vx + ko + pl), cij * 4u); nvy = F4((d.Vy + ko + pl), cij * 4u); nvz = F4((d.Vz + ko + 2 * pl), cij * 4u);
                    nmraw = U2((d.mat + ko + pl), cij * 2u);
                    nszz = F4((d.Szz + ko + pl), cij * 4u);
                    if (nmem) nrzz = F4((d.Rzz + ko + pl), cij * 4u);
                    if (!nfl) {
                        nsxx = F4((d.Sxx + ko + pl), cij * 4u); nsyy = F4((d.Syy + ko + pl), cij * 4u);
                        nrxx = F4((d.Rxx + ko + pl), cij * 4u); nryy = F4((d.Ryy + ko + pl), cij * 4u);
                    }
                }
                if (t.ok) nh = F4(ph + ko + pl, hofs);
                if (zi) npx = F4(d.psi[0], (unsigned)(qx + dqx) * 4u);
                if (zj) npy = F4(d.psi[1], (unsigned)(qy + dqy) * 4u);
                const int kn = k + 1;
                if (PML && valid && (kn < P || kn >= d.N3 - P)) npz = F4(d.psi[2], (unsigned)((unsigned)((kn < P ? kn : kn - (d.N3 - 2 * P)) * d.plane) + cij) * 4u);
            }
        };
        sV[b][0][own] = vx0; sV[b][1][own] = vy0;
        if (has) lh[b * (2 * LH * LW)] = hv;
        const int m = mraw & BFD_MAT_MASK;
        const bool fl = cl & BFD_CLS_FLUID, mem = !(cl & BFD_CLS_NOMEM) || !fl;
        float AP = 0, BP = 0, AS2 = 0, BS2 = 0;
        if (valid) { AP = d.AP[m]; if (mem) BP = d.BP[m]; if (!fl) { AS2 = d.AS2[m]; BS2 = d.BS2[m]; } }
        __syncthreads();

        prefetch_next();        // after the barrier (issuing these loads before it was measured slower: 2.37 -> 2.52 ms per step at C2-medium 512^3)
        if (valid) {
            const float *sx = &sV[b][0][own], *sy = &sV[b][1][own];
            float dxVx = dminus4(sx[-2], sx[-1], vx0, sx[1]);
            float dyVy = dminus4(sy[-2 * LW], sy[-LW], vy0, sy[LW]);
            float dzVz = dminus4(vzm2, vzm1, vz0, vzp1);
            if (cl & BFD_CLS_REFL) {
                F4((d.Sxx + ko), cij * 4u) = 0.f; F4((d.Syy + ko), cij * 4u) = 0.f; F4((d.SzzW + ko), cij * 4u) = 0.f;
                F4((d.Rxx + ko), cij * 4u) = 0.f; F4((d.Ryy + ko), cij * 4u) = 0.f; F4((d.RzzW + ko), cij * 4u) = 0.f;
                F4((d.Sxy + ko), cij * 4u) = 0.f; F4((d.Sxz + ko), cij * 4u) = 0.f; F4((d.Syz + ko), cij * 4u) = 0.f;
                F4((d.Rxy + ko), cij * 4u) = 0.f; F4((d.Rxz + ko), cij * 4u) = 0.f; F4((d.Ryz + ko), cij * 4u) = 0.f;
            } else {
                if (zi) { const float pn = bxc * px + ax * dxVx; F4(d.psi[0], (unsigned)(qx) * 4u) = pn; dxVx = dxVx + pn; }
                if (zj) { const float pn = byc * py + ay * dyVy; F4(d.psi[1], (unsigned)(qy) * 4u) = pn; dyVy = dyVy + pn; }
                if (PML && (k < P || k >= d.N3 - P)) {
                    const float pn = d.bzI[k] * pz + d.azI[k] * dzVz;
                    F4(d.psi[2], (unsigned)((unsigned)((k < P ? k : k - (d.N3 - 2 * P)) * d.plane) + cij) * 4u) = pn;
                    dzVz = dzVz + pn;
                }
                const float sXY = dxVx + dyVy;
                const float div = sXY + dzVz;
                if (fl) {               // fluid cell: one copy of the identical normal stresses
                    float val;
                    if (!mem) val = szz + AP * div;
                    else {
                        const float rn = c1 * rzz - BP * div;
                        val = szz + (AP * div + 0.5f * (rzz + rn));
                        ST4((d.RzzW + ko), cij * 4u, rn);
                    }
                    ST4((d.SzzW + ko), cij * 4u, val);
                } else {
                    const float sYZ = dyVy + dzVz, sXZ = dxVx + dzVz;
                    float rn;
                    rn = c1 * rxx - (BP * div - BS2 * sYZ);
                    ST4((d.Sxx + ko), cij * 4u, sxx + ((AP * div - AS2 * sYZ) + 0.5f * (rxx + rn))); ST4((d.Rxx + ko), cij * 4u, rn);
                    rn = c1 * ryy - (BP * div - BS2 * sXZ);
                    ST4((d.Syy + ko), cij * 4u, syy + ((AP * div - AS2 * sXZ) + 0.5f * (ryy + rn))); ST4((d.Ryy + ko), cij * 4u, rn);
                    rn = c1 * rzz - (BP * div - BS2 * sXY);
                    ST4((d.SzzW + ko), cij * 4u, szz + ((AP * div - AS2 * sXY) + 0.5f * (rzz + rn))); ST4((d.RzzW + ko), cij * 4u, rn);
                }
            }
        }
        vx0 = nvx; vy0 = nvy;
        vzm2 = vzm1; vzm1 = vz0; vz0 = vzp1; vzp1 = nvz;
        hv = nh; mraw = nmraw; cl = cl1; cl1 = ncl2;
        sxx = nsxx; syy = nsyy; szz = nszz; rxx = nrxx; ryy = nryy; rzz = nrzz;
        px = npx; py = npy; pz = npz; qx += dqx; qy += dqy;
    }
}

constexpr int SOLID_STRESS_WAVES_PER_SIMD = 4;
// (a GLOBAL / branch-free-prefetch body like velocity_solid_body_g was built and measured 1 % slower, 0.308-0.311 against 0.305 ms at the shear medium
// 512^3 -- this kernel is at the rate of the bytes it moves; removed; profiles/r4/experiment_solid_kernels_prefetch.txt)
__global__ __launch_bounds__(NTHREADS, SOLID_STRESS_WAVES_PER_SIMD) void stress_solid(bfd_dev d, int tilesX, int nblocks, const int *__restrict__ xmap, const int4 *__restrict__ runs)
{
    __shared__ float sV[2][2][LH * LW];
    const int ri = run_index(nblocks, xmap);
    if (ri < 0) return;
    const int4 run = runs[ri];
    if (run.z & 8) stress_solid_body<true>(d, run, tilesX, sV);
    else stress_solid_body<false>(d, run, tilesX, sV);
}

// ------------------------------------------------------------------------------------------------
// The solid-run kernels again with GLOBAL loads and a prefetch WITHOUT branches (round 4). In the bodies above every predicated
// load of the next plane sits in its own basic block and the loads are FLAT: the first LDS wait of an iteration (lgkmcnt, which
// flat loads count on) drains the whole prefetch, so an iteration is one memory round trip followed by the arithmetic, nothing
// overlaps. Here a load whose class predicate is off reads the first dword of its plane instead (one line every lane shares:
// an L1 hit, no traffic) and its result is replaced by 0, so every iteration issues the same loads in the same order, the
// compiler counts them (vmcnt(n) waits) and the plane k+1 loads stay in flight across the arithmetic of plane k.
// Same values, same arithmetic: bit-identical. The accessors (GL4, GLP, ...) are bfd_device.h's.
// ------------------------------------------------------------------------------------------------
// one halo value: SUBST (Sxx / Syy halos): Szz where the halo cell is fluid, the array itself otherwise; else a shear array where its
// edge bit is set, 0 elsewhere. One load on every path: the plane base is chosen per lane, the offset falls back to dword 0.
__device__ __forceinline__ float halo_value_g(const float *base, const float *alt, bool subst, unsigned bit, unsigned hc, unsigned off4, bool ok)
{
    const bool fluid = (hc & BFD_CLS_FLUID) != 0;
    const bool take = ok && (subst || (hc & bit));
    const unsigned long long pb = (unsigned long long)guni(base), pa = (unsigned long long)guni(alt);
    const unsigned long long pp = (subst && fluid) ? pa : pb;
    const float v = *(BFD_GLOBAL const float *)(pp + (take ? off4 : 0u));
    return take ? v : 0.0f;
}

// compact form: the halo cell's value comes from Szz (SUBST and fluid), from the compact array at byte offset e4 (SUBST: listed cell, else: edge bit
// set), or is 0
__device__ __forceinline__ float halo_value_c(const float *cbase, const float *alt, bool subst, unsigned bit, unsigned hc, unsigned off4, unsigned e4, bool ok)
{
    const bool fromAlt = subst && (hc & BFD_CLS_FLUID) != 0;
    const bool take = ok && (fromAlt || (subst ? css_listed(hc) : (hc & bit) != 0));
    const unsigned long long pp = fromAlt ? (unsigned long long)guni(alt) : (unsigned long long)guni(cbase);
    const float v = *(BFD_GLOBAL const float *)(pp + (take ? (fromAlt ? off4 : e4) : 0u));
    return take ? v : 0.0f;
}

// CSS: Sxx, Syy and the three shear stresses of listed cells come from the compact arrays (bfd_dev::cssRow). Entry of a cell = base of its
// row (per plane; own row and halo row: one scalar each, the halo columns: one table word per lane) + the listed cells before it in the row;
// the bases a plane needs are fetched one iteration ahead, so the prefetch still issues without waiting for anything.
// WHOLE (compact form only): the engine holds a whole domain and updates V in place -- the stores share the plane bases of the loads and a
// ghost plane's Sxz / Syz are the zeros nobody ever wrote, so the full-volume fallback and its two array bases go: ten scalar registers
// fewer in a kernel that spilled twelve (each spilled one comes back through a v_readlane in every plane, and scalar address arithmetic
// that no longer fits turns into vector instructions + readfirstlane). 0.400 -> 0.384 ms at the shear medium 512^3; a further flavour without
// the peak accumulator (six spilled registers less) changed nothing measurable and was not kept. profiles/r5/velocity_solid_scalar_registers.txt
template <bool ACC, bool PML, bool CSS, bool WHOLE = false, bool QUIET = false>
__device__ __forceinline__ void velocity_solid_body_g(const bfd_dev &d, const int4 &run, int tilesX, float (*sS)[5][LH * LW],
                                                      float *__restrict__ accP, float *__restrict__ pkP)
{
    unsigned nzb = 0u;          // QUIET: bits of everything stored
    const int N1 = d.N1, N2 = d.N2;
    const int bx = run.x % tilesX, by = run.x / tilesX;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * TX + tx;
    const int wv = __builtin_amdgcn_readfirstlane(ty);      // wave index = tile row (uniform)
    const int i0 = bx * TX, j0 = by * TY;
    const int i = i0 + tx, j = j0 + ty;
    const bool valid = (i < N1) && (j < N2);
    const long pl = d.plane;
    const int kbeg = run.y & 0xFFFF, kend = run.y >> 16;
    const int P = d.P;
    const int own = (ty + 2) * LW + tx + 2;
    const unsigned cij = valid ? (unsigned)(j * N1 + i) : 0u;
    const unsigned c4 = cij * 4u, c2 = cij * 2u;
    const bool hasX = valid && i + 1 < N1, hasY = valid && j + 1 < N2;
    const unsigned cx2 = c2 + (hasX ? 2u : 0u), cy2 = c2 + (hasY ? (unsigned)N1 * 2u : 0u);
    const bool accA = ACC && accP != nullptr, accK = ACC && pkP != nullptr;

    HaloTask ta, tb;
    const int arrA = wv < 4 ? 1 : 2;
    ytask(tid & 255, arrA, i0, j0, N1, N2, ta);
    const int arrB = wv < 4 ? 4 : (wv == 4 ? 0 : (wv == 5 ? 2 : 3));
    if (wv < 4) ytask(tid, 4, i0, j0, N1, N2, tb);
    else if (wv < 7 && tx < XT) xtask(tx, arrB, i0, j0, N1, N2, tb);
    else { tb.lofs = -1; tb.ok = false; tb.arr = arrB; tb.gofs = 0; }
    const float *baseA = arrA == 1 ? d.Syy : d.Sxy;
    const float *baseB = arrB == 4 ? d.Syz : (arrB == 0 ? d.Sxx : (arrB == 2 ? d.Sxy : d.Sxz));
    const bool substA = arrA == 1, substB = arrB == 0;
    const unsigned bitA = BFD_CLS_EXY, bitB = arrB == 4 ? BFD_CLS_EYZ : (arrB == 2 ? BFD_CLS_EXY : BFD_CLS_EXZ);
    const unsigned offA = ta.ok ? (unsigned)ta.gofs : 0u, offB = tb.ok ? (unsigned)tb.gofs : 0u;
    float *la = &sS[0][ta.arr][ta.lofs];
    float *lb = &sS[0][tb.arr][tb.lofs < 0 ? 0 : tb.lofs];
    const bool hasB = tb.lofs >= 0;
    const int bufStride = 5 * LH * LW;

    const bool zi = PML && valid && (i < P || i >= N1 - P);
    const bool zj = PML && valid && (j < P || j >= N2 - P);
    const bool inner = valid && i >= d.ND && i < N1 - d.ND && j >= d.ND && j < N2 - d.ND;

    // compact solid state: row table of the own row and of the halo row of task A (waves 0-3: also of task B), planes as a scalar stride;
    // the halo-column lanes (waves 4-6, lanes 0..31) read their table word themselves: cells i0-2, i0-1 count back from the base of this
    // tile's row, cells i0+64, i0+65 count on from the base of the next tile's
    const long rs = CSS ? (long)N2 * d.cssStride : 0;
    const unsigned *rowp = nullptr, *rowpA = nullptr;
    const float *cbaseA = nullptr, *cbaseB = nullptr;
    unsigned rtOfs = 0;
    const int cc = tx & 3;
    if (CSS) {
        rowp = d.cssRow + ((long)2 * N2 + min(j0 + wv, N2 - 1)) * d.cssStride + bx;
        const int rA = wv & 3, gjA = j0 - 2 + (rA < 2 ? rA : TY + rA);
        rowpA = d.cssRow + ((long)2 * N2 + min(max(gjA, 0), N2 - 1)) * d.cssStride + bx;
        cbaseA = arrA == 1 ? d.cSyy : d.cSxy;
        cbaseB = arrB == 4 ? d.cSyz : (arrB == 0 ? d.cSxx : (arrB == 2 ? d.cSxy : d.cSxz));
        if (wv >= 4 && wv < 7 && tx < XT) rtOfs = (unsigned)(((2 * N2 + min(j0 + (tx >> 2), N2 - 1)) * d.cssStride + bx + (cc >= 2 ? 1 : 0)) * 4);
    }
    // a scalar load (constant address space, wave-uniform address): it returns on lgkmcnt, so nothing in the prefetch below waits for it -- as a vector
    // load + readfirstlane the compiler put an s_waitcnt vmcnt in the middle of the prefetch section (a second memory round trip per plane)
    auto rowbase = [&](const unsigned *rp, int plane) { return *(const __attribute__((address_space(4))) unsigned *)(unsigned long long)(rp + plane * rs); };
    // entry of this lane's halo cell of task B: waves 0-3 a row like task A, waves 4-6 the columns
    auto entryB = [&](unsigned rbRow, unsigned rbx, unsigned hc) {
        const bool li = tb.ok && css_listed(hc);
        if (wv < 4) return rbRow + css_rank(li);
        const unsigned long long lb = __ballot(li);
        const unsigned pb = (unsigned)(lb >> ((cc == 0 ? tx + 1 : tx - 1) & 63)) & 1u;
        return cc < 2 ? rbx - 1u - (cc == 0 ? pb : 0u) : rbx + (cc == 3 ? pb : 0u);
    };
    unsigned rbB = BFD_CSS_NONE, rbC = BFD_CSS_NONE, rbA = 0, rbx = 0;      // row bases: own row at planes kl+1 / kl+2, halo row and column word at plane kl+1

    float zzm1 = 0, zz0 = 0, zzp1 = 0, zzp2 = 0, xzm2 = 0, xzm1 = 0, xz0 = 0, xzp1 = 0, yzm2 = 0, yzm1 = 0, yz0 = 0, yzp1 = 0;
    unsigned cB = BFD_CLS_FLUID, cC = BFD_CLS_FLUID;
    {
        const float *bzz = d.Szz + kbeg * pl, *bxz = d.Sxz + kbeg * pl, *byz = d.Syz + kbeg * pl;
        const uint8_t *bc = d.cls + kbeg * pl;
        unsigned cm2 = BFD_CLS_FLUID, cm1 = BFD_CLS_FLUID, c0 = BFD_CLS_FLUID;
        if (valid) { cm2 = GL1(bc - 2 * pl, cij); cm1 = GL1(bc - pl, cij); c0 = GL1(bc, cij); cB = GL1(bc + pl, cij); cC = GL1(bc + 2 * pl, cij); }
        zzm1 = GLP(bzz - pl, c4, valid); zz0 = GLP(bzz, c4, valid); zzp1 = GLP(bzz + pl, c4, valid); zzp2 = GLP(bzz + 2 * pl, c4, valid);
        const bool fl0 = (c0 & BFD_CLS_FLUID) != 0;
        float sxx, syy, sxy;
        if (CSS) {
            const unsigned rm2 = rowbase(rowp, kbeg - 2), rm1 = rowbase(rowp, kbeg - 1), rb0 = rowbase(rowp, kbeg);
            rbB = rowbase(rowp, kbeg + 1); rbC = rowbase(rowp, kbeg + 2);
            const unsigned em2 = (rm2 + css_rank(css_listed(cm2))) * 4u, em1 = (rm1 + css_rank(css_listed(cm1))) * 4u;
            const unsigned e0 = (rb0 + css_rank(css_listed(c0))) * 4u, e1 = (rbB + css_rank(css_listed(cB))) * 4u;
            // a ghost plane (row base BFD_CSS_NONE) has no compact values: its Sxz / Syz come out of the full-volume arrays, where a Z-neighbour's
            // planes arrive (the sparse kernel keeps full-volume copies of the planes a neighbour reads); zeros at the ends of the domain
            const bool gm2 = rm2 != BFD_CSS_NONE, gm1 = rm1 != BFD_CSS_NONE, g1 = rbB != BFD_CSS_NONE;
            if (WHOLE) {        // a ghost plane of a whole domain: zeros
                xzm2 = GLP(d.cSxz, em2, gm2 && (cm2 & BFD_CLS_EXZ) != 0); xzm1 = GLP(d.cSxz, em1, gm1 && (cm1 & BFD_CLS_EXZ) != 0);
                xz0 = GLP(d.cSxz, e0, (c0 & BFD_CLS_EXZ) != 0); xzp1 = GLP(d.cSxz, e1, g1 && (cB & BFD_CLS_EXZ) != 0);
                yzm2 = GLP(d.cSyz, em2, gm2 && (cm2 & BFD_CLS_EYZ) != 0); yzm1 = GLP(d.cSyz, em1, gm1 && (cm1 & BFD_CLS_EYZ) != 0);
                yz0 = GLP(d.cSyz, e0, (c0 & BFD_CLS_EYZ) != 0); yzp1 = GLP(d.cSyz, e1, g1 && (cB & BFD_CLS_EYZ) != 0);
            } else {
            xzm2 = GLP(gm2 ? d.cSxz : bxz - 2 * pl, gm2 ? em2 : c4, (cm2 & BFD_CLS_EXZ) != 0); xzm1 = GLP(gm1 ? d.cSxz : bxz - pl, gm1 ? em1 : c4, (cm1 & BFD_CLS_EXZ) != 0);
            xz0 = GLP(d.cSxz, e0, (c0 & BFD_CLS_EXZ) != 0); xzp1 = GLP(g1 ? d.cSxz : bxz + pl, g1 ? e1 : c4, (cB & BFD_CLS_EXZ) != 0);
            yzm2 = GLP(gm2 ? d.cSyz : byz - 2 * pl, gm2 ? em2 : c4, (cm2 & BFD_CLS_EYZ) != 0); yzm1 = GLP(gm1 ? d.cSyz : byz - pl, gm1 ? em1 : c4, (cm1 & BFD_CLS_EYZ) != 0);
            yz0 = GLP(d.cSyz, e0, (c0 & BFD_CLS_EYZ) != 0); yzp1 = GLP(g1 ? d.cSyz : byz + pl, g1 ? e1 : c4, (cB & BFD_CLS_EYZ) != 0);
            }
            sxx = GLP(d.cSxx, e0, css_listed(c0)); syy = GLP(d.cSyy, e0, css_listed(c0));
            sxy = GLP(d.cSxy, e0, (c0 & BFD_CLS_EXY) != 0);
        } else {
            xzm2 = GLP(bxz - 2 * pl, c4, valid && (cm2 & BFD_CLS_EXZ)); xzm1 = GLP(bxz - pl, c4, valid && (cm1 & BFD_CLS_EXZ));
            xz0 = GLP(bxz, c4, valid && (c0 & BFD_CLS_EXZ)); xzp1 = GLP(bxz + pl, c4, valid && (cB & BFD_CLS_EXZ));
            yzm2 = GLP(byz - 2 * pl, c4, valid && (cm2 & BFD_CLS_EYZ)); yzm1 = GLP(byz - pl, c4, valid && (cm1 & BFD_CLS_EYZ));
            yz0 = GLP(byz, c4, valid && (c0 & BFD_CLS_EYZ)); yzp1 = GLP(byz + pl, c4, valid && (cB & BFD_CLS_EYZ));
            sxx = GLP(d.Sxx + kbeg * pl, c4, valid && !fl0); syy = GLP(d.Syy + kbeg * pl, c4, valid && !fl0);
            sxy = GLP(d.Sxy + kbeg * pl, c4, valid && (c0 & BFD_CLS_EXY));
        }
        if (valid && fl0) { sxx = zz0; syy = zz0; }
        const int bo0 = (kbeg & 1) * bufStride;
        sS[0][0][bo0 + own] = sxx; sS[0][1][bo0 + own] = syy; sS[0][2][bo0 + own] = sxy; sS[0][3][bo0 + own] = xz0; sS[0][4][bo0 + own] = yz0;
    }
    float r0 = 0;
    unsigned mraw = 0, mraw1 = 0, mx = 0, my = 0;
    if (valid) {
        const uint16_t *bM = d.mat + kbeg * pl;
        mraw = GL2(bM, c2); mraw1 = GL2(bM + pl, c2); mx = GL2(bM, cx2); my = GL2(bM, cy2);
        r0 = d.invRho[mraw & BFD_MAT_MASK];
    }
    unsigned hcA = 0, hcB = 0;
    {
        unsigned h0A = 0, h0B = 0;
        if (ta.ok) { h0A = GL1(d.cls + kbeg * pl, offA); hcA = GL1(d.cls + kbeg * pl + pl, offA); }
        if (tb.ok) { h0B = GL1(d.cls + kbeg * pl, offB); hcB = GL1(d.cls + kbeg * pl + pl, offB); }
        float ha, hb;
        if (CSS) {
            const unsigned ra0 = rowbase(rowpA, kbeg);
            const unsigned rx0 = *(BFD_GLOBAL const unsigned *)((BFD_GLOBAL const char *)guni(d.cssRow + kbeg * rs) + pin(rtOfs));
            rbA = rowbase(rowpA, kbeg + 1);
            rbx = *(BFD_GLOBAL const unsigned *)((BFD_GLOBAL const char *)guni(d.cssRow + (kbeg + 1) * rs) + pin(rtOfs));
            const unsigned ea = ra0 + css_rank(ta.ok && css_listed(h0A)), eb = entryB(ra0, rx0, h0B);
            ha = halo_value_c(cbaseA, d.Szz + kbeg * pl, substA, bitA, h0A, offA * 4u, ea * 4u, ta.ok);
            hb = halo_value_c(cbaseB, d.Szz + kbeg * pl, substB, bitB, h0B, offB * 4u, eb * 4u, tb.ok);
        } else {
            ha = halo_value_g(baseA + kbeg * pl, d.Szz + kbeg * pl, substA, bitA, h0A, offA * 4u, ta.ok);
            hb = halo_value_g(baseB + kbeg * pl, d.Szz + kbeg * pl, substB, bitB, h0B, offB * 4u, tb.ok);
        }
        la[(kbeg & 1) * bufStride] = ha;
        if (hasB) lb[(kbeg & 1) * bufStride] = hb;
    }

    for (int kl = kbeg; kl < kend; kl++) {
        const int b = kl & 1;
        const long ko = (long)__builtin_amdgcn_readfirstlane(kl) * pl;
        const int k = d.k0 + kl;
        const int bn = (b ^ 1) * bufStride;     // buffer of plane kl+1
        // Round 6: the array bases are re-read from the kernel argument segment (d is the kernel's first argument; scalar loads, in the scalar cache
        // after the first plane) at three points of every plane instead of being held in scalar registers across the loop: ~19 pairs + ~10 lane
        // masks did not fit (17 scalars spilled to vector lanes, scalar address arithmetic done in vector registers). Spills 17 -> 8 (accumulating
        // flavour) / 27 -> 0 (Z-slab flavour) / 96 -> 34 (absorbing layer), 92 -> 80-82 vector registers: with the bound of 6 waves per SIMD every
        // flavour outside the layer fits 80 registers WITHOUT scratch (the round-5 build spilled 6-7 registers to scratch there and lost 12 %), so
        // three workgroups share a CU instead of two: 0.386 -> 0.362 ms at the shear medium 512^3 (the reload alone, at 5 waves: 0.386).
        // profiles/r6/velocity_solid_bases_reloaded.txt
        const __attribute__((address_space(4))) bfd_dev *kd = (const __attribute__((address_space(4))) bfd_dev *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kd));
        // own V and sums of this plane (before the barrier), then, after it, everything plane kl+1 needs: always the same loads
        const float vx = GLNT(kd->Vx + ko, c4), vy = GLNT(kd->Vy + ko, c4), vz = GLNT(kd->Vz + ko, c4);
        float av = 0, pv = 0;
        if (accA) av = GLNT(accP + ko, c4);
        if (accK) pv = GL4(pkP + ko, c4);
        float r1 = 0, rx = 0, ry = 0;
        if (valid) {
            r1 = kd->invRho[mraw1 & BFD_MAT_MASK];       // plane kl+1, becomes r0 of the next iteration
            rx = kd->invRho[mx & BFD_MAT_MASK];
            ry = kd->invRho[my & BFD_MAT_MASK];
        }
        __syncthreads();
        asm volatile("" : "+s"(kd));

        // The raw values are not touched before the end of the iteration (their class masks are applied there): nothing between
        // here and the staging waits for them.
        const bool more = kl + 1 < kend;                // uniform
        const unsigned nm2 = GL2(kd->mat + ko + 2 * pl, c2);                       // ghost planes make kl+2 addressable
        const unsigned nc3raw = GL1(kd->cls + ko + (kl + 2 < kend ? 3 : 2) * pl, cij);
        const bool bfl = (cB & BFD_CLS_FLUID) != 0;
        const long kn = more ? pl : 0;                  // the last iteration reads its own plane again (addressable, unused)
        const float nzzR = GL4(kd->Szz + ko + 2 * pl + kn, c4);
        bool pXZ, pYZ, pNN, pXY, takeA, takeB;
        float nxzR, nyzR, nxxR, nyyR, nxyR, nhaR, nhbR;
        unsigned nrb = BFD_CSS_NONE, nrbA = 0, nrbx = 0;
        if (CSS) {
            // entries of the own cell in planes kl+1 (in-plane values) and kl+2 (Sxz, Syz); the bases of the next iteration
            const bool lB = css_listed(cB);
            const unsigned eB = (rbB + css_rank(lB)) * 4u, eC = (rbC + css_rank(css_listed(cC))) * 4u;
            nrb = rowbase(rowp, kl + (kl + 2 < kend ? 3 : 2));
            nrbA = rowbase(rowpA, kl + (more ? 2 : 1));
            nrbx = *(BFD_GLOBAL const unsigned *)((BFD_GLOBAL const char *)guni(kd->cssRow + (kl + (more ? 2 : 1)) * rs) + pin(rtOfs));
            const bool gC = rbC != BFD_CSS_NONE;        // plane kl+2 may be the ghost plane nk: full-volume arrays there (uniform choice)
            pXZ = more && (cC & BFD_CLS_EXZ) && (!WHOLE || gC); pYZ = more && (cC & BFD_CLS_EYZ) && (!WHOLE || gC);
            pNN = more && lB; pXY = more && (cB & BFD_CLS_EXY);
            const unsigned eZ = (WHOLE || gC) ? eC : c4;
            if (WHOLE) { nxzR = GL4(kd->cSxz, pXZ ? eZ : 0u); nyzR = GL4(kd->cSyz, pYZ ? eZ : 0u); }
            else { nxzR = GL4(gC ? kd->cSxz : kd->Sxz + ko + pl + kn, pXZ ? eZ : 0u); nyzR = GL4(gC ? kd->cSyz : kd->Syz + ko + pl + kn, pYZ ? eZ : 0u); }
            nxxR = GL4(kd->cSxx, pNN ? eB : 0u); nyyR = GL4(kd->cSyy, pNN ? eB : 0u); nxyR = GL4(kd->cSxy, pXY ? eB : 0u);
            const unsigned eA = (rbA + css_rank(ta.ok && css_listed(hcA))) * 4u, eH = entryB(rbA, rbx, hcB) * 4u;
            const bool flA = substA && (hcA & BFD_CLS_FLUID), flB = substB && (hcB & BFD_CLS_FLUID);
            takeA = more && ta.ok && (flA || (substA ? css_listed(hcA) : (hcA & bitA) != 0));
            takeB = more && tb.ok && (flB || (substB ? css_listed(hcB) : (hcB & bitB) != 0));
            const unsigned long long paA = (unsigned long long)guni(kd->Szz + ko + kn);
            nhaR = *(BFD_GLOBAL const float *)((flA ? paA : (unsigned long long)guni(cbaseA)) + (takeA ? (flA ? offA * 4u : eA) : 0u));
            nhbR = *(BFD_GLOBAL const float *)((flB ? paA : (unsigned long long)guni(cbaseB)) + (takeB ? (flB ? offB * 4u : eH) : 0u));
        } else {
            pXZ = more && valid && (cC & BFD_CLS_EXZ); pYZ = more && valid && (cC & BFD_CLS_EYZ);
            pNN = more && valid && !bfl; pXY = more && valid && (cB & BFD_CLS_EXY);
            takeA = more && ta.ok && (substA || (hcA & bitA)); takeB = more && tb.ok && (substB || (hcB & bitB));
            nxzR = GL4(kd->Sxz + ko + pl + kn, pXZ ? c4 : 0u);
            nyzR = GL4(kd->Syz + ko + pl + kn, pYZ ? c4 : 0u);
            nxxR = GL4(kd->Sxx + ko + kn, pNN ? c4 : 0u);
            nyyR = GL4(kd->Syy + ko + kn, pNN ? c4 : 0u);
            nxyR = GL4(kd->Sxy + ko + kn, pXY ? c4 : 0u);
            const unsigned long long pbA = (unsigned long long)guni(baseA + ko + kn), paA = (unsigned long long)guni(kd->Szz + ko + kn);
            const unsigned long long pbB = (unsigned long long)guni(baseB + ko + kn);
            nhaR = *(BFD_GLOBAL const float *)(((substA && (hcA & BFD_CLS_FLUID)) ? paA : pbA) + (takeA ? offA * 4u : 0u));
            nhbR = *(BFD_GLOBAL const float *)(((substB && (hcB & BFD_CLS_FLUID)) ? paA : pbB) + (takeB ? offB * 4u : 0u));
        }
        const unsigned nmx = GL2(kd->mat + ko + kn, cx2), nmy = GL2(kd->mat + ko + kn, cy2);
        const unsigned nhcA = GL1(kd->cls + ko + pl + kn, offA), nhcB = GL1(kd->cls + ko + pl + kn, offB);

        asm volatile("" : "+s"(kd));
        float *wVx = (WHOLE ? kd->Vx : kd->VxW) + ko, *wVy = (WHOLE ? kd->Vy : kd->VyW) + ko, *wVz = (WHOLE ? kd->Vz : kd->VzW) + ko;
        if (valid) {
            const float sxx = sS[b][0][own], syy = sS[b][1][own], sxy = sS[b][2][own];
            if (ACC) {
                if (inner && k >= d.ND && k < d.N3 - d.ND) {
                    const float s = (sxx + syy) + zz0;
                    const float p = -s * (1.0f / 3.0f);
                    if (accA) GS4(accP + ko, c4, av + p * p);
                    if (accK) { const float ap = fabsf(p); if (ap > pv) GS4(pkP + ko, c4, ap); }
                }
            }
            if (mraw & BFD_REFLECTOR_BIT) {
                GS4(wVx, c4, 0.f); GS4(wVy, c4, 0.f); GS4(wVz, c4, 0.f);
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
                if (PML && (k < P || k >= d.N3 - P)) {
                    const int zk = k < P ? k : k - (d.N3 - 2 * P);
                    const unsigned q = (unsigned)(zk * d.plane) + cij;
                    dzSxz = cpml(d.psi[11], q, d.azI[k], d.bzI[k], dzSxz);
                    dzSyz = cpml(d.psi[14], q, d.azI[k], d.bzI[k], dzSyz);
                    dzSzz = cpml(d.psi[17], q, d.azH[k], d.bzH[k], dzSzz);
                }
                const float bxv = 0.5f * (r0 + rx), byv = 0.5f * (r0 + ry), bzv = 0.5f * (r0 + r1);
                { const float w = vx + bxv * ((dxSxx + dySxy) + dzSxz); GS4NT(wVx, c4, w); if (QUIET) nzb |= fbits(w); }
                { const float w = vy + byv * ((dxSxy + dySyy) + dzSyz); GS4NT(wVy, c4, w); if (QUIET) nzb |= fbits(w); }
                { const float w = vz + bzv * ((dxSxz + dySyz) + dzSzz); GS4NT(wVz, c4, w); if (QUIET) nzb |= fbits(w); }
            }
        }
        // masks of the prefetched values, queues, staging of plane kl+1
        const float nzz = (more && valid) ? nzzR : 0.0f, nxz = pXZ ? nxzR : 0.0f, nyz = pYZ ? nyzR : 0.0f;
        const float nxx = pNN ? nxxR : ((more && valid && bfl) ? zzp1 : 0.0f), nyy = pNN ? nyyR : ((more && valid && bfl) ? zzp1 : 0.0f);
        const float nxy = pXY ? nxyR : 0.0f, nha = takeA ? nhaR : 0.0f, nhb = takeB ? nhbR : 0.0f;
        const unsigned nc3 = (kl + 2 < kend && valid) ? nc3raw : (unsigned)BFD_CLS_FLUID;
        zzm1 = zz0; zz0 = zzp1; zzp1 = zzp2; zzp2 = nzz;
        xzm2 = xzm1; xzm1 = xz0; xz0 = xzp1; xzp1 = nxz;
        yzm2 = yzm1; yzm1 = yz0; yz0 = yzp1; yzp1 = nyz;
        sS[0][0][bn + own] = nxx; sS[0][1][bn + own] = nyy; sS[0][2][bn + own] = nxy; sS[0][3][bn + own] = xz0; sS[0][4][bn + own] = yz0;
        la[bn] = nha;
        if (hasB) lb[bn] = nhb;
        hcA = nhcA; hcB = nhcB;
        r0 = r1; mraw = mraw1; mraw1 = nm2; mx = nmx; my = nmy;
        cB = cC; cC = nc3;
        if (CSS) { rbB = rbC; rbC = nrb; rbA = nrbA; rbx = nrbx; }
    }
    if (QUIET) run_mark_active(d, run.x % tilesX, run.x / tilesX, run.y & 0xFFFF, run.y >> 16, nzb);
}

// two kernels (the absorbing-layer flavour needs ~18 registers more and would spill inside a common one); the solid run
// list keeps the runs that touch the layer at its two ends (bfd_tiles::nSolidBP / nSolidIP)
constexpr int SOLID_VELOCITY_WAVES_PER_SIMD = 6;      // 80 registers = three workgroups per CU; no scratch since the bases are re-read per plane (round 6). The absorbing-layer flavour needs 106 registers and gets 4
template <bool ACC, bool PML, bool CSS, bool WHOLE = false, bool QUIET = false>
__global__ __launch_bounds__(NTHREADS, PML ? 4 : SOLID_VELOCITY_WAVES_PER_SIMD) void velocity_solid(bfd_dev d, int tilesX, int nblocks, const int *__restrict__ xmap,
                                                        float *__restrict__ accP, float *__restrict__ pkP,
                                                        const int4 *__restrict__ runs)
{
    __shared__ float sS[2][5][LH * LW];
    const int ri = run_index(nblocks, xmap);
    if (ri < 0) return;
    const int4 run = runs[ri];
    if (QUIET && run_all_quiet(d, run.x % tilesX, run.x / tilesX, run.y & 0xFFFF, run.y >> 16)) return;
    // GLOBAL loads, prefetch without branches: since round 4 (0.405 -> 0.378 ms at the shear medium 512^3 against the FLAT body, removed)
    velocity_solid_body_g<ACC, PML, CSS, WHOLE, QUIET>(d, run, tilesX, sS, accP, pkP);
}

}  // namespace

void bfd_launch_stress_solid(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, const int4 *runs, int cnt, int m)
{
    const int tilesX = (d.N1 + TX - 1) / TX;
    BFD_LAUNCH_X(stress_solid, cnt, m, runs);
}

// pml: the runs touch the absorbing layer (the other kernel of the two); part as for the half-step (bfd_kernels_tiled.hip)
void bfd_launch_velocity_solid(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, int part, bool pml, const int4 *runs, int cnt, int m, float *accP, float *pkP)
{
    const int tilesX = (d.N1 + TX - 1) / TX;
    const bool acc = accP || pkP;
    // CSS: compact solid state; WHOLE: V updated in place on a whole domain, or the interior runs of a Z-slab (part 2 of a split half-step: they
    // reach no ghost plane); QUIET: runs without activity return at entry (production calls). WHOLE and QUIET exist in the compact form only.
    const bool css = d.cssRow != nullptr, inPlace = css && d.VxW == d.Vx && d.VyW == d.Vy && d.VzW == d.Vz;
    const bool whole = inPlace && ((d.k0 == 0 && d.nk == d.N3) || part == 2), quiet = inPlace && d.act != nullptr;
    lift([&](auto ACC, auto PML, auto CSS, auto WHOLE, auto QUIET) {
        constexpr bool C = decltype(CSS)::value, W = decltype(WHOLE)::value, Q = decltype(QUIET)::value;
        if constexpr (C || (!W && !Q))
            BFD_LAUNCH_X((velocity_solid<decltype(ACC)::value, decltype(PML)::value, C, W, Q>), cnt, m, accP, pkP, runs);
    }, acc, pml, css, whole, quiet);
}
