// Fluid-run kernels of the tiled path: the stress and the velocity half-step of the runs that hold no solid cell within 2 cells (and, with the
// compact solid state, Szz / Rzz of every run). One launch per half-step covers all of them; the workgroup switches on its run's flags into
// the body specialised for it (stress_fluid_body, velocity_fluid_body). Also the flush of the paired Pressure accumulation.
// Tile, z-march, LDS staging and the quiet-run helpers: bfd_tile.h. gfx950 only.
#include "bfd_tile.h"
#include "bfd_device.h"

namespace {

constexpr int FLUID_WAVES_PER_SIMD = 8;      // 57 / 64 VGPRs since the plane bases live in SGPRs (uni()); round 1, with 64-bit per-lane addresses: 6 -> 61 Gvoxel-steps/s, 8 (spills) -> 47
constexpr int VELOCITY_FLUID_WAVES_PER_SIMD = FLUID_WAVES_PER_SIMD;     // of velocity_fluid alone (64 VGPRs + one 8-byte spill at 8 waves; at 7 no spill): A/B in profiles/r4/

// ------------------------------------------------------------------------------------------------
// FLUID tiles: no solid cell within the tile grown by 2 cells in every direction. There
//   * shear stresses and their memory variables are never updated (a shear update needs the 4
//     cells around an edge to be solid), so they stay exactly 0 and need not be read;
//   * the three normal stresses (and their memory variables) receive the same update
//     (AS2 = BS2 = 0 in a fluid cell), so Sxx == Syy == Szz bit for bit: a fluid cell keeps only
//     Szz / Rzz (bfd_dev::cls), which is read and written here; every reader takes Szz there.
// Values equal the canonical sequence (only the sign of an exact zero can differ).
// ------------------------------------------------------------------------------------------------
// Fluid-tile bodies are specialised per tile on two more properties found at setup (classify_tiles):
//   UNI : the tile grown by 2 cells holds ONE material and no reflector -> coefficients are per-tile
//         scalars; no id loads, table lookups or reflector tests;
//   PML : some cell of the tile lies in an absorbing-layer zone (otherwise no CPML code at all).
// One launch covers all fluid tiles of a half-step in their natural (XCD-remapped) order; the workgroup
// switches on its tile's flags (block-uniform) into the matching instantiation.
// All bodies are software pipelined: every value plane kl needs is in registers when its iteration starts
// and the iteration issues the loads for plane kl+1 (CPML memory variables included).
// SOLID (round 5, compact solid state): the run may hold solid cells. Their Szz / Rzz take the solid formula (AS2, BS2 of the cell's material, 0 in
// a fluid: the same expression serves every lane, equal to the fluid one up to the sign of an exact zero); everything else a solid cell has --
// Sxx, Syy, the shear stresses and their memory variables -- is the sparse kernel's (stress_shear_sparse, which runs after this one and reads
// the absorbing-layer memory variables this kernel has just advanced).
// PAIR (paired Pressure accumulation; non-SOLID, non-QUIET flavours): the cell's old Szz is the final pressure of the previous step (velocity-type
// sources never touch Szz) and the new one that of this step, so ONE read-modify-write of the running sum here, in every second accumulating step, adds
// both squares in the order the velocity kernel adds them, (acc + p_old^2) + p_new^2, and velocity_fluid leaves the sum alone (bfd_api.hip, "paired
// accumulation"). The sum runs one plane ahead like the other streams; the peak is read where it is used, as in velocity_fluid_body.
// advVz (runs that carry BFD_RUN_ADV_VZ: plain fluid runs outside the absorbing layer, not QUIET; bfd_lists.hip, "advanced Vz"): the Vz update of
// velocity_fluid_body needs nothing from the x/y neighbours, only the column's NEW Szz of planes p-1 .. p+2, and this kernel holds the column's Vz in
// its z-queue. So it keeps its last three new Szz (and two ids) and stores the new Vz of plane p = kl-2 at iteration kl, after dzVz has used the old
// one: the very expression of velocity_fluid_body, which then neither loads nor stores Vz at those planes.
// Which planes: iteration kl of a run reads Vz(kl-2 .. kl+1), all loaded at least one iteration before the store to kl-2; the run below reads up to
// my kbeg, the run above down to my kend-2, x/y neighbours never read Vz; and the new Szz of p-1 .. p+2 must all be this run's. Hence exactly
// p in [kbeg+1, kend-3]; a run shorter than 4 planes advances nothing.
template <bool LOSSY, bool UNI, bool PML, bool SOLID = false, bool QUIET = false, bool PAIR = false>
__device__ __forceinline__ void stress_fluid_body(const bfd_dev &d, int bx, int by, int kbeg, int kend, int tm,
                                                  float (*sV)[2][LH * LW], float *__restrict__ accP = nullptr, float *__restrict__ pkP = nullptr,
                                                  bool advVz = false)
{
    constexpr bool ADVZ = !PML && !SOLID && !QUIET;
    static_assert(!PAIR || (!SOLID && !QUIET), "paired accumulation: plain fluid flavours only");
    unsigned nzb = 0u;          // QUIET: bits of everything stored
    // The three normal stresses are identical in a FLUID tile; Szz is the one that is kept (it is
    // also the one whose ghost planes the Z-neighbour exchange carries).
    const int N1 = d.N1, N2 = d.N2;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * TX + tx;
    const int i0 = bx * TX, j0 = by * TY;
    const int i = i0 + tx, j = j0 + ty;
    const bool valid = (i < N1) && (j < N2);
    const long pl = d.plane;
    const int P = d.P;
    const int own = (ty + 2) * LW + tx + 2;
    const unsigned cij = valid ? (unsigned)(j * N1 + i) : 0u;

    // halo tasks: Vy rows above/below (256), Vx columns left/right (32)
    HaloTask t; t.lofs = -1; t.ok = false; t.arr = 0; t.gofs = 0;
    if (tid < YT) ytask(tid, 1, i0, j0, N1, N2, t);
    else if (tid < YT + XT) xtask(tid - YT, 0, i0, j0, N1, N2, t);
    const bool has = t.lofs >= 0;
    // the array of the task is uniform per wave (waves 0-3: Vy rows, wave 4: Vx columns): SGPR base + 32-bit byte offset
    const float *ph = __builtin_amdgcn_readfirstlane(t.arr) == 0 ? d.Vx : d.Vy;
    const unsigned hofs = t.ok ? (unsigned)t.gofs * 4u : 0u;
    float *lh = &sV[0][t.arr][has ? t.lofs : 0];

    const float c1 = d.c1;
    float APu = 0.f, BPu = 0.f;
    if (UNI) { APu = d.AP[tm]; BPu = d.BP[tm]; }

    // absorbing layer (PML flavours only): per-thread x/y coefficients and running zone offsets
    const bool zi = PML && valid && (i < P || i >= N1 - P);
    const bool zj = PML && valid && (j < P || j >= N2 - P);
    float ax = 0, bxc = 0, ay = 0, byc = 0, px = 0, py = 0, pz = 0;
    unsigned qx = 0, qy = 0;
    const unsigned dqx = (unsigned)(N2 * 2 * P), dqy = (unsigned)(2 * P * N1);
    if (PML) {
        if (zi) { ax = d.axI[i]; bxc = d.bxI[i]; qx = (unsigned)((kbeg * N2 + j) * (2 * P) + (i < P ? i : i - (N1 - 2 * P))); px = F4(d.psi[0], (unsigned)(qx) * 4u); }
        if (zj) { ay = d.ayI[j]; byc = d.byI[j]; qy = (unsigned)((kbeg * (2 * P) + (j < P ? j : j - (N2 - 2 * P))) * N1 + i); py = F4(d.psi[1], (unsigned)(qy) * 4u); }
        const int kg = d.k0 + kbeg;
        if (valid && (kg < P || kg >= d.N3 - P)) pz = F4(d.psi[2], (unsigned)((long)(kg < P ? kg : kg - (d.N3 - 2 * P)) * pl + cij) * 4u);
    }

    const bool inner = PAIR && valid && i >= d.ND && i < N1 - d.ND && j >= d.ND && j < N2 - d.ND;
    const bool accA = PAIR && accP != nullptr, accK = PAIR && pkP != nullptr;
    float vx0 = 0, vy0 = 0, vzm2 = 0, vzm1 = 0, vz0 = 0, vzp1 = 0, szz = 0, rzz = 0, av = 0;
    unsigned mraw = 0;
    if (valid) {
        const float *bVz = d.Vz + kbeg * pl;
        if (accA) av = LD4((accP + kbeg * pl), cij * 4u);
        vx0 = F4((d.Vx + kbeg * pl), cij * 4u); vy0 = F4((d.Vy + kbeg * pl), cij * 4u);
        vzm2 = LD4((bVz - 2 * pl), cij * 4u); vzm1 = LD4((bVz - pl), cij * 4u); vz0 = LD4(bVz, cij * 4u); vzp1 = LD4((bVz + pl), cij * 4u);
        szz = LD4((d.Szz + kbeg * pl), cij * 4u);
        if (LOSSY) rzz = LD4((d.Rzz + kbeg * pl), cij * 4u);
        if (!UNI) mraw = U2((d.mat + kbeg * pl), cij * 2u);
    }
    float hv = t.ok ? F4(ph + kbeg * pl, hofs) : 0.0f;
    // advanced Vz: new Szz of planes kl-1, kl-2, kl-3 and the ids of planes kl-1, kl-2
    float sq1 = 0, sq2 = 0, sq3 = 0, ruv = 0;
    unsigned mq1 = 0, mq2 = 0;
    if (ADVZ && UNI) ruv = d.invRho[tm];

    for (int kl = kbeg; kl < kend; kl++) {
        const int b = kl & 1;
        const long ko = (long)kl * pl;
        const int k = d.k0 + kl;
        sV[b][0][own] = vx0; sV[b][1][own] = vy0;
        if (has) lh[b * (2 * LH * LW)] = hv;
        // table rows of this plane (cache-resident; short latency, overlaps the barrier)
        float AP = APu, BP = BPu, AS2 = 0.f, BS2 = 0.f;
        if (!UNI && valid) { const int m = mraw & BFD_MAT_MASK; AP = d.AP[m]; if (LOSSY) BP = d.BP[m]; if (SOLID) { AS2 = d.AS2[m]; BS2 = d.BS2[m]; } }
        __syncthreads();

        float nvx = 0, nvy = 0, nvz = 0, nh = 0, nszz = 0, nrzz = 0, npx = 0, npy = 0, npz = 0, nav = 0, nsq = 0;
        unsigned nmraw = 0;
        if (kl + 1 < kend) {
            if (valid) {
                nvx = F4((d.Vx + ko + pl), cij * 4u); nvy = F4((d.Vy + ko + pl), cij * 4u); nvz = LD4((d.Vz + ko + 2 * pl), cij * 4u);
                nszz = LD4((d.Szz + ko + pl), cij * 4u);
                if (accA) nav = LD4((accP + ko + pl), cij * 4u);
                if (LOSSY) nrzz = LD4((d.Rzz + ko + pl), cij * 4u);
                if (!UNI) nmraw = U2((d.mat + ko + pl), cij * 2u);
            }
            if (t.ok) nh = F4(ph + ko + pl, hofs);
            if (PML) {
                if (zi) npx = F4(d.psi[0], (unsigned)(qx + dqx) * 4u);
                if (zj) npy = F4(d.psi[1], (unsigned)(qy + dqy) * 4u);
                const int kn = k + 1;
                if (valid && (kn < P || kn >= d.N3 - P)) npz = F4(d.psi[2], (unsigned)((long)(kn < P ? kn : kn - (d.N3 - 2 * P)) * pl + cij) * 4u);
            }
        }
        if (valid) {
            const float *sx = &sV[b][0][own], *sy = &sV[b][1][own];
            float dxVx = dminus4(sx[-2], sx[-1], vx0, sx[1]);
            float dyVy = dminus4(sy[-2 * LW], sy[-LW], vy0, sy[LW]);
            float dzVz = dminus4(vzm2, vzm1, vz0, vzp1);
            float val = 0.f, rn = 0.f;
            if (UNI || !(mraw & BFD_REFLECTOR_BIT)) {
                if (PML) {
                    if (zi) { const float pn = bxc * px + ax * dxVx; F4(d.psi[0], (unsigned)(qx) * 4u) = pn; dxVx = dxVx + pn; }
                    if (zj) { const float pn = byc * py + ay * dyVy; F4(d.psi[1], (unsigned)(qy) * 4u) = pn; dyVy = dyVy + pn; }
                    if (k < P || k >= d.N3 - P) {
                        const float pn = d.bzI[k] * pz + d.azI[k] * dzVz;
                        F4(d.psi[2], (unsigned)((long)(k < P ? k : k - (d.N3 - 2 * P)) * pl + cij) * 4u) = pn;
                        dzVz = dzVz + pn;
                    }
                }
                const float sXY = dxVx + dyVy;
                const float div = sXY + dzVz;
                if (SOLID) {
                    rn = c1 * rzz - (BP * div - BS2 * sXY);
                    val = szz + ((AP * div - AS2 * sXY) + 0.5f * (rzz + rn));
                } else if (LOSSY) {
                    rn = c1 * rzz - BP * div;
                    val = szz + (AP * div + 0.5f * (rzz + rn));
                } else {
                    val = szz + AP * div;
                }
            }
            // a fluid cell keeps only Szz / Rzz (bfd_dev::cls): nobody reads its Sxx/Syy/Rxx/Ryy (expanded on demand, bfd_outputs.hip)
            ST4((d.SzzW + ko), cij * 4u, val);
            if (PAIR) {
                if (inner && k >= d.ND && k < d.N3 - d.ND) {
                    const float so = (szz + szz) + szz, sn = (val + val) + val;
                    const float po = -so * (1.0f / 3.0f), pn = -sn * (1.0f / 3.0f);
                    if (accA) ST4((accP + ko), cij * 4u, (av + po * po) + pn * pn);
                    if (accK) {
                        const float m0 = F4((pkP + ko), cij * 4u), ao = fabsf(po), an = fabsf(pn);
                        float m = m0;
                        if (ao > m) m = ao;
                        if (an > m) m = an;
                        if (m > m0) F4((pkP + ko), cij * 4u) = m;
                    }
                }
            }
            if (QUIET) nzb |= fbits(val) | fbits(rn);
            if (LOSSY) ST4((d.RzzW + ko), cij * 4u, rn);
            if (ADVZ) {
                nsq = val;
                if (advVz && kl >= kbeg + 3) {      // plane p = kl-2 in [kbeg+1, kend-3]: vzm2 is its old Vz, dzVz above was its last reader
                    float r0 = ruv, r1 = ruv;
                    if (!UNI) { r0 = d.invRho[mq2 & BFD_MAT_MASK]; r1 = d.invRho[mq1 & BFD_MAT_MASK]; }
                    const float dz = dplus4(sq3, sq2, sq1, val);
                    float w = vzm2 + (0.5f * (r0 + r1)) * dz;
                    if (!UNI && (mq2 & BFD_REFLECTOR_BIT)) w = 0.f;
                    ST4((d.VzW + ko - 2 * pl), cij * 4u, w);
                }
            }
        }
        if (ADVZ) { sq3 = sq2; sq2 = sq1; sq1 = nsq; mq2 = mq1; mq1 = mraw; }
        vx0 = nvx; vy0 = nvy;
        vzm2 = vzm1; vzm1 = vz0; vz0 = vzp1; vzp1 = nvz;
        hv = nh; szz = nszz; rzz = nrzz; mraw = nmraw; av = nav;
        px = npx; py = npy; pz = npz; qx += dqx; qy += dqy;
    }
    if (QUIET) run_mark_active(d, bx, by, kbeg, kend, nzb);
}

// advVz: the run carries BFD_RUN_ADV_VZ, so stress_fluid_body has already stored the new Vz of planes kbeg+1 .. kend-3 (see there): at those planes Vz
// is neither loaded nor stored here (a block-uniform predicate per plane); Vx, Vy, the accumulation and the reflector's zeros of Vx / Vy are as ever.
template <bool ACC, bool UNI, bool PML, bool QUIET = false>
__device__ __forceinline__ void velocity_fluid_body(const bfd_dev &d, int bx, int by, int kbeg, int kend, int tm,
                                                    float (*sS)[LH * LW], float *__restrict__ accP, float *__restrict__ pkP, bool advVz = false)
{
    const bool adv = !PML && !QUIET && advVz;
    const int N1 = d.N1, N2 = d.N2;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * TX + tx;
    const int i0 = bx * TX, j0 = by * TY;
    const int i = i0 + tx, j = j0 + ty;
    const bool valid = (i < N1) && (j < N2);
    const long pl = d.plane;
    const int P = d.P;
    const int own = (ty + 2) * LW + tx + 2;
    const unsigned cij = valid ? (unsigned)(j * N1 + i) : 0u;
    const unsigned cx = valid ? (unsigned)(j * N1 + min(i + 1, N1 - 1)) : 0u;      // (i+1, j)
    const unsigned cy = valid ? (unsigned)(min(j + 1, N2 - 1) * N1 + i) : 0u;      // (i, j+1)

    // halo ring of Szz (== Sxx == Syy here): rows (256) and columns (32)
    HaloTask t; t.lofs = -1; t.ok = false; t.arr = 0; t.gofs = 0;
    if (tid < YT) ytask(tid, 0, i0, j0, N1, N2, t);
    else if (tid < YT + XT) xtask(tid - YT, 0, i0, j0, N1, N2, t);
    const bool has = t.lofs >= 0;
    const float *ph = d.Szz;
    const unsigned hofs = t.ok ? (unsigned)t.gofs * 4u : 0u;
    float *lh = &sS[0][has ? t.lofs : 0];

    const bool inner = valid && i >= d.ND && i < N1 - d.ND && j >= d.ND && j < N2 - d.ND;
    const bool accA = ACC && accP != nullptr, accK = ACC && pkP != nullptr;
    unsigned nzb = 0u;          // QUIET: bits of everything stored
    float ru = 0.f;
    if (UNI) ru = d.invRho[tm];                       // 0.5*(r+r) == r exactly: every face of a UNI tile sees one 1/rho

    const bool zi = PML && valid && (i < P || i >= N1 - P);
    const bool zj = PML && valid && (j < P || j >= N2 - P);
    float ax = 0, bxc = 0, ay = 0, byc = 0, px = 0, py = 0, pz = 0;
    unsigned qx = 0, qy = 0;
    const unsigned dqx = (unsigned)(N2 * 2 * P), dqy = (unsigned)(2 * P * N1);
    if (PML) {
        if (zi) { ax = d.axH[i]; bxc = d.bxH[i]; qx = (unsigned)((kbeg * N2 + j) * (2 * P) + (i < P ? i : i - (N1 - 2 * P))); px = F4(d.psi[9], (unsigned)(qx) * 4u); }
        if (zj) { ay = d.ayH[j]; byc = d.byH[j]; qy = (unsigned)((kbeg * (2 * P) + (j < P ? j : j - (N2 - 2 * P))) * N1 + i); py = F4(d.psi[13], (unsigned)(qy) * 4u); }
        const int kg = d.k0 + kbeg;
        if (valid && (kg < P || kg >= d.N3 - P)) pz = F4(d.psi[17], (unsigned)((long)(kg < P ? kg : kg - (d.N3 - 2 * P)) * pl + cij) * 4u);
    }

    // own material id runs two planes ahead because the z face needs 1/rho of plane kl+1; neighbour ids
    // one plane ahead; table rows at the top of the iteration
    float sm1 = 0, s0 = 0, sp1 = 0, sp2 = 0, vx = 0, vy = 0, vz = 0, av = 0, r0 = ru;
    unsigned mraw = 0, mraw1 = 0, mx = 0, my = 0;
    if (valid) {
        const float *bS = d.Szz + kbeg * pl;
        sm1 = F4((bS - pl), cij * 4u); s0 = F4(bS, cij * 4u); sp1 = F4((bS + pl), cij * 4u); sp2 = F4((bS + 2 * pl), cij * 4u);
        vx = LD4((d.Vx + kbeg * pl), cij * 4u); vy = LD4((d.Vy + kbeg * pl), cij * 4u); vz = LD4((d.Vz + kbeg * pl), cij * 4u);
        if (accA) av = LD4((accP + kbeg * pl), cij * 4u);
        if (!UNI) {
            const uint16_t *bM = d.mat + kbeg * pl;
            mraw = U2(bM, cij * 2u); mraw1 = U2((bM + pl), cij * 2u); mx = U2(bM, cx * 2u); my = U2(bM, cy * 2u);
            r0 = d.invRho[mraw & BFD_MAT_MASK];
        }
    }
    float hv = t.ok ? F4(ph + kbeg * pl, hofs) : 0.0f;

    for (int kl = kbeg; kl < kend; kl++) {
        const int b = kl & 1;
        const long ko = (long)kl * pl;
        const int k = d.k0 + kl;
        sS[b][own] = s0;
        if (has) lh[b * (LH * LW)] = hv;
        float r1 = ru, rx = ru, ry = ru;
        if (!UNI && valid) {
            r1 = d.invRho[mraw1 & BFD_MAT_MASK];       // plane kl+1, becomes r0 of the next iteration
            rx = d.invRho[mx & BFD_MAT_MASK];
            ry = d.invRho[my & BFD_MAT_MASK];
        }
        __syncthreads();

        float ns = 0, nh = 0, nvx = 0, nvy = 0, nvz = 0, nav = 0, npx = 0, npy = 0, npz = 0;
        unsigned nm2 = 0, nmx = 0, nmy = 0;
        if (!UNI && valid) nm2 = U2((d.mat + ko + 2 * pl), cij * 2u);     // ghost planes make kl+2 addressable
        if (kl + 1 < kend) {
            if (valid) {
                ns = F4((d.Szz + ko + 3 * pl), cij * 4u);
                nvx = LD4((d.Vx + ko + pl), cij * 4u); nvy = LD4((d.Vy + ko + pl), cij * 4u);
                if (!(adv && kl + 1 < kend - 2)) nvz = LD4((d.Vz + ko + pl), cij * 4u);      // plane kl+1 > kbeg: advanced unless one of the run's last two
                if (!UNI) { nmx = U2((d.mat + ko + pl), cx * 2u); nmy = U2((d.mat + ko + pl), cy * 2u); }
                if (accA) nav = LD4((accP + ko + pl), cij * 4u);
            }
            if (t.ok) nh = F4(ph + ko + pl, hofs);
            if (PML) {
                if (zi) npx = F4(d.psi[9], (unsigned)(qx + dqx) * 4u);
                if (zj) npy = F4(d.psi[13], (unsigned)(qy + dqy) * 4u);
                const int kn = k + 1;
                if (valid && (kn < P || kn >= d.N3 - P)) npz = F4(d.psi[17], (unsigned)((long)(kn < P ? kn : kn - (d.N3 - 2 * P)) * pl + cij) * 4u);
            }
        }
        const bool ownVz = !(adv && kl > kbeg && kl < kend - 2);      // false: stress_fluid_body has stored this plane's new Vz
        if (valid) {
            if (ACC) {
                if (inner && k >= d.ND && k < d.N3 - d.ND) {
                    const float s = (s0 + s0) + s0;
                    const float p = -s * (1.0f / 3.0f);
                    if (accA) ST4((accP + ko), cij * 4u, av + p * p);
                    // the running peak is read here, not a plane ahead: one live register fewer (the accumulating flavour spilled one at 8 waves)
                    if (accK) { const float ap = fabsf(p); if (ap > F4((pkP + ko), cij * 4u)) F4((pkP + ko), cij * 4u) = ap; }
                }
            }
            if (!UNI && (mraw & BFD_REFLECTOR_BIT)) {
                F4((d.VxW + ko), cij * 4u) = 0.f; F4((d.VyW + ko), cij * 4u) = 0.f;
                if (ownVz) F4((d.VzW + ko), cij * 4u) = 0.f;
            } else {
                const float *p = &sS[b][own];
                float dx = dplus4(p[-1], s0, p[1], p[2]);
                float dy = dplus4(p[-LW], s0, p[LW], p[2 * LW]);
                float dz = dplus4(sm1, s0, sp1, sp2);
                if (PML) {
                    if (zi) { const float pn = bxc * px + ax * dx; F4(d.psi[9], (unsigned)(qx) * 4u) = pn; dx = dx + pn; }
                    if (zj) { const float pn = byc * py + ay * dy; F4(d.psi[13], (unsigned)(qy) * 4u) = pn; dy = dy + pn; }
                    if (k < P || k >= d.N3 - P) {
                        const float pn = d.bzH[k] * pz + d.azH[k] * dz;
                        F4(d.psi[17], (unsigned)((long)(k < P ? k : k - (d.N3 - 2 * P)) * pl + cij) * 4u) = pn;
                        dz = dz + pn;
                    }
                }
                if (!QUIET) {
                    ST4((d.VxW + ko), cij * 4u, vx + (0.5f * (r0 + rx)) * dx);
                    ST4((d.VyW + ko), cij * 4u, vy + (0.5f * (r0 + ry)) * dy);
                    if (ownVz) ST4((d.VzW + ko), cij * 4u, vz + (0.5f * (r0 + r1)) * dz);
                } else {
                    { const float w = vx + (0.5f * (r0 + rx)) * dx; ST4((d.VxW + ko), cij * 4u, w); nzb |= fbits(w); }
                    { const float w = vy + (0.5f * (r0 + ry)) * dy; ST4((d.VyW + ko), cij * 4u, w); nzb |= fbits(w); }
                    { const float w = vz + (0.5f * (r0 + r1)) * dz; ST4((d.VzW + ko), cij * 4u, w); nzb |= fbits(w); }
                }
            }
        }
        sm1 = s0; s0 = sp1; sp1 = sp2; sp2 = ns;
        hv = nh; vx = nvx; vy = nvy; vz = nvz; av = nav;
        r0 = r1; mraw = mraw1; mraw1 = nm2; mx = nmx; my = nmy;
        px = npx; py = npy; pz = npz; qx += dqx; qy += dqy;
    }
    if (QUIET) run_mark_active(d, bx, by, kbeg, kend, nzb);
}

// ---- dispatchers: one launch for all fluid runs; block-uniform switch on the run's flags ----
// run = (x: bx + tilesX*by, y: kbeg | kend<<16, z: flags, w: material id of UNI runs)
// flags: bit0 solid, bit1 lossy, bit2 UNI, bit3 PML, bit4 LEAN (the planner's count for the ABI; no kernel reads it), BFD_RUN_ADV_VZ (bfd_internal.h)
template <bool QUIET = false, bool PAIR = false>
__device__ __forceinline__ void stress_fluid_switch(const bfd_dev &d, const int4 &run, int tilesX, float (*sV)[2][LH * LW],
                                                    float *__restrict__ accP = nullptr, float *__restrict__ pkP = nullptr)
{
    const int bx = run.x % tilesX, by = run.x / tilesX, kbeg = run.y & 0xFFFF, kend = run.y >> 16, tm = run.w;
    const bool adv = (run.z & BFD_RUN_ADV_VZ) != 0;
    if (QUIET && run_all_quiet(d, bx, by, kbeg, kend)) return;
    if (run.z & 1) {          // a solid run in the fluid launch (compact solid state): memory variables, several materials
        if (run.z & 8) stress_fluid_body<true, false, true, true, QUIET>(d, bx, by, kbeg, kend, tm, sV);
        else stress_fluid_body<true, false, false, true, QUIET>(d, bx, by, kbeg, kend, tm, sV);
        return;
    }
    switch ((run.z >> 1) & 7) {
    case 0: stress_fluid_body<false, false, false, false, QUIET, PAIR>(d, bx, by, kbeg, kend, tm, sV, accP, pkP, adv); break;
    case 1: stress_fluid_body<true, false, false, false, QUIET, PAIR>(d, bx, by, kbeg, kend, tm, sV, accP, pkP, adv); break;
    case 2: stress_fluid_body<false, true, false, false, QUIET, PAIR>(d, bx, by, kbeg, kend, tm, sV, accP, pkP, adv); break;
    case 3: stress_fluid_body<true, true, false, false, QUIET, PAIR>(d, bx, by, kbeg, kend, tm, sV, accP, pkP, adv); break;
    case 4: stress_fluid_body<false, false, true, false, QUIET, PAIR>(d, bx, by, kbeg, kend, tm, sV, accP, pkP); break;
    case 5: stress_fluid_body<true, false, true, false, QUIET, PAIR>(d, bx, by, kbeg, kend, tm, sV, accP, pkP); break;
    case 6: stress_fluid_body<false, true, true, false, QUIET, PAIR>(d, bx, by, kbeg, kend, tm, sV, accP, pkP); break;
    default: stress_fluid_body<true, true, true, false, QUIET, PAIR>(d, bx, by, kbeg, kend, tm, sV, accP, pkP); break;
    }
}

// every run keeps only Szz / Rzz of its fluid cells (bfd_dev::cls), in all-fluid slabs and in slabs with solid tiles alike
template <bool QUIET = false, bool PAIR = false>
__global__ __launch_bounds__(NTHREADS, FLUID_WAVES_PER_SIMD) void stress_fluid(bfd_dev d, int tilesX, int nblocks, const int *__restrict__ xmap,
                                                                               const int4 *__restrict__ runs,
                                                                               float *__restrict__ accP, float *__restrict__ pkP)
{
    __shared__ float sV[2][2][LH * LW];
    const int ri = run_index(nblocks, xmap);
    if (ri < 0) return;
    const int4 run = runs[ri];
    stress_fluid_switch<QUIET, PAIR>(d, run, tilesX, sV, accP, pkP);
}

// Paired accumulation, flush: the Pressure of the current Szz that the pairing stress flavour has not added yet, at the cells velocity_fluid
// would have accumulated (fluid runs, inside the accumulation region): same expressions, one workgroup per run.
__global__ __launch_bounds__(NTHREADS) void flush_paired_pressure(bfd_dev d, int tilesX, int nruns, const int4 *__restrict__ runs,
                                                                  float *__restrict__ accP, float *__restrict__ pkP)
{
    if ((int)blockIdx.x >= nruns) return;
    const int4 run = runs[blockIdx.x];
    const int bx = run.x % tilesX, by = run.x / tilesX, kbeg = run.y & 0xFFFF, kend = run.y >> 16;
    const int i = bx * TX + (int)threadIdx.x, j = by * TY + (int)threadIdx.y;
    if (!(i >= d.ND && i < d.N1 - d.ND && j >= d.ND && j < d.N2 - d.ND)) return;
    const long cij = (long)j * d.N1 + i;
    for (int kl = kbeg; kl < kend; kl++) {
        const int k = d.k0 + kl;
        if (k < d.ND || k >= d.N3 - d.ND) continue;
        const long c = (long)kl * d.plane + cij;
        const float s0 = d.Szz[c];
        const float s = (s0 + s0) + s0;
        const float p = -s * (1.0f / 3.0f);
        if (accP) accP[c] = accP[c] + p * p;
        if (pkP) { const float ap = fabsf(p); if (ap > pkP[c]) pkP[c] = ap; }
    }
}

template <bool ACC, bool QUIET = false>
__global__ __launch_bounds__(NTHREADS, VELOCITY_FLUID_WAVES_PER_SIMD) void velocity_fluid(bfd_dev d, int tilesX, int nblocks, const int *__restrict__ xmap,
                                                                                 const int4 *__restrict__ runs,
                                                                                 float *__restrict__ accP, float *__restrict__ pkP)
{
    __shared__ float sS[2][LH * LW];
    const int ri = run_index(nblocks, xmap);
    if (ri < 0) return;
    const int4 run = runs[ri];
    const int bx = run.x % tilesX, by = run.x / tilesX, kbeg = run.y & 0xFFFF, kend = run.y >> 16, tm = run.w;
    const bool adv = (run.z & BFD_RUN_ADV_VZ) != 0;
    if (QUIET && run_all_quiet(d, bx, by, kbeg, kend)) return;
    switch ((run.z >> 2) & 3) {
    case 0: velocity_fluid_body<ACC, false, false, QUIET>(d, bx, by, kbeg, kend, tm, sS, accP, pkP, adv); break;
    case 1: velocity_fluid_body<ACC, true, false, QUIET>(d, bx, by, kbeg, kend, tm, sS, accP, pkP, adv); break;
    case 2: velocity_fluid_body<ACC, false, true, QUIET>(d, bx, by, kbeg, kend, tm, sS, accP, pkP); break;
    default: velocity_fluid_body<ACC, true, true, QUIET>(d, bx, by, kbeg, kend, tm, sS, accP, pkP); break;
    }
}

}  // namespace

// fluid stress kernel over cnt runs; m = index of the cost-balanced map of the range, -1 = none. Flavours: plain, QUIET, PAIR (never both)
void bfd_launch_stress_fluid(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, const int4 *runs, int cnt, int m, bool pair, float *accP, float *pkP)
{
    const int tilesX = (d.N1 + TX - 1) / TX;
    const int *xm = (m >= 0 && t->xmap) ? t->xmap + 10 * m : nullptr;
    lift([&](auto QUIET, auto PAIR) {
        constexpr bool Q = decltype(QUIET)::value, P = decltype(PAIR)::value;
        if constexpr (!(Q && P))
            hipLaunchKernelGGL((stress_fluid<Q, P>), dim3(xm ? 8 * t->xmapH[m][9] : cnt), dim3(TX, TY, 1), 0, s, d, tilesX, cnt, xm, runs,
                               P ? accP : (float *)nullptr, P ? pkP : (float *)nullptr);
    }, d.act != nullptr, pair);
}

// acc: this launch adds the Pressure of its runs (false in the steps the pairing stress flavour covers)
void bfd_launch_velocity_fluid(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, const int4 *runs, int cnt, int m, bool acc, float *accP, float *pkP)
{
    const int tilesX = (d.N1 + TX - 1) / TX;
    lift([&](auto ACC, auto QUIET) {
        BFD_LAUNCH_X((velocity_fluid<decltype(ACC)::value, decltype(QUIET)::value>), cnt, m, runs, accP, pkP);
    }, acc, d.act != nullptr);
}

void bfd_launch_flush_paired(const bfd_dev &d, hipStream_t s, float *accP, float *pkP, const bfd_tiles *t)
{
    const int tilesX = (d.N1 + TX - 1) / TX;
    if (t->nFluid > 0 && (accP || pkP))
        hipLaunchKernelGGL(flush_paired_pressure, dim3(t->nFluid), dim3(TX, TY, 1), 0, s, d, tilesX, t->nFluid, (const int4 *)t->runs, accP, pkP);
}
