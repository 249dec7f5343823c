// Order of the launches of a half-step of the tiled path. Host code only: every kernel and the launcher that picks its flavour are in the file
// of the kernel's class (bfd_kernels_fluid / _solid / _shear / _dense.hip); what is decided here is which runs go to which kernel, and when.
#include "bfd_tile.h"

void bfd_launch_stress_tiled(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, int part, float *accP, float *pkP)
{
    const bool pair = (accP || pkP) && !d.act;       // the pairing flavour of the plain fluid runs (quiet runs never pair)
    int off, n, offS, nS;
    part_range(t->nFluid, t->nFluidB, part, &off, &n);
    part_range(t->nSolid, t->nSolidB, part, &offS, &nS);
    // Compact solid state: Szz / Rzz of EVERY run, solid ones included, in one launch of the fluid kernel over the combined list (natural order:
    // a solid run sits between its fluid neighbours, their ring lines are shared in L2), then the sparse kernel with everything that exists
    // only at solid cells. It must come second: it reads the absorbing-layer memory variables the fluid kernel advances.
    const bool all = d.cssRow && t->runsAll;
    // fluid kernel over cnt runs; m = index of the cost-balanced map of the range, -1 = none
    auto stressFluid = [&](int cnt, int m, const int4 *runs) {
        BFD_KT(BFD_K_STRESS_FLUID, 0);
        bfd_launch_stress_fluid(d, s, t, runs, cnt, m, pair, accP, pkP);
        BFD_KT(BFD_K_STRESS_FLUID, 1);
    };
    if (all) {
        int offA, nA;
        part_range(t->nAll, t->nAllB, part, &offA, &nA);
        if (nA) stressFluid(nA, -1, t->runsAll + offA);
        n = 0; nS = 0;
    }
    if (nS) {
        BFD_KT(BFD_K_STRESS_SOLID, 0);
        if (t->shearCells) bfd_launch_stress_solid(d, s, t, t->runs + t->nFluid + offS, nS, BFD_XM_SS + part);
        else bfd_launch_stress_dense(d, s, t->runs + t->nFluid + offS, nS);     // variant 2: monolithic, dense
        BFD_KT(BFD_K_STRESS_SOLID, 1);
    }
    if (t->shearCells && t->nShear) {     // sparse shear: cells sorted by index; [0,lowEnd) and [highBeg,n) are the boundary chunks
        long b0 = 0, e0 = t->nShear, b1 = 0, e1 = 0;
        if (part == 1) { e0 = t->shearLowEnd; b1 = t->shearHighBeg; e1 = t->nShear; }
        else if (part == 2) { b0 = t->shearLowEnd; e0 = t->shearHighBeg; }
        BFD_KT(BFD_K_STRESS_SHEAR, 0);
        float *R0 = t->shearR ? t->shearR + b0 : nullptr, *R1 = t->shearR ? t->shearR + b1 : nullptr;
        bfd_launch_stress_shear(d, s, t, b0, e0, R0); bfd_launch_stress_shear(d, s, t, b1, e1, R1);
        BFD_KT(BFD_K_STRESS_SHEAR, 1);
    }
    if (n) stressFluid(n, BFD_XM_SF + part, t->runs + off);
}

void bfd_launch_velocity_tiled(const bfd_dev &d, hipStream_t s, float *accP, float *pkP, const bfd_tiles *t, int part, bool fluidAcc)
{
    const bool acc = accP || pkP;
    const bool accF = acc && fluidAcc;      // paired accumulation: the stress kernel adds the Pressure of the fluid runs
    int offF, nF, off, n;
    part_range(t->nFluid, t->nFluidB, part, &offF, &nF);
    part_range(t->nSolid, t->nSolidB, part, &off, &n);
    if (n) {
        BFD_KT(BFD_K_VELOCITY_SOLID, 0);
        if (t->shearCells) {
            // solid list = [boundary: PML | plain][interior: plain | PML]: the plain runs of the requested part are contiguous
            const int4 *base = t->runs + t->nFluid;
            int pb = 0, pe = 0, qb = 0, qe = 0;                 // PML pieces [pb,pe) and [qb,qe); plain piece between / around
            if (part != 2) { pb = 0; pe = t->nSolidBP; }
            if (part != 1) { qb = t->nSolid - t->nSolidIP; qe = t->nSolid; }
            const int nb = part == 2 ? t->nSolidB : t->nSolidBP, ne = part == 1 ? t->nSolidB : t->nSolid - t->nSolidIP;
            auto go = [&](bool pml, int a0, int a1, int m) {
                if (a1 > a0) bfd_launch_velocity_solid(d, s, t, part, pml, base + a0, a1 - a0, m, accP, pkP);
            };
            go(false, nb, ne, BFD_XM_VS + part); go(true, pb, pe, BFD_XM_VSP_LO); go(true, qb, qe, BFD_XM_VSP_HI);
        } else {                                                     // variant 2: dense
            bfd_launch_velocity_dense(d, s, t->runs + t->nFluid + off, n, accP, pkP);
        }
        BFD_KT(BFD_K_VELOCITY_SOLID, 1);
    }
    if (nF) {
        BFD_KT(BFD_K_VELOCITY_FLUID, 0);
        bfd_launch_velocity_fluid(d, s, t, t->runs + offF, nF, BFD_XM_VF + part, accF, accP, pkP);
        BFD_KT(BFD_K_VELOCITY_FLUID, 1);
    }
}
