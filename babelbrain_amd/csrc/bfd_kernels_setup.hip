// Setup kernels of the planner of the tiled path (bfd_lists.hip) and of the placement (bfd_placement.hip): class byte per cell, flags per
// sub-tile, class counts of the solid runs, the activity map's source sub-tiles, the placement probe; and the tile grid's sizes for the host.
// mark_source_subtiles is defined behind the anonymous namespace and has an external name: it keeps the symbol it has always had. gfx950 only.
#include "bfd_tile.h"
#include "bfd_device.h"
#include <algorithm>

namespace {

// placement probe (bfd_placement.hip, bfd_choose_placement): two float32 arrays updated in place at the same cell offset along the
// engine's own runs, planes below kmax only. a' = a + b, b' = b + a: the all-zero state of step 0 stays all zero.
__global__ __launch_bounds__(NTHREADS, 8) void probe_pair(float *__restrict__ a, float *__restrict__ b, long pl, int N1, int N2, int tilesX,
                                                          int nblocks, const int4 *__restrict__ runs, int kmax)
{
    const int4 run = runs[remap_block(blockIdx.x, nblocks)];
    const int bx = run.x % tilesX, by = run.x / tilesX;
    const int i = bx * TX + threadIdx.x, j = by * TY + threadIdx.y;
    const int kbeg = run.y & 0xFFFF, kend = min(run.y >> 16, kmax);
    if (i >= N1 || j >= N2 || kbeg >= kend) return;
    const unsigned o = (unsigned)(j * N1 + i) * 4u;
    float va = F4(a + kbeg * pl, o), vb = F4(b + kbeg * pl, o);
    for (int kl = kbeg; kl < kend; kl++) {
        const long ko = (long)kl * pl;
        float na = 0.f, nb = 0.f;
        if (kl + 1 < kend) { na = F4(a + ko + pl, o); nb = F4(b + ko + pl, o); }
        F4(a + ko, o) = va + vb; F4(b + ko, o) = vb + va;
        va = na; vb = nb;
    }
}

// setup: class byte of every allocated cell (local planes -2 .. nk+1). base pointers address allocation plane 0.
__global__ void cell_classes(bfd_dev d, const uint16_t *__restrict__ matBase, uint8_t *__restrict__ clsBase, long nalloc, int nplanes)
{
    const int N1 = d.N1, N2 = d.N2;
    const long pl = d.plane;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nalloc; v += (long)gridDim.x * blockDim.x) {
        const int kk = (int)(v / pl);
        const int r = (int)(v - (long)kk * pl);
        const int j = r / N1, i = r - j * N1;
        const unsigned raw = matBase[v];
        const int m = raw & BFD_MAT_MASK;
        const bool refl = raw & BFD_REFLECTOR_BIT;
        const float iv0 = d.invMu[m];
        unsigned c = 0;
        if (refl) c |= BFD_CLS_REFL;
        else if (!(iv0 > 0.f)) c |= BFD_CLS_FLUID;
        if (d.BP[m] == 0.f && d.BS2[m] == 0.f) c |= BFD_CLS_NOMEM;
        if (!refl && iv0 > 0.f) {
            const int i1 = min(i + 1, N1 - 1), j1 = min(j + 1, N2 - 1), k1 = min(kk + 1, nplanes - 1);
            const long r0 = (long)kk * pl + (long)j * N1, r1 = (long)kk * pl + (long)j1 * N1;
            const long z0 = (long)k1 * pl + (long)j * N1, z1 = (long)k1 * pl + (long)j1 * N1;
            const bool sx = d.invMu[matBase[r0 + i1] & BFD_MAT_MASK] > 0.f, sy = d.invMu[matBase[r1 + i] & BFD_MAT_MASK] > 0.f;
            const bool sz = d.invMu[matBase[z0 + i] & BFD_MAT_MASK] > 0.f;
            const int mXY = matBase[r1 + i1] & BFD_MAT_MASK, mXZ = matBase[z0 + i1] & BFD_MAT_MASK, mYZ = matBase[z1 + i] & BFD_MAT_MASK;
            if (sx && sy && d.invMu[mXY] > 0.f) c |= BFD_CLS_EXY;
            if (sx && sz && d.invMu[mXZ] > 0.f) c |= BFD_CLS_EXZ;
            if (sy && sz && d.invMu[mYZ] > 0.f) c |= BFD_CLS_EYZ;
        }
        clsBase[v] = (uint8_t)c;
    }
}

// class counts over the cells of the solid runs (byte accounting): one workgroup per run
__global__ __launch_bounds__(NTHREADS) void count_solid_cells(bfd_dev d, int tilesX, const int4 *__restrict__ runs, unsigned long long *__restrict__ out)
{
    const int4 run = runs[blockIdx.x];
    const int bx = run.x % tilesX, by = run.x / tilesX, kbeg = run.y & 0xFFFF, kend = run.y >> 16;
    const int i = bx * TX + threadIdx.x, j = by * TY + threadIdx.y;
    unsigned n[6] = {0, 0, 0, 0, 0, 0};
    if (i < d.N1 && j < d.N2)
        for (int kl = kbeg; kl < kend; kl++) {
            const unsigned c = d.cls[(long)kl * d.plane + (long)j * d.N1 + i];
            if (c & BFD_CLS_REFL) n[5]++;
            else n[((c & BFD_CLS_FLUID) ? 0 : 2) + ((c & BFD_CLS_NOMEM) && (c & BFD_CLS_FLUID) ? 0 : 1)]++;
            n[4] += ((c & BFD_CLS_EXY) ? 1 : 0) + ((c & BFD_CLS_EXZ) ? 1 : 0) + ((c & BFD_CLS_EYZ) ? 1 : 0);
        }
    for (int q = 0; q < 6; q++) {
        unsigned v = n[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if (threadIdx.x == 0 && v) atomicAdd(&out[q], (unsigned long long)v);
    }
}

// one workgroup per 64 x 8 x SUBZ sub-tile. flags: bit0 = a solid cell within the sub-tile grown by 2 cells;
// bit1 = a cell of the sub-tile relaxes (BP != 0); bit2 = UNI: one material and no reflector in the grown
// region; bit3 = PML: a cell of the sub-tile lies inside an absorbing-layer zone. mat = id at its first cell.
__global__ void classify_tiles(bfd_dev d, int tilesX, int tilesY, int *__restrict__ flags, int *__restrict__ tileMat)
{
    const int tile = blockIdx.x;
    const int bx = tile % tilesX, by = (tile / tilesX) % tilesY, bz = tile / (tilesX * tilesY);
    const int i0 = bx * TX - 2, j0 = by * TY - 2, k0 = bz * SUBZ - 2;
    const int nzOwn = min(SUBZ, d.nk - bz * SUBZ);
    const int nx = TX + 4, ny = TY + 4, nz = nzOwn + 4;
    const unsigned first = d.mat[(long)(bz * SUBZ) * d.plane + (long)min(by * TY, d.N2 - 1) * d.N1 + min(bx * TX, d.N1 - 1)];
    int solid = 0, lossy = 0, lossyG = 0, refl = 0, mixed = (first & BFD_REFLECTOR_BIT) ? 1 : 0;
    for (int v = threadIdx.x; v < nx * ny * nz; v += blockDim.x) {
        const int li = v % nx, lj = (v / nx) % ny, lk = v / (nx * ny);
        const int i = i0 + li, j = j0 + lj, kl = k0 + lk;       // kl in [-2, nk+2): ghost planes exist
        if (i < 0 || i >= d.N1 || j < 0 || j >= d.N2) continue;
        const unsigned raw = d.mat[(long)kl * d.plane + (long)j * d.N1 + i];
        const int m = raw & BFD_MAT_MASK;
        if (raw != first) mixed = 1;
        if (raw & BFD_REFLECTOR_BIT) refl = 1;
        if (d.invMu[m] > 0.f) solid = 1;
        if (d.BP[m] != 0.f) { lossyG = 1; if (li >= 2 && li < nx - 2 && lj >= 2 && lj < ny - 2 && lk >= 2 && lk < nz - 2) lossy = 1; }
    }
    solid = __syncthreads_or(solid);
    lossy = __syncthreads_or(lossy);
    lossyG = __syncthreads_or(lossyG);
    refl = __syncthreads_or(refl);
    mixed = __syncthreads_or(mixed);
    if (threadIdx.x == 0) {
        const int P = d.P;
        const int xa = bx * TX, xb = min(xa + TX, d.N1), ya = by * TY, yb = min(ya + TY, d.N2);
        const int za = d.k0 + bz * SUBZ, zb = za + nzOwn;
        const bool pml = xa < P || xb > d.N1 - P || ya < P || yb > d.N2 - P || za < P || zb > d.N3 - P;
        // bit6: an absorbing-layer cell (or the domain edge) within the sub-tile grown by 2 cells, or a ragged tile
        const bool pmlGrown = xa - 2 < P || xb + 2 > d.N1 - P || ya - 2 < P || yb + 2 > d.N2 - P || za - 2 < P || zb + 2 > d.N3 - P ||
                              xb - xa < TX || yb - ya < TY;
        // bit7: a cell of the GROWN region relaxes (the fused time step recomputes the stress there)
        flags[tile] = solid | (lossy << 1) | (mixed ? 0 : 4) | (pml ? 8 : 0) | (pmlGrown ? 64 : 0) | (lossyG ? 128 : 0) | (refl ? 256 : 0);      // bit8: a reflector voxel in the grown region
        tileMat[tile] = (int)(first & BFD_MAT_MASK);
    }
}

}  // namespace

// tiles in x and y; sub-tiles of SUBZ planes in z; ZCHUNK = longest run a workgroup marches
void bfd_tile_grid(const bfd_dev &d, int *tilesX, int *tilesY, int *subZ)
{
    *tilesX = (d.N1 + TX - 1) / TX; *tilesY = (d.N2 + TY - 1) / TY; *subZ = (d.nk + SUBZ - 1) / SUBZ;
}
int bfd_tile_zchunk(void) { return ZCHUNK; }
int bfd_tile_subz(void) { return SUBZ; }

void bfd_launch_probe_pair(const bfd_dev &d, hipStream_t s, const bfd_tiles *t, float *a, float *b, int kmax)
{
    const int n = t->nFluid + t->nSolid;
    if (n > 0) hipLaunchKernelGGL(probe_pair, dim3(n), dim3(TX, TY, 1), 0, s, a, b, (long)d.plane, d.N1, d.N2, (d.N1 + TX - 1) / TX, n, t->runs, kmax);
}

void bfd_launch_cell_classes(const bfd_dev &d, hipStream_t s, uint8_t *clsBase, long nalloc)
{
    const uint16_t *matBase = d.mat - 2 * (long)d.plane;
    hipLaunchKernelGGL(cell_classes, dim3((unsigned)std::min<long>((nalloc + 255) / 256, 16384)), dim3(256), 0, s, d, matBase, clsBase, nalloc, d.nk + 4);
}
void bfd_launch_count_solid_cells(const bfd_dev &d, hipStream_t s, const int4 *solidRuns, int nSolid, unsigned long long *counts6)
{
    if (nSolid) hipLaunchKernelGGL(count_solid_cells, dim3(nSolid), dim3(TX, TY, 1), 0, s, d, (d.N1 + TX - 1) / TX, solidRuns, counts6);
}

// activity map (bfd_dev::act): the sub-tiles that hold source voxels are active from the start
__global__ void mark_source_subtiles(bfd_dev d, const uint32_t *__restrict__ lin, long n)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const unsigned c = lin[t];
    const int kl = (int)(c / (unsigned)d.plane), r = (int)(c - (unsigned)kl * (unsigned)d.plane), j = r / d.N1, i = r - j * d.N1;
    d.act[((kl / SUBZ + 1) * d.actY + j / TY + 1) * d.actX + i / TX + 1] = 1;
}
void bfd_launch_mark_source_subtiles(const bfd_dev &d, hipStream_t s, const uint32_t *lin, long n)
{
    if (n > 0) hipLaunchKernelGGL(mark_source_subtiles, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, lin, n);
}

void bfd_launch_classify(const bfd_dev &d, hipStream_t s, int *flagsDev, int *tileMatDev)
{
    int tx, ty, tz; bfd_tile_grid(d, &tx, &ty, &tz);
    hipLaunchKernelGGL(classify_tiles, dim3(tx * ty * tz), dim3(256), 0, s, d, tx, ty, flagsDev, tileMatDev);
}
