// Device-side helpers shared by the tiled kernels (bfd_kernels_dense / _fluid / _solid / _shear / _setup.hip, bfd_kernels_fused.hip). gfx950 only.
#pragma once
#include "bfd_internal.h"

namespace {

__device__ __forceinline__ float dminus4(float fm2, float fm1, float f0, float fp1)
{
    float t1 = f0 - fm1;
    float t2 = fp1 - fm2;
    return BFD_CA * t1 - BFD_CB * t2;
}
__device__ __forceinline__ float dplus4(float fm1, float f0, float fp1, float fp2)
{
    float t1 = fp1 - f0;
    float t2 = fp2 - fm1;
    return BFD_CA * t1 - BFD_CB * t2;
}
__device__ __forceinline__ float cpml(float *__restrict__ psi, unsigned idx, float a, float b, float D)
{
    float pn = b * psi[idx] + a * D;
    psi[idx] = pn;
    return D + pn;
}


// Element access as (wave-uniform plane base) + (32-bit BYTE offset in a VGPR). Indexing a float* with a 32-bit cell index
// instead makes the compiler build 64-bit addresses in VGPR pairs that stay live (it cannot prove that index*4 stays below
// 2^32), and it reassociates (array + plane) + lane offset into (array + lane offset) + plane, hoisting the first sum out of
// the z loop: a loop-invariant VGPR pair per array.
// uni(): the plane base as an opaque wave-uniform value (SGPR pair); the address of an access is then one v_lshl_add_u64 of
// that pair and the shared offset register, live only until the access. The pointer is rebuilt from integers, so these are
// FLAT accesses; the variant with address_space(1) pointers and saddr-form global loads (scripts/r2/patches/) needs fewer
// registers still but measured 5-6 % slower on the solid-run kernels and equal on the fluid ones.
template <typename T>
__device__ __forceinline__ T *uni(T *p)
{
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (T *)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float &F4(float *base, unsigned byteOfs) { return *(float *)((char *)uni(base) + byteOfs); }
__device__ __forceinline__ const float &F4(const float *base, unsigned byteOfs) { return *(const float *)((const char *)uni(base) + byteOfs); }
// store of a value nobody reads before the next half-step: non-temporal, so that written lines do not displace halo lines in L2
// (fluid kernels: C3 89.1 -> 89.8 Gvoxel-steps/s on three alternating same-box runs; solid-run kernels: shear medium 63.87 -> 64.10 on
// five; profiles/r3/experiment_nontemporal_stores.txt).
__device__ __forceinline__ void ST4(float *base, unsigned byteOfs, float v)
{
    __builtin_nontemporal_store(v, (float *)((char *)uni(base) + byteOfs));
}
// load of a value only this lane reads in this half-step: non-temporal, it need not stay in L2 (fluid stress half-step: Szz / Rzz of
// the own cell, Vz; velocity half-steps: V of the own cell, the RMS sums; the sparse shear kernel's list, coefficients and entries).
// C3 89.7 -> 91.0, shear medium 64.1 -> 66.3 Gvoxel-steps/s on alternating same-box runs; NOT for the own-cell stresses of
// stress_solid (0.300 -> 0.313 ms). profiles/r3/experiment_nontemporal_stores.txt.
__device__ __forceinline__ float LD4(const float *base, unsigned byteOfs)
{
    return __builtin_nontemporal_load((const float *)((const char *)uni(base) + byteOfs));
}
template <typename T> __device__ __forceinline__ T LDNT(const T *p)               // sparse shear kernel: list entries, coefficients, its own S and R entries
{
    return __builtin_nontemporal_load(p);
}
__device__ __forceinline__ unsigned U2(const uint16_t *base, unsigned byteOfs) { return *(const uint16_t *)((const char *)uni(base) + byteOfs); }
__device__ __forceinline__ unsigned U1(const uint8_t *base, unsigned byteOfs) { return uni(base)[byteOfs]; }

// The same accesses as GLOBAL instructions (wave-uniform base in SGPRs + 32-bit byte offset), for the kernels whose prefetch has to stay in
// flight across their LDS phases (velocity_solid, the fused time step): a flat load counts on lgkmcnt as well, so the first wait for an LDS
// read would also wait for every load of the next plane just issued.
#define BFD_GLOBAL __attribute__((address_space(1)))
template <typename T> __device__ __forceinline__ BFD_GLOBAL T *guni(const T *p)
{
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (BFD_GLOBAL T *)(((unsigned long long)hi << 32) | lo);
}
// keeps the 32-bit offset a value of the block that uses it (hoisted out of the loop its zero-extension becomes a 64-bit VGPR address)
// (round 6: pinning the BASE as an opaque scalar pair instead of the lane's offset -- to save the v_mov each pinned offset costs -- makes the compiler form
// 64-bit vector addresses again: v_lshl_add_u64 6 -> 30 per plane, 92 -> 100 registers; not kept)
__device__ __forceinline__ unsigned pin(unsigned v) { asm("" : "+v"(v)); return v; }
__device__ __forceinline__ float GL4(const float *base, unsigned ofs) { return *(BFD_GLOBAL const float *)((BFD_GLOBAL const char *)guni(base) + pin(ofs)); }
__device__ __forceinline__ float GLNT(const float *base, unsigned ofs) { return __builtin_nontemporal_load((BFD_GLOBAL const float *)((BFD_GLOBAL const char *)guni(base) + pin(ofs))); }
__device__ __forceinline__ unsigned GL2(const uint16_t *base, unsigned ofs) { return *(BFD_GLOBAL const uint16_t *)((BFD_GLOBAL const char *)guni(base) + pin(ofs)); }
__device__ __forceinline__ unsigned GL1(const uint8_t *base, unsigned ofs) { return *(BFD_GLOBAL const uint8_t *)((BFD_GLOBAL const char *)guni(base) + pin(ofs)); }
// predicated: lanes with c == false read dword 0 of the plane and get 0
__device__ __forceinline__ float GLP(const float *base, unsigned ofs, bool c) { const float v = GL4(base, c ? ofs : 0u); return c ? v : 0.0f; }
__device__ __forceinline__ void GS4(float *base, unsigned ofs, float v) { *(BFD_GLOBAL float *)((BFD_GLOBAL char *)guni(base) + pin(ofs)) = v; }
__device__ __forceinline__ void GS4NT(float *base, unsigned ofs, float v)
{
    __builtin_nontemporal_store(v, (BFD_GLOBAL float *)((BFD_GLOBAL char *)guni(base) + pin(ofs)));
}

// XCD-aware tile order: consecutive block ids land on different XCDs (round robin over 8), so give
// XCD e the e-th contiguous run of tiles.
__device__ __forceinline__ int remap_block(int bid, int nblocks)
{
    const int per = nblocks >> 3;
    if (per == 0 || bid >= (per << 3)) return bid;     // tail blocks keep their id
    return (bid & 7) * per + (bid >> 3);
}

// Cost-balanced form (bfd_tiles::xmap): slot b & 7 = one XCD; its k-th block takes run seg[slot] + k of the launched range, -1 = nothing left
// for this block. The eighths are equal in estimated cost, not in count (profiles/r4/xcd_balance.txt).
__device__ __forceinline__ int xcd_run_index(const int *__restrict__ xmap)
{
    const int slot = __builtin_amdgcn_readfirstlane(blockIdx.x & 7), k = blockIdx.x >> 3;
    const int idx = xmap[slot] + k;
    return idx < xmap[slot + 1] ? idx : -1;
}
// the run of this block: cost-balanced map if the launch has one, otherwise equal counts per XCD; -1 = no run for this block
__device__ __forceinline__ int run_index(int nblocks, const int *__restrict__ xmap)
{
    return xmap ? xcd_run_index(xmap) : remap_block(blockIdx.x, nblocks);
}

}  // namespace
