// Mesh voxelisation, conformal masks and CT value mapping of Step 1 on MI355X: the last two callbacks CalculateMaskProcess.py:37-73 installs, and
// the scatter of the voxel centres through the rotated affine between them.
//
// Replaces
//     GPUFunctions.GPUVoxelize.Voxelize(mesh, targetResolution)        BabelDatasetPreps.py:570, :667, :670, :673 (skin, skull, CSF surfaces to
//                                                                      lists of voxel centres; host fallback trimesh.voxelized(...).fill())
//     the host lines BabelDatasetPreps.py:710-759                      (per mesh: hstack, float32 np.dot with InVAffineRot, np.round, int64 cast,
//                                                                      filter of the upper side, fancy-index store into the conformal mask)
//     GPUFunctions.GPUMapping.MappingFilter.MapFilter(HU, Sel, Unique) BabelDatasetPreps.py:1039 (host fallback :1034-1037, one pass per unique value)
//
// Voxelisation. The definition is in include/babelfdtd.h and, operation for operation, in bfd_voxelize_core.h: voxel (i, j, k) is set iff an odd
// number of triangles cover the column centre (j, k) in projection and lie at or beyond the voxel centre along x. Float64 throughout.
//   1. setup       one lane per triangle: the counter-clockwise projection, the normal, the clamped column box, its column count (vox_tri record);
//                  inclusive prefix sum of the counts (rocPRIM, the scan the labelling uses): ends[t] = pairs of triangles 0 .. t
//   2. crossings   one lane per (triangle, column) PAIR, not per triangle: a lane finds its triangle by binary search in ends[] (the lanes of a
//                  large face take the same path: one broadcast load per step), runs the three edge tests and, where they pass, issues ONE
//                  atomicXor of one bit: position c = min(floor(q), gx - 1) + 1 of the column's row in the crossing table (rows of gx + 1 bits
//                  padded to 64-bit words, x fastest). The per-voxel formulation issues xmax + 1 atomics here. A launch sweeps VOX_SWEEP pairs;
//                  longer pair ranges take further rounds of the same lanes (grid-stride).
//                  XOR is commutative and associative: the table, and everything derived from it, is the same from run to run and for every
//                  order of the triangles, whatever the arrival order of the atomics.
//   3. scan        one lane per table word (loads coalesce along x and across columns): suffix parity inside the word by shifts, the parity of
//                  the column's words above it as the carry. Voxel i is set iff an odd number of crossing bits sit at positions > i.
//   4. pack/count  one lane per word of the caller's table (bit 31 - (index % 32) of word index / 32, index = i + gx (j + gy k), the reference's
//                  packing): gathers its up-to-32 indices from the occupancy rows; popcounts are summed per wave, one atomic per wave (integer:
//                  order-free). The mask, when asked for, is expanded from the packed table.
//   bfd_voxel_points: popcount per table word, inclusive prefix sum, every word writes its points: ascending index order, deterministic
//   (the reference's atomic counter returns them in a different order every run).
// Scan and pack are two kernels where one could carry both: the scan is coalesced along the padded rows, the pack along the dense table, and the
// occupancy rows between them cost 1 bit per voxel each way.
// No kernel waits for another workgroup; every loop is bounded, see the comment at each.
//
// Conformal masks (bfd_voxel_scatter3d from a host table, bfd_voxelize_scatter3d from a mesh whose table never leaves the device; definition in
// include/babelfdtd.h, operation for operation in bfd_voxelize_core.h): one kernel, conf_scatter, see the comment there. Float32, one operation
// per rounding. mesh_to_table is the device section that bfd_voxelize_mesh and bfd_voxelize_scatter3d share.
//
// CT value mapping: one pass, 5 B read and 4 B written per voxel, four voxels per lane; binary search in the strictly increasing table, which is
// staged in LDS up to MAP_LDS_ROWS rows and read from global memory (L2) beyond. Values are compared as integer keys (bfd_voxelize_core.h).
#include <cmath>
#include <string.h>
#include "bfd_internal.h"
#include "bfd_call.h"
#include "bfd_scan.h"
#include "bfd_voxelize_core.h"

namespace {

constexpr int VX_THREADS = 256;
constexpr long VOX_SWEEP_BLOCKS = 4096;                        // pairs per sweep of the crossing kernel: 4096 x 256 = 2^20
constexpr long CONF_SWEEP_BLOCKS = 8192;                       // source voxels per sweep of the scatter kernel: 8192 x 256 = 2^21
constexpr int64_t VOX_MAX_VOXELS = (int64_t)1 << 40;
constexpr int MAP_LDS_ROWS = 4096;                             // 16 KiB of LDS
constexpr int MAP_MAX_ROWS = 65536;
constexpr long MAX_BLOCKS = 1L << 16;                          // work beyond this is taken by grid-stride loops

// ---------------------------------------------------------------- voxelisation kernels ----------------------------------------------------------------

__global__ __launch_bounds__(VX_THREADS) void vox_setup(const float *__restrict__ tris, int64_t n, const vox_grid g, vox_tri *__restrict__ recs,
                                                        int64_t *__restrict__ counts)
{
    for (int64_t t = (int64_t)blockIdx.x * VX_THREADS + threadIdx.x; t < n; t += (int64_t)gridDim.x * VX_THREADS) {      // grid-stride: ends
        float v[9];
#pragma unroll
        for (int q = 0; q < 9; q++) v[q] = tris[9 * t + q];
        vox_tri r;
        counts[t] = vox_setup_triangle(v, g, &r);
        recs[t] = r;
    }
}

__global__ __launch_bounds__(VX_THREADS) void vox_crossings(const vox_tri *__restrict__ recs, const int64_t *__restrict__ ends, int64_t n, const vox_grid g,
                                                            unsigned long long *__restrict__ cross)
{
    const int64_t nPairs = ends[n - 1];
    for (int64_t p = (int64_t)blockIdx.x * VX_THREADS + threadIdx.x; p < nPairs; p += (int64_t)gridDim.x * VX_THREADS) { // grid-stride: ends
        int64_t lo = 0, hi = n - 1;                  // the first triangle with ends[t] > p; ends[n - 1] > p holds. Ends: hi - lo halves
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (ends[mid] > p) hi = mid; else lo = mid + 1;
        }
        const vox_tri &t = recs[lo];
        const int64_t local = p - (lo ? ends[lo - 1] : 0);      // 0 <= local < nj nk
        const int64_t kk = local / t.nj, jj = local - kk * t.nj;           // j fastest: neighbouring lanes, neighbouring rows of the table
        const int64_t j = t.jl + jj, k = t.kl + kk;
        const int64_t c = vox_crossing(t, g, j, k);              // 0, or 1 .. gx
        if (c > 0) atomicXor(cross + (j + g.gy * k) * g.rowWords + (c >> 6), 1ull << (c & 63));
    }
}

__global__ __launch_bounds__(VX_THREADS) void vox_scan(const uint64_t *__restrict__ cross, uint64_t *__restrict__ occ, const vox_grid g, int64_t nWords)
{
    for (int64_t wd = (int64_t)blockIdx.x * VX_THREADS + threadIdx.x; wd < nWords; wd += (int64_t)gridDim.x * VX_THREADS) {     // grid-stride: ends
        const int64_t col = wd / g.rowWords;
        occ[wd] = vox_scan_word(cross + col * g.rowWords, wd - col * g.rowWords, g);      // its loop: at most rowWords - 1 rounds
    }
}

// count: the wave's popcounts in one atomic. The shuffles come after the loop, where every lane of the wave arrives.
__global__ __launch_bounds__(VX_THREADS) void vox_pack(const uint64_t *__restrict__ occ, uint32_t *__restrict__ table, const vox_grid g, int64_t nTable,
                                                       unsigned long long *__restrict__ count)
{
    unsigned long long mine = 0;
    for (int64_t o = (int64_t)blockIdx.x * VX_THREADS + threadIdx.x; o < nTable; o += (int64_t)gridDim.x * VX_THREADS) {        // grid-stride: ends
        const uint32_t w = vox_table_word(occ, o, g);            // its loop: at most 32 rounds
        table[o] = w;
        mine += (unsigned)__popc(w);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) mine += __shfl_xor(mine, s);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}

// one lane per table word: 32 bytes of the mask
__global__ __launch_bounds__(VX_THREADS) void vox_expand(const uint32_t *__restrict__ table, uint8_t *__restrict__ mask, int64_t nTable, int64_t nVoxels)
{
    for (int64_t o = (int64_t)blockIdx.x * VX_THREADS + threadIdx.x; o < nTable; o += (int64_t)gridDim.x * VX_THREADS) {        // grid-stride: ends
        const uint32_t w = table[o];
        const int64_t left = nVoxels - 32 * o;
        if (left >= 32) {
            uint32_t b[8];
#pragma unroll
            for (int q = 0; q < 8; q++)
                b[q] = ((w >> (31 - 4 * q)) & 1u) | (((w >> (30 - 4 * q)) & 1u) << 8) | (((w >> (29 - 4 * q)) & 1u) << 16) | (((w >> (28 - 4 * q)) & 1u) << 24);
            uint4 *dst = (uint4 *)(mask + 32 * o);               // 32-byte aligned: the base comes from hipMalloc
            dst[0] = make_uint4(b[0], b[1], b[2], b[3]);
            dst[1] = make_uint4(b[4], b[5], b[6], b[7]);
        } else {
            for (int q = 0; q < (int)left; q++) mask[32 * o + q] = (uint8_t)((w >> (31 - q)) & 1u);
        }
    }
}

// ---------------------------------------------------------------- points ----------------------------------------------------------------

__global__ __launch_bounds__(VX_THREADS) void pts_count(const uint32_t *__restrict__ table, int64_t *__restrict__ cnt, int64_t nTable, int64_t nVoxels)
{
    for (int64_t o = (int64_t)blockIdx.x * VX_THREADS + threadIdx.x; o < nTable; o += (int64_t)gridDim.x * VX_THREADS)         // grid-stride: ends
        cnt[o] = __popc(table[o] & vox_table_valid(o, nVoxels));
}

struct pts_args { int64_t gx, gy, nVoxels; double min[3], unit[3]; };

__global__ __launch_bounds__(VX_THREADS) void pts_write(const uint32_t *__restrict__ table, const int64_t *__restrict__ ends, float *__restrict__ points,
                                                        int64_t nTable, const pts_args a)
{
    for (int64_t o = (int64_t)blockIdx.x * VX_THREADS + threadIdx.x; o < nTable; o += (int64_t)gridDim.x * VX_THREADS) {        // grid-stride: ends
        uint32_t r = __brev(table[o] & vox_table_valid(o, a.nVoxels));      // bit b = index 32 o + b
        int64_t at = o ? ends[o - 1] : 0;
        while (r) {                                              // ends: every round clears a bit
            const int b = __ffs((int)r) - 1;
            r &= r - 1;
            const int64_t idx = 32 * o + b;
            const int64_t row = idx / a.gx;
            const int64_t i = idx - row * a.gx, k = row / a.gy, j = row - k * a.gy;
            points[3 * at] = vox_centre(a.min[0], a.unit[0], i);
            points[3 * at + 1] = vox_centre(a.min[1], a.unit[1], j);
            points[3 * at + 2] = vox_centre(a.min[2], a.unit[2], k);
            at++;
        }
    }
}

// ---------------------------------------------------------------- conformal masks ----------------------------------------------------------------

struct conf_args {
    int64_t gx, gy, rows, chunks;        // rows = gy gz source rows of ceil(gx / 64) chunks each
    double min[3], unit[3];
    float m[3][4];
    int64_t M[3];                        // read only where the volume is written
};
// lo and hi start at INT32_MAX / INT32_MIN, the counts at 0
struct conf_result { int32_t lo[3], hi[3]; unsigned long long counts[4]; };

// A wave takes 64 consecutive i of one source row per round; the rounds of a wave are the same for all its lanes, so the shuffles meet every lane.
// WRITE: a lane stores 1 at its point's voxel unless the lane before it has the same voxel (at ratio 0.75 about every other lane where the row
// runs along an output axis). The volume is zeroed before the launch; every store writes the same byte, so the result does not depend on any order.
// The bounds and counts are reduced per lane, then per wave, then by one atomic per wave and value (integer min, max and sum: order-free).
template <bool WRITE>
__global__ __launch_bounds__(VX_THREADS) void conf_scatter(const uint32_t *__restrict__ table, uint8_t *__restrict__ out, conf_result *__restrict__ res,
                                                           const conf_args a)
{
    const int lane = threadIdx.x & 63;
    const int64_t nUnits = a.rows * a.chunks, wavesPerBlock = VX_THREADS / 64;
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    unsigned cnt[4] = {0u, 0u, 0u, 0u};                          // at most 2^40 units over the 4 CONF_SWEEP_BLOCKS waves of a capped launch: 2^25 rounds a lane
    for (int64_t u = (int64_t)blockIdx.x * wavesPerBlock + (threadIdx.x >> 6); u < nUnits; u += (int64_t)gridDim.x * wavesPerBlock) {     // grid-stride: ends
        const int64_t row = u / a.chunks, i = (u - row * a.chunks) * 64 + lane;
        const int64_t k = row / a.gy, j = row - k * a.gy;
        int target = -1;                                         // the volume has fewer than 2^31 voxels
        if (i < a.gx && vox_table_bit(table, i + a.gx * row)) {
            const float x = vox_centre(a.min[0], a.unit[0], i), y = vox_centre(a.min[1], a.unit[1], j), z = vox_centre(a.min[2], a.unit[2], k);
            int32_t n[3];
            conf_point(a.m, x, y, z, n);
#pragma unroll
            for (int q = 0; q < 3; q++) { lo[q] = min(lo[q], n[q]); hi[q] = max(hi[q], n[q]); }
            cnt[0]++;
            if (WRITE) {
                int64_t at = -1;
                const int c = conf_target(n, a.M, &at);
                if (c == CONF_ABOVE) cnt[1]++;
                else if (c == CONF_WRAPPED) cnt[2]++;
                else if (c == CONF_BELOW) cnt[3]++;
                target = (int)at;
            }
        }
        if (WRITE) {
            const int before = __shfl_up(target, 1);
            if (target >= 0 && (lane == 0 || before != target)) out[target] = 1;
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int q = 0; q < 3; q++) { lo[q] = min(lo[q], __shfl_xor(lo[q], s)); hi[q] = max(hi[q], __shfl_xor(hi[q], s)); }
#pragma unroll
        for (int q = 0; q < 4; q++) cnt[q] += __shfl_xor(cnt[q], s);         // 64 lanes of at most 2^25 each
    }
    if (lane == 0 && cnt[0]) {
#pragma unroll
        for (int q = 0; q < 3; q++) { atomicMin(&res->lo[q], lo[q]); atomicMax(&res->hi[q], hi[q]); }
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (cnt[q]) atomicAdd(&res->counts[q], (unsigned long long)cnt[q]);
    }
}

// ---------------------------------------------------------------- CT value mapping ----------------------------------------------------------------

// hu arrives as the bits of its float32 values, the table as keys (map_key): no float comparison is made on the device
template <bool LDS>
__global__ __launch_bounds__(VX_THREADS) void map_values(const uint32_t *__restrict__ hu, const uint8_t *__restrict__ sel, const uint32_t *__restrict__ keys, int nU,
                                                         uint32_t *__restrict__ out, int64_t N)
{
    __shared__ uint32_t tab[LDS ? MAP_LDS_ROWS : 1];
    if (LDS) {
        for (int q = threadIdx.x; q < nU; q += VX_THREADS) tab[q] = keys[q];
        __syncthreads();
    }
    const uint32_t *t = LDS ? tab : keys;
    const int64_t n4 = N >> 2;
    for (int64_t q = (int64_t)blockIdx.x * VX_THREADS + threadIdx.x; q < n4; q += (int64_t)gridDim.x * VX_THREADS) {            // grid-stride: ends
        const uint4 h = ((const uint4 *)hu)[q];
        const uint32_t s = ((const uint32_t *)sel)[q];
        uint4 r;
        r.x = (s & 0xFFu) ? map_lookup(t, nU, h.x) : 0u;
        r.y = (s & 0xFF00u) ? map_lookup(t, nU, h.y) : 0u;
        r.z = (s & 0xFF0000u) ? map_lookup(t, nU, h.z) : 0u;
        r.w = (s & 0xFF000000u) ? map_lookup(t, nU, h.w) : 0u;
        ((uint4 *)out)[q] = r;
    }
    const int64_t v = 4 * n4 + (int64_t)blockIdx.x * VX_THREADS + threadIdx.x;      // the last N % 4 voxels
    if (v < N) out[v] = sel[v] ? map_lookup(t, nU, hu[v]) : 0u;
}

// the grid is usable: every extent in 1 .. 2^31 - 1 and at most VOX_MAX_VOXELS voxels, the product formed without overflow
bool grid_fits(int64_t gx, int64_t gy, int64_t gz)
{
    const int64_t LIMIT = ((int64_t)1 << 31) - 1;
    if (gx < 1 || gy < 1 || gz < 1 || gx > LIMIT || gy > LIMIT || gz > LIMIT) return false;
    if (gx > VOX_MAX_VOXELS / gy) return false;
    return gx * gy <= VOX_MAX_VOXELS / gz;
}

// the triangle count, grid and box errors of a call that starts from a mesh, in the order bfd_voxelize_mesh reports them; *g receives the grid
int mesh_grid_errors(const char *who, int64_t nTriangles, const double *min, const double *max, int64_t gx, int64_t gy, int64_t gz, vox_grid *g)
{
    if (nTriangles < 1) BFD_FAIL(-1, std::string(who) + ": at least one triangle is needed");
    if (nTriangles >= ((int64_t)1 << 31)) BFD_FAIL(-1, std::string(who) + ": 2^31 triangles or more");
    if (gx < 1 || gy < 1 || gz < 1) BFD_FAIL(-1, std::string(who) + ": every grid extent must be at least 1");
    if (!grid_fits(gx, gy, gz)) BFD_FAIL(-1, std::string(who) + ": the grid has an extent of 2^31 or more, or more than 2^40 voxels");
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(min[a]) || !std::isfinite(max[a])) BFD_FAIL(-1, std::string(who) + ": the box is not finite");
        if (!(max[a] > min[a])) BFD_FAIL(-1, std::string(who) + ": the box must have max > min on every axis");
    }
    *g = vox_make_grid(min, max, gx, gy, gz);
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(g->u[a]) || !(g->u[a] > 0)) BFD_FAIL(-1, std::string(who) + ": the voxel size (max - min) / g is not a positive finite number");
    return 0;
}

int mesh_vertex_errors(const char *who, const float *triangles, int64_t nTriangles)
{
    for (int64_t q = 0; q < 9 * nTriangles; q++)
        if (!std::isfinite(triangles[q])) BFD_FAIL(-1, std::string(who) + ": vertex coordinate " + std::to_string(q) + " is not finite");
    return 0;
}

// What a mesh leaves on the device on its way to the table; lives for the call.
struct MeshTable {
    DevTemp<float> dtri;
    DevTemp<vox_tri> recs;
    DevTemp<int64_t> ends;
    DevTemp<uint64_t> cross, occ;
    DevTemp<uint32_t> table;
    DevTemp<unsigned long long> count;
    InclusiveSum<int64_t> sum;
};

// Steps 5-8 of a call that starts from a mesh (bfd_voxelize_mesh, bfd_voxelize_scatter3d): the temporaries, the upload of the triangles,
// Events::record(0), then the memsets and kernels that leave the table and its population on the device. The caller's own temporaries are made
// before this; its kernels follow on the null stream, inside the same timed section.
int mesh_to_table(const char *who, const float *triangles, int64_t n, const vox_grid &g, MeshTable &t, Events &ev)
{
    const int64_t nWords = g.nColumns * g.rowWords, nTable = (g.nVoxels + 31) / 32;
    BFD_STEP(t.dtri.alloc((size_t)n * 9));
    BFD_STEP(t.recs.alloc((size_t)n));
    BFD_STEP(t.ends.alloc((size_t)n));
    BFD_STEP(t.cross.alloc((size_t)nWords));
    BFD_STEP(t.occ.alloc((size_t)nWords));
    BFD_STEP(t.table.alloc((size_t)nTable));
    BFD_STEP(t.count.alloc(1));
    BFD_STEP(t.sum.reserve(t.ends, (size_t)n));
    BFD_STEP(hipMemcpy(t.dtri, triangles, (size_t)n * 36, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    BFD_STEP(hipMemsetAsync(t.cross, 0, (size_t)nWords * 8, 0));
    BFD_STEP(hipMemsetAsync(t.count, 0, 8, 0));
    hipLaunchKernelGGL(vox_setup, dim3(blocks_for(n, VX_THREADS, MAX_BLOCKS)), dim3(VX_THREADS), 0, 0, t.dtri.p, n, g, t.recs.p, t.ends.p);
    BFD_STEP(hipGetLastError());
    BFD_STEP(t.sum.run(t.ends, (size_t)n));
    // the pair count stays on the device: the launch is sized by its bound n gy gz, the kernel reads the count itself
    const int64_t bound = n > VOX_SWEEP_BLOCKS * VX_THREADS / g.nColumns ? VOX_SWEEP_BLOCKS * VX_THREADS : n * g.nColumns;
    hipLaunchKernelGGL(vox_crossings, dim3(blocks_for(bound, VX_THREADS, VOX_SWEEP_BLOCKS)), dim3(VX_THREADS), 0, 0, t.recs.p, t.ends.p, n, g,
                       (unsigned long long *)t.cross.p);
    hipLaunchKernelGGL(vox_scan, dim3(blocks_for(nWords, VX_THREADS, MAX_BLOCKS)), dim3(VX_THREADS), 0, 0, t.cross.p, t.occ.p, g, nWords);
    hipLaunchKernelGGL(vox_pack, dim3(blocks_for(nTable, VX_THREADS, MAX_BLOCKS)), dim3(VX_THREADS), 0, 0, t.occ.p, t.table.p, g, nTable, t.count.p);
    BFD_STEP(hipGetLastError());
    return 0;
}

// The argument errors the two conformal entries share, after their grid and box errors and in the header's order; `inputs` are the entry's input
// ranges (pointer, bytes), which `out` may not overlap.
struct ByteRange { const void *p; size_t bytes; };
int conformal_errors(const char *who, const float *matrix, int64_t M1, int64_t M2, int64_t M3, const uint8_t *out, const int64_t *lo, const int64_t *hi,
                     const int64_t *counts, const ByteRange *inputs, int nInputs)
{
    for (int q = 0; q < 12; q++)
        if (!std::isfinite(matrix[q])) BFD_FAIL(-1, std::string(who) + ": the matrix is not finite");
    if (out) {
        if (M1 < 1 || M2 < 1 || M3 < 1) BFD_FAIL(-1, std::string(who) + ": every extent of out must be at least 1");
        if (!volume_fits(M1, M2, M3)) BFD_FAIL(-1, std::string(who) + ": out has 2^31 voxels or more");
        for (int q = 0; q < nInputs; q++)
            if (overlap(out, (size_t)(M1 * M2 * M3), inputs[q].p, inputs[q].bytes)) BFD_FAIL(-1, std::string(who) + ": out may not alias an input");
    }
    if ((lo == nullptr) != (hi == nullptr)) BFD_FAIL(-1, std::string(who) + ": lo and hi come together");
    if (!out && !lo && !counts) BFD_FAIL(-1, std::string(who) + ": no output asked for");
    return 0;
}

// The device side of a scatter from a table that is on the device: the output temporaries (step 5, with the start values of the bounds uploaded:
// step 6), the kernel (step 8), the results (step 11). Between alloc and launch the caller records event 0 (or mesh_to_table does).
struct Conformal {
    DevTemp<uint8_t> out;
    DevTemp<conf_result> res;
    conf_args a;
    size_t nOut = 0;

    Conformal(const vox_grid &g, const float *matrix, int64_t M1, int64_t M2, int64_t M3, bool write)
    {
        a.gx = g.gx; a.gy = g.gy; a.rows = g.nColumns; a.chunks = (g.gx + 63) / 64;
        for (int q = 0; q < 3; q++) { a.min[q] = g.min[q]; a.unit[q] = g.u[q]; }
        memcpy(a.m, matrix, sizeof a.m);
        a.M[0] = write ? M1 : 1; a.M[1] = write ? M2 : 1; a.M[2] = write ? M3 : 1;
        nOut = write ? (size_t)(M1 * M2 * M3) : 0;
    }
    int alloc(const char *who)
    {
        const conf_result start = {{INT32_MAX, INT32_MAX, INT32_MAX}, {INT32_MIN, INT32_MIN, INT32_MIN}, {0, 0, 0, 0}};
        if (nOut) BFD_STEP(out.alloc(nOut));
        BFD_STEP(res.alloc(1));
        BFD_STEP(hipMemcpy(res, &start, sizeof start, hipMemcpyHostToDevice));
        return 0;
    }
    int launch(const char *who, const uint32_t *table)
    {
        const unsigned blocks = blocks_for(a.rows * a.chunks, VX_THREADS / 64, CONF_SWEEP_BLOCKS);
        if (nOut) {
            BFD_STEP(hipMemsetAsync(out, 0, nOut, 0));
            hipLaunchKernelGGL(conf_scatter<true>, dim3(blocks), dim3(VX_THREADS), 0, 0, table, out.p, res.p, a);
        } else
            hipLaunchKernelGGL(conf_scatter<false>, dim3(blocks), dim3(VX_THREADS), 0, 0, table, (uint8_t *)nullptr, res.p, a);
        BFD_STEP(hipGetLastError());
        return 0;
    }
    // lo and hi are left alone when there was no point
    int download(const char *who, uint8_t *hout, int64_t *lo, int64_t *hi, int64_t *counts)
    {
        conf_result r;
        if (hout) BFD_STEP(hipMemcpy(hout, out, nOut, hipMemcpyDeviceToHost));
        BFD_STEP(hipMemcpy(&r, res, sizeof r, hipMemcpyDeviceToHost));
        for (int q = 0; q < 3 && lo && r.counts[0]; q++) { lo[q] = r.lo[q]; hi[q] = r.hi[q]; }
        for (int q = 0; q < 4 && counts; q++) counts[q] = (int64_t)r.counts[q];
        return 0;
    }
};

}  // namespace

extern "C" int bfd_voxelize_mesh(int device, const float *triangles, int64_t nTriangles, const double *min, const double *max,
                                 int64_t gx, int64_t gy, int64_t gz, uint32_t *table, uint8_t *mask, int64_t *count, float *kernelMs)
{
    static const char *who = "bfd_voxelize_mesh";
    // every argument error is reported before a device is looked for
    if (!triangles || !min || !max) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (!table && !mask && !count) BFD_FAIL(-1, std::string(who) + ": no output asked for");
    vox_grid g;
    if (int rc = mesh_grid_errors(who, nTriangles, min, max, gx, gy, gz, &g)) return rc;
    if (mask && g.nVoxels >= ((int64_t)1 << 31)) BFD_FAIL(-1, std::string(who) + ": a mask is written only below 2^31 voxels (ask for the table)");
    if (int rc = mesh_vertex_errors(who, triangles, nTriangles)) return rc;
    const int64_t nTable = (g.nVoxels + 31) / 32;
    const size_t tb = (size_t)nTable * 4, mb = (size_t)g.nVoxels;
    if ((table && overlap(table, tb, triangles, (size_t)nTriangles * 36)) || (mask && overlap(mask, mb, triangles, (size_t)nTriangles * 36)) ||
        (table && mask && overlap(table, tb, mask, mb)))
        BFD_FAIL(-1, std::string(who) + ": an output may not alias the triangles or another output");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;

    MeshTable t;
    DevTemp<uint8_t> dmask;
    Events ev;
    unsigned long long total = 0;
    if (mask) BFD_STEP(dmask.alloc(mb));
    if (int rc = mesh_to_table(who, triangles, nTriangles, g, t, ev)) return rc;
    if (mask) hipLaunchKernelGGL(vox_expand, dim3(blocks_for(nTable, VX_THREADS, MAX_BLOCKS)), dim3(VX_THREADS), 0, 0, t.table.p, dmask.p, nTable, g.nVoxels);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    if (table) BFD_STEP(hipMemcpy(table, t.table, tb, hipMemcpyDeviceToHost));
    if (mask) BFD_STEP(hipMemcpy(mask, dmask, mb, hipMemcpyDeviceToHost));
    if (count) {
        BFD_STEP(hipMemcpy(&total, t.count, 8, hipMemcpyDeviceToHost));
        *count = (int64_t)total;
    }
    return 0;
}

extern "C" int bfd_voxelize_scatter3d(int device, const float *triangles, int64_t nTriangles, const double *min, const double *max,
                                      int64_t gx, int64_t gy, int64_t gz, const float *matrix, int64_t M1, int64_t M2, int64_t M3,
                                      uint8_t *out, int64_t *lo, int64_t *hi, int64_t *counts, float *kernelMs)
{
    static const char *who = "bfd_voxelize_scatter3d";
    if (!triangles || !min || !max || !matrix) BFD_FAIL(-1, std::string(who) + ": null argument");
    vox_grid g;
    if (int rc = mesh_grid_errors(who, nTriangles, min, max, gx, gy, gz, &g)) return rc;
    if (int rc = mesh_vertex_errors(who, triangles, nTriangles)) return rc;
    const ByteRange inputs[] = {{triangles, (size_t)nTriangles * 36}, {min, 24}, {max, 24}, {matrix, 48}};
    if (int rc = conformal_errors(who, matrix, M1, M2, M3, out, lo, hi, counts, inputs, 4)) return rc;

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;

    MeshTable t;
    Conformal c(g, matrix, M1, M2, M3, out != nullptr);
    Events ev;
    if (int rc = c.alloc(who)) return rc;
    if (int rc = mesh_to_table(who, triangles, nTriangles, g, t, ev)) return rc;
    if (int rc = c.launch(who, t.table)) return rc;
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    return c.download(who, out, lo, hi, counts);
}

extern "C" int bfd_voxel_scatter3d(int device, const uint32_t *table, int64_t gx, int64_t gy, int64_t gz, const double *min, const double *unit,
                                   const float *matrix, int64_t M1, int64_t M2, int64_t M3, uint8_t *out, int64_t *lo, int64_t *hi, int64_t *counts,
                                   float *kernelMs)
{
    static const char *who = "bfd_voxel_scatter3d";
    if (!table || !min || !unit || !matrix) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (gx < 1 || gy < 1 || gz < 1) BFD_FAIL(-1, std::string(who) + ": every grid extent must be at least 1");
    if (!grid_fits(gx, gy, gz)) BFD_FAIL(-1, std::string(who) + ": the grid has an extent of 2^31 or more, or more than 2^40 voxels");
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(min[a]) || !std::isfinite(unit[a])) BFD_FAIL(-1, std::string(who) + ": min and unit must be finite");
    vox_grid g = vox_make_grid(min, min, gx, gy, gz);            // the extents and min; the caller names the voxel size itself
    for (int a = 0; a < 3; a++) g.u[a] = unit[a];
    const size_t tb = (size_t)((g.nVoxels + 31) / 32) * 4;
    const ByteRange inputs[] = {{table, tb}, {min, 24}, {unit, 24}, {matrix, 48}};
    if (int rc = conformal_errors(who, matrix, M1, M2, M3, out, lo, hi, counts, inputs, 4)) return rc;

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;

    DevTemp<uint32_t> dtable;
    Conformal c(g, matrix, M1, M2, M3, out != nullptr);
    Events ev;
    BFD_STEP(dtable.alloc(tb / 4));
    if (int rc = c.alloc(who)) return rc;
    BFD_STEP(hipMemcpy(dtable, table, tb, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    if (int rc = c.launch(who, dtable)) return rc;
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    return c.download(who, out, lo, hi, counts);
}

extern "C" int bfd_voxel_points(int device, const uint32_t *table, int64_t gx, int64_t gy, int64_t gz, const double *min, const double *unit,
                                float *points, int64_t capacity, int64_t *count, float *kernelMs)
{
    static const char *who = "bfd_voxel_points";
    if (!table || !min || !unit) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (gx < 1 || gy < 1 || gz < 1) BFD_FAIL(-1, std::string(who) + ": every grid extent must be at least 1");
    if (!grid_fits(gx, gy, gz)) BFD_FAIL(-1, std::string(who) + ": the grid has an extent of 2^31 or more, or more than 2^40 voxels");
    if (capacity < 0) BFD_FAIL(-1, std::string(who) + ": negative capacity");
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(min[a]) || !std::isfinite(unit[a])) BFD_FAIL(-1, std::string(who) + ": min and unit must be finite");
    const int64_t nVoxels = gx * gy * gz, nTable = (nVoxels + 31) / 32;
    // the table is the caller's: its population is known before a device is, and so is whether the points fit
    int64_t total = 0;
    for (int64_t o = 0; o < nTable; o++) total += __builtin_popcount(table[o] & vox_table_valid(o, nVoxels));
    if (count) *count = total;
    if (capacity < total) BFD_FAIL(-1, std::string(who) + ": the table holds " + std::to_string(total) + " voxels, capacity is " + std::to_string(capacity));
    if (total > 0 && !points) BFD_FAIL(-1, std::string(who) + ": null points");
    if (total > 0 && overlap(points, (size_t)total * 12, table, (size_t)nTable * 4)) BFD_FAIL(-1, std::string(who) + ": points may not alias the table");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (total == 0) return 0;

    pts_args a;
    a.gx = gx; a.gy = gy; a.nVoxels = nVoxels;
    for (int q = 0; q < 3; q++) { a.min[q] = min[q]; a.unit[q] = unit[q]; }
    DevTemp<uint32_t> dtable;
    DevTemp<int64_t> ends;
    DevTemp<float> dpts;
    InclusiveSum<int64_t> sum;
    Events ev;
    BFD_STEP(dtable.alloc((size_t)nTable));
    BFD_STEP(ends.alloc((size_t)nTable));
    BFD_STEP(dpts.alloc((size_t)total * 3));
    BFD_STEP(sum.reserve(ends, (size_t)nTable));
    BFD_STEP(hipMemcpy(dtable, table, (size_t)nTable * 4, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    const unsigned tbk = blocks_for(nTable, VX_THREADS, MAX_BLOCKS);
    hipLaunchKernelGGL(pts_count, dim3(tbk), dim3(VX_THREADS), 0, 0, dtable.p, ends.p, nTable, nVoxels);
    BFD_STEP(hipGetLastError());
    BFD_STEP(sum.run(ends, (size_t)nTable));
    hipLaunchKernelGGL(pts_write, dim3(tbk), dim3(VX_THREADS), 0, 0, dtable.p, ends.p, dpts.p, nTable, a);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    BFD_STEP(hipMemcpy(points, dpts, (size_t)total * 12, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int bfd_map_values3d(int device, const float *hu, const uint8_t *sel, const float *unique, int64_t nU, uint32_t *out, int64_t N,
                                float *kernelMs)
{
    static const char *who = "bfd_map_values3d";
    if (!hu || !sel || !unique || !out) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (N < 0) BFD_FAIL(-1, std::string(who) + ": negative size");
    if (nU < 1 || nU > MAP_MAX_ROWS) BFD_FAIL(-1, std::string(who) + ": the table must have 1 .. 65536 rows");
    if (unique[0] != unique[0]) BFD_FAIL(-1, std::string(who) + ": the table holds a NaN");
    for (int64_t m = 1; m < nU; m++)
        if (!(unique[m - 1] < unique[m])) BFD_FAIL(-1, std::string(who) + ": the table must be strictly increasing (row " + std::to_string(m) + " is not above the row before it)");
    const size_t n = (size_t)N;
    if (n && (overlap(out, 4 * n, hu, 4 * n) || overlap(out, 4 * n, sel, n) || overlap(out, 4 * n, unique, (size_t)nU * 4)))
        BFD_FAIL(-1, std::string(who) + ": out may not alias an input");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) return 0;

    std::vector<uint32_t> keys((size_t)nU);
    memcpy(keys.data(), unique, (size_t)nU * 4);
    for (uint32_t &k : keys) k = map_key(k);
    DevTemp<uint32_t> dhu, duni, dout;
    DevTemp<uint8_t> dsel;
    Events ev;
    BFD_STEP(dhu.alloc(n));
    BFD_STEP(dsel.alloc(n));
    BFD_STEP(duni.alloc((size_t)nU));
    BFD_STEP(dout.alloc(n));
    BFD_STEP(hipMemcpy(dhu, hu, 4 * n, hipMemcpyHostToDevice));
    BFD_STEP(hipMemcpy(dsel, sel, n, hipMemcpyHostToDevice));
    BFD_STEP(hipMemcpy(duni, keys.data(), (size_t)nU * 4, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    // at least one block's worth of lanes for the N % 4 tail; every block stages the table, so no more blocks than keep the device full
    const unsigned blocks = blocks_for(N / 4, VX_THREADS, 8192);
    if (nU <= MAP_LDS_ROWS) hipLaunchKernelGGL(map_values<true>, dim3(blocks), dim3(VX_THREADS), 0, 0, dhu.p, dsel.p, duni.p, (int)nU, dout.p, N);
    else hipLaunchKernelGGL(map_values<false>, dim3(blocks), dim3(VX_THREADS), 0, 0, dhu.p, dsel.p, duni.p, (int)nU, dout.p, N);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    BFD_STEP(hipMemcpy(out, dout, 4 * n, hipMemcpyDeviceToHost));
    return 0;
}
