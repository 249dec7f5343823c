// Binary morphology and component labelling of Step-1 masks on MI355X, in the caller's numpy C order (k fastest).
//
// Replaces, after the median of BabelDatasetPreps.py:870-876,
//     BinaryClosingFilter(fct, structure=np.ones(sf2, int))          BabelDatasetPreps.py:881-883 (scipy.ndimage.binary_closing; sf2 = 14 at 0.3675 mm)
//     binary_dilation(mask, iterations=6), binary_erosion(mask, iterations=n)     :901, :953, :1106
//     LabelImage(nfct), regionprops, the largest region              :888-894, :910-929, :1055-1058, :1078-1081
//     the same with np.isin(label_img, AllLabels) and a masked store :909-929, :1055-1061, :1077-1097 (bfd_paint_components3d: the labels stay here)
//
// Morphology. The mask is packed to one bit per voxel along k (__ballot: 64 voxels per wave-wide word; layout in bfd_morph_core.h) and every pass
// works on whole words, one thread per word:
//   box path (all-ones structure, 1..31 per axis): three 1-D passes per erosion / dilation, k (shifts across the two neighbouring words), then
//     j and i (AND / OR of whole words). s taps per word and pass, never s1 s2 s3.
//   general path (any structure up to 7 x 7 x 7, NULL = the cross): the true elements as a tap list grouped by (di, dj), one launch per iteration.
//   Both ping-pong two packed buffers. Outside the volume (and past N3 in a row's last word) every reader sees the border value.
// Labelling. Union-find on linear voxel indices; a parent is never larger than its child, so a root is its component's first voxel in raster order:
//   1. one workgroup per 8 x 8 x 64 tile: union-find of the tile in LDS (local ids), written out as global indices
//   2. one thread per voxel: unions with the preceding neighbours that lie in another tile (faces, edges, corners), atomicMin in global memory
//   3. flatten: every voxel points at its root
//   4. roots (parent == self) flagged, inclusive prefix sum in raster order (rocPRIM): label of a component = rank of its root, scipy's numbering
//   5. sizes by one histogram pass (one atomic per wave and distinct label), the largest by a reduction, its mask
//   Steps 1-5 up to the sizes are `Labelling`, which bfd_label3d and bfd_paint_components3d both run.
// Painting. A flag per label from the sizes and the largest (paint_flags: all but the largest, the ones below a tenth of it, or the largest alone),
//   then out = in with the voxels of flagged labels set to the fill value (paint_write): 6 B per voxel, and the int32 labels never reach the host.
// No kernel waits for another workgroup; every loop is bounded, see the comment at each.
#include <string.h>
#include "bfd_internal.h"
#include "bfd_call.h"
#include "bfd_scan.h"
#include "bfd_morph_core.h"
#include "bfd_step1_stages.h"

namespace {

constexpr int MB_THREADS = 256;
constexpr int MAX_BOX = 31;
constexpr long MAX_BLOCKS = 1L << 16;             // work beyond this is taken by grid-stride loops

// ---------------------------------------------------------------- morphology kernels ----------------------------------------------------------------

// one wave per word: lane l holds voxel 64 w + l of the row
__global__ __launch_bounds__(MB_THREADS) void morph_pack(const uint8_t *__restrict__ in, uint64_t *__restrict__ bits, const morph_dims g, long nWords)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // grid-stride, the same trip count for every lane of a wave (the word index is wave-uniform): ends after ceil(nWords / (4 gridDim)) rounds
    for (long wd = (long)blockIdx.x * (MB_THREADS / 64) + wave; wd < nWords; wd += (long)gridDim.x * (MB_THREADS / 64)) {
        const long row = wd / g.nW;
        const int w = (int)(wd - row * g.nW), k = w * 64 + lane;
        const bool on = k < g.N3 && in[row * g.N3 + k] != 0;
        const unsigned long long b = __ballot(on);
        if (lane == 0) bits[wd] = b;
    }
}

__global__ __launch_bounds__(MB_THREADS) void morph_unpack(const uint64_t *__restrict__ bits, uint8_t *__restrict__ out, const morph_dims g, long nVox)
{
    for (long v = (long)blockIdx.x * MB_THREADS + threadIdx.x; v < nVox; v += (long)gridDim.x * MB_THREADS) {      // grid-stride: ends
        const long row = v / g.N3;
        const int k = (int)(v - row * g.N3);
        out[v] = (uint8_t)((bits[row * g.nW + (k >> 6)] >> (k & 63)) & 1u);
    }
}

// axis 0, 1: whole words along i, j; axis 2: along k
__global__ __launch_bounds__(MB_THREADS) void morph_box_pass(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, const morph_dims g, long nWords,
                                                             int axis, int lo, int hi, int dilate, uint64_t fill)
{
    for (long wd = (long)blockIdx.x * MB_THREADS + threadIdx.x; wd < nWords; wd += (long)gridDim.x * MB_THREADS) {  // grid-stride: ends
        const long row = wd / g.nW;
        const int w = (int)(wd - row * g.nW), i = (int)(row / g.N2), j = (int)(row - (long)i * g.N2);
        dst[wd] = axis == 2 ? morph_pass_k(src, g, i, j, w, lo, hi, dilate != 0, fill) : morph_pass_ij(src, g, i, j, w, axis, lo, hi, dilate != 0, fill);
    }
}

__global__ __launch_bounds__(MB_THREADS) void morph_general_pass(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, const morph_dims g, long nWords,
                                                                 const morph_taps t, int dilate, uint64_t fill)
{
    for (long wd = (long)blockIdx.x * MB_THREADS + threadIdx.x; wd < nWords; wd += (long)gridDim.x * MB_THREADS) {  // grid-stride: ends
        const long row = wd / g.nW;
        const int w = (int)(wd - row * g.nW), i = (int)(row / g.N2), j = (int)(row - (long)i * g.N2);
        dst[wd] = morph_general(src, g, i, j, w, t, dilate != 0, fill);
    }
}

// ---------------------------------------------------------------- labelling kernels ----------------------------------------------------------------

// Parents are read with relaxed atomic loads: another thread may lower them at any time, and a value once read is still an ancestor-or-equal candidate
// that the caller's atomicMin checks.
static __device__ __forceinline__ int uf_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of x. Ends: a parent that is not the voxel itself is strictly smaller (the invariant parent <= child is kept by every write: uf_union only
// stores values smaller than the index it stores to, and the flatten stores roots), so x strictly decreases and is bounded by 0.
static __device__ __forceinline__ int uf_find(const int *L, int x)
{
    int p = uf_load(L + x);
    while (p != x) { x = p; p = uf_load(L + x); }
    return x;
}

// Joins the components of a and b. Ends: every round that does not return replaces a by a value read back from L[a] that differs from a; L[a] only
// ever holds a or smaller, so the new a is strictly smaller, while b never grows (find only descends): a + b strictly decreases and is bounded by 0.
// A retry therefore happens only after an atomicMin found L[a] already lowered by someone else; the link that our own atomicMin may have replaced
// (old, when b < old) is re-made by the next round, which joins old with b.
static __device__ __forceinline__ void uf_union(int *L, int a, int b)
{
    while (true) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b);        // a was a root when read: L[a] == a unless another thread linked it meanwhile
        if (old == a) return;
        a = old;
    }
}

struct label_dims { int N1, N2, N3, nTj, nTk; long nTiles; int conn; };

// 1. local union-find of one tile in LDS. The foreground is in != 0, or in == value where value >= 0 (bfd_paint_components3d)
__global__ __launch_bounds__(MB_THREADS) void label_local(const uint8_t *__restrict__ in, int *__restrict__ L, const label_dims g, const int value)
{
    __shared__ int lab[LT_VOX];                       // 16 KiB
    for (long t = blockIdx.x; t < g.nTiles; t += gridDim.x) {          // grid-stride over tiles, block-uniform: ends
        const int bk = (int)(t % g.nTk);
        const long q = t / g.nTk;
        const int bj = (int)(q % g.nTj), bi = (int)(q / g.nTj);
        const int i0 = bi * LT_I, j0 = bj * LT_J, k0 = bk * LT_K;
        __syncthreads();                              // the tile before this one has been written out
        for (int v = threadIdx.x; v < LT_VOX; v += MB_THREADS) {
            const int i = i0 + v / (LT_J * LT_K), j = j0 + (v / LT_K) % LT_J, k = k0 + v % LT_K;
            bool on = i < g.N1 && j < g.N2 && k < g.N3;
            if (on) {
                const int x = in[((long)i * g.N2 + j) * g.N3 + k];
                on = value < 0 ? x != 0 : x == value;
            }
            lab[v] = on ? v : -1;
        }
        __syncthreads();
        for (int v = threadIdx.x; v < LT_VOX; v += MB_THREADS) {
            if (uf_load(lab + v) < 0) continue;       // background stays -1 for ever
            const int ii = v / (LT_J * LT_K), jj = (v / LT_K) % LT_J, kk = v % LT_K;
            for (int nb = 0; nb < 13; nb++) {
                int di, dj, dk;
                if (!label_backward_neighbour(nb, g.conn, &di, &dj, &dk)) continue;
                const int ni = ii + di, nj = jj + dj, nk = kk + dk;
                if (ni < 0 || nj < 0 || nj >= LT_J || nk < 0 || nk >= LT_K) continue;       // in another tile: step 2
                const int u = (ni * LT_J + nj) * LT_K + nk;
                if (uf_load(lab + u) >= 0) uf_union(lab, v, u);
            }
        }
        __syncthreads();
        for (int v = threadIdx.x; v < LT_VOX; v += MB_THREADS) {
            const int i = i0 + v / (LT_J * LT_K), j = j0 + (v / LT_K) % LT_J, k = k0 + v % LT_K;
            if (i >= g.N1 || j >= g.N2 || k >= g.N3) continue;
            int r = lab[v];
            if (r >= 0) {
                r = uf_find(lab, v);                  // nobody writes lab any more
                r = (int)(((long)(i0 + r / (LT_J * LT_K)) * g.N2 + j0 + (r / LT_K) % LT_J) * g.N3 + k0 + r % LT_K);
            }
            L[((long)i * g.N2 + j) * g.N3 + k] = r;
        }
    }
}

// 2. unions across tile faces, edges and corners
__global__ __launch_bounds__(MB_THREADS) void label_merge(int *__restrict__ L, const label_dims g, long nVox)
{
    for (long v = (long)blockIdx.x * MB_THREADS + threadIdx.x; v < nVox; v += (long)gridDim.x * MB_THREADS) {      // grid-stride: ends
        const long row = v / g.N3;
        const int k = (int)(v - row * g.N3), i = (int)(row / g.N2), j = (int)(row - (long)i * g.N2);
        // a preceding neighbour is (i - 1, j +- 1, k +- 1), (i, j - 1, k +- 1) or (i, j, k - 1): away from the tile's low i face and from both of
        // its j and k faces all of them lie in the same tile
        const int tj = j % LT_J, tk = k % LT_K;
        if ((i % LT_I) && tj && tj != LT_J - 1 && tk && tk != LT_K - 1) continue;
        if (uf_load(L + v) < 0) continue;
        for (int nb = 0; nb < 13; nb++) {
            int di, dj, dk;
            if (!label_backward_neighbour(nb, g.conn, &di, &dj, &dk)) continue;
            const int ni = i + di, nj = j + dj, nk = k + dk;
            if (ni < 0 || nj < 0 || nj >= g.N2 || nk < 0 || nk >= g.N3) continue;
            if (ni / LT_I == i / LT_I && nj / LT_J == j / LT_J && nk / LT_K == k / LT_K) continue;     // joined in step 1
            const long u = ((long)ni * g.N2 + nj) * g.N3 + nk;
            if (uf_load(L + u) >= 0) uf_union(L, (int)v, (int)u);
        }
    }
}

// 3. every voxel points at its root; flag[v] = 1 at roots. Concurrent flattening only replaces a parent by an ancestor: the invariant holds.
__global__ __launch_bounds__(MB_THREADS) void label_flatten(int *__restrict__ L, int *__restrict__ flag, long nVox)
{
    for (long v = (long)blockIdx.x * MB_THREADS + threadIdx.x; v < nVox; v += (long)gridDim.x * MB_THREADS) {      // grid-stride: ends
        int r = uf_load(L + v);
        if (r >= 0) {
            r = uf_find(L, (int)v);
            __hip_atomic_store(L + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        flag[v] = r == (int)v ? 1 : 0;
    }
}

// 4. label = rank of the root among the roots (rank: inclusive prefix sum of the flags). In place: L[v] is read by thread v alone.
__global__ __launch_bounds__(MB_THREADS) void label_assign(int *__restrict__ L, const int *__restrict__ rank, long nVox)
{
    for (long v = (long)blockIdx.x * MB_THREADS + threadIdx.x; v < nVox; v += (long)gridDim.x * MB_THREADS) {      // grid-stride: ends
        const int r = L[v];
        L[v] = r >= 0 ? rank[r] : 0;
    }
}

// 5a. voxel counts: the lanes of a wave that hold the same label add once
__global__ __launch_bounds__(MB_THREADS) void label_sizes(const int *__restrict__ labels, unsigned long long *__restrict__ sizes, long nVox)
{
    const int lane = threadIdx.x & 63;
    const long rounds = (nVox + (long)gridDim.x * MB_THREADS - 1) / ((long)gridDim.x * MB_THREADS);
    for (long it = 0; it < rounds; it++) {            // the same trip count for every thread (the ballots below need whole waves)
        const long v = (it * gridDim.x + blockIdx.x) * MB_THREADS + threadIdx.x;
        const int lab = v < nVox ? labels[v] : 0;
        unsigned long long todo = __ballot(lab > 0);
        while (todo) {                                // ends: wave-uniform, and every round clears at least its leader's bit (at most 64 rounds)
            const int leader = __ffsll(todo) - 1;
            const int which = __shfl(lab, leader);
            const unsigned long long same = __ballot(lab == which) & todo;
            if (lane == leader) atomicAdd(sizes + (which - 1), (unsigned long long)__popcll(same));
            todo &= ~same;
        }
    }
}

// 5b. the label with the most voxels, among equals the highest; one workgroup. best[0] = label (0: no component)
__global__ __launch_bounds__(1024) void label_largest(const unsigned long long *__restrict__ sizes, int n, int *__restrict__ best)
{
    __shared__ unsigned long long sz[1024];
    __shared__ int id[1024];
    unsigned long long s = 0;
    int b = 0;
    for (int q = threadIdx.x; q < n; q += 1024)       // ascending labels: >= lets the later of two equals win
        if (sizes[q] >= s) { s = sizes[q]; b = q + 1; }
    sz[threadIdx.x] = s; id[threadIdx.x] = b;
    __syncthreads();
    for (int h = 512; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const unsigned long long s2 = sz[threadIdx.x + h];
            const int b2 = id[threadIdx.x + h];
            if (s2 > sz[threadIdx.x] || (s2 == sz[threadIdx.x] && b2 > id[threadIdx.x])) { sz[threadIdx.x] = s2; id[threadIdx.x] = b2; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) best[0] = id[0];
}

// 5b with the other tie rule: among equals the lowest label, what sorted(props, key=pixelcount, reverse=True)[0] selects (CTZTEProcessing.py:604-606)
__global__ __launch_bounds__(1024) void label_largest_lowest(const unsigned long long *__restrict__ sizes, int n, int *__restrict__ best)
{
    __shared__ unsigned long long sz[1024];
    __shared__ int id[1024];
    unsigned long long s = 0;
    int b = 0;
    for (int q = threadIdx.x; q < n; q += 1024)       // ascending labels: > lets the earlier of two equals stay
        if (sizes[q] > s) { s = sizes[q]; b = q + 1; }
    sz[threadIdx.x] = s; id[threadIdx.x] = b;
    __syncthreads();
    for (int h = 512; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const unsigned long long s2 = sz[threadIdx.x + h];
            const int b2 = id[threadIdx.x + h];
            // b2 == 0 is a thread without a component (s2 == 0): it never wins, a component has a voxel
            if (s2 > sz[threadIdx.x] || (s2 == sz[threadIdx.x] && b2 > 0 && b2 < id[threadIdx.x])) { sz[threadIdx.x] = s2; id[threadIdx.x] = b2; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) best[0] = id[0];
}

__global__ __launch_bounds__(MB_THREADS) void label_select(const int *__restrict__ labels, const int *__restrict__ best, uint8_t *__restrict__ out, long nVox)
{
    const int b = best[0];
    for (long v = (long)blockIdx.x * MB_THREADS + threadIdx.x; v < nVox; v += (long)gridDim.x * MB_THREADS)        // grid-stride: ends
        out[v] = (b > 0 && labels[v] == b) ? 1 : 0;
}

// ---------------------------------------------------------------- painting by size ----------------------------------------------------------------

// acc[0] = size of the largest component, acc[1] = components painted, acc[2] = voxels painted. flag[q] = 1 where label q + 1 is painted:
// select 0: all but the largest; 1: those of the others whose size a has (double)a < 0.1 * (double)L, the product formed once in float64 as Python
// forms 0.1*regions[-1].area; 2: the largest alone. `best` is label_largest's: among equal sizes the highest label is the largest.
__global__ __launch_bounds__(MB_THREADS) void paint_flags(const unsigned long long *__restrict__ sizes, int n, const int *__restrict__ best, int select,
                                                          uint8_t *__restrict__ flag, unsigned long long *__restrict__ acc)
{
    const int b = best[0];
    const unsigned long long big = b > 0 ? sizes[b - 1] : 0;
    const double limit = 0.1 * (double)big;
    unsigned long long comps = 0, vox = 0;
    for (long q = (long)blockIdx.x * MB_THREADS + threadIdx.x; q < n; q += (long)gridDim.x * MB_THREADS) {         // grid-stride: ends
        const unsigned long long a = sizes[q];
        const bool largest = (int)q + 1 == b;
        const bool on = select == 2 ? largest : (!largest && (select == 0 || (double)a < limit));
        flag[q] = on ? 1 : 0;
        if (on) { comps++; vox += a; }
    }
    for (int d = 32; d >= 1; d >>= 1) { comps += __shfl_xor(comps, d); vox += __shfl_xor(vox, d); }               // whole waves arrive here
    if ((threadIdx.x & 63) == 0 && comps) { atomicAdd(acc + 1, comps); atomicAdd(acc + 2, vox); }
    if (blockIdx.x == 0 && threadIdx.x == 0) acc[0] = big;
}

// out = in with the voxels of the flagged labels set to fill
__global__ __launch_bounds__(MB_THREADS) void paint_write(const uint8_t *__restrict__ in, const int *__restrict__ labels, const uint8_t *__restrict__ flag,
                                                          uint8_t *__restrict__ out, int fill, long nVox)
{
    for (long v = (long)blockIdx.x * MB_THREADS + threadIdx.x; v < nVox; v += (long)gridDim.x * MB_THREADS) {      // grid-stride: ends
        const int lab = labels[v];
        out[v] = (lab > 0 && flag[lab - 1]) ? (uint8_t)fill : in[v];
    }
}

// ---------------------------------------------------------------- the labelling, shared ----------------------------------------------------------------

// Steps 1-5a for bfd_label3d and bfd_paint_components3d: reserve() before the host-to-device copies, run() after them. run() leaves the labels in L,
// their number in nl, the voxel counts in dsz (wantSizes and nl > 0) and the milliseconds of its two timed sections in ms; its events are ev's.
struct Labelling {
    DevTemp<int> L, rank;
    InclusiveSum<int> sum;
    DevTemp<unsigned long long> dsz;
    int nl = 0;
    float ms = 0.f;

    int reserve(const char *who, size_t n)
    {
        BFD_STEP(L.alloc(n));
        BFD_STEP(rank.alloc(n));
        BFD_STEP(sum.reserve(rank, n));
        return 0;
    }

    // vol: the volume on the device; value < 0: the foreground is vol != 0
    int run(const char *who, const uint8_t *vol, int value, const label_dims &g, size_t n, bool wantSizes, Events &ev)
    {
        const long nv = (long)n;
        float ms1 = 0.f, ms2 = 0.f;
        BFD_STEP(ev.record(0));
        const unsigned vb = blocks_for(nv, MB_THREADS, MAX_BLOCKS);
        hipLaunchKernelGGL(label_local, dim3(blocks_for(g.nTiles, 1, MAX_BLOCKS)), dim3(MB_THREADS), 0, 0, vol, L.p, g, value);
        hipLaunchKernelGGL(label_merge, dim3(vb), dim3(MB_THREADS), 0, 0, L.p, g, nv);
        hipLaunchKernelGGL(label_flatten, dim3(vb), dim3(MB_THREADS), 0, 0, L.p, rank.p, nv);
        BFD_STEP(hipGetLastError());
        BFD_STEP(sum.run(rank, n));
        hipLaunchKernelGGL(label_assign, dim3(vb), dim3(MB_THREADS), 0, 0, L.p, rank.p, nv);
        BFD_STEP(hipGetLastError());
        BFD_STEP(ev.record(1));
        BFD_STEP(ev.sync(1));
        BFD_STEP(ev.elapsed(&ms1, 0, 1));
        // the number of components sizes the histogram: the one value the host needs between the kernels
        BFD_STEP(hipMemcpy(&nl, rank.p + (n - 1), sizeof(int), hipMemcpyDeviceToHost));
        if (wantSizes && nl > 0) {
            BFD_STEP(dsz.alloc((size_t)nl));
            BFD_STEP(hipMemset(dsz, 0, (size_t)nl * sizeof(unsigned long long)));
            BFD_STEP(ev.record(0));
            hipLaunchKernelGGL(label_sizes, dim3(vb), dim3(MB_THREADS), 0, 0, L.p, dsz.p, nv);
            BFD_STEP(hipGetLastError());
            BFD_STEP(ev.record(1));
            BFD_STEP(ev.sync(1));
            BFD_STEP(ev.elapsed(&ms2, 0, 1));
        }
        ms = ms1 + ms2;
        return 0;
    }
};

static label_dims make_label_dims(int64_t N1, int64_t N2, int64_t N3, int connectivity)
{
    label_dims g;
    g.N1 = (int)N1; g.N2 = (int)N2; g.N3 = (int)N3; g.conn = connectivity;
    g.nTj = (int)((N2 + LT_J - 1) / LT_J); g.nTk = (int)((N3 + LT_K - 1) / LT_K);
    g.nTiles = (long)g.nTk * g.nTj * ((N1 + LT_I - 1) / LT_I);
    return g;
}

}  // namespace

hipError_t bfd_stage_box_morphology(uint64_t *a, uint64_t *b, int N1, int N2, int N3, const int *s, int dilate, int borderValue, uint64_t **result)
{
    const morph_dims g = morph_make_dims(N1, N2, N3);
    const long nWords = (long)N1 * N2 * g.nW;
    const unsigned wb = blocks_for(nWords, MB_THREADS, MAX_BLOCKS);
    const uint64_t fill = borderValue ? ~(uint64_t)0 : 0;
    uint64_t *src = a, *dst = b;
    for (int axis = 2; axis >= 0; axis--) {
        if (s[axis] == 1) continue;
        int lo, hi;
        morph_box_taps(s[axis], dilate != 0, &lo, &hi);
        hipLaunchKernelGGL(morph_box_pass, dim3(wb), dim3(MB_THREADS), 0, 0, src, dst, g, nWords, axis, lo, hi, dilate, fill);
        std::swap(src, dst);
    }
    *result = src;
    return hipGetLastError();
}

extern "C" int bfd_binary_morphology3d(int device, int op, const uint8_t *in, uint8_t *out, int64_t N1, int64_t N2, int64_t N3,
                                       const uint8_t *structure, int s1, int s2, int s3, int iterations, int borderValue, float *kernelMs)
{
    static const char *who = "bfd_binary_morphology3d";
    // every argument error is reported before a device is looked for
    if (op < 0 || op > 3) BFD_FAIL(-1, std::string(who) + ": op must be 0 (erosion), 1 (dilation), 2 (closing) or 3 (opening)");
    if (!in || !out) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (N1 < 0 || N2 < 0 || N3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (!volume_fits(N1, N2, N3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    if (iterations < 1) BFD_FAIL(-1, std::string(who) + ": iterations must be at least 1");
    if (borderValue != 0 && borderValue != 1) BFD_FAIL(-1, std::string(who) + ": borderValue must be 0 or 1");
    if (op >= 2 && borderValue != 0) BFD_FAIL(-1, std::string(who) + ": borderValue is 0 for closing and opening");
    const size_t n = (size_t)(N1 * N2 * N3);
    if (overlap(in, n, out, n) && n) BFD_FAIL(-1, std::string(who) + ": out may not alias in");
    static const uint8_t cross[27] = {0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0};
    if (!structure) { structure = cross; s1 = s2 = s3 = 3; }
    if (s1 < 1 || s2 < 1 || s3 < 1) BFD_FAIL(-1, std::string(who) + ": every structure size must be at least 1");
    bool box = true;
    long nTrue = 0;
    for (long q = 0; q < (long)s1 * s2 * s3; q++) { if (structure[q]) nTrue++; else box = false; }
    if (box && (s1 > MAX_BOX || s2 > MAX_BOX || s3 > MAX_BOX))
        BFD_FAIL(-1, std::string(who) + ": an all-ones structure may have at most 31 elements per axis");
    if (!box && (s1 > MORPH_GEN_MAX || s2 > MORPH_GEN_MAX || s3 > MORPH_GEN_MAX))
        BFD_FAIL(-1, std::string(who) + ": a structure that is not all ones may have at most 7 elements per axis");
    if (nTrue == 0) BFD_FAIL(-1, std::string(who) + ": the structure has no true element");
    const int s[3] = {s1, s2, s3};
    morph_taps taps[2];                               // [0] erosion, [1] dilation
    if (!box) { morph_make_taps(structure, s1, s2, s3, false, &taps[0]); morph_make_taps(structure, s1, s2, s3, true, &taps[1]); }

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) return 0;

    const morph_dims g = morph_make_dims((int)N1, (int)N2, (int)N3);
    const long nWords = (long)N1 * N2 * g.nW;
    DevTemp<uint8_t> vol;
    DevTemp<uint64_t> bitsA, bitsB;
    Events ev;
    BFD_STEP(vol.alloc(n));
    BFD_STEP(bitsA.alloc((size_t)nWords));
    BFD_STEP(bitsB.alloc((size_t)nWords));
    BFD_STEP(hipMemcpy(vol, in, n, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    BFD_STEP(ev.record(0));
    uint64_t *src = bitsA, *dst = bitsB;
    hipLaunchKernelGGL(morph_pack, dim3(blocks_for(nWords, MB_THREADS / 64, MAX_BLOCKS)), dim3(MB_THREADS), 0, 0, vol.p, src, g, nWords);
    const unsigned wb = blocks_for(nWords, MB_THREADS, MAX_BLOCKS);
    // closing: dilations then erosions; opening: erosions then dilations (scipy: each `iterations` times)
    const int first = (op == 1 || op == 2) ? 1 : 0, stages = op >= 2 ? 2 : 1;
    for (int st = 0; st < stages; st++) {
        const int dilate = st == 0 ? first : 1 - first;
        const uint64_t fill = borderValue ? ~(uint64_t)0 : 0;
        for (int it = 0; it < iterations; it++) {
            if (box) {
                uint64_t *res = src;
                BFD_STEP(bfd_stage_box_morphology(src, dst, (int)N1, (int)N2, (int)N3, s, dilate, borderValue, &res));
                if (res != src) std::swap(src, dst);
            } else {
                hipLaunchKernelGGL(morph_general_pass, dim3(wb), dim3(MB_THREADS), 0, 0, src, dst, g, nWords, taps[dilate], dilate, fill);
                std::swap(src, dst);
            }
        }
    }
    hipLaunchKernelGGL(morph_unpack, dim3(blocks_for((long)n, MB_THREADS, MAX_BLOCKS)), dim3(MB_THREADS), 0, 0, src, vol.p, g, (long)n);
    BFD_STEP(hipGetLastError());
    BFD_STEP(ev.record(1));
    BFD_STEP(ev.sync(1));
    BFD_STEP(ev.elapsed(kernelMs, 0, 1));
    BFD_STEP(hipMemcpy(out, vol, n, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int bfd_label3d(int device, const uint8_t *in, int32_t *labels, int64_t N1, int64_t N2, int64_t N3, int connectivity,
                           int64_t *numLabels, int64_t *sizes, int64_t sizesCapacity, uint8_t *largest, float *kernelMs)
{
    static const char *who = "bfd_label3d";
    if (!in) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (!labels && !numLabels && !sizes && !largest) BFD_FAIL(-1, std::string(who) + ": no output asked for");
    if (N1 < 0 || N2 < 0 || N3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (!volume_fits(N1, N2, N3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    if (connectivity < 1 || connectivity > 3) BFD_FAIL(-1, std::string(who) + ": connectivity must be 1, 2 or 3");
    if (sizesCapacity < 0) BFD_FAIL(-1, std::string(who) + ": negative sizesCapacity");
    const size_t n = (size_t)(N1 * N2 * N3);
    if (n && ((labels && overlap(in, n, labels, 4 * n)) || (largest && overlap(in, n, largest, n)) || (labels && largest && overlap(labels, 4 * n, largest, n))))
        BFD_FAIL(-1, std::string(who) + ": an output may not alias in or another output");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (numLabels) *numLabels = 0;
    if (n == 0) return 0;

    const label_dims g = make_label_dims(N1, N2, N3, connectivity);
    const long nv = (long)n;
    const bool wantSizes = sizes || largest;

    DevTemp<uint8_t> vol;                             // the input; afterwards the mask of the largest component
    DevTemp<int> best;
    Labelling lab;
    Events ev;
    float ms2 = 0.f;
    BFD_STEP(vol.alloc(n));
    if (int rc = lab.reserve(who, n)) return rc;
    BFD_STEP(best.alloc(1));
    BFD_STEP(hipMemcpy(vol, in, n, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    if (int rc = lab.run(who, vol, -1, g, n, wantSizes, ev)) return rc;
    const int nl = lab.nl;
    if (wantSizes && nl > 0) {
        if (largest) {
            BFD_STEP(ev.record(0));
            hipLaunchKernelGGL(label_largest, dim3(1), dim3(1024), 0, 0, lab.dsz.p, nl, best.p);
            hipLaunchKernelGGL(label_select, dim3(blocks_for(nv, MB_THREADS, MAX_BLOCKS)), dim3(MB_THREADS), 0, 0, lab.L.p, best.p, vol.p, nv);
            BFD_STEP(hipGetLastError());
            BFD_STEP(ev.record(1));
            BFD_STEP(ev.sync(1));
            BFD_STEP(ev.elapsed(&ms2, 0, 1));
        }
        if (sizes && sizesCapacity >= nl) BFD_STEP(hipMemcpy(sizes, lab.dsz, (size_t)nl * sizeof(int64_t), hipMemcpyDeviceToHost));
        if (largest) BFD_STEP(hipMemcpy(largest, vol, n, hipMemcpyDeviceToHost));
    } else if (largest) {
        memset(largest, 0, n);                        // no component: an all-zero mask
    }
    if (labels) BFD_STEP(hipMemcpy(labels, lab.L, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (numLabels) *numLabels = nl;
    if (kernelMs) *kernelMs = lab.ms + ms2;
    return 0;
}

extern "C" int bfd_paint_components3d(int device, const uint8_t *in, uint8_t *out, int64_t N1, int64_t N2, int64_t N3, int value, int connectivity,
                                      int select, int fill, int64_t *counts, float *kernelMs)
{
    static const char *who = "bfd_paint_components3d";
    if (!in || !out || !counts) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (N1 < 0 || N2 < 0 || N3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (!volume_fits(N1, N2, N3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    if (value < 0 || value > 255 || fill < 0 || fill > 255) BFD_FAIL(-1, std::string(who) + ": value and fill must be uint8 values (0 .. 255)");
    if (connectivity < 1 || connectivity > 3) BFD_FAIL(-1, std::string(who) + ": connectivity must be 1, 2 or 3");
    if (select < 0 || select > 2) BFD_FAIL(-1, std::string(who) + ": select must be 0 (all but the largest), 1 (the small ones) or 2 (the largest)");
    const size_t n = (size_t)(N1 * N2 * N3);
    if (n && overlap(in, n, out, n)) BFD_FAIL(-1, std::string(who) + ": out may not alias in");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) { for (int q = 0; q < 4; q++) counts[q] = 0; return 0; }

    const label_dims g = make_label_dims(N1, N2, N3, connectivity);
    const long nv = (long)n;
    DevTemp<uint8_t> vol, dout;
    DevTemp<int> best;
    DevTemp<unsigned long long> acc;
    Labelling lab;
    Events ev;
    float ms2 = 0.f;
    unsigned long long r[3] = {0, 0, 0};
    BFD_STEP(vol.alloc(n));
    if (int rc = lab.reserve(who, n)) return rc;
    BFD_STEP(best.alloc(1));
    BFD_STEP(acc.alloc(3));
    BFD_STEP(hipMemcpy(vol, in, n, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    if (int rc = lab.run(who, vol, value, g, n, true, ev)) return rc;
    const int nl = lab.nl;
    if (nl > 0) {
        // the flags take the place of the root flags in `rank` (nl <= n bytes of 4 n), the result the place of nothing: out is a volume of its own
        uint8_t *flag = (uint8_t *)lab.rank.p;
        BFD_STEP(dout.alloc(n));
        BFD_STEP(hipMemset(acc, 0, 3 * sizeof(unsigned long long)));
        BFD_STEP(ev.record(0));
        hipLaunchKernelGGL(label_largest, dim3(1), dim3(1024), 0, 0, lab.dsz.p, nl, best.p);
        hipLaunchKernelGGL(paint_flags, dim3(blocks_for(nl, MB_THREADS, MAX_BLOCKS)), dim3(MB_THREADS), 0, 0, lab.dsz.p, nl, best.p, select, flag, acc.p);
        hipLaunchKernelGGL(paint_write, dim3(blocks_for(nv, MB_THREADS, MAX_BLOCKS)), dim3(MB_THREADS), 0, 0, vol.p, lab.L.p, flag, dout.p, fill, nv);
        BFD_STEP(hipGetLastError());
        BFD_STEP(ev.record(1));
        BFD_STEP(ev.sync(1));
        BFD_STEP(ev.elapsed(&ms2, 0, 1));
        BFD_STEP(hipMemcpy(r, acc, sizeof r, hipMemcpyDeviceToHost));
        BFD_STEP(hipMemcpy(out, dout, n, hipMemcpyDeviceToHost));
    } else {
        memcpy(out, in, n);                           // no foreground: nothing to paint
    }
    counts[0] = nl; counts[1] = (int64_t)r[0]; counts[2] = (int64_t)r[1]; counts[3] = (int64_t)r[2];
    if (kernelMs) *kernelMs = lab.ms + ms2;
    return 0;
}

extern "C" int bfd_select_component3d(int device, const uint8_t *in, uint8_t *out, int64_t N1, int64_t N2, int64_t N3, int connectivity, int tie,
                                      int64_t *info, float *kernelMs)
{
    static const char *who = "bfd_select_component3d";
    if (!in || !out || !info) BFD_FAIL(-1, std::string(who) + ": null argument");
    if (N1 < 0 || N2 < 0 || N3 < 0) BFD_FAIL(-1, std::string(who) + ": negative dimension");
    if (!volume_fits(N1, N2, N3)) BFD_FAIL(-1, std::string(who) + ": the volume has 2^31 voxels or more (limit: fewer than 2^31)");
    if (connectivity < 1 || connectivity > 3) BFD_FAIL(-1, std::string(who) + ": connectivity must be 1, 2 or 3");
    if (tie != 0 && tie != 1) BFD_FAIL(-1, std::string(who) + ": tie must be 0 (the highest label among equals) or 1 (the lowest)");
    const size_t n = (size_t)(N1 * N2 * N3);
    if (n && overlap(in, n, out, n)) BFD_FAIL(-1, std::string(who) + ": out may not alias in");

    if (int rc = pick_device(who, device)) return rc;
    if (kernelMs) *kernelMs = 0.f;
    if (n == 0) { info[0] = info[1] = 0; return 0; }

    const label_dims g = make_label_dims(N1, N2, N3, connectivity);
    const long nv = (long)n;
    DevTemp<uint8_t> vol;                             // the input; afterwards the mask of the chosen component
    DevTemp<int> best;
    Labelling lab;
    Events ev;
    float ms2 = 0.f;
    int chosen = 0;
    unsigned long long size = 0;
    BFD_STEP(vol.alloc(n));
    if (int rc = lab.reserve(who, n)) return rc;
    BFD_STEP(best.alloc(1));
    BFD_STEP(hipMemcpy(vol, in, n, hipMemcpyHostToDevice));
    BFD_STEP(ev.create());
    if (int rc = lab.run(who, vol, -1, g, n, true, ev)) return rc;
    const int nl = lab.nl;
    if (nl > 0) {
        BFD_STEP(ev.record(0));
        if (tie) hipLaunchKernelGGL(label_largest_lowest, dim3(1), dim3(1024), 0, 0, lab.dsz.p, nl, best.p);
        else hipLaunchKernelGGL(label_largest, dim3(1), dim3(1024), 0, 0, lab.dsz.p, nl, best.p);
        hipLaunchKernelGGL(label_select, dim3(blocks_for(nv, MB_THREADS, MAX_BLOCKS)), dim3(MB_THREADS), 0, 0, lab.L.p, best.p, vol.p, nv);
        BFD_STEP(hipGetLastError());
        BFD_STEP(ev.record(1));
        BFD_STEP(ev.sync(1));
        BFD_STEP(ev.elapsed(&ms2, 0, 1));
        BFD_STEP(hipMemcpy(&chosen, best, sizeof chosen, hipMemcpyDeviceToHost));
        if (chosen < 1 || chosen > nl) BFD_FAIL(-10, std::string(who) + ": the reduction returned a label outside 1 .. components");
        BFD_STEP(hipMemcpy(&size, lab.dsz.p + (chosen - 1), sizeof size, hipMemcpyDeviceToHost));
        BFD_STEP(hipMemcpy(out, vol, n, hipMemcpyDeviceToHost));
    } else {
        memset(out, 0, n);                            // no component: an all-zero mask
    }
    info[0] = nl; info[1] = (int64_t)size;
    if (kernelMs) *kernelMs = lab.ms + ms2;
    return 0;
}
