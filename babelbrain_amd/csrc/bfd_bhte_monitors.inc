// Monitor kernels of bfd_bhte_kernels.hip that are written ONCE over the material id type and compiled twice: bfd_bhte_kernels.hip includes this file inside its
// anonymous namespace with BHTE_ID = unsigned char and again with BHTE_ID = uint16_t, which gives two overloads of each kernel. The other kernels
// of that file get their two overloads from a *_body template; these three do not, because inlined through a body their 8-bit machine code
// came out in another instruction order than before (same instructions), and the 8-bit kernels are held to the code they had.
#ifndef BHTE_ID
#error "include from bfd_bhte_kernels.hip with BHTE_ID defined"
#endif

// Monitor points of the intermediate steps of an S-step pass: T(n + depth) at the listed voxels from T(n), depth 1 .. 3 -- the cube of side
// 2 depth + 1 around the voxel advanced level by level in LDS (one workgroup per point; the caller monitors 1 - 4 points,
// CalculateTemperatureEffects.py:1003-1023). The same cell update as everywhere: equal to the value a one-step run would hold.
template <bool REV>
__global__ __launch_bounds__(64) void cone_points(BM_ARGS(BHTE_ID), const unsigned *__restrict__ idx, float *__restrict__ out, long stride, long col, int depth)
{
    __shared__ float A[2][343];
    const int side = 2 * depth + 1, ncell = side * side * side;
    const unsigned c0 = idx[blockIdx.x];
    const int ci = (int)(c0 % (unsigned)N1), cj = (int)((c0 / (unsigned)N1) % (unsigned)N2), ck = (int)(c0 / ((unsigned)N1 * (unsigned)N2));
    const long pl = (long)N1 * N2;
    for (int v = threadIdx.x; v < ncell; v += 64) {
        const int li = v % side, lj = (v / side) % side, lk = v / (side * side);
        const int i = min(max(ci - depth + li, 0), N1 - 1), j = min(max(cj - depth + lj, 0), N2 - 1), k = min(max(ck - depth + lk, 0), N3 - 1);
        A[0][v] = Tin[(long)k * pl + (long)j * N1 + i];
    }
    __syncthreads();
    for (int lev = 1; lev <= depth; lev++) {
        const float *src = A[(lev - 1) & 1]; float *dst = A[lev & 1];
        for (int v = threadIdx.x; v < ncell; v += 64) {
            const int li = v % side, lj = (v / side) % side, lk = v / (side * side);
            float val = src[v];
            if (li >= lev && li < side - lev && lj >= lev && lj < side - lev && lk >= lev && lk < side - lev) {
                const int i = ci - depth + li, j = cj - depth + lj, k = ck - depth + lk;
                if (i > 0 && i < N1 - 1 && j > 0 && j < N2 - 1 && k > 0 && k < N3 - 1) {       // inside the volume and off its faces: all six neighbours exist
                    const long c = (long)k * pl + (long)j * N1 + i;
                    const int m = mat[c];
                    val = bhte_update<REV>(src[v], src[v - 1], src[v + 1], src[v - side], src[v + side], src[v - side * side], src[v + side * side], cd[m], cp[m], Tcore,
                                           q != nullptr, q ? q[c] : 0.0f);
                }
            }
            dst[v] = val;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(long)blockIdx.x * stride + col] = A[depth & 1][(depth * side + depth) * side + depth];
}

// The monitored plane at a step INSIDE a pass: T(n + depth) on the row j = jsel for a patch of 16 x 16 cells in (i, k), from T(n) -- the slab of
// (16 + 2 depth) x (2 depth + 1) x (16 + 2 depth) cells around the patch advanced level by level in LDS, like cone_points does for a cube. One sample of
// a 320 x 320 plane at depth 3 costs 400 workgroups x 3388 cells: a few per cent of one volume step, once per nFactorMonitoring steps.
template <bool REV>
__global__ __launch_bounds__(256) void cone_slice(BM_ARGS(BHTE_ID), float *__restrict__ out, int jsel, long sample, long nSamples, int depth)
{
    __shared__ float A[2][22 * 7 * 22];
    const int sx = 16 + 2 * depth, sy = 2 * depth + 1, sz = 16 + 2 * depth, ncell = sx * sy * sz;
    const int i0 = blockIdx.x * 16 - depth, j0 = jsel - depth, k0 = blockIdx.y * 16 - depth;
    const long pl = (long)N1 * N2;
    for (int v = threadIdx.x; v < ncell; v += 256) {
        const int li = v % sx, lj = (v / sx) % sy, lk = v / (sx * sy);
        const int i = min(max(i0 + li, 0), N1 - 1), j = min(max(j0 + lj, 0), N2 - 1), k = min(max(k0 + lk, 0), N3 - 1);
        A[0][v] = Tin[(long)k * pl + (long)j * N1 + i];
    }
    __syncthreads();
    for (int lev = 1; lev <= depth; lev++) {
        const float *src = A[(lev - 1) & 1]; float *dst = A[lev & 1];
        for (int v = threadIdx.x; v < ncell; v += 256) {
            const int li = v % sx, lj = (v / sx) % sy, lk = v / (sx * sy);
            float val = src[v];
            if (li >= lev && li < sx - lev && lj >= lev && lj < sy - lev && lk >= lev && lk < sz - lev) {
                const int i = i0 + li, j = j0 + lj, k = k0 + lk;
                if (i > 0 && i < N1 - 1 && j > 0 && j < N2 - 1 && k > 0 && k < N3 - 1) {
                    const long c = (long)k * pl + (long)j * N1 + i;
                    const int m = mat[c];
                    val = bhte_update<REV>(src[v], src[v - 1], src[v + 1], src[v - sx], src[v + sx], src[v - sx * sy], src[v + sx * sy], cd[m], cp[m], Tcore,
                                           q != nullptr, q ? q[c] : 0.0f);
                }
            }
            dst[v] = val;
        }
        __syncthreads();
    }
    const float *res = A[depth & 1];
    const int li = depth + (int)(threadIdx.x & 15), lk = depth + (int)(threadIdx.x >> 4);
    const int i = i0 + li, k = k0 + lk;
    if (i < N1 && k < N3) out[(REV ? (long)k * N1 + i : (long)i * N3 + k) * nSamples + sample] = res[(lk * sy + depth) * sx + li];
}
// A sample of the monitored plane at the FIRST step of a pass: T(n+1) on the row j = jsel, computed from T(n)
template <bool REV>
__global__ void step_slice(BM_ARGS(BHTE_ID), float *__restrict__ out, int jsel, long sample, long nSamples)
{
    const long n = (long)N1 * N3;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long)gridDim.x * blockDim.x) {
        const int i = (int)(v % N1), k = (int)(v / N1);
        out[(REV ? (long)k * N1 + i : (long)i * N3 + k) * nSamples + sample] = bhte_cell<REV>(Tin, q, mat, cd, cp, i, jsel, k, N1, N2, N3, Tcore);
    }
}
