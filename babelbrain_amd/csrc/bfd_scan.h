// In-place inclusive prefix sum of int or int64_t on the null stream (rocPRIM), for the Step-1 entries that rank or place by one: bfd_label3d,
// bfd_voxelize_mesh, bfd_voxel_points. In a file of its own so that bfd_median.hip and bfd_resample.hip do not compile rocPRIM. Host code only.
#pragma once
#include "bfd_internal.h"
#include <rocprim/device/device_scan.hpp>

template <typename T>
struct InclusiveSum {
    DevTemp<char> work;
    size_t bytes = 0;
    // sizes and allocates the scratch of a sum over d[0 .. n): launches nothing, and belongs before the timed section
    hipError_t reserve(T *d, size_t n)
    {
        const hipError_t e = rocprim::inclusive_scan((void *)nullptr, bytes, d, d, n, rocprim::plus<T>(), (hipStream_t)0);
        return e == hipSuccess ? work.alloc(std::max<size_t>(bytes, 1)) : e;
    }
    // the sum itself, queued; d and n as reserved
    hipError_t run(T *d, size_t n) { return rocprim::inclusive_scan((void *)work.p, bytes, d, d, n, rocprim::plus<T>(), (hipStream_t)0); }
};
