// seed_sort.hip -- K7's plumbing: rocPRIM's device radix sort and scan behind four plain functions (seed_device.h).  A translation unit of
// its own: rocPRIM's templates are megabytes of object code and minutes of nothing for the other kernels, none of which sees them.
// The sort is stable, which is what turns a sort on the key bits alone into (key, position) order: the sketch writes in position order.
#include <cstring>
#include <rocprim/rocprim.hpp>
#include "seed_device.h"

namespace clh {

size_t seed_sort_temp_bytes(int64_t n)
{
    size_t bytes = 0;
    if (n <= 0) return 256;
    if (rocprim::radix_sort_pairs(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)n, 0u, 64u) != hipSuccess)
        return 0;
    return bytes + 256;
}

hipError_t seed_sort_pairs(void* temp, size_t temp_bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint64_t* vals_in, uint64_t* vals_out, int64_t n, int bits,
                           hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (bits < 1) bits = 1;
    if (bits > 64) bits = 64;
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, (unsigned)bits, stream);
}

size_t seed_scan_temp_bytes(int64_t n)
{
    size_t bytes = 0;
    if (n <= 0) return 256;
    if (rocprim::exclusive_scan(nullptr, bytes, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)n, rocprim::plus<int64_t>()) != hipSuccess) return 0;
    return bytes + 256;
}

hipError_t seed_scan_counts(void* temp, size_t temp_bytes, const int32_t* counts, int64_t* out, int64_t n, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    return rocprim::exclusive_scan(temp, temp_bytes, counts, out, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), stream);
}

}  // namespace clh
