// Terms sorted by destination row, behind sage_embed_grad.hip and sage_csr_mean_backward_rows.hip: int32 (key, value) pairs with keys in
// [0, rows] (rows = the sentinel of an unused slot), a STABLE hipcub radix sort on the key bits that matter, so the order the terms
// were laid out in survives inside a run of equal keys, and a row pointer over the sorted keys.  The sort's temporary is reserved by
// host arithmetic (a workspace size query must answer without a device) and checked against the library before the sort.
#pragma once
#include <hipcub/hipcub.hpp>

#include "sage_csr_common.h"

namespace {

// Bits that tell the keys 0 .. rows apart.
inline int sort_key_bits(int64_t rows) {
    int bits = 1;
    while ((1ll << bits) <= rows) ++bits;
    return bits;
}

// Bytes reserved for the temporary of a sort of `slots` pairs (see sort_ws in sage_embed_grad.hip for what the bound covers).
inline size_t sort_temp_reserve(int64_t slots) { return (size_t)slots * 16 + 65536; }

inline hipError_t sort_temp_bytes(int slots, int bits, size_t* bytes) {
    *bytes = 0;
    return hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, (const int32_t*)nullptr, (int32_t*)nullptr, (const int32_t*)nullptr,
                                              (int32_t*)nullptr, slots, 0, bits, (hipStream_t)0);
}

// rowptr[e] = the first position of the sorted list whose key is >= e, e in [0, rows]: rowptr[rows] = the terms
__global__ __launch_bounds__(256) void sorted_rowptr_kernel(const int32_t* __restrict__ keys, int slots, int rows,
                                                            int64_t* __restrict__ rowptr) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e > rows) return;
    int lo = 0, hi = slots;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (keys[mid] < e) lo = mid + 1;
        else hi = mid;
    }
    rowptr[e] = lo;
}

}  // namespace
