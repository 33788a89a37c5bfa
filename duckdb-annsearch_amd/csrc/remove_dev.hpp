// remove_dev.hpp — device helpers shared by the per-list removal kernels (ivf_remove_rows in remove_kernels.hip,
// ivf_sq_remove_rows in ivf_sq8_remove.hip).
#pragma once
#include "common.hpp"

namespace hipann {

// exclusive position of a set flag among the block's flags (thread order) and their count; wsum: one int per wave
__device__ __forceinline__ int block_flag_scan(bool f, int *wsum, int *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const unsigned long long b = __ballot(f);
    const int pre = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(b);
    __syncthreads();
    int add = 0, tot = 0;
    for (int i = 0; i < nw; ++i) {
        const int c = wsum[i];
        if (i < w) add += c;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return pre + add;
}

// id is one of labels[0..m) (sorted, unique)
__device__ __forceinline__ bool label_member(const int64_t *__restrict__ labels, int64_t m, int64_t id) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (labels[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < m && labels[lo] == id;
}

}  // namespace hipann
