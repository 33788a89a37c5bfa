// rerank_rows.hpp — the direct-form distance of the exact forms' rerank, shared by every kernel that returns it
// (ivf_rerank_topk and the Flat candidate rerank in ivf_kernels.hip, the range scan's recheck in flat_range.hip): a
// row that two of them return carries the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace hipann {

// Direct-form sums of 4 rows against one query, lane-strided over the dims (e = lane, lane + 64, ...):
// the loads of 4 strides are issued before their fmas (3 memory round trips at d = 768 instead of 12);
// every accumulator still adds its terms in e order, so the sums are the one-stride loop's bit for bit.
// The caller finishes each row with the xor-butterfly (offsets 32, 16, ..., 1) over the wave.
template <bool IP>
__device__ __forceinline__ void rerank_rows4(const float *__restrict__ qp, const float *const (&xr)[4], int d, int lane,
                                             float (&acc)[4]) {
    int e = lane;
    for (; e + 192 < d; e += 256) {
        float qv[4], xv[4][4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            qv[s] = qp[e + 64 * s];
#pragma unroll
            for (int u = 0; u < 4; ++u) xv[s][u] = xr[u][e + 64 * s];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (IP) acc[u] = fmaf(qv[s], xv[s][u], acc[u]);
                else {
                    const float t = qv[s] - xv[s][u];
                    acc[u] = fmaf(t, t, acc[u]);
                }
            }
    }
    for (; e < d; e += 64) {
        const float qv = qp[e];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float xv = xr[u][e];
            if (IP) acc[u] = fmaf(qv, xv, acc[u]);
            else {
                const float t = qv - xv;
                acc[u] = fmaf(t, t, acc[u]);
            }
        }
    }
}

}  // namespace hipann
