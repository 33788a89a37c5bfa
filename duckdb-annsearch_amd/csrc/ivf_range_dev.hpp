// ivf_range_dev.hpp — the slot geometry shared by the IVF range kernels (ivf_range.hip, ivf_sq8_range.hip).
#pragma once
#include "common.hpp"

namespace hipann {

constexpr int RV_CH = 2048;     // rows per chunk (ivf_chunk_rows) = 64 passes = 64 mask words per slot
constexpr int RV_WORDS = RV_CH / 32;

// The (pair, chunk) slot of a per-slot block or wave: pair = idx / max_nch, chunk = idx % max_nch; false when the pair
// probes nothing on this shard or the chunk lies past its list's end.
__device__ __forceinline__ bool rv_slot(int64_t idx, int max_nch, int64_t npairs, const int64_t *__restrict__ probes,
                                        const int64_t *__restrict__ list_off, const int *__restrict__ list_len, int nlist,
                                        const int *__restrict__ slot_off, int64_t &pair, int &slot, int64_t &r0,
                                        int64_t &r1) {
    pair = idx / max_nch;
    const int chunk = (int)(idx - pair * max_nch);
    if (pair >= npairs) return false;
    const int64_t l = probes[pair];
    if (l < 0 || l >= nlist) return false;
    const int64_t len = list_len[l];
    if ((int64_t)chunk * RV_CH >= len) return false;
    slot = slot_off[pair] + chunk;
    r0 = list_off[l] + (int64_t)chunk * RV_CH;
    r1 = list_off[l] + len;
    if (r1 > r0 + RV_CH) r1 = r0 + RV_CH;
    return true;
}

}  // namespace hipann
