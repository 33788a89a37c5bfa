// diskann_kernels.hpp — (internal) the one declaration of every launcher of diskann_bfs.hip, diskann_build.hip,
// diskann_add.hip, diskann_remove.hip and diskann_sq8.hip, and the items those files, diskann.hip and
// diskann_host_bfs.cpp share.  Every one of them includes it, so a definition that disagrees with its callers does not
// compile.
#pragma once
#include "common.hpp"

namespace hipann {

constexpr uint32_t kNone = 0xffffffffu;  // the empty adjacency slot / no id
// what the id-gather kernels (diskann.hip) write for a candidate the query had already visited, and the host BFS
// (diskann_host_bfs.cpp) drops: a NaN payload no distance arithmetic produces
constexpr unsigned kVisitedBits = 0x7fc0deadu;

// wave64 butterfly sum, strides 32 … 1 in this order: the summation order is part of every exact-reference contract
__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// IP distances (−dot) take both signs, so their raw bits do not order like the floats.  ip_key_bits: −0.0 counts as
// +0.0, then all bits of a negative flip and the sign bit of a non-negative is set — an unsigned that orders like the
// float, for the high word of a (distance, id) key; ip_key_dist is its inverse.
__device__ __forceinline__ uint32_t ip_key_bits(float v) {
    const uint32_t u = __float_as_uint(v == 0.f ? 0.f : v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ip_key_dist(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}

// ---- diskann_bfs.hip ----
bool diskann_bfs_supported(int d, int fmt, int R, int n_ep, int L, uint32_t N);
void launch_diskann_dup_rows(const uint32_t *adj, int R, int64_t n, uint32_t *dupw, hipStream_t st);
void launch_diskann_bfs(const float *Q, int nq, int d, int fmt, const void *data, const float2 *ab,
                        const uint32_t *adj, const uint32_t *dupw, int R, uint32_t N, const uint32_t *eps, int n_ep, int k, int L,
                        int metric, uint32_t *visited, int64_t vwords, int64_t *out_ids, float *out_d, int *flags,
                        unsigned long long *stats, hipStream_t st);

// ---- diskann_build.hip ----
// One vamana_prune launch (the kernel takes the struct by value).  A call site names the fields it sets.
struct PruneArgs {
    const float *x = nullptr;
    int d = 0;
    uint32_t n = 0;
    const uint32_t *targets = nullptr;
    const int *m_ptr = nullptr;  // the target count on the device (nullptr: m)
    int m = 0;                   // the target count, or its upper bound when m_ptr holds the count
    const uint32_t *pool32 = nullptr;  // pool ids, or ...
    const int64_t *pool64 = nullptr;   // ... the traversal's labels (−1 = empty)
    const float *pool_d = nullptr;     // distances to the target (nullptr: computed here)
    const int *pool_beg = nullptr, *pool_len = nullptr;  // per target (nullptr: target t owns [t·pool_cap, (t+1)·pool_cap))
    int pool_cap = 0;
    int R = 0;
    float alpha = 0.f;
    int metric = kL2;  // kL2: the triangle-inequality rule of DESIGN §6; kIP: the occluding rule of §6.5
    uint32_t *out = nullptr;
    int out_by_target = 0;  // rows of `out` indexed by the target's id (the adjacency) instead of its position
    float *gram = nullptr;  // gridDim.x × 256² floats
    unsigned long long *counters = nullptr;  // [0] += targets, [1] += pools truncated to 256 (nullptr: none)
};
int vamana_prune_blocks(int64_t m);
size_t vamana_gram_bytes(int blocks);
void launch_vamana_prune(const PruneArgs &a, int blocks, hipStream_t st);
void launch_vamana_fill_targets(uint32_t *tg, int b, uint32_t o0, uint32_t ep, hipStream_t st);
void launch_vamana_backedges(uint32_t *adj, int R, const uint32_t *tg, int b, int *cnt, int *slot, uint32_t *touched,
                             int *off, int *fill, uint32_t *src, int *ctr, uint32_t *pool, uint32_t *ptgt, int *pbeg,
                             int *plen, hipStream_t st);

// ---- diskann_add.hip ----
void launch_vamana_batch_mates(const float *xb, int b, int d, uint32_t row0, int T, int metric, float *nrm,
                               uint32_t *out, unsigned long long *written, hipStream_t st);
void launch_vamana_concat_pool(const int64_t *sid, int K, const uint32_t *mates, int T, int b, uint32_t *pool,
                               int *pbeg, int *plen, hipStream_t st);
void launch_vamana_check_finite(const float *x, int64_t count, int *flag, hipStream_t st);

// ---- diskann_remove.hip ----
int64_t diskann_remove_scan_blocks(int64_t n);
void launch_diskann_remove_mark(const int64_t *labels, int64_t m, int64_t n, uint32_t *bits, uint32_t *wpre,
                                uint32_t *sums, hipStream_t st);
void launch_diskann_remove_sources(const uint32_t *bits, const uint32_t *wpre, int64_t n, int64_t *src, hipStream_t st);
void launch_diskann_remove_pool_len(const uint32_t *adj, int R, int64_t n, const uint32_t *bits, uint8_t *nrem,
                                    hipStream_t st);
void launch_diskann_remove_pool_fill(const uint32_t *adj, int R, int64_t n, const uint32_t *bits,
                                     const uint32_t *targets, const int *pbeg, const int *plen, int cnt, uint32_t *pool,
                                     unsigned long long *gathered, hipStream_t st);
void launch_diskann_remove_nearest(const float *x, int d, int64_t n, const uint32_t *bits, uint32_t ep, int metric,
                                   unsigned long long *best, hipStream_t st);
void launch_diskann_remove_compact_adj(const uint32_t *adj, int R, int64_t n, const uint32_t *bits,
                                       const uint32_t *wpre, uint32_t *out, hipStream_t st);

// ---- diskann_sq8.hip ----
// The column statistics split the rows into slabs of this many rows, one block each: a function of n alone, so the
// order of every fp64 addition is fixed.
constexpr int kSq8SlabRows = 512;
int64_t sq8_stat_slabs(int64_t n);
int medoid_nearest_blocks(int64_t n);
void launch_sq8_col_stats(const float *x, int64_t n, int d, bool minmax, bool sum, float *pmin, float *pmax,
                          double *psum, float *ms, double *mean, hipStream_t st);
void launch_sq8_encode(const float *x, int64_t n, int d, const float *ms, uint8_t *out, hipStream_t st);
void launch_medoid_nearest(const float *x, int64_t n, int d, const double *mean, double *bd, uint32_t *bi,
                           uint32_t *out, hipStream_t st);

}  // namespace hipann
