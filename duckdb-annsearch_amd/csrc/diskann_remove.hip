// diskann_remove.hip — removing rows from a DiskANN graph in place on gfx950 (diskann_hip_remove_ids):
// FreshDiskANN's delete consolidation.  Everything here is bandwidth- or gather-bound wave64 HIP; the one expensive
// step, RobustPrune of the repaired rows, is vamana_prune (diskann_build.hip) run unchanged on CSR pools.
//
//   rm_mark          labels → removed-row bitmap (atomicOr on 32-bit words; duplicates and labels outside [0, n) drop)
//   rm_word_sums / rm_scan_sums / rm_word_prefix
//                    exclusive prefix popcount over the bitmap words (block sums, one block scanning them with a
//                    carry, the per-block scan again): removed_before(id) = wpre[id / 32] + popc(low bits of its word)
//   rm_live_sources  src[new id] = old id of every surviving row (the index list of the fp32 row gather)
//   rm_pool_len      one wave per row, lane = adjacency slot: the number of removed ids among the row's stored ids
//                    (0: the row is dead or keeps its ids).  A row with c > 0 of them owns a pool of R·(1 + c) slots
//   rm_pool_fill     one wave per affected row: its live neighbours, then one coalesced read of each removed
//                    neighbour's row; removed ids, ids ≥ n and padding are written as UINT32_MAX, which the prune drops
//   rm_nearest_live  the live row nearest a removed entry point by (Σ(a−b)², id): the prune's direct distance (per-lane
//                    fma chain over float4 chunks lane, lane + 64, …, butterfly sum) and a 64-bit atomicMin on
//                    dist bits << 32 | id (the distance is non-negative, so its bit order is the float order); on an
//                    IP handle the distance is −dot and the key holds its order-preserving bits (ip_key_bits)
//   rm_compact_adj   one wave per surviving row: the repaired row written at its new position, every id replaced by
//                    its rank; slots past the first UINT32_MAX become UINT32_MAX
// No floating-point atomics: every result is the same from run to run.
#include "diskann_kernels.hpp"

#include <algorithm>
#include <cstdint>

namespace hipann {
namespace {

constexpr int kScanThreads = 256;
constexpr int kScanPer = 4;                          // bitmap words per thread of the prefix kernels
constexpr int kScanWords = kScanThreads * kScanPer;  // words per block

__device__ __forceinline__ bool removed(const uint32_t *__restrict__ bits, uint32_t id) {
    return (bits[id >> 5] >> (id & 31)) & 1u;
}

__device__ __forceinline__ uint32_t removed_before(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ wpre,
                                                   uint32_t id) {
    return wpre[id >> 5] + (uint32_t)__popc(bits[id >> 5] & ((1u << (id & 31)) - 1u));
}

__global__ void __launch_bounds__(256) rm_mark(const int64_t *__restrict__ labels, int64_t m, int64_t n, uint32_t *bits) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int64_t l = labels[i];
    if (l >= 0 && l < n) atomicOr(bits + (l >> 5), 1u << (l & 31));
}

__global__ void __launch_bounds__(kScanThreads) rm_word_sums(const uint32_t *__restrict__ bits, int64_t words,
                                                             uint32_t *__restrict__ sums) {
    __shared__ int wsum[kScanThreads / 64];
    const int64_t w0 = (int64_t)blockIdx.x * kScanWords + (int64_t)threadIdx.x * kScanPer;
    int c = 0;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j)
        if (w0 + j < words) c += __popc(bits[w0 + j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int i = 0; i < kScanThreads / 64; ++i) t += wsum[i];
        sums[blockIdx.x] = (uint32_t)t;
    }
}

// one block: sums[b] → exclusive prefix (in place), chunk by chunk with a running carry
__global__ void __launch_bounds__(kScanThreads) rm_scan_sums(uint32_t *__restrict__ sums, int64_t nb) {
    __shared__ uint32_t sh[kScanThreads];
    uint32_t carry = 0;
    for (int64_t c0 = 0; c0 < nb; c0 += kScanThreads) {
        const int64_t i = c0 + threadIdx.x;
        const uint32_t v = i < nb ? sums[i] : 0u;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < kScanThreads; o <<= 1) {  // Hillis-Steele inclusive scan
            const uint32_t a = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0u;
            __syncthreads();
            sh[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < nb) sums[i] = carry + sh[threadIdx.x] - v;
        carry += sh[kScanThreads - 1];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kScanThreads) rm_word_prefix(const uint32_t *__restrict__ bits, int64_t words,
                                                               const uint32_t *__restrict__ offs,
                                                               uint32_t *__restrict__ wpre) {
    __shared__ int wsum[kScanThreads / 64];
    const int64_t w0 = (int64_t)blockIdx.x * kScanWords + (int64_t)threadIdx.x * kScanPer;
    int k[kScanPer], c = 0;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
        k[j] = w0 + j < words ? __popc(bits[w0 + j]) : 0;
        c += k[j];
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int add = 0;
    for (int i = 0; i < w; ++i) add += wsum[i];
    uint32_t pos = offs[blockIdx.x] + (uint32_t)(add + inc - c);
#pragma unroll
    for (int j = 0; j < kScanPer; ++j)
        if (w0 + j < words) {
            wpre[w0 + j] = pos;
            pos += (uint32_t)k[j];
        }
}

__global__ void __launch_bounds__(256) rm_live_sources(const uint32_t *__restrict__ bits,
                                                       const uint32_t *__restrict__ wpre, int64_t n,
                                                       int64_t *__restrict__ src) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n || removed(bits, (uint32_t)r)) return;
    src[r - removed_before(bits, wpre, (uint32_t)r)] = r;
}

// a stored row: lane's id (kNone at and past the first kNone, and in lanes ≥ R)
__device__ __forceinline__ uint32_t load_row(const uint32_t *__restrict__ adj, int R, uint32_t row, int lane) {
    const uint32_t v = lane < R ? adj[(size_t)row * R + lane] : kNone;
    const unsigned long long sent = __ballot(v == kNone);
    const int deg = sent ? __ffsll(sent) - 1 : 64;
    return lane < deg ? v : kNone;
}

__global__ void __launch_bounds__(256) rm_pool_len(const uint32_t *__restrict__ adj, int R, int64_t n,
                                                   const uint32_t *__restrict__ bits, uint8_t *__restrict__ nrem) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;  // (wave-uniform)
    const uint32_t v = load_row(adj, R, (uint32_t)row, lane);
    const unsigned long long dead = __ballot(v < (uint64_t)n && removed(bits, v));
    if (lane == 0) nrem[row] = removed(bits, (uint32_t)row) ? (uint8_t)0 : (uint8_t)__popcll(dead);
}

// gathered: += the live ids written (integer; the order of arrival never shows)
__global__ void __launch_bounds__(256) rm_pool_fill(const uint32_t *__restrict__ adj, int R, int64_t n,
                                                    const uint32_t *__restrict__ bits,
                                                    const uint32_t *__restrict__ targets,
                                                    const int *__restrict__ pbeg, const int *__restrict__ plen, int cnt,
                                                    uint32_t *__restrict__ pool, unsigned long long *gathered) {
    const int lane = threadIdx.x & 63;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < cnt; t += gridDim.x * 4) {
        const uint32_t p = targets[t];
        uint32_t *dst = pool + pbeg[t];
        const int cap = plen[t] / R;  // 1 + removed neighbours, as rm_pool_len counted them
        const uint32_t v = load_row(adj, R, p, lane);
        const bool in = v < (uint64_t)n;
        const bool dead = in && removed(bits, v);
        unsigned long long db = __ballot(dead);
        int live = __popcll(__ballot(in && !dead));
        if (lane < R) dst[lane] = in && !dead ? v : kNone;
        int blk = 1;
        while (db && blk < cap) {
            const int s = __ffsll(db) - 1;
            db &= db - 1;
            const uint32_t u = __shfl(v, s);
            const uint32_t w = load_row(adj, R, u, lane);
            const bool ok = w < (uint64_t)n && !removed(bits, w);
            live += __popcll(__ballot(ok));
            if (lane < R) dst[blk * R + lane] = ok ? w : kNone;
            ++blk;
        }
        if (lane == 0) atomicAdd(gathered, (unsigned long long)live);
    }
}

template <bool IP>
__global__ void __launch_bounds__(256) rm_nearest_live(const float *__restrict__ x, int d, int64_t n,
                                                       const uint32_t *__restrict__ bits, uint32_t ep,
                                                       unsigned long long *best) {
    const int lane = threadIdx.x & 63;
    const float4 *xt = reinterpret_cast<const float4 *>(x + (size_t)ep * d);
    unsigned long long mine = ~0ull;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * 4) {
        if (removed(bits, (uint32_t)row)) continue;  // (wave-uniform)
        const float4 *xc = reinterpret_cast<const float4 *>(x + (size_t)row * d);
        float s = 0.f;
        for (int q4 = lane; q4 < (d >> 2); q4 += 64) {
            const float4 p4 = xt[q4], c4 = xc[q4];
            if constexpr (IP) {
                s = fmaf(p4.x, c4.x, s);
                s = fmaf(p4.y, c4.y, s);
                s = fmaf(p4.z, c4.z, s);
                s = fmaf(p4.w, c4.w, s);
            } else {
                float w;
                w = p4.x - c4.x; s = fmaf(w, w, s);
                w = p4.y - c4.y; s = fmaf(w, w, s);
                w = p4.z - c4.z; s = fmaf(w, w, s);
                w = p4.w - c4.w; s = fmaf(w, w, s);
            }
        }
        s = wave_sum(s);
        const uint32_t kb = IP ? ip_key_bits(-s) : __float_as_uint(s);
        const unsigned long long key = ((unsigned long long)kb << 32) | (uint32_t)row;
        mine = key < mine ? key : mine;
    }
    if (lane == 0 && mine != ~0ull) atomicMin(best, mine);
}

__global__ void __launch_bounds__(256) rm_compact_adj(const uint32_t *__restrict__ adj, int R, int64_t n,
                                                      const uint32_t *__restrict__ bits,
                                                      const uint32_t *__restrict__ wpre, uint32_t *__restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n || removed(bits, (uint32_t)row)) return;  // (wave-uniform)
    uint32_t v = load_row(adj, R, (uint32_t)row, lane);
    if (v < (uint64_t)n) v -= removed_before(bits, wpre, v);  // (ids ≥ n stay as they are)
    const size_t nrow = (size_t)row - removed_before(bits, wpre, (uint32_t)row);
    if (lane < R) out[nrow * R + lane] = v;
}

}  // namespace

int64_t diskann_remove_scan_blocks(int64_t n) { return std::max<int64_t>(1, ceil_div(ceil_div(n, 32), kScanWords)); }

// bits: ceil(n / 32) words (zeroed here), wpre: as many, sums: diskann_remove_scan_blocks(n) words.
void launch_diskann_remove_mark(const int64_t *labels, int64_t m, int64_t n, uint32_t *bits, uint32_t *wpre,
                                uint32_t *sums, hipStream_t st) {
    const int64_t words = ceil_div(n, 32), nb = diskann_remove_scan_blocks(n);
    HIPANN_REQUIRE(n > 0 && m > 0 && nb < (int64_t)0x7fffffff && ceil_div(m, 256) < (int64_t)0x7fffffff,
                   "diskann remove: grid too large");
    HIPANN_CHECK(hipMemsetAsync(bits, 0, (size_t)words * 4, st));
    hipLaunchKernelGGL(rm_mark, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, st, labels, m, n, bits);
    hipLaunchKernelGGL(rm_word_sums, dim3((unsigned)nb), dim3(kScanThreads), 0, st, bits, words, sums);
    hipLaunchKernelGGL(rm_scan_sums, dim3(1), dim3(kScanThreads), 0, st, sums, nb);
    hipLaunchKernelGGL(rm_word_prefix, dim3((unsigned)nb), dim3(kScanThreads), 0, st, bits, words, sums, wpre);
    HIPANN_CHECK(hipGetLastError());
}

void launch_diskann_remove_sources(const uint32_t *bits, const uint32_t *wpre, int64_t n, int64_t *src, hipStream_t st) {
    hipLaunchKernelGGL(rm_live_sources, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, bits, wpre, n, src);
    HIPANN_CHECK(hipGetLastError());
}

void launch_diskann_remove_pool_len(const uint32_t *adj, int R, int64_t n, const uint32_t *bits, uint8_t *nrem,
                                    hipStream_t st) {
    HIPANN_REQUIRE(R >= 1 && R <= 64 && ceil_div(n, 4) < (int64_t)0x7fffffff, "diskann remove: bad shape");
    hipLaunchKernelGGL(rm_pool_len, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, st, adj, R, n, bits, nrem);
    HIPANN_CHECK(hipGetLastError());
}

void launch_diskann_remove_pool_fill(const uint32_t *adj, int R, int64_t n, const uint32_t *bits,
                                     const uint32_t *targets, const int *pbeg, const int *plen, int cnt, uint32_t *pool,
                                     unsigned long long *gathered, hipStream_t st) {
    if (cnt <= 0) return;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(cnt, 4), 16384);
    hipLaunchKernelGGL(rm_pool_fill, dim3(grid), dim3(256), 0, st, adj, R, n, bits, targets, pbeg, plen, cnt, pool,
                       gathered);
    HIPANN_CHECK(hipGetLastError());
}

// best: one 64-bit word, all ones on entry; dist bits << 32 | id of the nearest live row on exit (IP: the distance is
// −dot and its bits are ip_key_bits')
void launch_diskann_remove_nearest(const float *x, int d, int64_t n, const uint32_t *bits, uint32_t ep, int metric,
                                   unsigned long long *best, hipStream_t st) {
    HIPANN_REQUIRE(d > 0 && d % 4 == 0, "diskann remove: d must be a multiple of 4");
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n, 4), 2048);
    HIPANN_REQUIRE(metric == kL2 || metric == kIP, "diskann remove: unsupported metric");
    if (metric == kIP) hipLaunchKernelGGL(rm_nearest_live<true>, dim3(grid), dim3(256), 0, st, x, d, n, bits, ep, best);
    else hipLaunchKernelGGL(rm_nearest_live<false>, dim3(grid), dim3(256), 0, st, x, d, n, bits, ep, best);
    HIPANN_CHECK(hipGetLastError());
}

void launch_diskann_remove_compact_adj(const uint32_t *adj, int R, int64_t n, const uint32_t *bits,
                                       const uint32_t *wpre, uint32_t *out, hipStream_t st) {
    hipLaunchKernelGGL(rm_compact_adj, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, st, adj, R, n, bits, wpre, out);
    HIPANN_CHECK(hipGetLastError());
}

}  // namespace hipann
