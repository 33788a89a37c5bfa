// diskann_add.hip — the device steps that inserting rows into an existing DiskANN graph adds to the build's
// (DESIGN.md §6.3): every batch row's nearest batch-mates, the pool that joins them to the traversal's list, and the
// finite check of the uploaded rows.  Search, RobustPrune and the back-edge update are the build's own kernels.
//
// vamana_batch_mates — the b × b all-pairs step of one batch (b rows of d floats, contiguous).
//   Gram: G = X_b·X_bᵀ on the fp32 matrix cores (v_mfma_f32_32x32x2_f32), as vamana_prune's Gram stage: K-slices of
//     64 dims through LDS, rows padded to 68 floats, every entry one fma chain over the dimensions in a fixed order.
//     A 256-thread workgroup owns a block of 32 rows and walks the column blocks of 128 rows (one 32 × 32 tile per
//     wave, 16 accumulator registers); b is not bounded.  The norms G_ii come from vamana_batch_norms, which runs the
//     same chain on the diagonal tiles, so equal rows give G_ii = G_jj = G_ij bit for bit and distance exactly 0.
//   d(i, j) = max(0, (G_ii + G_jj) − 2·G_ij), the prune's form; on an IP handle d(i, j) = −G_ij and no norms are read.
//   Selection: the tile's distances go through LDS (over the column slice, which is spent); each wave keeps the
//     sorted top-64 lists (wave_topk.hpp) of 8 of the block's rows in registers across the column blocks and offers
//     them 64 candidates at a time, ordered by (distance, id); the row itself never enters.
//   No floating-point atomics and no dependence on the block schedule: a row's list is one wave's, fed in column
//   order.  Exact whenever every partial sum is representable.
#include "diskann_kernels.hpp"
#include "wave_topk.hpp"

#include <algorithm>
#include <cstdint>

namespace hipann {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kKS = 64;        // dims per K-slice
constexpr int kLD = kKS + 4;   // LDS row stride: rows 16-B aligned, 4 banks of skew
constexpr int kRB = 32;        // rows per workgroup
constexpr int kCB = 128;       // columns per column block (4 waves × 32)
constexpr int kDD = kCB + 4;   // row stride of the distance tile

// rows [r0, r0 + nrows) of xb, dims [k0, k0 + 64), into LDS (zeros past b and past d); nthreads threads take part
__device__ __forceinline__ void stage_slice(float *s, const float *__restrict__ xb, int b, int d, int r0, int nrows,
                                            int k0, int t, int nthreads) {
    for (int f = t; f < nrows * (kKS / 4); f += nthreads) {
        const int row = f >> 4, kk = k0 + 4 * (f & 15);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + row < b && kk < d) v = *reinterpret_cast<const float4 *>(xb + (size_t)(r0 + row) * d + kk);
        *reinterpret_cast<float4 *>(s + row * kLD + 4 * (f & 15)) = v;
    }
}

// acc += A·Bᵀ over one staged K-slice: A, B point at 32 staged rows each.  Lane (l31, h) feeds row / column l31 and
// the MFMA's k index h; acc[r] is row (r & 3) + 8·(r >> 2) + 4·h, column l31.
__device__ __forceinline__ void mfma_slice(const float *A, const float *B, int l31, int h, f32x16 &acc) {
#pragma unroll
    for (int k0 = 0; k0 < kKS; k0 += 32) {
        f32x4 a4[4], b4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a4[u] = *reinterpret_cast<const f32x4 *>(A + l31 * kLD + k0 + 16 * h + 4 * u);
            b4[u] = *reinterpret_cast<const f32x4 *>(B + l31 * kLD + k0 + 16 * h + 4 * u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u][e], b4[u][e], acc, 0, 0, 0);
    }
}

// nrm[i] = G_ii by the chain the mates kernel runs for G_ij: one wave per 32 rows, the diagonal of their own tile
__global__ void __launch_bounds__(64) vamana_batch_norms(const float *__restrict__ xb, int b, int d,
                                                         float *__restrict__ nrm) {
    __shared__ __attribute__((aligned(16))) float s_a[kRB * kLD];
    const int lane = threadIdx.x, l31 = lane & 31, h = lane >> 5;
    const int rb0 = blockIdx.x * kRB;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < d; k0 += kKS) {
        stage_slice(s_a, xb, b, d, rb0, kRB, k0, lane, 64);
        __syncthreads();
        mfma_slice(s_a, s_a, l31, h, acc);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row == l31 && rb0 + row < b) nrm[rb0 + row] = acc[r];
    }
}

// out[i·T + j] = row0 + (the j-th nearest other row of batch row i), UINT32_MAX past min(T, b − 1); 1 ≤ T ≤ 64.
// IP: a row's mates are ordered by (−G_ij, id); no norms are read.
template <bool IP>
__global__ void __launch_bounds__(256) vamana_batch_mates(const float *__restrict__ xb, int b, int d,
                                                          const float *__restrict__ nrm, uint32_t row0, int T,
                                                          uint32_t *__restrict__ out, unsigned long long *written) {
    __shared__ __attribute__((aligned(16))) float s_a[kRB * kLD];
    __shared__ __attribute__((aligned(16))) float s_b[kCB * kLD];  // the column slice, then the distance tile
    static_assert(kRB * kDD <= kCB * kLD, "the distance tile takes over the column slice");
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int rb0 = blockIdx.x * kRB;
    WaveList<1, int> top[8];  // rows rb0 + 8·wave + 0..7
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) top[rr].init();
    float ni[16];  // the norms of this lane's 16 accumulator rows
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gi = rb0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        ni[r] = !IP && gi < b ? nrm[gi] : 0.f;
    }
    for (int cb0 = 0; cb0 < b; cb0 += kCB) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k0 = 0; k0 < d; k0 += kKS) {
            stage_slice(s_a, xb, b, d, rb0, kRB, k0, t, 256);
            stage_slice(s_b, xb, b, d, cb0, kCB, k0, t, 256);
            __syncthreads();
            mfma_slice(s_a, s_b + 32 * wave * kLD, l31, h, acc);
            __syncthreads();
        }
        // the tile's distances; the row itself and cells past b never compete
        const int gj = cb0 + 32 * wave + l31;
        const float nj = !IP && gj < b ? nrm[gj] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int gi = rb0 + row;
            float dj;
            if constexpr (IP) {
                dj = -acc[r];
            } else {
                dj = (ni[r] + nj) - 2.f * acc[r];
                dj = dj < 0.f ? 0.f : dj;
            }
            s_b[row * kDD + 32 * wave + l31] = (gi < b && gj < b && gi != gj) ? dj : __builtin_inff();
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            const int row = 8 * wave + rr;
            if (rb0 + row >= b) continue;  // (wave-uniform)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int col = 64 * hf + lane;
                const float cd = s_b[row * kDD + col];
                const bool live = cb0 + col < b && cb0 + col != rb0 + row;
                top[rr].offer(live ? cd : __builtin_inff(), live ? cb0 + col : IdTraits<int>::pad(), T - 1);
            }
        }
        __syncthreads();
    }
    int nw = 0;
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
        const int gi = rb0 + 8 * wave + rr;
        if (gi >= b) continue;
        const bool have = top[rr].id[0] != IdTraits<int>::pad();
        if (lane < T) out[(size_t)gi * T + lane] = have ? row0 + (uint32_t)top[rr].id[0] : kNone;
        nw += __popcll(__ballot(lane < T && have));
    }
    if (written && lane == 0 && nw) atomicAdd(written, (unsigned long long)nw);
}

// target i's pool = its traversal list (−1 = an empty slot) followed by its mates (mates == nullptr: none)
__global__ void __launch_bounds__(256) vamana_concat_pool(const int64_t *__restrict__ sid, int K,
                                                          const uint32_t *__restrict__ mates, int T, int b,
                                                          uint32_t *__restrict__ pool, int *__restrict__ pbeg,
                                                          int *__restrict__ plen) {
    const int W = K + T;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)b * W) return;
    const int i = (int)(idx / W), j = (int)(idx % W);
    uint32_t v = kNone;
    if (j < K) {
        const int64_t s = sid[(int64_t)i * K + j];
        if (s >= 0) v = (uint32_t)s;
    } else if (mates) {
        v = mates[(int64_t)i * T + (j - K)];
    }
    pool[idx] = v;
    if (j == 0) {
        pbeg[i] = i * W;
        plen[i] = W;
    }
}

// *flag |= 1 when some value is NaN or ±inf (an integer OR: no order shows)
__global__ void __launch_bounds__(256) vamana_check_finite(const float *__restrict__ x, int64_t count, int *flag) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        const float v = x[i];
        bad |= !(v - v == 0.f);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

}  // namespace

// xb: b rows of d floats on the device (16-B aligned, d % 4 == 0); nrm: b floats of scratch; out: b·T words
void launch_vamana_batch_mates(const float *xb, int b, int d, uint32_t row0, int T, int metric, float *nrm,
                               uint32_t *out, unsigned long long *written, hipStream_t st) {
    if (b <= 0) return;
    HIPANN_REQUIRE(d > 0 && d % 4 == 0 && d <= 2048 && T >= 1 && T <= 64, "vamana_batch_mates: unsupported shape");
    const dim3 grid((unsigned)ceil_div(b, kRB));
    HIPANN_REQUIRE(metric == kL2 || metric == kIP, "vamana_batch_mates: unsupported metric");
    if (metric == kIP) {
        hipLaunchKernelGGL(vamana_batch_mates<true>, grid, dim3(256), 0, st, xb, b, d, nrm, row0, T, out, written);
    } else {
        hipLaunchKernelGGL(vamana_batch_norms, grid, dim3(64), 0, st, xb, b, d, nrm);
        hipLaunchKernelGGL(vamana_batch_mates<false>, grid, dim3(256), 0, st, xb, b, d, nrm, row0, T, out, written);
    }
    HIPANN_CHECK(hipGetLastError());
}

void launch_vamana_concat_pool(const int64_t *sid, int K, const uint32_t *mates, int T, int b, uint32_t *pool,
                               int *pbeg, int *plen, hipStream_t st) {
    if (b <= 0) return;
    const int64_t total = (int64_t)b * (K + T);
    HIPANN_REQUIRE(total < (int64_t)0x7fffffff, "vamana_concat_pool: batch too large");
    hipLaunchKernelGGL(vamana_concat_pool, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, st, sid, K, mates, T, b,
                       pool, pbeg, plen);
    HIPANN_CHECK(hipGetLastError());
}

void launch_vamana_check_finite(const float *x, int64_t count, int *flag, hipStream_t st) {
    if (count <= 0) return;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(count, 256), 4096);
    hipLaunchKernelGGL(vamana_check_finite, dim3(grid), dim3(256), 0, st, x, count, flag);
    HIPANN_CHECK(hipGetLastError());
}

}  // namespace hipann
