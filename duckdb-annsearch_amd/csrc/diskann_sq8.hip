// diskann_sq8.hip — streaming kernels over the registered fp32 rows of a DiskANN DB: the per-column
// statistics of the SQ8 codec (Provider::quantize_sq8, rust_lib/src/provider.rs:161-210) and of the medoid, the SQ8
// encode, and the row nearest the mean.  Launchers are declared in diskann_kernels.hpp; host side: diskann_quantize.cpp.
//
// Determinism: no floating-point atomics.  The rows are split into slabs of kSq8SlabRows rows — a function of n alone —
// one block per slab; inside a slab every fp64 sum is one chain per (thread, column) in row order, the chains of a
// column folded in a fixed order, and the slabs folded in slab order.  So two runs give the same bits on any device.
#include "diskann_kernels.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace hipann {

namespace {

constexpr int kStatThreads = 256;

// One pass over a slab of rows: per column min / max (MM) and the fp64 sum (SUM) into the slab's partials.
// A thread owns one group of W columns (W = 4: float4 loads, d % 4 == 0; W = 1: any d).  With G = d / W groups:
//   G >= 256: a thread walks all rows of the slab for groups t, t + 256, ...
//   G <  256: 256 / G threads share a group and take interleaved rows; their results meet in LDS and the thread of
//             interleave 0 folds them in interleave order.
// Each row is read once, coalesced across the block.
template <int W, bool MM, bool SUM>
__global__ void __launch_bounds__(kStatThreads) sq8_col_stats(const float *__restrict__ x, int64_t n, int d,
                                                              float *__restrict__ pmin, float *__restrict__ pmax,
                                                              double *__restrict__ psum) {
    __shared__ float s_mn[MM ? kStatThreads * W : 1], s_mx[MM ? kStatThreads * W : 1];
    __shared__ double s_sm[SUM ? kStatThreads * W : 1];
    const int G = d / W;
    const int64_t r0 = (int64_t)blockIdx.x * kSq8SlabRows;
    const int rows = (int)(n - r0 < kSq8SlabRows ? n - r0 : kSq8SlabRows);
    const float *xs = x + r0 * d;
    const int64_t po = (int64_t)blockIdx.x * d;  // the slab's row of the partials
    const int t = threadIdx.x;
    const int RI = G < kStatThreads ? kStatThreads / G : 1;  // row interleaves per group
    const int ri = G < kStatThreads ? t / G : 0;
    const int g0 = t - ri * G;

    float mn[W], mx[W];
    double sm[W];
    auto reset = [&] {
#pragma unroll
        for (int c = 0; c < W; ++c) { mn[c] = FLT_MAX; mx[c] = -FLT_MAX; sm[c] = 0.0; }
    };
    auto take = [&](const float *v) {
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (MM) {
                if (v[c] < mn[c]) mn[c] = v[c];
                if (v[c] > mx[c]) mx[c] = v[c];
            }
            if (SUM) sm[c] += (double)v[c];
        }
    };
    auto walk = [&](int g, int first, int step) {
        reset();
        const float *col = xs + (int64_t)g * W;
#pragma unroll 4
        for (int r = first; r < rows; r += step) {
            float v[W];
            if constexpr (W == 4) {
                const float4 q = *reinterpret_cast<const float4 *>(col + (int64_t)r * d);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                v[0] = col[(int64_t)r * d];
            }
            take(v);
        }
    };
    auto store = [&](int g) {
        const int64_t o = po + (int64_t)g * W;
        if constexpr (W == 4) {
            if (MM) {
                *reinterpret_cast<float4 *>(pmin + o) = make_float4(mn[0], mn[1], mn[2], mn[3]);
                *reinterpret_cast<float4 *>(pmax + o) = make_float4(mx[0], mx[1], mx[2], mx[3]);
            }
            if (SUM) {
                *reinterpret_cast<double2 *>(psum + o) = make_double2(sm[0], sm[1]);
                *reinterpret_cast<double2 *>(psum + o + 2) = make_double2(sm[2], sm[3]);
            }
        } else {
            if (MM) { pmin[o] = mn[0]; pmax[o] = mx[0]; }
            if (SUM) psum[o] = sm[0];
        }
    };

    if (RI == 1) {  // (uniform over the block)
        for (int g = t; g < G; g += kStatThreads) {
            walk(g, 0, 1);
            store(g);
        }
        return;
    }
    const bool active = ri < RI;  // (256 % G threads are left over)
    if (active) walk(g0, ri, RI);
    else reset();
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (MM) { s_mn[t * W + c] = mn[c]; s_mx[t * W + c] = mx[c]; }
        if (SUM) s_sm[t * W + c] = sm[c];
    }
    __syncthreads();
    if (ri != 0) return;
    for (int k = 1; k < RI; ++k) {  // interleave order
        const int u = (k * G + g0) * W;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (MM) {
                if (s_mn[u + c] < mn[c]) mn[c] = s_mn[u + c];
                if (s_mx[u + c] > mx[c]) mx[c] = s_mx[u + c];
            }
            if (SUM) sm[c] += s_sm[u + c];
        }
    }
    store(g0);
}

// The slabs' partials folded in slab order, one thread per column: ms = min[d] then scale[d] (range > 0 ? range : 1)
// and / or mean[d] = sum / n in fp64.
template <bool MM, bool SUM>
__global__ void __launch_bounds__(256) sq8_fold_stats(const float *__restrict__ pmin, const float *__restrict__ pmax,
                                                      const double *__restrict__ psum, int nslab, int d, int64_t n,
                                                      float *__restrict__ ms, double *__restrict__ mean) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    float mn = FLT_MAX, mx = -FLT_MAX;
    double sm = 0.0;
#pragma unroll 8
    for (int s = 0; s < nslab; ++s) {
        const int64_t o = (int64_t)s * d + j;
        if (MM) {
            const float a = pmin[o], b = pmax[o];
            if (a < mn) mn = a;
            if (b > mx) mx = b;
        }
        if (SUM) sm += psum[o];
    }
    if (MM) {
        const float range = mx - mn;
        ms[j] = mn;
        ms[d + j] = range > 0.f ? range : 1.f;
    }
    if (SUM) mean[j] = sm / (double)n;
}

// the codec's one value: clamp(roundf(((v − min) / scale) · 255), 0, 255), every step rounded to fp32 on its own
__device__ __forceinline__ unsigned sq8_code(float v, float mn, float sc) {
    const float normalized = __fdiv_rn(v - mn, sc);
    float r = roundf(normalized * 255.0f);
    if (r < 0.f) r = 0.f;
    if (r > 255.f) r = 255.f;
    return (unsigned)r;
}
__device__ __forceinline__ unsigned sq8_code4(float4 v, float4 mn, float4 sc) {
    return sq8_code(v.x, mn.x, sc.x) | (sq8_code(v.y, mn.y, sc.y) << 8) | (sq8_code(v.z, mn.z, sc.z) << 16) |
           (sq8_code(v.w, mn.w, sc.w) << 24);
}

// Grid-stride over groups of W consecutive values of the n·d rows (W = 16: d % 16 == 0, four float4 loads and one
// 16-byte store; W = 4: d % 4 == 0, one float4 load and a 4-byte store; W = 1: any d).  A group never straddles a
// row.  ms (min[d], scale[d]) is staged in LDS (LDS) or read through L2.
template <int W, bool LDS>
__global__ void __launch_bounds__(256) sq8_encode(const float *__restrict__ x, int64_t groups, int d,
                                                  const float *__restrict__ ms, uint8_t *__restrict__ out) {
    extern __shared__ __align__(16) float s_ms[];
    if (LDS) {
        for (int i = threadIdx.x; i < 2 * d; i += 256) s_ms[i] = ms[i];
        __syncthreads();
    }
    const float *mn = LDS ? s_ms : ms;
    const float *sc = mn + d;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int64_t e = g * W;
        const int c = (int)(e % d);
        if constexpr (W == 16) {
            const float4 *xv = reinterpret_cast<const float4 *>(x + e);
            const float4 v0 = xv[0], v1 = xv[1], v2 = xv[2], v3 = xv[3];
            const float4 *mv = reinterpret_cast<const float4 *>(mn + c);
            const float4 *sv = reinterpret_cast<const float4 *>(sc + c);
            uint4 o;
            o.x = sq8_code4(v0, mv[0], sv[0]);
            o.y = sq8_code4(v1, mv[1], sv[1]);
            o.z = sq8_code4(v2, mv[2], sv[2]);
            o.w = sq8_code4(v3, mv[3], sv[3]);
            *reinterpret_cast<uint4 *>(out + e) = o;
        } else if constexpr (W == 4) {
            const float4 v = *reinterpret_cast<const float4 *>(x + e);
            *reinterpret_cast<unsigned *>(out + e) = sq8_code4(v, *reinterpret_cast<const float4 *>(mn + c),
                                                               *reinterpret_cast<const float4 *>(sc + c));
        } else {
            out[e] = (uint8_t)sq8_code(x[e], mn[c], sc[c]);
        }
    }
}

// wave64 butterfly sum in fp64, the stride order of wave_sum
__device__ __forceinline__ double wave_sum_f64(double s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

__device__ __forceinline__ bool pair_less(double da, uint32_t ia, double db, uint32_t ib) {
    return da < db || (da == db && ia < ib);
}

// One wave per row, grid-stride: Σ (double(x_j) − mean_j)² as one fp64 chain per lane over the lane's columns
// (V4: float4 groups lane, lane + 64, ...; else columns lane, lane + 64, ...), then the butterfly.  A block leaves its
// smallest (distance, id) in bd / bi[blockIdx.x].  The mean is staged in LDS (LDS) or read through L2.
template <bool V4, bool LDS>
__global__ void __launch_bounds__(256) medoid_nearest(const float *__restrict__ x, int64_t n, int d,
                                                      const double *__restrict__ mean, double *__restrict__ bd,
                                                      uint32_t *__restrict__ bi) {
    extern __shared__ double s_mean[];
    __shared__ double s_d[4];
    __shared__ uint32_t s_i[4];
    if (LDS) {
        for (int i = threadIdx.x; i < d; i += 256) s_mean[i] = mean[i];
        __syncthreads();
    }
    const double *c = LDS ? s_mean : mean;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double best = INFINITY;
    uint32_t besti = kNone;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
        const float *row = x + r * d;
        double s = 0.0;
        if (V4) {
            for (int g = lane; g < d / 4; g += 64) {
                const float4 v = *reinterpret_cast<const float4 *>(row + 4 * g);
                const double t0 = (double)v.x - c[4 * g], t1 = (double)v.y - c[4 * g + 1];
                const double t2 = (double)v.z - c[4 * g + 2], t3 = (double)v.w - c[4 * g + 3];
                s += t0 * t0;
                s += t1 * t1;
                s += t2 * t2;
                s += t3 * t3;
            }
        } else {
            for (int j = lane; j < d; j += 64) {
                const double t = (double)row[j] - c[j];
                s += t * t;
            }
        }
        s = wave_sum_f64(s);
        if (pair_less(s, (uint32_t)r, best, besti)) { best = s; besti = (uint32_t)r; }
    }
    if (lane == 0) { s_d[wave] = best; s_i[wave] = besti; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (pair_less(s_d[w], s_i[w], best, besti)) { best = s_d[w]; besti = s_i[w]; }
        bd[blockIdx.x] = best;
        bi[blockIdx.x] = besti;
    }
}

// the blocks' results reduced by one block, in block order; no row with a comparable distance: row 0
__global__ void __launch_bounds__(256) medoid_pick(const double *__restrict__ bd, const uint32_t *__restrict__ bi,
                                                   int nb, uint32_t *__restrict__ out) {
    __shared__ double s_d[256];
    __shared__ uint32_t s_i[256];
    double best = INFINITY;
    uint32_t besti = kNone;
    for (int b = threadIdx.x; b < nb; b += 256)
        if (pair_less(bd[b], bi[b], best, besti)) { best = bd[b]; besti = bi[b]; }
    s_d[threadIdx.x] = best;
    s_i[threadIdx.x] = besti;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < 256; ++t)
            if (pair_less(s_d[t], s_i[t], best, besti)) { best = s_d[t]; besti = s_i[t]; }
        out[0] = besti == kNone ? 0u : besti;
    }
}

constexpr size_t kLdsStage = 48 << 10;  // stage a per-dimension table in LDS up to this many bytes

}  // namespace

int64_t sq8_stat_slabs(int64_t n) { return ceil_div(n, kSq8SlabRows); }

int medoid_nearest_blocks(int64_t n) { return (int)std::min<int64_t>(ceil_div(n, 4), 4096); }

// x: n rows of d floats on the device (16-B aligned); pmin / pmax: slabs·d floats (minmax), psum: slabs·d doubles (sum);
// ms: 2·d floats (min, scale), mean: d doubles.  Outputs that are not asked for are neither computed nor written.
void launch_sq8_col_stats(const float *x, int64_t n, int d, bool minmax, bool sum, float *pmin, float *pmax,
                          double *psum, float *ms, double *mean, hipStream_t st) {
    if (n <= 0 || (!minmax && !sum)) return;
    HIPANN_REQUIRE(d > 0 && minmax != sum, "sq8_col_stats: min / max or sums");
    const int64_t slabs = sq8_stat_slabs(n);
    HIPANN_REQUIRE(slabs <= INT32_MAX, "sq8_col_stats: too many rows");
    const dim3 grid((unsigned)slabs), block(kStatThreads), fgrid((unsigned)ceil_div(d, 256));
    if (d % 4 == 0) {
        if (minmax) hipLaunchKernelGGL((sq8_col_stats<4, true, false>), grid, block, 0, st, x, n, d, pmin, pmax, psum);
        else hipLaunchKernelGGL((sq8_col_stats<4, false, true>), grid, block, 0, st, x, n, d, pmin, pmax, psum);
    } else {
        if (minmax) hipLaunchKernelGGL((sq8_col_stats<1, true, false>), grid, block, 0, st, x, n, d, pmin, pmax, psum);
        else hipLaunchKernelGGL((sq8_col_stats<1, false, true>), grid, block, 0, st, x, n, d, pmin, pmax, psum);
    }
    if (minmax) hipLaunchKernelGGL((sq8_fold_stats<true, false>), fgrid, dim3(256), 0, st, pmin, pmax, psum, (int)slabs, d, n, ms, mean);
    else hipLaunchKernelGGL((sq8_fold_stats<false, true>), fgrid, dim3(256), 0, st, pmin, pmax, psum, (int)slabs, d, n, ms, mean);
    HIPANN_CHECK(hipGetLastError());
}

// x: n·d floats, ms: min[d] then scale[d] (device), out: n·d codes (16-B aligned)
void launch_sq8_encode(const float *x, int64_t n, int d, const float *ms, uint8_t *out, hipStream_t st) {
    if (n <= 0) return;
    HIPANN_REQUIRE(d > 0, "sq8_encode: d must be positive");
    const int W = d % 16 == 0 ? 16 : d % 4 == 0 ? 4 : 1;
    const int64_t groups = n * d / W;
    const size_t smem = (size_t)d * 8;
    const bool lds = smem <= kLdsStage;
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(groups, 256), 8192)), block(256);
#define HIPANN_SQ8_ENC(WW)                                                                                           \
    do {                                                                                                             \
        if (lds) hipLaunchKernelGGL((sq8_encode<WW, true>), grid, block, smem, st, x, groups, d, ms, out);          \
        else hipLaunchKernelGGL((sq8_encode<WW, false>), grid, block, 0, st, x, groups, d, ms, out);                 \
    } while (0)
    if (W == 16) HIPANN_SQ8_ENC(16);
    else if (W == 4) HIPANN_SQ8_ENC(4);
    else HIPANN_SQ8_ENC(1);
#undef HIPANN_SQ8_ENC
    HIPANN_CHECK(hipGetLastError());
}

// mean: d doubles (device); bd / bi: medoid_nearest_blocks(n) doubles / words of scratch; out: one word (device)
void launch_medoid_nearest(const float *x, int64_t n, int d, const double *mean, double *bd, uint32_t *bi,
                           uint32_t *out, hipStream_t st) {
    if (n <= 0) return;
    HIPANN_REQUIRE(d > 0 && n <= (int64_t)UINT32_MAX, "medoid_nearest: unsupported shape");
    const int nb = medoid_nearest_blocks(n);
    const size_t smem = (size_t)d * 8;
    const bool lds = smem <= kLdsStage, v4 = d % 4 == 0;
    const dim3 grid((unsigned)nb), block(256);
    if (v4) {
        if (lds) hipLaunchKernelGGL((medoid_nearest<true, true>), grid, block, smem, st, x, n, d, mean, bd, bi);
        else hipLaunchKernelGGL((medoid_nearest<true, false>), grid, block, 0, st, x, n, d, mean, bd, bi);
    } else {
        if (lds) hipLaunchKernelGGL((medoid_nearest<false, true>), grid, block, smem, st, x, n, d, mean, bd, bi);
        else hipLaunchKernelGGL((medoid_nearest<false, false>), grid, block, 0, st, x, n, d, mean, bd, bi);
    }
    hipLaunchKernelGGL(medoid_pick, dim3(1), dim3(256), 0, st, bd, bi, nb, out);
    HIPANN_CHECK(hipGetLastError());
}

}  // namespace hipann
