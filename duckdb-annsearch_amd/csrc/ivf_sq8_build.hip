// ivf_sq8_build.hip — IVF SQ8 on the build side: training the 8-bit quantizer (hipann_ivfsq_train) and adding rows
// (hipann_ivfsq_add), both on the device.  The layout of the tiled codes, N(row) and the certificate they feed are
// stated at the head of ivf_sq8.hip.
//
// ivf_sq_minmax — FAISS's ScalarQuantizer::train for QT_8bit with the min/max range statistic: per dimension the
// minimum and maximum of e = x − g_assign (by_residual) or x.  A column reduction that reads the n·d·4 bytes once.
// Lanes run along the dimensions (a wave reads 64 consecutive floats of a row; for d < 64 it takes 64 / dpow2 rows at
// once), a block of 4 waves walks a strip of rows, grid.y tiles the columns by 256 so that a lane's running values are
// four (min, max) register pairs whatever d is.  The row's list id is read once per row and column tile, the centroid
// row comes from the L2.  The running values are order-preserving bits (sq_order_bits) compared as integers, so a NaN
// of either sign wins its column's maximum or minimum and the host sees a non-finite quantizer.  Waves combine with
// LDS atomics; one global atomicMin / atomicMax per dimension and block; ivf_sq_minmax_final turns the bits into vmin
// and vdiff = fl32(max − min).  Min and max are exact, so the result is determined by the assignment.
//
// ivf_sq_encode_append — FAISS's encode fused with the append: no row-major code buffer, no re-tile pass.  One wave per
// new row, a lane owns groups of 8 consecutive dimensions (two float4 of x, two of the centroid where the row is
// 16-byte aligned), vmin / vdiff / s staged in the LDS once per block.  Per entry, in fp32 and in this order:
// e = x − g, xi = vdiff != 0 ? (e − vmin) / vdiff : 0 clamped to [0, 1], code = (int)(255·xi); the division is the
// correctly rounded one (the file is built with -fhip-fp32-correctly-rounded-divide-sqrt).  The 8 codes are one 8-byte
// store at the row's (pass, row-in-pass) of the tiled layout; all 32·nstep dimensions are written (zeros past d: vdiff
// is staged as 0 there), so nothing depends on what the slack held.  The wave accumulates ‖c‖² and, for L2,
// N(row) = ‖s∘c‖² + 2 g·(s∘c) from the codes in its registers — per entry the terms ivf_sq_row_terms adds, in another
// order (8 consecutive dimensions per lane, not one per lane and stride): both are plain fp32 sums of the same 2·d
// terms, which is all the certificate's third line assumes of N (any order of d additions).  Lane 0 writes N, the label
// and raises the index's max ‖c‖² word (read first: once the maximum stands, a row costs a load, not an atomic).
// With dst == nullptr the kernel is the statistics-only pass: it flags rows holding a non-finite entry and writes
// nothing else, so a refused add leaves the index as it was.
//
// ivf_sq_regroup — growth in one launch: a block per pass of the new layout copies the old pass (nstep KiB, 16-byte
// accesses) or writes zeros; a tail of the grid moves labels and N(row), 1024 physical rows per block.
#include "ivf.hpp"
#include "ivf_sq8_dev.hpp"

#include <algorithm>

namespace hipann {
namespace {

constexpr int SQB_COLS = 256;   // dimensions per column tile of ivf_sq_minmax (4 per lane)
constexpr int SQB_ROWS = 1024;  // physical rows per tail block of ivf_sq_regroup
constexpr size_t SQB_LDS_MAX = 160 * 1024;

__global__ void __launch_bounds__(256) ivf_sq_minmax_init(unsigned *__restrict__ bits, int d) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < d) {
        bits[e] = 0xffffffffu;
        bits[d + e] = 0u;
    }
}

template <bool RES>
__global__ void __launch_bounds__(256)
ivf_sq_minmax(const float *__restrict__ x, const int64_t *__restrict__ assign, const float *__restrict__ cen, int64_t n,
              int d, int nlist, int dp2, int64_t strip, unsigned *__restrict__ bits) {
    __shared__ unsigned smin[SQB_COLS], smax[SQB_COLS];
    smin[threadIdx.x] = 0xffffffffu;
    smax[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rpw = 64 / dp2;  // rows a wave takes at once (1 from d = 33 on)
    const int sub = lane / dp2, col = lane - sub * dp2;
    const int c0 = blockIdx.y * SQB_COLS;
    const int nu = dp2 == 64 ? 4 : 1;
    const int64_t r_begin = (int64_t)blockIdx.x * strip, r_end = r_begin + strip < n ? r_begin + strip : n;
    unsigned mn[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[4] = {0u, 0u, 0u, 0u};
#pragma unroll 2
    for (int64_t r = r_begin + w * rpw + sub; r < r_end; r += 4 * rpw) {
        const float *xr = x + r * (int64_t)d;
        const float *g = nullptr;
        bool ok = true;
        if (RES) {
            const int64_t a = assign[r];
            ok = a >= 0 && a < nlist;
            g = cen + (ok ? a : 0) * (int64_t)d;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = c0 + 64 * u + col;
            if (u < nu && e < d) {
                float v = xr[e];
                if (RES) v = ok ? v - g[e] : __uint_as_float(0x7fc00000u);
                const unsigned o = sq_order_bits(v);
                mn[u] = o < mn[u] ? o : mn[u];
                mx[u] = o > mx[u] ? o : mx[u];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (u < nu && c0 + 64 * u + col < d && mx[u] >= mn[u]) {  // (a lane that saw no row holds max < min)
            atomicMin(&smin[64 * u + col], mn[u]);
            atomicMax(&smax[64 * u + col], mx[u]);
        }
    }
    __syncthreads();
    const int e = c0 + threadIdx.x;
    if (e < d && smax[threadIdx.x] >= smin[threadIdx.x]) {
        atomicMin(&bits[e], smin[threadIdx.x]);
        atomicMax(&bits[d + e], smax[threadIdx.x]);
    }
}

__global__ void __launch_bounds__(256)
ivf_sq_minmax_final(const unsigned *__restrict__ bits, int d, float *__restrict__ vmin, float *__restrict__ vdiff) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= d) return;
    const float lo = sq_order_float(bits[e]), hi = sq_order_float(bits[d + e]);
    vmin[e] = lo;
    vdiff[e] = hi - lo;
}

template <bool RES>
__global__ void __launch_bounds__(256)
ivf_sq_encode_append(const float *__restrict__ x, int64_t n, int d, int nstep, const int64_t *__restrict__ assign,
                     int nlist, const float *__restrict__ cen, const float *__restrict__ vmin,
                     const float *__restrict__ vdiff, const float *__restrict__ sb, const int64_t *__restrict__ dst,
                     const int64_t *__restrict__ labels, int64_t label_base, const int64_t *__restrict__ list_off,
                     const int64_t *__restrict__ tpass_off, int l2, unsigned char *__restrict__ codes_t,
                     float *__restrict__ rown, int64_t *__restrict__ ids, unsigned *__restrict__ cmax2,
                     unsigned *__restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) float smem_sqb[];
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (!dst) {  // the statistics-only pass (a kernel argument: the whole grid takes this branch)
        if (row >= n) return;
        bool nf = false;
        for (int e = lane; e < d; e += 64) nf |= (__float_as_uint(x[row * (int64_t)d + e]) & 0x7f800000u) == 0x7f800000u;
        if (nf) atomicOr(bad, 1u);
        return;
    }
    const int dpad = 32 * nstep;
    float *s_vmin = smem_sqb, *s_vdiff = smem_sqb + dpad, *s_s = smem_sqb + 2 * dpad;
    for (int t = threadIdx.x; t < dpad; t += 256) {
        s_vmin[t] = t < d ? vmin[t] : 0.f;
        s_vdiff[t] = t < d ? vdiff[t] : 0.f;  // 0 past d: those codes are 0
        s_s[t] = sb[t];
    }
    __syncthreads();
    if (row >= n) return;
    const int64_t a = assign[row], p = dst[row];
    if (a < 0 || a >= nlist || p < 0) return;  // (the host has checked both)
    const float *xr = x + row * (int64_t)d;
    const float *g = RES ? cen + a * (int64_t)d : nullptr;
    const int64_t rel = p - list_off[a];
    unsigned char *pass = codes_t + (tpass_off[a] + (rel >> 5)) * (int64_t)nstep * 1024;
    const int rr = (int)(rel & 31);
    // float4 loads where every row starts on 16 bytes
    const bool vec = (d & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | (RES ? reinterpret_cast<uintptr_t>(cen) : 0)) & 15) == 0;
    float nn = 0.f, cc = 0.f;
    for (int gi = lane; gi < nstep * 4; gi += 64) {
        const int e0 = gi * 8;
        float xv[8], gv[8];
        if (vec && e0 + 8 <= d) {
            const float4 x0 = *reinterpret_cast<const float4 *>(xr + e0), x1 = *reinterpret_cast<const float4 *>(xr + e0 + 4);
            xv[0] = x0.x, xv[1] = x0.y, xv[2] = x0.z, xv[3] = x0.w, xv[4] = x1.x, xv[5] = x1.y, xv[6] = x1.z, xv[7] = x1.w;
            if (RES) {
                const float4 g0 = *reinterpret_cast<const float4 *>(g + e0), g1 = *reinterpret_cast<const float4 *>(g + e0 + 4);
                gv[0] = g0.x, gv[1] = g0.y, gv[2] = g0.z, gv[3] = g0.w, gv[4] = g1.x, gv[5] = g1.y, gv[6] = g1.z, gv[7] = g1.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const bool in = e0 + k < d;
                xv[k] = in ? xr[e0 + k] : 0.f;
                if (RES) gv[k] = in ? g[e0 + k] : 0.f;
            }
        }
        unsigned w2[2] = {0u, 0u};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = e0 + k;
            const float ev = RES ? xv[k] - gv[k] : xv[k];
            const float vm = s_vmin[e], vd = s_vdiff[e];
            float xi = 0.f;
            if (vd != 0.f) {
                xi = (ev - vm) / vd;
                if (xi < 0.f) xi = 0.f;
                if (xi > 1.f) xi = 1.f;
            }
            const int c = (int)(255.0f * xi);
            const float cf = (float)c, sc = s_s[e] * cf;
            cc = fmaf(cf, cf, cc);
            nn = fmaf(sc, sc, nn);
            if (RES) nn = fmaf(2.f * gv[k], sc, nn);
            w2[k >> 2] |= (unsigned)(c & 255) << (8 * (k & 3));
        }
        *reinterpret_cast<uint2 *>(pass + sq_tile_off(rr, e0)) = make_uint2(w2[0], w2[1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nn += __shfl_xor(nn, o);
        cc += __shfl_xor(cc, o);
    }
    if (lane == 0) {
        if (l2) rown[p] = nn;
        ids[p] = labels ? labels[row] : label_base + row;
        const unsigned cb = __float_as_uint(cc);  // (bits of a non-negative float order as integers)
        if (cb > *reinterpret_cast<volatile unsigned *>(cmax2)) atomicMax(cmax2, cb);
    }
}

// the last l in [0, nlist) with off[l] <= v
__device__ __forceinline__ int sqb_find(const int64_t *__restrict__ off, int nlist, int64_t v) {
    int lo = 0, hi = nlist - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(256)
ivf_sq_regroup(const uint4 *__restrict__ src, const int64_t *__restrict__ tp_old, const int64_t *__restrict__ off_old,
               const int *__restrict__ len_old, const int64_t *__restrict__ tp_new, const int64_t *__restrict__ off_new,
               int nlist, int nstep, int64_t npass_new, int64_t nrows_new, const int64_t *__restrict__ ids_old,
               const float *__restrict__ rown_old, uint4 *__restrict__ dst, int64_t *__restrict__ ids_new,
               float *__restrict__ rown_new) {
    const int64_t b = blockIdx.x;
    if (b < npass_new) {
        const int l = sqb_find(tp_new, nlist, b);
        const int64_t rel = b - tp_new[l];
        const bool live = rel < ((int64_t)len_old[l] + 31) >> 5;
        const uint4 *in = src + (live ? tp_old[l] + rel : 0) * (int64_t)nstep * 64;
        uint4 *out = dst + b * (int64_t)nstep * 64;
        for (int t = threadIdx.x; t < nstep * 64; t += 256) out[t] = live ? in[t] : make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const int64_t r0 = (b - npass_new) * SQB_ROWS;
    for (int u = 0; u < SQB_ROWS / 256; ++u) {
        const int64_t r = r0 + u * 256 + threadIdx.x;
        if (r >= nrows_new) return;
        const int l = sqb_find(off_new, nlist, r);
        const int64_t rel = r - off_new[l];
        const bool live = rel < len_old[l];
        ids_new[r] = live ? ids_old[off_old[l] + rel] : (int64_t)-1;
        if (rown_new) rown_new[r] = live ? rown_old[off_old[l] + rel] : 0.f;
    }
}

}  // namespace

void launch_ivf_sq_minmax(const float *x, int64_t n, int d, const int64_t *assign, const float *centroids, int nlist,
                          unsigned *bits, float *vmin, float *vdiff, hipStream_t st) {
    HIPANN_REQUIRE(n > 0 && d > 0, "IVF SQ8 train: no rows");
    int dp2 = 1;
    while (dp2 < d && dp2 < 64) dp2 <<= 1;
    const int rpw = 64 / dp2, gy = (int)ceil_div(d, SQB_COLS), gd = (int)ceil_div(d, 256);
    // a few blocks per CU (256 CUs): strips of at least 64 wave steps, whole block steps
    int64_t strip = std::max<int64_t>(ceil_div(n, std::max(1, 2048 / gy)), (int64_t)64 * 4 * rpw);
    strip = ceil_div(strip, 4 * rpw) * (4 * rpw);
    const int64_t gx = ceil_div(n, strip);
    HIPANN_REQUIRE(gx < (int64_t)0x7fffffff && gy < 65536, "IVF SQ8 train: too many rows or dimensions");
    hipLaunchKernelGGL(ivf_sq_minmax_init, dim3((unsigned)gd), dim3(256), 0, st, bits, d);
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (centroids)
        hipLaunchKernelGGL(ivf_sq_minmax<true>, grid, dim3(256), 0, st, x, assign, centroids, n, d, nlist, dp2, strip, bits);
    else
        hipLaunchKernelGGL(ivf_sq_minmax<false>, grid, dim3(256), 0, st, x, assign, centroids, n, d, nlist, dp2, strip, bits);
    hipLaunchKernelGGL(ivf_sq_minmax_final, dim3((unsigned)gd), dim3(256), 0, st, bits, d, vmin, vdiff);
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_sq_encode_append(const float *x, int64_t n, const IvfSqView &v, const int64_t *assign,
                                 const int64_t *dst, const int64_t *labels, int64_t label_base, const int64_t *list_off,
                                 unsigned char *codes_t, float *rown, int64_t *ids, unsigned *cmax2, unsigned *bad,
                                 hipStream_t st) {
    if (n <= 0) return;
    HIPANN_REQUIRE(ceil_div(n, 4) < (int64_t)0x7fffffff, "IVF SQ8 add: too many rows");
    // (checked by the statistics pass too: an add is refused here before anything of the index has changed)
    const size_t lds = (size_t)3 * 32 * v.nstep * sizeof(float), smem = dst ? lds : 0;
    HIPANN_REQUIRE(lds <= SQB_LDS_MAX, "IVF SQ8 add: the quantizer does not fit the LDS");
    HIPANN_REQUIRE(!dst || v.metric == kIP || rown, "IVF SQ8 add: L2 needs the row terms");
    const dim3 grid((unsigned)ceil_div(n, 4)), block(256);
    auto go = [&](auto kern) {
        // above the default 64 KiB (d above 5440) the attribute is set on every launch: it is kept per device, and a
        // process-wide "done" flag would be wrong for a handle on a second device and racy between handles
        if (smem > (size_t)64 * 1024)
            HIPANN_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)SQB_LDS_MAX));
        hipLaunchKernelGGL(kern, grid, block, smem, st, x, n, v.d, v.nstep, assign, v.nlist, v.centroids, v.vmin, v.vdiff,
                           v.sb, dst, labels, label_base, list_off, v.tpass_off, v.metric == kL2 ? 1 : 0, codes_t, rown,
                           ids, cmax2, bad);
    };
    if (v.by_residual) go(ivf_sq_encode_append<true>);
    else go(ivf_sq_encode_append<false>);
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_sq_regroup(const IvfSqView &v, const int64_t *list_off, const int *list_len, const int64_t *tp_new,
                           const int64_t *off_new, int64_t npass_new, int64_t nrows_new, unsigned char *codes_new,
                           int64_t *ids_new, float *rown_new, hipStream_t st) {
    const int64_t blocks = npass_new + ceil_div(nrows_new, SQB_ROWS);
    if (blocks <= 0) return;
    HIPANN_REQUIRE(blocks < (int64_t)0x7fffffff, "IVF SQ8 add: too many passes");
    hipLaunchKernelGGL(ivf_sq_regroup, dim3((unsigned)blocks), dim3(256), 0, st,
                       reinterpret_cast<const uint4 *>(v.codes_t), v.tpass_off, list_off, list_len, tp_new, off_new,
                       v.nlist, v.nstep, npass_new, nrows_new, v.ids, v.rown, reinterpret_cast<uint4 *>(codes_new),
                       ids_new, rown_new);
    HIPANN_CHECK(hipGetLastError());
}

}  // namespace hipann
