// diskann.hip — DiskANN batch-distance bridge for gfx950 (include/hip_diskann_bridge.h).
//
// Replaces src/metal_diskann_bridge.mm (:155-253 single query, :255-323 multi query) and the Metal
// kernels faiss-metal/shaders/diskann_distance.metal:15-194 (one 32-lane simdgroup per candidate).
// Semantics: metric 0 → Σ(q−c)², metric 1 → −Σ q·c  (rust_lib/src/distance.rs:15-24).
//
// Kernels
//   dist_rows      — candidates as contiguous fp32 rows (the reference ABI: the caller gathered
//                    them on the host).  One wave per candidate, float4 loads, query chunks from
//                    L1/L2 (consecutive candidates share a query: query_map is grouped per query by
//                    the lock-step BFS, disk_provider.rs:556-577).
//   dist_ids_f32   — HBM-resident fp32 database, candidate = row id (gather).  One wave per row.
//   dist_ids_sq8   — HBM-resident SQ8 codes (provider.rs:161-210), half a wave per row, 16 codes per
//                    lane-load; dequantised bit-identically to the reference, (code/255)·scale + min
//                    (sq8_value).  The resident traversal (diskann_bfs.hip) keeps the fused
//                    (q − min) − code·(scale/255) form, within 1 ulp per element.
//
// Host side: per-thread stream + staging (thread-safe, unlike the Metal bridge's shared ring,
// metal_diskann_bridge.mm:52-53), the launchers, a registry of HBM databases, the resident search (the traversal of
// diskann_bfs.hip, the host BFS for the queries it flags) and the C ABI.  diskann_hip_search_batch — the lock-step
// best-first BFS of DiskProvider::search_batch (disk_provider.rs:470-652), whose per-step distances go through
// launch_ids — is diskann_host_bfs.cpp.  Graph build, add, remove and prune: diskann_graph.cpp.
#include "diskann_db.hpp"
#include "diskann_kernels.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace hipann {

// One lane's share of a wave's fp32 row distance: Σ q·c (IP) or Σ (q − c)² over the dims lane, lane + 64, … (float4
// units with VEC4).  The term order within a lane is part of the exact-reference contract.
template <bool IP, bool VEC4>
__device__ __forceinline__ float f32_lane_sum(const float *q, const float *c, int d, int lane) {
    float s = 0.f;
    if (VEC4) {
        const float4 *q4 = reinterpret_cast<const float4 *>(q);
        const float4 *c4 = reinterpret_cast<const float4 *>(c);
        for (int j = lane; j < (d >> 2); j += 64) {
            const float4 a = q4[j], b = c4[j];
            if (IP) {
                s = fmaf(a.x, b.x, s); s = fmaf(a.y, b.y, s); s = fmaf(a.z, b.z, s); s = fmaf(a.w, b.w, s);
            } else {
                float t;
                t = a.x - b.x; s = fmaf(t, t, s);
                t = a.y - b.y; s = fmaf(t, t, s);
                t = a.z - b.z; s = fmaf(t, t, s);
                t = a.w - b.w; s = fmaf(t, t, s);
            }
        }
    } else {
        for (int j = lane; j < d; j += 64) {
            if (IP) s = fmaf(q[j], c[j], s);
            else { const float t = q[j] - c[j]; s = fmaf(t, t, s); }
        }
    }
    return s;
}

// candidates: total_n rows of d floats; qmap == nullptr → every candidate uses query 0.
template <bool IP, bool VEC4>
__global__ void __launch_bounds__(256) dist_rows(const float *__restrict__ queries, const float *__restrict__ cands,
                                                 const unsigned *__restrict__ qmap, int total_n, int d,
                                                 float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= total_n) return;
    const unsigned qi = qmap ? qmap[w] : 0u;
    const float s = wave_sum(f32_lane_sum<IP, VEC4>(queries + (int64_t)qi * d, cands + w * (int64_t)d, d, lane));
    if (lane == 0) out[w] = IP ? -s : s;
}

// The host BFS's visited sets on the device (vbits != nullptr): one bit per (query, row), vwords words per query.
// A candidate whose bit was already set (an earlier step of its query; the host sends an id once per step, since the
// slots of one launch mark in no particular order) is not evaluated: its output is kVisitedBits
// (diskann_kernels.hpp).
__device__ __forceinline__ bool visit_first(unsigned *vbits, int64_t vwords, unsigned qi, unsigned id) {
    const unsigned bit = 1u << (id & 31u);
    return (atomicOr(vbits + (int64_t)qi * vwords + (id >> 5), bit) & bit) == 0u;
}

template <bool IP, bool VEC4>
__global__ void __launch_bounds__(256) dist_ids_f32(const float *__restrict__ queries, const float *__restrict__ db,
                                                    const unsigned *__restrict__ ids, const unsigned *__restrict__ qmap,
                                                    int total_n, int d, int64_t n, float *__restrict__ out,
                                                    unsigned *__restrict__ vbits, int64_t vwords) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= total_n) return;
    const unsigned id = ids[w];
    if (id >= n) return;  // empty slot of the BFS's fixed per-query layout
    if (vbits) {
        const int first = lane == 0 ? (int)visit_first(vbits, vwords, qmap[w], id) : 0;
        if (!__shfl(first, 0)) {
            if (lane == 0) out[w] = __uint_as_float(kVisitedBits);
            return;
        }
    }
    const float s = wave_sum(f32_lane_sum<IP, VEC4>(queries + (int64_t)qmap[w] * d, db + (int64_t)id * d, d, lane));
    if (lane == 0) out[w] = IP ? -s : s;
}

// SQ8 decode exactly as provider.rs:140-146: (code as f32 / 255.0) * scale + min, two roundings (no fma).
// code/255 is the correctly rounded quotient: q0 = code·fl(1/255), one fma residual step (checked for all
// 256 codes against IEEE division, tests/test_oracle.py).
__device__ __forceinline__ float sq8_value(float code, float scale, float mn) {
    constexpr float r = 1.0f / 255.0f;
    const float q0 = code * r;
    const float a = fmaf(fmaf(-q0, 255.0f, code), r, q0);
    const float b = a * scale;
    return b + mn;
}

// SQ8: a quarter wave (16 lanes) per candidate, 16 codes (one uint4) per lane per unit, every unit of the lane's
// share of the row (d <= 2048: up to 8) issued before any is consumed — 96 code loads of 16 B in flight per wave at
// d 1536, the gather's latency hidden by loads rather than waves.  `ab` holds per-dimension (scale, min) pairs in
// LDS, loaded once per block; blocks loop over groups of 16 candidates.  Requires d % 16 == 0 and d <= 2048 (host
// checks; otherwise the scalar path below).
template <bool IP>
__global__ void __launch_bounds__(256) dist_ids_sq8(const float *__restrict__ queries, const uint8_t *__restrict__ codes,
                                                    const float2 *__restrict__ ab_g, const unsigned *__restrict__ ids,
                                                    const unsigned *__restrict__ qmap, int total_n, int d,
                                                    int64_t n, float *__restrict__ out, unsigned *__restrict__ vbits,
                                                    int64_t vwords) {
    extern __shared__ __attribute__((aligned(16))) float2 ab[];
    for (int j = threadIdx.x; j < d; j += 256) ab[j] = ab_g[j];
    __syncthreads();
    const int ql = threadIdx.x & 15;
    for (int64_t c0 = (int64_t)blockIdx.x * 16; c0 < total_n; c0 += (int64_t)gridDim.x * 16) {
        const int64_t c = c0 + (threadIdx.x >> 4);
        const unsigned id = c < total_n ? ids[c] : 0xffffffffu;
        bool valid = id < n;  // also skips empty slots of the BFS's fixed per-query layout
        if (vbits) {  // the candidate's visited bit, by the first lane of its quarter wave
            const int first = valid && ql == 0 ? (int)visit_first(vbits, vwords, qmap[c], id) : 0;
            const bool fresh = __shfl(first, (int)(threadIdx.x & 63) & ~15) != 0;
            if (valid && !fresh && ql == 0) out[c] = __uint_as_float(kVisitedBits);
            valid = valid && fresh;
        }
        float s = 0.f;
        if (valid) {
            const float *q = queries + (int64_t)qmap[c] * d;
            const uint8_t *row = codes + (int64_t)id * d;
            uint4 raws[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j0 = ql * 16 + u * 256;
                if (j0 < d) raws[u] = *reinterpret_cast<const uint4 *>(row + j0);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j0 = ql * 16 + u * 256;
                if (j0 >= d) break;
                const uint4 raw = raws[u];
                const unsigned wv[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float4 qv = *reinterpret_cast<const float4 *>(q + j0 + 4 * e);
                    const float qa[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const float code = (float)((wv[e] >> (8 * b)) & 0xffu);
                        const float2 p = ab[j0 + 4 * e + b];
                        const float v = sq8_value(code, p.x, p.y);
                        if (IP) s = fmaf(qa[b], v, s);
                        else { const float t = qa[b] - v; s = fmaf(t, t, s); }
                    }
                }
            }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (valid && ql == 0) out[c] = IP ? -s : s;
    }
}

template <bool IP>
__global__ void __launch_bounds__(256) dist_ids_sq8_scalar(const float *__restrict__ queries,
                                                           const uint8_t *__restrict__ codes,
                                                           const float2 *__restrict__ ab, const unsigned *__restrict__ ids,
                                                           const unsigned *__restrict__ qmap, int total_n, int d,
                                                           int64_t n, float *__restrict__ out, unsigned *__restrict__ vbits,
                                                           int64_t vwords) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= total_n) return;
    const unsigned id = ids[w];
    if (id >= n) return;
    if (vbits) {
        const int first = lane == 0 ? (int)visit_first(vbits, vwords, qmap[w], id) : 0;
        if (!__shfl(first, 0)) {
            if (lane == 0) out[w] = __uint_as_float(kVisitedBits);
            return;
        }
    }
    const float *q = queries + (int64_t)qmap[w] * d;
    const uint8_t *row = codes + (int64_t)id * d;
    float s = 0.f;
    for (int j = lane; j < d; j += 64) {
        const float2 p = ab[j];
        const float v = sq8_value((float)row[j], p.x, p.y);
        if (IP) s = fmaf(q[j], v, s);
        else { const float t = q[j] - v; s = fmaf(t, t, s); }
    }
    s = wave_sum(s);
    if (lane == 0) out[w] = IP ? -s : s;
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
namespace {

int g_avail = -1;

bool device_ok() {
    if (g_avail < 0) {
        int n = 0;
        g_avail = (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? 1 : 0;
    }
    return g_avail == 1;
}

// Per-thread stream and staging (each calling thread owns its buffers).
struct ThreadCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf q, c, m, ids, out;
    HostBuf hq, hc, hm, hids, hout;
    ~ThreadCtx() {
        if (stream) { (void)hipStreamDestroy(stream); }
    }
    void init() {
        int dev = 0;
        HIPANN_CHECK(hipGetDevice(&dev));
        if (stream && dev == device) return;
        if (stream) (void)hipStreamDestroy(stream);
        device = dev;
        HIPANN_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    }
};

thread_local ThreadCtx t_ctx;
// host-pointer calls with at most this many candidate bytes run zero-copy from pinned staging
constexpr size_t kZeroCopyMax = (size_t)1 << 20;

void launch_rows(const float *q, const float *c, const unsigned *m, int total_n, int d, int metric, float *out,
                 hipStream_t st) {
    const bool v4 = (d % 4 == 0) && ((uintptr_t)q % 16 == 0) && ((uintptr_t)c % 16 == 0);
    dim3 grid((unsigned)ceil_div(total_n, 4)), block(256);
    if (metric == kIP) {
        if (v4) hipLaunchKernelGGL((dist_rows<true, true>), grid, block, 0, st, q, c, m, total_n, d, out);
        else hipLaunchKernelGGL((dist_rows<true, false>), grid, block, 0, st, q, c, m, total_n, d, out);
    } else {
        if (v4) hipLaunchKernelGGL((dist_rows<false, true>), grid, block, 0, st, q, c, m, total_n, d, out);
        else hipLaunchKernelGGL((dist_rows<false, false>), grid, block, 0, st, q, c, m, total_n, d, out);
    }
    HIPANN_CHECK(hipGetLastError());
}

}  // namespace

// (described where it is declared, diskann_db.hpp)
void launch_ids(DiskDB &db, const float *q, const unsigned *ids, const unsigned *m, int total_n, int metric,
                float *out, hipStream_t st, unsigned *vbits, int64_t vwords) {
    if (total_n <= 0) return;
    const int d = db.dim;
    if (db.fmt == DISKANN_HIP_FMT_F32) {
        const float *x = db.data.get<float>();
        const bool v4 = (d % 4 == 0) && ((uintptr_t)q % 16 == 0);
        dim3 grid((unsigned)ceil_div(total_n, 4)), block(256);
        if (metric == kIP) {
            if (v4) hipLaunchKernelGGL((dist_ids_f32<true, true>), grid, block, 0, st, q, x, ids, m, total_n, d, db.n, out, vbits, vwords);
            else hipLaunchKernelGGL((dist_ids_f32<true, false>), grid, block, 0, st, q, x, ids, m, total_n, d, db.n, out, vbits, vwords);
        } else {
            if (v4) hipLaunchKernelGGL((dist_ids_f32<false, true>), grid, block, 0, st, q, x, ids, m, total_n, d, db.n, out, vbits, vwords);
            else hipLaunchKernelGGL((dist_ids_f32<false, false>), grid, block, 0, st, q, x, ids, m, total_n, d, db.n, out, vbits, vwords);
        }
    } else {
        const uint8_t *x = db.data.get<uint8_t>();
        const float2 *ab = db.ab_raw.get<float2>();
        if (d % 16 == 0 && d <= 2048 && (uintptr_t)q % 16 == 0) {
            // ≤ 8 blocks per CU, each looping over groups of 16 candidates (dist_ids_sq8)
            dim3 grid((unsigned)std::min<int64_t>(ceil_div(total_n, 16), 2048)), block(256);
            const size_t smem = (size_t)d * sizeof(float2);
            if (metric == kIP) hipLaunchKernelGGL(dist_ids_sq8<true>, grid, block, smem, st, q, x, ab, ids, m, total_n, d, db.n, out, vbits, vwords);
            else hipLaunchKernelGGL(dist_ids_sq8<false>, grid, block, smem, st, q, x, ab, ids, m, total_n, d, db.n, out, vbits, vwords);
        } else {
            dim3 grid((unsigned)ceil_div(total_n, 4)), block(256);
            if (metric == kIP) hipLaunchKernelGGL(dist_ids_sq8_scalar<true>, grid, block, 0, st, q, x, ab, ids, m, total_n, d, db.n, out, vbits, vwords);
            else hipLaunchKernelGGL(dist_ids_sq8_scalar<false>, grid, block, 0, st, q, x, ab, ids, m, total_n, d, db.n, out, vbits, vwords);
        }
    }
    HIPANN_CHECK(hipGetLastError());
}

// (described where it is declared, diskann_db.hpp; the copies are from pageable memory, so the vectors may go once
// the calls return)
void sq8_fill_decode_tables(DiskDB &db, const float *sq8_min, const float *sq8_scale, hipStream_t st) {
    const int dim = db.dim;
    std::vector<float> ab((size_t)dim * 2), abr((size_t)dim * 2);
    for (int j = 0; j < dim; ++j) {
        ab[2 * j] = sq8_scale[j] / 255.0f;
        ab[2 * j + 1] = sq8_min[j];
        abr[2 * j] = sq8_scale[j];
        abr[2 * j + 1] = sq8_min[j];
    }
    db.ab.ensure(ab.size() * 4, db.device);
    db.ab_raw.ensure(abr.size() * 4, db.device);
    HIPANN_CHECK(hipMemcpyAsync(db.ab.p, ab.data(), ab.size() * 4, hipMemcpyHostToDevice, st));
    HIPANN_CHECK(hipMemcpyAsync(db.ab_raw.p, abr.data(), abr.size() * 4, hipMemcpyHostToDevice, st));
}

// (described where it is declared, diskann_db.hpp)
void resident_search_locked(DiskDB *db, const uint32_t *eps, int n_ep, const float *queries_dev, int nq, int k,
                            int l_search, int metric, int64_t *out_ids_dev, float *out_d_dev, int64_t *stats,
                            hipStream_t st) {
    if (stats) { stats[0] = stats[1] = stats[2] = stats[3] = 0; }
    if (nq == 0) return;
    const uint32_t N = (uint32_t)db->n;
    const int L = std::max(l_search, std::min<int>(k, (int)std::min<int64_t>(db->n, INT32_MAX)));
    const int kk = k;
    std::vector<int> flags((size_t)nq, 0);
    const bool gpu_ok = db->n > 0 && diskann_bfs_supported(db->dim, db->fmt, db->R, n_ep, L, N);
    int64_t gsteps = 0, gevals = 0, gpops = 0;
    if (gpu_ok) {
        const int64_t vwords = ((int64_t)N + 31) / 32;
        // bound the visited bitmaps to ~2 GiB: sub-batches of queries
        const int64_t per = std::max<int64_t>(1, std::min<int64_t>(nq, ((int64_t)2 << 30) / (vwords * 4)));
        db->visited.ensure((size_t)per * vwords * 4, db->device);
        db->flags.ensure((size_t)nq * 4, db->device);
        db->bstats.ensure(72, db->device);
        db->eps_dev.ensure((size_t)std::max(n_ep, 1) * 4, db->device);
        if (n_ep) HIPANN_CHECK(hipMemcpyAsync(db->eps_dev.p, eps, (size_t)n_ep * 4, hipMemcpyHostToDevice, st));
        HIPANN_CHECK(hipMemsetAsync(db->bstats.p, 0, 72, st));
        for (int64_t q0 = 0; q0 < nq; q0 += per) {
            const int64_t qn = std::min<int64_t>(per, nq - q0);
            HIPANN_CHECK(hipMemsetAsync(db->visited.p, 0, (size_t)qn * vwords * 4, st));
            ScopedTiming tm(db->timer, st);
            launch_diskann_bfs(queries_dev + q0 * db->dim, (int)qn, db->dim, db->fmt, db->data.p,
                               db->ab.get<float2>(), db->adj_dev.get<uint32_t>(), db->dupw.get<uint32_t>(), db->R, N,
                               db->eps_dev.get<uint32_t>(), n_ep, kk, L, metric, db->visited.get<uint32_t>(),
                               vwords, out_ids_dev + q0 * kk, out_d_dev + q0 * kk, db->flags.get<int>() + q0,
                               db->bstats.get<unsigned long long>(), st);
        }
        unsigned long long hs[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        HIPANN_CHECK(hipMemcpyAsync(flags.data(), db->flags.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipMemcpyAsync(hs, db->bstats.p, 72, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        if (hs[3] + hs[4] + hs[5] + hs[6] + hs[7] + hs[8]) {  // tuning builds (HIPANN_BFS_PROF)
            const double st = (double)std::max<unsigned long long>(hs[2], 1);
            std::fprintf(stderr,
                         "[bfs-prof] wave-0 cycles per step: select %.0f adjacency %.0f dedupe %.0f visited %.0f "
                         "dist %.0f insert %.0f\n",
                         hs[3] / st, hs[4] / st, hs[5] / st, hs[6] / st, hs[7] / st, hs[8] / st);
        }
        gevals = (int64_t)hs[0];
        gsteps = (int64_t)hs[1];
        gpops = (int64_t)hs[2];
    } else {
        std::fill(flags.begin(), flags.end(), 1);
    }
    // host BFS for flagged queries (exact; queries are independent)
    std::vector<int> redo;
    for (int i = 0; i < nq; ++i)
        if (flags[i]) redo.push_back(i);
    int64_t hsteps = 0, hevals = 0;
    if (!redo.empty()) {
        const int nr = (int)redo.size(), dim = db->dim;
        if (db->adj_host_stale) {  // a graph build in progress: the host copy as of this batch's frozen graph
            db->adj_host.resize((size_t)db->n * db->R);
            HIPANN_CHECK(hipMemcpyAsync(db->adj_host.data(), db->adj_dev.p, db->adj_host.size() * 4,
                                        hipMemcpyDeviceToHost, st));
            HIPANN_CHECK(hipStreamSynchronize(st));
            db->adj_host_stale = false;
        }
        std::vector<float> qh((size_t)nr * dim);
        for (int j = 0; j < nr; ++j)
            HIPANN_CHECK(hipMemcpyAsync(qh.data() + (size_t)j * dim, queries_dev + (size_t)redo[j] * dim,
                                        (size_t)dim * 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        std::vector<int64_t> oi((size_t)nr * kk);
        std::vector<float> od((size_t)nr * kk);
        int64_t hst[4] = {0, 0, 0, 0};
        host_bfs(db, db->adj_host.data(), db->R, eps, n_ep, qh.data(), nr, kk, l_search, metric, oi.data(),
                 od.data(), hst);
        for (int j = 0; j < nr; ++j) {
            HIPANN_CHECK(hipMemcpyAsync(out_ids_dev + (size_t)redo[j] * kk, oi.data() + (size_t)j * kk,
                                        (size_t)kk * 8, hipMemcpyHostToDevice, st));
            HIPANN_CHECK(hipMemcpyAsync(out_d_dev + (size_t)redo[j] * kk, od.data() + (size_t)j * kk,
                                        (size_t)kk * 4, hipMemcpyHostToDevice, st));
        }
        HIPANN_CHECK(hipStreamSynchronize(st));
        hevals = hst[0];
        hsteps = hst[1];
    }
    if (stats) {
        stats[0] = gevals + hevals;
        stats[1] = std::max(gsteps, hsteps);
        stats[2] = gpops;
        stats[3] = (int64_t)redo.size();
    }
}

}  // namespace hipann

using namespace hipann;

extern "C" {

int diskann_hip_available(void) {
    try {
        return device_ok() ? 1 : 0;
    } catch (...) {
        return 0;
    }
}

int diskann_hip_batch_distances(const float *query, const float *candidates, int n, int dim, int metric,
                                float *out_distances) {
    if (n <= 0 || dim <= 0 || !query || !candidates || !out_distances) return -1;
    if (metric != kL2 && metric != kIP) return -1;
    try {
        if (!device_ok()) return -1;
        ThreadCtx &t = t_ctx;
        t.init();
        const size_t qb = (size_t)dim * 4, cb = (size_t)n * dim * 4, ob = (size_t)n * 4;
        if (cb <= kZeroCopyMax) {
            // small calls (the per-step shapes of metal_ffi.rs): stage into this thread's pinned buffers
            // and let the kernel read / write them over PCIe — no DMA round trips (the reference's
            // zero-copy wrap of page-aligned buffers, metal_diskann_bridge.mm:182-222)
            t.hq.ensure(qb);
            t.hc.ensure(cb);
            t.hout.ensure(ob);
            std::memcpy(t.hq.p, query, qb);
            std::memcpy(t.hc.p, candidates, cb);
            void *dq = nullptr, *dc = nullptr, *dout = nullptr;
            HIPANN_CHECK(hipHostGetDevicePointer(&dq, t.hq.p, 0));
            HIPANN_CHECK(hipHostGetDevicePointer(&dc, t.hc.p, 0));
            HIPANN_CHECK(hipHostGetDevicePointer(&dout, t.hout.p, 0));
            launch_rows(static_cast<const float *>(dq), static_cast<const float *>(dc), nullptr, n, dim, metric,
                        static_cast<float *>(dout), t.stream);
            HIPANN_CHECK(hipStreamSynchronize(t.stream));
            std::memcpy(out_distances, t.hout.p, ob);
            return 0;
        }
        t.q.ensure(qb, t.device);
        t.c.ensure(cb, t.device);
        t.out.ensure(ob, t.device);
        HIPANN_CHECK(hipMemcpyAsync(t.q.p, query, qb, hipMemcpyHostToDevice, t.stream));
        HIPANN_CHECK(hipMemcpyAsync(t.c.p, candidates, cb, hipMemcpyHostToDevice, t.stream));
        launch_rows(t.q.get<float>(), t.c.get<float>(), nullptr, n, dim, metric, t.out.get<float>(), t.stream);
        HIPANN_CHECK(hipMemcpyAsync(out_distances, t.out.p, ob, hipMemcpyDeviceToHost, t.stream));
        HIPANN_CHECK(hipStreamSynchronize(t.stream));
        return 0;
    } catch (...) {
        return -1;
    }
}

int diskann_hip_multi_batch_distances(const float *queries, const float *candidates, const unsigned int *query_map,
                                      int total_n, int nq, int dim, int metric, float *out_distances) {
    if (total_n <= 0 || nq <= 0 || dim <= 0 || !queries || !candidates || !query_map || !out_distances) return -1;
    if (metric != kL2 && metric != kIP) return -1;
    for (int i = 0; i < total_n; ++i)
        if (query_map[i] >= (unsigned)nq) return -1;
    try {
        if (!device_ok()) return -1;
        ThreadCtx &t = t_ctx;
        t.init();
        const size_t qb = (size_t)nq * dim * 4, cb = (size_t)total_n * dim * 4, mb = (size_t)total_n * 4;
        t.q.ensure(qb, t.device);
        t.c.ensure(cb, t.device);
        t.m.ensure(mb, t.device);
        t.out.ensure(mb, t.device);
        HIPANN_CHECK(hipMemcpyAsync(t.q.p, queries, qb, hipMemcpyHostToDevice, t.stream));
        HIPANN_CHECK(hipMemcpyAsync(t.c.p, candidates, cb, hipMemcpyHostToDevice, t.stream));
        HIPANN_CHECK(hipMemcpyAsync(t.m.p, query_map, mb, hipMemcpyHostToDevice, t.stream));
        launch_rows(t.q.get<float>(), t.c.get<float>(), t.m.get<unsigned>(), total_n, dim, metric, t.out.get<float>(),
                    t.stream);
        HIPANN_CHECK(hipMemcpyAsync(out_distances, t.out.p, mb, hipMemcpyDeviceToHost, t.stream));
        HIPANN_CHECK(hipStreamSynchronize(t.stream));
        return 0;
    } catch (...) {
        return -1;
    }
}

// Drop-in aliases of the reference symbol names (metal_diskann_bridge.h:8-23).
int diskann_metal_available(void) { return diskann_hip_available(); }
int diskann_metal_batch_distances(const float *query, const float *candidates, int n, int dim, int metric,
                                  float *out_distances) {
    return diskann_hip_batch_distances(query, candidates, n, dim, metric, out_distances);
}
int diskann_metal_multi_batch_distances(const float *queries, const float *candidates, const unsigned int *query_map,
                                        int total_n, int nq, int dim, int metric, float *out_distances) {
    return diskann_hip_multi_batch_distances(queries, candidates, query_map, total_n, nq, dim, metric, out_distances);
}

void *diskann_hip_register_db(const void *data, int64_t n, int dim, int fmt, const float *sq8_min,
                              const float *sq8_scale) {
    try {
        if (!device_ok() || n < 0 || dim <= 0 || (n > 0 && !data)) return nullptr;
        if (fmt != DISKANN_HIP_FMT_F32 && fmt != DISKANN_HIP_FMT_SQ8) return nullptr;
        if (fmt == DISKANN_HIP_FMT_SQ8 && (!sq8_min || !sq8_scale)) return nullptr;
        auto db = std::make_unique<DiskDB>();
        HIPANN_CHECK(hipGetDevice(&db->device));
        HIPANN_CHECK(hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking));
        db->n = n;
        db->dim = dim;
        db->fmt = fmt;
        const size_t bytes = (size_t)n * dim * (fmt == DISKANN_HIP_FMT_F32 ? 4 : 1);
        db->data.ensure(bytes + 16, db->device);
        if (bytes) HIPANN_CHECK(hipMemcpyAsync(db->data.p, data, bytes, hipMemcpyHostToDevice, db->stream));
        if (fmt == DISKANN_HIP_FMT_SQ8) sq8_fill_decode_tables(*db, sq8_min, sq8_scale, db->stream);
        HIPANN_CHECK(hipStreamSynchronize(db->stream));
        return db.release();
    } catch (...) {
        return nullptr;
    }
}

int diskann_hip_multi_batch_distances_ids(void *h, const float *queries, int nq, const unsigned int *ids,
                                          const unsigned int *query_map, int total_n, int metric, float *out) {
    if (!h || !queries || nq <= 0 || total_n < 0 || (total_n > 0 && (!ids || !query_map || !out))) return -1;
    if (metric != kL2 && metric != kIP) return -1;
    auto *db = static_cast<DiskDB *>(h);
    for (int i = 0; i < total_n; ++i)
        if (query_map[i] >= (unsigned)nq || ids[i] >= (uint64_t)db->n) return -1;
    if (total_n == 0) return 0;
    try {
        std::lock_guard<std::mutex> lk(db->mu);
        DeviceGuard g(db->device);
        const size_t qb = (size_t)nq * db->dim * 4, mb = (size_t)total_n * 4;
        db->q.ensure(qb + 16, db->device);
        db->ids.ensure(mb, db->device);
        db->m.ensure(mb, db->device);
        db->out.ensure(mb, db->device);
        HIPANN_CHECK(hipMemcpyAsync(db->q.p, queries, qb, hipMemcpyHostToDevice, db->stream));
        HIPANN_CHECK(hipMemcpyAsync(db->ids.p, ids, mb, hipMemcpyHostToDevice, db->stream));
        HIPANN_CHECK(hipMemcpyAsync(db->m.p, query_map, mb, hipMemcpyHostToDevice, db->stream));
        launch_ids(*db, db->q.get<float>(), db->ids.get<unsigned>(), db->m.get<unsigned>(), total_n, metric,
                   db->out.get<float>(), db->stream);
        HIPANN_CHECK(hipMemcpyAsync(out, db->out.p, mb, hipMemcpyDeviceToHost, db->stream));
        HIPANN_CHECK(hipStreamSynchronize(db->stream));
        return 0;
    } catch (...) {
        return -1;
    }
}

int diskann_hip_multi_batch_distances_ids_device(void *h, const float *queries_dev, int nq, const unsigned int *ids_dev,
                                                 const unsigned int *query_map_dev, int total_n, int metric,
                                                 float *out_dev, void *stream) {
    if (!h || !queries_dev || nq <= 0 || total_n < 0) return -1;
    if (metric != kL2 && metric != kIP) return -1;
    auto *db = static_cast<DiskDB *>(h);
    try {
        DeviceGuard g(db->device);
        hipStream_t st = static_cast<hipStream_t>(stream);  // NULL = the default (null) stream
        ScopedTiming tm(db->timer, st);
        launch_ids(*db, queries_dev, ids_dev, query_map_dev, total_n, metric, out_dev, st);
        return 0;
    } catch (...) {
        return -1;
    }
}

int64_t diskann_hip_db_size(void *h) { return h ? static_cast<DiskDB *>(h)->n : -1; }

// the metric of the graph the handle builds and maintains (build_shape_check of diskann_graph.cpp reads it)
int diskann_hip_set_graph_metric(void *h, int metric, char *eb, int el) {
    return abi_call(eb, el, [&] {
        HIPANN_REQUIRE(h, "set_graph_metric: null db");
        HIPANN_REQUIRE(metric == kL2 || metric == kIP, "set_graph_metric: metric must be 0 (L2) or 1 (IP)");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        db->graph_metric = metric;
        return 0;
    });
}

int diskann_hip_graph_metric(void *h) {
    if (!h) return -1;
    auto *db = static_cast<DiskDB *>(h);
    std::lock_guard<std::mutex> lk(db->mu);
    return db->graph_metric;
}

int diskann_hip_set_kernel_timing(void *h, int on) {
    if (!h) return -1;
    auto *db = static_cast<DiskDB *>(h);
    try {
        std::lock_guard<std::mutex> lk(db->mu);
        db->timer.reset(on != 0, db->device);
        return 0;
    } catch (...) {
        return -1;
    }
}

int diskann_hip_kernel_stats(void *h, double *total_ms, int64_t *launches) {
    if (!h || !total_ms || !launches) return -1;
    auto *db = static_cast<DiskDB *>(h);
    try {
        std::lock_guard<std::mutex> lk(db->mu);
        DeviceGuard g(db->device);
        *launches = (int64_t)db->timer.used;
        *total_ms = db->timer.average_ms() * (double)db->timer.used;
        return 0;
    } catch (...) {
        return -1;
    }
}

void diskann_hip_release_db(void *h) {
    if (!h) return;
    try {
        delete static_cast<DiskDB *>(h);
    } catch (...) {
    }
}

// Lock-step multi-query BFS over an HBM-resident DB (DiskProvider::search_batch semantics, with the
// per-step distance work on the GPU via the id-gather kernel).  adjacency: N × R u32 (u32::MAX pads),
// entry points as in the .diskann header.  Outputs nq × k (ids −1 / dist FLT_MAX past the result).
// stats: [0] distance evaluations, [1] lock-step iterations, [2] GPU calls, [3] reserved.
int diskann_hip_search_batch(void *h, const uint32_t *adj, int R, const uint32_t *eps, int n_ep, const float *queries,
                             int nq, int k, int l_search, int metric, int64_t *out_ids, float *out_d, int64_t *stats,
                             char *eb, int el) {
    return abi_call(eb, el, [&] {
        HIPANN_REQUIRE(h && adj && eps && queries && out_ids && out_d, "null argument");
        HIPANN_REQUIRE(R > 0 && nq >= 0 && k > 0, "bad arguments");
        HIPANN_REQUIRE(metric == kL2 || metric == kIP, "metric must be 0 or 1");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        DeviceGuard g(db->device);
        RoctxRange rr("hipann.diskann.host_bfs");
        host_bfs(db, adj, R, eps, n_ep, queries, nq, k, l_search, metric, out_ids, out_d, stats);
        return 0;
    });
}

int diskann_hip_register_graph(void *h, const uint32_t *adj, int R) {
    if (!h || !adj || R <= 0) return -1;
    auto *db = static_cast<DiskDB *>(h);
    try {
        std::lock_guard<std::mutex> lk(db->mu);
        DeviceGuard g(db->device);
        const size_t cnt = (size_t)db->n * R;
        db->adj_host.assign(adj, adj + cnt);
        db->adj_host_stale = false;
        db->adj_dev.ensure(cnt * 4 + 16, db->device);
        if (cnt) HIPANN_CHECK(hipMemcpyAsync(db->adj_dev.p, adj, cnt * 4, hipMemcpyHostToDevice, db->stream));
        // rows with a repeated id (the traversal's first-occurrence dedupe runs only on those)
        if (R <= 64) {  // (wider graphs run on the host BFS)
            db->dupw.ensure((size_t)((db->n + 31) / 32) * 4 + 16, db->device);
            launch_diskann_dup_rows(db->adj_dev.get<uint32_t>(), R, db->n, db->dupw.get<uint32_t>(), db->stream);
        } else {
            db->dupw.release();
        }
        HIPANN_CHECK(hipStreamSynchronize(db->stream));
        db->R = R;
        return 0;
    } catch (...) {
        return -1;
    }
}

int diskann_hip_search_batch_resident_device(void *h, const uint32_t *eps, int n_ep, const float *queries_dev, int nq,
                                             int k, int l_search, int metric, int64_t *out_ids_dev,
                                             float *out_d_dev, int64_t *stats, void *stream, char *eb, int el) {
    RoctxRange r_all("hipann.diskann.resident");
    return abi_call(eb, el, [&] {
        HIPANN_REQUIRE(h && (n_ep == 0 || eps) && (nq == 0 || (queries_dev && out_ids_dev && out_d_dev)),
                       "null argument");
        HIPANN_REQUIRE(nq >= 0 && k > 0 && n_ep >= 0, "bad arguments");
        HIPANN_REQUIRE(metric == kL2 || metric == kIP, "metric must be 0 or 1");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        HIPANN_REQUIRE(db->R > 0, "no graph registered (diskann_hip_register_graph)");
        DeviceGuard g(db->device);
        const hipStream_t st = stream ? static_cast<hipStream_t>(stream) : db->stream;
        resident_search_locked(db, eps, n_ep, queries_dev, nq, k, l_search, metric, out_ids_dev, out_d_dev, stats, st);
        return 0;
    });
}

int diskann_hip_search_batch_resident(void *h, const uint32_t *eps, int n_ep, const float *queries, int nq, int k,
                                      int l_search, int metric, int64_t *out_ids, float *out_d, int64_t *stats,
                                      char *eb, int el) {
    return abi_call(eb, el, [&] {
        HIPANN_REQUIRE(h && (nq == 0 || (queries && out_ids && out_d)), "null argument");
        HIPANN_REQUIRE(nq >= 0 && k > 0, "bad arguments");
        auto *db = static_cast<DiskDB *>(h);
        DevBuf q, oi, od;
        int dev;
        {
            std::lock_guard<std::mutex> lk(db->mu);
            dev = db->device;
        }
        DeviceGuard g(dev);
        const size_t qb = (size_t)std::max(nq, 1) * db->dim * 4, ob = (size_t)std::max(nq, 1) * k;
        q.ensure(qb, dev);
        oi.ensure(ob * 8, dev);
        od.ensure(ob * 4, dev);
        hipStream_t st;
        HIPANN_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        struct SG { hipStream_t s; ~SG() { (void)hipStreamDestroy(s); } } sg{st};
        if (nq) HIPANN_CHECK(hipMemcpyAsync(q.p, queries, (size_t)nq * db->dim * 4, hipMemcpyHostToDevice, st));
        const int rc = diskann_hip_search_batch_resident_device(h, eps, n_ep, q.get<float>(), nq, k, l_search, metric,
                                                                oi.get<int64_t>(), od.get<float>(), stats, st, eb, el);
        if (rc != 0) return rc;
        if (nq) {
            HIPANN_CHECK(hipMemcpyAsync(out_ids, oi.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, st));
            HIPANN_CHECK(hipMemcpyAsync(out_d, od.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
        }
        HIPANN_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}

}  // extern "C"
