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
// metal_diskann_bridge.mm:52-53), a registry of HBM databases, and diskann_hip_search_batch — the
// lock-step best-first BFS of DiskProvider::search_batch (disk_provider.rs:470-652) whose per-step
// distances go through the id-gather kernel.
#include "../../include/hip_diskann_bridge.h"
#include "common.hpp"
#include "runtime.hpp"

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cstring>
#include <atomic>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>

namespace hipann {

bool diskann_bfs_supported(int d, int fmt, int R, int n_ep, int L, uint32_t N);
void launch_diskann_dup_rows(const uint32_t *adj, int R, int64_t n, uint32_t *dupw, hipStream_t st);
void launch_diskann_bfs(const float *Q, int nq, int d, int fmt, const void *data, const float2 *ab,
                        const uint32_t *adj, const uint32_t *dupw, int R, uint32_t N, const uint32_t *eps, int n_ep, int k, int L,
                        int metric, uint32_t *visited, int64_t vwords, int64_t *out_ids, float *out_d, int *flags,
                        unsigned long long *stats, hipStream_t st);
// diskann_build.hip
int vamana_prune_blocks(int64_t m);
size_t vamana_gram_bytes(int blocks);
void launch_vamana_prune(const float *x, int d, uint32_t n, const uint32_t *targets, int m, const int *m_ptr,
                         const uint32_t *pool32, const int64_t *pool64, const float *pool_d, const int *pool_beg,
                         const int *pool_len, int pool_cap, int R, float alpha, uint32_t *out, bool out_by_target,
                         float *gram, int blocks, unsigned long long *counters, hipStream_t st);
void launch_vamana_fill_targets(uint32_t *tg, int b, uint32_t o0, uint32_t ep, hipStream_t st);
void launch_vamana_backedges(uint32_t *adj, int R, const uint32_t *tg, int b, int *cnt, int *slot, uint32_t *touched,
                             int *off, int *fill, uint32_t *src, int *ctr, uint32_t *pool, uint32_t *ptgt, int *pbeg,
                             int *plen, hipStream_t st);
// diskann_add.hip
void launch_vamana_batch_mates(const float *xb, int b, int d, uint32_t row0, int T, float *nrm, uint32_t *out,
                               unsigned long long *written, hipStream_t st);
void launch_vamana_concat_pool(const int64_t *sid, int K, const uint32_t *mates, int T, int b, uint32_t *pool,
                               int *pbeg, int *plen, hipStream_t st);
void launch_vamana_check_finite(const float *x, int64_t count, int *flag, hipStream_t st);
// diskann_remove.hip
int64_t diskann_remove_scan_blocks(int64_t n);
void launch_diskann_remove_mark(const int64_t *labels, int64_t m, int64_t n, uint32_t *bits, uint32_t *wpre,
                                uint32_t *sums, hipStream_t st);
void launch_diskann_remove_sources(const uint32_t *bits, const uint32_t *wpre, int64_t n, int64_t *src, hipStream_t st);
void launch_diskann_remove_pool_len(const uint32_t *adj, int R, int64_t n, const uint32_t *bits, uint8_t *nrem,
                                    hipStream_t st);
void launch_diskann_remove_pool_fill(const uint32_t *adj, int R, int64_t n, const uint32_t *bits,
                                     const uint32_t *targets, const int *pbeg, const int *plen, int cnt, uint32_t *pool,
                                     unsigned long long *gathered, hipStream_t st);
void launch_diskann_remove_nearest(const float *x, int d, int64_t n, const uint32_t *bits, uint32_t ep,
                                   unsigned long long *best, hipStream_t st);
void launch_diskann_remove_compact_adj(const uint32_t *adj, int R, int64_t n, const uint32_t *bits,
                                       const uint32_t *wpre, uint32_t *out, hipStream_t st);

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
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
    const float *q = queries + (int64_t)qi * d;
    const float *c = cands + w * (int64_t)d;
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
    s = wave_sum(s);
    if (lane == 0) out[w] = IP ? -s : s;
}

// The host BFS's visited sets on the device (vbits != nullptr): one bit per (query, row), vwords words per query.
// A candidate whose bit was already set (an earlier step of its query, or an earlier slot of the same step) is not
// evaluated: its output is kVisitedBits, a NaN payload no distance arithmetic produces.
constexpr unsigned kVisitedBits = 0x7fc0deadu;
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
    const float *q = queries + (int64_t)qmap[w] * d;
    const float *c = db + (int64_t)id * d;
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
    s = wave_sum(s);
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
                                                    int64_t vwords, unsigned *__restrict__ done_ctr,
                                                    unsigned *__restrict__ done_tok, unsigned token) {
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
    // done_tok (the host BFS): the launch posts its own completion — every wave's distances (pinned host memory, device
    // mapping) made visible system-wide, the block counted, and the last block to finish writes `token` into the
    // host word the BFS polls — instead of an event recorded behind every step's launch (MI355X_MICROARCH.md,
    // inter-workgroup visibility: release, then the count; the compiler-hazard waits made explicit)
    if (done_tok) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __threadfence_system();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned old = __hip_atomic_fetch_add(done_ctr, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if (old == gridDim.x - 1) {
                __hip_atomic_store(done_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next launch
                __threadfence_system();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(done_tok, token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
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

struct DiskDB {
    int device = 0;
    int64_t n = 0;
    int dim = 0;
    int fmt = DISKANN_HIP_FMT_F32;
    DevBuf data;  // fp32 rows or u8 codes
    DevBuf ab;    // float2 per dim (SQ8): (scale/255, min), the traversal's fused decode
    DevBuf ab_raw;  // float2 per dim (SQ8): (scale, min), the id-gather kernels' exact decode
    hipStream_t stream = nullptr;
    std::mutex mu;
    DevBuf q, ids, m, out;
    HostBuf hids, hm, hout;
    KernelTimer timer;
    // resident graph + BFS scratch (diskann_hip_register_graph / _search_batch_resident)
    int R = 0;
    DevBuf adj_dev, dupw, visited, flags, bstats, eps_dev;
    DevBuf vbits;  // host BFS: the queries' visited bits on the device (one bit per row and query)
    DevBuf bfs_ctr;   // host BFS: per group, the id-gather launch's finished-block count (zero between launches)
    HostBuf bfs_tok;  // host BFS: per group, the token word the launch posts when it is done (polled)
    unsigned bfs_seq = 0;
    std::vector<uint32_t> adj_host;
    // diskann_hip_build_graph: adj_dev is ahead of adj_host (the resident search refreshes the host copy before it
    // re-runs a flagged query on it); the last build's seconds in search / out-edge prunes / back-edges
    bool adj_host_stale = false;
    double build_s[3] = {0.0, 0.0, 0.0};
    double remove_s[3] = {0.0, 0.0, 0.0};  // the last diskann_hip_remove_ids: pool build, prune, compact
    double add_s[4] = {0.0, 0.0, 0.0, 0.0};  // the last diskann_hip_add_rows: searches, mates, out-edge prunes, back-edges
    ~DiskDB() {
        if (stream) { DeviceGuard g(device); (void)hipStreamDestroy(stream); }
    }
};

// Whether launch_ids posts its own completion token for this DB (the SQ8 vector kernel).
bool ids_post_token(const DiskDB &db, const float *q) {
    return db.fmt != DISKANN_HIP_FMT_F32 && db.dim % 16 == 0 && db.dim <= 2048 && (uintptr_t)q % 16 == 0;
}

void launch_ids(DiskDB &db, const float *q, const unsigned *ids, const unsigned *m, int total_n, int metric,
                float *out, hipStream_t st, unsigned *vbits = nullptr, int64_t vwords = 0, unsigned *done_ctr = nullptr,
                unsigned *done_tok = nullptr, unsigned token = 0) {
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
            if (metric == kIP) hipLaunchKernelGGL(dist_ids_sq8<true>, grid, block, smem, st, q, x, ab, ids, m, total_n, d, db.n, out, vbits, vwords, done_ctr, done_tok, token);
            else hipLaunchKernelGGL(dist_ids_sq8<false>, grid, block, smem, st, q, x, ab, ids, m, total_n, d, db.n, out, vbits, vwords, done_ctr, done_tok, token);
        } else {
            dim3 grid((unsigned)ceil_div(total_n, 4)), block(256);
            if (metric == kIP) hipLaunchKernelGGL(dist_ids_sq8_scalar<true>, grid, block, 0, st, q, x, ab, ids, m, total_n, d, db.n, out, vbits, vwords);
            else hipLaunchKernelGGL(dist_ids_sq8_scalar<false>, grid, block, 0, st, q, x, ab, ids, m, total_n, d, db.n, out, vbits, vwords);
        }
    }
    HIPANN_CHECK(hipGetLastError());
}

void set_err(char *buf, int len, const char *msg) {
    if (!buf || len <= 0) return;
    std::strncpy(buf, msg, (size_t)len - 1);
    buf[len - 1] = '\0';
}

// ---- lock-step BFS (DiskProvider::search_batch, disk_provider.rs:470-652) ----
struct Cand {
    float d;
    uint32_t id;
};
struct CandGreater {  // min-heap on (d, id): BinaryHeap<Reverse<(FloatOrd, u32)>>
    bool operator()(const Cand &a, const Cand &b) const { return a.d > b.d || (a.d == b.d && a.id > b.id); }
};

// Rust slice::binary_search_by (std ≥ 1.82) with partial_cmp on distance; returns the insert position.
size_t rust_binary_search(const std::vector<Cand> &res, float dist) {
    size_t size = res.size();
    if (size == 0) return 0;
    size_t base = 0;
    while (size > 1) {
        const size_t half = size / 2, mid = base + half;
        base = (res[mid].d > dist) ? base : mid;
        size -= half;
    }
    const float p = res[base].d;
    if (!(p < dist) && !(p > dist)) return base;
    return base + (p < dist ? 1 : 0);
}

// Visited set: open addressing over u32 ids (linear probing, power-of-two capacity, load ≤ 1/2).
// Same membership semantics as the reference's hashbrown::HashSet<u32>; only speed differs.
struct VisitedSet {
    std::vector<uint32_t> slot;  // kEmpty = unused
    uint32_t mask = 0;
    size_t count = 0;
    static constexpr uint32_t kEmpty = 0xffffffffu;
    void init(size_t expect) {
        size_t cap = 64;
        while (cap < 2 * expect) cap <<= 1;
        slot.assign(cap, kEmpty);
        mask = (uint32_t)(cap - 1);
        count = 0;
    }
    static uint32_t hash(uint32_t v) { return (v * 0x9E3779B1u) ^ (v >> 15); }
    void prefetch(uint32_t v) const { __builtin_prefetch(slot.data() + (hash(v) & mask), 1); }
    // Returns true if v was newly inserted (HashSet::insert).  v == kEmpty is stored out of band.
    bool insert(uint32_t v) {
        if (v == kEmpty) {
            const bool fresh = !has_max;
            has_max = true;
            return fresh;
        }
        if (2 * (count + 1) > slot.size()) grow();
        uint32_t i = hash(v) & mask;
        for (;;) {
            const uint32_t x = slot[i];
            if (x == v) return false;
            if (x == kEmpty) { slot[i] = v; ++count; return true; }
            i = (i + 1) & mask;
        }
    }
    bool has_max = false;

  private:
    void grow() {
        std::vector<uint32_t> old;
        old.swap(slot);
        slot.assign(old.size() * 2, kEmpty);
        mask = (uint32_t)(slot.size() - 1);
        for (uint32_t v : old) {
            if (v == kEmpty) continue;
            uint32_t i = hash(v) & mask;
            while (slot[i] != kEmpty) i = (i + 1) & mask;
            slot[i] = v;
        }
    }
};

struct QState {
    VisitedSet visited;
    std::vector<Cand> cands;  // binary min-heap on (d, id) (CandGreater): BinaryHeap<Reverse<..>>
    std::vector<Cand> result;  // sorted by d, at most l entries
    bool active = true;
    int nnew = 0;  // candidates this query put into the current lock-step batch
};

// insert_result (disk_provider.rs:656-678).  (d, id) pairs in `cands` are unique (ids pass the
// visited set once), so any binary heap pops them in the same order as Rust's BinaryHeap.
void insert_result(QState &s, size_t l, float dist, uint32_t nb) {
    if (s.result.size() < l || dist < s.result.back().d) {
        const size_t pos = rust_binary_search(s.result, dist);
        s.result.insert(s.result.begin() + (ptrdiff_t)pos, Cand{dist, nb});
        if (s.result.size() > l) s.result.resize(l);
        s.cands.push_back(Cand{dist, nb});
        std::push_heap(s.cands.begin(), s.cands.end(), CandGreater());
    }
}

// Fork-join pool for the per-step host phases of the lock-step BFS: the calling thread is worker 0,
// the others spin on a generation counter (the phases are ~0.1 ms apart, too short for a futex
// round trip) and exit when the search returns.
class SpinPool {
  public:
    explicit SpinPool(int nthreads) : n_(nthreads < 1 ? 1 : nthreads) {
        for (int t = 1; t < n_; ++t) th_.emplace_back([this, t] { worker(t); });
    }
    ~SpinPool() {
        stop_.store(true, std::memory_order_release);
        gen_.fetch_add(1, std::memory_order_acq_rel);
        for (auto &t : th_) t.join();
    }
    int size() const { return n_; }
    // Runs fn(tid) on every worker and returns when all have finished.  Exceptions must not escape fn.
    template <typename F> void run(F &&fn) {
        if (n_ == 1) { fn(0); return; }
        std::function<void(int)> job(fn);
        job_ = &job;
        pending_.store(n_ - 1, std::memory_order_release);
        gen_.fetch_add(1, std::memory_order_acq_rel);
        fn(0);
        while (pending_.load(std::memory_order_acquire) != 0) spin_pause();
        job_ = nullptr;
    }

  private:
    static void spin_pause() { __builtin_ia32_pause(); }
    void worker(int tid) {
        uint64_t seen = 0;
        for (;;) {
            uint64_t g;
            int idle = 0;
            while ((g = gen_.load(std::memory_order_acquire)) == seen) {
                spin_pause();
                if (++idle > 4096) { std::this_thread::yield(); idle = 0; }
            }
            seen = g;
            if (stop_.load(std::memory_order_acquire)) return;
            (*job_)(tid);
            pending_.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
    int n_;
    std::vector<std::thread> th_;
    std::atomic<uint64_t> gen_{0};
    std::atomic<int> pending_{0};
    std::atomic<bool> stop_{false};
    std::function<void(int)> *job_ = nullptr;
};

int bfs_threads(int nq) {
    int t = 16;  // the GPU box's CPU share per GPU
    if (const char *e = std::getenv("HIPANN_BFS_THREADS")) t = std::atoi(e);
    const int hw = (int)std::thread::hardware_concurrency();
    if (hw > 0) t = std::min(t, hw);
    t = std::min(t, std::max(1, nq / 16));  // ≥ 16 queries per thread
    return std::max(1, t);
}

int bfs_groups(int nq) {
    // two pipelined groups: the GPU gathers one group's distances while the host threads run the other's inserts and
    // expansions (C4 host path, 16 threads: 1 group 34.8K QPS with 9.6 ms of GPU waits per batch, 2 groups 39.9K with
    // 0.5 ms, profiles/r05/diskann_host_bfs_r05.txt); HIPANN_BFS_GROUPS=1..8 for A/B
    int g = 2;
    if (const char *e = std::getenv("HIPANN_BFS_GROUPS")) g = std::atoi(e);
    g = std::min(g, std::max(1, nq / 64));  // ≥ 64 queries per group
    return std::max(1, std::min(g, 8));
}

// Host-driven lock-step BFS (the reference's structure: host state, one id-gather launch per step).
// Caller holds db.mu and the device.  Also the fallback of the resident path for flagged queries.
//
// The queries run in G groups (2 by default), each its own lock-step loop, pipelined: while the GPU gathers group
// g's distances, the host threads insert and expand group g+1's.  A query's trajectory depends only on its own
// state, so grouping changes no result; the batch's step count (the reference's loop iterations) is the largest
// group's.
void host_bfs(DiskDB *db, const uint32_t *adj, int R, const uint32_t *eps, int n_ep, const float *queries, int nq,
              int k, int l_search, int metric, int64_t *out_ids, float *out_d, int64_t *stats) {
    const uint32_t N = (uint32_t)db->n;
    const int dim = db->dim;
    int64_t nevals = 0, nsteps = 0, ncalls = 0;
    if (nq == 0) {
        if (stats) { stats[0] = stats[1] = stats[2] = stats[3] = 0; }
        return;
    }
    const size_t l = (size_t)std::max(l_search, k);
    const hipStream_t st = db->stream;
    // Fixed per-query slot layout: query qi owns slots [qi*S, qi*S + S) of every lock-step batch,
    // S = max(R, n_ep); unused slots hold UINT32_MAX and the kernel skips them.  The query map is
    // therefore constant (uploaded once) and the host phases run per query in parallel with no
    // compaction step.  Per query the candidate order is the reference's (neighbour order).
    const size_t S = (size_t)std::max(R, n_ep);
    const size_t cap = (size_t)nq * S;
    HIPANN_REQUIRE(cap <= (size_t)INT32_MAX, "nq * max(R, n_ep) exceeds INT32_MAX");
    db->q.ensure((size_t)nq * dim * 4 + 16, db->device);
    HIPANN_CHECK(hipMemcpyAsync(db->q.p, queries, (size_t)nq * dim * 4, hipMemcpyHostToDevice, st));
    db->ids.ensure(cap * 4, db->device);
    db->m.ensure(cap * 4, db->device);
    db->out.ensure(cap * 4, db->device);
    db->hids.ensure(cap * 4);
    db->hm.ensure(cap * 4);
    db->hout.ensure(cap * 4);
    uint32_t *hid = db->hids.get<uint32_t>();
    uint32_t *hm = db->hm.get<uint32_t>();
    float *hout = db->hout.get<float>();
    float *hout_dev = static_cast<float *>(host_device_ptr(hout));
    // HIPANN_BFS_ZC_IDS=0 (A/B): the step's ids copied to the device before each gather instead of read in place
    static const bool zc_ids = [] { const char *e = std::getenv("HIPANN_BFS_ZC_IDS"); return !e || std::atoi(e); }();
    const unsigned *hid_dev = static_cast<const unsigned *>(host_device_ptr(hid));
    for (size_t i = 0; i < cap; ++i) hm[i] = (uint32_t)(i / S);
    HIPANN_CHECK(hipMemcpyAsync(db->m.p, hm, cap * 4, hipMemcpyHostToDevice, st));
    std::vector<QState> Sq((size_t)nq);
    // The visited sets live on the device (default): the id-gather kernel sets each candidate's bit and skips the ones
    // already set, so the host phases never probe a per-query hash set (≈ 6K ids, 32-64 KB per query: a cache miss
    // per neighbour).  The host hands over every valid neighbour of the expanded row; an already-visited one comes
    // back as kVisitedBits and is dropped.  HIPANN_BFS_GPU_VISITED=0 (A/B), or more than 1 GiB of bits: the host sets.
    static const bool gv_env = [] { const char *e = std::getenv("HIPANN_BFS_GPU_VISITED"); return !e || std::atoi(e); }();
    const int64_t vwords = ((int64_t)N + 31) / 32;
    const bool gv = gv_env && (int64_t)nq * vwords * 4 <= ((int64_t)1 << 30);
    if (gv) {
        db->vbits.ensure((size_t)nq * vwords * 4, db->device);
        HIPANN_CHECK(hipMemsetAsync(db->vbits.p, 0, (size_t)nq * vwords * 4, st));
    }
    unsigned *vbits = gv ? db->vbits.get<unsigned>() : nullptr;
    auto visited_mark = [](float v) { return __builtin_bit_cast(uint32_t, v) == kVisitedBits; };
    SpinPool pool(bfs_threads(nq));
    const int T = pool.size();
    struct Group {
        int q0 = 0, q1 = 0;
        bool seed = true, done = false, launched = false;
        int64_t steps = 0;
        hipEvent_t ev = nullptr;
        unsigned token = 0;  // the token its last launch posts (tokened launches)
    };
    const int G = bfs_groups(nq);
    // HIPANN_BFS_TOKEN=1 (A/B, measured and rejected in r06): the SQ8 gather posts its own completion (a token word per
    // group in coherent pinned memory, written by the launch's last block) instead of an event recorded behind every
    // step's launch.  Every block must release its distance writes at system scope before it is counted — an L2
    // write-back per block, 2048 per launch — and the C4 host path fell from 71K to 15K QPS (same box, alternating).
    static const bool tok_env = [] { const char *e = std::getenv("HIPANN_BFS_TOKEN"); return e && std::atoi(e); }();
    const bool tok = tok_env && ids_post_token(*db, db->q.get<float>());
    if (tok) {
        if (!db->bfs_ctr.p || db->bfs_ctr.bytes < sizeof(unsigned) * 8) {
            db->bfs_ctr.ensure(sizeof(unsigned) * 8, db->device);
            HIPANN_CHECK(hipMemsetAsync(db->bfs_ctr.p, 0, db->bfs_ctr.bytes, st));
        }
        // coherent pinned memory: the launch's system-scope token store is visible to the polling host at once (the
        // default non-coherent allocation held it back until the stream's end-of-kernel release: 5x slower batches)
        if (db->bfs_tok.ensure(sizeof(unsigned) * 8, hipHostMallocCoherent))
            std::memset(db->bfs_tok.p, 0, sizeof(unsigned) * 8);
    }
    unsigned *tok_dev = tok ? static_cast<unsigned *>(host_device_ptr(db->bfs_tok.p)) : nullptr;
    const volatile unsigned *tok_host = tok ? db->bfs_tok.get<unsigned>() : nullptr;
    std::vector<Group> grp((size_t)G);
    for (int g = 0; g < G; ++g) {
        grp[g].q0 = (int)((int64_t)nq * g / G);
        grp[g].q1 = (int)((int64_t)nq * (g + 1) / G);
        HIPANN_CHECK(hipEventCreateWithFlags(&grp[g].ev, hipEventDisableTiming));
    }
    struct EvFree {
        std::vector<Group> &g;
        ~EvFree() { for (auto &x : g) if (x.ev) (void)hipEventDestroy(x.ev); }
    } ev_free{grp};
    // the group's slots with work (up to its last query with new candidates) through the id-gather kernel
    auto launch = [&](Group &g) {
        int last = g.q0;
        int64_t tot = 0;
        for (int qi = g.q0; qi < g.q1; ++qi)
            if (Sq[qi].nnew) { last = qi + 1; tot += Sq[qi].nnew; }
        g.launched = tot > 0;
        if (!tot) return;
        const size_t o = (size_t)g.q0 * S, span = (size_t)(last - g.q0) * S;
        // zc_ids: the kernel reads the step's ids straight from the pinned host buffer (its device mapping) instead of
        // a host-to-device copy ahead of it (a DMA operation the kernel waits behind, per step)
        if (!zc_ids)
            HIPANN_CHECK(hipMemcpyAsync(db->ids.get<unsigned>() + o, hid + o, span * 4, hipMemcpyHostToDevice, st));
        {
            // the distances go straight into the pinned host buffer through its device mapping (posted writes: no
            // device-to-host copy and its round trip per step)
            ScopedTiming tm(db->timer, st);
            const int gi = (int)(&g - grp.data());
            if (tok) g.token = ++db->bfs_seq == 0 ? ++db->bfs_seq : db->bfs_seq;  // never 0 (the words start at 0)
            launch_ids(*db, db->q.get<float>(), (zc_ids ? hid_dev : db->ids.get<unsigned>()) + o,
                       db->m.get<unsigned>() + o, (int)span, metric, hout_dev + o, st, vbits, vwords,
                       tok ? db->bfs_ctr.get<unsigned>() + gi : nullptr, tok ? tok_dev + gi : nullptr, g.token);
        }
        if (!tok) HIPANN_CHECK(hipEventRecord(g.ev, st));
        ncalls++;
        if (!gv) nevals += tot;  // (gv: the first visits, counted as the phases read them)
    };
    // seed entry points (disk_provider.rs:524-538)
    pool.run([&](int t) {
        const int q0 = (int)((int64_t)nq * t / T), q1 = (int)((int64_t)nq * (t + 1) / T);
        for (int qi = q0; qi < q1; ++qi) {
            QState &s = Sq[qi];
            if (!gv) s.visited.init(std::max<size_t>(l * 2, 1024));
            s.cands.reserve(l * 2);
            s.result.reserve(l + 1);
            uint32_t *slot = hid + (size_t)qi * S;
            int cnt = 0;
            for (int e = 0; e < n_ep; ++e) {
                const uint32_t ep = eps[e];
                if (gv ? ep < N : (s.visited.insert(ep) && ep < N)) slot[cnt++] = ep;
            }
            for (size_t j = (size_t)cnt; j < S; ++j) slot[j] = 0xffffffffu;
            s.nnew = cnt;
        }
    });
    for (auto &g : grp) launch(g);
    // One host phase of a group: the results of its last GPU call (the seeds' into cands + result; later steps'
    // through insert_result), then the loop head (disk_provider.rs:545-652): pop, stop rule, expansion.
    // Returns the loop-head active count.
    std::vector<int64_t> red((size_t)T * 8, 0);  // per-thread head counts, padded against false sharing
    // HIPANN_BFS_CHUNK (A/B): queries per work item taken from a shared counter (default 0: a static 1/T range per
    // thread — measured r05: 8-query chunks 27.6 ms of phases per batch against 19.7 static, 2-query chunks 38 ms: a
    // query's state stays in one core's caches only when the same thread keeps it)
    static const int chunk = [] { const char *e = std::getenv("HIPANN_BFS_CHUNK"); return e ? std::atoi(e) : 0; }();
    std::atomic<int> next_q{0};
    auto phase = [&](Group &g) {
        const int n = g.q1 - g.q0;
        const bool seed = g.seed;
        next_q.store(g.q0, std::memory_order_relaxed);
        pool.run([&](int t) {
            int64_t head = 0, evals = 0;
            int q0, q1;
            if (chunk > 0) {
                q0 = next_q.fetch_add(chunk, std::memory_order_relaxed);
                q1 = std::min(q0 + chunk, g.q1);
            } else {
                q0 = g.q0 + (int)((int64_t)n * t / T);
                q1 = g.q0 + (int)((int64_t)n * (t + 1) / T);
            }
            for (; q0 < g.q1; ) {
            for (int qi = q0; qi < q1; ++qi) {
                QState &s = Sq[qi];
                uint32_t *slot = hid + (size_t)qi * S;
                const float *dd = hout + (size_t)qi * S;
                if (seed) {
                    for (int j = 0; j < s.nnew; ++j) {
                        if (gv && visited_mark(dd[j])) continue;  // a repeated entry point
                        ++evals;
                        s.cands.push_back(Cand{dd[j], slot[j]});
                        std::push_heap(s.cands.begin(), s.cands.end(), CandGreater());
                        s.result.push_back(Cand{dd[j], slot[j]});
                    }
                    std::stable_sort(s.result.begin(), s.result.end(),
                                     [](const Cand &x, const Cand &y) { return x.d < y.d; });
                } else {
                    for (int j = 0; j < s.nnew; ++j) {
                        if (gv && visited_mark(dd[j])) continue;
                        ++evals;
                        insert_result(s, l, dd[j], slot[j]);
                    }
                }
                const int prev = s.nnew;  // slots >= prev are already empty
                s.nnew = 0;
                head += s.active ? 1 : 0;  // the reference's loop-head active count
                if (s.active) {
                    if (s.cands.empty()) {
                        s.active = false;
                    } else {
                        std::pop_heap(s.cands.begin(), s.cands.end(), CandGreater());
                        const Cand c = s.cands.back();
                        s.cands.pop_back();
                        if (s.result.size() >= l && c.d > s.result[l - 1].d) {
                            s.active = false;
                        } else {
                            const uint32_t *nbr = adj + (size_t)c.id * R;
                            if (gv) {  // every valid neighbour: the device keeps the visited sets
                                int cnt = 0;
                                for (int r = 0; r < R; ++r) {
                                    const uint32_t nb = nbr[r];
                                    if (nb == 0xffffffffu) break;  // get_neighbors trims at the first sentinel
                                    if (nb < N) slot[cnt++] = nb;
                                }
                                s.nnew = cnt;
                            } else {
                            // the row's valid neighbours first, with their visited-set slots prefetched: the set
                            // (≈ 6K ids, 32-64 KB per query) misses cache on nearly every probe, and 64 overlapped
                            // misses cost about one
                            uint32_t nv[256];
                            int cnt = 0;
                            bool end = false;
                            for (int r0 = 0; r0 < R && !end; r0 += 256) {  // (rows wider than 256 in pieces)
                                int m = 0;
                                for (int r = r0; r < R && r < r0 + 256; ++r) {
                                    const uint32_t nb = nbr[r];
                                    if (nb == 0xffffffffu) {  // get_neighbors trims at the first sentinel
                                        end = true;
                                        break;
                                    }
                                    if (nb >= N) continue;
                                    nv[m++] = nb;
                                    s.visited.prefetch(nb);
                                }
                                for (int j = 0; j < m; ++j)
                                    if (s.visited.insert(nv[j])) slot[cnt++] = nv[j];
                            }
                            s.nnew = cnt;
                            }
                        }
                    }
                }
                for (int j = s.nnew; j < prev; ++j) slot[j] = 0xffffffffu;
                // the adjacency row the next pop most likely takes (the heap's top now; the next step's inserts rarely
                // change it), into cache while the GPU computes this step's distances
                if (s.active && !s.cands.empty()) __builtin_prefetch(adj + (size_t)s.cands.front().id * R);
            }
            if (chunk <= 0) break;
            q0 = next_q.fetch_add(chunk, std::memory_order_relaxed);
            q1 = std::min(q0 + chunk, g.q1);
            }
            red[(size_t)t * 8] = head;
            red[(size_t)t * 8 + 1] = evals;
        });
        g.seed = false;
        int64_t head = 0;
        for (int t = 0; t < T; ++t) {
            head += red[(size_t)t * 8];
            if (gv) nevals += red[(size_t)t * 8 + 1];
        }
        return head;
    };
    // HIPANN_BFS_PROF=1 (tuning): host time in the GPU waits, the host phases and the launches, on stderr
    static const bool prof = std::getenv("HIPANN_BFS_PROF") != nullptr;
    using clk = std::chrono::steady_clock;
    double t_wait = 0, t_phase = 0, t_launch = 0;
    auto since = [](clk::time_point a) { return std::chrono::duration<double, std::micro>(clk::now() - a).count(); };
    const auto t_all = clk::now();
    for (int live = G; live > 0;) {
        for (auto &g : grp) {
            if (g.done) continue;
            auto t0 = clk::now();
            if (g.launched) {
                if (tok) wait_posted(tok_host + (&g - grp.data()), g.token, st);
                else wait_event(g.ev);
            }
            auto t1 = clk::now();
            const int64_t head = phase(g);
            auto t2 = clk::now();
            if (prof) {
                t_wait += std::chrono::duration<double, std::micro>(t1 - t0).count();
                t_phase += std::chrono::duration<double, std::micro>(t2 - t1).count();
            }
            if (!head) {
                g.done = true;
                --live;
                continue;
            }
            g.steps++;
            launch(g);  // (nothing when no query of the group expanded new neighbours)
            if (prof) t_launch += since(t2);
        }
    }
    if (prof)
        std::fprintf(stderr, "hipann bfs: nq %d groups %d threads %d calls %lld: total %.0f us, waits %.0f, phases %.0f, "
                             "launches %.0f\n", nq, G, T, (long long)ncalls, since(t_all), t_wait, t_phase, t_launch);
    for (auto &g : grp) nsteps = std::max(nsteps, g.steps);
    for (int qi = 0; qi < nq; ++qi) {
        const auto &r = Sq[qi].result;
        for (int j = 0; j < k; ++j) {
            if ((size_t)j < r.size()) {
                out_ids[(size_t)qi * k + j] = r[j].id;
                out_d[(size_t)qi * k + j] = r[j].d;
            } else {
                out_ids[(size_t)qi * k + j] = -1;
                out_d[(size_t)qi * k + j] = FLT_MAX;
            }
        }
    }
    if (stats) { stats[0] = nevals; stats[1] = nsteps; stats[2] = ncalls; stats[3] = 0; }
}

}  // namespace
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
        if (fmt == DISKANN_HIP_FMT_SQ8) {
            // ab: (scale/255, min) for the traversal's fused form; ab_raw: (scale, min) for the id-gather
            // kernels' exact decode
            std::vector<float> ab((size_t)dim * 2), abr((size_t)dim * 2);
            for (int j = 0; j < dim; ++j) {
                ab[2 * j] = sq8_scale[j] / 255.0f;
                ab[2 * j + 1] = sq8_min[j];
                abr[2 * j] = sq8_scale[j];
                abr[2 * j + 1] = sq8_min[j];
            }
            db->ab.ensure(ab.size() * 4, db->device);
            db->ab_raw.ensure(abr.size() * 4, db->device);
            HIPANN_CHECK(hipMemcpyAsync(db->ab.p, ab.data(), ab.size() * 4, hipMemcpyHostToDevice, db->stream));
            HIPANN_CHECK(hipMemcpyAsync(db->ab_raw.p, abr.data(), abr.size() * 4, hipMemcpyHostToDevice, db->stream));
        }
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
    try {
        HIPANN_REQUIRE(h && adj && eps && queries && out_ids && out_d, "null argument");
        HIPANN_REQUIRE(R > 0 && nq >= 0 && k > 0, "bad arguments");
        HIPANN_REQUIRE(metric == kL2 || metric == kIP, "metric must be 0 or 1");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        DeviceGuard g(db->device);
        RoctxRange rr("hipann.diskann.host_bfs");
        host_bfs(db, adj, R, eps, n_ep, queries, nq, k, l_search, metric, out_ids, out_d, stats);
        return 0;
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return -1;
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

// Resident search: queries / outputs in HBM, asynchronous launch on `stream`, then a wait for the
// per-query flags (the rare flagged queries and unsupported shapes go through host_bfs).
// (the caller holds db->mu and the device; the graph build searches its own frozen graph through this)
static void resident_search_locked(DiskDB *db, const uint32_t *eps, int n_ep, const float *queries_dev, int nq, int k,
                                   int l_search, int metric, int64_t *out_ids_dev, float *out_d_dev, int64_t *stats,
                                   hipStream_t st) {
    {
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
            db->bstats.ensure(80, db->device);
            db->eps_dev.ensure((size_t)std::max(n_ep, 1) * 4, db->device);
            if (n_ep) HIPANN_CHECK(hipMemcpyAsync(db->eps_dev.p, eps, (size_t)n_ep * 4, hipMemcpyHostToDevice, st));
            HIPANN_CHECK(hipMemsetAsync(db->bstats.p, 0, 80, st));
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
            unsigned long long hs[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            HIPANN_CHECK(hipMemcpyAsync(flags.data(), db->flags.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
            HIPANN_CHECK(hipMemcpyAsync(hs, db->bstats.p, 80, hipMemcpyDeviceToHost, st));
            HIPANN_CHECK(hipStreamSynchronize(st));
            if (hs[3] + hs[4] + hs[5] + hs[6] + hs[7] + hs[8]) {  // tuning builds (HIPANN_BFS_PROF)
                const double st = (double)std::max<unsigned long long>(hs[2], 1);
                std::fprintf(stderr,
                             "[bfs-prof] wave-0 cycles per step: select %.0f adjacency %.0f dedupe %.0f visited %.0f "
                             "dist %.0f insert %.0f; speculated rows used %.3f\n",
                             hs[3] / st, hs[4] / st, hs[5] / st, hs[6] / st, hs[7] / st, hs[8] / st, hs[9] / st);
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
}

int diskann_hip_search_batch_resident_device(void *h, const uint32_t *eps, int n_ep, const float *queries_dev, int nq,
                                             int k, int l_search, int metric, int64_t *out_ids_dev,
                                             float *out_d_dev, int64_t *stats, void *stream, char *eb, int el) {
    RoctxRange r_all("hipann.diskann.resident");
    try {
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
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return -1;
}

int diskann_hip_search_batch_resident(void *h, const uint32_t *eps, int n_ep, const float *queries, int nq, int k,
                                      int l_search, int metric, int64_t *out_ids, float *out_d, int64_t *stats,
                                      char *eb, int el) {
    try {
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
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return -1;
}

// ---- graph build on the device (kernels in diskann_build.hip) ----
static void swap_buf(DevBuf &a, DevBuf &b) {
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
    std::swap(a.device, b.device);
}

// the shapes the build entry points and remove_ids refuse (a message, never a slow path); `who` names the call
static void build_shape_check(const DiskDB *db, int R, float alpha, int metric, const char *who = "graph build") {
    const std::string w = std::string(who) + ": ";
    HIPANN_REQUIRE(metric != kIP, w + "IP is not supported (the crate prunes IP by a different rule)");
    HIPANN_REQUIRE(metric == kL2, w + "metric must be 0 (L2)");
    HIPANN_REQUIRE(db->fmt == DISKANN_HIP_FMT_F32, w + "an fp32 DB is required (SQ8 is not supported)");
    HIPANN_REQUIRE(R >= 1 && R <= 64, w + "R must be in [1, 64]");
    HIPANN_REQUIRE(db->dim % 4 == 0 && db->dim <= 2048, w + "d must be a multiple of 4 and at most 2048");
    HIPANN_REQUIRE(db->n < ((int64_t)1 << 31), w + "n must be below 2^31");
    HIPANN_REQUIRE(alpha >= 1.0f, w + "alpha must be >= 1");  // (a NaN fails the comparison)
}

// the host copy of the adjacency brought level with the device's (the caller holds db->mu and the device)
static void refresh_adj_host(DiskDB *db, hipStream_t st) {
    db->adj_host.resize((size_t)db->n * db->R);
    HIPANN_CHECK(hipMemcpyAsync(db->adj_host.data(), db->adj_dev.p, db->adj_host.size() * 4, hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));
    db->adj_host_stale = false;
}

// rows a walk from entry_point over the host adjacency does not reach (rows end at the first UINT32_MAX)
static int64_t unreached_rows(const std::vector<uint32_t> &a, int64_t n, int R, uint32_t entry_point) {
    std::vector<uint8_t> seen((size_t)n, 0);
    std::vector<uint32_t> stack{entry_point};
    seen[entry_point] = 1;
    int64_t reached = 1;
    while (!stack.empty()) {
        const uint32_t v = stack.back();
        stack.pop_back();
        for (int r = 0; r < R; ++r) {
            const uint32_t w = a[(size_t)v * R + r];
            if (w == 0xffffffffu) break;
            if (w < (uint64_t)n && !seen[w]) { seen[w] = 1; ++reached; stack.push_back(w); }
        }
    }
    return n - reached;
}

int diskann_hip_build_graph(void *h, int R, int l_build, float alpha, int metric, uint32_t entry_point, int batch_max,
                            uint32_t *adjacency_out, int64_t *stats, char *eb, int el) {
    try {
        HIPANN_REQUIRE(h, "graph build: null db");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        build_shape_check(db, R, alpha, metric);
        HIPANN_REQUIRE(l_build >= 1 && l_build <= 256, "graph build: L must be in [1, 256]");
        HIPANN_REQUIRE(batch_max >= 1, "graph build: batch_max must be >= 1");
        HIPANN_REQUIRE((int64_t)entry_point < db->n, "graph build: entry_point must be below n");
        DeviceGuard g(db->device);
        RoctxRange rr("hipann.diskann.build_graph");
        const hipStream_t st = db->stream;
        const int64_t n = db->n;
        const int d = db->dim, dev = db->device;
        int64_t s8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        // The graph under construction sits in the DB's own graph slots (the traversal reads them); the slots' former
        // contents come back if the build fails.  No built row repeats an id, so dupw stays zero.
        DevBuf nadj, ndupw;
        std::vector<uint32_t> nhost;
        int nR = R;
        nadj.ensure((size_t)n * R * 4 + 16, dev);
        ndupw.ensure((size_t)((n + 31) / 32) * 4 + 16, dev);
        HIPANN_CHECK(hipMemsetAsync(nadj.p, 0xff, (size_t)n * R * 4, st));
        HIPANN_CHECK(hipMemsetAsync(ndupw.p, 0, (size_t)((n + 31) / 32) * 4, st));
        struct Slots {
            DiskDB *db;
            DevBuf &a, &w;
            std::vector<uint32_t> &hst;
            int &R;
            bool keep = false;
            bool stale0;  // whether the former graph's host copy was behind its device copy (after add_rows)
            void exchange() {
                swap_buf(db->adj_dev, a);
                swap_buf(db->dupw, w);
                db->adj_host.swap(hst);
                std::swap(db->R, R);
            }
            ~Slots() {
                if (!keep) exchange();
                db->adj_host_stale = keep ? false : stale0;
            }
        } slots{db, nadj, ndupw, nhost, nR, false, db->adj_host_stale};
        slots.exchange();
        db->adj_host_stale = false;
        double secs[3] = {0.0, 0.0, 0.0};
        using clk = std::chrono::steady_clock;
        auto since = [](clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); };
        if (n > 1) {
            const uint32_t ep = entry_point;
            const int K = (int)std::min<int64_t>(l_build, n);
            const int bmax = (int)std::min<int64_t>(batch_max, n - 1);
            const int64_t pairs = (int64_t)bmax * R;
            const int64_t rows_max = std::min<int64_t>(pairs, n);  // rows one batch's back-edges can touch
            const int64_t pool_words = rows_max * R + pairs;
            HIPANN_REQUIRE(pairs < INT32_MAX && pool_words < INT32_MAX, "graph build: batch_max too large");
            // scratch, once per build
            DevBuf sid, sd, tg, cnt, slot, touched, off, fill, src, pool, ptgt, pbeg, plen, ctr, pctr, gram;
            sid.ensure((size_t)bmax * K * 8, dev);
            sd.ensure((size_t)bmax * K * 4, dev);
            tg.ensure((size_t)bmax * 4, dev);
            cnt.ensure((size_t)n * 4, dev);
            slot.ensure((size_t)n * 4, dev);
            touched.ensure((size_t)pairs * 4, dev);
            off.ensure((size_t)pairs * 4, dev);
            fill.ensure((size_t)pairs * 4, dev);
            src.ensure((size_t)pairs * 4, dev);
            pool.ensure((size_t)pool_words * 4, dev);
            ptgt.ensure((size_t)rows_max * 4, dev);
            pbeg.ensure((size_t)rows_max * 4, dev);
            plen.ensure((size_t)rows_max * 4, dev);
            ctr.ensure(16, dev);
            pctr.ensure(32, dev);
            const int blocks = vamana_prune_blocks(std::max<int64_t>(bmax, rows_max));
            gram.ensure(vamana_gram_bytes(blocks), dev);
            HIPANN_CHECK(hipMemsetAsync(pctr.p, 0, 32, st));
            const float *x = db->data.get<float>();
            uint32_t *adj = db->adj_dev.get<uint32_t>();
            const uint32_t eps1[1] = {ep};
            int64_t o0 = 0;  // rows inserted so far in insertion order (row order, the entry point left out)
            while (o0 < n - 1) {
                const int b = (int)std::min<int64_t>(std::min<int64_t>(bmax, std::max<int64_t>(1, o0 + 1)), n - 1 - o0);
                const int64_t o1 = o0 + b;
                // 1. search the frozen graph: the batch's rows are contiguous but for the entry point's gap
                auto t0 = clk::now();
                const int64_t seg[2][2] = {{o0, std::min<int64_t>(o1, ep)}, {std::max<int64_t>(o0, ep), o1}};
                for (int sgi = 0; sgi < 2; ++sgi) {
                    const int64_t oa = seg[sgi][0], ob = seg[sgi][1];
                    if (ob <= oa) continue;
                    const int64_t row0 = sgi == 0 ? oa : oa + 1;
                    int64_t sst[4] = {0, 0, 0, 0};
                    resident_search_locked(db, eps1, 1, x + row0 * d, (int)(ob - oa), K, l_build, kL2,
                                           sid.get<int64_t>() + (oa - o0) * K, sd.get<float>() + (oa - o0) * K, sst, st);
                    s8[0] += sst[0];
                    s8[4] += sst[3];
                }
                secs[0] += since(t0);
                // 2. out-edges: N(p) = prune(p, the traversal's list)
                auto t1 = clk::now();
                launch_vamana_fill_targets(tg.get<uint32_t>(), b, (uint32_t)o0, ep, st);
                launch_vamana_prune(x, d, (uint32_t)n, tg.get<uint32_t>(), b, nullptr, nullptr, sid.get<int64_t>(),
                                    sd.get<float>(), nullptr, nullptr, K, R, alpha, adj, true, gram.get<float>(), blocks,
                                    pctr.get<unsigned long long>() + 2, st);
                HIPANN_CHECK(hipStreamSynchronize(st));
                secs[1] += since(t1);
                // 3. back-edges, grouped per target row on the device; rows that overflow are pruned
                auto t2 = clk::now();
                HIPANN_CHECK(hipMemsetAsync(cnt.p, 0, (size_t)n * 4, st));
                HIPANN_CHECK(hipMemsetAsync(ctr.p, 0, 16, st));
                launch_vamana_backedges(adj, R, tg.get<uint32_t>(), b, cnt.get<int>(), slot.get<int>(),
                                        touched.get<uint32_t>(), off.get<int>(), fill.get<int>(), src.get<uint32_t>(),
                                        ctr.get<int>(), pool.get<uint32_t>(), ptgt.get<uint32_t>(), pbeg.get<int>(),
                                        plen.get<int>(), st);
                launch_vamana_prune(x, d, (uint32_t)n, ptgt.get<uint32_t>(), (int)std::min<int64_t>((int64_t)b * R, n),
                                    ctr.get<int>() + 3, pool.get<uint32_t>(), nullptr, nullptr, pbeg.get<int>(),
                                    plen.get<int>(), 0, R, alpha, adj, true, gram.get<float>(), blocks,
                                    pctr.get<unsigned long long>(), st);
                HIPANN_CHECK(hipStreamSynchronize(st));
                secs[2] += since(t2);
                db->adj_host_stale = true;
                s8[1] += 1;
                s8[2] += b;
                o0 = o1;
            }
            unsigned long long pc[4] = {0, 0, 0, 0};
            HIPANN_CHECK(hipMemcpyAsync(pc, pctr.p, 32, hipMemcpyDeviceToHost, st));
            HIPANN_CHECK(hipStreamSynchronize(st));
            s8[3] = (int64_t)pc[0];
            s8[5] = (int64_t)(pc[1] + pc[3]);
        }
        // registered as after diskann_hip_register_graph: the host copy and the repeated-id row bits
        launch_diskann_dup_rows(db->adj_dev.get<uint32_t>(), R, n, db->dupw.get<uint32_t>(), st);
        db->adj_host.resize((size_t)n * R);
        HIPANN_CHECK(hipMemcpyAsync(db->adj_host.data(), db->adj_dev.p, (size_t)n * R * 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        s8[6] = unreached_rows(db->adj_host, n, R, entry_point);
        if (adjacency_out) std::memcpy(adjacency_out, db->adj_host.data(), (size_t)n * R * 4);
        if (stats) std::memcpy(stats, s8, sizeof(s8));
        for (int i = 0; i < 3; ++i) db->build_s[i] = secs[i];
        slots.keep = true;
        return 0;
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return -1;
}

int diskann_hip_build_phase_seconds(void *h, double *seconds) {
    if (!h || !seconds) return -1;
    auto *db = static_cast<DiskDB *>(h);
    std::lock_guard<std::mutex> lk(db->mu);
    for (int i = 0; i < 3; ++i) seconds[i] = db->build_s[i];
    return 0;
}

// ---- row insertion into the device graph (kernels in diskann_add.hip and diskann_build.hip) ----
// `buf` with room for `need` bytes and its first `keep` bytes preserved: in place when the capacity suffices, else
// a new buffer a quarter larger than the old one (at least `need`) in `grown`, for the caller to swap in.
static void *grow_keep(DevBuf &buf, DevBuf &grown, size_t need, size_t keep, int dev, hipStream_t st) {
    if (buf.p && need <= buf.bytes) return buf.p;
    grown.ensure(std::max(need, buf.bytes + buf.bytes / 4), dev);
    if (keep) HIPANN_CHECK(hipMemcpyAsync(grown.p, buf.p, keep, hipMemcpyDeviceToDevice, st));
    return grown.p;
}

int64_t diskann_hip_add_rows(void *h, const float *rows, int64_t m, int l_build, float alpha, int metric,
                             uint32_t entry_point, int batch_max, int batch_mates, uint32_t *adjacency_out,
                             int64_t *stats, char *eb, int el) {
    try {
        HIPANN_REQUIRE(h, "add_rows: null db");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        HIPANN_REQUIRE(db->R > 0, "add_rows: no graph registered (diskann_hip_register_graph / _build_graph)");
        build_shape_check(db, db->R, alpha, metric, "add_rows");
        HIPANN_REQUIRE(l_build >= 1 && l_build <= 256, "add_rows: L must be in [1, 256]");
        HIPANN_REQUIRE(batch_max >= 1, "add_rows: batch_max must be >= 1");
        HIPANN_REQUIRE(batch_mates >= 0 && batch_mates <= 64, "add_rows: batch_mates must be in [0, 64]");
        HIPANN_REQUIRE(l_build + batch_mates <= 512, "add_rows: L + batch_mates must be at most 512");
        HIPANN_REQUIRE((int64_t)entry_point < db->n, "add_rows: entry_point must be below n");
        HIPANN_REQUIRE(m >= 0 && (m == 0 || rows), "add_rows: null rows");
        HIPANN_REQUIRE(db->n + m < ((int64_t)1 << 31), "add_rows: n + m must be below 2^31");
        DeviceGuard g(db->device);
        const hipStream_t st = db->stream;
        const int64_t n0 = db->n, n1 = n0 + m;
        const int R = db->R, d = db->dim, dev = db->device, T = batch_mates, L = l_build;
        int64_t s8[8] = {0, 0, 0, 0, 0, 0, -1, 0};
        if (m == 0) {  // nothing moves
            if (adjacency_out) {
                if (db->adj_host_stale) refresh_adj_host(db, st);
                s8[6] = unreached_rows(db->adj_host, n0, R, entry_point);
                std::memcpy(adjacency_out, db->adj_host.data(), (size_t)n0 * R * 4);
            }
            if (stats) std::memcpy(stats, s8, sizeof(s8));
            return 0;
        }
        RoctxRange rr("hipann.diskann.add_rows");
        using clk = std::chrono::steady_clock;
        auto since = [](clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); };
        double secs[4] = {0.0, 0.0, 0.0, 0.0};
        const uint32_t ep = entry_point;

        // ---- everything that can refuse or allocate, before anything a search reads changes ----
        const int bmax = (int)std::min<int64_t>(batch_max, m);
        const int W = L + T;  // pool slots of an out-edge prune with mates
        const int64_t pairs = (int64_t)bmax * R;
        const int64_t rows_max = std::min<int64_t>(pairs, n1);  // rows one batch's back-edges can touch
        const int64_t pool_words = rows_max * R + pairs;
        HIPANN_REQUIRE(pairs < INT32_MAX && pool_words < INT32_MAX && (int64_t)bmax * W < INT32_MAX,
                       "add_rows: batch_max too large");
        DevBuf sid, sd, tg, cnt, slot, touched, off, fill, src, pool, ptgt, pbeg, plen, ctr, pctr, gram;
        DevBuf mates, nrm, opool, obeg, olen;
        sid.ensure((size_t)bmax * L * 8, dev);
        sd.ensure((size_t)bmax * L * 4, dev);
        tg.ensure((size_t)bmax * 4, dev);
        cnt.ensure((size_t)n1 * 4, dev);
        slot.ensure((size_t)n1 * 4, dev);
        touched.ensure((size_t)pairs * 4, dev);
        off.ensure((size_t)pairs * 4, dev);
        fill.ensure((size_t)pairs * 4, dev);
        src.ensure((size_t)pairs * 4, dev);
        pool.ensure((size_t)pool_words * 4, dev);
        ptgt.ensure((size_t)rows_max * 4, dev);
        pbeg.ensure((size_t)rows_max * 4, dev);
        plen.ensure((size_t)rows_max * 4, dev);
        ctr.ensure(16, dev);
        pctr.ensure(48, dev);  // [0..3] the prunes' counters, [4] mate ids written, [5] (int) the non-finite flag
        if (T > 0) {
            mates.ensure((size_t)bmax * T * 4, dev);
            nrm.ensure((size_t)bmax * 4, dev);
            opool.ensure((size_t)bmax * W * 4, dev);
            obeg.ensure((size_t)bmax * 4, dev);
            olen.ensure((size_t)bmax * 4, dev);
        }
        const int blocks = vamana_prune_blocks(std::max<int64_t>(bmax, rows_max));
        gram.ensure(vamana_gram_bytes(blocks), dev);
        {  // the traversal's own scratch at its largest (resident_search_locked sizes it the same way)
            const int64_t vwords = (n1 + 31) / 32;
            const int64_t per = std::max<int64_t>(1, std::min<int64_t>(bmax, ((int64_t)2 << 30) / (vwords * 4)));
            db->visited.ensure((size_t)per * vwords * 4, dev);
            db->flags.ensure((size_t)bmax * 4, dev);
            db->bstats.ensure(80, dev);
            db->eps_dev.ensure(4, dev);
        }
        db->adj_host.reserve((size_t)n1 * R);
        // rows, adjacency and repeated-id bits with room for n1 rows: in place, or grown copies swapped in below
        DevBuf gdata, gadj, gdupw;
        const size_t w0 = (size_t)((n0 + 31) / 32), w1 = (size_t)((n1 + 31) / 32);
        float *x = static_cast<float *>(grow_keep(db->data, gdata, (size_t)n1 * d * 4 + 16, (size_t)n0 * d * 4, dev, st));
        uint32_t *adj =
            static_cast<uint32_t *>(grow_keep(db->adj_dev, gadj, (size_t)n1 * R * 4 + 16, (size_t)n0 * R * 4, dev, st));
        uint32_t *dupw = static_cast<uint32_t *>(grow_keep(db->dupw, gdupw, w1 * 4 + 16, w0 * 4, dev, st));
        // the tails no search reads yet: the new rows, empty adjacency rows, clear bits (the bits past n0 in word
        // w0 − 1 are clear already)
        HIPANN_CHECK(hipMemcpyAsync(x + (size_t)n0 * d, rows, (size_t)m * d * 4, hipMemcpyHostToDevice, st));
        HIPANN_CHECK(hipMemsetAsync(adj + (size_t)n0 * R, 0xff, (size_t)m * R * 4, st));
        if (w1 > w0) HIPANN_CHECK(hipMemsetAsync(dupw + w0, 0, (w1 - w0) * 4, st));
        HIPANN_CHECK(hipMemsetAsync(pctr.p, 0, 48, st));
        launch_vamana_check_finite(x + (size_t)n0 * d, m * (int64_t)d, pctr.get<int>() + 10, st);
        int bad = 0;
        HIPANN_CHECK(hipMemcpyAsync(&bad, pctr.get<int>() + 10, 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        HIPANN_REQUIRE(!bad, "add_rows: rows hold a non-finite value");

        // ---- from here on the handle changes; a failure leaves it without a graph (it cannot be rolled back) ----
        struct Guard {
            DiskDB *db;
            int64_t n0;
            bool armed = true;
            ~Guard() {
                if (!armed) return;
                db->n = n0;
                db->R = 0;
                db->adj_host.clear();
                db->adj_host_stale = false;
            }
        } guard{db, n0};
        if (gdata.p) swap_buf(db->data, gdata);
        if (gadj.p) swap_buf(db->adj_dev, gadj);
        if (gdupw.p) swap_buf(db->dupw, gdupw);
        gdata.release();
        gadj.release();
        gdupw.release();
        const uint32_t eps1[1] = {ep};
        unsigned long long *pc64 = pctr.get<unsigned long long>();
        int64_t c = n0;  // rows in the graph
        while (c < n1) {
            const int b = (int)std::min<int64_t>(std::min<int64_t>(bmax, c), n1 - c);
            const int K = (int)std::min<int64_t>(L, c);
            db->n = c;  // the searches see the graph as it stands at the batch's start
            // 1. search
            auto t0 = clk::now();
            int64_t sst[4] = {0, 0, 0, 0};
            resident_search_locked(db, eps1, 1, x + (size_t)c * d, b, K, K, kL2, sid.get<int64_t>(), sd.get<float>(), sst,
                                   st);
            s8[0] += sst[0];
            s8[4] += sst[3];
            secs[0] += since(t0);
            // 2. mates
            const bool with_mates = T > 0 && b > 1;
            if (with_mates) {
                auto tm = clk::now();
                launch_vamana_batch_mates(x + (size_t)c * d, b, d, (uint32_t)c, T, nrm.get<float>(),
                                          mates.get<uint32_t>(), pc64 + 4, st);
                HIPANN_CHECK(hipStreamSynchronize(st));
                secs[1] += since(tm);
            }
            // 3. out-edges (the targets are rows c .. c + b − 1: insertion order c − 1 + i with the entry point below)
            auto t1 = clk::now();
            launch_vamana_fill_targets(tg.get<uint32_t>(), b, (uint32_t)(c - 1), ep, st);
            if (T == 0) {
                launch_vamana_prune(x, d, (uint32_t)(c + b), tg.get<uint32_t>(), b, nullptr, nullptr, sid.get<int64_t>(),
                                    sd.get<float>(), nullptr, nullptr, K, R, alpha, adj, true, gram.get<float>(), blocks,
                                    pc64 + 2, st);
            } else {
                launch_vamana_concat_pool(sid.get<int64_t>(), K, with_mates ? mates.get<uint32_t>() : nullptr, T, b,
                                          opool.get<uint32_t>(), obeg.get<int>(), olen.get<int>(), st);
                launch_vamana_prune(x, d, (uint32_t)(c + b), tg.get<uint32_t>(), b, nullptr, opool.get<uint32_t>(),
                                    nullptr, nullptr, obeg.get<int>(), olen.get<int>(), 0, R, alpha, adj, true,
                                    gram.get<float>(), blocks, pc64 + 2, st);
            }
            HIPANN_CHECK(hipStreamSynchronize(st));
            secs[2] += since(t1);
            // 4. back-edges (a target may be a batch row: the stream puts every read of the out-edges before be_merge)
            auto t2 = clk::now();
            HIPANN_CHECK(hipMemsetAsync(cnt.p, 0, (size_t)(c + b) * 4, st));
            HIPANN_CHECK(hipMemsetAsync(ctr.p, 0, 16, st));
            launch_vamana_backedges(adj, R, tg.get<uint32_t>(), b, cnt.get<int>(), slot.get<int>(),
                                    touched.get<uint32_t>(), off.get<int>(), fill.get<int>(), src.get<uint32_t>(),
                                    ctr.get<int>(), pool.get<uint32_t>(), ptgt.get<uint32_t>(), pbeg.get<int>(),
                                    plen.get<int>(), st);
            launch_vamana_prune(x, d, (uint32_t)(c + b), ptgt.get<uint32_t>(),
                                (int)std::min<int64_t>((int64_t)b * R, c + b), ctr.get<int>() + 3, pool.get<uint32_t>(),
                                nullptr, nullptr, pbeg.get<int>(), plen.get<int>(), 0, R, alpha, adj, true,
                                gram.get<float>(), blocks, pc64, st);
            HIPANN_CHECK(hipStreamSynchronize(st));
            secs[3] += since(t2);
            db->adj_host_stale = true;
            s8[1] += 1;
            s8[2] += b;
            c += b;
        }
        unsigned long long pc[5] = {0, 0, 0, 0, 0};
        HIPANN_CHECK(hipMemcpyAsync(pc, pctr.p, 40, hipMemcpyDeviceToHost, st));
        // the repeated-id row bits of all rows (one pass over the adjacency; no pruned or appended row repeats an id)
        launch_diskann_dup_rows(adj, R, n1, dupw, st);
        HIPANN_CHECK(hipStreamSynchronize(st));
        s8[3] = (int64_t)pc[0];
        s8[5] = (int64_t)(pc[1] + pc[3]);
        s8[7] = (int64_t)pc[4];
        db->adj_host.resize((size_t)n1 * R);  // (reserved above: cannot throw)
        db->n = n1;
        guard.armed = false;
        // the host copy stays behind (the next host re-run refreshes it) unless the caller wants the graph
        if (adjacency_out) {
            refresh_adj_host(db, st);
            s8[6] = unreached_rows(db->adj_host, n1, R, ep);
            std::memcpy(adjacency_out, db->adj_host.data(), (size_t)n1 * R * 4);
        }
        if (stats) std::memcpy(stats, s8, sizeof(s8));
        for (int i = 0; i < 4; ++i) db->add_s[i] = secs[i];
        return n1;
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return -1;
}

int diskann_hip_batch_mates(void *h, int64_t row0, int b, int T, uint32_t *out, char *eb, int el) {
    try {
        HIPANN_REQUIRE(h, "batch_mates: null db");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        build_shape_check(db, 1, 1.0f, kL2, "batch_mates");
        HIPANN_REQUIRE(T >= 1 && T <= 64, "batch_mates: T must be in [1, 64]");
        HIPANN_REQUIRE(row0 >= 0 && b >= 0 && row0 + b <= db->n, "batch_mates: rows out of range");
        HIPANN_REQUIRE(b == 0 || out, "batch_mates: null out");
        if (b == 0) return 0;
        DeviceGuard g(db->device);
        const hipStream_t st = db->stream;
        DevBuf nrm, od;
        nrm.ensure((size_t)b * 4, db->device);
        od.ensure((size_t)b * T * 4, db->device);
        launch_vamana_batch_mates(db->data.get<float>() + (size_t)row0 * db->dim, b, db->dim, (uint32_t)row0, T,
                                  nrm.get<float>(), od.get<uint32_t>(), nullptr, st);
        HIPANN_CHECK(hipMemcpyAsync(out, od.p, (size_t)b * T * 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        return 0;
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return -1;
}

int diskann_hip_add_phase_seconds(void *h, double *seconds) {
    if (!h || !seconds) return -1;
    auto *db = static_cast<DiskDB *>(h);
    std::lock_guard<std::mutex> lk(db->mu);
    for (int i = 0; i < 4; ++i) seconds[i] = db->add_s[i];
    return 0;
}

// ---- row removal from the device graph (kernels in diskann_remove.hip) ----
int64_t diskann_hip_remove_ids(void *h, const int64_t *labels, int64_t n_labels, float alpha, int metric,
                               uint32_t *entry_point, int64_t scratch_words, uint32_t *adjacency_out, int64_t *stats,
                               char *eb, int el) {
    try {
        HIPANN_REQUIRE(h, "remove_ids: null db");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        HIPANN_REQUIRE(db->R > 0, "remove_ids: no graph registered (diskann_hip_register_graph / _build_graph)");
        build_shape_check(db, db->R, alpha, metric, "remove_ids");
        HIPANN_REQUIRE(entry_point, "remove_ids: null entry_point");
        HIPANN_REQUIRE(n_labels >= 0 && (n_labels == 0 || labels) && scratch_words >= 0, "remove_ids: bad arguments");
        HIPANN_REQUIRE((int64_t)*entry_point < db->n, "remove_ids: entry_point must be below n");
        const int64_t n = db->n;
        const int R = db->R, d = db->dim, dev = db->device;
        const uint32_t ep = *entry_point;
        int64_t s8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        // D: the distinct labels in range
        std::vector<uint32_t> dead;
        for (int64_t i = 0; i < n_labels; ++i)
            if (labels[i] >= 0 && labels[i] < n) dead.push_back((uint32_t)labels[i]);
        std::sort(dead.begin(), dead.end());
        dead.erase(std::unique(dead.begin(), dead.end()), dead.end());
        const int64_t nd = (int64_t)dead.size(), n2 = n - nd;
        if (nd == 0) {  // nothing moves
            if (db->adj_host_stale) {  // (add_rows leaves the host copy behind)
                DeviceGuard g(db->device);
                refresh_adj_host(db, db->stream);
            }
            s8[6] = unreached_rows(db->adj_host, n, R, ep);
            if (adjacency_out) std::memcpy(adjacency_out, db->adj_host.data(), (size_t)n * R * 4);
            if (stats) std::memcpy(stats, s8, sizeof(s8));
            return 0;
        }
        HIPANN_REQUIRE(n2 > 0, "remove_ids: every row would be removed");
        DeviceGuard g(db->device);
        RoctxRange rr("hipann.diskann.remove_ids");
        const hipStream_t st = db->stream;
        using clk = std::chrono::steady_clock;
        auto since = [](clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); };
        double secs[3] = {0.0, 0.0, 0.0};
        KernelTimer fill_ev, prune_ev;  // device time of the slabs' pool fills and prunes (read after the last sync)
        fill_ev.reset(true, db->device);
        prune_ev.reset(true, db->device);
        const auto t_call = clk::now();
        const float *x = db->data.get<float>();
        const uint32_t *adj = db->adj_dev.get<uint32_t>();

        // 1. mark, rank, and every live row's count of removed neighbours
        auto t0 = clk::now();
        const int64_t words = (n + 31) / 32;
        DevBuf lab, bits, wpre, sums, nrem, radj, ctr;
        lab.ensure((size_t)n_labels * 8, dev);
        bits.ensure((size_t)words * 4, dev);
        wpre.ensure((size_t)words * 4, dev);
        sums.ensure((size_t)diskann_remove_scan_blocks(n) * 4, dev);
        nrem.ensure((size_t)n, dev);
        radj.ensure((size_t)n * R * 4 + 16, dev);
        ctr.ensure(32, dev);
        HIPANN_CHECK(hipMemcpyAsync(lab.p, labels, (size_t)n_labels * 8, hipMemcpyHostToDevice, st));
        launch_diskann_remove_mark(lab.get<int64_t>(), n_labels, n, bits.get<uint32_t>(), wpre.get<uint32_t>(),
                                   sums.get<uint32_t>(), st);
        launch_diskann_remove_pool_len(adj, R, n, bits.get<uint32_t>(), nrem.get<uint8_t>(), st);
        // the repaired graph in the old id space: the stored rows, the pruned ones written over them
        HIPANN_CHECK(hipMemcpyAsync(radj.p, adj, (size_t)n * R * 4, hipMemcpyDeviceToDevice, st));
        HIPANN_CHECK(hipMemsetAsync(ctr.p, 0, 32, st));
        std::vector<uint8_t> hrem((size_t)n);
        HIPANN_CHECK(hipMemcpyAsync(hrem.data(), nrem.p, (size_t)n, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        // slabs of affected rows whose pool slots fit the budget (a row over the budget takes a slab alone)
        const int64_t budget = std::min<int64_t>(scratch_words > 0 ? scratch_words : (int64_t)1 << 28, 0x7fff0000);
        std::vector<uint32_t> tg;
        std::vector<int> pbeg, plen;
        std::vector<int64_t> slab_at{0};
        int64_t used = 0, pool_words = 0, slab_rows = 0;
        for (int64_t p = 0; p < n; ++p) {
            if (!hrem[p]) continue;
            const int len = R * (1 + (int)hrem[p]);
            if (used > 0 && used + len > budget) {
                slab_at.push_back((int64_t)tg.size());
                used = 0;
            }
            tg.push_back((uint32_t)p);
            pbeg.push_back((int)used);
            plen.push_back(len);
            used += len;
            pool_words = std::max(pool_words, used);
        }
        slab_at.push_back((int64_t)tg.size());
        const int64_t na = (int64_t)tg.size();
        for (size_t s = 0; s + 1 < slab_at.size(); ++s) slab_rows = std::max(slab_rows, slab_at[s + 1] - slab_at[s]);
        secs[0] += since(t0);
        if (na > 0) {
            DevBuf dtg, dbeg, dlen, pool, gram;
            dtg.ensure((size_t)na * 4, dev);
            dbeg.ensure((size_t)na * 4, dev);
            dlen.ensure((size_t)na * 4, dev);
            pool.ensure((size_t)pool_words * 4, dev);
            const int blocks = vamana_prune_blocks(slab_rows);
            gram.ensure(vamana_gram_bytes(blocks), dev);
            HIPANN_CHECK(hipMemcpyAsync(dtg.p, tg.data(), (size_t)na * 4, hipMemcpyHostToDevice, st));
            HIPANN_CHECK(hipMemcpyAsync(dbeg.p, pbeg.data(), (size_t)na * 4, hipMemcpyHostToDevice, st));
            HIPANN_CHECK(hipMemcpyAsync(dlen.p, plen.data(), (size_t)na * 4, hipMemcpyHostToDevice, st));
            unsigned long long *c64 = ctr.get<unsigned long long>();
            // the stream orders fill, prune and the next slab's reuse of `pool`; events split the device time
            for (size_t s = 0; s + 1 < slab_at.size(); ++s) {
                const int64_t a0 = slab_at[s];
                const int cnt = (int)(slab_at[s + 1] - a0);
                if (cnt <= 0) continue;
                {
                    ScopedTiming tm(fill_ev, st);
                    launch_diskann_remove_pool_fill(adj, R, n, bits.get<uint32_t>(), dtg.get<uint32_t>() + a0,
                                                    dbeg.get<int>() + a0, dlen.get<int>() + a0, cnt,
                                                    pool.get<uint32_t>(), c64 + 2, st);
                }
                {
                    ScopedTiming tm(prune_ev, st);
                    launch_vamana_prune(x, d, (uint32_t)n, dtg.get<uint32_t>() + a0, cnt, nullptr, pool.get<uint32_t>(),
                                        nullptr, nullptr, dbeg.get<int>() + a0, dlen.get<int>() + a0, 0, R, alpha,
                                        radj.get<uint32_t>(), true, gram.get<float>(), blocks, c64, st);
                }
                s8[4] += 1;
            }
        }
        // 2. the entry point: relabelled, or replaced by the nearest live row before the rows move
        uint32_t nep = ep;
        unsigned long long hc[4] = {0, 0, 0, ~0ull};
        if (std::binary_search(dead.begin(), dead.end(), ep)) {
            HIPANN_CHECK(hipMemsetAsync(ctr.get<unsigned long long>() + 3, 0xff, 8, st));
            launch_diskann_remove_nearest(x, d, n, bits.get<uint32_t>(), ep, ctr.get<unsigned long long>() + 3, st);
            s8[5] = 1;
        }
        // 3. compact into fresh buffers: rows, adjacency (ids replaced by their ranks), repeated-id row bits
        DevBuf src, nx, nadj, ndupw;
        std::vector<uint32_t> nhost((size_t)n2 * R);
        src.ensure((size_t)n2 * 8, dev);
        nx.ensure((size_t)n2 * d * 4 + 16, dev);
        nadj.ensure((size_t)n2 * R * 4 + 16, dev);
        ndupw.ensure((size_t)((n2 + 31) / 32) * 4 + 16, dev);
        launch_diskann_remove_sources(bits.get<uint32_t>(), wpre.get<uint32_t>(), n, src.get<int64_t>(), st);
        launch_flat_gather_rows(x, src.get<int64_t>(), n2, d, nx.get<float>(), st);
        launch_diskann_remove_compact_adj(radj.get<uint32_t>(), R, n, bits.get<uint32_t>(), wpre.get<uint32_t>(),
                                          nadj.get<uint32_t>(), st);
        launch_diskann_dup_rows(nadj.get<uint32_t>(), R, n2, ndupw.get<uint32_t>(), st);
        HIPANN_CHECK(hipMemcpyAsync(nhost.data(), nadj.p, (size_t)n2 * R * 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipMemcpyAsync(hc, ctr.p, 32, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        if (s8[5]) {
            HIPANN_REQUIRE(hc[3] != ~0ull, "remove_ids: no live row found for the entry point");
            nep = (uint32_t)(hc[3] & 0xffffffffull);
        }
        nep -= (uint32_t)(std::lower_bound(dead.begin(), dead.end(), nep) - dead.begin());
        s8[0] = nd;
        s8[1] = (int64_t)hc[0];
        s8[2] = (int64_t)hc[1];
        s8[3] = (int64_t)hc[2];
        s8[6] = unreached_rows(nhost, n2, R, nep);
        // phases: host time up to the slab plan plus the fills' device time; the prunes' device time; the rest
        secs[0] += fill_ev.average_ms() * (double)fill_ev.used * 1e-3;
        secs[1] = prune_ev.average_ms() * (double)prune_ev.used * 1e-3;
        secs[2] = std::max(0.0, since(t_call) - secs[0] - secs[1]);
        // everything is built: swap it in
        swap_buf(db->data, nx);
        swap_buf(db->adj_dev, nadj);
        swap_buf(db->dupw, ndupw);
        db->adj_host.swap(nhost);
        db->adj_host_stale = false;
        db->n = n2;
        *entry_point = nep;
        if (adjacency_out) std::memcpy(adjacency_out, db->adj_host.data(), (size_t)n2 * R * 4);
        if (stats) std::memcpy(stats, s8, sizeof(s8));
        for (int i = 0; i < 3; ++i) db->remove_s[i] = secs[i];
        return nd;
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return -1;
}

int diskann_hip_remove_phase_seconds(void *h, double *seconds) {
    if (!h || !seconds) return -1;
    auto *db = static_cast<DiskDB *>(h);
    std::lock_guard<std::mutex> lk(db->mu);
    for (int i = 0; i < 3; ++i) seconds[i] = db->remove_s[i];
    return 0;
}

int diskann_hip_robust_prune(void *h, const uint32_t *targets, int m, const uint32_t *pools, int pool_cap, int R,
                             float alpha, int metric, uint32_t *out, char *eb, int el) {
    try {
        HIPANN_REQUIRE(h, "robust prune: null db");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        build_shape_check(db, R, alpha, metric);
        HIPANN_REQUIRE(m >= 0 && pool_cap >= 1 && (m == 0 || (targets && pools && out)), "robust prune: bad arguments");
        for (int i = 0; i < m; ++i) HIPANN_REQUIRE((int64_t)targets[i] < db->n, "robust prune: target id out of range");
        if (m == 0) return 0;
        DeviceGuard g(db->device);
        const hipStream_t st = db->stream;
        const int dev = db->device;
        DevBuf tg, pl, od, gram;
        const size_t pw = (size_t)m * pool_cap;
        tg.ensure((size_t)m * 4, dev);
        pl.ensure(pw * 4, dev);
        od.ensure((size_t)m * R * 4, dev);
        const int blocks = vamana_prune_blocks(m);
        gram.ensure(vamana_gram_bytes(blocks), dev);
        HIPANN_CHECK(hipMemcpyAsync(tg.p, targets, (size_t)m * 4, hipMemcpyHostToDevice, st));
        HIPANN_CHECK(hipMemcpyAsync(pl.p, pools, pw * 4, hipMemcpyHostToDevice, st));
        launch_vamana_prune(db->data.get<float>(), db->dim, (uint32_t)db->n, tg.get<uint32_t>(), m, nullptr,
                            pl.get<uint32_t>(), nullptr, nullptr, nullptr, nullptr, pool_cap, R, alpha,
                            od.get<uint32_t>(), false, gram.get<float>(), blocks, nullptr, st);
        HIPANN_CHECK(hipMemcpyAsync(out, od.p, (size_t)m * R * 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        return 0;
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return -1;
}

}  // extern "C"
