// diskann_build.hip — the insert half of a DiskANN (Vamana) graph build on gfx950: RobustPrune and the back-edge update
// for a batch of rows searched against the frozen graph (the crate's multi_insert shape,
// rust_lib/diskann-patch/src/graph/index.rs:990-1163, occlude_list :3329-3500).
//
// vamana_prune — one 256-thread workgroup per target node.
//   1. pool: ids (+ the traversal's distances, or Σ(a−b)² computed here, one wave per candidate) → 64-bit keys
//      (dist bits << 32 | id), bitonic sort in LDS in chunks of 256 merged into the 256 smallest kept so far;
//      repeated ids are adjacent after the sort (same target, same id, same distance) and dropped.  M ≤ 256 survive.
//   2. pairwise: the M × M Gram matrix G = X·Xᵀ of the candidates' rows on the fp32 matrix cores
//      (v_mfma_f32_32x32x2_f32: exact fp32 fma chains, so sums of exactly representable partials are exact and the
//      result is the same from run to run).  Rows are staged through LDS in K-slices of 128 dims (M ≤ 128:
//      [row][132] floats) or 64 dims ([row][68]), 68 KB either way, four 16-B gathers in flight per thread; a wave
//      owns one 32-row tile × four 32-column tiles (64 accumulator registers); M ≤ 128
//      is one pass over K, M = 256 four.  Only tiles on or above the diagonal are computed.  M ≤ 128: G (≤ 64 KB)
//      takes over the staging buffer in LDS.  Larger pools: a 256² fp32 matrix does not fit the LDS next to the
//      slices, so G goes to a per-workgroup global scratch (M² floats, ≤ 256 KB, re-read from L2).
//      d(i, j) = max(0, (G_ii + G_jj) − 2·G_ij).
//   3. selection: wave 0 runs the greedy passes over the finished matrix, 4 pool positions per lane: threshold
//      t = 1, ·min(alpha, 1.2) …, capped at alpha; a position is selected when its occlusion factor
//      max_j d(p, i) / d(j, i) over the selected j ahead of it is ≤ t; selecting i updates every later position.
//   vamana_prune<kIP> (a handle whose graph metric is IP): d = −dot, so (1) computes −Σ p·v by the same
//   lane split and the keys hold ip_key_bits(dist), (2) is unchanged and d(j, i) = −G_ji (no norms, no clamp), and
//   (3) is the crate's occluding rule, which remembers per position how many selected entries it has met.
//
// Back-edges of a batch — count (atomic per target row; integer), offsets, fill, then one wave per touched row:
// the row's new sources rank-sorted ascending (the order of arrival never shows), appended when the row has room,
// else row + sources become a pool for vamana_prune.
#include "diskann_kernels.hpp"

#include <algorithm>
#include <cfloat>
#include <cstdint>

namespace hipann {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr unsigned long long kBadKey = ~0ull;
constexpr int kPoolMax = 256;  // pool positions kept (the crate's u16 positions)
constexpr int kGK = 32;        // dims per MFMA group (16 MFMAs of K = 2 per tile pair)
// LDS floats of a staged K-slice: 256 rows × (64 + 4) or 128 rows × (128 + 4); rows 16-B aligned, 4 banks of skew
constexpr int kTileFloats = kPoolMax * (64 + 4);

// a word another wave of this workgroup (or this wave's other lanes) stored earlier in the launch: past this CU's L1
__device__ __forceinline__ float load_l2(const float *p) {
    return __uint_as_float(
        __hip_atomic_load(reinterpret_cast<const unsigned *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ uint32_t load_l2(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int METRIC>
__global__ void __launch_bounds__(256) vamana_prune(PruneArgs a) {
    __shared__ unsigned long long s_key[2 * kPoolMax];
    __shared__ __attribute__((aligned(16))) float s_tile[kTileFloats];
    __shared__ int s_wtot[4];
    __shared__ int s_M, s_trunc;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int d = a.d, R = a.R;
    const int m = a.m_ptr ? *a.m_ptr : a.m;
    float *gs = a.gram + (size_t)blockIdx.x * (kPoolMax * kPoolMax);
    if (a.counters && blockIdx.x == 0 && t == 0 && m > 0) atomicAdd(a.counters + 0, (unsigned long long)m);

    for (int tt = blockIdx.x; tt < m; tt += gridDim.x) {
        const uint32_t tgt = a.targets[tt];
        const int64_t beg = a.pool_beg ? (int64_t)a.pool_beg[tt] : (int64_t)tt * a.pool_cap;
        const int len = a.pool_len ? a.pool_len[tt] : a.pool_cap;
        const float4 *xt = reinterpret_cast<const float4 *>(a.x + (size_t)tgt * d);

        // ---- 1. the pool's 256 smallest distinct (dist, id) ----
        s_key[t] = kBadKey;
        if (t == 0) { s_M = 0; s_trunc = 0; }
        __syncthreads();
        for (int c0 = 0; c0 < len; c0 += 256) {
            const int e = c0 + t;
            uint32_t id = kNone;
            if (e < len) id = a.pool64 ? (uint32_t)a.pool64[beg + e] : a.pool32[beg + e];
            const bool valid = id < a.n && id != tgt;
            float dist = 0.f;
            if (a.pool_d) {
                if (valid) dist = a.pool_d[beg + e];
            } else {
                // four candidates' rows in flight per wave (an empty slot re-reads the target's row; its sum is dropped)
                const uint32_t mine = valid ? id : kNone;
                for (int j0 = 0; j0 < 64; j0 += 4) {
                    uint32_t cj[4];
                    const float4 *xc[4];
                    float s[4];
                    bool any = false;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        cj[u] = __shfl(mine, j0 + u);
                        any |= cj[u] != kNone;
                        xc[u] = reinterpret_cast<const float4 *>(a.x + (size_t)(cj[u] != kNone ? cj[u] : tgt) * d);
                        s[u] = 0.f;
                    }
                    if (!any) continue;  // (wave-uniform)
                    for (int q4 = lane; q4 < (d >> 2); q4 += 64) {
                        const float4 p4 = xt[q4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const float4 v = xc[u][q4];
                            if constexpr (METRIC == kIP) {
                                s[u] = fmaf(p4.x, v.x, s[u]);
                                s[u] = fmaf(p4.y, v.y, s[u]);
                                s[u] = fmaf(p4.z, v.z, s[u]);
                                s[u] = fmaf(p4.w, v.w, s[u]);
                            } else {
                                float w;
                                w = p4.x - v.x; s[u] = fmaf(w, w, s[u]);
                                w = p4.y - v.y; s[u] = fmaf(w, w, s[u]);
                                w = p4.z - v.z; s[u] = fmaf(w, w, s[u]);
                                w = p4.w - v.w; s[u] = fmaf(w, w, s[u]);
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float r = wave_sum(s[u]);
                        if (lane == j0 + u) dist = METRIC == kIP ? -r : r;
                    }
                }
            }
            const uint32_t kb = METRIC == kIP ? ip_key_bits(dist) : __float_as_uint(dist);
            s_key[kPoolMax + t] = valid ? (((unsigned long long)kb << 32) | id) : kBadKey;
            __syncthreads();
            // bitonic sort of the 512 keys (ascending)
            for (int k = 2; k <= 2 * kPoolMax; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    const int i = 2 * t - (t & (j - 1)), p = i + j;
                    const unsigned long long A = s_key[i], B = s_key[p];
                    const bool asc = (i & k) == 0;
                    if ((A > B) == asc) { s_key[i] = B; s_key[p] = A; }
                    __syncthreads();
                }
            // drop repeats (adjacent), keep the first 256
            const unsigned long long k0 = s_key[2 * t], k1 = s_key[2 * t + 1];
            const unsigned long long kp = t ? s_key[2 * t - 1] : kBadKey;
            const int f0 = k0 != kBadKey && (t == 0 || k0 != kp);
            const int f1 = k1 != kBadKey && k1 != k0;
            const int c = f0 + f1;
            int inc = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(inc, o);
                if (lane >= o) inc += v;
            }
            if (lane == 63) s_wtot[wave] = inc;
            __syncthreads();
            int base = inc - c;
            for (int w = 0; w < wave; ++w) base += s_wtot[w];
            const int total = s_wtot[0] + s_wtot[1] + s_wtot[2] + s_wtot[3];
            s_key[2 * t] = kBadKey;
            s_key[2 * t + 1] = kBadKey;
            __syncthreads();
            if (f0 && base < kPoolMax) s_key[base] = k0;
            if (f1 && base + f0 < kPoolMax) s_key[base + f0] = k1;
            if (t == 0) {
                s_M = total < kPoolMax ? total : kPoolMax;
                if (total > kPoolMax) s_trunc = 1;
            }
            __syncthreads();
        }
        const int M = s_M;
        const int MP = (M + 31) & ~31;
        const bool g_lds = MP <= 128;  // G in LDS (the selection reads it there) instead of the global scratch

        // ---- 2. Gram matrix of the candidates' rows (tiles on or above the diagonal) ----
        if (M > 1) {
            const int MT = MP >> 5, NCG = (MT + 3) >> 2, nitems = MT * NCG;
            // dims per K-slice: 128 when at most 128 rows are staged, else 64 (the same LDS either way); LD = row stride
            const int KS = MP <= 128 ? 128 : 64, LD = KS + 4, sh = MP <= 128 ? 5 : 4;
            const int nk = (d + KS - 1) / KS, nld = MP << sh;
            for (int it0 = 0; it0 < nitems; it0 += 4) {
                const int it = it0 + wave;
                const int ti = it / NCG, tj0 = (it % NCG) * 4;
                const int tjl = tj0 + 3 < MT - 1 ? tj0 + 3 : MT - 1;
                const bool work = it < nitems && tjl >= ti;
                f32x16 acc[4];
#pragma unroll
                for (int cg = 0; cg < 4; ++cg)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[cg][r] = 0.f;
                for (int kc = 0; kc < nk; ++kc) {
                    // four 16-B gathers in flight per thread, then their LDS stores
                    for (int f0 = t; f0 < nld; f0 += 1024) {
                        float4 v[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int f = f0 + 256 * u;
                            const int row = f >> sh, kk = kc * KS + 4 * (f & ((KS >> 2) - 1));
                            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                            if (f < nld && row < M && kk < d)
                                v[u] = *reinterpret_cast<const float4 *>(a.x + (size_t)(uint32_t)s_key[row] * d + kk);
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int f = f0 + 256 * u;
                            if (f < nld)
                                *reinterpret_cast<float4 *>(s_tile + (f >> sh) * LD + 4 * (f & ((KS >> 2) - 1))) = v[u];
                        }
                    }
                    __syncthreads();
                    if (work) {
                        for (int k0 = 0; k0 < KS; k0 += kGK) {
                            f32x4 a4[4], b4[4][4];
#pragma unroll
                            for (int u = 0; u < 4; ++u)
                                a4[u] = *reinterpret_cast<const f32x4 *>(s_tile + (32 * ti + l31) * LD + k0 + 16 * h + 4 * u);
#pragma unroll
                            for (int cg = 0; cg < 4; ++cg) {
                                const int tj = tj0 + cg < MT ? tj0 + cg : MT - 1;
#pragma unroll
                                for (int u = 0; u < 4; ++u)
                                    b4[cg][u] = *reinterpret_cast<const f32x4 *>(s_tile + (32 * tj + l31) * LD + k0 +
                                                                                 16 * h + 4 * u);
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u)
#pragma unroll
                                for (int e = 0; e < 4; ++e)
#pragma unroll
                                    for (int cg = 0; cg < 4; ++cg)
                                        acc[cg] =
                                            __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u][e], b4[cg][u][e], acc[cg], 0, 0, 0);
                        }
                    }
                    __syncthreads();
                }
                if (work) {
#pragma unroll
                    for (int cg = 0; cg < 4; ++cg) {
                        const int tj = tj0 + cg;
                        if (tj >= MT || tj < ti) continue;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = 32 * ti + (r & 3) + 8 * (r >> 2) + 4 * h;
                            // M ≤ 128: one round of tiles, so the staging buffer is free and holds G (≤ 64 KB)
                            if (g_lds) s_tile[row * MP + 32 * tj + l31] = acc[cg][r];
                            else gs[row * MP + 32 * tj + l31] = acc[cg][r];
                        }
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }

        // ---- 3. selection (wave 0; position p = s·64 + lane) ----
        if constexpr (METRIC == kIP) {
            // The order-dependent rule of DESIGN §6.5 (the crate's lazy loop).  A position is tested against the
            // selected entries in selection order and stops at its first occluder, so its verdict against the entries
            // that exist never changes when more are appended: every alive position catches up with the entries it has
            // not seen at the start of a pass, and the ones still unoccluded meet each new entry as it is selected.
            if (wave == 0) {
                float f[4], cd[4];
                int c[4];     // entries of sel already compared with the position
                bool pend[4];  // alive in this pass and not occluded so far
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int p = s * 64 + lane;
                    f[s] = FLT_MAX;
                    cd[s] = 0.f;
                    c[s] = 0;
                    if (p < M) {
                        f[s] = 0.f;
                        cd[s] = ip_key_dist((uint32_t)(s_key[p] >> 32));
                    }
                }
                const float alpha = a.alpha, step = fminf(alpha, 1.2f);
                float th = 1.0f;
                int nsel = 0;
                int selpos = 0;  // lane r: the position of the r-th selected entry
                for (;;) {
                    const float occ = th + 0.01f;
                    float bound[4];  // t · d(p, i)
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        pend[s] = f[s] <= th;
                        bound[s] = __fmul_rn(th, cd[s]);
                    }
                    // catch up with the entries selected in earlier passes
                    for (int l = 0; l < nsel; ++l) {
                        bool need = false;
#pragma unroll
                        for (int s = 0; s < 4; ++s) need |= pend[s] && c[s] <= l;
                        if (!__ballot(need)) continue;  // (wave-uniform)
                        const int j = __builtin_amdgcn_readlane(selpos, l);
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const int p = s * 64 + lane;
                            if (pend[s] && c[s] <= l) {
                                c[s] = l + 1;
                                if (j < p) {
                                    const float g = g_lds ? s_tile[j * MP + p] : load_l2(gs + j * MP + p);
                                    if (-g < bound[s]) { pend[s] = false; f[s] = occ; }
                                }
                            }
                        }
                    }
                    // the first unoccluded position is selected; the later ones meet it
                    while (nsel < R) {
                        int i = -1;
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const unsigned long long mask = __ballot(pend[s]);
                            if (i < 0 && mask) i = s * 64 + __ffsll(mask) - 1;
                        }
                        if (i < 0) break;
                        if (lane == nsel) selpos = i;
                        nsel++;
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const int p = s * 64 + lane;
                            if (p == i) {
                                pend[s] = false;
                                f[s] = FLT_MAX;
                            } else if (pend[s]) {  // (p > i: i is the first)
                                c[s] = nsel;
                                const float g = g_lds ? s_tile[i * MP + p] : load_l2(gs + i * MP + p);
                                if (-g < bound[s]) { pend[s] = false; f[s] = occ; }
                            }
                        }
                    }
                    if (nsel >= R || !(th < alpha)) break;
                    th = fminf(th * step, alpha);
                }
                uint32_t *o = a.out + (size_t)(a.out_by_target ? tgt : (uint32_t)tt) * R;
                if (lane < R) o[lane] = lane < nsel ? (uint32_t)s_key[selpos] : kNone;
                if (lane == 0 && s_trunc && a.counters) atomicAdd(a.counters + 1, 1ull);
            }
        } else if (wave == 0) {
            float f[4], cd[4], nrm[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int p = s * 64 + lane;
                f[s] = FLT_MAX;
                cd[s] = 0.f;
                nrm[s] = 0.f;
                if (p < M) {
                    f[s] = 0.f;
                    cd[s] = __uint_as_float((unsigned)(s_key[p] >> 32));
                    if (M > 1) nrm[s] = g_lds ? s_tile[p * MP + p] : load_l2(gs + p * MP + p);
                }
            }
            const float alpha = a.alpha, step = fminf(alpha, 1.2f);
            float th = 1.0f;
            int nsel = 0;
            uint32_t mine = kNone;  // lane r: the r-th selected id
            for (;;) {
                int pos = 0;
                while (nsel < R) {
                    int i = -1;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int p = s * 64 + lane;
                        const unsigned long long mask = __ballot(p >= pos && f[s] <= th);
                        if (i < 0 && mask) i = s * 64 + __ffsll(mask) - 1;
                    }
                    if (i < 0) break;
                    if (lane == nsel) mine = (uint32_t)s_key[i];
                    nsel++;
                    float ni = 0.f;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const float v = __shfl(nrm[s], i & 63);
                        if ((i >> 6) == s) ni = v;
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int p = s * 64 + lane;
                        if (p == i) {
                            f[s] = FLT_MAX;
                        } else if (p > i && p < M && f[s] <= alpha) {
                            const float g = g_lds ? s_tile[i * MP + p] : load_l2(gs + i * MP + p);
                            float dj = (ni + nrm[s]) - 2.f * g;
                            dj = dj < 0.f ? 0.f : dj;
                            const float fac = dj == 0.f ? FLT_MAX : cd[s] / dj;
                            f[s] = fmaxf(f[s], fac);
                        }
                    }
                    pos = i + 1;
                }
                if (nsel >= R || !(th < alpha)) break;
                th = fminf(th * step, alpha);
            }
            uint32_t *o = a.out + (size_t)(a.out_by_target ? tgt : (uint32_t)tt) * R;
            if (lane < R) o[lane] = lane < nsel ? mine : kNone;
            if (lane == 0 && s_trunc && a.counters) atomicAdd(a.counters + 1, 1ull);
        }
        __syncthreads();
    }
}

// the batch's rows: insertion order o (the entry point left out) → row id
__global__ void __launch_bounds__(256) vamana_fill_targets(uint32_t *tg, int b, uint32_t o0, uint32_t ep) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < b) tg[i] = o0 + (uint32_t)i < ep ? o0 + (uint32_t)i : o0 + (uint32_t)i + 1u;
}

// ctr: [0] rows touched, [1] pairs placed, [2] pool words used, [3] rows to prune
__global__ void __launch_bounds__(256) be_count(const uint32_t *__restrict__ adj, int R, const uint32_t *__restrict__ tg,
                                                int b, int *cnt, uint32_t *touched, int *ctr) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= b * R) return;
    const uint32_t q = adj[(size_t)tg[idx / R] * R + idx % R];
    if (q == kNone) return;
    if (atomicAdd(cnt + q, 1) == 0) touched[atomicAdd(ctr + 0, 1)] = q;
}

__global__ void __launch_bounds__(256) be_offsets(const uint32_t *__restrict__ touched, const int *__restrict__ cnt,
                                                  int *ctr, int *off, int *slot, int *fill) {
    const int nt = ctr[0];
    for (int u = blockIdx.x * 256 + threadIdx.x; u < nt; u += gridDim.x * 256) {
        const uint32_t q = touched[u];
        off[u] = atomicAdd(ctr + 1, cnt[q]);
        slot[q] = u;
        fill[u] = 0;
    }
}

__global__ void __launch_bounds__(256) be_fill(const uint32_t *__restrict__ adj, int R, const uint32_t *__restrict__ tg,
                                               int b, const int *__restrict__ slot, const int *__restrict__ off,
                                               int *fill, uint32_t *src) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= b * R) return;
    const uint32_t p = tg[idx / R];
    const uint32_t q = adj[(size_t)p * R + idx % R];
    if (q == kNone) return;
    const int u = slot[q];
    src[off[u] + atomicAdd(fill + u, 1)] = p;
}

// One wave per touched row q: cand = N(q) in stored order, then the new sources ascending that are not in N(q).
// |cand| ≤ R: stored; otherwise cand becomes a pool (ptgt / pbeg / plen) for vamana_prune.
__global__ void __launch_bounds__(256) be_merge(uint32_t *adj, int R, const uint32_t *__restrict__ touched,
                                                const int *__restrict__ cnt, const int *__restrict__ off, uint32_t *src,
                                                int *ctr, uint32_t *pool, uint32_t *ptgt, int *pbeg, int *plen) {
    const int lane = threadIdx.x & 63;
    const int nt = ctr[0];
    for (int u = blockIdx.x * 4 + (threadIdx.x >> 6); u < nt; u += gridDim.x * 4) {
        const uint32_t q = touched[u];
        const int c = cnt[q], o = off[u];
        const uint32_t rv = lane < R ? adj[(size_t)q * R + lane] : kNone;
        const unsigned long long sent = __ballot(rv == kNone);
        const int deg = sent ? __ffsll(sent) - 1 : 64;
        // sources already in the row leave the list
        int nnew = 0;
        for (int i0 = 0; i0 < c; i0 += 64) {
            const int i = i0 + lane;
            const uint32_t v = i < c ? src[o + i] : kNone;
            bool present = false;
            for (int r = 0; r < deg; ++r) present |= __shfl(rv, r) == v;
            if (i < c && present) __hip_atomic_store(src + o + i, kNone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            nnew += __popcll(__ballot(i < c && !present));
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int len = deg + nnew;
        uint32_t *dst;
        if (len <= R) {
            dst = adj + (size_t)q * R + deg;
        } else {
            int pb = 0;
            if (lane == 0) {
                pb = atomicAdd(ctr + 2, len);
                const int pi = atomicAdd(ctr + 3, 1);
                ptgt[pi] = q;
                pbeg[pi] = pb;
                plen[pi] = len;
            }
            pb = __shfl(pb, 0);
            if (lane < deg) pool[pb + lane] = rv;
            dst = pool + pb + deg;
        }
        // rank sort: a source's place is the number of smaller ones (ids are distinct)
        for (int i = lane; i < c; i += 64) {
            const uint32_t v = load_l2(src + o + i);
            if (v == kNone) continue;
            int rank = 0;
            for (int j = 0; j < c; ++j) rank += load_l2(src + o + j) < v ? 1 : 0;
            dst[rank] = v;
        }
    }
}

}  // namespace

// workgroups of a prune launch (each owns 256 KB of Gram scratch)
int vamana_prune_blocks(int64_t m) { return (int)(m < 1 ? 1 : m > 512 ? 512 : m); }
size_t vamana_gram_bytes(int blocks) { return (size_t)blocks * kPoolMax * kPoolMax * sizeof(float); }

void launch_vamana_prune(const PruneArgs &a, int blocks, hipStream_t st) {
    if (a.m <= 0) return;
    HIPANN_REQUIRE(a.d > 0 && a.d % 4 == 0 && a.R >= 1 && a.R <= 64 && blocks >= 1, "vamana_prune: unsupported shape");
    HIPANN_REQUIRE(a.metric == kL2 || a.metric == kIP, "vamana_prune: unsupported metric");
    const dim3 grid((unsigned)std::min(blocks, a.m));
    if (a.metric == kIP) hipLaunchKernelGGL(vamana_prune<kIP>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(vamana_prune<kL2>, grid, dim3(256), 0, st, a);
    HIPANN_CHECK(hipGetLastError());
}

void launch_vamana_fill_targets(uint32_t *tg, int b, uint32_t o0, uint32_t ep, hipStream_t st) {
    if (b <= 0) return;
    hipLaunchKernelGGL(vamana_fill_targets, dim3((unsigned)ceil_div(b, 256)), dim3(256), 0, st, tg, b, o0, ep);
    HIPANN_CHECK(hipGetLastError());
}

// The batch's back-edges up to the pools of the rows that overflow (ctr[3] of them: ptgt / pbeg / plen / pool).
// cnt: n ints, zero on entry (the launch leaves the touched rows' counts in it); ctr: 4 ints, zero on entry.
void launch_vamana_backedges(uint32_t *adj, int R, const uint32_t *tg, int b, int *cnt, int *slot, uint32_t *touched,
                             int *off, int *fill, uint32_t *src, int *ctr, uint32_t *pool, uint32_t *ptgt, int *pbeg,
                             int *plen, hipStream_t st) {
    if (b <= 0) return;
    const int64_t pairs = (int64_t)b * R;
    HIPANN_REQUIRE(pairs < (int64_t)0x7fffffff, "vamana_backedges: batch too large");
    const dim3 gp((unsigned)ceil_div(pairs, 256)), blk(256);
    const dim3 gt((unsigned)std::min<int64_t>(ceil_div(pairs, 256), 1024));
    const dim3 gm((unsigned)std::min<int64_t>(ceil_div(pairs, 4), 4096));
    hipLaunchKernelGGL(be_count, gp, blk, 0, st, adj, R, tg, b, cnt, touched, ctr);
    hipLaunchKernelGGL(be_offsets, gt, blk, 0, st, touched, cnt, ctr, off, slot, fill);
    hipLaunchKernelGGL(be_fill, gp, blk, 0, st, adj, R, tg, b, slot, off, fill, src);
    hipLaunchKernelGGL(be_merge, gm, blk, 0, st, adj, R, touched, cnt, off, src, ctr, pool, ptgt, pbeg, plen);
    HIPANN_CHECK(hipGetLastError());
}

}  // namespace hipann
