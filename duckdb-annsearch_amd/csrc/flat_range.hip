// flat_range.hip — Flat range search (faiss::IndexFlat::range_search): every row with direct-form Σ(q−x)² < radius
// (L2) or q·x > radius (IP), per query in ascending label order, as a variable-length result.
//
// Two passes over one schedule, no atomics on the result order.  Pass A (count) writes one count per (query, part);
// range_offsets turns the counts, query-major, into offsets and lims; pass B (fill) repeats the scan and writes
// (distance, label) at offset + rank, the rank being the number of admitted rows before it in row order.  Parts are
// contiguous row ranges in ascending order, so a query's slice is ascending by label with no sort, and both passes
// evaluate the same comparisons on the same bits: the result is the same on every run.
//
// nq >= 20, finite rows — flat_range_scan: a threshold-epilogue scan over the tiled bf16 image of the rows
// (flat_bf16.hip's image and measured residuals, reused).  A block of 4 waves owns a 128-query tile and streams the
// 256-row image tiles of its row split through a 4-stage LDS ring (LDS-DMA, 16 KiB per 32-dim chunk); each wave
// owns 32 queries × the tile's 256 rows (8 accumulators of 32×32, v_mfma_f32_32x32x16_bf16) and reads its query
// fragments from the L2-resident query image into a register ring.  Epilogue per tile, in registers: with
// key = ‖q‖² + ‖x‖² − 2·acc (L2) or acc (IP), a row survives when key ≤ radius + E(q) (IP: key ≥ radius − E(q)) —
// one fma + compare per element against a per-query constant, one ballot per accumulator register; a tile without a
// survivor (the common one) touches no LDS.  Survivors are rechecked in place: the wave recomputes the direct-form
// distance from the fp32 row and query (rerank_rows4 and the rerank's butterfly: the bits hipann_flat_search's exact
// forms return) and admits the row only if that value passes the strict comparison.
//
// The slack E(q) — the bound ivf_rerank_topk proves for this image (its rxmax >= 0 branch), restated.  Let q̂, x̂ be
// the bf16 roundings, rq = ‖q̂ − q‖ (computed per query), ‖x̂ − x‖ ≤ rxmax and ‖x‖² ≤ xmax2 for every row (measured
// when the image is built; running maxima over adds, kept over removes: upper bounds).  Then
//   |q̂·x̂ − q·x| ≤ ‖q‖·rxmax + rq·(√xmax2 + rxmax)                                         (Cauchy-Schwarz)
//   |acc − q̂·x̂| ≤ d·2⁻²⁴·(‖q‖ + rq)·(√xmax2 + rxmax)                     (fp32 accumulation of exact products)
//   |key − dist|, |direct-form fp32 value − dist| and the fp32 roundings of ‖q‖², ‖x‖² ≤ (d + 8)·2⁻²⁴·2(‖q‖² + xmax2)
// E = 1.01·((L2: 2, IP: 1)·(first two lines) + third line) + 2⁻²²·(‖q‖² + xmax2); the last term covers the roundings
// of radius + E and of the per-query constant the filter compares against (each ≤ 2⁻²⁴ of a magnitude that, wherever a
// row can lie within E of the radius, is ≤ 2(‖q‖² + xmax2) + E).  Proof obligations: (1) rxmax and xmax2 bound every
// row the image holds; (2) the image is the RNE bf16 of the rows the recheck reads; (3) a non-finite E (a query with
// non-finite or huge entries) makes every row a survivor.  So the filter only ever adds rows to be rechecked: a row the
// direct form admits has key within E of its direct-form value and survives.  Nothing here is tuned from data.
//
// nq < 20, rows with a non-finite entry (no bound exists) — flat_range_direct: flat_scan_topk's direct form with the
// same sum order (queries in LDS, each wave streams its rows with 16-byte loads, 4 rows in flight), so the distance
// equals the small-batch hipann_flat_search's; the value it computes is the one compared and returned.
#include "rerank_rows.hpp"
#include "runtime.hpp"

#include <type_traits>
#include <utility>

namespace hipann {

typedef __bf16 rg_b16x8 __attribute__((ext_vector_type(8)));
typedef float rg_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned rg_u32x4 __attribute__((ext_vector_type(4)));  // 16-B unit of the bf16 images
typedef __attribute__((address_space(3))) void rg_lds_void;

constexpr int RG_TN = 256;  // rows per image tile (flat_bf16_tile_rows)
constexpr int RG_W = 4;     // waves per block
constexpr int RG_QM = 32 * RG_W;  // queries per block
constexpr int RG_NB = 4;    // LDS stages of one 32-dim chunk of a row tile
constexpr int RG_BU = RG_TN * 4, RG_AU = RG_QM * 4;  // 16-B units per chunk of a row tile / a query tile

template <int N>
__device__ __forceinline__ void rg_wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Per query: the constant the scan's filter compares 2·acc − ‖x‖² (IP: 2·acc) against — ‖q‖² − (radius + E) for L2,
// 2·(radius − E) for IP — from the query's own ‖q‖² and bf16 residual (summed in the rerank's order) and the shard's
// measured row terms.  A non-finite E: −inf, every row is rechecked.  One wave per query.
template <bool IP>
__global__ void __launch_bounds__(256) range_query_prep(const float *__restrict__ Q, int64_t nq, int d, float radius,
                                                        float xmax2, float rxmax, float *__restrict__ cth) {
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int lane = threadIdx.x & 63;
    const float *qp = Q + q * (int64_t)d;
    float qq = 0.f, rq2 = 0.f;
    for (int e = lane; e < d; e += 64) {
        const float v = qp[e];
        qq = fmaf(v, v, qq);
        const float r = v - (float)(__bf16)v;  // RNE, as the bf16 image of the queries
        rq2 = fmaf(r, r, rq2);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        qq += __shfl_xor(qq, o);
        rq2 += __shfl_xor(rq2, o);
    }
    const float qn = sqrtf(qq), rq = sqrtf(rq2), xh = sqrtf(xmax2) + rxmax;
    const float g = (float)d * 0x1p-24f;
    const float eip = qn * rxmax + rq * xh + g * (qn + rq) * xh;
    const float E = 1.01f * ((IP ? 1.f : 2.f) * eip + (float)(d + 8) * 0x1p-24f * 2.f * (qq + xmax2)) +
                    0x1p-22f * (qq + xmax2);
    float c = IP ? 2.f * (radius - E) : qq - (radius + E);
    if (!(E <= 3.4e38f)) c = -__builtin_inff();
    if (lane == 0) cth[q] = c;
}

// The scan.  FILL = false: counts[q·nsplit + split] = admitted rows of query q in the split's rows; stat (optional)
// += the filter's survivors.  FILL = true: the admitted rows' (distance, label) at off[q·nsplit + split] + rank.
template <bool L2M, bool FILL>
__global__ void __launch_bounds__(64 * RG_W, 1)
flat_range_scan(const rg_u32x4 *__restrict__ Qt, const float *__restrict__ cth_g, int64_t nq,
                const rg_u32x4 *__restrict__ Xt, const float *__restrict__ xnorm, int64_t N, int nk, int nqt, int nsplit,
                int64_t tiles_per_split, const float *__restrict__ Q, const float *__restrict__ X, int d, float radius,
                int *__restrict__ counts, const int64_t *__restrict__ off, float *__restrict__ D,
                int64_t *__restrict__ I, int64_t label_offset, unsigned long long *__restrict__ stat) {
    constexpr int NB = RG_NB;
    constexpr int IB = RG_BU / 64 / RG_W;  // global_load_lds (1 KiB each) per wave per chunk
    constexpr int NI = IB + 2;             // vector-memory ops per wave per chunk (+ the two query fragments)
    extern __shared__ __attribute__((aligned(16))) rg_u32x4 smem_rg[];
    volatile int *cnt = reinterpret_cast<volatile int *>(smem_rg + NB * RG_BU);  // per query: admitted so far

    const int nblocks = nqt * nsplit;
    const int lb = xcd_remap(blockIdx.x, nblocks);
    const int qt = lb % nqt;
    const int split = lb / nqt;
    const int64_t q0 = (int64_t)qt * RG_QM;
    const int64_t ntiles = ceil_div(N, RG_TN);
    const int64_t t0 = (int64_t)split * tiles_per_split;
    const int64_t t1 = t0 + tiles_per_split < ntiles ? t0 + tiles_per_split : ntiles;
    const int64_t G = t1 > t0 ? (t1 - t0) * nk : 0;

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int l31 = lane & 31, h = lane >> 5;

    if (tid < RG_QM) cnt[tid] = 0;
    float cth[16];  // +inf past nq: those rows never survive
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t q = q0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h;
        cth[r] = q < nq ? cth_g[q] : __builtin_inff();
    }

    // chunk g = (t − t0)·nk + kc: the row tile's chunk by LDS-DMA into stage g % NB (lane-linear: the swizzle is in
    // the image), this lane's two query fragments of chunk kc into register slot g % NB
    const rg_u32x4 *Xb = Xt + t0 * nk * RG_BU + lane;
    const rg_u32x4 *Qw = Qt + (int64_t)qt * nk * RG_AU + 32 * wave;
    int kc_issue = 0;
    rg_u32x4 ar[NB][2];
    auto issue = [&](int64_t g, int stage, auto slot_c) {
        constexpr int SL = decltype(slot_c)::value;
        rg_u32x4 *dst = smem_rg + stage * RG_BU;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const int c = 2 * s2 + h;
            ar[SL][s2] = Qw[(int64_t)kc_issue * RG_AU + c * RG_QM + (l31 ^ (c << 1))];
        }
#pragma unroll
        for (int i = 0; i < IB; ++i) {
            const int inst = wave * IB + i;
            __builtin_amdgcn_global_load_lds((const void *)(Xb + g * RG_BU + inst * 64),
                                             (rg_lds_void *)(dst + inst * 64), 16, 0, 0);
        }
        kc_issue = kc_issue + 1 < nk ? kc_issue + 1 : 0;
    };

    rg_f32x16 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    __syncthreads();  // the counts' initialisation
    if (G > 0) {      // the ring starts full (past the end: the last chunk again)
        [&]<int... P>(std::integer_sequence<int, P...>) {
            (issue(P < G ? P : G - 1, P, std::integral_constant<int, P>{}), ...);
        }(std::make_integer_sequence<int, NB - 1>{});
    }

    unsigned nsurv = 0;
    // The survivors of one tile, rechecked: for every accumulator register with a survivor (rmask) and each of its two
    // queries (one per half wave), the rows in (row group, lane) order = ascending row, four at a time.  pb: this
    // lane's survivor bits, bit 8·(r & 3) + j of pb[r >> 2] = row group j of accumulator register r.
    auto recheck = [&](unsigned rmask, const unsigned (&pb)[4], int64_t x0) {
        while (rmask) {
            const int r = __builtin_ctz(rmask);
            rmask &= rmask - 1;
            const unsigned pw = ((r >> 2) == 0 ? pb[0] : (r >> 2) == 1 ? pb[1] : (r >> 2) == 2 ? pb[2] : pb[3]) >>
                                (8 * (r & 3));
            for (int hh = 0; hh < 2; ++hh) {
                const int ql = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * hh;
                const int64_t q = q0 + ql;
                if (q >= nq) continue;
                const float *qp = Q + q * (int64_t)d;
                int c = __builtin_amdgcn_readfirstlane(cnt[ql]);
                const int64_t base = FILL ? off[q * nsplit + split] : 0;
                for (int j = 0; j < 8; ++j) {
                    const unsigned long long pm = __ballot((pw >> j) & 1u);
                    unsigned bits = (unsigned)(pm >> (32 * hh));
                    while (bits) {
                        int64_t row[4];
                        bool ok[4];
                        const float *xr[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            ok[u] = bits != 0;
                            if (ok[u]) {
                                row[u] = x0 + 32 * j + __builtin_ctz(bits);
                                bits &= bits - 1;
                            } else {
                                row[u] = row[0];
                            }
                            ok[u] = ok[u] && row[u] < N;  // rows past N in the last tile never pass
                            xr[u] = X + (row[u] < N ? row[u] : N - 1) * (int64_t)d;
                        }
                        float a4[4] = {0.f, 0.f, 0.f, 0.f};
                        rerank_rows4<!L2M>(qp, xr, d, lane, a4);
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            float a = a4[u];
#pragma unroll
                            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
                            const bool pass = ok[u] && (L2M ? a < radius : a > radius);
                            if (ok[u]) ++nsurv;
                            if (__builtin_amdgcn_readfirstlane((int)pass)) {
                                if (FILL && lane == 0) {
                                    D[base + c] = a;
                                    I[base + c] = label_offset + row[u];
                                }
                                ++c;
                            }
                        }
                    }
                }
                cnt[ql] = c;
            }
        }
    };

    int kc = 0, stage = 0;
    int64_t t = t0;
    auto body = [&](int64_t g, auto slot_c) {
        constexpr int SL = decltype(slot_c)::value;
        // retire this wave's copies of chunk g (the later chunks' stay in flight), finish this wave's reads of the
        // stage about to be refilled, one barrier: every wave's chunk-g copies have landed and nobody still reads
        // chunk g−1's stage.  The issue is unconditional (past the end it re-reads the last chunk into a free stage),
        // so every iteration has the same count of vector-memory ops.
        rg_wait_vm<NI * (NB - 2)>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const int st_next = stage == 0 ? NB - 1 : stage - 1;
        issue(g + NB - 1 < G ? g + NB - 1 : G - 1, st_next, std::integral_constant<int, (SL + NB - 1) % NB>{});
        const rg_u32x4 *Bb = smem_rg + stage * RG_BU;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int c = 2 * s + h;
            const int lx = l31 ^ (c << 1);
            const rg_b16x8 a = __builtin_bit_cast(rg_b16x8, ar[SL][s]);
            const rg_u32x4 *Bc = Bb + c * RG_TN + lx;
            rg_b16x8 bf[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) bf[j] = __builtin_bit_cast(rg_b16x8, Bc[32 * j]);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bf[j], acc[j], 0, 0, 0);
        }
        stage = stage + 1 < NB ? stage + 1 : 0;
        if (++kc == nk) {
            kc = 0;
            const int64_t x0 = t * RG_TN;
            float xnv[8];  // +inf past N
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int64_t x = x0 + 32 * j + l31;
                xnv[j] = x < N ? (L2M ? xnorm[x] : 0.f) : __builtin_inff();
            }
            unsigned rmask = 0;
            unsigned pb[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                bool any = false;
#pragma unroll
                for (int j = 0; j < 8; ++j) any |= fmaf(2.f, acc[j][r], -xnv[j]) >= cth[r];
                if (__ballot(any) == 0ull) continue;
                unsigned m8 = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) m8 |= (fmaf(2.f, acc[j][r], -xnv[j]) >= cth[r] ? 1u : 0u) << j;
                pb[r >> 2] |= m8 << (8 * (r & 3));
                rmask |= 1u << r;
            }
            if (rmask) recheck(rmask, pb, x0);
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
            ++t;
        }
    };
    for (int64_t g = 0; g < G; g += NB) {
        [&]<int... P>(std::integer_sequence<int, P...>) {
            ((g + P < G ? body(g + P, std::integral_constant<int, P>{}) : void()), ...);
        }(std::make_integer_sequence<int, NB>{});
    }
    rg_wait_vm<0>();  // no LDS-DMA copy may land after the block's LDS is handed to the next block
    if (!FILL) {
        const int64_t q = q0 + 32 * wave + lane;
        if (lane < 32 && q < nq) counts[q * nsplit + split] = cnt[32 * wave + lane];
        if (stat && lane == 0 && nsurv) atomicAdd(stat, (unsigned long long)nsurv);
    }
}

// Exclusive scan of the M = nq·nparts counts (query-major) into off, lims[q] = off[q·nparts], lims[nq] = the total.
// One block: the counts are a few hundred thousand at most.
__global__ void __launch_bounds__(1024) range_offsets(const int *__restrict__ counts, int64_t M, int64_t nparts,
                                                      int64_t nq, int64_t *__restrict__ off, int64_t *__restrict__ lims) {
    __shared__ long long wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    long long carry = 0;
    for (int64_t b = 0; b < M; b += 1024) {
        const int64_t i = b + tid;
        const long long v = i < M ? counts[i] : 0;
        long long inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        long long before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const long long s = wsum[w];
            if (w < wv) before += s;
            total += s;
        }
        const long long ex = carry + before + inc - v;
        if (i < M) {
            off[i] = ex;
            if (i % nparts == 0) lims[i / nparts] = ex;
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) lims[nq] = carry;
}

// The direct form (flat_scan_topk's sums, bit for bit): nq <= 64 queries in LDS, wave gw over rows
// [gw·rpw, (gw + 1)·rpw) in groups of 64 (lane j ends up holding row base + j), 4 queries × 4 rows per pass over the
// dims.  Lane qi carries query qi's admitted count.  counts / off: [query][nparts], part = gw.
template <bool VEC4, bool FILL>
__global__ void __launch_bounds__(256)
flat_range_direct(const float *__restrict__ Q, int nq, const float *__restrict__ X, int64_t N, int d, int metric,
                  float radius, int64_t rows_per_wave, int64_t nparts, int *__restrict__ counts,
                  const int64_t *__restrict__ off, float *__restrict__ D, int64_t *__restrict__ I,
                  int64_t label_offset) {
    extern __shared__ __attribute__((aligned(16))) float qs_rg[];  // nq × dpad
    const int dpad = (d + 3) & ~3;
    for (int i = threadIdx.x; i < nq * dpad; i += 256) {
        const int qi = i / dpad, j = i - qi * dpad;
        qs_rg[i] = j < d ? Q[(int64_t)qi * d + j] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t r0 = gw * rows_per_wave;
    int64_t r1 = r0 + rows_per_wave;
    if (r1 > N) r1 = N;
    const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
    int cntv = 0;
    const int nd4 = dpad >> 2;
    for (int64_t base = r0; base < r1; base += 64) {
        const int64_t gend = base + 64 < r1 ? base + 64 : r1;
        const int64_t myrow = base + lane;
        for (int qb = 0; qb < nq; qb += 4) {
            float cand[4] = {0.f, 0.f, 0.f, 0.f};
            for (int64_t rr = base; rr < gend; rr += 4) {
                float acc[4][4];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int qi = 0; qi < 4; ++qi) acc[r][qi] = 0.f;
                for (int j4 = lane; j4 < nd4; j4 += 64) {
                    float4 xv[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t row = rr + r;
                        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (row < gend) {
                            const float *src = X + row * (int64_t)d + 4 * j4;
                            if (VEC4) v = *reinterpret_cast<const float4 *>(src);
                            else {
                                const int j = 4 * j4;
                                if (j + 0 < d) v.x = src[0];
                                if (j + 1 < d) v.y = src[1];
                                if (j + 2 < d) v.z = src[2];
                                if (j + 3 < d) v.w = src[3];
                            }
                        }
                        xv[r] = v;
                    }
#pragma unroll
                    for (int qi = 0; qi < 4; ++qi) {
                        const int qx = qb + qi < nq ? qb + qi : nq - 1;
                        const float4 qv = *reinterpret_cast<const float4 *>(qs_rg + qx * dpad + 4 * j4);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (metric == kL2) {
                                float t;
                                t = qv.x - xv[r].x; acc[r][qi] = fmaf(t, t, acc[r][qi]);
                                t = qv.y - xv[r].y; acc[r][qi] = fmaf(t, t, acc[r][qi]);
                                t = qv.z - xv[r].z; acc[r][qi] = fmaf(t, t, acc[r][qi]);
                                t = qv.w - xv[r].w; acc[r][qi] = fmaf(t, t, acc[r][qi]);
                            } else {
                                acc[r][qi] = fmaf(qv.x, xv[r].x, acc[r][qi]);
                                acc[r][qi] = fmaf(qv.y, xv[r].y, acc[r][qi]);
                                acc[r][qi] = fmaf(qv.z, xv[r].z, acc[r][qi]);
                                acc[r][qi] = fmaf(qv.w, xv[r].w, acc[r][qi]);
                            }
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int slot = (int)(rr + r - base);
#pragma unroll
                    for (int qi = 0; qi < 4; ++qi) {
                        float s = acc[r][qi];
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
                        if (lane == slot) cand[qi] = s;
                    }
                }
            }
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) {
                const int q = qb + qi;
                if (q >= nq) break;
                const bool pass = myrow < gend && (metric == kL2 ? cand[qi] < radius : cand[qi] > radius);
                const unsigned long long m = __ballot(pass);
                const int c = __shfl(cntv, q);
                if (FILL && pass) {
                    const int64_t pos = off[q * nparts + gw] + c + __popcll(m & below);
                    D[pos] = cand[qi];
                    I[pos] = label_offset + myrow;
                }
                if (lane == q) cntv += __popcll(m);
            }
        }
    }
    if (!FILL && lane < nq) counts[lane * nparts + gw] = cntv;
}

// ------------------------------------------------------------------------------------------------
int flat_range_query_tile() { return RG_QM; }

void launch_flat_range_query_prep(const float *Q, int64_t nq, int d, int metric, float radius, float xmax2, float rxmax,
                                  float *cth, hipStream_t st) {
    if (nq <= 0) return;
    const dim3 grid((unsigned)ceil_div(nq, 4)), block(256);
    if (metric == kL2)
        hipLaunchKernelGGL(range_query_prep<false>, grid, block, 0, st, Q, nq, d, radius, xmax2, rxmax, cth);
    else hipLaunchKernelGGL(range_query_prep<true>, grid, block, 0, st, Q, nq, d, radius, xmax2, rxmax, cth);
    HIPANN_CHECK(hipGetLastError());
}

void launch_flat_range_scan(const FlatRangeArgs &a, bool fill, hipStream_t st) {
    const int nk = (a.d + 31) / 32;
    const int nqt = (int)ceil_div(a.nq, RG_QM);
    HIPANN_REQUIRE((int64_t)nqt * a.nparts < 0x7fffffff, "grid too large");
    HIPANN_REQUIRE(a.tiles_per_split > 0 && a.nparts * a.tiles_per_split >= ceil_div(a.N, RG_TN), "range scan: bad split");
    const size_t smem = (size_t)RG_NB * RG_BU * 16 + RG_QM * sizeof(int);
    const dim3 grid((unsigned)(nqt * a.nparts)), block(64 * RG_W);
    const rg_u32x4 *qa = static_cast<const rg_u32x4 *>(a.qimg), *xa = static_cast<const rg_u32x4 *>(a.ximg);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, smem, st, qa, a.cth, a.nq, xa, a.xn, a.N, nk, nqt, (int)a.nparts,
                           a.tiles_per_split, a.Q, a.X, a.d, a.radius, a.counts, a.off, a.D, a.I, a.label_offset,
                           a.stat);
    };
    if (a.metric == kL2) {
        if (fill) go(flat_range_scan<true, true>);
        else go(flat_range_scan<true, false>);
    } else {
        if (fill) go(flat_range_scan<false, true>);
        else go(flat_range_scan<false, false>);
    }
    HIPANN_CHECK(hipGetLastError());
}

void launch_flat_range_offsets(const int *counts, int64_t nq, int64_t nparts, int64_t *off, int64_t *lims,
                               hipStream_t st) {
    hipLaunchKernelGGL(range_offsets, dim3(1), dim3(1024), 0, st, counts, nq * nparts, nparts, nq, off, lims);
    HIPANN_CHECK(hipGetLastError());
}

// the direct kernel's waves (parts) over n rows and the rows each walks: flat_direct_scan's rule (≥ 512 rows per wave
// on large tables, small ones spread over waves of ≥ 16 rows), rounded up to whole 4-wave blocks
int64_t flat_range_direct_parts(int64_t n, int64_t *rows_per_wave) {
    const int64_t want = std::min<int64_t>(8192, std::max<int64_t>(std::min<int64_t>(256, ceil_div(n, 16)),
                                                                     ceil_div(n, 512)));
    *rows_per_wave = ceil_div(n, std::max<int64_t>(want, 1));
    return ceil_div(ceil_div(n, *rows_per_wave), 4) * 4;
}

// the queries of one launch: at most 64 (one lane per count) and 64 KiB of LDS (the direct top-k scan's rule)
int flat_range_direct_chunk(int64_t nq, int d) {
    int qc = (int)std::min<int64_t>(nq, 64);
    while (qc > 1 && scan_smem_bytes(qc, d) > 64 * 1024) --qc;
    HIPANN_REQUIRE(scan_smem_bytes(qc, d) <= 64 * 1024, "dimension too large for the scan path");
    return qc;
}

// One query chunk (a.Q / a.nq: its queries; a.counts / a.off: its rows of the [query][nparts] arrays).
void launch_flat_range_direct(const FlatRangeArgs &a, int64_t rows_per_wave, bool fill, hipStream_t st) {
    const size_t smem = scan_smem_bytes((int)a.nq, a.d);
    const dim3 grid((unsigned)(a.nparts / 4)), block(256);
    const bool vec4 = a.d % 4 == 0 && (reinterpret_cast<uintptr_t>(a.X) & 15) == 0;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, smem, st, a.Q, (int)a.nq, a.X, a.N, a.d, a.metric, a.radius,
                           rows_per_wave, a.nparts, a.counts, a.off, a.D, a.I, a.label_offset);
    };
    if (vec4) {
        if (fill) go(flat_range_direct<true, true>);
        else go(flat_range_direct<true, false>);
    } else {
        if (fill) go(flat_range_direct<false, true>);
        else go(flat_range_direct<false, false>);
    }
    HIPANN_CHECK(hipGetLastError());
}

}  // namespace hipann
