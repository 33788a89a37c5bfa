// ivf_range.hip — IVF range search (faiss::IndexIVF::range_search with the IVFFlat scanner): per query, every live row
// of its probed lists with direct-form Σ(q−x)² < radius (L2) or q·x > radius (IP), in probe order and then list order,
// as a variable-length result.
//
// One scan, no atomics on the result order.  The lists are scanned once, list-major over the plan's items (list,
// 2048-row chunk, group of the (query, probe) pairs that probe the list); the scan leaves, per (query, probe, chunk)
// slot, a bitmask of the admitted rows (2048 bits = 64 words, one word per 32-row pass) and their count.
// ivf_range_offsets turns the counts, in slot order = (query, probe, chunk) order, into slot offsets, per-pair limits
// and lims; ivf_range_fill walks each slot's bitmask — a row's rank is the popcount before it — and writes (distance,
// id) at offset + rank, recomputing the distance in the same direct form (rerank_rows4 and its butterfly: the same
// bits the scan compared, and the bits the exact top-k forms return).  Every mask word has exactly one writer, so the
// result is the same bits in the same order on every run.
//
// ivf_range_scan_h — the threshold scan over the tiled fp16 image of form 6 (ivf_mfma.hip: [pass][32-dim super-step]
// [row tile][lane (g, m)][8 halves]) with the queries' prepared high fp16 term (ivf_split_queries_h).  A block of 8
// waves owns an item: the item's queries' terms sit in LDS ([query][super-step][g][4 dwords], stride ≡ 8 mod 64
// dwords), wave w streams the chunk's passes w, w + 8, ... through a register ring of 6 super-steps (two 1 KiB
// wave loads each) and holds a 16-query × 32-row accumulator per query tile (v_mfma_f32_16x16x32_f16, up to 6 tiles =
// 96 queries).  Epilogue per pass, in registers: with v = a_q·acc + ‖x‖² (a_q = −2/(t·s); IP: a_q = −1/(t·s), no row
// term) a row survives unless v > c_q — one fma and one compare per accumulator element against the per-query
// constants (a_q, c_q) the lanes hold in registers, then one ballot; a pass without a survivor touches no LDS and no
// fp32 row.  Survivors are rechecked in place by the whole wave in the direct form and admitted only under the
// strict comparison; lane q mod 64 keeps query q's word of the pass and stores it after the pass.
//
// The constant c_q = (radius + E) − ‖q‖² (IP: E − radius), from ivf_range_query_prep.  E is the bound ivf_rerank_topk
// proves for this image (its rxmax >= 0 branch with the query's own split residual), restated.  Let q̂ = h/t be the
// query's high fp16 term and x̂ the image row, both unscaled; rq = ‖q̂ − q‖ (the one-term residual the preparation
// measured), ‖x̂ − x‖ ≤ rxmax (half_rxmax: measured when the image is built, a running maximum over adds, kept over
// removes) and ‖x‖² ≤ xmax2 for every row.  The scales t and s are powers of two, so acc/(t·s) is the fp32-accumulated
// q̂·x̂ exactly.  Then
//   |q̂·x̂ − q·x| ≤ ‖q‖·rxmax + rq·(√xmax2 + rxmax)                                          (Cauchy-Schwarz)
//   |acc/(t·s) − q̂·x̂| ≤ 2d·2⁻²⁴·(‖q‖ + rq)·(√xmax2 + rxmax)                  (fp32 accumulation of exact products)
//   |v + ‖q‖² − dist|, |direct-form fp32 value − dist| and the fp32 roundings of ‖q‖², ‖x‖² ≤ (d + 8)·2⁻²⁴·2(‖q‖² + xmax2)
// E = 1.01·((L2: 2, IP: 1)·(first two lines) + third line) + 2⁻²²·(‖q‖² + xmax2); the last term covers the roundings of
// radius + E and of c_q (each ≤ 2⁻²⁴ of a magnitude that, wherever a row can lie within E of the radius, is ≤
// 2(‖q‖² + xmax2) + E).  Proof obligations: (1) half_rxmax and xmax2 bound every live row of the shard; (2) the image is
// the fp16 rounding (subnormals flushed) of the rows the recheck reads, and the residuals were measured against exactly
// that rounding; (3) a non-finite E (a query the preparation could not scale, non-finite entries, an overflowing
// norm) gives c_q = +inf, and the test is the negated `v > c_q`, so a NaN on either side keeps the row: every row is
// rechecked; (4) rows past the list's live length and queries past the item's count are masked, never compared.  So
// the filter only ever adds rows to be rechecked: a row the direct form admits has v + ‖q‖² within E of its direct-form
// value and survives.  Nothing here is tuned from data.
//
// ivf_range_direct — shards without a usable image (a non-finite code, a scale outside the fp16 form's range, a
// dimension the image scan does not hold): one block of 4 waves per (query, probe, chunk) slot, wave w over the
// chunk's passes w, w + 4, ..., four rows at a time through rerank_rows4 — the rows are read with lane-contiguous
// dword loads (256 B per wave instruction, sixteen in flight), which is what keeps the sum order, and so the bits,
// those of the recheck and of the fill.  It writes the same mask words and counts; offsets and fill are shared.
//
// Every kernel reads list_len, never list_off[l + 1]: the zero-filled append slack is never scanned, and a chunk past
// a list's end or an empty list owns no slot.
#include "ivf_range_dev.hpp"
#include "rerank_rows.hpp"
#include "runtime.hpp"

#include <algorithm>

namespace hipann {

typedef float rv_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 rv_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned rv_u32x4 __attribute__((ext_vector_type(4)));

constexpr int RV_W = 8;         // waves per scan block
constexpr int RV_P = 6;         // super-steps in flight per wave
constexpr int RV_QT = 6;        // query tiles of an item (96 queries)
constexpr size_t RV_LDS_MAX = 160 * 1024;

__host__ __device__ inline int rv_stride(int nsup) { return nsup * 16 + 8; }

// Per query: (a_q, c_q) of the header, from the query's own ‖q‖², the split residual rq the preparation measured and
// the shard's row terms.  One wave per query.
template <bool IP>
__global__ void __launch_bounds__(256)
ivf_range_query_prep(const float *__restrict__ Q, int64_t nq, int d, float radius, float xmax2, float rxmax,
                     const float *__restrict__ its, const float *__restrict__ rq1, float2 *__restrict__ par) {
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int lane = threadIdx.x & 63;
    const float *qp = Q + q * (int64_t)d;
    float qq = 0.f;
    for (int e = lane; e < d; e += 64) qq = fmaf(qp[e], qp[e], qq);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) qq += __shfl_xor(qq, o);
    const float qn = sqrtf(qq), rq = rq1[q], xh = sqrtf(xmax2) + rxmax;
    const float g = (float)(2 * d) * 0x1p-24f;
    const float eip = qn * rxmax + rq * xh + g * (qn + rq) * xh;
    const float E = 1.01f * ((IP ? 1.f : 2.f) * eip + (float)(d + 8) * 0x1p-24f * 2.f * (qq + xmax2)) +
                    0x1p-22f * (qq + xmax2);
    float c = IP ? E - radius : (radius + E) - qq;
    if (!(E <= 3.4e38f)) c = __builtin_inff();
    if (lane == 0) par[q] = make_float2(IP ? -its[q] : -2.f * its[q], c);
}

// The recheck's and the fill's direct-form value of up to four rows against one query (whole wave; every lane
// returns the same sums).
template <bool IP>
__device__ __forceinline__ void rv_direct4(const float *__restrict__ qp, const float *const (&xr)[4], int d, int lane,
                                           float (&out)[4]) {
    float a4[4] = {0.f, 0.f, 0.f, 0.f};
    rerank_rows4<IP>(qp, xr, d, lane, a4);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        float a = a4[u];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        out[u] = a;
    }
}

// One wave's share of an item: passes wave, wave + RV_W, ... of rows [r0, r1).
template <int QT, bool IP>
__device__ __forceinline__ void rv_item(int d, int nsup, const uint4 *__restrict__ codes_h, int64_t tp0,
                                        const float *__restrict__ xn, int64_t r0, int64_t r1, int nqi,
                                        const unsigned *__restrict__ qs, const float2 *__restrict__ qpar,
                                        const int *__restrict__ bucket, int boff, int nprobe,
                                        const int *__restrict__ slot_off, int chunk, const float *__restrict__ Q,
                                        const float *__restrict__ codes, float radius, unsigned *__restrict__ mask,
                                        int *__restrict__ counts, int *red, unsigned long long *__restrict__ stat) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, g = lane >> 4;
    const int stride = rv_stride(nsup);
    const int npass_all = (int)ceil_div(r1 - r0, 32);
    const int npass = npass_all > wave ? (npass_all - wave + RV_W - 1) / RV_W : 0;
    const int ilast = npass > 0 ? npass - 1 : 0;

    // the row stream: unconditional loads (past the wave's last super-step they re-read it), so every iteration has
    // the same count of vector-memory operations in flight
    const uint4 *rp = codes_h;
    int ld_i = 0, ld_s = 0;
    auto set_pass = [&](int i) { rp = codes_h + ((tp0 + wave + RV_W * i) * nsup) * 128 + lane; };
    auto next_load = [&](uint4 (&dst)[2]) {
        const int s = ld_i <= ilast ? ld_s : nsup - 1;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const rv_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const rv_u32x4 *>(rp + (int64_t)s * 128 + r * 64));
            dst[r] = make_uint4(v[0], v[1], v[2], v[3]);
        }
        if (++ld_s == nsup) {
            ld_s = 0;
            ++ld_i;
            set_pass(ld_i <= ilast ? ld_i : ilast);
        }
    };
    auto row_of = [&](int i, int r) -> int64_t {
        const int64_t row = r0 + (int64_t)(wave + RV_W * i) * 32 + 16 * r + m;
        return row < r1 ? row : r1 - 1;
    };

    uint4 ring[RV_P][2];
    float xnr[2] = {0.f, 0.f};
    if (npass > 0) {
        set_pass(0);
#pragma unroll
        for (int p = 0; p < RV_P; ++p) next_load(ring[p]);
        if (!IP) {
#pragma unroll
            for (int r = 0; r < 2; ++r) xnr[r] = xn[row_of(0, r)];
        }
    }
    // the item's query image and constants were written by every thread before the call: wait for them only now, with
    // this wave's first super-steps of rows in flight (an LDS-only wait: the row loads stay outstanding)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // this lane's queries: qt·16 + 4g + v — constants in registers, validity as a bit per (qt, row tile, v)
    float pa[QT][4], pc[QT][4];
    uint64_t valid = 0;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int q = qt * 16 + 4 * g + v;
            const float2 p = qpar[q < nqi ? q : 0];
            pa[qt][v] = p.x;
            pc[qt][v] = p.y;
            if (q < nqi) valid |= (uint64_t)0x11u << (qt * 8 + v);
        }
    const unsigned *qrow[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) qrow[qt] = qs + (qt * 16 + m) * stride + 4 * g;
    // lane j keeps the mask words of the item's queries j and j + 64
    int64_t sb0 = 0, sb1 = 0;
    if (lane < nqi) sb0 = ((int64_t)slot_off[bucket[boff + lane]] + chunk) * RV_WORDS;
    if (lane + 64 < nqi) sb1 = ((int64_t)slot_off[bucket[boff + lane + 64]] + chunk) * RV_WORDS;
    int cnt0 = 0, cnt1 = 0;
    unsigned nsurv = 0, nadm = 0;

    rv_f32x4 acc[QT][2];
    for (int i = 0; i < npass; ++i) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int r = 0; r < 2; ++r) acc[qt][r] = rv_f32x4{0.f, 0.f, 0.f, 0.f};
        float xnr_next[2] = {0.f, 0.f};
        if (!IP) {
#pragma unroll
            for (int r = 0; r < 2; ++r) xnr_next[r] = xn[row_of(i + 1 <= ilast ? i + 1 : ilast, r)];
        }
        for (int S0 = 0; S0 < nsup; S0 += RV_P) {
#pragma unroll
            for (int p = 0; p < RV_P; ++p) {
                const int S = S0 + p;
                uint4 qa[QT];
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) qa[qt] = *reinterpret_cast<const uint4 *>(qrow[qt] + S * 16);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                    for (int r = 0; r < 2; ++r)
                        acc[qt][r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(rv_f16x8, qa[qt]),
                                                                            __builtin_bit_cast(rv_f16x8, ring[p][r]),
                                                                            acc[qt][r], 0, 0, 0);
                next_load(ring[p]);
            }
        }
        const int pi = wave + RV_W * i;
        const int64_t prow0 = r0 + (int64_t)pi * 32;
        // bit qt·8 + 4r + v of sm: query qt·16 + 4g + v against row 16r + m of the pass survives the filter
        uint64_t sm = 0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const bool rok = prow0 + 16 * r + m < r1;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const bool s = rok && !(fmaf(pa[qt][v], acc[qt][r][v], xnr[r]) > pc[qt][v]);
                    sm |= (uint64_t)(s ? 1u : 0u) << (qt * 8 + 4 * r + v);
                }
        }
        sm &= valid;
        unsigned w0 = 0, w1 = 0;
        if (__ballot(sm != 0) != 0ull) {
            // the recheck: for every (query tile, row tile, v) with a survivor and each of its four queries (one per
            // 16-lane group), the rows in ascending order, four at a time, by the whole wave
            for (int b = 0; b < QT * 8; ++b) {
                const uint64_t bal = __ballot((sm >> b) & 1ull);
                if (bal == 0ull) continue;
                const int qt = b >> 3, r = (b >> 2) & 1, v = b & 3;
                for (int gg = 0; gg < 4; ++gg) {
                    unsigned bits = (unsigned)(bal >> (16 * gg)) & 0xffffu;
                    if (!bits) continue;
                    const int ql = qt * 16 + 4 * gg + v;
                    const float *qp = Q + (int64_t)(bucket[boff + ql] / nprobe) * d;
                    while (bits) {
                        int rb[4];
                        bool ok[4];
                        const float *xr[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            ok[u] = bits != 0;
                            if (ok[u]) {
                                rb[u] = 16 * r + __builtin_ctz(bits);
                                bits &= bits - 1;
                            } else {
                                rb[u] = rb[0];
                            }
                            xr[u] = codes + (prow0 + rb[u]) * (int64_t)d;  // (a survivor's row is below r1)
                        }
                        float a4[4];
                        rv_direct4<IP>(qp, xr, d, lane, a4);
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const bool pass = ok[u] && (IP ? a4[u] > radius : a4[u] < radius);
                            nsurv += ok[u];
                            nadm += pass;
                            if (pass && lane == (ql & 63)) {
                                if (ql < 64) w0 |= 1u << rb[u];
                                else w1 |= 1u << rb[u];
                            }
                        }
                    }
                }
            }
        }
        if (lane < nqi) mask[sb0 + pi] = w0;
        if (lane + 64 < nqi) mask[sb1 + pi] = w1;
        cnt0 += __popc(w0);
        cnt1 += __popc(w1);
#pragma unroll
        for (int r = 0; r < 2; ++r) xnr[r] = xnr_next[r];
    }

    // the slots' counts: the waves' per-query sums through LDS (the query image is no longer read)
    __syncthreads();
    red[wave * (16 * RV_QT) + lane] = cnt0;
    if (lane < 32) red[wave * (16 * RV_QT) + 64 + lane] = cnt1;
    __syncthreads();
    for (int q = threadIdx.x; q < nqi; q += 64 * RV_W) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < RV_W; ++w) c += red[w * (16 * RV_QT) + q];
        counts[slot_off[bucket[boff + q]] + chunk] = c;
    }
    if (stat && lane == 0 && nsurv) {
        atomicAdd(stat, (unsigned long long)nsurv);
        atomicAdd(stat + 1, (unsigned long long)nadm);
    }
}

template <bool IP>
__global__ void __launch_bounds__(64 * RV_W, RV_W / 4)
ivf_range_scan_h(const uint4 *__restrict__ qsplit, const float2 *__restrict__ par, int d, int nsup,
                 const uint4 *__restrict__ codes_h, const int64_t *__restrict__ tpass_off, const float *__restrict__ xn,
                 const int64_t *__restrict__ list_off, const int *__restrict__ list_len, const int *__restrict__ cnt,
                 const int *__restrict__ bucket_off, const int *__restrict__ item_off, const int *__restrict__ bucket,
                 const int *__restrict__ slot_off, int nlist, int nprobe, int group, const float *__restrict__ Q,
                 const float *__restrict__ codes, float radius, unsigned *__restrict__ mask, int *__restrict__ counts,
                 unsigned long long *__restrict__ stat) {
    extern __shared__ __attribute__((aligned(16))) float smem_rv[];
    const int total = item_off[nlist];
    if ((int)blockIdx.x >= total) return;
    const int item = xcd_remap((int)blockIdx.x, total);
    const int l = ivf_phase_list(0, item_off, nullptr, nlist, item);
    const int64_t lr0 = list_off[l], lr1 = lr0 + list_len[l];
    const int c = cnt[l];
    const int ng = ivf_ngroups(c, group);
    int chunk, grp;
    ivf_phase_decode(0, item - item_off[l], ng, chunk, grp);
    const int q_begin = (int)((int64_t)grp * c / ng), q_end = (int)((int64_t)(grp + 1) * c / ng);
    const int nqi = q_end - q_begin;
    const int64_t r0 = lr0 + (int64_t)chunk * RV_CH;
    const int64_t r1 = r0 + RV_CH < lr1 ? r0 + RV_CH : lr1;
    const int boff = bucket_off[l] + q_begin;
    const int nqt = (nqi + 15) >> 4;
    const int64_t tp0 = tpass_off[l] + (int64_t)chunk * RV_WORDS;

    // LDS: the queries' high terms [query][super-step][g][4 dwords], then (a_q, c_q) per query
    unsigned *qs = reinterpret_cast<unsigned *>(smem_rv);
    const int stride = rv_stride(nsup);
    float2 *qpar = reinterpret_cast<float2 *>(qs + nqi * stride);
    const int per_q = nsup * 4;
    for (int t = threadIdx.x; t < nqi * per_q; t += 64 * RV_W) {
        const int q = t / per_q, r2 = t - q * per_q;
        const int gq = bucket[boff + q] / nprobe;
        *reinterpret_cast<uint4 *>(qs + q * stride + r2 * 4) = qsplit[(int64_t)gq * 2 * per_q + r2];
    }
    for (int t = threadIdx.x; t < nqi; t += 64 * RV_W) qpar[t] = par[bucket[boff + t] / nprobe];
    // (no barrier here: rv_item waits for the fill after issuing its first row loads)
    int *red = reinterpret_cast<int *>(smem_rv);
#define RV_CASE(QTV)                                                                                              \
    rv_item<QTV, IP>(d, nsup, codes_h, tp0, xn, r0, r1, nqi, qs, qpar, bucket, boff, nprobe, slot_off, chunk, Q, \
                     codes, radius, mask, counts, red, stat);
    switch (nqt) {
    case 0: case 1: RV_CASE(1) break;
    case 2: RV_CASE(2) break;
    case 3: RV_CASE(3) break;
    case 4: RV_CASE(4) break;
    case 5: RV_CASE(5) break;
    default: RV_CASE(6) break;
    }
#undef RV_CASE
}

// The direct form: one block of 4 waves per slot, the same mask words and count as the image scan.
template <bool IP>
__global__ void __launch_bounds__(256)
ivf_range_direct(const float *__restrict__ Q, int d, const float *__restrict__ codes, const int64_t *__restrict__ probes,
                 int64_t npairs, int nprobe, int max_nch, const int64_t *__restrict__ list_off,
                 const int *__restrict__ list_len, int nlist, const int *__restrict__ slot_off, float radius,
                 unsigned *__restrict__ mask, int *__restrict__ counts) {
    __shared__ int red[4];
    int64_t pair, r0, r1;
    int slot;
    if (!rv_slot(blockIdx.x, max_nch, npairs, probes, list_off, list_len, nlist, slot_off, pair, slot, r0, r1)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *qp = Q + (pair / nprobe) * (int64_t)d;
    const int npass = (int)ceil_div(r1 - r0, 32);
    int cnt = 0;
    for (int pi = wave; pi < npass; pi += 4) {
        unsigned w = 0;
        for (int j = 0; j < 32; j += 4) {
            const int64_t row0 = r0 + (int64_t)pi * 32 + j;
            if (row0 >= r1) break;
            const float *xr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) xr[u] = codes + (row0 + u < r1 ? row0 + u : row0) * (int64_t)d;
            float a4[4];
            rv_direct4<IP>(qp, xr, d, lane, a4);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (row0 + u < r1 && (IP ? a4[u] > radius : a4[u] < radius)) w |= 1u << (j + u);
        }
        if (lane == 0) mask[(int64_t)slot * RV_WORDS + pi] = w;
        cnt += __popc(w);
    }
    if (lane == 0) red[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[slot] = red[0] + red[1] + red[2] + red[3];
}

// Exclusive scan of the S = slot_off[npairs] slot counts (slot order = (query, probe, chunk) order) into soff
// (soff[S] = the total), in runs of 4096 with a carry; then plim[i] = soff[slot_off[i]] for the npairs + 1 pair
// boundaries and lims[q] = plim[q·nprobe].  chain: everything starts at lims[0] as the previous query slice left it.
__global__ void __launch_bounds__(1024)
ivf_range_offsets(const int *__restrict__ counts, const int *__restrict__ slot_off, int64_t npairs, int nprobe,
                  int chain, int64_t *__restrict__ soff, int64_t *__restrict__ plim, int64_t *__restrict__ lims) {
    __shared__ long long wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t S = slot_off[npairs];
    long long carry = chain ? lims[0] : 0;
    __syncthreads();
    for (int64_t b = 0; b < S; b += 4096) {
        const int64_t i0 = b + 4 * (int64_t)tid;
        long long v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i0 + u < S ? counts[i0 + u] : 0;
        const long long mine = v[0] + v[1] + v[2] + v[3];
        long long inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
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
        long long ex = carry + before + inc - mine;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u < S) soff[i0 + u] = ex;
            ex += v[u];
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) soff[S] = carry;
    __syncthreads();  // (one block: its own global writes are visible to it after the barrier)
    for (int64_t i = tid; i <= npairs; i += 1024) {
        const long long e = soff[slot_off[i]];
        plim[i] = e;
        if (i % nprobe == 0) lims[i / nprobe] = e;
    }
}

// One wave per slot: the admitted rows' (distance, id) at soff[slot] + rank, rank = the set bits before the row's.
template <bool IP>
__global__ void __launch_bounds__(256)
ivf_range_fill(const float *__restrict__ Q, int d, const float *__restrict__ codes, const int64_t *__restrict__ ids,
               const int64_t *__restrict__ probes, int64_t npairs, int nprobe, int max_nch,
               const int64_t *__restrict__ list_off, const int *__restrict__ list_len, int nlist,
               const int *__restrict__ slot_off, const unsigned *__restrict__ mask, const int *__restrict__ counts,
               const int64_t *__restrict__ soff, float *__restrict__ D, int64_t *__restrict__ I) {
    int64_t pair, r0, r1;
    int slot;
    const int lane = threadIdx.x & 63;
    if (!rv_slot((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), max_nch, npairs, probes, list_off, list_len, nlist,
                 slot_off, pair, slot, r0, r1))
        return;
    if (counts[slot] == 0) return;
    const float *qp = Q + (pair / nprobe) * (int64_t)d;
    const int npass = (int)ceil_div(r1 - r0, 32);
    const unsigned word = lane < npass ? mask[(int64_t)slot * RV_WORDS + lane] : 0u;
    int inc = __popc(word);
    const int own = inc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    const int before = inc - own;
    const int64_t base = soff[slot];
    for (int pi = 0; pi < npass; ++pi) {
        unsigned bits = (unsigned)__shfl((int)word, pi);
        int64_t pos = base + __shfl(before, pi);
        while (bits) {
            int64_t row[4];
            const float *xr[4];
            int n = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (bits) {
                    row[u] = r0 + (int64_t)pi * 32 + __builtin_ctz(bits);
                    bits &= bits - 1;
                    ++n;
                } else {
                    row[u] = row[0];
                }
                xr[u] = codes + row[u] * (int64_t)d;
            }
            float a4[4];
            rv_direct4<IP>(qp, xr, d, lane, a4);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (u < n && lane == u) {
                    D[pos + u] = a4[u];
                    I[pos + u] = ids[row[u]];
                }
            pos += n;
        }
    }
}

// ------------------------------------------------------------------------------------------------
void launch_ivf_range_query_prep(const float *Q, int64_t nq, int d, int metric, float radius, float xmax2, float rxmax,
                                 const float *its, const float *rq1, void *par, hipStream_t st) {
    if (nq <= 0) return;
    const dim3 grid((unsigned)ceil_div(nq, 4)), block(256);
    float2 *p = static_cast<float2 *>(par);
    if (metric == kIP)
        hipLaunchKernelGGL(ivf_range_query_prep<true>, grid, block, 0, st, Q, nq, d, radius, xmax2, rxmax, its, rq1, p);
    else hipLaunchKernelGGL(ivf_range_query_prep<false>, grid, block, 0, st, Q, nq, d, radius, xmax2, rxmax, its, rq1, p);
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_range_scan_h(const IvfRangeArgs &a, const IvfPlanView &plan, int64_t max_items, hipStream_t st) {
    if (max_items <= 0 || a.nq <= 0) return;
    HIPANN_REQUIRE(ivf_chunk_rows() == RV_CH, "IVF range scan: chunks of 2048 rows");
    HIPANN_REQUIRE(max_items < (int64_t)0x7fffffff, "too many IVF work items");
    HIPANN_REQUIRE(a.qsplit && a.par && a.codes_h && a.tpass_off && a.mask && a.counts, "IVF range scan: missing buffers");
    HIPANN_REQUIRE(a.metric == kIP || a.xn, "IVF range scan: L2 needs the row norms");
    const int nsup = (int)(ivf_half_pass_bytes(a.d) / (2 * 64 * 16));
    HIPANN_REQUIRE(nsup > 0 && nsup % RV_P == 0, "IVF range scan: the image's super-steps come in runs of 6");
    const int group = ivf_mfma_h_group(a.d), wide = ivf_group_wide(group);
    HIPANN_REQUIRE(wide >= 16 && wide <= 16 * RV_QT && ivf_group_narrow(group) == 0, "IVF range scan: unsupported group");
    const size_t smem = std::max((size_t)wide * ((size_t)rv_stride(nsup) * 4 + 8), (size_t)RV_W * 16 * RV_QT * sizeof(int));
    HIPANN_REQUIRE(smem <= RV_LDS_MAX, "IVF range scan: LDS image too large");
    const dim3 grid((unsigned)max_items), block(64 * RV_W);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, smem, st, static_cast<const uint4 *>(a.qsplit),
                           static_cast<const float2 *>(a.par), a.d, nsup, static_cast<const uint4 *>(a.codes_h),
                           a.tpass_off, a.xn, HIPANN_PLAN_ARGS(plan), group, a.Q, a.codes, a.radius, a.mask, a.counts,
                           a.stat);
    };
    if (a.metric == kIP) go(ivf_range_scan_h<true>);
    else go(ivf_range_scan_h<false>);
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_range_direct(const IvfRangeArgs &a, const IvfPlanView &plan, hipStream_t st) {
    const int64_t blocks = a.nq * plan.nprobe * a.max_nch;
    if (blocks <= 0) return;
    HIPANN_REQUIRE(ivf_chunk_rows() == RV_CH, "IVF range scan: chunks of 2048 rows");
    HIPANN_REQUIRE(blocks < (int64_t)0x7fffffff, "IVF range scan: too many slots");
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, st, a.Q, a.d, a.codes, a.probes,
                           a.nq * plan.nprobe, plan.nprobe, a.max_nch, plan.list_off, plan.list_len, plan.nlist,
                           plan.slot_off, a.radius, a.mask, a.counts);
    };
    if (a.metric == kIP) go(ivf_range_direct<true>);
    else go(ivf_range_direct<false>);
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_range_offsets(const int *counts, const int *slot_off, int64_t nq, int nprobe, bool chain, int64_t *soff,
                              int64_t *plim, int64_t *lims, hipStream_t st) {
    hipLaunchKernelGGL(ivf_range_offsets, dim3(1), dim3(1024), 0, st, counts, slot_off, nq * nprobe, nprobe,
                       chain ? 1 : 0, soff, plim, lims);
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_range_fill(const IvfRangeArgs &a, const IvfPlanView &plan, const int64_t *ids, const int64_t *soff,
                           float *D, int64_t *I, hipStream_t st) {
    const int64_t waves = a.nq * plan.nprobe * a.max_nch;
    if (waves <= 0) return;
    HIPANN_REQUIRE(ceil_div(waves, 4) < (int64_t)0x7fffffff, "IVF range fill: too many slots");
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div(waves, 4)), dim3(256), 0, st, a.Q, a.d, a.codes, ids, a.probes,
                           a.nq * plan.nprobe, plan.nprobe, a.max_nch, plan.list_off, plan.list_len, plan.nlist,
                           plan.slot_off, a.mask, a.counts, soff, D, I);
    };
    if (a.metric == kIP) go(ivf_range_fill<true>);
    else go(ivf_range_fill<false>);
    HIPANN_CHECK(hipGetLastError());
}

}  // namespace hipann
