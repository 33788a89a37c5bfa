// ivf_sq8.hip — IVF SQ8 (faiss::IndexIVFScalarQuantizer, QT_8bit): the kernels behind hipann_ivfsq_*.
//
// A row of list l is the codes c (one byte per dimension) and stands for x̂ = g + dec, g = g_l (by_residual) or 0,
// dec_i = vmin_i + ((float)c_i + 0.5f) / 255.0f * vdiff_i in fp32, in this order.  The distance returned is the direct
// form in fp32 over the decoded row — L2: Σ (t_i − dec_i)², t = q − g; IP: q·g + Σ q_i·dec_i — and sq_row_dist is the
// one device function that computes it, for the rerank and for the direct kernel: a row carries the same bits
// whichever path returned it.
//
// The scan never decodes.  With s = vdiff/255, b = vmin + s/2 (fp32, fixed at create): x̂ = g + b + s∘c and
//   L2: ‖q − x̂‖² = A(q,l) + N(row) − 2·u_q·c,  u_q = (q − b)∘s,  A = ‖q − g − b‖²,  N = ‖s∘c‖² + 2 g·(s∘c)
//   IP: q·x̂ = P(q,l) + u_q·c,                    u_q = q∘s,        P = q·(g + b)
// so the only large product is a per-query vector against the raw codes, whatever the list.
//
// Layout.  The codes are kept only tiled: per list, 32-row passes; per pass, nstep 32-dim K steps (d padded with zero
// codes to 4 steps up to d = 128, to 8 steps above); per step 1 KiB = [lane (g = lane >> 4, m = lane & 15)][row tile
// r][8 bytes]: the bytes of row 16r + m, dims 32·step + 8g .. + 7 — a lane's 16-byte load is its B operand of both row
// tiles of v_mfma_f32_16x16x32_f16.
//
// ivf_sq_scan — the hot path, list-major over the plan's items (list, 2048-row chunk, group of (query, probe) pairs).
// A block of 8 waves owns an item.  LDS: the group's query terms, ONE fp16 term û = fp16(u·t)/t per query (t a power
// of two; [query][step][g][8 halves], stride nstep·16 + 8 dwords), and one 16-entry sorted (key, row) list per (wave,
// query).  Wave w streams passes w, w + 8, ... of the chunk through a register ring of P steps (P = 4 or 8 wave loads
// of 1 KiB in flight), turns each dword of four codes into two dwords of exact fp16 — v_perm_b32 to 0x6400 | c, which
// is 1024 + c, and a packed fp16 subtract of 1024 — and accumulates 16 queries × 32 rows per query tile (up to 4
// tiles).  One term, not two: a code is exact in fp16, so the only rounding is the query's; its measured residual
// enters the bound below, and the rerank reads every candidate within the bound of the k-th key, so a looser key costs
// more rows to recheck (measured: 369 per query for k = 10 at 2M x 768; the two-term variant was never built, so the
// trade is argued, not measured) while the second term would double the matrix-core work and the LDS image (48 instead of
// 32 queries per item at d = 768).  Epilogue per pass: key = A + N − 2·acc/t (IP: −(P + acc/t); smaller is better
// throughout), admitted when key <= thr, thr = min(the wave list's 16th key, B_q + 2E_q) with B_q the smallest 16th
// key any wave has published for the query (an atomic min on order-preserving bits, re-read every pass).  An
// admitted key is inserted by the whole wave (one ballot, one popcount, one shuffle).  At the item's end every wave
// writes its lists to the (slot, wave) sub-lists of the slot = (query, probe, chunk).
//
// ivf_sq_rerank — one wave per query, k <= 16.  τ = the k-th smallest key of the query's sub-lists; every candidate
// with key <= τ + 2E is recomputed by sq_row_dist and the k best by (distance, id) are returned.
//
// The certificate.  E(q) bounds |key − dist| for every probed row, dist the direct-form fp32 value:
//   |û·c − u·c| <= rq·cmax, rq = ‖u − û‖ measured by the preparation, cmax >= ‖c‖ of every row   (Cauchy-Schwarz)
//   |acc/t − û·c| <= 2·32·nstep·2⁻²⁴·(‖u‖ + rq)·cmax              (fp32 accumulation of exact products; t = 2^e)
//   the fp32 roundings of s, b, u, A or P, N, the key's two additions, the decode and the direct form's d terms, each
//   a few 2⁻²⁴ of products of magnitudes <= W = ‖q‖ + max‖g_l‖ + ‖(|vmin_i| + |vdiff_i|·256/255)_i‖:  <= (d + 16)·2⁻²²·W²
//   E = 1.01·(2·(first two lines) + third line).
// Proof obligations: (1) cmax and max‖g_l‖ are maxima over every row and list of the index (taken at create; an add
// raises cmax by its rows' ‖c‖ before it returns, ivf_sq8_build.hip, a removal keeps it — an upper bound is all the
// first line needs, and a maximum over a superset of the rows held is one, ivf_sq8_remove.hip — and the centroids
// never change); (2) a row is dropped only (a) against B_q + 2E at a time when some wave list held 16 rows with key <= B_q,
// which it still holds or has replaced by better ones at the end, so τ <= B_q for k <= 16 and the row's key > τ + 2E;
// or (b) from a full wave list, with key >= that list's final 16th key; the rerank flags the query unless every full
// sub-list's 16th key is > τ + 2E.  Then every dropped row has key > τ + 2E, so dist > τ + E, while the k rows with
// the smallest keys have dist <= τ + E: no dropped row is among the k best, and every kept row that is has key <=
// τ + 2E and is rechecked; (3) the comparisons are written so that a NaN key is never admitted and a NaN or
// non-finite E flags the query; (4) rows past the list's length and queries past the item's count are masked.
//
// The deep variant, 17 <= k <= 64.  sq_item / ivf_sq_scan / ivf_sq_rerank are templates on the depth KF of the wave
// lists: KF = 16 is the kernel above, KF = 32 keeps a (wave, query) list in lanes 0..31 (insertion is still one
// ballot, one popcount, one shuffle), a slot holds 8 sub-lists of 32, and the LDS per query is sq_stride·4 + 16 +
// 8·KF·8 bytes (d = 768: 32 queries per item instead of 48; d <= 128: 64 still; above d = 3840 not even 16 fit).
// One published 32nd key no longer bounds the k-th key when k > 32, so the wave lists are split into
// J = ceil(k / KF) classes, class = wave % J, with one published word per (query, class): the shard's qbound for
// class 0, qbound2 (the handle's own, reset to +inf by ivf_sq_query_prep) for class 1.  A full list min's its KF-th
// key into its class's word; the gate is B_q = the max of the J words, +inf until every class has published.
// Obligation (2a), amended: the list that attains a class's word held KF rows with key <= that word at that time,
// and holds them or better ones at the end.  Lists of different classes are different lists, and their rows are
// distinct — a row belongs to one pass, a pass to one wave, and a slot to exactly one item.  So at least
// J·KF >= k distinct rows have key <= B_q at the end, hence τ <= B_q, and a row dropped at the gate has key >
// τ + 2E.  (2b) with 16 replaced by KF: a row leaves a full wave list only with key >= that list's final KF-th key,
// and the rerank flags the query unless every full sub-list's KF-th key is > τ + 2E.  (3) and (4) are unchanged.  The
// rerank stays one wave per query: WaveList<1> holds 64 entries, so τ and the result list serve k <= 64.
//
// Flagged queries, k above 64 and dimensions whose query terms do not fit the LDS (d > 4352; for 17 <= k <= 64,
// d > 3840) take ivf_sq_direct: sq_row_dist over all rows of the probed lists, one wave per slot, with no host
// readback in between.
//
// Resources (hipcc 7, gfx950, -O3): see DESIGN.md §5; no kernel here uses scratch.
#include "runtime.hpp"
#include "ivf_sq8_dev.hpp"
#include "wave_topk.hpp"

#include <algorithm>

namespace hipann {

constexpr int SQ_W = kSqWaves;
constexpr int SQ_KF = kSqKeep;
constexpr int SQ_KD = kSqDeep;  // the deep variant's depth (17 <= k <= 64)
constexpr int SQ_CH = 2048;  // rows per chunk (ivf_chunk_rows)
constexpr int SQ_QT = 4;     // query tiles of an item at most
constexpr size_t SQ_LDS_MAX = 160 * 1024;
constexpr int SQ_PAD_ROW = 0x7fffffff;

int ivf_sq_nstep(int d) {
    const int raw = (d + 31) / 32, p = raw <= 4 ? 4 : 8;
    return (raw + p - 1) / p * p;
}
static size_t sq_lds_bytes(int nstep, int nq, int kf) {
    return (size_t)nq * ((size_t)sq_stride(nstep) * 4 + 16 + (size_t)SQ_W * kf * 8);
}
int ivf_sq_group(int d, int kf) {
    const int nstep = ivf_sq_nstep(d);
    int qt = SQ_QT;
    while (qt > 0 && sq_lds_bytes(nstep, 16 * qt, kf) > SQ_LDS_MAX) --qt;
    return 16 * qt;
}

// ---- create time ----------------------------------------------------------------------------------------------
// one block per pass: row-major codes -> the pass's tiled bytes (rows past the list and dims past d: code 0)
__global__ void __launch_bounds__(256)
ivf_sq_tile(const unsigned char *__restrict__ codes, const int64_t *__restrict__ list_off,
            const int *__restrict__ list_len, const int64_t *__restrict__ tpass_off, int nlist, int d, int nstep,
            unsigned char *__restrict__ dst) {
    const int64_t pass = blockIdx.x;
    int lo = 0, hi = nlist - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tpass_off[mid] <= pass) lo = mid; else hi = mid - 1;
    }
    const int64_t r0 = list_off[lo] + (pass - tpass_off[lo]) * 32, r1 = list_off[lo] + list_len[lo];
    unsigned char *out = dst + pass * (int64_t)nstep * 1024;
    for (int t = threadIdx.x; t < 32 * nstep * 32; t += 256) {
        const int rr = t / (nstep * 32), e = t - rr * (nstep * 32);
        out[sq_tile_off(rr, e)] = (r0 + rr < r1 && e < d) ? codes[(r0 + rr) * (int64_t)d + e] : (unsigned char)0;
    }
}

// one block per pass: the pass's live rows -> row-major codes and labels at out_off[list] + the row's place in its list
// (out_off = the dense offsets: the export of lists that carry append slack); codes or ids_out may be null
__global__ void __launch_bounds__(256)
ivf_sq_untile(const unsigned char *__restrict__ src, const int64_t *__restrict__ list_off,
              const int *__restrict__ list_len, const int64_t *__restrict__ tpass_off,
              const int64_t *__restrict__ out_off, const int64_t *__restrict__ ids, int nlist, int d, int nstep,
              unsigned char *__restrict__ codes, int64_t *__restrict__ ids_out) {
    const int64_t pass = blockIdx.x;
    int lo = 0, hi = nlist - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tpass_off[mid] <= pass) lo = mid; else hi = mid - 1;
    }
    const int64_t rel = (pass - tpass_off[lo]) * 32, o0 = out_off[lo] + rel;
    const int64_t left = (int64_t)list_len[lo] - rel;
    const int live = left < 32 ? (int)left : 32;  // (<= 0: a slack pass)
    const unsigned char *in = src + pass * (int64_t)nstep * 1024;
    for (int t = threadIdx.x; codes && t < 32 * d; t += 256) {
        const int rr = t / d, e = t - rr * d;
        if (rr < live) codes[(o0 + rr) * (int64_t)d + e] = in[sq_tile_off(rr, e)];
    }
    if (ids_out && (int)threadIdx.x < live) ids_out[o0 + threadIdx.x] = ids[list_off[lo] + rel + threadIdx.x];
}

// one wave per row: N(row) (L2) and the running max of ‖c‖² (bits of a non-negative float order as integers)
__global__ void __launch_bounds__(256)
ivf_sq_row_terms(const unsigned char *__restrict__ codes, int64_t n, int d, const float *__restrict__ sb, int sbn,
                 const float *__restrict__ centroids, const int64_t *__restrict__ list_off, int nlist, int l2,
                 float *__restrict__ rown, unsigned *__restrict__ cmax2) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int lane = threadIdx.x & 63;
    const float *g = nullptr;
    if (centroids) {
        int lo = 0, hi = nlist - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (list_off[mid] <= row) lo = mid; else hi = mid - 1;
        }
        g = centroids + (int64_t)lo * d;
    }
    float nn = 0.f, cc = 0.f;
    for (int e = lane; e < d; e += 64) {
        const float c = (float)codes[row * (int64_t)d + e];
        const float sc = sb[e] * c;
        cc = fmaf(c, c, cc);
        nn = fmaf(sc, sc, nn);
        if (g) nn = fmaf(2.f * g[e], sc, nn);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nn += __shfl_xor(nn, o);
        cc += __shfl_xor(cc, o);
    }
    if (lane == 0) {
        if (l2) rown[row] = nn;
        atomicMax(cmax2, __float_as_uint(cc));
    }
}

// ---- per call -------------------------------------------------------------------------------------------------
// One wave per query: u, the scale t = 2^e with max|u|·t in [2^13, 2^14), the fp16 term [step][g][8 halves] (dims
// past d: 0), and par[q] = (1/t, E, 2E, ‖q‖²).
template <bool IP>
__global__ void __launch_bounds__(256)
ivf_sq_query_prep(const float *__restrict__ Q, int64_t nq, int d, int nstep, const float *__restrict__ sb, float cmax,
                  float wbase, _Float16 *__restrict__ qimg, float4 *__restrict__ par, unsigned *__restrict__ qbound2) {
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int lane = threadIdx.x & 63;
    if (qbound2 && lane == 0) qbound2[q] = 0xff800000u;  // (+inf: the deep scan's second gate class has not published)
    const float *qp = Q + q * (int64_t)d;
    const float *s = sb, *b = sb + 32 * nstep;
    float umax = 0.f, qq = 0.f, uu = 0.f;
    for (int e = lane; e < d; e += 64) {
        const float u = (IP ? qp[e] : qp[e] - b[e]) * s[e];
        umax = fmaxf(umax, fabsf(u));
        if (!(u == u)) umax = __builtin_inff();
        qq = fmaf(qp[e], qp[e], qq);
        uu = fmaf(u, u, uu);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        umax = fmaxf(umax, __shfl_xor(umax, o));
        qq += __shfl_xor(qq, o);
        uu += __shfl_xor(uu, o);
    }
    const bool fin = umax < 3.0e38f;
    int ex = 0;
    if (fin && umax > 0.f) {
        (void)frexpf(umax, &ex);  // umax = f·2^ex, f in [0.5, 1)
        ex = 14 - ex;
        ex = ex > 100 ? 100 : ex < -100 ? -100 : ex;
    }
    const float t = ldexpf(1.f, ex), it = ldexpf(1.f, -ex);
    float res = 0.f;
    _Float16 *out = qimg + q * (int64_t)nstep * 32;
    for (int e = lane; e < 32 * nstep; e += 64) {
        float ut = 0.f;
        if (e < d && fin) ut = (IP ? qp[e] : qp[e] - b[e]) * s[e] * t;
        const _Float16 h = (_Float16)ut;
        const float r = ut - (float)h;
        res = fmaf(r, r, res);
        out[e] = h;  // ([step][g][8]: dim e = 32·step + 8g + j is element e)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) res += __shfl_xor(res, o);
    const float rq = sqrtf(res) * it * 1.0001f, un = sqrtf(uu) * 1.0001f;
    const float W = sqrtf(qq) * 1.0001f + wbase;
    float E = 1.01f * (2.f * (rq * cmax + (float)(64 * nstep) * 0x1p-24f * (un + rq) * cmax) +
                       (float)(d + 16) * 0x1p-22f * W * W);
    if (!fin || !(E < 3.0e38f)) E = __builtin_inff();
    if (lane == 0) par[q] = make_float4(it, E, 2.f * E, qq);
}

// One wave per (query, probe) pair: A = Σ (q − g − b)² (L2) or P = q·(g + b) (IP), fp32.
template <bool IP>
__global__ void __launch_bounds__(256)
ivf_sq_pair_terms(const float *__restrict__ Q, int64_t npairs, int nprobe, const int64_t *__restrict__ probes, int d,
                  int nstep, int nlist, const float *__restrict__ centroids, const float *__restrict__ sb,
                  float *__restrict__ pair_a) {
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= npairs) return;
    const int lane = threadIdx.x & 63;
    const int64_t l = probes[pair];
    const float *qp = Q + (pair / nprobe) * (int64_t)d;
    const float *g = centroids && l >= 0 && l < nlist ? centroids + l * (int64_t)d : nullptr;
    const float *b = sb + 32 * nstep;
    float acc = 0.f;
    for (int e = lane; e < d; e += 64) {
        const float ge = g ? g[e] : 0.f;
        if (IP) {
            acc = fmaf(qp[e], ge + b[e], acc);
        } else {
            const float t = (qp[e] - ge) - b[e];
            acc = fmaf(t, t, acc);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) pair_a[pair] = acc;
}

// A wave-uniform candidate into the sorted KF-entry list (lk, lr) of this wave (lanes 0..KF-1 hold the entries).
template <int KF>
__device__ __forceinline__ void sq_list_insert(float *lk, int *lr, float ck, int crow, int lane) {
    const float ek = lane < KF ? lk[lane] : __builtin_inff();
    const int er = lane < KF ? lr[lane] : SQ_PAD_ROW;
    const int pos = __popcll(__ballot(lane < KF && lex_less(ek, er, ck, crow)));
    if (pos >= KF) return;
    const float pk = shfl_up1_f(ek);
    const int pr = shfl_up1_i(er);
    if (lane < KF) {
        if (lane == pos) { lk[lane] = ck; lr[lane] = crow; }
        else if (lane > pos) { lk[lane] = pk; lr[lane] = pr; }
    }
}

// KF: the depth of the wave lists.  KF > 16 (the deep variant): nclass gate classes, class = wave % nclass, class 1's
// published words in qbound2 (null when nclass = 1).
template <int QT, int P, bool IP, int KF>
__device__ __forceinline__ void sq_item(int nstep, const uint4 *__restrict__ codes_t, int64_t tp0,
                                        const float *__restrict__ rown, int64_t r0, int64_t r1, int nqi, int gcap,
                                        const unsigned *__restrict__ qs, const float4 *__restrict__ qpar,
                                        float *lkeys, int *lrows, const int *__restrict__ bucket, int boff, int nprobe,
                                        const int *__restrict__ slot_off, int chunk, unsigned *__restrict__ qbound,
                                        unsigned *__restrict__ qbound2, float *__restrict__ cand_d,
                                        int *__restrict__ cand_i) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, g = lane >> 4;
    const int stride = sq_stride(nstep);
    const int npass_all = (int)ceil_div(r1 - r0, 32);
    const int npass = npass_all > wave ? (npass_all - wave + SQ_W - 1) / SQ_W : 0;
    const int ilast = npass > 0 ? npass - 1 : 0;
    float *wk = lkeys + wave * gcap * KF;
    int *wr = lrows + wave * gcap * KF;
    // the word this wave's full lists publish into: its class's
    unsigned *qpub = qbound;
    if constexpr (KF > SQ_KF) {
        if (qbound2 && (wave & 1)) qpub = qbound2;
    }

    // the row stream: unconditional loads (past the wave's last step they re-read it)
    const uint4 *rp = codes_t;
    int ld_i = 0, ld_s = 0;
    auto set_pass = [&](int i) { rp = codes_t + ((tp0 + wave + SQ_W * i) * nstep) * 64 + lane; };
    auto next_load = [&](uint4 &dst) {
        const int s = ld_i <= ilast ? ld_s : nstep - 1;
        const sq_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const sq_u32x4 *>(rp + (int64_t)s * 64));
        dst = make_uint4(v[0], v[1], v[2], v[3]);
        if (++ld_s == nstep) {
            ld_s = 0;
            ++ld_i;
            set_pass(ld_i <= ilast ? ld_i : ilast);
        }
    };
    auto row_of = [&](int i, int r) -> int64_t {
        const int64_t row = r0 + (int64_t)(wave + SQ_W * i) * 32 + 16 * r + m;
        return row < r1 ? row : r1 - 1;
    };
    uint4 ring[P];
    float xnr[2] = {0.f, 0.f};
    if (npass > 0) {
        set_pass(0);
#pragma unroll
        for (int p = 0; p < P; ++p) next_load(ring[p]);
        if (!IP) {
#pragma unroll
            for (int r = 0; r < 2; ++r) xnr[r] = rown[row_of(0, r)];
        }
    }
    // this wave's lists start empty
    for (int t = lane; t < nqi * KF; t += 64) {
        wk[t] = __builtin_inff();
        wr[t] = SQ_PAD_ROW;
    }
    // the query image and constants were written by every thread before the call
    __syncthreads();

    // this lane's queries qt·16 + 4g + v: their thresholds in registers, their key constants in LDS
    float thr[QT][4];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int v = 0; v < 4; ++v)  // (nothing passes -inf: the queries past the item's count)
            thr[qt][v] = qt * 16 + 4 * g + v < nqi ? __builtin_inff() : -__builtin_inff();
    const unsigned *qrow[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) qrow[qt] = qs + (qt * 16 + m) * stride + 4 * g;

    sq_f32x4 acc[QT][2];
    for (int i = 0; i < npass; ++i) {
        // the queries' published bounds, read under the pass's products
        unsigned gb[QT][4];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int q = qt * 16 + 4 * g + v;
                gb[qt][v] = q < nqi ? __hip_atomic_load(qbound + bucket[boff + q] / nprobe, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT)
                                    : 0xff800000u;
                if constexpr (KF > SQ_KF) {
                    // two classes: the gate is the larger word (order-preserving bits), +inf until both have published
                    if (qbound2 && q < nqi) {
                        const unsigned g2 = __hip_atomic_load(qbound2 + bucket[boff + q] / nprobe, __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_AGENT);
                        gb[qt][v] = gb[qt][v] > g2 ? gb[qt][v] : g2;
                    }
                }
            }
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int r = 0; r < 2; ++r) acc[qt][r] = sq_f32x4{0.f, 0.f, 0.f, 0.f};
        float xnr_next[2] = {0.f, 0.f};
        if (!IP) {
#pragma unroll
            for (int r = 0; r < 2; ++r) xnr_next[r] = rown[row_of(i + 1 <= ilast ? i + 1 : ilast, r)];
        }
        for (int S0 = 0; S0 < nstep; S0 += P) {
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int S = S0 + p;
                uint4 qa[QT];
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) qa[qt] = *reinterpret_cast<const uint4 *>(qrow[qt] + S * 16);
                const sq_f16x8 c0 = sq_cvt8(ring[p].x, ring[p].y), c1 = sq_cvt8(ring[p].z, ring[p].w);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    acc[qt][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(sq_f16x8, qa[qt]), c0,
                                                                        acc[qt][0], 0, 0, 0);
                    acc[qt][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(sq_f16x8, qa[qt]), c1,
                                                                        acc[qt][1], 0, 0, 0);
                }
                next_load(ring[p]);
            }
        }
        const int64_t prow0 = r0 + (int64_t)(wave + SQ_W * i) * 32;
        bool any = false;
#pragma clang loop unroll(full)
        for (int qt = 0; qt < QT; ++qt)
#pragma clang loop unroll(full)
            for (int v = 0; v < 4; ++v) {
                // thr = min(own list's KF-th key, published bound + 2E): margins sit with the constants in LDS
                // (−2/t | −1/t, A | −P, 2E) of the query
                const int q = qt * 16 + 4 * g + v;
                const float4 kc = qpar[q < nqi ? q : 0];
                const float gthr = sq_order_float(gb[qt][v]) + kc.z;
                const float th = fminf(thr[qt][v], gthr == gthr ? gthr : __builtin_inff());
#pragma clang loop unroll(full)
                for (int r = 0; r < 2; ++r) {
                    const float key = (kc.y + xnr[r]) + kc.x * acc[qt][r][v];
                    const bool s = prow0 + 16 * r + m < r1 && key <= th;
                    const unsigned long long bal = __ballot(s);
                    if (bal == 0ull) continue;
                    any = true;
                    for (int gg = 0; gg < 4; ++gg) {
                        unsigned bits = (unsigned)(bal >> (16 * gg)) & 0xffffu;
                        const int ql = qt * 16 + 4 * gg + v;
                        while (bits) {
                            const int mm = __builtin_ctz(bits);
                            bits &= bits - 1;
                            const float ck = readlane_f(key, 16 * gg + mm);
                            sq_list_insert<KF>(wk + ql * KF, wr + ql * KF, ck, (int)(prow0 + 16 * r + mm), lane);
                        }
                    }
                }
            }
        if (any) {
            // the lists changed: this lane's thresholds again, and a smaller full-list key is published
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int q = qt * 16 + 4 * g + v;
                    if (q < nqi) {
                        const float k16 = wk[q * KF + KF - 1];  // (the list's KF-th key)
                        const bool fresh = k16 < thr[qt][v];
                        thr[qt][v] = k16;
                        if (m == 0 && fresh) {
                            atomicMin(qpub + bucket[boff + q] / nprobe, sq_order_bits(k16));
                        }
                    }
                }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) xnr[r] = xnr_next[r];
    }
    // the wave's lists -> the (slot, wave) sub-lists
    for (int t = lane; t < nqi * KF; t += 64) {
        const int q = t / KF, e = t - q * KF;
        const int64_t dst = (((int64_t)slot_off[bucket[boff + q]] + chunk) * SQ_W + wave) * KF + e;
        cand_d[dst] = wk[t];
        cand_i[dst] = wr[t];
    }
}

template <int P, bool IP, int KF>
__global__ void __launch_bounds__(64 * SQ_W, 2)
ivf_sq_scan(const uint4 *__restrict__ qimg, const float4 *__restrict__ par, const float *__restrict__ pair_a, int nstep,
            const uint4 *__restrict__ codes_t, const int64_t *__restrict__ tpass_off, const float *__restrict__ rown,
            const int64_t *__restrict__ list_off, const int *__restrict__ list_len, const int *__restrict__ cnt,
            const int *__restrict__ bucket_off, const int *__restrict__ item_off, const int *__restrict__ bucket,
            const int *__restrict__ slot_off, int nlist, int nprobe, int group, unsigned *__restrict__ qbound,
            unsigned *__restrict__ qbound2, float *__restrict__ cand_d, int *__restrict__ cand_i) {
    extern __shared__ __attribute__((aligned(16))) float smem_sq[];
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
    const int64_t r0 = lr0 + (int64_t)chunk * SQ_CH;
    const int64_t r1 = r0 + SQ_CH < lr1 ? r0 + SQ_CH : lr1;
    const int boff = bucket_off[l] + q_begin;
    const int nqt = (nqi + 15) >> 4;
    const int64_t tp0 = tpass_off[l] + (int64_t)chunk * (SQ_CH / 32);
    const int gcap = ivf_group_wide(group);

    // LDS: the queries' terms [query][step][g][4 dwords]; (−2/t | −1/t, A | −P, 2E, −) per query; the waves' lists
    unsigned *qs = reinterpret_cast<unsigned *>(smem_sq);
    const int stride = sq_stride(nstep);
    float4 *qpar = reinterpret_cast<float4 *>(qs + gcap * stride);
    float *lkeys = reinterpret_cast<float *>(qpar + gcap);
    int *lrows = reinterpret_cast<int *>(lkeys + SQ_W * gcap * KF);
    const int per_q = nstep * 4;
    for (int t = threadIdx.x; t < nqi * per_q; t += 64 * SQ_W) {
        const int q = t / per_q, r2 = t - q * per_q;
        const int gq = bucket[boff + q] / nprobe;
        *reinterpret_cast<uint4 *>(qs + q * stride + r2 * 4) = qimg[(int64_t)gq * per_q + r2];
    }
    for (int t = threadIdx.x; t < nqi; t += 64 * SQ_W) {
        const int pair = bucket[boff + t];
        const float4 p = par[pair / nprobe];
        const float a = pair_a[pair];
        qpar[t] = make_float4(IP ? -p.x : -2.f * p.x, IP ? -a : a, p.z, 0.f);
    }
#define SQ_CASE(QTV)                                                                                                 \
    sq_item<QTV, P, IP, KF>(nstep, codes_t, tp0, rown, r0, r1, nqi, gcap, qs, qpar, lkeys, lrows, bucket, boff,    \
                            nprobe, slot_off, chunk, qbound, qbound2, cand_d, cand_i);
    switch (nqt) {
    case 0: case 1: SQ_CASE(1) break;
    case 2: SQ_CASE(2) break;
    case 3: SQ_CASE(3) break;
    default: SQ_CASE(4) break;
    }
#undef SQ_CASE
}

// One wave per query (k <= 16 at KF = 16, k <= 64 at KF = 32): τ, the certificate, the recheck of every candidate
// within 2E of τ.  A slot holds SQ_W sub-lists of KF entries; a sub-list is full when its entry KF − 1 is not a pad.
template <bool IP, int KF>
__global__ void __launch_bounds__(256)
ivf_sq_rerank(const float *__restrict__ Q, int64_t nq, int d, int nstep, int k, const float4 *__restrict__ par,
              const float *__restrict__ cand_d, const int *__restrict__ cand_i, const int *__restrict__ slot_off,
              int nprobe, const int64_t *__restrict__ probes, const int64_t *__restrict__ list_off, int nlist,
              const float *__restrict__ centroids, const float *__restrict__ vmin, const float *__restrict__ vdiff,
              const unsigned char *__restrict__ codes_t, const int64_t *__restrict__ tpass_off,
              const int64_t *__restrict__ ids, int *__restrict__ nflag, int *__restrict__ flagged,
              unsigned long long *__restrict__ fb_total, float *__restrict__ D, int64_t *__restrict__ I) {
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int lane = threadIdx.x & 63;
    constexpr int SL = SQ_W * KF;  // entries per slot
    const int64_t e0 = (int64_t)slot_off[q * nprobe] * SL, e1 = (int64_t)slot_off[(q + 1) * nprobe] * SL;
    WaveList<1, int> L;
    L.init();
    float minfull = __builtin_inff();
    bool anyfull = false;
    for (int64_t c0 = e0; c0 < e1; c0 += 64) {  // (SL is a multiple of 64)
        const float key = cand_d[c0 + lane];
        const int row = cand_i[c0 + lane];
        if ((lane & (KF - 1)) == KF - 1 && row != SQ_PAD_ROW) {
            anyfull = true;
            minfull = fminf(minfull, key);
        }
        L.offer(row != SQ_PAD_ROW ? key : __builtin_inff(), row, k - 1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) minfull = fminf(minfull, __shfl_xor(minfull, o));
    anyfull = __ballot(anyfull) != 0ull;
    float tau;
    int trow;
    L.threshold(k - 1, tau, trow);
    const float4 p = par[q];
    const float thr2 = tau + p.z;
    if (!(p.y < __builtin_inff()) || (anyfull && !(minfull > thr2))) {
        if (lane == 0) {
            flagged[atomicAdd(nflag, 1)] = (int)q;
            atomicAdd(fb_total, 1ull);
        }
        return;
    }
    const float *qp = Q + q * (int64_t)d;
    WaveList<1, long long> R;
    R.init();
    unsigned nre = 0;
    for (int pr = 0; pr < nprobe; ++pr) {
        const int64_t pair = q * nprobe + pr;
        const int64_t b0 = (int64_t)slot_off[pair] * SL, b1 = (int64_t)slot_off[pair + 1] * SL;
        if (b0 == b1) continue;
        const int64_t l = probes[pair];
        const float *g = centroids ? centroids + l * (int64_t)d : nullptr;
        const float base = IP && g ? sq_wave_dot(qp, g, d, lane) : 0.f;
        for (int64_t c0 = b0; c0 < b1; c0 += 64) {
            const float key = cand_d[c0 + lane];
            const int row = cand_i[c0 + lane];
            unsigned long long sel = __ballot(row != SQ_PAD_ROW && key <= thr2);
            nre += (unsigned)__popcll(sel);
            while (sel) {
                const int j = __ffsll(sel) - 1;
                sel &= sel - 1;
                const int64_t rw = readlane_i(row, j);
                int rr;
                const unsigned char *ps = sq_row_pass(codes_t, tpass_off, list_off, l, rw, nstep, rr);
                const float dist = sq_row_dist<IP>(qp, g, base, ps, rr, d, vmin, vdiff, lane);
                const float cd = IP ? -dist : dist;
                const long long cid = ids[rw];
                float td;
                long long tid;
                R.threshold(k - 1, td, tid);
                if (lex_less(cd, cid, td, tid)) R.insert(cd, cid);
            }
        }
    }
    if (lane == 0) atomicAdd(fb_total + 2, (unsigned long long)nre);  // (hipann_debug_ivfsq_info "rechecked")
    if (lane < k) {
        const bool pad = R.id[0] == IdTraits<long long>::pad();
        D[q * k + lane] = pad ? (IP ? -__builtin_inff() : __builtin_inff()) : (IP ? -R.d[0] : R.d[0]);
        I[q * k + lane] = pad ? -1 : (int64_t)R.id[0];
    }
}

// The direct kernel: one wave per (query | flagged query, probe, chunk) slot, every row by sq_row_dist.  ALL: the
// slot's 2048 entries are all its rows (k > 64); else its 64 best.
template <bool IP, bool ALL>
__global__ void __launch_bounds__(256)
ivf_sq_direct(const float *__restrict__ Q, int64_t nq, int d, int nstep, int nprobe, int max_nch,
              const int *__restrict__ nflag, const int *__restrict__ flagged, const int64_t *__restrict__ probes,
              const int64_t *__restrict__ list_off, const int *__restrict__ list_len, int nlist,
              const int *__restrict__ slot_off, const float *__restrict__ centroids, const float *__restrict__ vmin,
              const float *__restrict__ vdiff, const unsigned char *__restrict__ codes_t,
              const int64_t *__restrict__ tpass_off, const int64_t *__restrict__ ids, float *__restrict__ dl_d,
              void *__restrict__ dl_iv) {
    const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t per_q = (int64_t)nprobe * max_nch;
    const int64_t fi = idx / per_q;
    if (fi >= (nflag ? (int64_t)*nflag : nq)) return;
    const int64_t q = nflag ? flagged[fi] : fi;
    const int rem = (int)(idx - fi * per_q);
    const int pr = rem / max_nch, chunk = rem - pr * max_nch;
    const int64_t pair = q * nprobe + pr;
    const int64_t l = probes[pair];
    if (l < 0 || l >= nlist) return;
    const int64_t len = list_len[l];
    if ((int64_t)chunk * SQ_CH >= len) return;
    const int64_t r0 = list_off[l] + (int64_t)chunk * SQ_CH;
    const int64_t r1 = r0 + SQ_CH < list_off[l] + len ? r0 + SQ_CH : list_off[l] + len;
    const int64_t slot = (int64_t)slot_off[pair] + chunk;
    const float *qp = Q + q * (int64_t)d;
    const float *g = centroids ? centroids + l * (int64_t)d : nullptr;
    const float base = IP && g ? sq_wave_dot(qp, g, d, lane) : 0.f;
    constexpr int KS = ALL ? SQ_CH : kSqDirectK;
    // (the 64 best by (distance, id), as the merge orders them: labels; every row: shard rows for launch_ivf_merge)
    float *od = dl_d + slot * KS;
    int *oi = static_cast<int *>(dl_iv) + slot * KS;
    long long *ol = static_cast<long long *>(dl_iv) + slot * KS;
    WaveList<1, long long> L;
    L.init();
    for (int64_t row = r0; row < r1; ++row) {
        int rr;
        const unsigned char *ps = sq_row_pass(codes_t, tpass_off, list_off, l, row, nstep, rr);
        const float dist = sq_row_dist<IP>(qp, g, base, ps, rr, d, vmin, vdiff, lane);
        const float cd = IP ? -dist : dist;
        if (ALL) {
            if (lane == 0) {
                od[row - r0] = cd;
                oi[row - r0] = (int)row;
            }
        } else {
            float td;
            long long tid;
            const long long cid = ids[row];
            L.threshold(kSqDirectK - 1, td, tid);
            if (lex_less(cd, cid, td, tid)) L.insert(cd, cid);
        }
    }
    if (ALL) {
        for (int64_t e = (r1 - r0) + lane; e < SQ_CH; e += 64) {
            od[e] = __builtin_inff();
            oi[e] = SQ_PAD_ROW;
        }
    } else {
        L.store(od, ol, kSqDirectK);
    }
}

// One wave per (flagged) query: its slots' 64-entry lists merged to the k best by (distance, id), k <= 64.
__global__ void __launch_bounds__(256)
ivf_sq_merge(int64_t nq, int k, int nprobe, const int *__restrict__ nflag, const int *__restrict__ flagged,
             const int *__restrict__ slot_off, const float *__restrict__ dl_d, const long long *__restrict__ dl_l,
             float sign, float *__restrict__ D, int64_t *__restrict__ I) {
    const int64_t fi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (fi >= (nflag ? (int64_t)*nflag : nq)) return;
    const int64_t q = nflag ? flagged[fi] : fi;
    const int lane = threadIdx.x & 63;
    const int64_t e0 = (int64_t)slot_off[q * nprobe] * kSqDirectK, e1 = (int64_t)slot_off[(q + 1) * nprobe] * kSqDirectK;
    WaveList<1, long long> L;
    L.init();
    for (int64_t c0 = e0; c0 < e1; c0 += 64) {
        L.offer(dl_d[c0 + lane], dl_l[c0 + lane], k - 1);
    }
    if (lane < k) {
        const bool pad = L.id[0] == IdTraits<long long>::pad();
        D[q * k + lane] = pad ? sign * __builtin_inff() : sign * L.d[0];
        I[q * k + lane] = pad ? -1 : (int64_t)L.id[0];
    }
}

// ------------------------------------------------------------------------------------------------
void launch_ivf_sq_tile(const unsigned char *codes, const int64_t *list_off, const int *list_len,
                        const int64_t *tpass_off, int nlist, int64_t total_pass, int d, int nstep, unsigned char *dst,
                        hipStream_t st) {
    if (total_pass <= 0) return;
    HIPANN_REQUIRE(total_pass < (int64_t)0x7fffffff, "IVF SQ8: too many passes");
    hipLaunchKernelGGL(ivf_sq_tile, dim3((unsigned)total_pass), dim3(256), 0, st, codes, list_off, list_len, tpass_off,
                       nlist, d, nstep, dst);
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_sq_untile(const IvfSqView &v, const int64_t *list_off, const int *list_len, const int64_t *out_off,
                          int64_t total_pass, unsigned char *codes, int64_t *ids_out, hipStream_t st) {
    if (total_pass <= 0) return;
    hipLaunchKernelGGL(ivf_sq_untile, dim3((unsigned)total_pass), dim3(256), 0, st, v.codes_t, list_off, list_len,
                       v.tpass_off, out_off, v.ids, v.nlist, v.d, v.nstep, codes, ids_out);
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_sq_row_terms(const unsigned char *codes, const IvfSqView &v, const int64_t *list_off, int nlist,
                             float *rown, unsigned *cmax2, hipStream_t st) {
    if (v.nrows <= 0) return;
    hipLaunchKernelGGL(ivf_sq_row_terms, dim3((unsigned)ceil_div(v.nrows, 4)), dim3(256), 0, st, codes, v.nrows, v.d,
                       v.sb, 32 * v.nstep, v.by_residual ? v.centroids : nullptr, list_off, nlist,
                       v.metric == kL2 ? 1 : 0, rown, cmax2);
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_sq_query_prep(const float *Q, int64_t nq, const IvfSqView &v, float cmax, float wbase, void *qimg,
                              float *par, unsigned *qbound2, hipStream_t st) {
    if (nq <= 0) return;
    const dim3 grid((unsigned)ceil_div(nq, 4)), block(256);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, st, Q, nq, v.d, v.nstep, v.sb, cmax, wbase,
                           static_cast<_Float16 *>(qimg), reinterpret_cast<float4 *>(par), qbound2);
    };
    if (v.metric == kIP) go(ivf_sq_query_prep<true>);
    else go(ivf_sq_query_prep<false>);
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_sq_pair_terms(const float *Q, int64_t nq, int nprobe, const int64_t *probes, const IvfSqView &v,
                              float *pair_a, hipStream_t st) {
    const int64_t npairs = nq * nprobe;
    if (npairs <= 0) return;
    const dim3 grid((unsigned)ceil_div(npairs, 4)), block(256);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, st, Q, npairs, nprobe, probes, v.d, v.nstep, v.nlist,
                           v.by_residual ? v.centroids : nullptr, v.sb, pair_a);
    };
    if (v.metric == kIP) go(ivf_sq_pair_terms<true>);
    else go(ivf_sq_pair_terms<false>);
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_sq_scan(const IvfSqView &v, const IvfPlanView &plan, int group, int kf, int nclass, int64_t max_items,
                        const void *qimg, const float *par, const float *pair_a, unsigned *qbound, unsigned *qbound2,
                        float *cand_d, int *cand_i, hipStream_t st) {
    if (max_items <= 0) return;
    HIPANN_REQUIRE(kf == SQ_KF || kf == SQ_KD, "IVF SQ8 scan: filter depth");
    HIPANN_REQUIRE(nclass == 1 || (nclass == 2 && kf == SQ_KD && qbound2), "IVF SQ8 scan: gate classes");
    HIPANN_REQUIRE(ivf_chunk_rows() == SQ_CH, "IVF SQ8 scan: chunks of 2048 rows");
    HIPANN_REQUIRE(max_items < (int64_t)0x7fffffff, "too many IVF work items");
    const int wide = ivf_group_wide(group);
    HIPANN_REQUIRE(wide >= 16 && wide <= 16 * SQ_QT && wide % 16 == 0 && ivf_group_narrow(group) == 0,
                   "IVF SQ8 scan: unsupported group");
    const size_t smem = sq_lds_bytes(v.nstep, wide, kf);
    HIPANN_REQUIRE(smem <= SQ_LDS_MAX, "IVF SQ8 scan: LDS image too large");
    HIPANN_REQUIRE(v.metric == kIP || v.rown, "IVF SQ8 scan: L2 needs the row terms");
    const dim3 grid((unsigned)max_items), block(64 * SQ_W);
    auto go = [&](auto kern, bool &ready) {
        if (!ready) {  // once per kernel instance
            HIPANN_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)SQ_LDS_MAX));
            ready = true;
        }
        hipLaunchKernelGGL(kern, grid, block, smem, st, static_cast<const uint4 *>(qimg),
                           reinterpret_cast<const float4 *>(par), pair_a, v.nstep,
                           reinterpret_cast<const uint4 *>(v.codes_t), v.tpass_off, v.rown, HIPANN_PLAN_ARGS(plan), group,
                           qbound, nclass == 2 ? qbound2 : nullptr, cand_d, cand_i);
    };
    const bool p8 = v.nstep % 8 == 0;
    static bool ready[8] = {false, false, false, false, false, false, false, false};
    if (kf == SQ_KF) {
        if (v.metric == kIP) { if (p8) go(ivf_sq_scan<8, true, SQ_KF>, ready[0]); else go(ivf_sq_scan<4, true, SQ_KF>, ready[1]); }
        else { if (p8) go(ivf_sq_scan<8, false, SQ_KF>, ready[2]); else go(ivf_sq_scan<4, false, SQ_KF>, ready[3]); }
    } else {
        if (v.metric == kIP) { if (p8) go(ivf_sq_scan<8, true, SQ_KD>, ready[4]); else go(ivf_sq_scan<4, true, SQ_KD>, ready[5]); }
        else { if (p8) go(ivf_sq_scan<8, false, SQ_KD>, ready[6]); else go(ivf_sq_scan<4, false, SQ_KD>, ready[7]); }
    }
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_sq_rerank(const IvfSqView &v, const IvfPlanView &plan, const int64_t *probes, const float *Q, int64_t nq,
                          int k, int kf, int nclass, const float *par, const float *cand_d, const int *cand_i, int *nflag, int *flagged,
                          unsigned long long *fb_total, float *D, int64_t *I, hipStream_t st) {
    if (nq <= 0) return;
    HIPANN_REQUIRE(kf == SQ_KF || kf == SQ_KD, "IVF SQ8 rerank: filter depth");
    // (the scan's gate bounds the k-th key only while nclass·kf rows stand behind it; the result list holds 64)
    HIPANN_REQUIRE(k >= 1 && k <= nclass * kf && k <= kSqDirectK, "IVF SQ8 rerank: k above the filter depth");
    const dim3 grid((unsigned)ceil_div(nq, 4)), block(256);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, st, Q, nq, v.d, v.nstep, k, reinterpret_cast<const float4 *>(par), cand_d,
                           cand_i, plan.slot_off, plan.nprobe, probes, plan.list_off, plan.nlist,
                           v.by_residual ? v.centroids : nullptr, v.vmin, v.vdiff, v.codes_t, v.tpass_off, v.ids, nflag,
                           flagged, fb_total, D, I);
    };
    if (kf == SQ_KF) { if (v.metric == kIP) go(ivf_sq_rerank<true, SQ_KF>); else go(ivf_sq_rerank<false, SQ_KF>); }
    else { if (v.metric == kIP) go(ivf_sq_rerank<true, SQ_KD>); else go(ivf_sq_rerank<false, SQ_KD>); }
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_sq_direct(const IvfSqView &v, const IvfPlanView &plan, const int64_t *probes, const float *Q, int64_t nq,
                          int max_nch, int kslot, const int *nflag, const int *flagged, float *dl_d, void *dl_i,
                          hipStream_t st) {
    const int64_t waves = nq * plan.nprobe * max_nch;
    if (waves <= 0) return;
    HIPANN_REQUIRE(ceil_div(waves, 4) < (int64_t)0x7fffffff, "IVF SQ8 direct: too many slots");
    HIPANN_REQUIRE(kslot == kSqDirectK || kslot == SQ_CH, "IVF SQ8 direct: slot size");
    const dim3 grid((unsigned)ceil_div(waves, 4)), block(256);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, st, Q, nq, v.d, v.nstep, plan.nprobe, max_nch, nflag, flagged, probes,
                           plan.list_off, plan.list_len, plan.nlist, plan.slot_off,
                           v.by_residual ? v.centroids : nullptr, v.vmin, v.vdiff, v.codes_t, v.tpass_off, v.ids, dl_d, dl_i);
    };
    const bool all = kslot == SQ_CH;
    if (v.metric == kIP) { if (all) go(ivf_sq_direct<true, true>); else go(ivf_sq_direct<true, false>); }
    else { if (all) go(ivf_sq_direct<false, true>); else go(ivf_sq_direct<false, false>); }
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_sq_merge(const IvfSqView &v, const IvfPlanView &plan, int64_t nq, int k, const int *nflag,
                         const int *flagged, const float *dl_d, const void *dl_i, float *D, int64_t *I, hipStream_t st) {
    if (nq <= 0) return;
    HIPANN_REQUIRE(k >= 1 && k <= kSqDirectK, "IVF SQ8 merge: k above the slot lists");
    hipLaunchKernelGGL(ivf_sq_merge, dim3((unsigned)ceil_div(nq, 4)), dim3(256), 0, st, nq, k, plan.nprobe, nflag,
                       flagged, plan.slot_off, dl_d, static_cast<const long long *>(dl_i), v.metric == kIP ? -1.f : 1.f, D, I);
    HIPANN_CHECK(hipGetLastError());
}

}  // namespace hipann
