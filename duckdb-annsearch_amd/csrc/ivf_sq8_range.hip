// ivf_sq8_range.hip — IVF SQ8 range search (faiss::IndexIVF::range_search with the 8-bit scalar-quantizer scanner): per
// query, every live row of its probed lists whose direct-form fp32 distance over the decoded row (sq_row_dist, the
// function and the bits of every top-k path) passes the strict comparison — L2: dist < radius, IP: dist > radius — in
// probe order, then list order.  The slot / bitmask / prefix-sum / fill scheme is ivf_range.hip's: the scan leaves, per
// (query, probe, 2048-row chunk) slot, a 64-word mask of the admitted rows and their count; launch_ivf_range_offsets
// (reused as it is) turns the counts into slot offsets and lims; the fill writes (distance, id) at offset + rank.
// Every mask word has one writer and no atomic decides a position: the same bits in the same order on every run.
//
// ivf_sq_range_scan — the threshold scan of the tiled codes, list-major over the plan's items (list, chunk, group of
// (query, probe) pairs).  A block of 8 waves owns an item; wave w streams the 32-row passes w, w + 8, ... through the
// register ring of ivf_sq_scan (P = 4 or 8 one-KiB wave loads in flight), makes the codes exact fp16 with sq_cvt8 and
// accumulates 16 queries × 32 rows per query tile on v_mfma_f32_16x16x32_f16 (up to 4 tiles).  What it does not carry is
// the top-k scan's selection: no lists in LDS, no published bounds, no atomics, no insertion.  LDS holds the group's
// query terms and four constants per query — (16·nstep + 8)·4 + 16 bytes per query, 64 queries in 99 KiB at d = 768
// where the top-k scan fits 48.  Epilogue per pass, in registers: key = (A + N) + kx·acc (IP: −P + kx·acc), the
// expression and so the bits of ivf_sq_scan's key; a row survives unless key > thr_q.  One ballot per accumulator
// element group; a pass without a survivor touches no LDS, no atomic and no decode.  Survivors are rechecked in place by
// the whole wave with sq_row_dist, decoding from the pass already addressed, and admitted only under the strict
// comparison; lane q keeps query q's word of the pass and stores it after the pass; the slot's count is the sum of the
// waves' popcounts through LDS at the item's end.
//
// The bound.  ivf_sq8.hip proves |key − dist| <= E(q) for every probed row, dist the direct-form fp32 value (IP: of
// −dist), E(q) = par.y of ivf_sq_query_prep: nothing new is measured here.  thr_q = fl(R + E'), R = radius (IP:
// −radius), E' = fl(E + 2⁻²²·(|R| + E)): the three roundings of E' lose at most 2⁻²⁴·(1 + 2⁻²¹)·(|R| + E) of the slack,
// so E' >= E + 2⁻²³·(|R| + E), and the rounding of R + E' is at most 2⁻²⁴·(|R| + E') < 2⁻²³·(|R| + E): thr_q >= R + E in
// real numbers.  A row the direct form admits has dist < R (IP: −dist < R), so key <= dist + E < R + E <= thr_q and it
// survives.  Proof obligations: (1) cmax and max‖g_l‖ cover every row and list held (ivf_sq8.hip's obligation (1): an
// add raises cmax before it returns, a removal keeps it, the centroids never change); (2) a non-finite E (a query
// the preparation could not scale, a NaN entry) gives thr_q = +inf, and the test is the negated `key > thr_q`, so a NaN
// on either side keeps the row: every row of such a query is rechecked, and a NaN distance fails both strict
// comparisons; an infinite radius is taken as it is (R + E' could be inf − inf); (3) rows past list_len and queries past
// the item's count are masked, never compared; (4) the filter can only add rows to the recheck — membership is the
// recheck's strict comparison alone.  Nothing here is tuned from data.
//
// ivf_sq_range_direct — dimensions whose query terms do not fit the LDS (d > 4352, the top-k path's limit): one block
// of 4 waves per slot, sq_row_dist over every row, the same mask words and counts.
// ivf_sq_range_fill — one wave per slot: a row's rank is the popcount before its bit; the distance is recomputed with
// sq_row_dist (the bits the recheck compared), two admitted rows per step so that one row's loads are in flight under
// the other's reduction.
//
// Every kernel reads list_len, never list_off[l + 1]: append slack is never scanned, an empty list owns no slot.
// Resources (hipcc 7, gfx950, -O3): see DESIGN.md §5; no kernel here uses scratch.
#include "ivf_range_dev.hpp"
#include "ivf_sq8_dev.hpp"
#include "runtime.hpp"

#include <algorithm>

namespace hipann {

constexpr int SR_W = kSqWaves;  // waves per scan block
constexpr int SR_QT = 4;        // query tiles of an item at most (64 queries: one mask word per lane and pass)
constexpr size_t SR_LDS_MAX = 160 * 1024;

static size_t sr_lds_bytes(int nstep, int nq) { return (size_t)nq * ((size_t)sq_stride(nstep) * 4 + 16); }

int ivf_sq_range_group(int d) {
    const int nstep = ivf_sq_nstep(d);
    int qt = SR_QT;
    while (qt > 0 && sr_lds_bytes(nstep, 16 * qt) > SR_LDS_MAX) --qt;
    return 16 * qt;
}

// thr_q of the header: R = radius (IP: −radius)
__device__ __forceinline__ float sr_threshold(float E, float R) {
    if (!(E < 3.0e38f)) return __builtin_inff();
    if (!(fabsf(R) < __builtin_inff())) return R;
    const float e1 = E + 0x1p-22f * (fabsf(R) + E);
    return R + e1;
}

// One wave's share of an item: passes wave, wave + SR_W, ... of rows [r0, r1) of list l.
template <int QT, int P, bool IP>
__device__ __forceinline__ void sr_item(int d, int nstep, const uint4 *__restrict__ codes_t, int64_t tp0,
                                        const float *__restrict__ rown, int64_t r0, int64_t r1, int nqi,
                                        const unsigned *__restrict__ qs, const float4 *__restrict__ qpar,
                                        const int *__restrict__ bucket, int boff, int nprobe,
                                        const int *__restrict__ slot_off, int chunk, const float *__restrict__ Q,
                                        const float *__restrict__ g, const float *__restrict__ vmin,
                                        const float *__restrict__ vdiff, float radius, unsigned *__restrict__ mask,
                                        int *__restrict__ counts, int *red, unsigned long long *__restrict__ stat) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, gl = lane >> 4;
    const int stride = sq_stride(nstep);
    const int npass_all = (int)ceil_div(r1 - r0, 32);
    const int npass = npass_all > wave ? (npass_all - wave + SR_W - 1) / SR_W : 0;
    const int ilast = npass > 0 ? npass - 1 : 0;

    // the row stream: unconditional loads (past the wave's last step they re-read it)
    const uint4 *rp = codes_t;
    int ld_i = 0, ld_s = 0;
    auto set_pass = [&](int i) { rp = codes_t + ((tp0 + wave + SR_W * i) * nstep) * 64 + lane; };
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
        const int64_t row = r0 + (int64_t)(wave + SR_W * i) * 32 + 16 * r + m;
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
    // the query image and constants were written by every thread before the call
    __syncthreads();

    // this lane's queries qt·16 + 4·gl + v: (kx, A | −P, thr) in registers, validity as a bit per (qt, row tile, v)
    float kx[QT][4], ka[QT][4], thr[QT][4];
    unsigned valid = 0;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int q = qt * 16 + 4 * gl + v;
            const float4 p = qpar[q < nqi ? q : 0];
            kx[qt][v] = p.x;
            ka[qt][v] = p.y;
            thr[qt][v] = p.z;
            if (q < nqi) valid |= 0x11u << (qt * 8 + v);
        }
    const unsigned *qrow[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) qrow[qt] = qs + (qt * 16 + m) * stride + 4 * gl;
    // lane j keeps the mask words of the item's query j
    int64_t sb = 0;
    if (lane < nqi) sb = ((int64_t)slot_off[bucket[boff + lane]] + chunk) * RV_WORDS;
    int cnt = 0;
    unsigned nsurv = 0, nadm = 0;
    const unsigned char *bytes = reinterpret_cast<const unsigned char *>(codes_t);

    sq_f32x4 acc[QT][2];
    for (int i = 0; i < npass; ++i) {
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
        const int pi = wave + SR_W * i;
        const int64_t prow0 = r0 + (int64_t)pi * 32;
        // bit qt·8 + 4r + v of sm: query qt·16 + 4·gl + v against row 16r + m of the pass survives the filter
        unsigned sm = 0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const bool rok = prow0 + 16 * r + m < r1;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float key = (ka[qt][v] + xnr[r]) + kx[qt][v] * acc[qt][r][v];
                    const bool s = rok && !(key > thr[qt][v]);
                    sm |= (s ? 1u : 0u) << (qt * 8 + 4 * r + v);
                }
        }
        sm &= valid;
        unsigned w = 0;
        if (__ballot(sm != 0) != 0ull) {
            // the recheck: per (query tile, row tile, v) with a survivor and each of its four queries (one per 16-lane
            // group), the rows in ascending order by the whole wave, decoded from this pass's tiled bytes
            const unsigned char *ps = bytes + (tp0 + pi) * (int64_t)nstep * 1024;
            for (int b = 0; b < QT * 8; ++b) {
                const unsigned long long bal = __ballot((sm >> b) & 1u);
                if (bal == 0ull) continue;
                const int qt = b >> 3, r = (b >> 2) & 1, v = b & 3;
                for (int gg = 0; gg < 4; ++gg) {
                    unsigned bits = (unsigned)(bal >> (16 * gg)) & 0xffffu;
                    if (!bits) continue;
                    const int ql = qt * 16 + 4 * gg + v;
                    const float *qp = Q + (int64_t)(bucket[boff + ql] / nprobe) * d;
                    const float base = qpar[ql].w;
                    while (bits) {
                        const int rr = 16 * r + __builtin_ctz(bits);  // (a survivor's row is below r1)
                        bits &= bits - 1;
                        const float dist = sq_row_dist<IP>(qp, g, base, ps, rr, d, vmin, vdiff, lane);
                        const bool pass = IP ? dist > radius : dist < radius;
                        ++nsurv;
                        nadm += pass;
                        if (pass && lane == ql) w |= 1u << rr;
                    }
                }
            }
        }
        if (lane < nqi) mask[sb + pi] = w;
        cnt += __popc(w);
#pragma unroll
        for (int r = 0; r < 2; ++r) xnr[r] = xnr_next[r];
    }

    // the slots' counts: the waves' per-query sums through LDS (the query image is no longer read)
    __syncthreads();
    red[wave * 64 + lane] = cnt;
    __syncthreads();
    for (int q = threadIdx.x; q < nqi; q += 64 * SR_W) {
        int c = 0;
#pragma unroll
        for (int wv = 0; wv < SR_W; ++wv) c += red[wv * 64 + q];
        counts[slot_off[bucket[boff + q]] + chunk] = c;
    }
    if (stat && lane == 0 && nsurv) {
        atomicAdd(stat, (unsigned long long)nsurv);
        atomicAdd(stat + 1, (unsigned long long)nadm);
    }
}

template <int P, bool IP>
__global__ void __launch_bounds__(64 * SR_W, 2)
ivf_sq_range_scan(const uint4 *__restrict__ qimg, const float4 *__restrict__ par, const float *__restrict__ pair_a,
                  int d, int nstep, const uint4 *__restrict__ codes_t, const int64_t *__restrict__ tpass_off,
                  const float *__restrict__ rown, const int64_t *__restrict__ list_off, const int *__restrict__ list_len,
                  const int *__restrict__ cnt, const int *__restrict__ bucket_off, const int *__restrict__ item_off,
                  const int *__restrict__ bucket, const int *__restrict__ slot_off, int nlist, int nprobe, int group,
                  const float *__restrict__ Q, const float *__restrict__ centroids, const float *__restrict__ vmin,
                  const float *__restrict__ vdiff, float radius, unsigned *__restrict__ mask, int *__restrict__ counts,
                  unsigned long long *__restrict__ stat) {
    extern __shared__ __attribute__((aligned(16))) float smem_sr[];
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
    const float *g = centroids ? centroids + (int64_t)l * d : nullptr;

    // LDS: the queries' terms [query][step][g][4 dwords], then (−2/t | −1/t, A | −P, thr, IP: q·g) per query
    unsigned *qs = reinterpret_cast<unsigned *>(smem_sr);
    const int stride = sq_stride(nstep);
    float *qpar = reinterpret_cast<float *>(qs + nqi * stride);
    const int per_q = nstep * 4;
    for (int t = threadIdx.x; t < nqi * per_q; t += 64 * SR_W) {
        const int q = t / per_q, r2 = t - q * per_q;
        const int gq = bucket[boff + q] / nprobe;
        *reinterpret_cast<uint4 *>(qs + q * stride + r2 * 4) = qimg[(int64_t)gq * per_q + r2];
    }
    for (int t = threadIdx.x; t < nqi; t += 64 * SR_W) {
        const int pair = bucket[boff + t];
        const float4 p = par[pair / nprobe];
        const float a = pair_a[pair];
        qpar[4 * t + 0] = IP ? -p.x : -2.f * p.x;
        qpar[4 * t + 1] = IP ? -a : a;
        qpar[4 * t + 2] = sr_threshold(p.y, IP ? -radius : radius);
        if (!(IP && g)) qpar[4 * t + 3] = 0.f;
    }
    if (IP && g) {  // the recheck's q·g, by the function the other paths use: query t by wave t mod 8
        const int lane = threadIdx.x & 63;
        for (int t = threadIdx.x >> 6; t < nqi; t += SR_W) {
            const float base = sq_wave_dot(Q + (int64_t)(bucket[boff + t] / nprobe) * d, g, d, lane);
            if (lane == 0) qpar[4 * t + 3] = base;
        }
    }
    int *red = reinterpret_cast<int *>(smem_sr);
#define SR_CASE(QTV)                                                                                                  \
    sr_item<QTV, P, IP>(d, nstep, codes_t, tp0, rown, r0, r1, nqi, qs, reinterpret_cast<const float4 *>(qpar), bucket, \
                        boff, nprobe, slot_off, chunk, Q, g, vmin, vdiff, radius, mask, counts, red, stat);
    switch (nqt) {
    case 0: case 1: SR_CASE(1) break;
    case 2: SR_CASE(2) break;
    case 3: SR_CASE(3) break;
    default: SR_CASE(4) break;
    }
#undef SR_CASE
}

// The direct kernel: one block of 4 waves per slot, the same mask words and count as the scan.
template <bool IP>
__global__ void __launch_bounds__(256)
ivf_sq_range_direct(const float *__restrict__ Q, int d, int nstep, const unsigned char *__restrict__ codes_t,
                    const int64_t *__restrict__ tpass_off, const int64_t *__restrict__ probes, int64_t npairs,
                    int nprobe, int max_nch, const int64_t *__restrict__ list_off, const int *__restrict__ list_len,
                    int nlist, const int *__restrict__ slot_off, const float *__restrict__ centroids,
                    const float *__restrict__ vmin, const float *__restrict__ vdiff, float radius,
                    unsigned *__restrict__ mask, int *__restrict__ counts) {
    __shared__ int red[4];
    int64_t pair, r0, r1;
    int slot;
    if (!rv_slot(blockIdx.x, max_nch, npairs, probes, list_off, list_len, nlist, slot_off, pair, slot, r0, r1)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t l = probes[pair];
    const float *qp = Q + (pair / nprobe) * (int64_t)d;
    const float *g = centroids ? centroids + l * (int64_t)d : nullptr;
    const float base = IP && g ? sq_wave_dot(qp, g, d, lane) : 0.f;
    const int npass = (int)ceil_div(r1 - r0, 32);
    int cnt = 0;
    for (int pi = wave; pi < npass; pi += 4) {
        int rr;
        const unsigned char *ps = sq_row_pass(codes_t, tpass_off, list_off, l, r0 + (int64_t)pi * 32, nstep, rr);
        unsigned w = 0;
        for (int j = 0; j < 32 && r0 + (int64_t)pi * 32 + j < r1; ++j) {
            const float dist = sq_row_dist<IP>(qp, g, base, ps, j, d, vmin, vdiff, lane);
            if (IP ? dist > radius : dist < radius) w |= 1u << j;
        }
        if (lane == 0) mask[(int64_t)slot * RV_WORDS + pi] = w;
        cnt += __popc(w);
    }
    if (lane == 0) red[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[slot] = red[0] + red[1] + red[2] + red[3];
}

// One wave per slot: the admitted rows' (distance, id) at soff[slot] + rank, rank = the set bits before the row's.
template <bool IP>
__global__ void __launch_bounds__(256)
ivf_sq_range_fill(const float *__restrict__ Q, int d, int nstep, const unsigned char *__restrict__ codes_t,
                  const int64_t *__restrict__ tpass_off, const int64_t *__restrict__ ids,
                  const int64_t *__restrict__ probes, int64_t npairs, int nprobe, int max_nch,
                  const int64_t *__restrict__ list_off, const int *__restrict__ list_len, int nlist,
                  const int *__restrict__ slot_off, const float *__restrict__ centroids, const float *__restrict__ vmin,
                  const float *__restrict__ vdiff, const unsigned *__restrict__ mask, const int *__restrict__ counts,
                  const int64_t *__restrict__ soff, float *__restrict__ D, int64_t *__restrict__ I) {
    int64_t pair, r0, r1;
    int slot;
    const int lane = threadIdx.x & 63;
    if (!rv_slot((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), max_nch, npairs, probes, list_off, list_len, nlist,
                 slot_off, pair, slot, r0, r1))
        return;
    if (counts[slot] == 0) return;
    const int64_t l = probes[pair];
    const float *qp = Q + (pair / nprobe) * (int64_t)d;
    const float *g = centroids ? centroids + l * (int64_t)d : nullptr;
    const float base = IP && g ? sq_wave_dot(qp, g, d, lane) : 0.f;
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
    const int64_t out0 = soff[slot];
    for (int pi = 0; pi < npass; ++pi) {
        unsigned bits = (unsigned)__shfl((int)word, pi);
        int64_t pos = out0 + __shfl(before, pi);
        if (!bits) continue;
        int rr;
        const unsigned char *ps = sq_row_pass(codes_t, tpass_off, list_off, l, r0 + (int64_t)pi * 32, nstep, rr);
        while (bits) {
            // two admitted rows per step: the second row's loads are issued under the first's reduction
            const int j0 = __builtin_ctz(bits);
            bits &= bits - 1;
            const bool two = bits != 0;
            const int j1 = two ? __builtin_ctz(bits) : j0;
            bits &= bits - 1;
            const float d0 = sq_row_dist<IP>(qp, g, base, ps, j0, d, vmin, vdiff, lane);
            const float d1 = two ? sq_row_dist<IP>(qp, g, base, ps, j1, d, vmin, vdiff, lane) : 0.f;
            if (lane == 0) {
                D[pos] = d0;
                I[pos] = ids[r0 + (int64_t)pi * 32 + j0];
            }
            if (two && lane == 1) {
                D[pos + 1] = d1;
                I[pos + 1] = ids[r0 + (int64_t)pi * 32 + j1];
            }
            pos += two ? 2 : 1;
        }
    }
}

// ------------------------------------------------------------------------------------------------
void launch_ivf_sq_range_scan(const IvfSqRangeArgs &a, const IvfSqView &v, const IvfPlanView &plan, int group,
                              int64_t max_items, hipStream_t st) {
    if (max_items <= 0 || a.nq <= 0) return;
    HIPANN_REQUIRE(ivf_chunk_rows() == RV_CH, "IVF SQ8 range scan: chunks of 2048 rows");
    HIPANN_REQUIRE(max_items < (int64_t)0x7fffffff, "too many IVF work items");
    HIPANN_REQUIRE(a.qimg && a.par && a.pair_a && a.mask && a.counts, "IVF SQ8 range scan: missing buffers");
    HIPANN_REQUIRE(v.metric == kIP || v.rown, "IVF SQ8 range scan: L2 needs the row terms");
    const int wide = ivf_group_wide(group);
    HIPANN_REQUIRE(wide >= 16 && wide <= 16 * SR_QT && wide % 16 == 0 && ivf_group_narrow(group) == 0,
                   "IVF SQ8 range scan: unsupported group");
    const size_t smem = std::max(sr_lds_bytes(v.nstep, wide), (size_t)SR_W * 64 * sizeof(int));
    HIPANN_REQUIRE(smem <= SR_LDS_MAX, "IVF SQ8 range scan: LDS image too large");
    const dim3 grid((unsigned)max_items), block(64 * SR_W);
    auto go = [&](auto kern, bool &ready) {
        if (!ready) {  // once per kernel instance
            HIPANN_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)SR_LDS_MAX));
            ready = true;
        }
        hipLaunchKernelGGL(kern, grid, block, smem, st, static_cast<const uint4 *>(a.qimg),
                           reinterpret_cast<const float4 *>(a.par), a.pair_a, v.d, v.nstep,
                           reinterpret_cast<const uint4 *>(v.codes_t), v.tpass_off, v.rown, HIPANN_PLAN_ARGS(plan), group,
                           a.Q, v.by_residual ? v.centroids : nullptr, v.vmin, v.vdiff, a.radius, a.mask, a.counts,
                           a.stat);
    };
    const bool p8 = v.nstep % 8 == 0;
    static bool ready[4] = {false, false, false, false};
    if (v.metric == kIP) { if (p8) go(ivf_sq_range_scan<8, true>, ready[0]); else go(ivf_sq_range_scan<4, true>, ready[1]); }
    else { if (p8) go(ivf_sq_range_scan<8, false>, ready[2]); else go(ivf_sq_range_scan<4, false>, ready[3]); }
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_sq_range_direct(const IvfSqRangeArgs &a, const IvfSqView &v, const IvfPlanView &plan, hipStream_t st) {
    const int64_t blocks = a.nq * plan.nprobe * a.max_nch;
    if (blocks <= 0) return;
    HIPANN_REQUIRE(ivf_chunk_rows() == RV_CH, "IVF SQ8 range scan: chunks of 2048 rows");
    HIPANN_REQUIRE(blocks < (int64_t)0x7fffffff, "IVF SQ8 range scan: too many slots");
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, st, a.Q, v.d, v.nstep, v.codes_t, v.tpass_off,
                           a.probes, a.nq * plan.nprobe, plan.nprobe, a.max_nch, plan.list_off, plan.list_len, plan.nlist,
                           plan.slot_off, v.by_residual ? v.centroids : nullptr, v.vmin, v.vdiff, a.radius, a.mask,
                           a.counts);
    };
    if (v.metric == kIP) go(ivf_sq_range_direct<true>);
    else go(ivf_sq_range_direct<false>);
    HIPANN_CHECK(hipGetLastError());
}

void launch_ivf_sq_range_fill(const IvfSqRangeArgs &a, const IvfSqView &v, const IvfPlanView &plan, const int64_t *soff,
                              float *D, int64_t *I, hipStream_t st) {
    const int64_t waves = a.nq * plan.nprobe * a.max_nch;
    if (waves <= 0) return;
    HIPANN_REQUIRE(ceil_div(waves, 4) < (int64_t)0x7fffffff, "IVF SQ8 range fill: too many slots");
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div(waves, 4)), dim3(256), 0, st, a.Q, v.d, v.nstep, v.codes_t,
                           v.tpass_off, v.ids, a.probes, a.nq * plan.nprobe, plan.nprobe, a.max_nch, plan.list_off,
                           plan.list_len, plan.nlist, plan.slot_off, v.by_residual ? v.centroids : nullptr, v.vmin,
                           v.vdiff, a.mask, a.counts, soff, D, I);
    };
    if (v.metric == kIP) go(ivf_sq_range_fill<true>);
    else go(ivf_sq_range_fill<false>);
    HIPANN_CHECK(hipGetLastError());
}

}  // namespace hipann
