// remove_kernels.hip — row removal on the resident copies (hipann_flat_remove_ids / hipann_ivf_remove_ids).
//
// Flat (faiss::IndexFlatCodes::remove_ids): a stable compaction.  Over the rows from the first removed one to the
// shard's end: a keep mask (1, cleared at the removed rows), an exclusive prefix sum of the mask in three launches
// (per-block sums, one block scanning the sums, the per-block scan again writing each kept row's source index at its
// destination), and gathers of the fp32 rows and the per-row floats (‖x‖², int8 scales) into FRESH buffers — a
// parallel shift in place would overwrite source rows other blocks have yet to read.
//
// IVF (faiss::IndexIVF::remove_ids, DirectMap NoMap): one block per list marks its live rows (binary search of each
// id in the sorted label set; the slack is never read), derives FAISS's sequential fill-the-hole-with-the-last-entry
// order in closed form — with L live rows, r of them marked and L' = L − r, the marked positions below L' ascending
// receive the unmarked positions at or above L' descending — moves the pairs (sources and destinations are
// disjoint), zeroes the vacated rows and publishes the new length and the tiled passes it touched.
#include "runtime.hpp"

#include <algorithm>

namespace hipann {

namespace {

constexpr int kScanThreads = 256;
constexpr int kScanPer = 4;                          // rows per thread of the prefix-sum kernels
constexpr int kScanRows = kScanThreads * kScanPer;  // rows per block

// exclusive position of a set flag among the block's flags (thread order) and their count; wsum: one int per wave
__device__ __forceinline__ int block_flag_scan(bool f, int *wsum, int *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const unsigned long long b = __ballot(f);
    const int pre = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(b);
    __syncthreads();
    int add = 0, tot = 0;
    for (int i = 0; i < nw; ++i) {
        const int c = wsum[i];
        if (i < w) add += c;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return pre + add;
}

// keep[labels[i] − first] = 0 (labels: the shard's removed rows, sorted, unique, local; keep was set to 1)
__global__ void __launch_bounds__(256)
flat_remove_mask(const int64_t *__restrict__ rows, int64_t m, int64_t first, unsigned char *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) keep[rows[i] - first] = 0;
}

__global__ void __launch_bounds__(kScanThreads)
flat_remove_block_sums(const unsigned char *__restrict__ keep, int64_t cnt, int64_t *__restrict__ sums) {
    __shared__ int wsum[kScanThreads / 64];
    const int64_t r0 = (int64_t)blockIdx.x * kScanRows + (int64_t)threadIdx.x * kScanPer;
    int c = 0;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j)
        if (r0 + j < cnt) c += keep[r0 + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int i = 0; i < kScanThreads / 64; ++i) t += wsum[i];
        sums[blockIdx.x] = t;
    }
}

// one block: sums[b] → exclusive prefix (in place), chunk by chunk with a running carry
__global__ void __launch_bounds__(kScanThreads)
flat_remove_scan_sums(int64_t *__restrict__ sums, int64_t nb) {
    __shared__ int64_t sh[kScanThreads];
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < nb; c0 += kScanThreads) {
        const int64_t i = c0 + threadIdx.x;
        const int64_t v = i < nb ? sums[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < kScanThreads; o <<= 1) {  // Hillis-Steele inclusive scan
            const int64_t a = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < nb) sums[i] = carry + sh[threadIdx.x] - v;
        carry += sh[kScanThreads - 1];
        __syncthreads();
    }
}

// src[exclusive prefix of keep at r] = r for every kept row r (offs: the blocks' exclusive prefixes)
__global__ void __launch_bounds__(kScanThreads)
flat_remove_sources(const unsigned char *__restrict__ keep, int64_t cnt, const int64_t *__restrict__ offs,
                    int64_t *__restrict__ src) {
    __shared__ int wsum[kScanThreads / 64];
    const int64_t r0 = (int64_t)blockIdx.x * kScanRows + (int64_t)threadIdx.x * kScanPer;
    int k[kScanPer], c = 0;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
        k[j] = r0 + j < cnt ? keep[r0 + j] : 0;
        c += k[j];
    }
    // exclusive prefix of c over the block: within the wave by shuffles, across waves through LDS
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int add = 0;
    for (int i = 0; i < w; ++i) add += wsum[i];
    int64_t pos = offs[blockIdx.x] + add + inc - c;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j)
        if (k[j]) src[pos++] = r0 + j;
}

// dst row j ← src row idx[j] (rows of d floats); V: 16-byte loads and stores (d % 4 == 0, both bases 16-B aligned).
// 2^shift lanes share a row (the smallest power of two covering its elements, at most a wave).
template <bool V>
__global__ void __launch_bounds__(256)
flat_remove_gather_rows(const float *__restrict__ X, const int64_t *__restrict__ idx, int64_t cnt, int d, int shift,
                        float *__restrict__ out) {
    const int per = V ? d >> 2 : d;  // elements per row
    const int lpr = 1 << shift;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; (g >> shift) < cnt; g += (int64_t)gridDim.x * 256) {
        const int64_t j = g >> shift, s = idx[j];
        for (int c = (int)(g & (lpr - 1)); c < per; c += lpr) {
            if (V)
                reinterpret_cast<float4 *>(out)[j * per + c] = reinterpret_cast<const float4 *>(X)[s * per + c];
            else
                out[j * per + c] = X[s * per + c];
        }
    }
}

__global__ void __launch_bounds__(256)
flat_remove_gather_f32(const float *__restrict__ v, const int64_t *__restrict__ idx, int64_t cnt,
                       float *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < cnt) out[j] = v[idx[j]];
}

__device__ __forceinline__ bool label_member(const int64_t *__restrict__ labels, int64_t m, int64_t id) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (labels[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < m && labels[lo] == id;
}

// One block per list (grid-stride).  mark: one byte per physical row; plan: one int per physical row — the list's
// holes at plan[off + i], their sources at plan[off + L − 1 − i] (2·h ≤ L, so the two runs never meet).
// pass_ids / npass (optional): the tiled images' 32-row passes holding a destination or a vacated row.
__global__ void __launch_bounds__(256)
ivf_remove_rows(const int64_t *__restrict__ labels, int64_t m, const int64_t *__restrict__ list_off, int *list_len,
                int nlist, int d, float *codes, int64_t *ids, float *xnorm, unsigned char *mark, int *plan,
                const int64_t *__restrict__ tpass_off, int64_t *__restrict__ pass_ids,
                unsigned long long *__restrict__ npass, int *__restrict__ newlen) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool vec = (d & 3) == 0 && ((uintptr_t)codes & 15) == 0;
    for (int l = blockIdx.x; l < nlist; l += gridDim.x) {
        const int64_t off = list_off[l];
        const int L = list_len[l];
        // mark (live rows only) and count
        int r = 0;
        for (int c0 = 0; c0 < L; c0 += 256) {
            const int j = c0 + tid;
            const bool f = j < L && label_member(labels, m, ids[off + j]);
            if (j < L) mark[off + j] = f ? 1 : 0;
            int tot;
            (void)block_flag_scan(f, wsum, &tot);
            r += tot;
        }
        if (r == 0) {  // (block-uniform) nothing leaves this list
            if (tid == 0) newlen[l] = L;
            continue;
        }
        const int Lp = L - r;
        __syncthreads();  // the marks are visible to the whole block
        // holes: marked positions below L', ascending
        int h = 0;
        for (int c0 = 0; c0 < Lp; c0 += 256) {
            const int j = c0 + tid;
            const bool f = j < Lp && mark[off + j];
            int tot;
            const int pos = block_flag_scan(f, wsum, &tot);
            if (f) plan[off + h + pos] = j;
            h += tot;
        }
        // their sources: unmarked positions at or above L', descending (equally many)
        int hs = 0;
        for (int c0 = 0; c0 < r; c0 += 256) {
            const int j = L - 1 - (c0 + tid);
            const bool f = c0 + tid < r && !mark[off + j];
            int tot;
            const int pos = block_flag_scan(f, wsum, &tot);
            if (f) plan[off + L - 1 - (hs + pos)] = j;
            hs += tot;
        }
        __syncthreads();
        // move: one wave per pair (code row, id, norm)
        for (int i = w; i < h; i += 4) {
            const int64_t s = off + plan[off + L - 1 - i], t = off + plan[off + i];
            if (vec) {
                const float4 *sp = reinterpret_cast<const float4 *>(codes + s * d);
                float4 *tp = reinterpret_cast<float4 *>(codes + t * d);
                for (int c = lane; c < (d >> 2); c += 64) tp[c] = sp[c];
            } else {
                for (int c = lane; c < d; c += 64) codes[t * d + c] = codes[s * d + c];
            }
            if (lane == 0) {
                ids[t] = ids[s];
                if (xnorm) xnorm[t] = xnorm[s];
            }
        }
        __syncthreads();  // every source has been read
        // the vacated rows [L', L) back to zero slack (whole-table maxima read it)
        {
            float *z = codes + (off + Lp) * d;
            const int64_t nz = (int64_t)r * d;
            for (int64_t c = tid; c < nz; c += 256) z[c] = 0.f;
            if (xnorm)
                for (int c = tid; c < r; c += 256) xnorm[off + Lp + c] = 0.f;
        }
        if (pass_ids) {
            const int pv = Lp / 32;  // first vacated pass (r > 0: it exists)
            for (int i = tid; i < h; i += 256) {
                const int p = plan[off + i] / 32;
                const int prev = i > 0 ? plan[off + i - 1] / 32 : -1;
                if (p != prev && p != pv) pass_ids[atomicAdd(npass, 1ull)] = tpass_off[l] + p;
            }
            for (int p = pv + tid; p <= (L - 1) / 32; p += 256) pass_ids[atomicAdd(npass, 1ull)] = tpass_off[l] + p;
        }
        __syncthreads();  // plan / mark of this list are done before the next list reuses wsum
        if (tid == 0) {
            list_len[l] = Lp;
            newlen[l] = Lp;
        }
    }
}

}  // namespace

int64_t flat_remove_scan_blocks(int64_t cnt) { return ceil_div(cnt, kScanRows); }

// Flat removal plan over rows [first, first + cnt) of a shard: rows[0..m) (device, sorted unique local row numbers,
// all ≥ first) leave; src[j] = the (range-relative) source row of the j-th surviving row.  keep: cnt bytes, sums:
// flat_remove_scan_blocks(cnt) int64, src: cnt − m int64.
void launch_flat_remove_plan(const int64_t *rows, int64_t m, int64_t first, int64_t cnt, unsigned char *keep,
                             int64_t *sums, int64_t *src, hipStream_t st) {
    if (cnt <= 0) return;
    const int64_t nb = flat_remove_scan_blocks(cnt);
    HIPANN_REQUIRE(nb < (int64_t)0x7fffffff && ceil_div(m, 256) < (int64_t)0x7fffffff, "removal grid too large");
    HIPANN_CHECK(hipMemsetAsync(keep, 1, (size_t)cnt, st));
    if (m > 0) {
        hipLaunchKernelGGL(flat_remove_mask, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, st, rows, m, first, keep);
        HIPANN_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(flat_remove_block_sums, dim3((unsigned)nb), dim3(kScanThreads), 0, st, keep, cnt, sums);
    HIPANN_CHECK(hipGetLastError());
    hipLaunchKernelGGL(flat_remove_scan_sums, dim3(1), dim3(kScanThreads), 0, st, sums, nb);
    HIPANN_CHECK(hipGetLastError());
    hipLaunchKernelGGL(flat_remove_sources, dim3((unsigned)nb), dim3(kScanThreads), 0, st, keep, cnt, sums, src);
    HIPANN_CHECK(hipGetLastError());
}

// out row j ← X row idx[j], j < cnt (16-byte accesses when d % 4 == 0 and both bases are 16-byte aligned)
void launch_flat_gather_rows(const float *X, const int64_t *idx, int64_t cnt, int d, float *out, hipStream_t st) {
    if (cnt <= 0) return;
    const bool vec = d % 4 == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)out % 16 == 0;
    const int per = vec ? d / 4 : d;
    int shift = 0;
    while (shift < 6 && (1 << shift) < per) ++shift;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(cnt << shift, 256), 256 * 64);
    if (vec)
        hipLaunchKernelGGL(flat_remove_gather_rows<true>, dim3(grid), dim3(256), 0, st, X, idx, cnt, d, shift, out);
    else
        hipLaunchKernelGGL(flat_remove_gather_rows<false>, dim3(grid), dim3(256), 0, st, X, idx, cnt, d, shift, out);
    HIPANN_CHECK(hipGetLastError());
}

void launch_flat_gather_f32(const float *v, const int64_t *idx, int64_t cnt, float *out, hipStream_t st) {
    if (cnt <= 0) return;
    HIPANN_REQUIRE(ceil_div(cnt, 256) < (int64_t)0x7fffffff, "removal grid too large");
    hipLaunchKernelGGL(flat_remove_gather_f32, dim3((unsigned)ceil_div(cnt, 256)), dim3(256), 0, st, v, idx, cnt, out);
    HIPANN_CHECK(hipGetLastError());
}

// IVF removal of the labels (device, sorted unique) from every list of a shard, in FAISS's order; newlen[l] = the
// list's new live length.  mark: one byte, plan: one int per physical row.  pass_ids (with tpass_off, npass zeroed by
// the caller): the tiled images' passes to re-tile, each once.
void launch_ivf_remove_rows(const int64_t *labels, int64_t m, const int64_t *list_off, int *list_len, int nlist, int d,
                            float *codes, int64_t *ids, float *xnorm, unsigned char *mark, int *plan,
                            const int64_t *tpass_off, int64_t *pass_ids, unsigned long long *npass, int *newlen,
                            hipStream_t st) {
    if (nlist <= 0) return;
    const unsigned grid = (unsigned)std::min(nlist, 65536);
    hipLaunchKernelGGL(ivf_remove_rows, dim3(grid), dim3(256), 0, st, labels, m, list_off, list_len, nlist, d, codes,
                       ids, xnorm, mark, plan, tpass_off, pass_ids, npass, newlen);
    HIPANN_CHECK(hipGetLastError());
}

}  // namespace hipann
