// ivf_sq8_remove.hip — IVF SQ8: rows leave the tiled device lists in place (hipann_ivfsq_remove_ids).
//
// faiss::IndexIVF::remove_ids (DirectMap NoMap) per list: j = 0, l = len; while (j < l) { if member(id[j]) { --l;
// entry[j] = entry[l]; } else ++j; }.  In closed form, with L live rows, r of them marked and L' = L − r: the marked
// positions below L' ascending (the holes) receive the unmarked positions at or above L' descending (their sources);
// the two sets have the same size h <= r, h <= L'.
//
// ivf_sq_remove_rows — one launch, a block of four waves per list (grid-stride), three phases between block barriers:
//   1. mark and count: a thread per live row binary-searches the row's id in the sorted labels, writes the mark byte
//      and joins a block flag scan.  A list that loses nothing leaves here (8 bytes read per live row).
//   2. plan: holes at plan[off + i], their sources at plan[off + L − 1 − i] (list-relative; 2·h <= L, so the runs
//      never meet) — the arrangement ivf_remove_rows (remove_kernels.hip) uses, with the same helpers.
//   3. move, inside the tiled layout: an SQ8 handle has no row-major copy, a row is 4·nstep pieces of 8 bytes, one per
//      (K step, dimension octet), 16 bytes or more apart (sq_tile_off).  One wave moves one (hole, source) pair, lane
//      j piece j (the wave loops when 4·nstep > 64: d = 768 has 96 pieces), all 32·nstep dimensions — the padding is
//      zero on both sides; lane 0 moves the label and, for L2, N(row).  Holes lie below L' and sources at or above
//      it, so no pair reads what another writes and the phase needs no ordering inside it.
// After a barrier (every source has been read) the vacated rows [L', L) go back to the state ivf_sq_tile and
// ivf_sq_regroup leave slack in: zero codes — 16-byte stores over the passes vacated whole, 8-byte pieces per row in
// the pass that holds L' — label −1 and N = 0.  No search reads them (every scan bounds rows by list_len); a later
// add fills them, and an export or a handle re-created from one sees clean slack.  Thread 0 publishes the length.
#include "ivf.hpp"
#include "ivf_sq8_dev.hpp"
#include "remove_dev.hpp"

#include <algorithm>

namespace hipann {
namespace {

__global__ void __launch_bounds__(256)
ivf_sq_remove_rows(const int64_t *__restrict__ labels, int64_t m, const int64_t *__restrict__ list_off, int *list_len,
                   const int64_t *__restrict__ tpass_off, int nlist, int nstep, unsigned char *codes_t, int64_t *ids,
                   float *rown, unsigned char *mark, int *plan, int *__restrict__ newlen) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int npiece = 4 * nstep;
    const int64_t pass_bytes = (int64_t)nstep * 1024;
    for (int l = blockIdx.x; l < nlist; l += gridDim.x) {
        const int64_t off = list_off[l];
        const int L = list_len[l];
        // 1. mark (live rows only) and count
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
        // 2. holes: marked positions below L', ascending
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
        // 3. move: one wave per pair, a lane per 8-byte piece of the row
        unsigned char *base = codes_t + tpass_off[l] * pass_bytes;
        for (int i = w; i < h; i += 4) {
            const int s = plan[off + L - 1 - i], t = plan[off + i];
            const unsigned char *sp = base + (int64_t)(s >> 5) * pass_bytes;
            unsigned char *tp = base + (int64_t)(t >> 5) * pass_bytes;
            const int rs = s & 31, rt = t & 31;
            for (int j = lane; j < npiece; j += 64)
                *reinterpret_cast<uint2 *>(tp + sq_tile_off(rt, 8 * j)) =
                    *reinterpret_cast<const uint2 *>(sp + sq_tile_off(rs, 8 * j));
            if (lane == 0) {
                ids[off + t] = ids[off + s];
                if (rown) rown[off + t] = rown[off + s];
            }
        }
        __syncthreads();  // every source has been read
        // the vacated rows [L', L) back to slack: the part of the pass that holds L', then the passes vacated whole
        const int pv = Lp >> 5, pw = (Lp + 31) >> 5, pe = (L - 1) >> 5;
        if (Lp & 31) {
            unsigned char *pp = base + (int64_t)pv * pass_bytes;
            const int r1 = L < (pv + 1) * 32 ? L - pv * 32 : 32, nr = r1 - (Lp & 31);
            for (int c = tid; c < nr * npiece; c += 256) {
                const int rr = (Lp & 31) + c / npiece, j = c % npiece;
                *reinterpret_cast<uint2 *>(pp + sq_tile_off(rr, 8 * j)) = make_uint2(0u, 0u);
            }
        }
        if (pe >= pw) {
            uint4 *z = reinterpret_cast<uint4 *>(base + (int64_t)pw * pass_bytes);
            const int64_t nz = (int64_t)(pe - pw + 1) * nstep * 64;
            for (int64_t c = tid; c < nz; c += 256) z[c] = make_uint4(0u, 0u, 0u, 0u);
        }
        for (int c = tid; c < r; c += 256) {
            ids[off + Lp + c] = (int64_t)-1;
            if (rown) rown[off + Lp + c] = 0.f;
        }
        if (tid == 0) {
            list_len[l] = Lp;
            newlen[l] = Lp;
        }
    }
}

}  // namespace

void launch_ivf_sq_remove_rows(const int64_t *labels, int64_t m, const IvfSqView &v, const int64_t *list_off,
                               int *list_len, unsigned char *codes_t, int64_t *ids, float *rown, unsigned char *mark,
                               int *plan, int *newlen, hipStream_t st) {
    if (v.nlist <= 0) return;
    HIPANN_REQUIRE(v.metric == kIP || rown, "IVF SQ8 remove: L2 needs the row terms");
    const unsigned grid = (unsigned)std::min(v.nlist, 65536);
    hipLaunchKernelGGL(ivf_sq_remove_rows, dim3(grid), dim3(256), 0, st, labels, m, list_off, list_len, v.tpass_off,
                       v.nlist, v.nstep, codes_t, ids, v.metric == kL2 ? rown : nullptr, mark, plan, newlen);
    HIPANN_CHECK(hipGetLastError());
}

}  // namespace hipann
