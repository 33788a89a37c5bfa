// ivf_sq8_host.hpp — the pure host functions of the IVF SQ8 stages (ivf_sq8.cpp): argument checks, CSR validation,
// scratch and slot sizing.  No HIP call in here: tools/ivf_sq8_hostcheck.cpp runs them under the host sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <numeric>
#include <vector>

namespace hipann {

// nullptr when the arguments of hipann_ivfsq_create describe an index, else what is wrong with them
inline const char *ivf_sq_check_create(int d, int metric, int nlist, int nprobe, const float *centroids,
                                       const float *vmin, const float *vdiff, const int64_t *list_offsets,
                                       const int64_t *ids, const uint8_t *codes) {
    if (d <= 0 || nlist <= 0) return "d and nlist must be > 0";
    if (metric != 0 && metric != 1) return "metric must be 0 (L2) or 1 (IP)";
    if (nprobe < 1) return "nprobe must be >= 1";
    if (!centroids || !vmin || !vdiff || !list_offsets) return "null centroids / vmin / vdiff / offsets";
    if (list_offsets[0] != 0) return "list offsets must start at 0";
    for (int l = 0; l < nlist; ++l)
        if (list_offsets[l + 1] < list_offsets[l]) return "list offsets not ascending";
    const int64_t n = list_offsets[nlist];
    if (n >= (int64_t)0x7fffffff) return "more than 2^31-1 rows";
    if (n > 0 && (!ids || !codes)) return "null ids / codes";
    for (int i = 0; i < d; ++i)
        if (!std::isfinite(vmin[i]) || !std::isfinite(vdiff[i])) return "vmin / vdiff must be finite";
    for (int64_t i = 0; i < (int64_t)nlist * d; ++i)
        if (!std::isfinite(centroids[i])) return "centroids must be finite";
    return nullptr;
}

// nullptr when a search call's (nq, k) are valid
inline const char *ivf_sq_check_search(int64_t nq, int64_t k, int64_t max_k, bool have_ptrs) {
    if (k <= 0) return "k must be > 0";
    if (k > max_k) return "k larger than HIPANN_MAX_K";
    if (nq < 0 || (nq > 0 && !have_ptrs)) return "invalid arguments";
    return nullptr;
}

// the call's probe count: nprobe <= 0 means the index's value, a value above nlist means nlist
inline int ivf_sq_call_nprobe(int nprobe, int index_nprobe, int nlist) {
    return std::min(nprobe <= 0 ? index_nprobe : nprobe, nlist);
}

// s = vdiff/255, b = vmin + s/2 in fp32, zero-padded to dpad each: [s | b]
inline std::vector<float> ivf_sq_scale_bias(const float *vmin, const float *vdiff, int d, int dpad) {
    std::vector<float> sb((size_t)2 * dpad, 0.f);
    for (int i = 0; i < d; ++i) {
        const float s = vdiff[i] / 255.0f;
        sb[i] = s;
        sb[(size_t)dpad + i] = vmin[i] + s / 2.0f;
    }
    return sb;
}

// the bound's magnitudes: max ‖g_l‖ (0 without residual) and ‖(|vmin_i| + |vdiff_i|·256/255)_i‖
inline void ivf_sq_magnitudes(const float *centroids, int nlist, int d, bool by_residual, const float *vmin,
                              const float *vdiff, double *gmax, double *mnorm) {
    double g2 = 0.0, m2 = 0.0;
    for (int l = 0; by_residual && l < nlist; ++l) {
        double a = 0.0;
        for (int i = 0; i < d; ++i) a += (double)centroids[(size_t)l * d + i] * centroids[(size_t)l * d + i];
        g2 = std::max(g2, a);
    }
    for (int i = 0; i < d; ++i) {
        const double m = std::fabs((double)vmin[i]) + std::fabs((double)vdiff[i]) * (256.0 / 255.0);
        m2 += m * m;
    }
    *gmax = std::sqrt(g2);
    *mnorm = std::sqrt(m2);
}

// 32-row pass offsets of the lists (nlist + 1)
inline std::vector<int64_t> ivf_sq_pass_offsets(const int64_t *list_offsets, int nlist) {
    std::vector<int64_t> tp((size_t)nlist + 1, 0);
    for (int l = 0; l < nlist; ++l) tp[l + 1] = tp[l] + (list_offsets[l + 1] - list_offsets[l] + 31) / 32;
    return tp;
}

// nullptr when the arguments of hipann_ivfsq_train describe a training set, else what is wrong with them
inline const char *ivf_sq_check_train(int d, int metric, int nlist, int by_residual, bool have_centroids, int64_t n,
                                      bool have_rows, bool have_out) {
    if (d <= 0 || nlist <= 0) return "d and nlist must be > 0";
    if (metric != 0 && metric != 1) return "metric must be 0 (L2) or 1 (IP)";
    if (n < 1) return "training needs at least one row";
    if (!have_rows || !have_out || (by_residual && !have_centroids)) return "null rows / centroids / vmin / vdiff";
    return nullptr;
}

// nullptr when a trained quantizer is usable, else the error
inline const char *ivf_sq_check_trained(const float *vmin, const float *vdiff, int d) {
    for (int i = 0; i < d; ++i)
        if (!std::isfinite(vmin[i]) || !std::isfinite(vdiff[i])) return "trained vmin / vdiff must be finite";
    return nullptr;
}

// true when list l cannot take add[l] more rows in its slack for some l
inline bool ivf_sq_must_grow(const std::vector<int64_t> &off, const std::vector<int64_t> &len,
                             const std::vector<int64_t> &add) {
    for (size_t l = 0; l < len.size(); ++l)
        if (len[l] + add[l] > off[l + 1] - off[l]) return true;
    return false;
}

// The list starts after growth (IVFFlat's rule, ivf_relayout): every list leaves with capacity max(cap, need +
// max(need / 4, 64)) rows, need = len + add, rounded up to whole 32-row passes.
inline std::vector<int64_t> ivf_sq_grown_offsets(const std::vector<int64_t> &off, const std::vector<int64_t> &len,
                                                 const std::vector<int64_t> &add) {
    std::vector<int64_t> out(off.size(), 0);
    for (size_t l = 0; l < len.size(); ++l) {
        const int64_t cap = off[l + 1] - off[l], need = len[l] + add[l];
        const int64_t ncap = std::max(cap, need + std::max<int64_t>(need / 4, 64));
        out[l + 1] = out[l] + (ncap + 31) / 32 * 32;
    }
    return out;
}

// hipann_ivfsq_remove_ids: the caller's labels as a set (FAISS's IDSelectorBatch), sorted for the kernel's search
inline std::vector<int64_t> ivf_sq_label_set(const int64_t *labels, int64_t n) {
    std::vector<int64_t> lab(labels, labels + n);
    std::sort(lab.begin(), lab.end());
    lab.erase(std::unique(lab.begin(), lab.end()), lab.end());
    return lab;
}

// The lists' lengths after a removal, from the kernel's readback: the rows removed, or -1 when a new length is not
// within [0, old length] (nothing of len has changed then).
inline int64_t ivf_sq_removed_lengths(std::vector<int64_t> &len, const int *newlen) {
    int64_t removed = 0;
    for (size_t l = 0; l < len.size(); ++l) {
        if (newlen[l] < 0 || newlen[l] > len[l]) return -1;
        removed += len[l] - newlen[l];
    }
    for (size_t l = 0; l < len.size(); ++l) len[l] = newlen[l];
    return removed;
}

// the most (probe, chunk) slots a query can own: the chunk counts of its nprobe longest lists
inline int64_t ivf_sq_query_slots(const std::vector<int64_t> &len, int np, int chunk_rows) {
    std::vector<int64_t> nch;
    for (int64_t l : len)
        if (l > 0) nch.push_back((l + chunk_rows - 1) / chunk_rows);
    if ((int64_t)nch.size() > np) {
        std::nth_element(nch.begin(), nch.begin() + np, nch.end(), std::greater<int64_t>());
        nch.resize((size_t)np);
    }
    return std::max<int64_t>(1, std::accumulate(nch.begin(), nch.end(), (int64_t)0));
}

// queries per slice so that the per-slot scratch (slot_bytes each) stays within budget
inline int64_t ivf_sq_slice_queries(int64_t nq, int64_t query_slots, int64_t slot_bytes, int64_t budget) {
    const int64_t per_q = std::max<int64_t>(1, query_slots * slot_bytes);
    return std::max<int64_t>(1, std::min<int64_t>(nq, budget / per_q));
}

}  // namespace hipann
