// ivf.hpp — internal entry points shared between the C ABI translation units.
#pragma once
#include "runtime.hpp"

namespace hipann {
// form_override >= 0 replaces ix.form for this call (the exact forms' re-run of flagged queries).  pend == nullptr:
// the whole search (one host synchronisation when an exact form's flag count must be read); otherwise only the
// launch phase — no host synchronisation — and *pend holds what flat_shard_finish must run after the caller has
// synchronised with `st` (hipann_flat_search: every shard launched before any is waited on).
void flat_shard_search(FlatIndex &ix, FlatShard &sh, int64_t nq, const float *xq, int k, int kout, float *D,
                       int64_t *I, hipStream_t st, int form_override = -1, FlatPending *pend = nullptr);
void flat_shard_finish(FlatIndex &ix, FlatShard &sh, const FlatPending &pend, hipStream_t st);
struct IvfSearchOpts {
    // >= 0 replaces ix.form for this call (a re-run inside a search: it leaves ix.last_* and sh.dbg_* alone)
    int form_override = -1;
    // (device, nq × min(nprobe, nlist) int64): the caller's probe lists replace the coarse quantizer's
    const int64_t *probes_in = nullptr;
    // the filter-image probation's int8 pass: no flagged query is re-run, the flag count is left in sh.nflag
    bool count_only = false;
    bool record() const { return form_override < 0; }
};
void ivf_shard_search(IvfIndex &ix, IvfShard &sh, int64_t nq, const float *xq, int k, int kout, float *D, int64_t *I,
                      hipStream_t st, const IvfSearchOpts &opts = {});
// IVF SQ8 (ivf_sq8.cpp) shares the IVFFlat coarse step and plan.  ivf_make_core: an IvfIndex on one device with
// centroids, labels, list offsets and the coarse quantizer, and no fp32 rows.  ivf_coarse_plan: the coarse step (probe
// lists in sh.coarse_i) and launch_ivf_plan for scan items of `group` queries; qbound (nq words, +inf) and *nflag (0)
// are reset by the plan.
std::unique_ptr<IvfIndex> ivf_make_core(int d, int metric, int nlist, int nprobe, const float *centroids,
                                        const int64_t *list_offsets, const int64_t *ids, int device);
IvfPlanView ivf_coarse_plan(IvfIndex &ix, IvfShard &sh, int np, int64_t nq, const float *xq, int group, hipStream_t st);
// The pieces of ivf_make_core an SQ8 build needs on their own.  ivf_make_quantizer: the coarse quantizer over device
// centroids (borrowed; exact fp32 products) — flat_shard_search(k = 1) on it is the assignment hipann_ivf_add makes.
// ivf_set_list_meta: a shard's list starts (physical rows, nlist + 1) and live lengths on the host and the device, with
// n, live and max_nch (synchronises the shard's stream).
std::unique_ptr<FlatIndex> ivf_make_quantizer(int d, int metric, const float *centroids_dev, int nlist, int device,
                                              hipStream_t st);
void ivf_set_list_meta(IvfShard &sh, const std::vector<int64_t> &off, const std::vector<int64_t> &len, int nlist);

// ivf_sq8_build.hip — IVF SQ8 train and add.
// Column min / max of e = x − g_assign (centroids != nullptr) or x over n rows -> vmin, vdiff = fl32(max − min); bits:
// 2·d words of scratch.  A NaN entry or an assignment outside [0, nlist) leaves a NaN in its column.
void launch_ivf_sq_minmax(const float *x, int64_t n, int d, const int64_t *assign, const float *centroids, int nlist,
                          unsigned *bits, float *vmin, float *vdiff, hipStream_t st);
// FAISS's QT_8bit encode of n rows, each written to physical row dst[i] of its list assign[i]: tiled codes (all
// 32·nstep dims), N(row) (L2), label (labels[i], or label_base + i) and the running max ‖c‖² (*cmax2, float bits).
// dst == nullptr: the statistics-only pass — nothing is written but *bad |= 1 when a row holds a non-finite entry.
// list_off: the list starts the destinations refer to (v.tpass_off: their passes).
void launch_ivf_sq_encode_append(const float *x, int64_t n, const IvfSqView &v, const int64_t *assign,
                                 const int64_t *dst, const int64_t *labels, int64_t label_base, const int64_t *list_off,
                                 unsigned char *codes_t, float *rown, int64_t *ids, unsigned *cmax2, unsigned *bad,
                                 hipStream_t st);
// Growth: every pass, label and N(row) of the old layout (v, list_off, list_len) into the new one (pass offsets
// tp_new, list starts off_new, nrows_new physical rows); slack passes and rows are cleared.
void launch_ivf_sq_regroup(const IvfSqView &v, const int64_t *list_off, const int *list_len, const int64_t *tp_new,
                           const int64_t *off_new, int64_t npass_new, int64_t nrows_new, unsigned char *codes_new,
                           int64_t *ids_new, float *rown_new, hipStream_t st);
// ivf_sq8_remove.hip — hipann_ivfsq_remove_ids: every live row whose id is in labels (device, sorted unique) leaves
// its list in FAISS's order, moved inside the tiled layout (one block per list: mark, closed-form plan, move the 8-byte
// pieces, label and N(row); the vacated rows back to zero slack; list_len and newlen[l] = the new length).  mark: one
// byte, plan: one int per physical row; v.tpass_off: the lists' passes.
void launch_ivf_sq_remove_rows(const int64_t *labels, int64_t m, const IvfSqView &v, const int64_t *list_off,
                               int *list_len, unsigned char *codes_t, int64_t *ids, float *rown, unsigned char *mark,
                               int *plan, int *newlen, hipStream_t st);
}  // namespace hipann
