// ivf_sq8.cpp — IVF SQ8 part of the C ABI (include/hip_ann.h, hipann_ivfsq_*): faiss::IndexIVFScalarQuantizer with
// QT_8bit codes on one device.  The coarse step and the plan are the IVFFlat ones (ivf.hpp ivf_coarse_plan); the
// kernels are in ivf_sq8.hip, the pure host functions in ivf_sq8_host.hpp.
#include "../../include/hip_ann.h"
#include "ivf.hpp"
#include "ivf_sq8_host.hpp"

#include <cstring>
#include <exception>
#include <string>

using namespace hipann;

namespace {

void set_err(char *buf, int len, const char *msg) {
    if (!buf || len <= 0) return;
    std::strncpy(buf, msg, (size_t)len - 1);
    buf[len - 1] = '\0';
}

template <typename R, typename F>
R guard(char *eb, int el, R fail, F &&f) {
    try {
        return f();
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return fail;
}

IvfSqIndex *as_sq(void *h) {
    auto *ix = static_cast<IndexBase *>(h);
    return ix && ix->kind == Kind::IVFSQ ? static_cast<IvfSqIndex *>(ix) : nullptr;
}

// The per-slot scratch of one query slice stays within this.  A slice streams every probed list again (a list's rows
// are read once per group of queries, whatever the slice holds), so slicing costs a scan each: 1 GiB keeps the headline
// batch (1024 queries × 32 probes of up to 3 chunks × 1.75 KiB) in one slice — at 256 MiB it ran as two and took twice
// the time.
constexpr int64_t kSqScratchBudget = (int64_t)1 << 30;

IvfSqView sq_view(const IvfSqIndex &ix) {
    const IvfShard &sh = *ix.core->shards[0];
    IvfSqView v;
    v.d = ix.d, v.nstep = ix.nstep, v.metric = ix.metric, v.by_residual = ix.by_residual, v.nlist = ix.core->nlist;
    v.centroids = sh.centroids, v.vmin = ix.vmin.get<float>(), v.vdiff = ix.vdiff.get<float>();
    v.sb = ix.sb.get<float>(), v.rown = ix.rown.get<float>();
    v.codes_t = ix.codes_t.get<unsigned char>(), v.tpass_off = ix.tpass_off.get<int64_t>(), v.ids = sh.ids;
    v.nrows = sh.n;
    return v;
}

// ---- one query slice: the stages of a search, in their order on the stream ----
struct SqBatch {
    IvfSqIndex &ix;
    IvfShard &sh;
    const IvfSqView v;
    const int64_t nq;
    const float *const xq;
    const int k, np;
    float *const D;
    int64_t *const I;
    const hipStream_t st;
    bool scan = false;  // the code scan + rerank (else the direct kernel for every query)
    int kf = 0;         // the scan's sub-list depth (kSqKeep | kSqDeep) and its gate classes, ceil(k / kf)
    int nclass = 1;
    int group = 0;
    IvfPlanView plan{};
    int64_t slots = 0;  // the host's bound of the slice's slots
};

// the scan serves k <= 16 at depth 16 and k <= 64 at depth 32, at dimensions whose query terms fit the LDS beside
// the lists of that depth; everything else the direct kernel
void sq_pick_mode(SqBatch &b) {
    const int kf = b.k <= kSqKeep ? kSqKeep : b.k <= kSqDirectK ? kSqDeep : 0;
    const int wide = kf ? ivf_sq_group(b.ix.d, kf) : 0;
    b.scan = wide >= 16;
    b.kf = b.scan ? kf : 0;
    b.nclass = b.scan ? (b.k + kf - 1) / kf : 1;
    b.group = b.scan ? wide << 8 : 16 << 8;
    b.slots = b.nq * ivf_sq_query_slots(b.sh.h_len, b.np, ivf_chunk_rows());
    HIPANN_REQUIRE(b.slots < (int64_t)0x7fffffff / (kSqWaves * (b.scan ? kf : kSqKeep)), "IVF SQ8: too many slots");
    b.ix.last_form = b.scan ? 1 : 0;
    b.ix.last_kfilt = b.kf;
    b.ix.last_sublists = b.scan ? kSqWaves : 0;
}

// the fp16 query terms and (1/t, E, 2E, ‖q‖²) per query
void sq_prepare_queries(SqBatch &b) {
    if (!b.scan) return;
    IvfSqIndex &ix = b.ix;
    ix.qimg.ensure((size_t)b.nq * ix.nstep * 32 * 2, b.sh.device);
    ix.par.ensure((size_t)b.nq * 16, b.sh.device);
    const float wbase = (float)((ix.gmax + ix.mnorm) * 1.0001);
    if (b.nclass == 2) ix.qbound2.ensure(sizeof(unsigned) * (size_t)b.nq, b.sh.device);
    launch_ivf_sq_query_prep(b.xq, b.nq, b.v, ix.cmax, wbase, ix.qimg.p, ix.par.get<float>(),
                             b.nclass == 2 ? ix.qbound2.get<unsigned>() : nullptr, b.st);
}

// the IVFFlat coarse step and plan, then A(q, l) (IP: q·(g + b)) per pair
void sq_coarse_and_plan(SqBatch &b) {
    b.plan = ivf_coarse_plan(*b.ix.core, b.sh, b.np, b.nq, b.xq, b.group, b.st);
    if (!b.scan) return;
    b.ix.pair_a.ensure(sizeof(float) * (size_t)b.nq * b.np, b.sh.device);
    launch_ivf_sq_pair_terms(b.xq, b.nq, b.np, b.sh.coarse_i.get<int64_t>(), b.v, b.ix.pair_a.get<float>(), b.st);
}

// the code scan over the plan's items: kSqWaves sub-lists of b.kf (key, row) per slot
void sq_scan(SqBatch &b) {
    IvfSqIndex &ix = b.ix;
    const size_t entries = (size_t)b.slots * kSqWaves * b.kf;
    ix.cand_d.ensure(entries * sizeof(float), b.sh.device);
    ix.cand_i.ensure(entries * sizeof(int), b.sh.device);
    RoctxRange rr("hipann.ivfsq.scan");
    ScopedTiming t(ix.timer_main, b.st);
    launch_ivf_sq_scan(b.v, b.plan, b.group, b.kf, b.nclass,
                       ivf_max_items(b.nq, b.np, ix.core->nlist, b.sh.max_nch, b.sh.n, b.group), ix.qimg.p,
                       ix.par.get<float>(), ix.pair_a.get<float>(), b.sh.qbound.get<unsigned>(),
                       ix.qbound2.get<unsigned>(), ix.cand_d.get<float>(), ix.cand_i.get<int>(), b.st);
}

// the candidates' direct-form distances and the certificate; flagged queries into sh.nflag / ix.flagged
void sq_rerank(SqBatch &b) {
    IvfSqIndex &ix = b.ix;
    ix.flagged.ensure(sizeof(int) * (size_t)b.nq, b.sh.device);
    ScopedTiming t(ix.timer_merge, b.st);
    launch_ivf_sq_rerank(b.v, b.plan, b.sh.coarse_i.get<int64_t>(), b.xq, b.nq, b.k, b.kf, b.nclass, ix.par.get<float>(),
                         ix.cand_d.get<float>(), ix.cand_i.get<int>(), b.sh.nflag.get<int>(), ix.flagged.get<int>(),
                         ix.fb_total.get<unsigned long long>(), b.D, b.I, b.st);
}

// the direct kernel and its merge: the flagged queries after a scan (the device reads the count), else every query
void sq_direct(SqBatch &b) {
    IvfSqIndex &ix = b.ix;
    const int kslot = b.k <= kSqDirectK ? kSqDirectK : ivf_chunk_rows();
    ix.dl_d.ensure((size_t)b.slots * kslot * sizeof(float), b.sh.device);
    ix.dl_i.ensure((size_t)b.slots * kslot * (kslot == kSqDirectK ? sizeof(int64_t) : sizeof(int)), b.sh.device);
    const int *nflag = b.scan ? b.sh.nflag.get<int>() : nullptr;
    const int *flagged = b.scan ? ix.flagged.get<int>() : nullptr;
    RoctxRange rr("hipann.ivfsq.direct");
    TimerPause tp(ix.timer_main);
    launch_ivf_sq_direct(b.v, b.plan, b.sh.coarse_i.get<int64_t>(), b.xq, b.nq, std::max(b.sh.max_nch, 1), kslot, nflag,
                         flagged, ix.dl_d.get<float>(), ix.dl_i.p, b.st);
    if (kslot == kSqDirectK) {
        launch_ivf_sq_merge(b.v, b.plan, b.nq, b.k, nflag, flagged, ix.dl_d.get<float>(), ix.dl_i.p, b.D, b.I,
                            b.st);
    } else {
        launch_ivf_merge(ix.dl_d.get<float>(), ix.dl_i.get<int>(), b.v.ids, b.v.nrows, b.plan.slot_off, b.np, b.nq, kslot,
                         b.k, ix.metric == kIP ? -1.f : 1.f, b.D, b.I, b.st);
    }
}

// nq queries on the index's device -> D / I (nq × k) on the same device, asynchronous on st
void sq_search_device(IvfSqIndex &ix, int nprobe, int64_t nq, const float *xq, int k, float *D, int64_t *I,
                      hipStream_t st) {
    IvfShard &sh = *ix.core->shards[0];
    DeviceGuard g(sh.device);
    const int np = ivf_sq_call_nprobe(nprobe, ix.core->nprobe, ix.core->nlist);
    ix.last_nq = nq;
    ix.last_np = np;
    ix.probes_kept = false;
    if (nq <= 0) return;
    const bool deep = k > kSqKeep && k <= kSqDirectK && ivf_sq_group(ix.d, kSqDeep) >= 16;
    const int64_t slot_bytes = k <= kSqKeep        ? (int64_t)(kSqWaves * kSqKeep * 8 + kSqDirectK * 12)
                               : deep            ? (int64_t)(kSqWaves * kSqDeep * 8 + kSqDirectK * 12)
                               : k <= kSqDirectK ? (int64_t)kSqDirectK * 12
                                                 : (int64_t)ivf_chunk_rows() * 8;
    const int64_t step = ivf_sq_slice_queries(nq, ivf_sq_query_slots(sh.h_len, np, ivf_chunk_rows()), slot_bytes,
                                              kSqScratchBudget);
    if (step < nq) ix.probes.ensure(sizeof(int64_t) * (size_t)nq * np, sh.device);
    for (int64_t q0 = 0; q0 < nq; q0 += step) {
        const int64_t nqs = std::min(step, nq - q0);
        SqBatch b{ix, sh, sq_view(ix), nqs, xq + q0 * ix.d, k, np, D + q0 * k, I + q0 * k, st};
        sq_pick_mode(b);
        sq_prepare_queries(b);
        sq_coarse_and_plan(b);
        if (b.scan) {
            sq_scan(b);
            sq_rerank(b);
        }
        sq_direct(b);
        if (step < nq) {
            HIPANN_CHECK(hipMemcpyAsync(ix.probes.get<int64_t>() + q0 * np, sh.coarse_i.p,
                                        sizeof(int64_t) * (size_t)nqs * np, hipMemcpyDeviceToDevice, st));
            ix.probes_kept = true;
        }
    }
}

// ---- range search (ivf_sq8_range.hip): one query slice, the stages in their order on the stream ----
// The slots' masks take 256 bytes per (query, probe, chunk) slot, a query's slots bounded by the chunk counts of its
// nprobe longest lists (ivf_sq_query_slots); above 64 MiB of masks the batch runs in query slices with lims chained on
// the device — IVFFlat's rule (ivf.cpp kRangeMaskBudget), restated.  The masks, counts, offsets, lims and the stage
// events are the core shard's range scratch (rg_*), under the handle's lock.
constexpr int64_t kSqRangeMaskBudget = (int64_t)64 << 20;

struct SqRangeSlice {
    IvfSqRangeArgs a;
    IvfPlanView plan{};
    int64_t slots = 0;  // the host's bound of the slice's slots
};

// a timed call's stage marks (scan | offsets | fill: begin and end each), read by hipann_debug_ivfsq_info
void sq_range_mark(bool on, IvfShard &sh, int i, hipStream_t st) {
    if (!on) return;
    if (!sh.rg_ev[i]) HIPANN_CHECK(hipEventCreate(&sh.rg_ev[i]));
    HIPANN_CHECK(hipEventRecord(sh.rg_ev[i], st));
    if (i == 0) sh.rg_ev_fill = false;
    if (i == 5) sh.rg_ev_fill = true;
}

// the scan serves dimensions whose query terms fit the LDS (the top-k scan's limit); the others the direct kernel
void sq_range_mode(SqBatch &b) {
    b.scan = ivf_sq_group(b.ix.d, kSqKeep) >= 16;
    b.group = (b.scan ? ivf_sq_range_group(b.ix.d) : 16) << 8;
    b.slots = b.nq * ivf_sq_query_slots(b.sh.h_len, b.np, ivf_chunk_rows());
    HIPANN_REQUIRE(b.slots < (int64_t)0x7fffffff, "IVF SQ8 range search: too many slots");
}

// the masks and counts of every (query, probe, chunk) slot: the threshold scan of the codes, or the direct kernel
void sq_range_scan(SqBatch &b, SqRangeSlice &r, float radius) {
    IvfSqIndex &ix = b.ix;
    IvfShard &sh = b.sh;
    r.slots = b.slots;
    r.plan = b.plan;
    sh.rg_mask.ensure((size_t)b.slots * 256, sh.device);
    sh.rg_cnt.ensure(sizeof(int) * (size_t)b.slots, sh.device);
    if (!sh.rg_stat.p) {
        sh.rg_stat.ensure(2 * sizeof(unsigned long long), sh.device);
        HIPANN_CHECK(hipMemsetAsync(sh.rg_stat.p, 0, 2 * sizeof(unsigned long long), b.st));
    }
    IvfSqRangeArgs &a = r.a;
    a.Q = b.xq, a.nq = b.nq, a.radius = radius, a.probes = sh.coarse_i.get<int64_t>(), a.max_nch = std::max(sh.max_nch, 1);
    a.mask = sh.rg_mask.get<unsigned>(), a.counts = sh.rg_cnt.get<int>();
    RoctxRange rr("hipann.ivfsq.range_scan");
    ScopedTiming t(ix.timer_main, b.st);
    sq_range_mark(ix.timer_main.on, sh, 0, b.st);
    if (b.scan) {
        a.qimg = ix.qimg.p, a.par = ix.par.get<float>(), a.pair_a = ix.pair_a.get<float>();
        a.stat = sh.rg_stat.get<unsigned long long>();
        launch_ivf_sq_range_scan(a, b.v, b.plan, b.group,
                                 ivf_max_items(b.nq, b.np, ix.core->nlist, sh.max_nch, sh.n, b.group), b.st);
    } else {
        launch_ivf_sq_range_direct(a, b.v, b.plan, b.st);
    }
    sq_range_mark(ix.timer_main.on, sh, 1, b.st);
}

// slot offsets, pair limits and the slice's lims (chain: continuing from lims[0], the slice before)
void sq_range_offsets(SqBatch &b, SqRangeSlice &r, int64_t *lims_dev, bool chain) {
    IvfShard &sh = b.sh;
    sh.rg_soff.ensure(sizeof(int64_t) * ((size_t)r.slots + 1), sh.device);
    sh.rg_plim.ensure(sizeof(int64_t) * ((size_t)b.nq * b.np + 1), sh.device);
    sq_range_mark(b.ix.timer_main.on, sh, 2, b.st);
    launch_ivf_range_offsets(r.a.counts, r.plan.slot_off, b.nq, b.np, chain, sh.rg_soff.get<int64_t>(),
                             sh.rg_plim.get<int64_t>(), lims_dev, b.st);
    sq_range_mark(b.ix.timer_main.on, sh, 3, b.st);
}

// (distance, id) of the slice's admitted rows at their offsets in D / I
void sq_range_fill(IvfSqIndex &ix, const SqRangeSlice &r, float *D, int64_t *I, hipStream_t st) {
    IvfShard &sh = *ix.core->shards[0];
    RoctxRange rr("hipann.ivfsq.range_fill");
    sq_range_mark(ix.timer_main.on, sh, 4, st);  // (hipann_last_kernel_ms reports the threshold scan alone)
    launch_ivf_sq_range_fill(r.a, sq_view(ix), r.plan, sh.rg_soff.get<int64_t>(), D, I, st);
    sq_range_mark(ix.timer_main.on, sh, 5, st);
}

// Query preparation, coarse step, plan, scan and offsets of one slice: lims_dev (nq + 1, device) is written, the slice
// is ready to fill.
SqRangeSlice sq_range_count(IvfSqIndex &ix, int np, int64_t nq, const float *xq, float radius, int64_t *lims_dev,
                            bool chain, hipStream_t st) {
    IvfShard &sh = *ix.core->shards[0];
    SqBatch b{ix, sh, sq_view(ix), nq, xq, 1, np, nullptr, nullptr, st};
    SqRangeSlice r;
    sq_range_mode(b);
    sq_prepare_queries(b);
    sq_coarse_and_plan(b);
    sq_range_scan(b, r, radius);
    sq_range_offsets(b, r, lims_dev, chain);
    return r;
}

int64_t sq_range_slice_queries(const IvfSqIndex &ix, int np) {
    const int64_t qslots = ivf_sq_query_slots(ix.core->shards[0]->h_len, np, ivf_chunk_rows());
    return std::max<int64_t>(1, (ix.range_mask_budget > 0 ? ix.range_mask_budget : kSqRangeMaskBudget) / (qslots * 256));
}

// a sliced batch's probe lists, kept for hipann_ivfsq_last_probes (the coarse step's buffer holds one slice's)
void sq_range_keep_probes(IvfSqIndex &ix, int64_t q0, int64_t nqs, int np, hipStream_t st) {
    HIPANN_CHECK(hipMemcpyAsync(ix.probes.get<int64_t>() + q0 * np, ix.core->shards[0]->coarse_i.p,
                                sizeof(int64_t) * (size_t)nqs * np, hipMemcpyDeviceToDevice, st));
    ix.probes_kept = true;
}

// Host variant.  Per query slice: count, one synchronisation for the slice's lims, fill, the rows back.
int sq_range_host(IvfSqIndex &ix, int nprobe, int64_t nq, const float *xq, float radius, int64_t *lims, float **D,
                  int64_t **I) {
    HIPANN_REQUIRE(lims && D && I, "null output");
    HIPANN_REQUIRE(nq >= 0 && (nq == 0 || xq), "invalid arguments");
    HIPANN_REQUIRE(radius == radius, "radius is NaN");
    *D = nullptr, *I = nullptr;
    std::fill(lims, lims + nq + 1, (int64_t)0);
    IvfShard &sh = *ix.core->shards[0];
    DeviceGuard g(sh.device);
    const int np = ivf_sq_call_nprobe(nprobe, ix.core->nprobe, ix.core->nlist);
    ix.last_nq = sh.live == 0 ? 0 : nq;
    ix.last_np = np;
    ix.probes_kept = false;
    if (nq == 0 || sh.live == 0) return 0;
    const hipStream_t st = sh.stream;
    const size_t qbytes = (size_t)nq * ix.d * sizeof(float);
    ix.h_q.ensure(qbytes);
    std::memcpy(ix.h_q.p, xq, qbytes);
    ix.q.ensure(qbytes, sh.device);
    const int64_t qs = sq_range_slice_queries(ix, np);
    if (qs < nq) ix.probes.ensure(sizeof(int64_t) * (size_t)nq * np, sh.device);
    FenceScope fs(sh.fence, st, sh.device);
    HIPANN_CHECK(hipMemcpyAsync(ix.q.p, ix.h_q.p, qbytes, hipMemcpyHostToDevice, st));
    float *od = nullptr;
    int64_t *oi = nullptr;
    int64_t run = 0;
    try {
        for (int64_t q0 = 0; q0 < nq; q0 += qs) {
            const int64_t nqs = std::min(qs, nq - q0);
            const size_t lbytes = sizeof(int64_t) * (size_t)(nqs + 1);
            sh.rg_lims.ensure(lbytes, sh.device);
            sh.h_rg.ensure(lbytes);
            const SqRangeSlice r = sq_range_count(ix, np, nqs, ix.q.get<float>() + q0 * ix.d, radius,
                                                  sh.rg_lims.get<int64_t>(), false, st);
            HIPANN_CHECK(hipMemcpyAsync(sh.h_rg.p, sh.rg_lims.p, lbytes, hipMemcpyDeviceToHost, st));
            if (qs < nq) sq_range_keep_probes(ix, q0, nqs, np, st);
            HIPANN_CHECK(hipStreamSynchronize(st));
            const int64_t *hl = sh.h_rg.get<int64_t>();
            const int64_t total = hl[nqs];
            for (int64_t i = 0; i < nqs; ++i) lims[q0 + i] = run + hl[i];
            if (total == 0) continue;
            float *nd = static_cast<float *>(std::realloc(od, sizeof(float) * (size_t)(run + total)));
            if (nd) od = nd;
            int64_t *ni = static_cast<int64_t *>(std::realloc(oi, sizeof(int64_t) * (size_t)(run + total)));
            if (ni) oi = ni;
            HIPANN_REQUIRE(nd && ni, "range search: out of host memory");
            sh.rg_d.ensure(sizeof(float) * (size_t)total, sh.device);
            sh.rg_i.ensure(sizeof(int64_t) * (size_t)total, sh.device);
            sq_range_fill(ix, r, sh.rg_d.get<float>(), sh.rg_i.get<int64_t>(), st);
            HIPANN_CHECK(hipMemcpyAsync(od + run, sh.rg_d.p, sizeof(float) * (size_t)total, hipMemcpyDeviceToHost, st));
            HIPANN_CHECK(hipMemcpyAsync(oi + run, sh.rg_i.p, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToHost, st));
            HIPANN_CHECK(hipStreamSynchronize(st));
            run += total;
        }
        lims[nq] = run;
    } catch (...) {
        std::free(od);
        std::free(oi);
        throw;
    }
    *D = od, *I = oi;
    return 0;
}

// Device variant.  One slice: count, read the total back, fill.  Several: every slice counts first (lims chained from
// slice to slice), the total is read back, and only a result that fits runs the slices again, each with its fill.
int sq_range_device(IvfSqIndex &ix, int nprobe, int64_t nq, const float *xq, float radius, int64_t *lims_dev, float *D,
                    int64_t *I, int64_t cap, hipStream_t st) {
    IvfShard &sh = *ix.core->shards[0];
    DeviceGuard g(sh.device);
    FenceScope fs(sh.fence, st, sh.device);
    const int np = ivf_sq_call_nprobe(nprobe, ix.core->nprobe, ix.core->nlist);
    ix.last_nq = sh.live == 0 ? 0 : nq;
    ix.last_np = np;
    ix.probes_kept = false;
    if (nq == 0 || sh.live == 0) {
        HIPANN_CHECK(hipMemsetAsync(lims_dev, 0, sizeof(int64_t) * (size_t)(nq + 1), st));
        return 0;
    }
    const int64_t qs = sq_range_slice_queries(ix, np);
    const bool sliced = qs < nq;
    if (sliced) ix.probes.ensure(sizeof(int64_t) * (size_t)nq * np, sh.device);
    SqRangeSlice one;
    for (int64_t q0 = 0; q0 < nq; q0 += qs) {
        const int64_t nqs = std::min(qs, nq - q0);
        one = sq_range_count(ix, np, nqs, xq + q0 * ix.d, radius, lims_dev + q0, q0 > 0, st);
        if (sliced) sq_range_keep_probes(ix, q0, nqs, np, st);
    }
    sh.h_rg.ensure(sizeof(int64_t));
    HIPANN_CHECK(hipMemcpyAsync(sh.h_rg.p, lims_dev + nq, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));  // the one readback: the total, against cap
    const int64_t total = *sh.h_rg.get<int64_t>();
    if (total > cap) return 1;
    if (total == 0) return 0;
    if (!sliced) {
        sq_range_fill(ix, one, D, I, st);
        return 0;
    }
    for (int64_t q0 = 0; q0 < nq; q0 += qs) {
        const int64_t nqs = std::min(qs, nq - q0);
        const SqRangeSlice r = sq_range_count(ix, np, nqs, xq + q0 * ix.d, radius, lims_dev + q0, q0 > 0, st);
        sq_range_fill(ix, r, D, I, st);
    }
    return 0;
}

// ---- train: the assignment in blocks of 65536 rows (by_residual), then the column min / max ----
void sq_train_device(int d, int metric, int nlist, int by_residual, const float *cen_dev, int64_t n, const float *x_dev,
                     int device, float *vmin_dev, float *vdiff_dev, hipStream_t st) {
    DeviceGuard g(device);
    DevBuf assign, cd, bits;
    bits.ensure(sizeof(unsigned) * 2 * (size_t)d, device);
    std::unique_ptr<FlatIndex> quant;
    if (by_residual) {
        const int64_t bs = 65536;
        assign.ensure(sizeof(int64_t) * (size_t)n, device);
        cd.ensure(sizeof(float) * (size_t)std::min(n, bs), device);
        quant = ivf_make_quantizer(d, metric, cen_dev, nlist, device, st);
        for (int64_t r0 = 0; r0 < n; r0 += bs)
            flat_shard_search(*quant, *quant->shards[0], std::min(bs, n - r0), x_dev + r0 * d, 1, 1, cd.get<float>(),
                              assign.get<int64_t>() + r0, st);
    }
    launch_ivf_sq_minmax(x_dev, n, d, assign.get<int64_t>(), by_residual ? cen_dev : nullptr, nlist,
                         bits.get<unsigned>(), vmin_dev, vdiff_dev, st);
    std::vector<float> h((size_t)2 * d);
    HIPANN_CHECK(hipMemcpyAsync(h.data(), vmin_dev, sizeof(float) * d, hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipMemcpyAsync(h.data() + d, vdiff_dev, sizeof(float) * d, hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));  // (the scratch above is released on return)
    const char *bad = ivf_sq_check_trained(h.data(), h.data() + d, d);
    HIPANN_REQUIRE(!bad, bad);
}

// ---- add: n rows on the index's device; labels on the device (lab_dev), on the host (lab_host) or ntotal + i ----
// Stages, on st: the statistics-only pass of the encode kernel (non-finite rows) and the assignment in blocks of 65536
// rows; ONE readback of both; on the host the per-list counts and every row's physical destination (rows of a later
// block follow an earlier block's: i ascends); when a list overflows its slack, the grown layout — every new buffer
// is allocated before anything of the index changes, then one regroup launch and the swap; one pinned upload
// [destination | label per row | list starts]; the encode kernel; the max ‖c‖² word back and the list metadata.
// an add's staging goes back when the call ends, however it ends, unless it is small (IvfSqIndex::kAddStagingKeep)
struct AddStagingScope {
    IvfSqIndex &ix;
    ~AddStagingScope() {
        try { ix.release_add_staging(); } catch (...) {}
    }
};

void sq_add_rows(IvfSqIndex &ix, int64_t n, const float *x_dev, const int64_t *lab_dev, const int64_t *lab_host,
                 hipStream_t st) {
    IvfShard &sh = *ix.core->shards[0];
    DeviceGuard g(sh.device);
    RoctxRange rr("hipann.ivfsq.add");
    const int nlist = ix.core->nlist, d = ix.d, dev = sh.device;
    HIPANN_REQUIRE(sh.live + n < (int64_t)0x7fffffff, "more than 2^31-1 rows");
    const int64_t bs = 65536, base = sh.live;
    ix.add_assign.ensure(sizeof(int64_t) * (size_t)(n + 1), dev);
    ix.add_cd.ensure(sizeof(float) * (size_t)std::min(n, bs), dev);
    ix.h_add.ensure(sizeof(int64_t) * (size_t)(n + 1));
    int64_t *assign_dev = ix.add_assign.get<int64_t>();
    unsigned *bad_dev = reinterpret_cast<unsigned *>(assign_dev + n);
    unsigned *cmax2 = reinterpret_cast<unsigned *>(ix.fb_total.get<unsigned long long>() + 1);
    HIPANN_CHECK(hipMemsetAsync(bad_dev, 0, sizeof(int64_t), st));
    launch_ivf_sq_encode_append(x_dev, n, sq_view(ix), nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                                nullptr, bad_dev, st);
    for (int64_t r0 = 0; r0 < n; r0 += bs)
        flat_shard_search(*sh.quant, *sh.quant->shards[0], std::min(bs, n - r0), x_dev + r0 * d, 1, 1,
                          ix.add_cd.get<float>(), assign_dev + r0, st);
    HIPANN_CHECK(hipMemcpyAsync(ix.h_add.p, assign_dev, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));
    const int64_t *assign = ix.h_add.get<int64_t>();
    HIPANN_REQUIRE(assign[n] == 0, "IVF SQ8 add: every entry of the rows must be finite");
    std::vector<int64_t> add(nlist, 0);
    for (int64_t i = 0; i < n; ++i) {
        HIPANN_REQUIRE(assign[i] >= 0 && assign[i] < nlist, "coarse assignment out of range");
        ++add[assign[i]];
    }
    const bool grow = ivf_sq_must_grow(sh.h_off, sh.h_len, add);
    const std::vector<int64_t> off = grow ? ivf_sq_grown_offsets(sh.h_off, sh.h_len, add) : sh.h_off;
    const std::vector<int64_t> tp = ivf_sq_pass_offsets(off.data(), nlist);
    const int64_t N = off[nlist];
    HIPANN_REQUIRE(N < (int64_t)0x7fffffff, "more than 2^31-1 physical rows");
    // everything the call allocates, before anything of the index changes
    DevBuf codes_new, ids_new, rown_new, tp_new;
    if (grow) {
        codes_new.ensure((size_t)tp[nlist] * ix.nstep * 1024, dev);
        ids_new.ensure(sizeof(int64_t) * (size_t)N, dev);
        if (ix.metric == kL2) rown_new.ensure(sizeof(float) * (size_t)N, dev);
        tp_new.ensure(sizeof(int64_t) * (size_t)(nlist + 1), dev);
    }
    const size_t up_n = (size_t)2 * n + 2 * ((size_t)nlist + 1);
    ix.add_up.ensure(sizeof(int64_t) * up_n, dev);
    ix.h_up.ensure(sizeof(int64_t) * up_n);
    int64_t *dst = ix.h_up.get<int64_t>(), *lab = dst + n, *hoff = lab + n, *htp = hoff + nlist + 1;
    std::vector<int64_t> len = sh.h_len;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t l = assign[i];
        dst[i] = off[l] + len[l]++;
        lab[i] = lab_host ? lab_host[i] : base + i;
    }
    std::copy(off.begin(), off.end(), hoff);
    std::copy(tp.begin(), tp.end(), htp);
    HIPANN_CHECK(hipMemcpyAsync(ix.add_up.p, ix.h_up.p, sizeof(int64_t) * up_n, hipMemcpyHostToDevice, st));
    const int64_t *ddst = ix.add_up.get<int64_t>(), *dlab = ddst + n, *doff = dlab + n, *dtp = doff + nlist + 1;
    if (grow) {
        HIPANN_CHECK(hipMemcpyAsync(tp_new.p, dtp, sizeof(int64_t) * (size_t)(nlist + 1), hipMemcpyDeviceToDevice, st));
        launch_ivf_sq_regroup(sq_view(ix), sh.list_off.get<int64_t>(), sh.list_len.get<int>(), tp_new.get<int64_t>(), doff,
                              tp[nlist], N, codes_new.get<unsigned char>(), ids_new.get<int64_t>(),
                              rown_new.get<float>(), st);
        HIPANN_CHECK(hipStreamSynchronize(st));  // the old buffers are freed when the locals above go
        auto take = [](DevBuf &a, DevBuf &b) {
            std::swap(a.p, b.p);
            std::swap(a.bytes, b.bytes);
            std::swap(a.device, b.device);
        };
        take(ix.codes_t, codes_new);
        take(sh.ids_buf, ids_new);
        if (ix.metric == kL2) take(ix.rown, rown_new);
        take(ix.tpass_off, tp_new);
        sh.ids = sh.ids_buf.get<int64_t>();
        ix.total_pass = tp[nlist];
    }
    launch_ivf_sq_encode_append(x_dev, n, sq_view(ix), assign_dev, ddst, lab_dev ? lab_dev : dlab, base, doff,
                                ix.codes_t.get<unsigned char>(), ix.rown.get<float>(), sh.ids_buf.get<int64_t>(), cmax2,
                                nullptr, st);
    float *c2 = reinterpret_cast<float *>(ix.h_add.p);
    HIPANN_CHECK(hipMemcpyAsync(c2, cmax2, sizeof(float), hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));
    // the certificate's Cauchy-Schwarz term covers the new rows from here on (the create-time formula)
    ix.cmax = std::max(ix.cmax, std::sqrt(*c2) * 1.0001f);
    ivf_set_list_meta(sh, off, len, nlist);
}

// ---- remove: every row whose label is in lab (sorted, unique) leaves its list, in FAISS's order ----
// Stages, on st: the labels up; ALL scratch (labels, one mark byte and one plan int per physical row, one new length
// per list) allocated before the launch, so a failed allocation leaves the handle as it was; the one kernel
// (ivf_sq8_remove.hip); the new lengths back in one copy; the host mirror through ivf_set_list_meta.  List starts,
// pass offsets and every buffer of the index stay: the freed rows are append slack.  cmax stays too — obligation (1)
// of ivf_sq8.hip asks for an upper bound of ‖c‖ over the rows held, and the maximum over a superset of them is one.
int64_t sq_remove_rows(IvfSqIndex &ix, const std::vector<int64_t> &lab, hipStream_t st) {
    IvfShard &sh = *ix.core->shards[0];
    if (!sh.live || lab.empty()) return 0;
    DeviceGuard g(sh.device);
    RoctxRange rr("hipann.ivfsq.remove");
    const int nlist = ix.core->nlist, dev = sh.device;
    const int64_t m = (int64_t)lab.size();
    DevBuf labels, mark, plan, newlen;
    labels.ensure(sizeof(int64_t) * (size_t)m, dev);
    mark.ensure((size_t)sh.n, dev);
    plan.ensure(sizeof(int) * (size_t)sh.n, dev);
    newlen.ensure(sizeof(int) * (size_t)nlist, dev);
    std::vector<int> hl((size_t)nlist);
    std::vector<int64_t> len = sh.h_len;
    HIPANN_CHECK(hipMemcpyAsync(labels.p, lab.data(), sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, st));
    {
        ScopedTiming t(ix.timer_main, st);
        launch_ivf_sq_remove_rows(labels.get<int64_t>(), m, sq_view(ix), sh.list_off.get<int64_t>(),
                                  sh.list_len.get<int>(), ix.codes_t.get<unsigned char>(), sh.ids_buf.get<int64_t>(),
                                  ix.rown.get<float>(), mark.get<unsigned char>(), plan.get<int>(), newlen.get<int>(), st);
    }
    HIPANN_CHECK(hipMemcpyAsync(hl.data(), newlen.p, sizeof(int) * (size_t)nlist, hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));  // (the scratch above is released on return)
    const int64_t removed = ivf_sq_removed_lengths(len, hl.data());
    HIPANN_REQUIRE(removed >= 0, "IVF SQ8 remove: a list's new length is out of range");
    if (removed > 0) ivf_set_list_meta(sh, sh.h_off, len, nlist);  // h_len, live, max_nch and the device lengths
    return removed;
}

}  // namespace

extern "C" {

int hipann_ivfsq_train_device(int d, int metric, int nlist, int by_residual, const float *centroids_dev, int64_t n,
                              const float *x_dev, int device, float *vmin_dev, float *vdiff_dev, void *stream, char *eb,
                              int el) {
    return guard<int>(eb, el, -1, [&]() -> int {
        int ndevs = 0;
        if (hipGetDeviceCount(&ndevs) != hipSuccess || ndevs <= 0) throw HipError("hipann: no HIP device");
        const char *bad = ivf_sq_check_train(d, metric, nlist, by_residual, centroids_dev != nullptr, n, x_dev != nullptr,
                                             vmin_dev && vdiff_dev);
        HIPANN_REQUIRE(!bad, bad);
        HIPANN_REQUIRE(device >= 0 && device < ndevs, "invalid device");
        sq_train_device(d, metric, nlist, by_residual ? 1 : 0, centroids_dev, n, x_dev, device, vmin_dev, vdiff_dev,
                        static_cast<hipStream_t>(stream));
        return 0;
    });
}

int hipann_ivfsq_train(int d, int metric, int nlist, int by_residual, const float *centroids, int64_t n, const float *x,
                       int device, float *vmin, float *vdiff, char *eb, int el) {
    return guard<int>(eb, el, -1, [&]() -> int {
        int ndevs = 0;
        if (hipGetDeviceCount(&ndevs) != hipSuccess || ndevs <= 0) throw HipError("hipann: no HIP device");
        const char *bad = ivf_sq_check_train(d, metric, nlist, by_residual, centroids != nullptr, n, x != nullptr,
                                             vmin && vdiff);
        HIPANN_REQUIRE(!bad, bad);
        HIPANN_REQUIRE(device >= 0 && device < ndevs, "invalid device");
        DeviceGuard g(device);
        DevBuf rows, cen, out;
        rows.ensure(sizeof(float) * (size_t)n * d, device);
        out.ensure(sizeof(float) * 2 * (size_t)d, device);
        HIPANN_CHECK(hipMemcpy(rows.p, x, sizeof(float) * (size_t)n * d, hipMemcpyHostToDevice));
        if (by_residual) {
            cen.ensure(sizeof(float) * (size_t)nlist * d, device);
            HIPANN_CHECK(hipMemcpy(cen.p, centroids, sizeof(float) * (size_t)nlist * d, hipMemcpyHostToDevice));
        }
        hipStream_t st = nullptr;
        HIPANN_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        try {
            sq_train_device(d, metric, nlist, by_residual ? 1 : 0, cen.get<float>(), n, rows.get<float>(), device,
                            out.get<float>(), out.get<float>() + d, st);
        } catch (...) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
            throw;
        }
        HIPANN_CHECK(hipStreamDestroy(st));
        HIPANN_CHECK(hipMemcpy(vmin, out.p, sizeof(float) * d, hipMemcpyDeviceToHost));
        HIPANN_CHECK(hipMemcpy(vdiff, out.get<float>() + d, sizeof(float) * d, hipMemcpyDeviceToHost));
        return 0;
    });
}

int hipann_ivfsq_add_device(void *h, int64_t n, const float *xb_dev, const int64_t *ids_dev, void *stream, char *eb,
                            int el) {
    return guard<int>(eb, el, -1, [&]() -> int {
        IvfSqIndex *ix = as_sq(h);
        HIPANN_REQUIRE(ix, "not an IVF SQ8 index");
        HIPANN_REQUIRE(n >= 0 && (n == 0 || xb_dev), "invalid arguments");
        if (n == 0) return 0;
        std::lock_guard<std::mutex> lk(ix->mu);
        IvfShard &sh = *ix->core->shards[0];
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : sh.stream;
        FenceScope fs(sh.fence, st, sh.device);
        AddStagingScope staging{*ix};
        sq_add_rows(*ix, n, xb_dev, ids_dev, nullptr, st);
        return 0;
    });
}

int hipann_ivfsq_add(void *h, int64_t n, const float *xb, const int64_t *ids, char *eb, int el) {
    return guard<int>(eb, el, -1, [&]() -> int {
        IvfSqIndex *ix = as_sq(h);
        HIPANN_REQUIRE(ix, "not an IVF SQ8 index");
        HIPANN_REQUIRE(n >= 0 && (n == 0 || xb), "invalid arguments");
        if (n == 0) return 0;
        std::lock_guard<std::mutex> lk(ix->mu);
        IvfShard &sh = *ix->core->shards[0];
        DeviceGuard g(sh.device);
        FenceScope fs(sh.fence, sh.stream, sh.device);
        AddStagingScope staging{*ix};
        // the whole call's rows on the device (n·d·4 bytes of staging: the refusal of a non-finite row comes before
        // any row is appended, so no block can be committed ahead of a later block's check)
        ix->add_rows.ensure(sizeof(float) * (size_t)n * ix->d, sh.device);
        HIPANN_CHECK(hipMemcpyAsync(ix->add_rows.p, xb, sizeof(float) * (size_t)n * ix->d, hipMemcpyHostToDevice, sh.stream));
        sq_add_rows(*ix, n, ix->add_rows.get<float>(), nullptr, ids, sh.stream);
        return 0;
    });
}

int64_t hipann_ivfsq_remove_ids(void *h, const int64_t *labels, int64_t n, char *eb, int el) {
    return guard<int64_t>(eb, el, -1, [&]() -> int64_t {
        IvfSqIndex *ix = as_sq(h);
        HIPANN_REQUIRE(ix, "not an IVF SQ8 index");
        HIPANN_REQUIRE(n >= 0 && (n == 0 || labels), "invalid labels");
        if (n == 0) return 0;
        std::lock_guard<std::mutex> lk(ix->mu);
        IvfShard &sh = *ix->core->shards[0];
        FenceScope fs(sh.fence, sh.stream, sh.device);
        return sq_remove_rows(*ix, ivf_sq_label_set(labels, n), sh.stream);
    });
}

void *hipann_ivfsq_create(int d, int metric, int nlist, int nprobe, int by_residual, const float *centroids,
                          const float *vmin, const float *vdiff, const int64_t *list_offsets, const int64_t *ids,
                          const uint8_t *codes, int device, char *eb, int el) {
    return guard<void *>(eb, el, nullptr, [&]() -> void * {
        int ndevs = 0;
        if (hipGetDeviceCount(&ndevs) != hipSuccess || ndevs <= 0) throw HipError("hipann: no HIP device");
        const char *bad = ivf_sq_check_create(d, metric, nlist, nprobe, centroids, vmin, vdiff, list_offsets, ids, codes);
        HIPANN_REQUIRE(!bad, bad);
        HIPANN_REQUIRE(device >= 0 && device < ndevs, "invalid device");
        auto ix = std::make_unique<IvfSqIndex>();
        ix->d = d, ix->metric = metric, ix->by_residual = by_residual ? 1 : 0;
        ix->core = ivf_make_core(d, metric, nlist, nprobe, centroids, list_offsets, ids, device);
        IvfShard &sh = *ix->core->shards[0];
        DeviceGuard g(device);
        const hipStream_t st = sh.stream;
        const int64_t n = list_offsets[nlist];
        ix->nstep = ivf_sq_nstep(d);
        const int dpad = 32 * ix->nstep;
        ivf_sq_magnitudes(centroids, nlist, d, by_residual != 0, vmin, vdiff, &ix->gmax, &ix->mnorm);
        const std::vector<float> sb = ivf_sq_scale_bias(vmin, vdiff, d, dpad);
        const std::vector<int64_t> tp = ivf_sq_pass_offsets(list_offsets, nlist);
        ix->total_pass = tp[nlist];
        ix->vmin.ensure(sizeof(float) * d, device);
        ix->vdiff.ensure(sizeof(float) * d, device);
        ix->sb.ensure(sizeof(float) * sb.size(), device);
        ix->tpass_off.ensure(sizeof(int64_t) * tp.size(), device);
        ix->fb_total.ensure(3 * sizeof(unsigned long long), device);  // [flagged since creation | max ‖c‖² bits | rechecked]
        HIPANN_CHECK(hipMemcpyAsync(ix->vmin.p, vmin, sizeof(float) * d, hipMemcpyHostToDevice, st));
        HIPANN_CHECK(hipMemcpyAsync(ix->vdiff.p, vdiff, sizeof(float) * d, hipMemcpyHostToDevice, st));
        HIPANN_CHECK(hipMemcpyAsync(ix->sb.p, sb.data(), sizeof(float) * sb.size(), hipMemcpyHostToDevice, st));
        HIPANN_CHECK(hipMemcpyAsync(ix->tpass_off.p, tp.data(), sizeof(int64_t) * tp.size(), hipMemcpyHostToDevice, st));
        HIPANN_CHECK(hipMemsetAsync(ix->fb_total.p, 0, 3 * sizeof(unsigned long long), st));
        // (L2's row terms exist for an empty index too: the scan of no items still takes the pointer)
        if (metric == kL2) ix->rown.ensure(sizeof(float) * (size_t)std::max<int64_t>(n, 1), device);
        if (n > 0) {
            // the row-major codes live on the device only until they are tiled and N(row), max ‖c‖² are taken
            DevBuf raw;
            raw.ensure((size_t)n * d, device);
            HIPANN_CHECK(hipMemcpyAsync(raw.p, codes, (size_t)n * d, hipMemcpyHostToDevice, st));
            ix->codes_t.ensure((size_t)ix->total_pass * ix->nstep * 1024, device);
            const IvfSqView v = sq_view(*ix);
            launch_ivf_sq_tile(raw.get<unsigned char>(), sh.list_off.get<int64_t>(), sh.list_len.get<int>(),
                               ix->tpass_off.get<int64_t>(), nlist, ix->total_pass, d, ix->nstep,
                               ix->codes_t.get<unsigned char>(), st);
            unsigned *cmax2 = reinterpret_cast<unsigned *>(ix->fb_total.get<unsigned long long>() + 1);
            launch_ivf_sq_row_terms(raw.get<unsigned char>(), v, sh.list_off.get<int64_t>(), nlist, ix->rown.get<float>(),
                                    cmax2, st);
            float c2 = 0.f;
            HIPANN_CHECK(hipMemcpyAsync(&c2, cmax2, sizeof(float), hipMemcpyDeviceToHost, st));
            HIPANN_CHECK(hipStreamSynchronize(st));
            ix->cmax = std::sqrt(c2) * 1.0001f;
        }
        HIPANN_CHECK(hipStreamSynchronize(st));
        return ix.release();
    });
}

int hipann_ivfsq_search_device(void *h, int nprobe, int64_t nq, const float *xq_dev, int64_t k, float *D_dev,
                               int64_t *I_dev, void *stream, char *eb, int el) {
    return guard<int>(eb, el, -1, [&]() -> int {
        IvfSqIndex *ix = as_sq(h);
        HIPANN_REQUIRE(ix, "not an IVF SQ8 index");
        std::lock_guard<std::mutex> lk(ix->mu);
        const char *bad = ivf_sq_check_search(nq, k, HIPANN_MAX_K, xq_dev && D_dev && I_dev);
        HIPANN_REQUIRE(!bad, bad);
        IvfShard &sh = *ix->core->shards[0];
        hipStream_t st = static_cast<hipStream_t>(stream);
        FenceScope fs(sh.fence, st, sh.device);
        sq_search_device(*ix, nprobe, nq, xq_dev, (int)k, D_dev, I_dev, st);
        return 0;
    });
}

int hipann_ivfsq_search(void *h, int nprobe, int64_t nq, const float *xq, int64_t k, float *D, int64_t *I, char *eb,
                        int el) {
    return guard<int>(eb, el, -1, [&]() -> int {
        IvfSqIndex *ix = as_sq(h);
        HIPANN_REQUIRE(ix, "not an IVF SQ8 index");
        std::lock_guard<std::mutex> lk(ix->mu);
        const char *bad = ivf_sq_check_search(nq, k, HIPANN_MAX_K, xq && D && I);
        HIPANN_REQUIRE(!bad, bad);
        IvfShard &sh = *ix->core->shards[0];
        DeviceGuard g(sh.device);
        if (nq == 0) {
            ix->last_nq = 0;
            return 0;
        }
        const size_t qbytes = (size_t)nq * ix->d * sizeof(float), ob = (size_t)nq * k;
        ix->h_q.ensure(qbytes);
        ix->h_d.ensure(ob * sizeof(float));
        ix->h_i.ensure(ob * sizeof(int64_t));
        std::memcpy(ix->h_q.p, xq, qbytes);
        ix->q.ensure(qbytes, sh.device);
        ix->out_d.ensure(ob * sizeof(float), sh.device);
        ix->out_i.ensure(ob * sizeof(int64_t), sh.device);
        FenceScope fs(sh.fence, sh.stream, sh.device);
        HIPANN_CHECK(hipMemcpyAsync(ix->q.p, ix->h_q.p, qbytes, hipMemcpyHostToDevice, sh.stream));
        sq_search_device(*ix, nprobe, nq, ix->q.get<float>(), (int)k, ix->out_d.get<float>(), ix->out_i.get<int64_t>(),
                         sh.stream);
        HIPANN_CHECK(hipMemcpyAsync(ix->h_d.p, ix->out_d.p, ob * sizeof(float), hipMemcpyDeviceToHost, sh.stream));
        HIPANN_CHECK(hipMemcpyAsync(ix->h_i.p, ix->out_i.p, ob * sizeof(int64_t), hipMemcpyDeviceToHost, sh.stream));
        HIPANN_CHECK(hipStreamSynchronize(sh.stream));
        std::memcpy(D, ix->h_d.p, ob * sizeof(float));
        std::memcpy(I, ix->h_i.p, ob * sizeof(int64_t));
        return 0;
    });
}

int hipann_ivfsq_range_search(void *h, int nprobe, int64_t nq, const float *xq, float radius, int64_t *lims, float **D,
                              int64_t **I, char *eb, int el) {
    return guard<int>(eb, el, -1, [&]() -> int {
        IvfSqIndex *ix = as_sq(h);
        HIPANN_REQUIRE(ix, "not an IVF SQ8 index");
        std::lock_guard<std::mutex> lk(ix->mu);
        return sq_range_host(*ix, nprobe, nq, xq, radius, lims, D, I);
    });
}

int hipann_ivfsq_range_search_device(void *h, int nprobe, int64_t nq, const float *xq_dev, float radius,
                                     int64_t *lims_dev, float *D_dev, int64_t *I_dev, int64_t cap, void *stream, char *eb,
                                     int el) {
    return guard<int>(eb, el, -1, [&]() -> int {
        IvfSqIndex *ix = as_sq(h);
        HIPANN_REQUIRE(ix, "not an IVF SQ8 index");
        std::lock_guard<std::mutex> lk(ix->mu);
        HIPANN_REQUIRE(nq >= 0 && lims_dev && (nq == 0 || xq_dev) && cap >= 0 && (cap == 0 || (D_dev && I_dev)),
                       "invalid arguments");
        HIPANN_REQUIRE(radius == radius, "radius is NaN");
        return sq_range_device(*ix, nprobe, nq, xq_dev, radius, lims_dev, D_dev, I_dev, cap,
                               static_cast<hipStream_t>(stream));
    });
}

int hipann_ivfsq_last_probes(void *h, int64_t *probes, int64_t cap, char *eb, int el) {
    return guard<int>(eb, el, -1, [&]() -> int {
        IvfSqIndex *ix = as_sq(h);
        HIPANN_REQUIRE(ix && probes, "not an IVF SQ8 index, or a null buffer");
        std::lock_guard<std::mutex> lk(ix->mu);
        const int64_t m = ix->last_nq * ix->last_np;
        HIPANN_REQUIRE(cap >= m, "probe buffer too small");
        if (m == 0) return 0;
        IvfShard &sh = *ix->core->shards[0];
        DeviceGuard g(sh.device);
        HIPANN_CHECK(hipDeviceSynchronize());
        HIPANN_CHECK(hipMemcpy(probes, ix->probes_kept ? ix->probes.p : sh.coarse_i.p, sizeof(int64_t) * (size_t)m,
                               hipMemcpyDeviceToHost));
        return 0;
    });
}

int hipann_ivfsq_export(void *h, float *centroids, float *vmin, float *vdiff, int64_t *list_offsets, int64_t *ids,
                        uint8_t *codes, char *eb, int el) {
    return guard<int>(eb, el, -1, [&]() -> int {
        IvfSqIndex *ix = as_sq(h);
        HIPANN_REQUIRE(ix, "not an IVF SQ8 index");
        std::lock_guard<std::mutex> lk(ix->mu);
        IvfShard &sh = *ix->core->shards[0];
        DeviceGuard g(sh.device);
        HIPANN_CHECK(hipDeviceSynchronize());
        const int nlist = ix->core->nlist, d = ix->d;
        // dense CSR: the cumulative live lengths (the lists' append slack is not exported)
        const int64_t n = sh.live;
        std::vector<int64_t> doff((size_t)nlist + 1, 0);
        for (int l = 0; l < nlist; ++l) doff[l + 1] = doff[l] + sh.h_len[l];
        if (list_offsets) std::memcpy(list_offsets, doff.data(), sizeof(int64_t) * (nlist + 1));
        if (centroids) HIPANN_CHECK(hipMemcpy(centroids, sh.centroids, sizeof(float) * (size_t)nlist * d, hipMemcpyDeviceToHost));
        if (vmin) HIPANN_CHECK(hipMemcpy(vmin, ix->vmin.p, sizeof(float) * d, hipMemcpyDeviceToHost));
        if (vdiff) HIPANN_CHECK(hipMemcpy(vdiff, ix->vdiff.p, sizeof(float) * d, hipMemcpyDeviceToHost));
        if ((ids || codes) && n) {
            DevBuf raw, rid, dof;
            if (codes) raw.ensure((size_t)n * d, sh.device);
            if (ids) rid.ensure(sizeof(int64_t) * (size_t)n, sh.device);
            dof.ensure(sizeof(int64_t) * doff.size(), sh.device);
            HIPANN_CHECK(hipMemcpyAsync(dof.p, doff.data(), sizeof(int64_t) * doff.size(), hipMemcpyHostToDevice, sh.stream));
            launch_ivf_sq_untile(sq_view(*ix), sh.list_off.get<int64_t>(), sh.list_len.get<int>(), dof.get<int64_t>(),
                                 ix->total_pass, raw.get<unsigned char>(), rid.get<int64_t>(), sh.stream);
            if (codes) HIPANN_CHECK(hipMemcpyAsync(codes, raw.p, (size_t)n * d, hipMemcpyDeviceToHost, sh.stream));
            if (ids) HIPANN_CHECK(hipMemcpyAsync(ids, rid.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, sh.stream));
            HIPANN_CHECK(hipStreamSynchronize(sh.stream));
        }
        return 0;
    });
}

int64_t hipann_ivfsq_rerank_fallbacks(void *h) {
    try {
        IvfSqIndex *ix = as_sq(h);
        if (!ix) return -1;
        std::lock_guard<std::mutex> lk(ix->mu);
        IvfShard &sh = *ix->core->shards[0];
        DeviceGuard g(sh.device);
        HIPANN_CHECK(hipDeviceSynchronize());
        unsigned long long v = 0;
        HIPANN_CHECK(hipMemcpy(&v, ix->fb_total.p, sizeof(v), hipMemcpyDeviceToHost));
        return (int64_t)v;
    } catch (...) {
        return -1;
    }
}

// measurement hook (tools/ivf_sq8_bench.py, tools/ivf_sq8_range_bench.py): "rechecked" = candidates the rerank has
// recomputed in the direct form since creation; "filter_depth" = the sub-list depth of the last search call's scan
// (16, 32, or 0 for the direct kernel); "cmax" = the handle's current bound of max ‖c‖ (tests: it follows an
// add); "range_survivors" / "range_admitted" and "range_scan_ms" / "range_offsets_ms" / "range_fill_ms": the range
// scan's filter counters and the last timed range call's stages; "range_mask_budget" is an input (tests: the query slices
// of a range call at a small size); 0 on success
int hipann_debug_ivfsq_info(void *h, const char *name, double *out) {
    try {
        IvfSqIndex *ix = as_sq(h);
        if (!ix || !name || !out) return -1;
        std::lock_guard<std::mutex> lk(ix->mu);
        if (std::strcmp(name, "cmax") == 0) {
            *out = (double)ix->cmax;
            return 0;
        }
        if (std::strcmp(name, "filter_depth") == 0) {
            *out = (double)ix->last_kfilt;
            return 0;
        }
        IvfShard &sh = *ix->core->shards[0];
        const std::string s(name);
        if (s == "range_mask_budget") {  // in: the mask bytes above which a range call runs in query slices (0: 64 MiB)
            HIPANN_REQUIRE(*out >= 0.0, "negative budget");
            ix->range_mask_budget = (int64_t)*out;
            return 0;
        }
        if (s == "range_survivors" || s == "range_admitted") {
            // the range scan's filter since creation: rows sent to the recheck, rows the recheck admitted
            unsigned long long v[2] = {0, 0};
            if (sh.rg_stat.p) {
                DeviceGuard g(sh.device);
                HIPANN_CHECK(hipDeviceSynchronize());
                HIPANN_CHECK(hipMemcpy(v, sh.rg_stat.p, sizeof(v), hipMemcpyDeviceToHost));
            }
            *out = (double)v[s == "range_admitted" ? 1 : 0];
            return 0;
        }
        if (s == "range_scan_ms" || s == "range_offsets_ms" || s == "range_fill_ms") {
            // the stages of the last range call made with timing on (its last slice); 0 for a stage that did not run
            const int i = s == "range_scan_ms" ? 0 : s == "range_offsets_ms" ? 2 : 4;
            float ms = 0.f;
            if (sh.rg_ev[i] && sh.rg_ev[i + 1] && (i < 4 || sh.rg_ev_fill)) {
                DeviceGuard g(sh.device);
                HIPANN_CHECK(hipEventSynchronize(sh.rg_ev[i + 1]));
                HIPANN_CHECK(hipEventElapsedTime(&ms, sh.rg_ev[i], sh.rg_ev[i + 1]));
            }
            *out = ms;
            return 0;
        }
        if (s != "rechecked") return -1;
        DeviceGuard g(sh.device);
        HIPANN_CHECK(hipDeviceSynchronize());
        unsigned long long v = 0;
        HIPANN_CHECK(hipMemcpy(&v, ix->fb_total.get<unsigned long long>() + 2, sizeof(v), hipMemcpyDeviceToHost));
        *out = (double)v;
        return 0;
    } catch (...) {
        return -1;
    }
}

}  // extern "C"
