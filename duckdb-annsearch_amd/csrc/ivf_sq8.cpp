// ivf_sq8.cpp — IVF SQ8 part of the C ABI (include/hip_ann.h, hipann_ivfsq_*): faiss::IndexIVFScalarQuantizer with
// QT_8bit codes on one device.  The coarse step and the plan are the IVFFlat ones (ivf.hpp ivf_coarse_plan); the
// kernels are in ivf_sq8.hip, the pure host functions in ivf_sq8_host.hpp.
#include "../../include/hip_ann.h"
#include "ivf.hpp"
#include "ivf_sq8_host.hpp"

#include <cstring>
#include <exception>

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
    int group = 0;
    IvfPlanView plan{};
    int64_t slots = 0;  // the host's bound of the slice's slots
};

// the scan serves k up to its filter depth and dimensions whose query terms fit the LDS
void sq_pick_mode(SqBatch &b) {
    const int wide = ivf_sq_group(b.ix.d);
    b.scan = b.k <= kSqKeep && wide >= 16;
    b.group = b.scan ? wide << 8 : 16 << 8;
    b.slots = b.nq * ivf_sq_query_slots(b.sh.h_len, b.np, ivf_chunk_rows());
    HIPANN_REQUIRE(b.slots < (int64_t)0x7fffffff / (kSqWaves * kSqKeep), "IVF SQ8: too many slots");
    b.ix.last_form = b.scan ? 1 : 0;
    b.ix.last_kfilt = b.scan ? kSqKeep : 0;
    b.ix.last_sublists = b.scan ? kSqWaves : 0;
}

// the fp16 query terms and (1/t, E, 2E, ‖q‖²) per query
void sq_prepare_queries(SqBatch &b) {
    if (!b.scan) return;
    IvfSqIndex &ix = b.ix;
    ix.qimg.ensure((size_t)b.nq * ix.nstep * 32 * 2, b.sh.device);
    ix.par.ensure((size_t)b.nq * 16, b.sh.device);
    const float wbase = (float)((ix.gmax + ix.mnorm) * 1.0001);
    launch_ivf_sq_query_prep(b.xq, b.nq, b.v, ix.cmax, wbase, ix.qimg.p, ix.par.get<float>(), b.st);
}

// the IVFFlat coarse step and plan, then A(q, l) (IP: q·(g + b)) per pair
void sq_coarse_and_plan(SqBatch &b) {
    b.plan = ivf_coarse_plan(*b.ix.core, b.sh, b.np, b.nq, b.xq, b.group, b.st);
    if (!b.scan) return;
    b.ix.pair_a.ensure(sizeof(float) * (size_t)b.nq * b.np, b.sh.device);
    launch_ivf_sq_pair_terms(b.xq, b.nq, b.np, b.sh.coarse_i.get<int64_t>(), b.v, b.ix.pair_a.get<float>(), b.st);
}

// the code scan over the plan's items: kSqWaves sub-lists of kSqKeep (key, row) per slot
void sq_scan(SqBatch &b) {
    IvfSqIndex &ix = b.ix;
    const size_t entries = (size_t)b.slots * kSqWaves * kSqKeep;
    ix.cand_d.ensure(entries * sizeof(float), b.sh.device);
    ix.cand_i.ensure(entries * sizeof(int), b.sh.device);
    RoctxRange rr("hipann.ivfsq.scan");
    ScopedTiming t(ix.timer_main, b.st);
    launch_ivf_sq_scan(b.v, b.plan, b.group,
                       ivf_max_items(b.nq, b.np, ix.core->nlist, b.sh.max_nch, b.sh.n, b.group), ix.qimg.p,
                       ix.par.get<float>(), ix.pair_a.get<float>(), b.sh.qbound.get<unsigned>(), ix.cand_d.get<float>(),
                       ix.cand_i.get<int>(), b.st);
}

// the candidates' direct-form distances and the certificate; flagged queries into sh.nflag / ix.flagged
void sq_rerank(SqBatch &b) {
    IvfSqIndex &ix = b.ix;
    ix.flagged.ensure(sizeof(int) * (size_t)b.nq, b.sh.device);
    ScopedTiming t(ix.timer_merge, b.st);
    launch_ivf_sq_rerank(b.v, b.plan, b.sh.coarse_i.get<int64_t>(), b.xq, b.nq, b.k, ix.par.get<float>(),
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
    const int64_t slot_bytes = k <= kSqKeep        ? (int64_t)(kSqWaves * kSqKeep * 8 + kSqDirectK * 12)
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

}  // namespace

extern "C" {

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
        const int64_t n = sh.n;
        if (list_offsets) std::memcpy(list_offsets, sh.h_off.data(), sizeof(int64_t) * (nlist + 1));
        if (centroids) HIPANN_CHECK(hipMemcpy(centroids, sh.centroids, sizeof(float) * (size_t)nlist * d, hipMemcpyDeviceToHost));
        if (vmin) HIPANN_CHECK(hipMemcpy(vmin, ix->vmin.p, sizeof(float) * d, hipMemcpyDeviceToHost));
        if (vdiff) HIPANN_CHECK(hipMemcpy(vdiff, ix->vdiff.p, sizeof(float) * d, hipMemcpyDeviceToHost));
        if (ids && n) HIPANN_CHECK(hipMemcpy(ids, sh.ids, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
        if (codes && n) {
            DevBuf raw;
            raw.ensure((size_t)n * d, sh.device);
            launch_ivf_sq_untile(sq_view(*ix), sh.list_off.get<int64_t>(), sh.list_len.get<int>(), ix->total_pass,
                                 raw.get<unsigned char>(), sh.stream);
            HIPANN_CHECK(hipMemcpyAsync(codes, raw.p, (size_t)n * d, hipMemcpyDeviceToHost, sh.stream));
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

// measurement hook (tools/ivf_sq8_bench.py): "rechecked" = candidates the rerank has recomputed in the direct form since
// creation; 0 on success
int hipann_debug_ivfsq_info(void *h, const char *name, double *out) {
    try {
        IvfSqIndex *ix = as_sq(h);
        if (!ix || !name || !out || std::strcmp(name, "rechecked") != 0) return -1;
        std::lock_guard<std::mutex> lk(ix->mu);
        DeviceGuard g(ix->core->shards[0]->device);
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
