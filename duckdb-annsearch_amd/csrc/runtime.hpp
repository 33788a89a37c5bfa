// runtime.hpp — device buffers, per-handle streams/scratch and the index objects behind hip_ann.h.
#pragma once
#include "common.hpp"
#include <cstdlib>
#include <ctime>
#include <memory>
#include <mutex>
#include <vector>

namespace hipann {

struct DeviceGuard {
    int prev = 0;
    explicit DeviceGuard(int dev) {
        HIPANN_CHECK(hipGetDevice(&prev));
        if (prev != dev) HIPANN_CHECK(hipSetDevice(dev));
    }
    ~DeviceGuard() { (void)hipSetDevice(prev); }
};

// Device allocation that grows on demand (never shrinks) — the per-handle scratch arena.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int device = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) { DeviceGuard g(device); (void)hipFree(p); }
        p = nullptr;
        bytes = 0;
    }
    template <typename T> T *get() const { return static_cast<T *>(p); }
    // Grow to at least `need` bytes on `dev`.  Contents are NOT preserved.  A buffer that grows again (per-batch
    // scratch whose size follows the longest list as appends lengthen it) takes a quarter of headroom below 1 GiB, so
    // a run of appends does not free and re-allocate it — each hipFree synchronises the device — on every search
    // (HIPANN_BUF_HEADROOM=0: exact sizes, A/B).
    void ensure(size_t need, int dev) {
        if (need <= bytes && dev == device && p) return;
        static const bool headroom = [] { const char *e = std::getenv("HIPANN_BUF_HEADROOM"); return !e || std::atoi(e); }();
        const bool regrow = p && dev == device && headroom && need < ((size_t)1 << 30);
        release();
        device = dev;
        DeviceGuard g(dev);
        size_t alloc = need < 256 ? 256 : need;
        if (regrow) alloc += alloc / 4;
        HIPANN_CHECK(hipMalloc(&p, alloc));
        bytes = alloc;
    }
};

// Pinned host staging buffer.
struct HostBuf {
    void *p = nullptr;
    size_t bytes = 0;
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    ~HostBuf() { if (p) (void)hipHostFree(p); }
    // (returns true when it allocated: the contents are undefined then)
    bool ensure(size_t need, unsigned flags = hipHostMallocDefault) {
        if (need <= bytes && p) return false;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        HIPANN_CHECK(hipHostMalloc(&p, need < 256 ? 256 : need, flags));
        bytes = need < 256 ? 256 : need;
        return true;
    }
    template <typename T> T *get() const { return static_cast<T *>(p); }
};

// HIP-event timing of a kernel across calls (bench.py reads the average).
struct KernelTimer {
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    size_t used = 0;
    int device = 0;
    ~KernelTimer() { clear(); }
    void clear() {
        for (auto &e : ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
        ev.clear();
        used = 0;
    }
    void reset(bool enable, int dev) { clear(); on = enable; device = dev; }
    // Returns the event pair to record around a launch (nullptr pair when off).
    std::pair<hipEvent_t, hipEvent_t> next() {
        if (!on) return {nullptr, nullptr};
        if (used == ev.size()) {
            hipEvent_t a, b;
            // timing-only events: no system-scope fence (an L2 writeback + invalidate per record, ≈5 µs of
            // idle GPU between the timed kernel and the next launch); average_ms reads them after a sync
            HIPANN_CHECK(hipEventCreateWithFlags(&a, hipEventDisableSystemFence));
            HIPANN_CHECK(hipEventCreateWithFlags(&b, hipEventDisableSystemFence));
            ev.push_back({a, b});
        }
        return ev[used++];
    }
    double average_ms() {
        if (!used) return 0.0;
        double tot = 0.0;
        for (size_t i = 0; i < used; ++i) {
            HIPANN_CHECK(hipEventSynchronize(ev[i].second));
            float ms = 0.f;
            HIPANN_CHECK(hipEventElapsedTime(&ms, ev[i].first, ev[i].second));
            tot += ms;
        }
        return tot / (double)used;
    }
};

struct ScopedTiming {
    hipEvent_t b;
    hipStream_t s;
    ScopedTiming(KernelTimer &t, hipStream_t st) : s(st) {
        auto e = t.next();
        b = e.second;
        if (e.first) HIPANN_CHECK(hipEventRecord(e.first, st));
    }
    ~ScopedTiming() { if (b) (void)hipEventRecord(b, s); }
};

// roctx ranges around the host stages of a call (HIPANN_ROCTX=1; off by default, then a scope costs one branch):
// `rocprofv3 --marker-trace` shows each stage's enqueue span beside the kernels it launched (profiles/r06/).
bool roctx_enabled();
void roctx_push(const char *name);
void roctx_pop();
struct RoctxRange {
    bool on;
    explicit RoctxRange(const char *name) : on(roctx_enabled()) { if (on) roctx_push(name); }
    ~RoctxRange() { if (on) roctx_pop(); }
    RoctxRange(const RoctxRange &) = delete;
    RoctxRange &operator=(const RoctxRange &) = delete;
};

// Pauses a timer for a scope (the exact forms' re-runs of flagged queries stay out of the main kernel's
// timing, which the roofline reads).
struct TimerPause {
    KernelTimer &t;
    bool was;
    explicit TimerPause(KernelTimer &tt) : t(tt), was(tt.on) { t.on = false; }
    ~TimerPause() { t.on = was; }
};

// Orders a handle's calls across streams.  Every search / add of a shard runs its kernels on the caller's
// stream (device API) or the shard's own (host API) and reuses the shard's scratch (plan counts, partial
// lists, flags).  The handle mutex only covers enqueueing, so a call on another stream must not start
// before the previous call's kernels are done with that scratch: each call waits for the event the
// previous call recorded (when the streams differ) and records its own at the end.
// Host waits by polling instead of blocking.  hipStreamSynchronize / hipEventSynchronize may put the thread to
// sleep until the completion interrupt, whose wake-up adds tens of µs to every short call (r05 C2 traces: a 44 µs
// idle gap before each search after the previous one's synchronisation).  HIPANN_SPIN_WAIT=0 (A/B): the blocking
// calls.
inline bool spin_wait() {
    static const bool v = [] { const char *e = std::getenv("HIPANN_SPIN_WAIT"); return !e || std::atoi(e) != 0; }();
    return v;
}
// The spin is bounded: after HIPANN_SPIN_US microseconds (default 2000 — the C2 batch and every IVF batch finish
// inside it; a 10M-row Flat batch of ≈8 ms pays one wake-up, < 1 %) the wait blocks, so a long search does not hold a
// host core (DuckDB's worker pool runs concurrent searches).
inline int64_t spin_budget_ns() {
    static const int64_t v = [] {
        const char *e = std::getenv("HIPANN_SPIN_US");
        return (int64_t)(e ? std::atoll(e) : 2000) * 1000;
    }();
    return v;
}
inline int64_t mono_ns() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (int64_t)ts.tv_sec * 1000000000 + ts.tv_nsec;
}
// until `ev` has completed (hipEventQuery in a pause loop; errors surface as from the blocking call)
inline void wait_event(hipEvent_t ev) {
    if (spin_wait()) {
        const int64_t t_end = mono_ns() + spin_budget_ns();
        for (unsigned it = 1;; ++it) {
            const hipError_t e = hipEventQuery(ev);
            if (e == hipSuccess) return;
            if (e != hipErrorNotReady) HIPANN_CHECK(e);
            for (int i = 0; i < 16; ++i) __builtin_ia32_pause();
            if ((it & 63) == 0 && mono_ns() > t_end) break;
        }
    }
    HIPANN_CHECK(hipEventSynchronize(ev));
}
// until the token word `tok` (written by launch_post_words, the last work on `st`) reads `token`: every earlier
// kernel on the stream has completed then.  The stream is queried now and then, so a failed or finished stream
// ends the wait too (its error raised as hipStreamSynchronize would).
inline void wait_posted(const volatile unsigned *tok, unsigned token, hipStream_t st) {
    if (spin_wait()) {
        const int64_t t_end = mono_ns() + spin_budget_ns();
        for (unsigned it = 1;; ++it) {
            if (__atomic_load_n(tok, __ATOMIC_ACQUIRE) == token) return;
            if ((it & 1023) == 0) {
                const hipError_t e = hipStreamQuery(st);
                if (e == hipSuccess) return;
                if (e != hipErrorNotReady) HIPANN_CHECK(hipStreamSynchronize(st));
                if (mono_ns() > t_end) break;
            }
            __builtin_ia32_pause();
        }
    }
    HIPANN_CHECK(hipStreamSynchronize(st));
}

struct StreamFence {
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool armed = false;
    bool multi = false;  // a call has arrived on a different stream than its predecessor: events from now on
    bool ev_valid = false;  // ev holds the previous call's end
    int device = 0;
    StreamFence() = default;
    StreamFence(const StreamFence &) = delete;
    StreamFence &operator=(const StreamFence &) = delete;
    ~StreamFence() { if (ev) { DeviceGuard g(device); (void)hipEventDestroy(ev); } }
    // Adaptive.  While every call of the handle comes on one stream nothing is recorded per call — an event record is
    // a marker packet the next kernel waits behind (≈6 µs of idle GPU between consecutive searches on one stream, r05
    // kernel traces).  The first call on a different stream synchronises the handle's device once (no event of the
    // previous call exists; its stream may have been destroyed since) and switches the fence to events: from then on
    // every call records one at its end, and a call on another stream waits for it on the device (hipStreamWaitEvent)
    // — per-connection streams cost one marker per call, not a device-wide drain per alternation.
    // HIPANN_FENCE_EAGER=1: events from the first call.
    static bool eager() {
        static const bool v = [] { const char *e = std::getenv("HIPANN_FENCE_EAGER"); return e && std::atoi(e) != 0; }();
        return v;
    }
    void enter(hipStream_t st) {
        if (!armed || st == last) return;
        if (ev_valid) {
            HIPANN_CHECK(hipStreamWaitEvent(st, ev, 0));
        } else {
            DeviceGuard g(device);
            HIPANN_CHECK(hipDeviceSynchronize());
        }
        multi = true;
    }
    void leave(hipStream_t st, int dev) {
        if (eager() || multi) {
            if (!ev) {
                DeviceGuard g(dev);
                HIPANN_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            }
            HIPANN_CHECK(hipEventRecord(ev, st));
            ev_valid = true;
        }
        device = dev;
        last = st;
        armed = true;
    }
};
struct FenceScope {
    StreamFence &f;
    hipStream_t st;
    int dev;
    FenceScope(StreamFence &ff, hipStream_t s, int d) : f(ff), st(s), dev(d) { f.enter(st); }
    ~FenceScope() {
        try { f.leave(st, dev); } catch (...) {}
    }
};

enum class Kind { Flat = 1, IVF = 2 };

// One contiguous row range of a Flat index resident on one device.
struct FlatShard {
    int device = 0;
    int64_t n = 0, cap = 0;
    int64_t label_offset = 0;
    float *xb = nullptr;  // n × d fp32 (owned unless borrowed)
    bool owns = true;
    DevBuf xb_buf;        // owned storage
    DevBuf xn;            // ‖x‖² (L2 only)
    hipStream_t stream = nullptr;
    // scratch
    DevBuf q, qn, part_d, part_i, out_d, out_i;
    // IVF coarse quantizer only: the plan's per-query count step fused into the probe select (set by
    // ivf_shard_search around its coarse call; done = the select consumed it)
    struct IvfPlanHook *plan_hook = nullptr;
    const float *qn_of = nullptr;  // sh.qn holds ‖q‖² of these queries (the last search's, nq of them)
    int64_t qn_nq = 0;
    // set by the caller before a search: sh.qn already holds ‖q‖² of these queries (the IVF query preparation
    // computed it), so the search does not launch row_norms again
    const float *qn_given = nullptr;
    int64_t qn_given_nq = 0;
    DevBuf keys, run_d, run_i, run2_d, run2_i;  // k > 64 path
    DevBuf mid_d, mid_i;                        // two-level merge of the direct scan's per-wave lists
    DevBuf qsplit;                              // split-bf16 form: the batch's queries as bf16 terms
    // kFlatSplit2Exact: max row ‖x‖² (the rerank's error bound; −1 until computed / after an add), the
    // flagged queries of the last batch and the re-run's buffers
    float xmax2 = -1.f;
    DevBuf nflag, flagged, fq, fD, fI, tmpnorm;
    DevBuf crd, cri, covf, nflag2, flagged2;  // form 4: flagged queries reranked over all their buffered candidates
    // kFlatBf16Exact: tiled bf16 image of the rows (built at the first search after an add) and the
    // batch's query image
    DevBuf xb16, qimg, seed;
    DevBuf cand;  // bounded passes: per-(query, split) candidate buffers and counts
    bool xb16_ok = false;
    bool keys_bf3 = false;    // the small-table key GEMM on the bf16 matrix cores (3 terms): the IVF coarse step
    float bf16_rxmax = 0.f;  // max over rows of ‖bf16(x) − x‖ (the rerank's bound)
    // kFlatI8Exact: tiled int8 image, per-row scales, max row residual ‖x − s·x̂‖; the batch's query scales and
    // residuals (the rerank's query term)
    DevBuf xi8, xscale, qscale, qres;
    bool xi8_ok = false;
    float i8_rxmax = 0.f;
    StreamFence fence;       // cross-stream ordering of this shard's calls
    HostBuf h_nflag;         // the launch phase's flag count, read back with the results (flat_shard_finish),
                             // and the token word after it (wait_posted)
    unsigned flag_seq = 0;   // the last token posted
    DevBuf app_stat;         // an append's new-row maxima (‖x‖², int8 residual, bf16 residual²)
    hipEvent_t done = nullptr;  // multi-device search: the shard's launch phase has drained (shard 0's stream waits)
};

// What a deferred Flat shard search (flat_shard_search with a FlatPending) leaves to flat_shard_finish: the exact
// forms' flagged queries, whose count is read back into the shard's h_nflag by the launch phase.
struct FlatPending {
    enum Kind { kNone = 0, kSmallI8 = 1, kExact = 2 };
    int kind = kNone;
    int64_t nq = 0;
    const float *xq = nullptr;
    int k = 0, kout = 0;  // k of the re-run (k_user on the batched exact forms), output width
    int rerun_form = kFlatSplit3;  // the form the flagged queries re-run on (FlatForm)
    float *D = nullptr;
    int64_t *I = nullptr;
    // kExact over the bounded passes: the candidate buffers and pass bound for the all-candidate rerank
    const float *cr_d = nullptr, *cr_bound = nullptr;
    const int *cr_i = nullptr, *cr_n = nullptr;
    int cr_nsplit = 0, cr_cap = 0;
    float xmax2 = 0.f, rxmax = 0.f;
    bool i8 = false;
};

struct IndexBase {
    Kind kind;
    int d = 0;
    int metric = kL2;
    std::mutex mu;
    KernelTimer timer_main, timer_merge;
    // the last search's path (hipann_last_search_path): the scan form that ran (FlatForm / IvfForm; an exact
    // form's flagged re-runs excluded), its rerank filter depth (0: no rerank) and sub-lists per slot (IVF)
    int last_form = -1, last_kfilt = 0, last_sublists = 0;
    // per shard, set at create (enable_peer_access): 2 = on shard 0's device (no peer copy), 1 = peer access enabled
    // both ways between its device and shard 0's (the result gather rides xGMI), 0 = not available (the runtime
    // stages the gather through host memory)
    std::vector<int> peer;
    explicit IndexBase(Kind k) : kind(k) {}
    virtual ~IndexBase() = default;
    virtual int64_t ntotal() const = 0;
    virtual int64_t memory_bytes() const = 0;
};

struct FlatIndex : IndexBase {
    std::vector<std::unique_ptr<FlatShard>> shards;
    int form = kFlatI8Exact;  // BLAS-path q·x form (FlatForm); shapes the int8 passes do not take run kFlatBf16Exact
    int64_t rerank_fallbacks = 0;  // queries re-run on the 3-term path by the exact form's bound check
    int64_t cand_reranked = 0;     // form 4: flagged queries sent to the all-candidate rerank first
    int64_t host_syncs = 0;        // host synchronisations in search calls (hipann_flat_host_syncs)
    HostBuf h_q, h_d, h_i;
    DevBuf gather_d, gather_i, merged_d, merged_i;  // multi-device merge on shards[0]'s device
    FlatIndex() : IndexBase(Kind::Flat) {}
    ~FlatIndex() override;
    int64_t ntotal() const override {
        int64_t t = 0;
        for (auto &s : shards) t += s->n;
        return t;
    }
    int64_t memory_bytes() const override {
        int64_t b = 0;
        for (auto &s : shards)
            b += s->n * (int64_t)d * 4 + (metric == kL2 ? s->n * 4 : 0) + (int64_t)s->xb16.bytes +
                 (int64_t)s->xi8.bytes + (int64_t)s->xscale.bytes;
        return b;
    }
};

// IVF: CSR inverted lists resident on one device.  With several devices the lists are partitioned
// (size-balanced); every shard keeps all centroids and an empty range for lists it does not own.
struct IvfShard {
    int device = 0;
    // Physical CSR rows: list l occupies rows [h_off[l], h_off[l+1]) of codes / ids / xnorm, its first h_len[l] live
    // (the rest is append slack, zero-filled; the kernels read list_len, never the gap).  n = h_off[nlist] (the
    // physical row count every whole-table kernel walks), live = Σ h_len (ntotal).
    int64_t n = 0;
    int64_t live = 0;
    const float *centroids = nullptr;
    const float *codes = nullptr;  // n × d fp32, list-contiguous
    const int64_t *ids = nullptr;  // n labels
    DevBuf centroids_buf, codes_buf, ids_buf;  // owned storage (empty when borrowed)
    DevBuf list_off;               // int64 nlist+1 (shard-local physical row offsets: list starts)
    DevBuf list_len;               // int nlist (0 = empty or not owned)
    DevBuf xnorm;                  // ‖x‖² per row (L2; the decomposed scan form)
    std::unique_ptr<FlatIndex> quant;  // coarse quantizer over `centroids` (borrowed)
    hipStream_t stream = nullptr;
    // scratch
    DevBuf q, qn, coarse_d, coarse_i, cnt, bucket_off, item_off, cursor, bucket, slot_off, part_d, part_i, out_d, out_i;
    DevBuf qbound;                 // per query: best known k-th key (order-preserving u32; MFMA scan)
    DevBuf goff, run_cnt;          // the plan's group prefix; seeded int8 scan: the queries' appended-entry cursors
    DevBuf qsplit;                 // split-bf16 scans: the batch's queries as bf16 terms
    // kFormSplit2Exact: max row ‖x‖² (for the rerank's error bound; −1 until computed), the flagged
    // queries of the last batch and the re-run's buffers
    float xmax2 = -1.f;
    DevBuf nflag, flagged, fq, fD, fI, coarse_save, tmpnorm;
    DevBuf ccnt, qtot;             // the plan: per-list running counts (kept zero between batches), per-query slot totals
    // the fused plan + fill (ivf_planfill_q): counts and fill cursors double-buffered by batch parity
    // ([2][nlist] each in ccnt / cursor2, zeroed at allocation; each batch zeroes the other parity's pair)
    DevBuf cursor2;
    uint64_t plan_batch = 0;
    int plan_nlist = 0;
    DevBuf fpd, fpi;               // device fallback: per (flagged query, probe) partial lists
    DevBuf fb_total;               // u64 running count of flagged queries (device side)
    DevBuf fbc_d, fbc_i, fbc_done;  // ivf_fallback_chunks: per (flagged query, probe, chunk) lists, per-query counts
    int fbc_cap = 0;               // flagged queries fbc_done holds counters for (zeroed at allocation)
    // MFMA scan copy of the codes, built at the first search that uses it: per list, 32-row passes of
    // [16-dim step][2 row tiles][64 lanes][float4] (ivf_mfma.hip), zero-padded rows / dims
    std::vector<int64_t> h_off;    // host copy of list_off
    std::vector<int64_t> h_len;    // host copy of list_len (live rows per list)
    bool owns_codes = false;       // codes / ids / xnorm in codes_buf / ids_buf (else borrowed: the first add copies)
    DevBuf codes_t, tpass_off;     // tiled codes; int64 nlist+1 pass offsets
    // kFormHalfExact: tiled fp16 image of x·2^half_es (same passes as codes_t), its largest row
    // residual ‖x − x̂·2^−half_es‖ and the batch's query terms / 1/(t·s) / split residuals.
    // half_state: 0 not built, 1 built, −1 unsupported (non-finite or out-of-range codes)
    int half_state = 0, half_es = 0;
    float half_rxmax = 0.f;
    DevBuf codes_h, hsplit, hits, hres;
    // kFormI8Exact: tiled int8 image (same passes), per-row scales (xs8) and residuals ‖x − s·x̂‖ (xr8), the batch's
    // int8 queries / scales / residuals / dequantised norms (‖q̂‖², ‖q̂‖); i8_state as half_state.  Adds and removes
    // re-tile the touched passes (i8_tiled: passes tiled since creation).  i8_rxmax: the largest row residual, the IP
    // bound's only (−1: to be taken from xr8 at the next IP search; L2 certifies with each row's own residual)
    int i8_state = 0;
    float i8_rxmax = -1.f;
    int64_t i8_tiled = 0;
    DevBuf codes_i8, xs8, xr8, qi8, qs8, qres8, qhn2, qhn;
    // The exact fp16 form's choice of filter image (hipann_ivf_set_filter_image, auto): auto8 0 untested, 1 int8,
    // −1 fp16; auto8_live: the live rows at the last probation (a quarter more rows: probation again); auto8_over:
    // consecutive int8 batches whose flag count broke the byte rule.  fb_host (pinned, host-mapped): batch number
    // << 32 | flag count of the latest int8 batch, written by its fallback launch and read by the next call — no
    // host synchronisation and no stream marker in the steady state.  probe_D / probe_I: the scratch outputs of
    // probation's int8 pass (IvfSearchOpts::count_only).
    int auto8 = 0, auto8_over = 0;
    int64_t auto8_live = 0;
    HostBuf fb_host;
    uint64_t fb_seq = 0, fb_seen = 0;
    DevBuf probe_D, probe_I;
    // test hooks (hipann_debug_ivf_*, tests/test_ivf_scan_gpu.py).  dbg_stop: ivf_shard_search returns after its scan
    // step (no merge, no rerank; D / I stay unwritten).  dbg_seed: the seeded int8 scan by HIPANN_IVF_SEED (-1), off
    // (0) or on (1).  The last search's shape as the scan saw it: queries, probes, entries per slot, sub-lists, image
    // (0 none, 1 fp16, 2 int8), seeded, the first entry of the candidate runs inside part_d / part_i (-1: none) and
    // the ‖q‖² (L2 key term) the scan read.
    int dbg_stop = 0, dbg_seed = -1;
    int64_t dbg_nq = 0, dbg_cand_off = -1;
    int dbg_np = 0, dbg_kslot = 0, dbg_sub = 0, dbg_img = 0, dbg_seeded = 0, dbg_kfilt = 0;
    const float *dbg_qn = nullptr;
    // an append's staging (hipann_ivf_add): the new rows grouped by list, labels, physical destinations, norms,
    // the tiled passes they touch, and the new rows' maxima (‖x‖², |x|, fp16 residual²)
    DevBuf app_rows, app_norm, app_assign, app_up, app_stat;
    DevBuf app_cd;  // hipann_ivf_coarse_device: the coarse distances (discarded)
    // pinned: the assignment on its way down, [destinations | labels | touched passes | live lengths] on their way
    // up (one copy), the maxima on their way down
    HostBuf app_hassign, app_hup[2];
    hipEvent_t app_ev[2] = {nullptr, nullptr};  // app_hup[b]'s upload has been consumed (reused two blocks later)
    hipEvent_t app_sync = nullptr;              // the assignment readback of an append block (polled)
    int app_buf = 0;
    int max_nch = 1;  // largest list's row-chunk count
    StreamFence fence;  // cross-stream ordering of this shard's calls (its coarse quantizer's scratch included)
    hipEvent_t done = nullptr;  // multi-device search: the shard's search has drained (shard 0's stream waits)
};

struct IvfIndex : IndexBase {
    int nlist = 0, nprobe = 1;
    std::vector<int> owner;  // list → shard (size-balanced at create; appended rows follow their list)
    int form = kFormHalfExact;
    int filter_image = 2, last_filter_image = 0;  // hipann_ivf_set_filter_image (0 fp16, 1 int8, 2 auto); the last search's
    int last_seeded = 0;  // the last search's int8 scan ran seeded: two launches around ivf_seed_bound (hipann_ivf_last_seeded)
    int64_t rerank_fallbacks = 0;  // queries re-run from the host (HIPANN_IVF_HOST_FALLBACK); device re-runs: fb_total
    std::vector<std::unique_ptr<IvfShard>> shards;
    int64_t last_nq = 0;
    int last_np = 0;
    HostBuf h_q, h_d, h_i;
    DevBuf gather_d, gather_i, merged_d, merged_i;
    IvfIndex() : IndexBase(Kind::IVF) {}
    ~IvfIndex() override;
    int64_t ntotal() const override {
        int64_t t = 0;
        for (auto &s : shards) t += s->live;
        return t;
    }
    int64_t memory_bytes() const override {
        int64_t b = 0;
        for (auto &s : shards)
            b += s->n * ((int64_t)d * 4 + 8 + (metric == kL2 ? 4 : 0)) + (int64_t)nlist * d * 4 +
                 (int64_t)s->codes_h.bytes + (int64_t)s->codes_t.bytes + (int64_t)s->codes_i8.bytes + (int64_t)s->xs8.bytes +
                 (int64_t)s->xr8.bytes;
        return b;
    }
};

// Peer access between every listed device and devs[0] (hipDeviceCanAccessPeer both ways, then
// hipDeviceEnablePeerAccess; an already-enabled pair counts as enabled).  Returns the per-shard state of IndexBase::peer.
std::vector<int> enable_peer_access(const std::vector<int> &devs);

// ---- kernel launchers (flat_kernels.hip, ivf_kernels.hip, ivf_mfma.hip) ----
// host-pointer calls up to this many bytes each way move queries / results with a copy kernel through
// the pinned buffers' device mapping instead of DMA round trips
constexpr size_t kKernelCopyMax = (size_t)64 << 10;
void launch_copy_words(const void *src, void *dst, size_t bytes, hipStream_t st);
// `words` words from device memory to a pinned host buffer (through its device mapping), then `token` into the
// word after them once the copy is visible to the host: the host spins on the token (wait_posted) instead of a
// stream synchronisation.
void launch_post_words(const void *src, void *host_dst, int words, unsigned token, hipStream_t st);
void *host_device_ptr(void *pinned);
void launch_row_norms(const float *x, int64_t n, int d, float *out, hipStream_t st);
size_t gemm_smem_bytes();
void launch_flat_gemm_topk(const float *Q, const float *qn, int64_t nq, const float *X, const float *xn, int64_t N,
                           int d, int metric, int k, int nsplit, int64_t tiles_per_split, float *pd, int *pi,
                           hipStream_t st);
size_t flat_bf_qsplit_bytes(int64_t nq, int d, int np);
void launch_flat_gemm_topk_bf(int np, const float *Q, const float *qn, int64_t nq, void *qsplit, const float *X,
                              const float *xn, int64_t N, int d, int metric, int k, int nsplit, int64_t tiles_per_split,
                              float *pd, int *pi, int qmajor, hipStream_t st);
size_t scan_smem_bytes(int nq, int d);
void launch_flat_gemm_keys(const float *Q, const float *qn, int64_t nq, const float *X, const float *xn, int64_t N,
                           int d, int metric, float *keys, int64_t ldk, hipStream_t st, bool bf3 = false);
void launch_flat_scan_keys(const float *Q, int nq, const float *X, int64_t N, int d, int metric, float *keys,
                           int64_t ldk, hipStream_t st);
void launch_rows_topk(const float *keys, int64_t ldk, int64_t ncols, int64_t nq, int64_t seg_len, int nseg, int k,
                      int id0, float *pd, int *pi, hipStream_t st);
bool launch_rows_select_out(const float *keys, int64_t ldk, int64_t ncols, int64_t nq, int k, int kout,
                            int64_t label_offset, float out_sign, float *D, int64_t *I, hipStream_t st,
                            IvfPlanHook *hook = nullptr);
void launch_merge_raw(const float *pd, const int *pi, int nparts, int64_t nq, int k, float *od, int *oi,
                      hipStream_t st);
void launch_flat_scan_topk(const float *Q, int nq, const float *X, int64_t N, int d, int metric, int k, int nwaves,
                           int64_t rows_per_wave, float *pd, int *pi, hipStream_t st);
// What launch_ivf_plan leaves for the scans (device arrays; goff: the group prefix, read by the seeded image scan only).
struct IvfPlanView {
    const int64_t *list_off;
    const int *list_len, *cnt, *bucket_off, *item_off, *bucket, *slot_off, *goff;
    int nlist, nprobe;
};
// the nine leading plan parameters of every item scan kernel, in their order
#define HIPANN_PLAN_ARGS(p) \
    (p).list_off, (p).list_len, (p).cnt, (p).bucket_off, (p).item_off, (p).bucket, (p).slot_off, (p).nlist, (p).nprobe
void launch_ivf_plan(const int64_t *probes, int64_t nq, int nprobe, const int *list_len, int nlist, int group,
                     int *cnt, int *bucket_off, int *item_off, int *cursor, int *bucket, int *slot_off,
                     hipStream_t st, int *nflag_reset, unsigned *qbound, int *ccnt, int *qtot, bool counted,
                     int *ccnt_next, int *cursor_next,
                     // goff[l] = the query groups of the lists before l (nlist + 1 entries): list l's chunk-0 items
                     int *goff);
int64_t ivf_max_items(int64_t nq, int nprobe, int nlist, int max_nch, int64_t nrows, int group);
int ivf_mfma_bf_group(int d, int np);
bool ivf_mfma_bf_supported(int d, bool aligned16, int k, int np);
bool ivf_mfma_bf_supported(const float *Q, int d, const float *codes, int k, int np);
int64_t ivf_mfma_bf_qsplit_bytes(int64_t nq, int d, int np);
// Form 4 (bounded passes): the flagged queries' exact top-kout over ALL their buffered candidates, certified
// against the pass bound (every unbuffered row has scan key > bound[q]); queries it cannot certify (a cell
// overflowed, or the k-th distance within the error bound of bound[q]) are appended to flagged2.
struct FlatCandRerankArgs {
    const int *flagged = nullptr;  // the nf flagged queries
    int nf = 0;
    // the passes' candidate buffers (nsplit cells of cap entries per query), their counts and the pass bound
    const float *cand_d = nullptr;
    const int *cand_i = nullptr, *cand_n = nullptr;
    int nsplit = 0, cap = 0;
    const float *bound = nullptr;
    const float *Q = nullptr, *X = nullptr;
    int d = 0;
    int64_t nrows = 0, label_offset = 0;
    float xmax2 = 0.f, rxmax = 0.f;
    int metric = kL2, kout = 0;
    // scratch: flat_cand_rerank_parts(nsplit) partial lists of kout per flagged query, their overflow marks
    float *part_d = nullptr;
    long long *part_i = nullptr;
    int *ovf = nullptr;
    float *D = nullptr;
    int64_t *I = nullptr;
    int *nflag2 = nullptr, *flagged2 = nullptr;
    float *dbg = nullptr;         // HIPANN_FLAT_CAND_DEBUG: 4 floats per flagged query
    const float *qres = nullptr;  // the int8 image: the queries' residuals
};
void launch_flat_cand_rerank(const FlatCandRerankArgs &a, hipStream_t st);
int flat_cand_rerank_parts(int nsplit);
// launch_ivf_rerank's arguments: the scan's lists (pd / pi: nprobe slots of kslot entries per query, or slot_off's
// slots), the filter depth k, the rows and the outputs; then what only some callers set.
struct IvfRerankArgs {
    const float *pd = nullptr;
    const int *pi = nullptr, *slot_off = nullptr;
    int nprobe = 0;
    int64_t nq = 0;
    int k = 0, kout = 0, metric = kL2;
    const float *Q = nullptr, *codes = nullptr;
    int d = 0;
    const int64_t *ids = nullptr;
    int64_t nrows = 0, label_offset = 0;
    float xmax2 = 0.f;
    float *D = nullptr;
    int64_t *I = nullptr;
    int *nflag = nullptr, *flagged = nullptr;
    float eps = kSplit2Eps, rxmax = -1.f;
    const float *qres = nullptr;
    const int64_t *probes = nullptr, *list_off = nullptr;
    int nlist = 0;
    const unsigned *qbound = nullptr;
    const float *qnorm = nullptr;
    int kslot = 0, sub = 0;
    // fpd != nullptr: flagged IVF queries re-run inline, except the first fb_cap, left to launch_ivf_fallback_chunks
    const int *list_len = nullptr;
    float *fpd = nullptr;
    long long *fpi = nullptr;
    unsigned long long *fb_total = nullptr;
    int fb_cap = 0;
    int i8_l2 = 0;  // the int8 image's L2 certificate (qres = ‖q − q̂‖, lower-bound scan keys)
    // the seeded int8 scan: pd / pi hold every query's candidate run (common.hpp ivf_seed_run_slot), query q's of
    // kSeedK + seed_cnt[q] entries; slot_off only places the runs
    const int *seed_cnt = nullptr;
};
void launch_ivf_rerank(const IvfRerankArgs &a, hipStream_t st);
// the rerank's first fb_cap flagged queries re-run in parallel (one wave per (query, probe, chunk) item); cpd/cpi:
// fb_cap·nprobe·maxch·kout entries, done: fb_cap counters (zero on entry; left zero)
void launch_ivf_fallback_chunks(const int *nflag, const int *flagged, int fb_cap, int nprobe, int maxch, int chunk_rows,
                                int kout, int metric, const float *Q, const float *codes, int d, const int64_t *ids,
                                int64_t label_offset, const int64_t *probes, const int64_t *list_off,
                                const int *list_len, int nlist, float *cpd, long long *cpi, unsigned *done, float *D,
                                int64_t *I, unsigned long long *total, hipStream_t st,
                                unsigned long long *host_word = nullptr, unsigned host_seq = 0);
// ivf_mfma.hip, fp16-image scan (kFormHalfExact)
int ivf_mfma_h_group(int d);
void ivf_mh_stats_report();  // HIPANN_MH_STATS tuning builds: the fp16 / int8 scan epilogue's counters, to stderr
int ivf_scan_sublists();  // sub-lists per slot of the matrix-core scans in sub-list mode (one per wave)
int64_t ivf_half_pass_bytes(int d);
int64_t ivf_half_qsplit_bytes(int64_t nq, int d);
bool ivf_mfma_h_supported(int d, int k);
void launch_ivf_max_abs(const float *x, int64_t cnt, unsigned *out, hipStream_t st);
// (pass_ids != nullptr: only the listed global passes, one block each — the passes an append touched)
void launch_ivf_tile_half(const float *codes, const int64_t *list_off, const int *list_len, const int64_t *tpass_off,
                          int nlist, int64_t total_pass, int d, float scale, void *dst, hipStream_t st,
                          const int64_t *pass_ids = nullptr);
void launch_ivf_half_residual(const float *codes, int64_t n, int d, float scale, unsigned *out, hipStream_t st);
// The image scan's arguments (the batch's queries already prepared: launch_ivf_split_queries_h, or
// launch_ivf_split_queries_i8 with i8mode).
struct IvfImageScanArgs {
    // the prepared queries: image, 1/(t·s) or scales, residuals, the L2 key's query term; int8 L2: ‖q̂‖
    int64_t nq = 0;
    const void *qsplit = nullptr;
    const float *its = nullptr;
    float *qres = nullptr;
    const float *qn = nullptr, *qhn = nullptr;
    // the rows' image: fp16 or (i8mode) int8 with its per-row scales and, for L2, residuals
    const void *codes = nullptr;
    const int64_t *tpass_off = nullptr;
    const float *xn = nullptr, *xs8 = nullptr, *xr8 = nullptr;
    int i8mode = 0;
    int d = 0, metric = kL2, k = 0, sub = 0;
    unsigned *qbound = nullptr;
    // the seeded scan's two launches (ivf_scan_mfma_h): 1 = the chunk-0 items (plan.slot_off == nullptr: one slot per
    // pair), 2 = the others (plan.slot_off = the plan's slot prefixes; the waves append their rows to the queries'
    // candidate runs through cursor, one int per query, zeroed by launch_ivf_seed_bound); both read plan.goff
    int phase = 0;
    int *cursor = nullptr;
};
void launch_ivf_scan_mfma_h(const IvfImageScanArgs &a, const IvfPlanView &plan, int64_t max_items, float *pd, int *pi,
                            hipStream_t st);
// The seeded int8 scan's step between its two launches, one block per query: the kSeedK best of the query's nprobe·kslot
// chunk-0 entries (pa_d / pa_i, one kslot-entry slot per pair; pairs without rows skipped) into the tail of the query's
// first candidate slot (cd / ci), the kSeedK-th key min'ed into qbound[q] when all kSeedK are real; cursor[q] = 0, the
// query's count of entries appended after its seed list (the second launch adds to it).
bool ivf_seed_supported(int nprobe, int kslot);
void launch_ivf_seed_bound(const float *pa_d, const int *pa_i, const int *slot_off, int nprobe, int64_t nq, int kslot,
                           int64_t nrows, unsigned *qbound, float *cd, int *ci, int *cursor, hipStream_t st);
// int8 image (kFormI8Exact): packed group (wide items only), pass / query-image bytes, support, the tiling (one scale
// and one residual per row into xs8 / xr8; *nonfin != 0 afterwards: a non-finite row), the batch's int8 queries (units,
// scales, residuals, ‖q̂‖² and ‖q̂‖ of the dequantised queries)
int ivf_mfma_i8_group(int d);
int64_t ivf_i8_pass_bytes(int d);
int64_t ivf_i8_qimg_bytes(int64_t nq, int d);
bool ivf_mfma_i8_supported(int d, int k);
void launch_ivf_tile_i8(const float *codes, const int64_t *list_off, const int *list_len, const int64_t *tpass_off,
                        int nlist, int64_t total_pass, int d, void *dst, float *xs8, float *xr8, unsigned *nonfin,
                        hipStream_t st, const int64_t *pass_ids = nullptr);
void launch_ivf_split_queries_i8(const float *Q, int64_t nq, int d, void *qi8, float *qs8, float *qres8,
                                 float *qhn2, float *qhn, hipStream_t st);
// the batch's fp16 query terms (+ 1/(t·s), split residuals) and, when qn != nullptr, ‖q‖² (row_norms_f32's bits)
void launch_ivf_split_queries_h(const float *Q, int64_t nq, int d, int es, void *qsplit, float *its, float *qres,
                                float *qn, hipStream_t st);
// flat_bf16.hip
int flat_bf16_waves(int64_t nq);
int flat_bf16_tile_rows();
int flat_bf16_topk_kmax(int64_t nq);
int flat_gemm_topk_bf_kmax(int np);
size_t flat_bf16_img_bytes(int64_t n, int d, int R);
void launch_b16_tile_rows(const float *X, int64_t n, int d, int R, void *out, hipStream_t st);
void launch_b16_row_residual2(const float *X, int64_t n, int d, float *out, hipStream_t st);
void launch_flat_bf16_topk(const float *Q, const float *qn, int64_t nq, void *qimg, const void *ximg, const float *xn,
                           int64_t N, int d, int metric, int k, int nsplit, int64_t tiles_per_split, float *pd, int *pi,
                           const float *seed, bool image_ready, hipStream_t st);
// bounded passes of the 64-dim K-step kernel (flat_b16k64.hip): candidate buffers, their bound and select
// (k64_on: the caller's HIPANN_B16_K64 switch)
bool flat_bf16_resumable(int64_t nq, int d, int k, bool k64_on);
// One launch of flat_bf16_k64: nqt query tiles × nsplit column splits, each block over tiles [tile_begin, tile_end) of
// its split's tiles_per_split.  A pass appends the rows with key ≤ bound[q] to the (query, split) cells of cand_d /
// cand_i (cap entries each, counts in cand_n; resume: the counts continue).  keys: cand_d is the dense nq × N key
// matrix instead, and bound / cand_i / cand_n / cap stay unset.  qscale and xscale: the int8 images' scales (both or
// neither).
struct FlatK64Args {
    const void *qimg = nullptr;  // the queries: image, ‖q‖² (L2), count
    const float *qn = nullptr;
    int64_t nq = 0;
    const void *ximg = nullptr;  // the rows: image, ‖x‖² (L2), count
    const float *xn = nullptr;
    int64_t N = 0;
    int nk = 0, metric = kL2;    // chunks per row of the images
    int nqt = 0, nsplit = 1;
    int64_t tiles_per_split = 0, tile_begin = 0, tile_end = 0;
    const float *bound = nullptr;
    float *cand_d = nullptr;
    int *cand_i = nullptr, *cand_n = nullptr;
    int cap = 0;
    bool resume = false, keys = false;
    const float *qscale = nullptr, *xscale = nullptr;
};
void launch_flat_bf16_k64(const FlatK64Args &a, hipStream_t st);
// form kFlatI8Exact (flat_b16k64.hip): per-row int8 scale s = max|x|/127 and residual ‖x − s·x̂‖ (×1.0001) per row;
// the tiled int8 image (64 dims per 64-B chunk row, chunk count rounded up to even, zero-filled); its bytes
int flat_i8_nk(int d);
size_t flat_i8_img_bytes(int64_t n, int d, int R);
void launch_i8_row_scale(const float *X, int64_t n, int d, float *scale, float *resid, hipStream_t st);
void launch_i8_tile_rows(const float *X, const float *scale, int64_t n, int d, int R, void *out, hipStream_t st);
// ‖q‖² (qn optional), the int8 scales / residuals and the tiled int8 image of a query batch in one launch
void launch_i8_query_prep(const float *X, int64_t n, int d, float *qn, float *scale, float *resid, int R, void *out,
                          hipStream_t st);
int flat_i8_scan_k();
int flat_i8_scan_max_nq();
int64_t flat_i8_scan_waves(int64_t n);
void launch_flat_i8_scan(const float *Q, int64_t nq, int d, int metric, const void *ximg, const float *xscale,
                         const float *xnorm, int64_t n, float *qscale, float *qres, const float *qnorm, void *qimg,
                         float *part_d, int *part_i, int64_t nw, hipStream_t st);
void launch_flat_i8_group_merge(const float *pd, const int *pi, int nw, int nq, int ngroup, float *od, int *oi,
                                hipStream_t st);
int flat_keys_kth_max();
void launch_flat_keys_kth(const float *keys, int S, int64_t nq, int k, float *bound, hipStream_t st);
void launch_flat_cand_bound(const float *cand_d, const int *cand_n, int nsplit, int cap, int64_t nq, int k,
                            float *bound, hipStream_t st);
void launch_flat_cand_select(const float *cand_d, const int *cand_i, const int *cand_n, int nsplit, int cap, int64_t nq,
                             int k, float *out_d, int *out_i, int *nflag, int *flagged, hipStream_t st);
void launch_flat_bf16_seed(const float *pd, int nsplit, int64_t nq, int k, float *seed, hipStream_t st);
bool flat_bf16_k64_supported(int nk, int k);
void launch_ivf_max_norm(const float *xn, int64_t n, unsigned *out, hipStream_t st);
void launch_ivf_gather_queries(const float *Q, const int *idx, int nf, int d, float *out, hipStream_t st);
// hipann_ivf_add: an append block's rows into their CSR rows + the new live lengths + the new rows' maxima
// (stat[0] max ‖x‖², stat[1] max |x| bits, stat[2] max fp16 residual² at hscale; hscale 0: no residual)
void launch_ivf_append_rows(const float *rows, const float *norms, const int64_t *dst, const int64_t *ids_in, int64_t n,
                            int d, float *codes, int64_t *ids, float *xnorm, const int *newlen, int *list_len, int nlist,
                            float hscale, unsigned *stat, hipStream_t st);
// remove_kernels.hip — hipann_flat_remove_ids: the plan over rows [first, first + cnt) of a shard (keep mask from the
// sorted unique removed rows, exclusive prefix sum, src[j] = range-relative source of the j-th survivor; keep: cnt
// bytes, sums: flat_remove_scan_blocks(cnt) int64, src: cnt − m int64) and the gathers into fresh buffers
int64_t flat_remove_scan_blocks(int64_t cnt);
void launch_flat_remove_plan(const int64_t *rows, int64_t m, int64_t first, int64_t cnt, unsigned char *keep,
                             int64_t *sums, int64_t *src, hipStream_t st);
void launch_flat_gather_rows(const float *X, const int64_t *idx, int64_t cnt, int d, float *out, hipStream_t st);
void launch_flat_gather_f32(const float *v, const int64_t *idx, int64_t cnt, float *out, hipStream_t st);
// hipann_ivf_remove_ids: every live row whose id is in labels (device, sorted unique) leaves its list in FAISS's
// order (one block per list: mark, closed-form plan, move, zero the vacated rows, new length); mark: one byte, plan:
// one int per physical row; pass_ids / npass (optional, npass zeroed by the caller): the tiled passes to re-tile
void launch_ivf_remove_rows(const int64_t *labels, int64_t m, const int64_t *list_off, int *list_len, int nlist, int d,
                            float *codes, int64_t *ids, float *xnorm, unsigned char *mark, int *plan,
                            const int64_t *tpass_off, int64_t *pass_ids, unsigned long long *npass, int *newlen,
                            hipStream_t st);
void launch_ivf_scatter_results(const float *Df, const int64_t *If, const int *idx, int nf, int kout, float *D,
                                int64_t *I, hipStream_t st);
void launch_ivf_scan_mfma_bf(int np, const float *Q, int64_t nq, void *qsplit, const float *qn, int d, int metric,
                             const float *codes_t, const int64_t *tpass_off, const float *xn, const IvfPlanView &plan,
                             int k, int64_t max_items, unsigned *qbound, float *pd, int *pi, hipStream_t st, int sub = 0);
int ivf_group_size(int form, int d);  // queries per work item of the form's scan kernel
int ivf_chunk_rows();
void launch_ivf_scan_bigk(const float *Q, int d, int metric, const float *codes, const IvfPlanView &plan,
                          const int64_t *probes, int64_t npairs, int64_t nslots, int k, float *pd, int *pi, hipStream_t st);
size_t ivf_scan_smem_bytes();
// (aligned16: the queries and the codes both start on 16 bytes)
bool ivf_dot_supported(int d, bool aligned16);
bool ivf_dot_supported(const float *Q, int d, const float *codes);
void launch_ivf_scan(const float *Q, const float *qn, int d, int metric, int form, const float *codes, const float *xn,
                     const IvfPlanView &plan, int64_t nq, int k, int64_t max_items, unsigned *qbound, float *pd, int *pi,
                     hipStream_t st);
bool ivf_mfma_supported(int d, bool aligned16, int k);
bool ivf_mfma_supported(const float *Q, int d, const float *codes, int k);
int ivf_mfma_group(int d);
int64_t ivf_mfma_pass_floats(int d);  // floats per 32-row pass of the tiled codes
void launch_ivf_tile_codes(const float *codes, const int64_t *list_off, const int *list_len, const int64_t *tpass_off,
                           int nlist, int64_t total_pass, int d, float *dst, hipStream_t st,
                           const int64_t *pass_ids = nullptr);
void launch_ivf_scan_mfma(const float *Q, const float *qn, int d, int metric, const float *codes_t,
                          const int64_t *tpass_off, const float *xn, const IvfPlanView &plan, int k, int64_t max_items,
                          unsigned *qbound, float *pd, int *pi, hipStream_t st, int sub = 0);
void launch_ivf_merge(const float *pd, const int *pi, const int64_t *ids, int64_t nrows, const int *slot_off, int nprobe, int64_t nq,
                      int k, int kout, float out_sign, float *D, int64_t *I, hipStream_t st);
template <typename InId>
void launch_merge_parts(const float *pd, const InId *pi, int nparts, int64_t nq, int k, int kout,
                        int64_t label_offset, float in_sign, float out_sign, float *D, int64_t *I, hipStream_t st,
                        int64_t pstride_d = -1, int64_t pstride_i = -1);  // part strides (elements); -1: nq*k
// Many parts, few queries: groups of parts merged by ngroups·nq waves into md/mi ([g][nq][kout]), then the
// group lists by launch_merge_parts (kout <= 64).
template <typename InId>
void launch_merge_parts_2level(const float *pd, const InId *pi, int nparts, int64_t nq, int k, int kout,
                               int64_t label_offset, float in_sign, float out_sign, float *D, int64_t *I, float *md,
                               long long *mi, int ngroups, hipStream_t st);

}  // namespace hipann
