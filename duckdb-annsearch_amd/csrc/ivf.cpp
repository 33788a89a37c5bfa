// ivf.cpp — IVFFlat part of the C ABI (include/hip_ann.h).
//
// Mirrors index_cpu_to_metal_ivf (faiss-metal/src/MetalIndexIVFFlat.mm:283-326: centroids, per-list
// ids and raw fp32 codes copied out of a FAISS IndexIVFFlat; nprobe taken from the CPU index) and
// MetalIndexIVFFlat::search (:122-256: k <= 0 throws, empty → (±inf, −1) pads, ids remapped to the
// stored labels).  The parity target is FAISS CPU IndexIVFFlat::search: coarse search
// with nprobe = min(nprobe, nlist), lists scanned with direct distances.
#include "../../include/hip_ann.h"
#include "ivf.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <numeric>

using namespace hipann;

namespace {

void set_err(char *buf, int len, const char *msg) {
    if (!buf || len <= 0) return;
    std::strncpy(buf, msg, (size_t)len - 1);
    buf[len - 1] = '\0';
}

template <typename F>
int guard_int(char *eb, int el, F &&f) {
    try {
        return f();
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return -1;
}

template <typename F>
void *guard_ptr(char *eb, int el, F &&f) {
    try {
        return f();
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return nullptr;
}

hipStream_t make_stream(int dev) {
    DeviceGuard g(dev);
    hipStream_t s;
    HIPANN_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return s;
}

// The search-time coarse step's key GEMM on the bf16 matrix cores (flat_keys_bf3: three-term split, fp32-level
// keys).  List assignment (add / append) keeps fp32.
struct CoarseKeysScope {
    FlatShard &s;
    explicit CoarseKeysScope(FlatShard &x) : s(x) { s.keys_bf3 = true; }
    ~CoarseKeysScope() { s.keys_bf3 = false; }
};

// Borrowed-centroid coarse quantizer on the shard's device.
std::unique_ptr<FlatIndex> make_quantizer(int d, int metric, const float *cen, int nlist, int device,
                                          hipStream_t stream) {
    auto q = std::make_unique<FlatIndex>();
    q->form = kFlatFp32;  // coarse assignment stays on exact fp32 products
    q->d = d;
    q->metric = metric;
    auto sh = std::make_unique<FlatShard>();
    sh->device = device;
    sh->stream = nullptr;  // searches run on the IVF shard's stream
    sh->xb = const_cast<float *>(cen);
    sh->owns = false;
    sh->n = nlist;
    sh->cap = nlist;
    if (metric == kL2) {
        DeviceGuard g(device);
        sh->xn.ensure((size_t)nlist * sizeof(float), device);
        launch_row_norms(cen, nlist, d, sh->xn.get<float>(), stream);
        HIPANN_CHECK(hipStreamSynchronize(stream));
    }
    q->shards.push_back(std::move(sh));
    return q;
}

// off: physical list starts (nlist + 1; list l owns rows [off[l], off[l+1])), len: live rows per list (≤ capacity).
void upload_list_meta(IvfShard &sh, const std::vector<int64_t> &off, const std::vector<int64_t> &len, int nlist) {
    DeviceGuard g(sh.device);
    std::vector<int> hl(nlist);
    int64_t maxlen = 0, live = 0;
    for (int l = 0; l < nlist; ++l) {
        HIPANN_REQUIRE(len[l] >= 0 && len[l] <= off[l + 1] - off[l], "list length exceeds its capacity");
        HIPANN_REQUIRE(len[l] < (int64_t)0x7fffffff, "inverted list longer than 2^31-1 rows");
        hl[l] = (int)len[l];
        maxlen = std::max<int64_t>(maxlen, len[l]);
        live += len[l];
    }
    sh.max_nch = (int)std::max<int64_t>(1, ceil_div(maxlen, ivf_chunk_rows()));
    sh.h_off = off;
    sh.h_len = len;
    sh.n = off[nlist];
    sh.live = live;
    sh.list_off.ensure(sizeof(int64_t) * (nlist + 1), sh.device);
    sh.list_len.ensure(sizeof(int) * nlist, sh.device);
    HIPANN_CHECK(hipMemcpyAsync(sh.list_off.p, off.data(), sizeof(int64_t) * (nlist + 1), hipMemcpyHostToDevice,
                                sh.stream));
    HIPANN_CHECK(hipMemcpyAsync(sh.list_len.p, hl.data(), sizeof(int) * nlist, hipMemcpyHostToDevice, sh.stream));
    HIPANN_CHECK(hipStreamSynchronize(sh.stream));
}

std::vector<int64_t> dense_lengths(const std::vector<int64_t> &off, int nlist) {
    std::vector<int64_t> len(nlist);
    for (int l = 0; l < nlist; ++l) len[l] = off[l + 1] - off[l];
    return len;
}

// 32-row pass offsets of every list (the tiled copies' layout); returns the total pass count.
int64_t ensure_tpass(IvfShard &sh, int nlist, hipStream_t st) {
    std::vector<int64_t> tp(nlist + 1, 0);
    for (int l = 0; l < nlist; ++l) tp[l + 1] = tp[l] + ceil_div(sh.h_off[l + 1] - sh.h_off[l], 32);
    if (!sh.tpass_off.p) {
        sh.tpass_off.ensure(sizeof(int64_t) * (nlist + 1), sh.device);
        HIPANN_CHECK(hipMemcpyAsync(sh.tpass_off.p, tp.data(), sizeof(int64_t) * (nlist + 1), hipMemcpyHostToDevice, st));
        HIPANN_CHECK(hipStreamSynchronize(st));  // tp (host) is released on return
    }
    return tp[nlist];
}

// The MFMA scan's tiled copy of the codes (built once, at the first search that uses it).
void ensure_tiled_codes(IvfShard &sh, int d, int nlist, hipStream_t st) {
    if (sh.codes_t.p || sh.n == 0) return;
    const int64_t np = ensure_tpass(sh, nlist, st);
    const int64_t pf = ivf_mfma_pass_floats(d);
    sh.codes_t.ensure(sizeof(float) * (size_t)std::max<int64_t>(np, 1) * pf, sh.device);
    launch_ivf_tile_codes(sh.codes, sh.list_off.get<int64_t>(), sh.list_len.get<int>(), sh.tpass_off.get<int64_t>(), nlist,
                          np, d, sh.codes_t.get<float>(), st);
    HIPANN_CHECK(hipStreamSynchronize(st));
}

// kFormHalfExact: the tiled fp16 image of x·s, s = 2^half_es with max|x| = f·2^e, f ∈ [½, 1), half_es =
// 14 − e (every scaled element < 2^14), and the largest row residual ‖x − x̂/s‖ (built once).  Codes
// with a non-finite entry or a scale outside 2^±100 leave the form unsupported (the search then takes
// kFormSplit2Exact).  Returns whether the image is usable.
bool ensure_half_codes(IvfShard &sh, int d, int nlist, hipStream_t st) {
    if (sh.half_state != 0) return sh.half_state > 0;
    if (sh.n == 0) return false;  // nothing to scan (and nothing to measure); retried after an add
    sh.nflag.ensure(sizeof(int), sh.device);
    unsigned bits = 0;
    launch_ivf_max_abs(sh.codes, sh.n * (int64_t)d, sh.nflag.get<unsigned>(), st);
    HIPANN_CHECK(hipMemcpyAsync(&bits, sh.nflag.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));
    float mx;
    std::memcpy(&mx, &bits, sizeof(mx));
    int e = 0;
    if (bits != 0 && bits < 0x7f800000u) (void)std::frexp(mx, &e);
    if (bits >= 0x7f800000u || e < -100 || e > 100) {
        sh.half_state = -1;
        return false;
    }
    sh.half_es = 14 - e;
    const float scale = std::ldexp(1.f, sh.half_es);
    const int64_t np = ensure_tpass(sh, nlist, st);
    sh.codes_h.ensure((size_t)std::max<int64_t>(np, 1) * (size_t)ivf_half_pass_bytes(d), sh.device);
    launch_ivf_tile_half(sh.codes, sh.list_off.get<int64_t>(), sh.list_len.get<int>(), sh.tpass_off.get<int64_t>(), nlist,
                         np, d, scale, sh.codes_h.p, st);
    launch_ivf_half_residual(sh.codes, sh.n, d, scale, sh.nflag.get<unsigned>(), st);
    HIPANN_CHECK(hipMemcpyAsync(&bits, sh.nflag.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));
    float r2;
    std::memcpy(&r2, &bits, sizeof(r2));
    sh.half_rxmax = std::sqrt(r2) * 1.0001f;  // fp32 sum of d exact squares: relative error ≪ 1e-4
    sh.half_state = 1;
    return true;
}

void release_i8_codes(IvfShard &sh, int state) {
    sh.i8_state = state;
    sh.i8_rxmax = -1.f;
    sh.codes_i8.release();
    sh.xs8.release();
    sh.xr8.release();
}

// kFormI8Exact: the tiled int8 image with one scale and one residual per row (ivf_mfma.hip), built at the first search
// that needs it and kept across adds and removes (they re-tile the passes they touch: no whole-table statistic
// belongs to the L2 certificate).  A non-finite row: the form does not apply (kFormSplit2Exact runs), as the fp16 image.
bool ensure_i8_codes(IvfShard &sh, int d, int nlist, hipStream_t st) {
    if (sh.i8_state != 0) return sh.i8_state > 0;
    if (sh.n == 0) return false;
    const int64_t np = ensure_tpass(sh, nlist, st);
    sh.codes_i8.ensure((size_t)std::max<int64_t>(np, 1) * (size_t)ivf_i8_pass_bytes(d), sh.device);
    sh.xs8.ensure(sizeof(float) * (size_t)sh.n, sh.device);
    sh.xr8.ensure(sizeof(float) * (size_t)sh.n, sh.device);
    // rows no pass covers (none today: a list's passes span its capacity) read as scale 0, residual 0
    HIPANN_CHECK(hipMemsetAsync(sh.xs8.p, 0, sh.xs8.bytes, st));
    HIPANN_CHECK(hipMemsetAsync(sh.xr8.p, 0, sh.xr8.bytes, st));
    sh.nflag.ensure(sizeof(int), sh.device);
    launch_ivf_tile_i8(sh.codes, sh.list_off.get<int64_t>(), sh.list_len.get<int>(), sh.tpass_off.get<int64_t>(), nlist, np,
                       d, sh.codes_i8.p, sh.xs8.get<float>(), sh.xr8.get<float>(), sh.nflag.get<unsigned>(), st);
    sh.i8_tiled += np;
    unsigned nonfin = 0;
    HIPANN_CHECK(hipMemcpyAsync(&nonfin, sh.nflag.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));
    if (nonfin) {
        release_i8_codes(sh, -1);
        return false;
    }
    sh.i8_rxmax = -1.f;
    sh.i8_state = 1;
    return true;
}

// the IP bound's largest row residual of the int8 image: the maximum of the residual plane (its slack rows are 0),
// taken again after an add (removes leave it: a maximum over a superset of the rows is still an upper bound)
float shard_i8_rxmax(IvfShard &sh, hipStream_t st) {
    if (sh.i8_rxmax >= 0.f) return sh.i8_rxmax;
    sh.nflag.ensure(sizeof(int), sh.device);
    launch_ivf_max_abs(sh.xr8.get<float>(), sh.n, sh.nflag.get<unsigned>(), st);
    unsigned bits = 0;
    HIPANN_CHECK(hipMemcpyAsync(&bits, sh.nflag.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));
    // (the plane's entries already carry the ×1.0001 of their fp32 sums); a NaN entry (magnitude bits above +inf's)
    // reads as +inf: the rerank's `rxmax >= 0` must pick the Cauchy-Schwarz bound, whose non-finite E flags the query
    if (bits > 0x7f800000u) bits = 0x7f800000u;
    std::memcpy(&sh.i8_rxmax, &bits, sizeof(float));
    return sh.i8_rxmax;
}

// ‖x‖² of every stored row (L2 only): the decomposed scan form reads it with the codes
// (faiss-metal stores the same norms with its lists, MetalIndexIVFFlat.mm:313-318).
void compute_row_norms(IvfShard &sh, int d, int metric) {
    if (metric != kL2 || sh.n == 0) return;
    DeviceGuard g(sh.device);
    sh.xnorm.ensure(sizeof(float) * (size_t)sh.n, sh.device);
    launch_row_norms(sh.codes, sh.n, d, sh.xnorm.get<float>(), sh.stream);
    HIPANN_CHECK(hipStreamSynchronize(sh.stream));
}

}  // namespace

namespace hipann {

IvfIndex::~IvfIndex() {
    if (!shards.empty()) {
        DeviceGuard g(shards[0]->device);
        ivf_mh_stats_report();
    }
    for (auto &s : shards) {
        s->quant.reset();
        DeviceGuard g(s->device);
        if (s->done) (void)hipEventDestroy(s->done);
        for (hipEvent_t e : s->app_ev)
            if (e) (void)hipEventDestroy(e);
        if (s->app_sync) (void)hipEventDestroy(s->app_sync);
        if (s->stream) (void)hipStreamDestroy(s->stream);
    }
}

// HIPANN_IVF_HOST_FALLBACK=1: the flagged queries of the exact forms are re-run from the host on the 3-term
// path after a readback of the flag count (the r01/r02 scheme; A/B only).  Default: on the device.
static bool host_fallback() {
    static const bool v = [] { const char *e = std::getenv("HIPANN_IVF_HOST_FALLBACK"); return e && std::atoi(e) != 0; }();
    return v;
}

// max‖x‖² of the shard (once): the rerank's error bound
static float shard_xmax2(IvfShard &sh, int d, hipStream_t st) {
    if (sh.xmax2 >= 0.f) return sh.xmax2;
    const float *xn = sh.xnorm.get<float>();
    if (!xn) {
        sh.tmpnorm.ensure(sizeof(float) * (size_t)std::max<int64_t>(sh.n, 1), sh.device);
        launch_row_norms(sh.codes, sh.n, d, sh.tmpnorm.get<float>(), st);
        xn = sh.tmpnorm.get<float>();
    }
    sh.nflag.ensure(sizeof(int), sh.device);
    launch_ivf_max_norm(xn, sh.n, sh.nflag.get<unsigned>(), st);
    unsigned bits = 0;
    HIPANN_CHECK(hipMemcpyAsync(&bits, sh.nflag.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));
    sh.tmpnorm.release();
    float v;
    std::memcpy(&v, &bits, sizeof(v));
    sh.xmax2 = v;
    return v;
}

// ---- the exact fp16 form's filter image (hipann_ivf_set_filter_image) ----
// Batches below this many queries keep the fp16 image under auto.  Measured on the 10M x 768 index (nlist 1024,
// nprobe 32, profiles/ivf_i8_auto/): nq 64 / 128 / 256 / 1024 run 2.11 / 2.41 / 2.46 / 2.55 ms on the fp16 image and
// 1.24 / 1.40 / 1.45 / 2.11 ms on the int8 image, run-to-run spread below 0.04 ms — the int8 image wins at every
// measured size; smaller batches (the extension's nq = 1 call is latency-bound, not byte-bound) are left as they were.
constexpr int64_t kAutoI8MinBatch = 64;

// the setting, or the one environment override HIPANN_IVF_FILTER_IMAGE = 0 / 1 / 2 (A/B)
static int filter_image_mode(const IvfIndex &ix) {
    static const int env = [] { const char *e = std::getenv("HIPANN_IVF_FILTER_IMAGE"); return e && *e ? std::atoi(e) : -1; }();
    return env >= 0 && env <= 2 ? env : ix.filter_image;
}

// The byte rule of the auto choice.  A flagged query is re-run in the direct form over its nprobe lists of fp32 rows:
// flagged · nprobe · mean_list_rows · 4d bytes, mean_list_rows = live / nlist.  Against the fp16 image (2d + 4 B per
// row) the int8 image (d + 8 B) saves about d bytes per row, n · d over the table a large batch streams once.  The
// int8 image stays only while the re-runs cost less than a quarter of that saving:
//     flagged · nprobe · mean_list_rows · 4d < 0.25 · n · d   ⇔   flagged < nlist / (16 · nprobe)
// — fewer than 2 of 1024 queries at nlist 1024, nprobe 32.
static bool auto8_over_rule(int64_t flagged, int nprobe, int nlist, int64_t live, int d) {
    const double mean_list_rows = (double)live / (double)nlist;
    return (double)flagged * nprobe * mean_list_rows * 4.0 * d >= 0.25 * (double)live * d;
}

static unsigned long long *auto8_host_word(IvfShard &sh) {
    if (sh.fb_host.ensure(sizeof(uint64_t))) {
        *sh.fb_host.get<uint64_t>() = 0;
        sh.fb_seen = 0;
    }
    return static_cast<unsigned long long *>(host_device_ptr(sh.fb_host.p));
}

namespace {

// ---- the scan mode: what a batch's requested form resolves to ("Scan modes", has the table) ----
// Everything ivf_resolve_mode reads; no pointer, no shard, no environment.
struct IvfModeIn {
    int form = kFormHalfExact;  // the requested form (IvfForm)
    bool is_override = false;   // ... from the caller's options (a re-run), not the index
    int metric = kL2, d = 0, k = 0, kout = 0;
    int np = 0;                 // min(nprobe, nlist)
    int max_nch = 1;
    bool aligned16 = true;      // the queries and the codes both start on 16 bytes
    bool host_fb = false;       // HIPANN_IVF_HOST_FALLBACK
    bool seed_on = true;        // HIPANN_IVF_SEED / the test hook's override
    bool use_int8 = false;      // the fp16 form filters through the int8 image (ivf_choose_filter_image)
};

struct IvfScanMode {
    int form = kFormDirect;       // the scan that runs (an image scan: kFormSplit2)
    int last_form = kFormDirect;  // what hipann_last_search_path reports
    bool exact = false;           // 16-deep filter + exact rerank
    int image = 0;                // 0 none, 1 fp16, 2 int8
    bool as_half = false;         // image 2 standing in for the fp16 form's image
    bool sub = false;             // every wave's list a sub-list of the slot
    int kscan = 0;                // per-list k of the scan (the output keeps kout)
    int kslot = 0, kfilt = 0;     // entries per (query, probe, chunk) slot; the rerank's filter depth
    bool seeded = false, tiled = false, cert8 = false, bigk = false;
    int group = 0;                // queries per work item (packed for the image scans)
};

// The filter-image choice applies to: the index's own fp16 form, L2 (the per-row certificate), kout <= kRerankMaxK
// without a sub-list request, a shape the int8 scan holds, the device fallback, and a shard whose int8 image exists or
// can still be built.
bool ivf_filter_image_eligible(const IvfModeIn &in, int64_t nrows, int i8_state) {
    return !in.is_override && in.form == kFormHalfExact && in.metric == kL2 && in.kout <= kRerankMaxK && in.k <= 64 &&
           !in.host_fb && ivf_mfma_i8_supported(in.d, kRerankK) && nrows > 0 && i8_state >= 0;
}

// ensure(image) builds (or finds) the tiled image 1 = fp16 / 2 = int8 and says whether it is usable; it is asked only
// once every other condition for that image holds, and a refusal (a non-finite row) falls through to the next form.
template <typename Ensure>
IvfScanMode ivf_resolve_mode(const IvfModeIn &in, Ensure &&ensure) {
    IvfScanMode m;
    const int d = in.d, kout = in.kout;
    int req = in.form;
    m.bigk = in.k > 64;  // per-slot direct scan + LDS sort (ivf_scan_slot_bigk), same plan / merge
    m.as_half = in.use_int8 && ensure(2);
    if (m.as_half) req = kFormI8Exact;
    const bool sub_req = (((req == kFormHalfExact || req == kFormSplit2Exact) && kout > kRerankMaxK) ||
                          req == kFormI8Exact) && kout <= kIvfSubMaxK && !m.bigk;
    if (req == kFormHalfExact) {
        if ((kout <= kRerankMaxK || sub_req) && !m.bigk && ivf_mfma_h_supported(d, kRerankK) && ensure(1)) m.image = 1;
        req = kFormSplit2Exact;
    } else if (req == kFormI8Exact) {
        if (sub_req && ivf_mfma_i8_supported(d, kRerankK) && ensure(2)) m.image = 2;
        req = kFormSplit2Exact;
    }
    const bool want_exact = req == kFormSplit2Exact;
    if (want_exact) req = kout <= kRerankMaxK || sub_req ? kFormSplit2 : kFormSplit3;
    m.kscan = want_exact && req == kFormSplit2 ? kRerankK : in.k;
    m.form = req != kFormDirect && !m.bigk && ivf_dot_supported(d, in.aligned16) ? req : kFormDirect;
    if (m.image) m.form = kFormSplit2;  // any d: the images are zero-padded to whole super-steps
    if (!m.image && ivf_form_split(m.form) && !ivf_mfma_bf_supported(d, in.aligned16, m.kscan, ivf_form_terms(m.form)))
        m.form = kFormDecomposed;
    if (m.form == kFormDecomposed && !ivf_mfma_supported(d, in.aligned16, m.kscan)) m.form = kFormDecomposedValu;
    m.exact = want_exact && m.form == kFormSplit2;
    m.sub = m.exact && sub_req;
    m.kslot = m.sub ? ivf_scan_sublists() * m.kscan : m.kscan;
    m.kfilt = m.sub ? (m.image == 2 ? 64 : std::min(64, std::max(kout + 4, 2 * kout))) : m.kscan;
    m.last_form = !m.exact ? m.form
                  : m.image == 2 ? (m.as_half ? kFormHalfExact : kFormI8Exact)
                  : m.image == 1 ? kFormHalfExact : kFormSplit2Exact;
    m.cert8 = m.image == 2 && in.metric == kL2;
    m.seeded = in.seed_on && m.cert8 && m.sub && in.max_nch > 1 && ivf_seed_supported(in.np, m.kslot);
    m.tiled = m.form == kFormDecomposed || ivf_form_split(m.form);  // the matrix-core scans
    m.group = m.image == 2 ? ivf_mfma_i8_group(d) : m.image == 1 ? ivf_mfma_h_group(d) : ivf_group_size(m.form, d);
    return m;
}

// The fp16 form's filter image for this batch (hipann_ivf_set_filter_image): mode 1 always takes the int8 image; auto
// (2) from kAutoI8MinBatch queries on, per shard: untested -> probation (the batch is answered through the fp16 image
// and judged afterwards), on -> off after two consecutive batches over the byte rule, read from fb_host (the previous
// int8 batch's flag count: no host synchronisation), and probation again once the shard has grown by a quarter.
struct IvfImageChoice {
    bool use_int8, probation;
};
IvfImageChoice ivf_choose_filter_image(IvfShard &sh, bool eligible, int mode, int64_t nq, int np, int nlist, int d) {
    if (!eligible || mode == 0 || (mode == 2 && nq < kAutoI8MinBatch)) return {false, false};
    if (mode == 1) return {true, false};
    if (sh.auto8 == 1 && sh.fb_host.p) {
        const uint64_t w = __atomic_load_n(sh.fb_host.get<uint64_t>(), __ATOMIC_RELAXED);
        if (w != sh.fb_seen) {  // a batch not yet judged
            sh.fb_seen = w;
            sh.auto8_over = auto8_over_rule((int64_t)(w & 0xffffffffu), np, nlist, sh.live, d) ? sh.auto8_over + 1 : 0;
            if (sh.auto8_over >= 2) sh.auto8 = -1;
        }
    }
    if (sh.auto8 != 0 && sh.live >= sh.auto8_live + sh.auto8_live / 4 + 1) sh.auto8 = 0;
    return {sh.auto8 == 1, sh.auto8 == 0};
}

// ---- one batch on one shard: the stages of ivf_shard_search, in their order on the stream ----
struct IvfBatch {
    IvfIndex &ix;
    IvfShard &sh;
    const int64_t nq;
    const float *const xq;
    const int k_user, kout;
    float *const D;
    int64_t *const I;
    const hipStream_t st;
    const IvfSearchOpts &opts;
    const int np;  // min(nprobe, nlist)
    IvfScanMode m;
    bool probation = false;
    FlatShard &qsh;  // the coarse quantizer's shard (its qn holds ‖q‖² of the batch when the preparation wrote it)
    // this batch's and the next one's plan counts / fill cursors (double-buffered by batch parity)
    int *ccnt_cur = nullptr, *ccnt_next = nullptr, *cur_cur = nullptr, *cur_next = nullptr;
    float xmax2 = 0.f, rxmax8 = -1.f;
    unsigned *qbound = nullptr;
    const float *qn = nullptr;
    float *cand_d = nullptr;  // the seeded scan: the queries' candidate runs (inside part_d / part_i)
    int *cand_i = nullptr;
    IvfPlanView plan() const {
        return {sh.list_off.get<int64_t>(), sh.list_len.get<int>(), sh.cnt.get<int>(), sh.bucket_off.get<int>(),
                sh.item_off.get<int>(), sh.bucket.get<int>(), sh.slot_off.get<int>(), sh.goff.get<int>(), ix.nlist, np};
    }
};

// The coarse step's outputs and the plan's per-list counts and fill cursors, double-buffered by batch parity
// (ivf_planfill_q zeroes the other parity's pair for the next batch; ivf_plan_q zeroes its own after use) — zeroed
// once per list count.
void ivf_plan_scratch(IvfBatch &b) {
    IvfShard &sh = b.sh;
    const int nlist = b.ix.nlist;
    sh.coarse_d.ensure((size_t)b.nq * b.np * sizeof(float), sh.device);
    sh.coarse_i.ensure((size_t)b.nq * b.np * sizeof(int64_t), sh.device);
    HIPANN_REQUIRE((int64_t)b.nq * b.np < (int64_t)0x7fffffff, "nq * nprobe too large");
    sh.slot_off.ensure(sizeof(int) * ((size_t)b.nq * b.np + 1), sh.device);
    if (!sh.ccnt.p || !sh.cursor2.p || sh.plan_nlist != nlist) {
        sh.ccnt.ensure(sizeof(int) * 2 * kPlanCopies * (size_t)nlist, sh.device);
        sh.cursor2.ensure(sizeof(int) * 2 * kPlanCopies * (size_t)nlist, sh.device);
        HIPANN_CHECK(hipMemsetAsync(sh.ccnt.p, 0, sizeof(int) * 2 * kPlanCopies * (size_t)nlist, b.st));
        HIPANN_CHECK(hipMemsetAsync(sh.cursor2.p, 0, sizeof(int) * 2 * kPlanCopies * (size_t)nlist, b.st));
        sh.plan_nlist = nlist;
        sh.plan_batch = 0;
    }
    const int par = (int)(sh.plan_batch & 1u);
    const size_t pstride = (size_t)kPlanCopies * nlist;  // one parity's [copy][list] counts / cursors
    b.ccnt_cur = sh.ccnt.get<int>() + par * pstride, b.ccnt_next = sh.ccnt.get<int>() + (1 - par) * pstride;
    b.cur_cur = sh.cursor2.get<int>() + par * pstride, b.cur_next = sh.cursor2.get<int>() + (1 - par) * pstride;
    sh.qtot.ensure(sizeof(int) * (size_t)b.nq, sh.device);
}

// this batch's counts must be zero on entry; the coarse select's count step adds to them, so if anything throws
// before the plan has consumed them, zero them again on the way out
struct CcntReset {
    int *p;
    int nlist;
    hipStream_t st;
    bool armed;
    ~CcntReset() {
        if (armed && std::uncaught_exceptions() > 0) (void)hipMemsetAsync(p, 0, sizeof(int) * kPlanCopies * (size_t)nlist, st);
    }
};

// The filter image, the mode (building an image at its first use) and the index's record of it.
void ivf_pick_mode(IvfBatch &b) {
    IvfIndex &ix = b.ix;
    IvfShard &sh = b.sh;
    const int nlist = ix.nlist, d = ix.d;
    // HIPANN_IVF_SEED=0 (A/B): the single launch
    static const bool seed_env = [] { const char *e = std::getenv("HIPANN_IVF_SEED"); return !e || std::atoi(e) != 0; }();
    IvfModeIn in;
    in.is_override = b.opts.form_override >= 0;
    in.form = in.is_override ? b.opts.form_override : ix.form;
    in.metric = ix.metric, in.d = d, in.k = b.k_user, in.kout = b.kout, in.np = b.np, in.max_nch = sh.max_nch;
    in.aligned16 = (uintptr_t)b.xq % 16 == 0 && (uintptr_t)sh.codes % 16 == 0;
    in.host_fb = host_fallback();
    in.seed_on = sh.dbg_seed < 0 ? seed_env : sh.dbg_seed != 0;  // (a test's per-handle override)
    const IvfImageChoice c = ivf_choose_filter_image(sh, ivf_filter_image_eligible(in, sh.n, sh.i8_state),
                                                     filter_image_mode(ix), b.nq, b.np, nlist, d);
    in.use_int8 = c.use_int8;
    b.probation = c.probation;
    b.m = ivf_resolve_mode(in, [&](int image) {
        return image == 2 ? ensure_i8_codes(sh, d, nlist, b.st) : ensure_half_codes(sh, d, nlist, b.st);
    });
    if (!b.opts.record()) return;
    const IvfScanMode &m = b.m;
    ix.last_form = m.last_form;
    ix.last_filter_image = m.exact && m.image == 2 ? 1 : 0;
    ix.last_kfilt = m.exact ? m.kfilt : 0;
    ix.last_sublists = m.sub ? ivf_scan_sublists() : 0;
    ix.last_seeded = m.seeded ? 1 : 0;
}

// The rerank's bounds and flags, the queries' bound words, and the batch's query preparation — one launch before the
// coarse step: the fp16 query terms, 1/(t·s) and the split residuals, or the int8 queries (units, scales, residuals),
// with ‖q‖² (row_norms_f32's bits) for the coarse quantizer and the scan.
void ivf_prepare_queries(IvfBatch &b) {
    IvfShard &sh = b.sh;
    const IvfScanMode &m = b.m;
    const int d = b.ix.d;
    const int64_t nq = b.nq;
    if (m.exact) {  // max‖x‖² (once per row set; nflag is its scratch, so before the plan resets the flag count)
        b.xmax2 = shard_xmax2(sh, d, b.st);
        // the int8 image's L2 certificate reads every row's own residual (ivf_rerank_topk); IP keeps the
        // Cauchy-Schwarz bound with the largest row residual
        if (m.image == 2 && !m.cert8) b.rxmax8 = shard_i8_rxmax(sh, b.st);
        sh.nflag.ensure(sizeof(int), sh.device);
        sh.flagged.ensure(sizeof(int) * (size_t)nq, sh.device);
    }
    if (m.tiled) {  // every query's bound starts at +inf (order-preserving bits 0xff800000), set by the plan
        sh.qbound.ensure(sizeof(unsigned) * (size_t)nq, sh.device);
        b.qbound = sh.qbound.get<unsigned>();
    }
    if (!m.image) return;
    float *qn_out = nullptr;
    if (b.ix.metric == kL2) {  // the quantizer's BLAS-form paths (nq >= 20) and the scan's L2 keys read ‖q‖²
        b.qsh.qn.ensure(sizeof(float) * (size_t)nq, sh.device);
        qn_out = b.qsh.qn.get<float>();
    }
    if (m.image == 1) {
        sh.hsplit.ensure((size_t)ivf_half_qsplit_bytes(nq, d), sh.device);
        sh.hits.ensure(sizeof(float) * (size_t)nq, sh.device);
        sh.hres.ensure(sizeof(float) * 2 * (size_t)nq, sh.device);  // two- and one-term split residuals
        RoctxRange rr("hipann.ivf.prepare");
        launch_ivf_split_queries_h(b.xq, nq, d, sh.half_es, sh.hsplit.p, sh.hits.get<float>(), sh.hres.get<float>(), qn_out,
                                   b.st);
    } else {
        sh.qi8.ensure((size_t)ivf_i8_qimg_bytes(nq, d), sh.device);
        sh.qs8.ensure(sizeof(float) * (size_t)nq, sh.device);
        sh.qres8.ensure(sizeof(float) * (size_t)nq, sh.device);
        sh.qhn2.ensure(sizeof(float) * (size_t)nq, sh.device);
        sh.qhn.ensure(sizeof(float) * (size_t)nq, sh.device);
        if (qn_out) launch_row_norms(b.xq, nq, d, qn_out, b.st);  // (row_norms_f32 itself: the coarse step's bits)
        RoctxRange rr("hipann.ivf.prepare");
        launch_ivf_split_queries_i8(b.xq, nq, d, sh.qi8.p, sh.qs8.get<float>(), sh.qres8.get<float>(),
                                    sh.qhn2.get<float>(), sh.qhn.get<float>(), b.st);
    }
    b.qsh.qn_given = qn_out ? b.xq : nullptr;
    b.qsh.qn_given_nq = nq;
}

// 1. coarse quantizer (FAISS: quantizer->search(n, x, nprobe) — Flat rules incl. nq < 20), 2. list-major work plan
void ivf_coarse_and_plan(IvfBatch &b) {
    IvfShard &sh = b.sh;
    const int nlist = b.ix.nlist, np = b.np;
    const int64_t nq = b.nq;
    // the plan's per-query count step rides on the coarse probe select when that path is taken
    IvfPlanHook hook{sh.list_len.get<int>(), nlist, ivf_chunk_rows(), b.ccnt_cur, sh.slot_off.get<int>(),
                     sh.qtot.get<int>(), false};
    if (b.opts.probes_in) {
        // the probe lists come from the caller (the coarse step partitioned over ranks, hipann_ivf_coarse_device +
        // one all-gather): no quantizer launch; the plan counts the probes itself
        HIPANN_CHECK(hipMemcpyAsync(sh.coarse_i.p, b.opts.probes_in, sizeof(int64_t) * (size_t)nq * np,
                                    hipMemcpyDeviceToDevice, b.st));
    } else {
        RoctxRange rr("hipann.ivf.coarse");
        b.qsh.plan_hook = &hook;
        CoarseKeysScope ck(b.qsh);
        try {
            flat_shard_search(*sh.quant, b.qsh, nq, b.xq, np, np, sh.coarse_d.get<float>(), sh.coarse_i.get<int64_t>(), b.st);
        } catch (...) {
            b.qsh.plan_hook = nullptr;
            b.qsh.qn_given = nullptr;
            throw;
        }
    }
    b.qsh.plan_hook = nullptr;
    b.qsh.qn_given = nullptr;
    sh.cnt.ensure(sizeof(int) * (nlist + 1), sh.device);
    sh.bucket_off.ensure(sizeof(int) * (nlist + 1), sh.device);
    sh.item_off.ensure(sizeof(int) * (nlist + 1), sh.device);
    sh.goff.ensure(sizeof(int) * (nlist + 1), sh.device);
    sh.bucket.ensure(sizeof(int) * (size_t)nq * np, sh.device);
    RoctxRange rr("hipann.ivf.plan");
    launch_ivf_plan(sh.coarse_i.get<int64_t>(), nq, np, sh.list_len.get<int>(), nlist, b.m.group, sh.cnt.get<int>(),
                    sh.bucket_off.get<int>(), sh.item_off.get<int>(), b.cur_cur, sh.bucket.get<int>(),
                    sh.slot_off.get<int>(), b.st, b.m.exact ? sh.nflag.get<int>() : nullptr, b.qbound, b.ccnt_cur,
                    sh.qtot.get<int>(), hook.done, b.ccnt_next, b.cur_next, sh.goff.get<int>());
    sh.plan_batch++;
}

// the scan's L2 key term ‖q‖² (nullptr: the direct form, or IP)
const float *ivf_query_norms(IvfBatch &b) {
    IvfShard &sh = b.sh;
    if (b.m.form == kFormDirect || b.ix.metric != kL2) return nullptr;
    if (b.opts.probes_in && b.m.image) return b.qsh.qn.get<float>();  // the query preparation wrote ‖q‖² there
    // the coarse quantizer's ‖q‖² of the same queries, written by THIS call's coarse step (with probes_in the
    // quantizer did not run, and a cached pointer match may name a buffer whose contents changed)
    if (!b.opts.probes_in && b.qsh.qn_of == b.xq && b.qsh.qn_nq == b.nq) return b.qsh.qn.get<float>();
    sh.qn.ensure(sizeof(float) * (size_t)b.nq, sh.device);
    launch_row_norms(b.xq, b.nq, b.ix.d, sh.qn.get<float>(), b.st);
    return sh.qn.get<float>();
}

// The seeded int8 scan: the chunk-0 items first, every wave's list a sub-list of the pair's slot; then
// the 64 best of a query's chunk-0 entries, whose 64th key is min'ed into the query's bound (ivf_seed_bound); then the
// other items under that bound, sub-lists again (so the rerank's bound B — the 64th candidate key or the smallest full
// sub-list's 16th — is the single launch's).  The chunk-0 slots (one per pair) take the head of part_d / part_i, the
// queries' candidate slots (common.hpp ivf_seed_run_slot) the rest: a query's run is its seed list, then the rows the
// second launch's waves append under run_cnt[q] — room for every (pair, chunk >= 1) sub-list in full, so no append can
// overflow; the rerank reads kSeedK + run_cnt[q] entries.
void ivf_scan_seeded(IvfBatch &b, IvfImageScanArgs a) {
    IvfShard &sh = b.sh;
    const int nlist = b.ix.nlist, np = b.np, kslot = b.m.kslot, group = b.m.group;
    const int64_t nq = b.nq;
    HIPANN_REQUIRE((int64_t)np * nq * sh.max_nch + nq < (int64_t)0x7fffffff, "too many candidate slots");
    HIPANN_REQUIRE((int64_t)np * sh.max_nch * kslot < (int64_t)0x7fffffff, "candidate run too long");
    sh.run_cnt.ensure(sizeof(int) * (size_t)nq, sh.device);
    b.cand_d = sh.part_d.get<float>() + (size_t)np * nq * kslot;
    b.cand_i = sh.part_i.get<int>() + (size_t)np * nq * kslot;
    IvfPlanView pairs = b.plan();
    pairs.slot_off = nullptr;
    a.phase = 1;
    launch_ivf_scan_mfma_h(a, pairs, ivf_max_items(nq, np, nlist, 1, 0, group), sh.part_d.get<float>(), sh.part_i.get<int>(),
                           b.st);
    launch_ivf_seed_bound(sh.part_d.get<float>(), sh.part_i.get<int>(), sh.slot_off.get<int>(), np, nq, kslot, sh.n,
                          b.qbound, b.cand_d, b.cand_i, sh.run_cnt.get<int>(), b.st);
    a.phase = 2;
    a.cursor = sh.run_cnt.get<int>();
    launch_ivf_scan_mfma_h(a, b.plan(), ivf_max_items(nq, np, nlist, sh.max_nch - 1, sh.n, group), b.cand_d, b.cand_i, b.st);
    // HIPANN_IVF_RUN_STATS=1 (measurement only: a stream sync and a readback per batch): the appended entries per query
    static const bool run_stats = [] { const char *e = std::getenv("HIPANN_IVF_RUN_STATS"); return e && std::atoi(e) != 0; }();
    if (!run_stats) return;
    std::vector<int> h((size_t)nq);
    HIPANN_CHECK(hipMemcpyAsync(h.data(), sh.run_cnt.p, sizeof(int) * (size_t)nq, hipMemcpyDeviceToHost, b.st));
    HIPANN_CHECK(hipStreamSynchronize(b.st));
    int64_t sum = 0, over = 0;
    int mx = 0;
    for (int c : h) { sum += c; mx = std::max(mx, c); over += kSeedK + c > 4096; }
    std::fprintf(stderr, "HIPANN_IVF_RUN_STATS nq=%lld appended_total=%lld mean=%.1f max=%d runs_over_4096=%lld\n",
                 (long long)nq, (long long)sum, (double)sum / (double)nq, mx, (long long)over);
}

// 3. scan: one k-list per (query, probe, row chunk) slot — every slot is written by exactly one item
// (the seeded scan: the pairs' chunk-0 slots, then the queries' candidate slots — one more per query)
void ivf_scan(IvfBatch &b) {
    IvfShard &sh = b.sh;
    const IvfScanMode &m = b.m;
    const int nlist = b.ix.nlist, d = b.ix.d, metric = b.ix.metric, np = b.np, k = m.kscan;
    const int64_t nq = b.nq;
    const size_t parts = ((size_t)np * nq * sh.max_nch + (m.seeded ? (size_t)np * nq + (size_t)nq : 0)) * m.kslot;
    HIPANN_REQUIRE((int64_t)np * nq * sh.max_nch < (int64_t)0x7fffffff, "too many partial lists");
    sh.part_d.ensure(parts * sizeof(float), sh.device);
    sh.part_i.ensure(parts * sizeof(int), sh.device);
    const int64_t max_items = ivf_max_items(nq, np, nlist, sh.max_nch, sh.n, m.group);
    const float *qn = b.qn = ivf_query_norms(b);
    if (m.tiled && !m.image) ensure_tiled_codes(sh, d, nlist, b.st);
    if (!m.image && ivf_form_split(m.form))  // (an image's query terms were prepared before the coarse step)
        sh.qsplit.ensure((size_t)ivf_mfma_bf_qsplit_bytes(nq, d, ivf_form_terms(m.form)), sh.device);
    float *pd = sh.part_d.get<float>();
    int *pi = sh.part_i.get<int>();
    const IvfPlanView plan = b.plan();
    RoctxRange rr("hipann.ivf.scan");
    ScopedTiming t(b.ix.timer_main, b.st);
    if (m.image) {
        const bool i8 = m.image == 2;
        IvfImageScanArgs a;
        a.nq = nq, a.d = d, a.metric = metric, a.k = k, a.sub = m.sub ? 1 : 0, a.qbound = b.qbound;
        a.tpass_off = sh.tpass_off.get<int64_t>(), a.xn = sh.xnorm.get<float>();
        if (i8) {  // its query units, scales and residuals; L2: ‖q̂‖² of the dequantised queries as the key's query term
            a.qsplit = sh.qi8.p, a.its = sh.qs8.get<float>(), a.qres = sh.qres8.get<float>();
            a.codes = sh.codes_i8.p, a.i8mode = 1, a.xs8 = sh.xs8.get<float>();
            a.qn = m.cert8 ? sh.qhn2.get<float>() : qn;
            if (m.cert8) a.xr8 = sh.xr8.get<float>(), a.qhn = sh.qhn.get<float>();
        } else {
            a.qsplit = sh.hsplit.p, a.its = sh.hits.get<float>(), a.qres = sh.hres.get<float>(), a.qn = qn;
            a.codes = sh.codes_h.p;
        }
        if (m.seeded) ivf_scan_seeded(b, a);
        else launch_ivf_scan_mfma_h(a, plan, max_items, pd, pi, b.st);
    } else if (m.bigk) {
        launch_ivf_scan_bigk(b.xq, d, metric, sh.codes, plan, sh.coarse_i.get<int64_t>(), nq * np,
                             nq * np * std::max(sh.max_nch, 1), k, pd, pi, b.st);
    } else if (ivf_form_split(m.form)) {
        launch_ivf_scan_mfma_bf(ivf_form_terms(m.form), b.xq, nq, sh.qsplit.p, qn, d, metric, sh.codes_t.get<float>(),
                                sh.tpass_off.get<int64_t>(), sh.xnorm.get<float>(), plan, k, max_items, b.qbound, pd, pi,
                                b.st, m.sub ? 1 : 0);
    } else if (m.form == kFormDecomposed) {
        launch_ivf_scan_mfma(b.xq, qn, d, metric, sh.codes_t.get<float>(), sh.tpass_off.get<int64_t>(),
                             sh.xnorm.get<float>(), plan, k, max_items, b.qbound, pd, pi, b.st);
    } else {
        launch_ivf_scan(b.xq, qn, d, metric, m.form, sh.codes, sh.xnorm.get<float>(), plan, nq, k, max_items, b.qbound, pd,
                        pi, b.st);
    }
}

// what the scan saw (hipann_debug_ivf_info / _read)
void ivf_record_debug(IvfBatch &b) {
    IvfShard &sh = b.sh;
    const IvfScanMode &m = b.m;
    sh.dbg_nq = b.nq;
    sh.dbg_np = b.np;
    sh.dbg_kslot = m.kslot;
    sh.dbg_sub = m.sub ? 1 : 0;
    sh.dbg_img = m.image;
    sh.dbg_seeded = m.seeded ? 1 : 0;
    sh.dbg_kfilt = m.exact ? m.kfilt : 0;
    sh.dbg_cand_off = m.seeded ? (int64_t)b.np * b.nq * m.kslot : -1;
    sh.dbg_qn = b.qn;  // (the int8 L2 scan's key term is qhn2 instead; the rerank reads this one)
}

// 4. the exact forms: merge + exact rerank + bound check.  Flagged queries re-run on the device in the direct form,
// each by the rerank wave that flagged it (ivf_block_fallback inline: no host readback and no launch of its own) —
// inline_fb; else they are left in nflag / flagged (probation's count, or the host's re-run).
void ivf_rerank(IvfBatch &b, bool inline_fb) {
    IvfShard &sh = b.sh;
    const IvfScanMode &m = b.m;
    const int nlist = b.ix.nlist, d = b.ix.d, metric = b.ix.metric, np = b.np, kout = b.kout;
    const int64_t nq = b.nq;
    int fb_cap = 0, fb_maxch = 1;
    if (inline_fb) {
        if (!sh.fb_total.p) {
            sh.fb_total.ensure(sizeof(unsigned long long), sh.device);
            HIPANN_CHECK(hipMemsetAsync(sh.fb_total.p, 0, sizeof(unsigned long long), b.st));
        }
        sh.fpd.ensure(sizeof(float) * (size_t)nq * np * kout, sh.device);
        sh.fpi.ensure(sizeof(long long) * (size_t)nq * np * kout, sh.device);
        // the parallel re-run of the batch's first fb_cap flagged queries (ivf_fallback_chunks): one wave per (query,
        // probe, chunk) item; its lists take ≤ 64 MB (fb_cap shrinks for long lists), later flagged queries re-run in
        // the flagging wave as before
        fb_maxch = sh.max_nch;
        const size_t per_f = (size_t)np * fb_maxch * kout * (sizeof(float) + sizeof(long long));
        fb_cap = (int)std::min<int64_t>({nq, 64, std::max<int64_t>(1, (int64_t)(((size_t)64 << 20) / per_f))});
        sh.fbc_d.ensure(sizeof(float) * (size_t)fb_cap * np * fb_maxch * kout, sh.device);
        sh.fbc_i.ensure(sizeof(long long) * (size_t)fb_cap * np * fb_maxch * kout, sh.device);
        if (sh.fbc_cap < fb_cap || !sh.fbc_done.p) {  // counters start (and are left) at zero
            sh.fbc_done.ensure(sizeof(unsigned) * (size_t)std::max(fb_cap, 64), sh.device);
            HIPANN_CHECK(hipMemsetAsync(sh.fbc_done.p, 0, sh.fbc_done.bytes, b.st));
            sh.fbc_cap = (int)(sh.fbc_done.bytes / sizeof(unsigned));
        }
    }
    RoctxRange rr("hipann.ivf.rerank");
    ScopedTiming t(b.ix.timer_merge, b.st);
    IvfRerankArgs a;
    a.pd = m.seeded ? b.cand_d : sh.part_d.get<float>(), a.pi = m.seeded ? b.cand_i : sh.part_i.get<int>();
    a.slot_off = sh.slot_off.get<int>(), a.nprobe = np, a.nq = nq, a.k = m.kfilt, a.kout = kout, a.metric = metric;
    a.Q = b.xq, a.codes = sh.codes, a.d = d, a.ids = sh.ids, a.nrows = sh.n, a.xmax2 = b.xmax2, a.D = b.D, a.I = b.I;
    a.nflag = sh.nflag.get<int>(), a.flagged = sh.flagged.get<int>();
    a.rxmax = m.image == 2 ? b.rxmax8 : m.image == 1 ? sh.half_rxmax : -1.f;
    a.qres = m.image == 2 ? sh.qres8.get<float>() : m.image == 1 ? sh.hres.get<float>() : nullptr;
    a.probes = sh.coarse_i.get<int64_t>(), a.list_off = sh.list_off.get<int64_t>(), a.nlist = nlist, a.qbound = b.qbound;
    a.qnorm = m.image && metric == kL2 ? b.qn : nullptr, a.kslot = m.kslot, a.sub = m.sub ? 1 : 0;
    if (inline_fb) {
        a.list_len = sh.list_len.get<int>(), a.fpd = sh.fpd.get<float>(), a.fpi = sh.fpi.get<long long>();
        a.fb_total = sh.fb_total.get<unsigned long long>();
    }
    a.fb_cap = fb_cap, a.i8_l2 = m.cert8 ? 1 : 0, a.seed_cnt = m.seeded ? sh.run_cnt.get<int>() : nullptr;
    launch_ivf_rerank(a, b.st);
    if (fb_cap > 0)
        launch_ivf_fallback_chunks(sh.nflag.get<int>(), sh.flagged.get<int>(), fb_cap, np, fb_maxch, ivf_chunk_rows(),
                                   kout, metric, b.xq, sh.codes, d, sh.ids, 0, sh.coarse_i.get<int64_t>(),
                                   sh.list_off.get<int64_t>(), sh.list_len.get<int>(), nlist, sh.fbc_d.get<float>(),
                                   sh.fbc_i.get<long long>(), sh.fbc_done.get<unsigned>(), b.D, b.I,
                                   sh.fb_total.get<unsigned long long>(), b.st,
                                   m.as_half && !b.probation ? auto8_host_word(sh) : nullptr, (unsigned)++sh.fb_seq);
}

// Probation: the batch has been answered through the fp16 image; the same batch runs once more on the same stream
// through the int8 image into scratch outputs, counting only (no flagged query is re-run, nothing the caller sees is
// written).  The flag count is read back — probation's one host synchronisation — and decides by the byte rule.
void ivf_probation(IvfBatch &b) {
    IvfIndex &ix = b.ix;
    IvfShard &sh = b.sh;
    sh.auto8_live = sh.live;
    sh.auto8_over = 0;
    sh.auto8 = -1;
    if (!ensure_i8_codes(sh, ix.d, ix.nlist, b.st)) return;
    sh.probe_D.ensure(sizeof(float) * (size_t)b.nq * b.kout, sh.device);
    sh.probe_I.ensure(sizeof(int64_t) * (size_t)b.nq * b.kout, sh.device);
    {
        TimerPause p0(ix.timer_main), p1(ix.timer_merge);
        IvfSearchOpts o;
        o.form_override = kFormI8Exact, o.probes_in = b.opts.probes_in, o.count_only = true;
        ivf_shard_search(ix, sh, b.nq, b.xq, b.k_user, b.kout, sh.probe_D.get<float>(), sh.probe_I.get<int64_t>(), b.st, o);
    }
    int nf = 0;
    HIPANN_CHECK(hipMemcpyAsync(&nf, sh.nflag.p, sizeof(int), hipMemcpyDeviceToHost, b.st));
    HIPANN_CHECK(hipStreamSynchronize(b.st));
    if (!auto8_over_rule(nf, std::min(ix.nprobe, ix.nlist), ix.nlist, sh.live, ix.d)) sh.auto8 = 1;
}

// HIPANN_IVF_HOST_FALLBACK=1: the flag count is read back and the flagged queries re-run on the 3-term path (the
// batch's probe lists are kept for last_probes)
void ivf_host_rerun(IvfBatch &b) {
    IvfIndex &ix = b.ix;
    IvfShard &sh = b.sh;
    const int d = ix.d, kout = b.kout;
    int nf = 0;
    HIPANN_CHECK(hipMemcpyAsync(&nf, sh.nflag.p, sizeof(int), hipMemcpyDeviceToHost, b.st));
    HIPANN_CHECK(hipStreamSynchronize(b.st));
    if (nf <= 0) return;
    ix.rerank_fallbacks += nf;
    const size_t pbytes = sizeof(int64_t) * (size_t)b.nq * b.np;
    sh.coarse_save.ensure(pbytes, sh.device);
    HIPANN_CHECK(hipMemcpyAsync(sh.coarse_save.p, sh.coarse_i.p, pbytes, hipMemcpyDeviceToDevice, b.st));
    sh.fq.ensure(sizeof(float) * (size_t)nf * d, sh.device);
    sh.fD.ensure(sizeof(float) * (size_t)nf * kout, sh.device);
    sh.fI.ensure(sizeof(int64_t) * (size_t)nf * kout, sh.device);
    launch_ivf_gather_queries(b.xq, sh.flagged.get<int>(), nf, d, sh.fq.get<float>(), b.st);
    {
        TimerPause p0(ix.timer_main), p1(ix.timer_merge);
        IvfSearchOpts o;
        o.form_override = kFormSplit3;
        ivf_shard_search(ix, sh, nf, sh.fq.get<float>(), b.k_user, kout, sh.fD.get<float>(), sh.fI.get<int64_t>(), b.st, o);
    }
    launch_ivf_scatter_results(sh.fD.get<float>(), sh.fI.get<int64_t>(), sh.flagged.get<int>(), nf, kout, b.D, b.I, b.st);
    HIPANN_CHECK(hipMemcpyAsync(sh.coarse_i.p, sh.coarse_save.p, pbytes, hipMemcpyDeviceToDevice, b.st));
}

}  // namespace

// One shard: queries on the shard's device → D/I (nq × kout) on the same device, async on `st`.
void ivf_shard_search(IvfIndex &ix, IvfShard &sh, int64_t nq, const float *xq, int k, int kout, float *D, int64_t *I,
                      hipStream_t st, const IvfSearchOpts &opts) {
    RoctxRange r_all("hipann.ivf.search_shard");
    DeviceGuard g(sh.device);
    if (nq <= 0) return;
    IvfBatch b{ix, sh, nq, xq, k, kout, D, I, st, opts, std::min(ix.nprobe, ix.nlist), {}, false, *sh.quant->shards[0]};
    ivf_plan_scratch(b);
    CcntReset ccnt_reset{b.ccnt_cur, ix.nlist, st, true};
    ivf_pick_mode(b);
    ivf_prepare_queries(b);
    ivf_coarse_and_plan(b);
    ccnt_reset.armed = false;
    ivf_scan(b);
    if (opts.record()) ivf_record_debug(b);
    if (sh.dbg_stop) return;  // a test reads the scan's buffers as they are
    if (!b.m.exact) {  // 4. merge each query's partial lists
        ScopedTiming t(ix.timer_merge, st);
        launch_ivf_merge(sh.part_d.get<float>(), sh.part_i.get<int>(), sh.ids, sh.n, sh.slot_off.get<int>(), b.np, nq,
                         b.m.kscan, kout, ix.metric == kIP ? -1.f : 1.f, D, I, st);
        return;
    }
    const bool inline_fb = !host_fallback() && !opts.count_only;
    ivf_rerank(b, inline_fb);
    if (opts.count_only) return;  // probation's pass: the flag count stays in nflag, nothing is re-run
    if (b.probation) ivf_probation(b);
    if (!inline_fb) ivf_host_rerun(b);
}



// Grow a shard's CSR so that list l can take add[l] more rows: every list gets capacity max(cap, need + max(need / 4,
// 64)) rows — geometric growth (O(1) amortised copies per appended row, the doubling of MetalIndexFlat::add,
// MetalIndexFlat.mm:255-269, at ×1.25: a 10M × 768 table at ×2 would hold 61 GB of codes);
// borrowed storage is copied into owned buffers.  Live rows, labels, norms and the tiled images' passes move list by
// list (device-to-device, in order); the slack rows are zero (whole-table maxima read them).
static void ivf_relayout(IvfIndex &ix, IvfShard &sh, const std::vector<int64_t> &add) {
    const int nlist = ix.nlist, d = ix.d;
    hipStream_t st = sh.stream;
    // every list leaves with room for a quarter more than it will hold (≥ 64 rows): DuckDB's 2048-row chunks touch
    // most lists of a 1024-list index, so growing only the overflowing ones would relayout on nearly every append
    std::vector<int64_t> off(nlist + 1, 0);
    for (int l = 0; l < nlist; ++l) {
        const int64_t cap = sh.h_off[l + 1] - sh.h_off[l], need = sh.h_len[l] + add[l];
        const int64_t ncap = std::max(cap, need + std::max<int64_t>(need / 4, 64));
        off[l + 1] = off[l] + ncap;
    }
    const int64_t N = off[nlist];
    std::vector<int64_t> tp_old(nlist + 1, 0), tp(nlist + 1, 0);
    for (int l = 0; l < nlist; ++l) {
        tp_old[l + 1] = tp_old[l] + ceil_div(sh.h_off[l + 1] - sh.h_off[l], 32);
        tp[l + 1] = tp[l] + ceil_div(off[l + 1] - off[l], 32);
    }
    auto take = [](DevBuf &dst, DevBuf &src) {
        std::swap(dst.p, src.p);
        std::swap(dst.bytes, src.bytes);
        std::swap(dst.device, src.device);
    };
    // One array at a time — allocate its new layout, move its live lists (device-to-device, list by list, in order),
    // wait, swap, free the old one — so the transient peak is one array's old + new copy (2× the codes at most), not
    // every array twice.  `unit` = bytes per row (rows) or per 32-row pass (the tiled images); `pass` = per pass.
    auto move_array = [&](DevBuf &cur, const void *src_base, size_t unit, bool pass, size_t count) {
        auto nb = std::make_unique<DevBuf>();
        nb->ensure(unit * std::max<size_t>(count, 1), sh.device);
        HIPANN_CHECK(hipMemsetAsync(nb->p, 0, nb->bytes, st));
        for (int l = 0; l < nlist; ++l) {
            const int64_t len = sh.h_len[l];
            if (!len) continue;
            const int64_t o0 = pass ? tp_old[l] : sh.h_off[l], o1 = pass ? tp[l] : off[l];
            const int64_t cnt = pass ? ceil_div(len, 32) : len;  // passes holding live rows (past len: zero)
            HIPANN_CHECK(hipMemcpyAsync(static_cast<char *>(nb->p) + unit * (size_t)o1,
                                        static_cast<const char *>(src_base) + unit * (size_t)o0, unit * (size_t)cnt,
                                        hipMemcpyDeviceToDevice, st));
        }
        HIPANN_CHECK(hipStreamSynchronize(st));
        take(cur, *nb);  // nb now holds the old storage; freed here (borrowed storage: cur was empty)
    };
    move_array(sh.codes_buf, sh.codes, sizeof(float) * (size_t)d, false, (size_t)N);
    sh.codes = sh.codes_buf.get<float>();  // borrowed storage becomes owned here
    move_array(sh.ids_buf, sh.ids, sizeof(int64_t), false, (size_t)N);
    sh.ids = sh.ids_buf.get<int64_t>();
    sh.owns_codes = true;
    // L2 shards always leave with a norm array: a shard created empty (compute_row_norms skips n = 0) has none yet,
    // and ivf_append_rows writes the new rows' norms into it (the decomposed / fp16 scans read it)
    if (ix.metric == kL2) {
        if (sh.xnorm.p) {
            move_array(sh.xnorm, sh.xnorm.p, sizeof(float), false, (size_t)N);
        } else {
            sh.xnorm.ensure(sizeof(float) * (size_t)std::max<int64_t>(N, 1), sh.device);
            HIPANN_CHECK(hipMemsetAsync(sh.xnorm.p, 0, sh.xnorm.bytes, st));
        }
    }
    const bool img_h = sh.half_state > 0 && sh.codes_h.p, img_t = sh.codes_t.p != nullptr;
    const bool img_8 = sh.i8_state > 0 && sh.codes_i8.p;
    if (img_h) move_array(sh.codes_h, sh.codes_h.p, (size_t)ivf_half_pass_bytes(d), true, (size_t)tp[nlist]);
    if (img_t)
        move_array(sh.codes_t, sh.codes_t.p, sizeof(float) * (size_t)ivf_mfma_pass_floats(d), true, (size_t)tp[nlist]);
    if (img_8) {  // the int8 image's passes and its per-row scales and residuals
        move_array(sh.codes_i8, sh.codes_i8.p, (size_t)ivf_i8_pass_bytes(d), true, (size_t)tp[nlist]);
        move_array(sh.xs8, sh.xs8.p, sizeof(float), false, (size_t)N);
        move_array(sh.xr8, sh.xr8.p, sizeof(float), false, (size_t)N);
    }
    if (img_h || img_t || img_8) {
        sh.tpass_off.ensure(sizeof(int64_t) * (nlist + 1), sh.device);
        HIPANN_CHECK(hipMemcpyAsync(sh.tpass_off.p, tp.data(), sizeof(int64_t) * (nlist + 1), hipMemcpyHostToDevice, st));
        HIPANN_CHECK(hipStreamSynchronize(st));  // tp (host) is released on return
    } else {
        sh.tpass_off.release();  // recomputed from the new capacities when an image is built
    }
    upload_list_meta(sh, off, sh.h_len, nlist);
}

// IndexIVF::add_with_ids (FAISS 1.13.2, external): rows are assigned to their nearest centroid by the
// coarse quantizer (quantizer->assign, k = 1) and appended to their lists in insertion order; labels are `ids`
// or ntotal + i.  On the GPU copy this replaces the reference's invalidate-on-append (faiss_index.cpp:469): the new
// rows go into their lists' slack in HBM (ivf_relayout grows the lists that overflow, amortised), with their norms,
// the touched passes of the tiled images and running maxima — the cost of an append is the appended rows, not the
// table.
static void ivf_add_block(IvfIndex &ix, int64_t n, const float *xb, const int64_t *ids, int64_t base);

static void ivf_add_rows(IvfIndex &ix, int64_t n, const float *xb, const int64_t *ids) {
    // every shard's pending searches (possibly on other streams) finish before its buffers change
    std::vector<std::unique_ptr<FenceScope>> fences;
    for (auto &shp : ix.shards) fences.push_back(std::make_unique<FenceScope>(shp->fence, shp->stream, shp->device));
    // FAISS assigns in blocks of 65536 rows (so the Flat nq < 20 direct-form rule applies per block); each block's
    // rows follow the previous block's in their lists (insertion order)
    const int64_t bs = 65536;
    for (int64_t r0 = 0; r0 < n; r0 += bs) {
        const int64_t m = std::min(bs, n - r0);
        ivf_add_block(ix, m, xb + r0 * (int64_t)ix.d, ids ? ids + r0 : nullptr, ix.ntotal());
    }
}

// One block of an add: rows to the device once; on shard 0's device the block's norms and, per shard, the block's
// maxima at that shard's fp16 scale (ivf_append_rows' statistics-only pass), then the coarse assignment on the GPU
// (shard 0's quantizer; every shard holds all centroids) — assignment and maxima come back in ONE readback, the block's
// only host wait.  The host folds the maxima (an image the new rows leave is dropped before it is re-tiled) and
// computes each row's physical destination; then per shard owning a list with new rows: grow the lists that overflow
// (ivf_relayout, amortised), one pinned upload (double-buffered: the next block writes the other buffer while this
// one's copy may still be queued), scatter each row straight into its list's slack (one kernel: codes, label, norm),
// re-tile the tiled images' touched passes.  Nothing waits for that tail: the next search is queued behind it.
static void ivf_add_block(IvfIndex &ix, int64_t n, const float *xb, const int64_t *ids, int64_t base) {
    RoctxRange r_all("hipann.ivf.add");
    const int d = ix.d, nlist = ix.nlist, metric = ix.metric;
    const int nsh = (int)ix.shards.size();
    IvfShard &s0 = *ix.shards[0];
    DeviceGuard g0(s0.device);
    hipStream_t st = s0.stream;
    // HIPANN_APPEND_PROF=1 (tuning): host-side phase times of each block on stderr
    static const bool prof = std::getenv("HIPANN_APPEND_PROF") != nullptr;
    using clk = std::chrono::steady_clock;
    const auto t_0 = clk::now();
    auto us = [&](clk::time_point a) { return std::chrono::duration<double, std::micro>(clk::now() - a).count(); };
    s0.app_rows.ensure(sizeof(float) * (size_t)n * d, s0.device);
    s0.app_norm.ensure(sizeof(float) * (size_t)n, s0.device);
    s0.app_assign.ensure(sizeof(int64_t) * (size_t)n, s0.device);
    HIPANN_CHECK(hipMemcpyAsync(s0.app_rows.p, xb, sizeof(float) * (size_t)n * d, hipMemcpyHostToDevice, st));
    double t_h2d = 0.0;
    if (prof) {
        HIPANN_CHECK(hipStreamSynchronize(st));
        t_h2d = us(t_0);
    }
    // the block's ‖x‖² (the table kernel's bits, the norms the append writes on shard 0) and per shard the maxima
    // [max ‖x‖², max |x|, max fp16 residual² at the shard's image scale]
    launch_row_norms(s0.app_rows.get<float>(), n, d, s0.app_norm.get<float>(), st);
    s0.app_stat.ensure(sizeof(unsigned) * 4 * (size_t)nsh, s0.device);
    unsigned *stat = s0.app_stat.get<unsigned>();
    for (int s = 0; s < nsh; ++s) {
        const IvfShard &sh = *ix.shards[s];
        const bool img_h = sh.half_state > 0 && sh.codes_h.p;
        launch_ivf_append_rows(s0.app_rows.get<float>(), s0.app_norm.get<float>(), nullptr, nullptr, n, d, nullptr,
                               nullptr, nullptr, nullptr, nullptr, 0, img_h ? std::ldexp(1.f, sh.half_es) : 0.f,
                               stat + 4 * s, st);
    }
    s0.app_cd.ensure(sizeof(float) * (size_t)n, s0.device);  // the assignment's distances (discarded)
    flat_shard_search(*s0.quant, *s0.quant->shards[0], n, s0.app_rows.get<float>(), 1, 1, s0.app_cd.get<float>(),
                      s0.app_assign.get<int64_t>(), st);
    s0.app_hassign.ensure(sizeof(int64_t) * (size_t)n + sizeof(unsigned) * 4 * (size_t)nsh);
    const int64_t *assign = s0.app_hassign.get<int64_t>();
    const unsigned *hstat = reinterpret_cast<const unsigned *>(assign + n);
    HIPANN_CHECK(hipMemcpyAsync(s0.app_hassign.p, s0.app_assign.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost,
                                st));
    HIPANN_CHECK(hipMemcpyAsync(const_cast<unsigned *>(hstat), stat, sizeof(unsigned) * 4 * (size_t)nsh,
                                hipMemcpyDeviceToHost, st));
    // the block's one host wait, polled (wait_event: no interrupt wake-up on the append's critical path)
    if (!s0.app_sync) HIPANN_CHECK(hipEventCreateWithFlags(&s0.app_sync, hipEventDisableTiming));
    HIPANN_CHECK(hipEventRecord(s0.app_sync, st));
    wait_event(s0.app_sync);
    const double t_assign = prof ? us(t_0) : 0.0;
    std::vector<int64_t> cnt(nlist, 0);
    for (int64_t i = 0; i < n; ++i) {
        HIPANN_REQUIRE(assign[i] >= 0 && assign[i] < nlist, "coarse assignment out of range");
        ++cnt[assign[i]];
    }
    for (int s = 0; s < nsh; ++s) {
        IvfShard &sh = *ix.shards[s];
        std::vector<int64_t> add(nlist, 0);
        int64_t add_s = 0;
        bool grow = !sh.owns_codes;
        for (int l = 0; l < nlist; ++l) {
            if (ix.owner[l] != s) continue;
            add[l] = cnt[l];
            add_s += add[l];
            if (sh.h_len[l] + add[l] > sh.h_off[l + 1] - sh.h_off[l]) grow = true;
        }
        if (!add_s) continue;
        // the block's maxima (over all its rows: for a shard that takes only some of them the bounds are at worst
        // slightly loose, never wrong) folded before anything is written
        const unsigned *hs = hstat + 4 * s;
        float v;
        std::memcpy(&v, &hs[0], sizeof(v));
        if (sh.xmax2 >= 0.f) sh.xmax2 = std::max(sh.xmax2, v);  // max ‖x‖² (the rerank bound's row term)
        if (sh.half_state > 0 && sh.codes_h.p) {
            float mx, r2;
            std::memcpy(&mx, &hs[1], sizeof(mx));
            std::memcpy(&r2, &hs[2], sizeof(r2));
            if (hs[1] >= 0x7f800000u) {  // a non-finite new entry: the fp16 form no longer applies (form 5 runs)
                sh.half_state = -1;
                sh.codes_h.release();
            } else if (mx >= std::ldexp(1.f, 14 - sh.half_es)) {  // outside the image's scale: rebuilt at the next search
                sh.half_state = 0;
                sh.codes_h.release();
            } else {
                sh.half_rxmax = std::max(sh.half_rxmax, std::sqrt(r2) * 1.0001f);
            }
        }
        // the int8 image keeps no whole-table statistic for L2 (per-row residuals): only a non-finite new entry ends it
        if (sh.i8_state > 0 && hs[1] >= 0x7f800000u) release_i8_codes(sh, -1);
        DeviceGuard g(sh.device);
        hipStream_t ss = sh.stream;
        if (&sh != &s0) {  // the block's rows (and their norms) on this shard's device too
            sh.app_rows.ensure(sizeof(float) * (size_t)n * d, sh.device);
            sh.app_norm.ensure(sizeof(float) * (size_t)n, sh.device);
            HIPANN_CHECK(hipMemcpyAsync(sh.app_rows.p, xb, sizeof(float) * (size_t)n * d, hipMemcpyHostToDevice, ss));
            launch_row_norms(sh.app_rows.get<float>(), n, d, sh.app_norm.get<float>(), ss);
        }
        if (grow) ivf_relayout(ix, sh, add);
        // one pinned upload: [physical destination per row (−1: another shard's list) | label per row | the tiled
        // passes the rows touch | the new live length per list (int)]
        std::vector<int64_t> len = sh.h_len;
        std::vector<int64_t> tp0(nlist);
        int64_t np = 0, tp = 0;
        for (int l = 0; l < nlist; ++l) {
            tp0[l] = tp;
            tp += ceil_div(sh.h_off[l + 1] - sh.h_off[l], 32);
            if (add[l]) np += ceil_div(len[l] + add[l], 32) - len[l] / 32;
        }
        const size_t up_bytes = sizeof(int64_t) * (size_t)(2 * n + np) + sizeof(int) * (size_t)nlist;
        const int b = sh.app_buf;
        sh.app_buf ^= 1;
        if (sh.app_ev[b]) HIPANN_CHECK(hipEventSynchronize(sh.app_ev[b]));  // its copy two blocks ago (long done)
        HostBuf &hup = sh.app_hup[b];
        hup.ensure(up_bytes);
        int64_t *dst = hup.get<int64_t>(), *lab = dst + n, *passes = lab + n;
        int *newlen = reinterpret_cast<int *>(passes + np);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t l = assign[i];
            dst[i] = ix.owner[l] == s ? sh.h_off[l] + len[l]++ : -1;
            lab[i] = ids ? ids[i] : base + i;
        }
        int64_t pi = 0, maxlen = 0, live = 0;
        for (int l = 0; l < nlist; ++l) {
            for (int64_t p = sh.h_len[l] / 32; add[l] && p < ceil_div(len[l], 32); ++p) passes[pi++] = tp0[l] + p;
            HIPANN_REQUIRE(len[l] < (int64_t)0x7fffffff, "inverted list longer than 2^31-1 rows");
            newlen[l] = (int)len[l];
            maxlen = std::max(maxlen, len[l]);
            live += len[l];
        }
        sh.app_up.ensure(up_bytes, sh.device);
        HIPANN_CHECK(hipMemcpyAsync(sh.app_up.p, hup.p, up_bytes, hipMemcpyHostToDevice, ss));
        if (!sh.app_ev[b]) HIPANN_CHECK(hipEventCreateWithFlags(&sh.app_ev[b], hipEventDisableTiming));
        HIPANN_CHECK(hipEventRecord(sh.app_ev[b], ss));
        const int64_t *ddst = sh.app_up.get<int64_t>(), *dlab = ddst + n, *dpass = dlab + n;
        const int *dlen = reinterpret_cast<const int *>(dpass + np);
        const bool img_h = sh.half_state > 0 && sh.codes_h.p, img_t = sh.codes_t.p != nullptr;
        const bool img_8 = sh.i8_state > 0 && sh.codes_i8.p;
        const float hscale = std::ldexp(1.f, sh.half_es);
        // one kernel: rows, labels and norms into their CSR rows, the new lengths
        launch_ivf_append_rows(sh.app_rows.get<float>(), sh.app_norm.get<float>(), ddst, dlab, n, d,
                               sh.codes_buf.get<float>(), sh.ids_buf.get<int64_t>(),
                               metric == kL2 ? sh.xnorm.get<float>() : nullptr, dlen, sh.list_len.get<int>(), nlist,
                               0.f, nullptr, ss);
        sh.h_len = len;
        sh.live = live;
        sh.max_nch = (int)std::max<int64_t>(1, ceil_div(maxlen, ivf_chunk_rows()));
        // the touched passes of the tiled images, re-tiled from the grown lists
        if (np > 0 && img_h)
            launch_ivf_tile_half(sh.codes, sh.list_off.get<int64_t>(), sh.list_len.get<int>(), sh.tpass_off.get<int64_t>(),
                                 nlist, np, d, hscale, sh.codes_h.p, ss, dpass);
        if (np > 0 && img_t)
            launch_ivf_tile_codes(sh.codes, sh.list_off.get<int64_t>(), sh.list_len.get<int>(),
                                  sh.tpass_off.get<int64_t>(), nlist, np, d, sh.codes_t.get<float>(), ss, dpass);
        if (np > 0 && img_8) {  // (scales and residuals of the passes' rows with them; the IP bound's maximum is retaken)
            launch_ivf_tile_i8(sh.codes, sh.list_off.get<int64_t>(), sh.list_len.get<int>(), sh.tpass_off.get<int64_t>(),
                               nlist, np, d, sh.codes_i8.p, sh.xs8.get<float>(), sh.xr8.get<float>(), nullptr, ss, dpass);
            sh.i8_tiled += np;
            sh.i8_rxmax = -1.f;
        }
        if (prof) {
            HIPANN_CHECK(hipStreamSynchronize(ss));
            std::fprintf(stderr, "hipann append: n %lld h2d %.0f us, assign %.0f us, shard %d done %.0f us (grow %d, %lld passes)\n",
                         (long long)n, t_h2d, t_assign, s, us(t_0), (int)grow, (long long)np);
        }
    }
}

// What one shard's removal needs on the device, allocated for every shard before any shard's rows move.
struct IvfRemoval {
    DevBuf labels, mark, plan, pass_ids, out;  // out: [npass u64 | newlen int × nlist]
    bool img_h = false, img_t = false, img_8 = false;
};

// faiss::IndexIVF::remove_ids (FAISS 1.13.2, DirectMap NoMap: per list j = 0, l = len; while (j < l) { if
// member(id[j]) { --l; entry[j] = entry[l]; } else ++j; }) on the GPU copy.  Each shard works on the lists it owns,
// on the device (ivf_remove_rows: one block per list marks, plans the moves in closed form, moves code row, id and
// norm, zeroes the vacated rows — the slack stays zero for the whole-table maxima — and writes the new length); the
// host reads back only the new lengths and the count of tiled passes to re-tile.  List starts do not change: the
// freed rows are append slack a later add reuses.  The fp16 / fp32 tiled images are re-tiled at the passes holding a
// destination or a vacated row; the int8 image's likewise, with its rows' scales and residuals.  xmax2, half_rxmax and the fp16
// scale stay: maxima over a superset of the rows, still upper bounds.  A borrowed handle moves into owned storage
// first (ivf_relayout, as at its first add).  Every buffer of every shard is allocated before the first kernel that
// moves a row; the cost is the label lookup (8 B per live row) plus the rows moved.
static int64_t ivf_remove_rows(IvfIndex &ix, const std::vector<int64_t> &lab) {
    const int nlist = ix.nlist, d = ix.d;
    const int64_t m = (int64_t)lab.size();
    const int64_t before = ix.ntotal();
    // every shard's pending searches (possibly on other streams) finish before its rows move
    std::vector<std::unique_ptr<FenceScope>> fences;
    for (auto &shp : ix.shards) fences.push_back(std::make_unique<FenceScope>(shp->fence, shp->stream, shp->device));
    const size_t ns = ix.shards.size();
    std::vector<IvfRemoval> rm(ns);
    for (size_t s = 0; s < ns; ++s) {
        IvfShard &sh = *ix.shards[s];
        if (!sh.live) continue;
        DeviceGuard g(sh.device);
        if (!sh.owns_codes) ivf_relayout(ix, sh, std::vector<int64_t>(nlist, 0));  // same rows, owned storage
        IvfRemoval &r = rm[s];
        r.img_h = sh.half_state > 0 && sh.codes_h.p;
        r.img_t = sh.codes_t.p != nullptr;
        r.img_8 = sh.i8_state > 0 && sh.codes_i8.p;
        r.labels.ensure(sizeof(int64_t) * (size_t)m, sh.device);
        r.mark.ensure((size_t)sh.n, sh.device);
        r.plan.ensure(sizeof(int) * (size_t)sh.n, sh.device);
        r.out.ensure(sizeof(unsigned long long) + sizeof(int) * (size_t)nlist, sh.device);
        if (r.img_h || r.img_t || r.img_8) {
            HIPANN_REQUIRE(sh.tpass_off.p, "tiled image without pass offsets");
            int64_t tp = 0;
            for (int l = 0; l < nlist; ++l) tp += ceil_div(sh.h_off[l + 1] - sh.h_off[l], 32);
            r.pass_ids.ensure(sizeof(int64_t) * (size_t)std::max<int64_t>(tp, 1), sh.device);  // each pass at most once
        }
    }
    for (size_t s = 0; s < ns; ++s) {
        IvfShard &sh = *ix.shards[s];
        if (!sh.live) continue;
        IvfRemoval &r = rm[s];
        DeviceGuard g(sh.device);
        hipStream_t st = sh.stream;
        unsigned long long *npass = r.out.get<unsigned long long>();
        int *newlen = reinterpret_cast<int *>(npass + 1);
        HIPANN_CHECK(hipMemcpyAsync(r.labels.p, lab.data(), sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, st));
        HIPANN_CHECK(hipMemsetAsync(npass, 0, sizeof(unsigned long long), st));
        launch_ivf_remove_rows(r.labels.get<int64_t>(), m, sh.list_off.get<int64_t>(), sh.list_len.get<int>(), nlist, d,
                               sh.codes_buf.get<float>(), sh.ids_buf.get<int64_t>(),
                               ix.metric == kL2 ? sh.xnorm.get<float>() : nullptr, r.mark.get<unsigned char>(),
                               r.plan.get<int>(), r.pass_ids.p ? sh.tpass_off.get<int64_t>() : nullptr,
                               r.pass_ids.get<int64_t>(), npass, newlen, st);
        std::vector<char> host(sizeof(unsigned long long) + sizeof(int) * (size_t)nlist);
        HIPANN_CHECK(hipMemcpyAsync(host.data(), r.out.p, host.size(), hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        unsigned long long np = 0;
        std::memcpy(&np, host.data(), sizeof(np));
        const int *hl = reinterpret_cast<const int *>(host.data() + sizeof(unsigned long long));
        int64_t live = 0, maxlen = 0;
        for (int l = 0; l < nlist; ++l) {
            sh.h_len[l] = hl[l];
            live += hl[l];
            maxlen = std::max<int64_t>(maxlen, hl[l]);
        }
        const bool changed = live != sh.live;
        sh.live = live;
        sh.max_nch = (int)std::max<int64_t>(1, ceil_div(maxlen, ivf_chunk_rows()));
        if (!changed) continue;
        // the touched passes of the tiled images, re-tiled from the shortened lists
        if (np > 0 && r.img_h)
            launch_ivf_tile_half(sh.codes, sh.list_off.get<int64_t>(), sh.list_len.get<int>(), sh.tpass_off.get<int64_t>(),
                                 nlist, (int64_t)np, d, std::ldexp(1.f, sh.half_es), sh.codes_h.p, st,
                                 r.pass_ids.get<int64_t>());
        if (np > 0 && r.img_t)
            launch_ivf_tile_codes(sh.codes, sh.list_off.get<int64_t>(), sh.list_len.get<int>(),
                                  sh.tpass_off.get<int64_t>(), nlist, (int64_t)np, d, sh.codes_t.get<float>(), st,
                                  r.pass_ids.get<int64_t>());
        if (np > 0 && r.img_8) {
            launch_ivf_tile_i8(sh.codes, sh.list_off.get<int64_t>(), sh.list_len.get<int>(), sh.tpass_off.get<int64_t>(),
                               nlist, (int64_t)np, d, sh.codes_i8.p, sh.xs8.get<float>(), sh.xr8.get<float>(), nullptr, st,
                               r.pass_ids.get<int64_t>());
            sh.i8_tiled += (int64_t)np;
        }
        HIPANN_CHECK(hipStreamSynchronize(st));  // synchronous: the staging buffers are freed on return
        if (sh.i8_state < 0) sh.i8_state = 0;  // the non-finite row may be gone: tried again at the next int8 search
    }
    return before - ix.ntotal();
}

}  // namespace hipann

extern "C" {

void *hipann_ivf_create(int d, int metric, int nlist, int nprobe, const float *centroids, const int64_t *list_offsets,
                        const int64_t *ids, const float *codes, const int *devices, int ndev, char *eb, int el) {
    return guard_ptr(eb, el, [&]() -> void * {
        int ndevs = 0;
        if (hipGetDeviceCount(&ndevs) != hipSuccess || ndevs <= 0) throw HipError("hipann: no HIP device");
        HIPANN_REQUIRE(d > 0 && nlist > 0, "d and nlist must be > 0");
        HIPANN_REQUIRE(metric == kL2 || metric == kIP, "metric must be 0 (L2) or 1 (IP)");
        HIPANN_REQUIRE(nprobe >= 1, "nprobe must be >= 1");
        HIPANN_REQUIRE(centroids && list_offsets, "null centroids / offsets");
        std::vector<int> devs;
        if (!devices || ndev <= 0) devs.push_back(0);
        else devs.assign(devices, devices + ndev);
        for (int dv : devs) HIPANN_REQUIRE(dv >= 0 && dv < ndevs, "invalid device id");
        const int64_t n = list_offsets[nlist];
        HIPANN_REQUIRE(list_offsets[0] == 0 && n >= 0, "list offsets must start at 0");
        for (int l = 0; l < nlist; ++l) HIPANN_REQUIRE(list_offsets[l + 1] >= list_offsets[l], "offsets not monotone");
        HIPANN_REQUIRE(n == 0 || (ids && codes), "null ids / codes");

        auto ix = std::make_unique<IvfIndex>();
        ix->d = d;
        ix->metric = metric;
        ix->nlist = nlist;
        ix->nprobe = nprobe;
        // size-balanced list → shard assignment (largest first onto the least-loaded shard)
        const int ns = (int)devs.size();
        std::vector<int> owner(nlist, 0);
        if (ns > 1) {
            std::vector<int> order(nlist);
            std::iota(order.begin(), order.end(), 0);
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
                return list_offsets[a + 1] - list_offsets[a] > list_offsets[b + 1] - list_offsets[b];
            });
            std::vector<int64_t> load(ns, 0);
            for (int l : order) {
                const int s = (int)(std::min_element(load.begin(), load.end()) - load.begin());
                owner[l] = s;
                load[s] += list_offsets[l + 1] - list_offsets[l];
            }
        }
        ix->owner = owner;
        for (int s = 0; s < ns; ++s) {
            auto sh = std::make_unique<IvfShard>();
            sh->device = devs[s];
            sh->stream = make_stream(devs[s]);
            DeviceGuard g(sh->device);
            std::vector<int64_t> off(nlist + 1, 0);
            for (int l = 0; l < nlist; ++l)
                off[l + 1] = off[l] + (owner[l] == s ? list_offsets[l + 1] - list_offsets[l] : 0);
            sh->n = off[nlist];
            sh->centroids_buf.ensure(sizeof(float) * (size_t)nlist * d, sh->device);
            HIPANN_CHECK(hipMemcpyAsync(sh->centroids_buf.p, centroids, sizeof(float) * (size_t)nlist * d,
                                        hipMemcpyHostToDevice, sh->stream));
            sh->centroids = sh->centroids_buf.get<float>();
            sh->codes_buf.ensure(sizeof(float) * (size_t)std::max<int64_t>(sh->n, 1) * d, sh->device);
            sh->ids_buf.ensure(sizeof(int64_t) * (size_t)std::max<int64_t>(sh->n, 1), sh->device);
            for (int l = 0; l < nlist; ++l) {
                if (owner[l] != s) continue;
                const int64_t cnt = list_offsets[l + 1] - list_offsets[l];
                if (!cnt) continue;
                HIPANN_CHECK(hipMemcpyAsync(sh->codes_buf.get<float>() + off[l] * d, codes + list_offsets[l] * d,
                                            sizeof(float) * (size_t)cnt * d, hipMemcpyHostToDevice, sh->stream));
                HIPANN_CHECK(hipMemcpyAsync(sh->ids_buf.get<int64_t>() + off[l], ids + list_offsets[l],
                                            sizeof(int64_t) * (size_t)cnt, hipMemcpyHostToDevice, sh->stream));
            }
            sh->codes = sh->codes_buf.get<float>();
            sh->ids = sh->ids_buf.get<int64_t>();
            sh->owns_codes = true;
            HIPANN_CHECK(hipStreamSynchronize(sh->stream));
            upload_list_meta(*sh, off, dense_lengths(off, nlist), nlist);
            compute_row_norms(*sh, d, metric);
            sh->quant = make_quantizer(d, metric, sh->centroids, nlist, sh->device, sh->stream);
            ix->shards.push_back(std::move(sh));
        }
        ix->peer = enable_peer_access(devs);
        return ix.release();
    });
}

void *hipann_ivf_create_device(int d, int metric, int nlist, int nprobe, const float *centroids_dev,
                               const int64_t *list_offsets, const int64_t *ids_dev, const float *codes_dev, int device,
                               int copy, char *eb, int el) {
    return guard_ptr(eb, el, [&]() -> void * {
        int ndevs = 0;
        if (hipGetDeviceCount(&ndevs) != hipSuccess || ndevs <= 0) throw HipError("hipann: no HIP device");
        HIPANN_REQUIRE(device >= 0 && device < ndevs, "invalid device");
        HIPANN_REQUIRE(d > 0 && nlist > 0 && nprobe >= 1, "bad arguments");
        HIPANN_REQUIRE(metric == kL2 || metric == kIP, "metric must be 0 (L2) or 1 (IP)");
        HIPANN_REQUIRE(centroids_dev && list_offsets, "null centroids / offsets");
        const int64_t n = list_offsets[nlist];
        HIPANN_REQUIRE(list_offsets[0] == 0 && n >= 0, "list offsets must start at 0");
        HIPANN_REQUIRE(n == 0 || (ids_dev && codes_dev), "null ids / codes");
        auto ix = std::make_unique<IvfIndex>();
        ix->d = d;
        ix->metric = metric;
        ix->nlist = nlist;
        ix->nprobe = nprobe;
        ix->owner.assign(nlist, 0);
        auto sh = std::make_unique<IvfShard>();
        sh->device = device;
        sh->stream = make_stream(device);
        sh->n = n;
        DeviceGuard g(device);
        HIPANN_CHECK(hipDeviceSynchronize());  // caller's writes to the inputs may still be in flight
        if (copy) {
            sh->centroids_buf.ensure(sizeof(float) * (size_t)nlist * d, device);
            sh->codes_buf.ensure(sizeof(float) * (size_t)std::max<int64_t>(n, 1) * d, device);
            sh->ids_buf.ensure(sizeof(int64_t) * (size_t)std::max<int64_t>(n, 1), device);
            HIPANN_CHECK(hipMemcpyAsync(sh->centroids_buf.p, centroids_dev, sizeof(float) * (size_t)nlist * d,
                                        hipMemcpyDeviceToDevice, sh->stream));
            if (n) {
                HIPANN_CHECK(hipMemcpyAsync(sh->codes_buf.p, codes_dev, sizeof(float) * (size_t)n * d,
                                            hipMemcpyDeviceToDevice, sh->stream));
                HIPANN_CHECK(hipMemcpyAsync(sh->ids_buf.p, ids_dev, sizeof(int64_t) * (size_t)n,
                                            hipMemcpyDeviceToDevice, sh->stream));
            }
            sh->centroids = sh->centroids_buf.get<float>();
            sh->codes = sh->codes_buf.get<float>();
            sh->ids = sh->ids_buf.get<int64_t>();
            sh->owns_codes = true;
        } else {
            sh->centroids = centroids_dev;
            sh->codes = codes_dev;
            sh->ids = ids_dev;
        }
        std::vector<int64_t> off(list_offsets, list_offsets + nlist + 1);
        upload_list_meta(*sh, off, dense_lengths(off, nlist), nlist);
        compute_row_norms(*sh, d, metric);
        sh->quant = make_quantizer(d, metric, sh->centroids, nlist, device, sh->stream);
        ix->shards.push_back(std::move(sh));
        return ix.release();
    });
}

static int ivf_search_host(IvfIndex &ix, int64_t nq, const float *xq, int64_t k, float *D, int64_t *I) {
    HIPANN_REQUIRE(k > 0, "k must be > 0");
    HIPANN_REQUIRE(k <= HIPANN_MAX_K, "k larger than HIPANN_MAX_K");
    HIPANN_REQUIRE(nq >= 0 && (nq == 0 || (xq && D && I)), "invalid arguments");
    const float pad = ix.metric == kIP ? -__builtin_inff() : __builtin_inff();
    const int64_t ntot = ix.ntotal();
    ix.last_nq = nq;
    ix.last_np = std::min(ix.nprobe, ix.nlist);
    if (nq == 0) return 0;
    if (ntot == 0) {
        for (int64_t i = 0; i < nq * k; ++i) { D[i] = pad; I[i] = -1; }
        return 0;
    }
    const int keff = (int)std::min<int64_t>(k, ntot);
    const int kout = (int)k;
    const size_t qbytes = (size_t)nq * ix.d * sizeof(float);
    ix.h_q.ensure(qbytes);
    std::memcpy(ix.h_q.p, xq, qbytes);
    const size_t ob = (size_t)nq * kout;
    for (auto &shp : ix.shards) {
        IvfShard &sh = *shp;
        DeviceGuard g(sh.device);
        sh.q.ensure(qbytes, sh.device);
        sh.out_d.ensure(ob * sizeof(float), sh.device);
        sh.out_i.ensure(ob * sizeof(int64_t), sh.device);
        FenceScope fs(sh.fence, sh.stream, sh.device);
        if (qbytes <= kKernelCopyMax) launch_copy_words(host_device_ptr(ix.h_q.p), sh.q.p, qbytes, sh.stream);
        else HIPANN_CHECK(hipMemcpyAsync(sh.q.p, ix.h_q.p, qbytes, hipMemcpyHostToDevice, sh.stream));
        ivf_shard_search(ix, sh, nq, sh.q.get<float>(), keff, kout, sh.out_d.get<float>(), sh.out_i.get<int64_t>(),
                         sh.stream);
        if (ix.shards.size() > 1) {  // shard 0's stream waits for it on the device (no host wait per shard)
            if (!sh.done) HIPANN_CHECK(hipEventCreateWithFlags(&sh.done, hipEventDisableTiming));
            HIPANN_CHECK(hipEventRecord(sh.done, sh.stream));
        }
    }
    ix.h_d.ensure(ob * sizeof(float));
    ix.h_i.ensure(ob * sizeof(int64_t));
    IvfShard &s0 = *ix.shards[0];
    if (ix.shards.size() == 1) {
        DeviceGuard g(s0.device);
        if (ob * sizeof(int64_t) <= kKernelCopyMax) {
            launch_copy_words(s0.out_d.p, host_device_ptr(ix.h_d.p), ob * sizeof(float), s0.stream);
            launch_copy_words(s0.out_i.p, host_device_ptr(ix.h_i.p), ob * sizeof(int64_t), s0.stream);
        } else {
            HIPANN_CHECK(hipMemcpyAsync(ix.h_d.p, s0.out_d.p, ob * sizeof(float), hipMemcpyDeviceToHost, s0.stream));
            HIPANN_CHECK(hipMemcpyAsync(ix.h_i.p, s0.out_i.p, ob * sizeof(int64_t), hipMemcpyDeviceToHost, s0.stream));
        }
        HIPANN_CHECK(hipStreamSynchronize(s0.stream));
    } else {
        const int np = (int)ix.shards.size();
        ix.gather_d.ensure(ob * np * sizeof(float), s0.device);
        ix.gather_i.ensure(ob * np * sizeof(int64_t), s0.device);
        ix.merged_d.ensure(ob * sizeof(float), s0.device);
        ix.merged_i.ensure(ob * sizeof(int64_t), s0.device);
        DeviceGuard g0(s0.device);
        for (int p = 0; p < np; ++p) {
            IvfShard &sh = *ix.shards[p];
            if (p > 0) HIPANN_CHECK(hipStreamWaitEvent(s0.stream, sh.done, 0));
            HIPANN_CHECK(hipMemcpyPeerAsync(ix.gather_d.get<float>() + p * ob, s0.device, sh.out_d.p, sh.device,
                                            ob * sizeof(float), s0.stream));
            HIPANN_CHECK(hipMemcpyPeerAsync(ix.gather_i.get<int64_t>() + p * ob, s0.device, sh.out_i.p, sh.device,
                                            ob * sizeof(int64_t), s0.stream));
        }
        const float sign = ix.metric == kIP ? -1.f : 1.f;
        launch_merge_parts<long long>(ix.gather_d.get<float>(), ix.gather_i.get<long long>(), np, nq, kout, kout, 0,
                                      sign, sign, ix.merged_d.get<float>(), ix.merged_i.get<int64_t>(), s0.stream);
        HIPANN_CHECK(hipMemcpyAsync(ix.h_d.p, ix.merged_d.p, ob * sizeof(float), hipMemcpyDeviceToHost, s0.stream));
        HIPANN_CHECK(hipMemcpyAsync(ix.h_i.p, ix.merged_i.p, ob * sizeof(int64_t), hipMemcpyDeviceToHost, s0.stream));
        HIPANN_CHECK(hipStreamSynchronize(s0.stream));
    }
    std::memcpy(D, ix.h_d.p, ob * sizeof(float));
    std::memcpy(I, ix.h_i.p, ob * sizeof(int64_t));
    return 0;
}

int hipann_ivf_search(void *h, int64_t nq, const float *xq, int64_t k, float *D, int64_t *I, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h, "null index");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::IVF, "not an IVFFlat index");
        auto *vx = static_cast<IvfIndex *>(ix);
        std::lock_guard<std::mutex> lk(vx->mu);
        return ivf_search_host(*vx, nq, xq, k, D, I);
    });
}

int hipann_ivf_search_np(void *h, int nprobe, int64_t nq, const float *xq, int64_t k, float *D, int64_t *I, char *eb,
                         int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h, "null index");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::IVF, "not an IVFFlat index");
        auto *vx = static_cast<IvfIndex *>(ix);
        std::lock_guard<std::mutex> lk(vx->mu);
        if (nprobe <= 0) return ivf_search_host(*vx, nq, xq, k, D, I);
        // the call's nprobe, read and restored under the handle's lock (concurrent connections with
        // different SearchParametersIVF never see each other's value)
        const int saved = vx->nprobe;
        vx->nprobe = nprobe;
        try {
            const int rc = ivf_search_host(*vx, nq, xq, k, D, I);
            vx->nprobe = saved;
            return rc;
        } catch (...) {
            vx->nprobe = saved;
            throw;
        }
    });
}

int hipann_ivf_search_device(void *h, int64_t nq, const float *xq_dev, int64_t k, float *D_dev, int64_t *I_dev,
                             void *stream, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h, "null index");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::IVF, "not an IVFFlat index");
        auto *vx = static_cast<IvfIndex *>(ix);
        std::lock_guard<std::mutex> lk(vx->mu);
        HIPANN_REQUIRE(vx->shards.size() == 1, "device search needs a single-device index");
        HIPANN_REQUIRE(k > 0 && k <= HIPANN_MAX_K, "k out of range");
        IvfShard &sh = *vx->shards[0];
        hipStream_t st = static_cast<hipStream_t>(stream);  // NULL = the default (null) stream
        vx->last_nq = nq;
        vx->last_np = std::min(vx->nprobe, vx->nlist);
        const int keff = (int)std::min<int64_t>(k, std::max<int64_t>(sh.live, 1));
        FenceScope fs(sh.fence, st, sh.device);  // the previous call's kernels may still use this shard's scratch
        ivf_shard_search(*vx, sh, nq, xq_dev, keff, (int)k, D_dev, I_dev, st);
        return 0;
    });
}

int hipann_ivf_coarse_device(void *h, int64_t nq, const float *xq_dev, int64_t *probes_dev, void *stream, char *eb,
                             int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h, "null index");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::IVF, "not an IVFFlat index");
        auto *vx = static_cast<IvfIndex *>(ix);
        std::lock_guard<std::mutex> lk(vx->mu);
        HIPANN_REQUIRE(vx->shards.size() == 1, "device coarse step needs a single-device index");
        HIPANN_REQUIRE(nq >= 0 && (nq == 0 || (xq_dev && probes_dev)), "invalid arguments");
        if (nq == 0) return 0;
        IvfShard &sh = *vx->shards[0];
        DeviceGuard g(sh.device);
        hipStream_t st = static_cast<hipStream_t>(stream);
        const int np = std::min(vx->nprobe, vx->nlist);
        FenceScope fs(sh.fence, st, sh.device);
        sh.app_cd.ensure(sizeof(float) * (size_t)nq * np, sh.device);
        // FAISS quantizer->search(nq, x, nprobe): the Flat rules of the coarse quantizer (exact fp32 products)
        CoarseKeysScope ck(*sh.quant->shards[0]);
        flat_shard_search(*sh.quant, *sh.quant->shards[0], nq, xq_dev, np, np, sh.app_cd.get<float>(), probes_dev, st);
        return 0;
    });
}

int hipann_ivf_search_probes_device(void *h, int64_t nq, const float *xq_dev, const int64_t *probes_dev, int64_t k,
                                    float *D_dev, int64_t *I_dev, void *stream, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h, "null index");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::IVF, "not an IVFFlat index");
        auto *vx = static_cast<IvfIndex *>(ix);
        std::lock_guard<std::mutex> lk(vx->mu);
        HIPANN_REQUIRE(vx->shards.size() == 1, "device search needs a single-device index");
        HIPANN_REQUIRE(k > 0 && k <= HIPANN_MAX_K, "k out of range");
        HIPANN_REQUIRE(nq >= 0 && (nq == 0 || (xq_dev && probes_dev && D_dev && I_dev)), "invalid arguments");
        IvfShard &sh = *vx->shards[0];
        hipStream_t st = static_cast<hipStream_t>(stream);
        vx->last_nq = nq;
        vx->last_np = std::min(vx->nprobe, vx->nlist);
        const int keff = (int)std::min<int64_t>(k, std::max<int64_t>(sh.live, 1));
        FenceScope fs(sh.fence, st, sh.device);
        IvfSearchOpts o;
        o.probes_in = probes_dev;
        ivf_shard_search(*vx, sh, nq, xq_dev, keff, (int)k, D_dev, I_dev, st, o);
        return 0;
    });
}

int hipann_ivf_add(void *h, int64_t n, const float *xb, const int64_t *ids, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h, "null index");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::IVF, "not an IVFFlat index");
        auto *vx = static_cast<IvfIndex *>(ix);
        std::lock_guard<std::mutex> lk(vx->mu);
        HIPANN_REQUIRE(n >= 0 && (n == 0 || xb), "invalid vectors");
        if (n > 0) ivf_add_rows(*vx, n, xb, ids);
        return 0;
    });
}

int64_t hipann_ivf_remove_ids(void *h, const int64_t *labels, int64_t n, char *eb, int el) {
    try {
        HIPANN_REQUIRE(h, "null index");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::IVF, "not an IVFFlat index");
        HIPANN_REQUIRE(n >= 0 && (n == 0 || labels), "invalid labels");
        if (n == 0) return 0;
        auto *vx = static_cast<IvfIndex *>(ix);
        std::lock_guard<std::mutex> lk(vx->mu);
        std::vector<int64_t> lab(labels, labels + n);  // FAISS's IDSelectorBatch: a set
        std::sort(lab.begin(), lab.end());
        lab.erase(std::unique(lab.begin(), lab.end()), lab.end());
        return ivf_remove_rows(*vx, lab);
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return -1;
}

// the handle as an IVFFlat index (nullptr: null, or another kind)
static IvfIndex *as_ivf(void *h) {
    auto *ix = static_cast<IndexBase *>(h);
    return ix && ix->kind == Kind::IVF ? static_cast<IvfIndex *>(ix) : nullptr;
}

int hipann_ivf_nlist(void *h) {
    IvfIndex *vx = as_ivf(h);
    return vx ? vx->nlist : -1;
}

int hipann_ivf_get_nprobe(void *h) {
    IvfIndex *vx = as_ivf(h);
    if (!vx) return -1;
    std::lock_guard<std::mutex> lk(vx->mu);
    return vx->nprobe;
}

int hipann_ivf_export(void *h, float *centroids, int64_t *list_offsets, int64_t *ids, float *codes, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h, "null index");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::IVF, "not an IVFFlat index");
        auto *vx = static_cast<IvfIndex *>(ix);
        std::lock_guard<std::mutex> lk(vx->mu);
        const int nlist = vx->nlist, d = vx->d;
        std::vector<int64_t> off(nlist + 1, 0);
        for (int l = 0; l < nlist; ++l) {
            const IvfShard &sh = *vx->shards[vx->owner[l]];
            off[l + 1] = off[l] + sh.h_len[l];  // live rows (the shard's physical list may hold append slack)
        }
        if (list_offsets) std::memcpy(list_offsets, off.data(), sizeof(int64_t) * (nlist + 1));
        IvfShard &s0 = *vx->shards[0];
        if (centroids) {
            DeviceGuard g(s0.device);
            HIPANN_CHECK(hipMemcpyAsync(centroids, s0.centroids, sizeof(float) * (size_t)nlist * d, hipMemcpyDeviceToHost,
                                        s0.stream));
            HIPANN_CHECK(hipStreamSynchronize(s0.stream));
        }
        for (int l = 0; l < nlist && (ids || codes); ++l) {
            IvfShard &sh = *vx->shards[vx->owner[l]];
            const int64_t len = off[l + 1] - off[l];
            if (!len) continue;
            DeviceGuard g(sh.device);
            if (codes)
                HIPANN_CHECK(hipMemcpyAsync(codes + off[l] * d, sh.codes + sh.h_off[l] * d, sizeof(float) * (size_t)len * d,
                                            hipMemcpyDeviceToHost, sh.stream));
            if (ids)
                HIPANN_CHECK(hipMemcpyAsync(ids + off[l], sh.ids + sh.h_off[l], sizeof(int64_t) * (size_t)len,
                                            hipMemcpyDeviceToHost, sh.stream));
        }
        for (auto &shp : vx->shards) {
            DeviceGuard g(shp->device);
            HIPANN_CHECK(hipStreamSynchronize(shp->stream));
        }
        return 0;
    });
}

int hipann_ivf_last_probes(void *h, int64_t *probes, int64_t cap, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h && probes, "null argument");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::IVF, "not an IVFFlat index");
        auto *vx = static_cast<IvfIndex *>(ix);
        std::lock_guard<std::mutex> lk(vx->mu);
        const int64_t m = vx->last_nq * vx->last_np;
        HIPANN_REQUIRE(cap >= m, "probe buffer too small");
        if (m == 0) return 0;
        IvfShard &sh = *vx->shards[0];
        DeviceGuard g(sh.device);
        HIPANN_CHECK(hipStreamSynchronize(sh.stream));
        HIPANN_CHECK(hipDeviceSynchronize());
        HIPANN_CHECK(hipMemcpy(probes, sh.coarse_i.p, sizeof(int64_t) * (size_t)m, hipMemcpyDeviceToHost));
        return 0;
    });
}

int hipann_ivf_set_nprobe(void *h, int nprobe) {
    IvfIndex *vx = as_ivf(h);
    if (!vx || nprobe < 1) return -1;
    std::lock_guard<std::mutex> lk(vx->mu);
    vx->nprobe = nprobe;
    return 0;
}

int hipann_ivf_set_form(void *h, int form) {
    IvfIndex *vx = as_ivf(h);
    if (!vx || form < kFormDecomposed || form > kFormI8Exact) return -1;
    std::lock_guard<std::mutex> lk(vx->mu);
    vx->form = form;
    return 0;
}

int64_t hipann_ivf_rerank_fallbacks(void *h) {
    IvfIndex *vx = as_ivf(h);
    if (!vx) return -1;
    std::lock_guard<std::mutex> lk(vx->mu);
    int64_t t = vx->rerank_fallbacks;  // host re-runs (HIPANN_IVF_HOST_FALLBACK)
    for (auto &sh : vx->shards) {       // + the device re-runs' running count
        if (!sh->fb_total.p) continue;
        DeviceGuard g(sh->device);
        unsigned long long v = 0;
        if (hipDeviceSynchronize() != hipSuccess) return -1;
        if (hipMemcpy(&v, sh->fb_total.p, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        t += (int64_t)v;
    }
    return t;
}

int hipann_ivf_set_filter_image(void *h, int mode) {
    IvfIndex *vx = as_ivf(h);
    if (!vx || mode < 0 || mode > 2) return -1;
    std::lock_guard<std::mutex> lk(vx->mu);
    vx->filter_image = mode;
    return 0;
}

int hipann_ivf_get_filter_image(void *h) {
    IvfIndex *vx = as_ivf(h);
    return vx ? vx->filter_image : -1;
}

int hipann_ivf_last_filter_image(void *h) {
    IvfIndex *vx = as_ivf(h);
    return vx ? vx->last_filter_image : -1;
}

int hipann_ivf_last_seeded(void *h) {
    IvfIndex *vx = as_ivf(h);
    return vx ? vx->last_seeded : -1;
}

int64_t hipann_ivf_i8_passes_tiled(void *h) {
    IvfIndex *vx = as_ivf(h);
    if (!vx) return -1;
    std::lock_guard<std::mutex> lk(vx->mu);
    int64_t t = 0;
    for (auto &sh : vx->shards) t += sh->i8_tiled;
    return t;
}

int hipann_ivf_get_form(void *h) {
    IvfIndex *vx = as_ivf(h);
    return vx ? vx->form : -1;
}

// ---- test hooks ------------------------------------------------------------------------------------------------------
// The scan mode of a batch as ivf_shard_search resolves it, with no device (tests/test_ivf_scan_mode.py).
// in[0..17): form, is_override, metric, d, k, kout, np, max_nch, alignment (bit 0: queries, bit 1: codes on 16 bytes),
// host fallback, seed switch, build mask (bit 0: the fp16 image "builds", bit 1: the int8 image), filter-image mode,
// nq, the shard's rows, i8_state, auto8.  out[0..17): form, last_form, exact, image, sub, kscan, kslot, kfilt, seeded,
// tiled, cert8, group, bigk, the images asked for (mask as the build mask), filter image eligible, taken, probation.
// 0, or -1 on short arrays or a value out of range.
int hipann_debug_ivf_scan_mode(const int *in, int nin, int *out, int nout) {
    if (!in || !out || nin < 17 || nout < 17 || in[3] < 1 || in[4] < 1 || in[5] < 1 || in[6] < 1 || in[7] < 1) return -1;
    if (in[0] < kFormDecomposed || in[0] > kFormI8Exact || (in[2] != kL2 && in[2] != kIP) || in[12] < 0 || in[12] > 2) return -1;
    IvfModeIn mi;
    mi.form = in[0], mi.is_override = in[1] != 0, mi.metric = in[2], mi.d = in[3], mi.k = in[4], mi.kout = in[5];
    mi.np = in[6], mi.max_nch = in[7], mi.aligned16 = (in[8] & 3) == 3, mi.host_fb = in[9] != 0, mi.seed_on = in[10] != 0;
    const int build = in[11];
    IvfShard sh;  // host fields only
    sh.n = sh.live = sh.auto8_live = in[14];
    sh.i8_state = in[15];
    sh.auto8 = in[16];
    const bool eligible = ivf_filter_image_eligible(mi, sh.n, sh.i8_state);
    const IvfImageChoice c = ivf_choose_filter_image(sh, eligible, in[12], in[13], mi.np, /*nlist=*/mi.np, mi.d);
    mi.use_int8 = c.use_int8;
    int asked = 0;
    const IvfScanMode m = ivf_resolve_mode(mi, [&](int image) {
        asked |= 1 << (image - 1);
        return (build >> (image - 1) & 1) != 0;
    });
    const int o[17] = {m.form, m.last_form, m.exact, m.image, m.sub, m.kscan, m.kslot, m.kfilt, m.seeded,
                       m.tiled, m.cert8, m.group, m.bigk, asked, eligible, m.as_half, c.probation};
    std::copy(o, o + 17, out);
    return 0;
}

// tests/test_ivf_scan_gpu.py: a single-shard IVF handle's scan stages as the product runs them
static IvfShard *dbg_shard(void *h) {
    IvfIndex *vx = as_ivf(h);
    return vx && vx->shards.size() == 1 ? vx->shards[0].get() : nullptr;
}

// stop: 1 = ivf_shard_search returns after its scan step (D / I stay unwritten), 0 = the normal search.
// seed: the seeded int8 scan by HIPANN_IVF_SEED (-1), off (0), on (1).  -1 on a bad handle or value.
int hipann_debug_ivf_set(void *h, int stop, int seed) {
    IvfShard *sh = dbg_shard(h);
    if (!sh || stop < 0 || stop > 1 || seed < -1 || seed > 1) return -1;
    std::lock_guard<std::mutex> lk(static_cast<IvfIndex *>(h)->mu);
    sh->dbg_stop = stop;
    sh->dbg_seed = seed;
    return 0;
}

// A scalar of the shard or of its last search by name; 0 on success, -1 on a bad handle or an unknown name.
int hipann_debug_ivf_info(void *h, const char *name, double *out) {
    IvfShard *sh = dbg_shard(h);
    if (!sh || !name || !out) return -1;
    auto *vx = static_cast<IvfIndex *>(h);
    std::lock_guard<std::mutex> lk(vx->mu);
    const std::string s(name);
    const int d = vx->d;
    if (s == "half_state") *out = sh->half_state;
    else if (s == "half_es") *out = sh->half_es;
    else if (s == "half_rxmax") *out = sh->half_rxmax;
    else if (s == "half_nsup") *out = (double)(ivf_half_pass_bytes(d) / 2048);
    else if (s == "i8_state") *out = sh->i8_state;
    else if (s == "i8_rxmax") *out = sh->i8_rxmax;
    else if (s == "i8_nsup") *out = (double)(ivf_i8_pass_bytes(d) / 2048);
    else if (s == "xmax2") *out = sh->xmax2;
    else if (s == "max_nch") *out = sh->max_nch;
    else if (s == "n") *out = (double)sh->n;
    else if (s == "nq") *out = (double)sh->dbg_nq;
    else if (s == "nprobe") *out = sh->dbg_np;
    else if (s == "kslot") *out = sh->dbg_kslot;
    else if (s == "kfilt") *out = sh->dbg_kfilt;
    else if (s == "sub") *out = sh->dbg_sub;
    else if (s == "image") *out = sh->dbg_img;
    else if (s == "seeded") *out = sh->dbg_seeded;
    else if (s == "cand_off") *out = (double)sh->dbg_cand_off;
    else if (s == "group") *out = sh->dbg_img == 2 ? ivf_mfma_i8_group(d) : sh->dbg_img == 1 ? ivf_mfma_h_group(d) : 0;
    else return -1;
    return 0;
}

// A shard buffer by name: copies min(cap, its bytes) into host memory `out` (fill >= 0: instead sets every byte of the
// buffer to `fill`, for sentinels) after the device has drained.  Returns the buffer's allocated bytes (0: not
// allocated), or -1 on a bad handle, an unknown name or a HIP error.
int64_t hipann_debug_ivf_read(void *h, const char *name, void *out, int64_t cap, int fill) {
    IvfShard *sh = dbg_shard(h);
    if (!sh || !name || cap < 0 || (cap > 0 && !out) || fill > 255) return -1;
    auto *vx = static_cast<IvfIndex *>(h);
    std::lock_guard<std::mutex> lk(vx->mu);
    const std::string s(name);
    const void *p = nullptr;
    size_t bytes = 0;
    const std::pair<const char *, const DevBuf *> tab[] = {
        {"codes_h", &sh->codes_h}, {"codes_i8", &sh->codes_i8}, {"xs8", &sh->xs8}, {"xr8", &sh->xr8},
        {"tpass_off", &sh->tpass_off}, {"xnorm", &sh->xnorm}, {"hsplit", &sh->hsplit}, {"hits", &sh->hits},
        {"hres", &sh->hres}, {"qi8", &sh->qi8}, {"qs8", &sh->qs8}, {"qres8", &sh->qres8}, {"qhn2", &sh->qhn2},
        {"qhn", &sh->qhn}, {"cnt", &sh->cnt}, {"bucket_off", &sh->bucket_off}, {"item_off", &sh->item_off},
        {"goff", &sh->goff}, {"bucket", &sh->bucket}, {"slot_off", &sh->slot_off}, {"part_d", &sh->part_d},
        {"part_i", &sh->part_i}, {"qbound", &sh->qbound}, {"run_cnt", &sh->run_cnt}, {"list_len", &sh->list_len},
        {"list_off", &sh->list_off}, {"nflag", &sh->nflag}, {"flagged", &sh->flagged}};
    bool found = false;
    for (const auto &e : tab)
        if (s == e.first) {
            p = e.second->p;
            bytes = e.second->bytes;
            found = true;
        }
    if (s == "qn") {  // the ‖q‖² of the last search's queries (the coarse quantizer's or the shard's buffer)
        p = sh->dbg_qn;
        bytes = p ? sizeof(float) * (size_t)sh->dbg_nq : 0;
        found = true;
    }
    if (!found) return -1;
    if (!p) return 0;
    DeviceGuard g(sh->device);
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (fill >= 0) {
        if (s == "qn" || hipMemset(const_cast<void *>(p), fill, bytes) != hipSuccess) return -1;
    } else if (cap > 0) {
        if (hipMemcpy(out, p, std::min<size_t>((size_t)cap, bytes), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    }
    return (int64_t)bytes;
}

}  // extern "C"
