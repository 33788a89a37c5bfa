// hip_ann.cpp — C ABI (include/hip_ann.h) over the gfx950 Flat / IVFFlat search kernels.
//
// Reference behaviour mirrored here:
//   MetalIndexFlat::search (faiss-metal/src/MetalIndexFlat.mm:294-369): k <= 0 throws; empty
//     index / empty batch → (±inf, −1); effective_k = min(k, ntotal); labels int64.
//   MetalIndexFlat::add (MetalIndexFlat.mm:173-292): append rows, ‖x‖² computed on the device.
//   faiss_index.cpp:108-149 (EnsureGpuIndex) only needs create/search/free + availability.
#include "../../include/hip_ann.h"
#include "runtime.hpp"
#include "ivf.hpp"

#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>

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

int g_device_count = -1;

int device_count() {
    if (g_device_count < 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        g_device_count = n;
    }
    return g_device_count;
}

void require_device() { HIPANN_REQUIRE(device_count() > 0, "no HIP device"); }

std::vector<int> device_list(const int *devices, int ndev) {
    std::vector<int> v;
    if (!devices || ndev <= 0) v.push_back(0);
    else v.assign(devices, devices + ndev);
    for (int d : v) HIPANN_REQUIRE(d >= 0 && d < device_count(), "invalid device id " + std::to_string(d));
    return v;
}

}  // namespace

namespace hipann {
bool roctx_enabled() {
    static const bool on = [] { const char *e = std::getenv("HIPANN_ROCTX"); return e && std::atoi(e); }();
    return on;
}
void roctx_push(const char *name) { roctxRangePushA(name); }
void roctx_pop() { roctxRangePop(); }

std::vector<int> enable_peer_access(const std::vector<int> &devs) {
    std::vector<int> st(devs.size(), 2);
    if (devs.empty()) return st;
    const int d0 = devs[0];
    auto enable = [](int from, int to) -> bool {  // `from` may access `to`'s memory
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, from, to) != hipSuccess || !can) return false;
        DeviceGuard g(from);
        const hipError_t e = hipDeviceEnablePeerAccess(to, 0);
        if (e == hipErrorPeerAccessAlreadyEnabled) {
            (void)hipGetLastError();  // clear the sticky-free "already enabled" status
            return true;
        }
        return e == hipSuccess;
    };
    for (size_t p = 1; p < devs.size(); ++p) {
        if (devs[p] == d0) continue;
        st[p] = enable(d0, devs[p]) && enable(devs[p], d0) ? 1 : 0;
    }
    return st;
}
}  // namespace hipann

namespace {

hipStream_t make_stream(int dev) {
    DeviceGuard g(dev);
    hipStream_t s;
    HIPANN_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return s;
}

constexpr int kFusedMaxK = 64;   // fused GEMM / scan lists: one element per lane
constexpr int kBlasThreshold = 20;  // FAISS distance_compute_blas_threshold
constexpr int64_t kSmallTable = 16384;  // rows: below this, GEMM keys + per-query selection

// Grow `b` to at least `need` bytes keeping its first `keep` bytes (device-to-device on `st`).
void grow_keep(DevBuf &b, size_t need, size_t keep, int dev, hipStream_t st) {
    if (b.p && need <= b.bytes) return;
    DevBuf nb;
    nb.ensure(need, dev);
    if (b.p && keep) HIPANN_CHECK(hipMemcpyAsync(nb.p, b.p, std::min(keep, b.bytes), hipMemcpyDeviceToDevice, st));
    HIPANN_CHECK(hipStreamSynchronize(st));  // the old buffer is freed on return
    std::swap(b.p, nb.p);
    std::swap(b.bytes, nb.bytes);
    std::swap(b.device, nb.device);
}

float bits_to_float(unsigned u) {
    float v;
    std::memcpy(&v, &u, sizeof(v));
    return v;
}

// Append rows to a shard's owned storage (capacity doubling, as MetalIndexFlat::add does, MetalIndexFlat.mm:255-269).
// The search images built from the rows (int8 / bf16 tiles, per-row int8 scales) grow with the same capacity and
// only the tiles holding new rows are re-tiled; the exact forms' bound terms (max ‖x‖², the largest int8 / bf16 row
// residual) become running maxima over the new rows — an append costs the appended rows, not the table.
void shard_append(FlatShard &sh, int d, int metric, const float *x_host, const float *x_dev, int64_t n) {
    if (n <= 0) return;
    DeviceGuard g(sh.device);
    FenceScope fs(sh.fence, sh.stream, sh.device);  // searches still running on other streams read sh.xb
    hipStream_t st = sh.stream;
    const int64_t n0 = sh.n, need = sh.n + n;
    if (need > sh.cap || !sh.owns) {
        const int64_t cap = std::max<int64_t>(need, std::max<int64_t>(1024, sh.cap * 2));
        DevBuf nb;
        nb.ensure((size_t)cap * d * sizeof(float), sh.device);
        if (sh.n > 0)
            HIPANN_CHECK(hipMemcpyAsync(nb.get<float>(), sh.xb, (size_t)sh.n * d * sizeof(float), hipMemcpyDeviceToDevice,
                                        st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        std::swap(sh.xb_buf.p, nb.p);
        std::swap(sh.xb_buf.bytes, nb.bytes);
        sh.xb_buf.device = sh.device;
        sh.xb = sh.xb_buf.get<float>();
        sh.cap = cap;
        sh.owns = true;
        if (metric == kL2) grow_keep(sh.xn, (size_t)cap * sizeof(float), (size_t)sh.n * sizeof(float), sh.device, st);
    }
    float *dst = sh.xb + n0 * (int64_t)d;
    if (x_host)
        HIPANN_CHECK(hipMemcpyAsync(dst, x_host, (size_t)n * d * sizeof(float), hipMemcpyHostToDevice, st));
    else
        HIPANN_CHECK(hipMemcpyAsync(dst, x_dev, (size_t)n * d * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (metric == kL2) launch_row_norms(dst, n, d, sh.xn.get<float>() + n0, st);
    sh.n = need;
    // the images and bound terms, when built: tiles from the first one holding a new row to the end
    const bool upd = sh.xmax2 >= 0.f || sh.xi8_ok || sh.xb16_ok;
    if (upd) {
        const int R = flat_bf16_tile_rows();
        const int64_t t0 = n0 / R;                  // first tile with a new row (tiles before it are unchanged)
        const int64_t capr = ceil_div(sh.cap, (int64_t)R) * R;
        sh.app_stat.ensure(sizeof(unsigned) * 4, sh.device);
        unsigned *stat = sh.app_stat.get<unsigned>();
        HIPANN_CHECK(hipMemsetAsync(stat, 0, sizeof(unsigned) * 4, st));
        sh.tmpnorm.ensure(sizeof(float) * (size_t)n, sh.device);
        if (sh.xmax2 >= 0.f) {
            const float *xn_new = sh.xn.get<float>() + n0;
            if (metric != kL2) {
                launch_row_norms(dst, n, d, sh.tmpnorm.get<float>(), st);
                xn_new = sh.tmpnorm.get<float>();
            }
            launch_ivf_max_norm(xn_new, n, stat + 0, st);
        }
        if (sh.xi8_ok) {
            const size_t tb = flat_i8_img_bytes(R, d, R);  // one tile
            grow_keep(sh.xi8, flat_i8_img_bytes(capr, d, R), (size_t)t0 * tb, sh.device, st);
            grow_keep(sh.xscale, sizeof(float) * (size_t)capr, sizeof(float) * (size_t)n0, sh.device, st);
            float *rs = sh.tmpnorm.get<float>();
            launch_i8_row_scale(dst, n, d, sh.xscale.get<float>() + n0, rs, st);
            launch_ivf_max_norm(rs, n, stat + 1, st);
            launch_i8_tile_rows(sh.xb + t0 * R * (int64_t)d, sh.xscale.get<float>() + t0 * R, sh.n - t0 * R, d, R,
                                static_cast<char *>(sh.xi8.p) + (size_t)t0 * tb, st);
        }
        if (sh.xb16_ok) {
            const size_t tb = flat_bf16_img_bytes(R, d, R);
            grow_keep(sh.xb16, flat_bf16_img_bytes(capr, d, R), (size_t)t0 * tb, sh.device, st);
            float *rs = sh.tmpnorm.get<float>();
            launch_b16_row_residual2(dst, n, d, rs, st);
            launch_ivf_max_norm(rs, n, stat + 2, st);
            launch_b16_tile_rows(sh.xb + t0 * R * (int64_t)d, sh.n - t0 * R, d, R,
                                 static_cast<char *>(sh.xb16.p) + (size_t)t0 * tb, st);
        }
        unsigned hs[4] = {0u, 0u, 0u, 0u};
        HIPANN_CHECK(hipMemcpyAsync(hs, stat, sizeof(hs), hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        if (sh.xmax2 >= 0.f) sh.xmax2 = std::max(sh.xmax2, bits_to_float(hs[0]));
        if (sh.xi8_ok) sh.i8_rxmax = std::max(sh.i8_rxmax, bits_to_float(hs[1]));
        if (sh.xb16_ok) sh.bf16_rxmax = std::max(sh.bf16_rxmax, std::sqrt(bits_to_float(hs[2])) * 1.0001f);
    } else {
        HIPANN_CHECK(hipStreamSynchronize(st));
    }
}

// faiss::IndexFlatCodes::remove_ids on one shard, in two steps so that a call over several shards changes none of
// them unless every shard's new storage exists.  flat_remove_prepare compacts the rows from the first removed one to
// the end (remove_kernels.hip: keep mask, prefix sum, gather) into FRESH buffers — rows, ‖x‖² and, when the int8
// image is built, its per-row scales: gathered bits equal recomputed ones — and copies the unmoved prefix beside them;
// nothing a search reads has changed when it returns or throws.  flat_remove_commit re-tiles the int8 / bf16 images
// in place from the first 256-row tile holding a moved row (tiles before it stay, as in shard_append) and swaps the
// buffers in; it allocates nothing.  The bound terms (xmax2, i8_rxmax, bf16_rxmax) keep their pre-removal values:
// maxima over a superset of the rows, still upper bounds.  A borrowed table becomes owned, as at its first add.
struct FlatRemoval {
    int64_t m = 0, first = 0, n_new = 0, cap = 0;
    DevBuf xb, xn, xscale;
};

void flat_remove_prepare(FlatShard &sh, int d, int metric, const std::vector<int64_t> &rows, FlatRemoval &rm) {
    rm.m = (int64_t)rows.size();
    if (!rm.m) return;
    DeviceGuard g(sh.device);
    FenceScope fs(sh.fence, sh.stream, sh.device);  // searches still running on other streams read sh.xb
    hipStream_t st = sh.stream;
    const int R = flat_bf16_tile_rows();
    const int64_t first = rows.front(), cnt = sh.n - first, kept = cnt - rm.m;
    rm.first = first;
    rm.n_new = sh.n - rm.m;
    rm.cap = std::max<int64_t>(rm.n_new, 1);
    rm.xb.ensure((size_t)rm.cap * d * sizeof(float), sh.device);
    if (metric == kL2) rm.xn.ensure((size_t)rm.cap * sizeof(float), sh.device);
    if (sh.xi8_ok) rm.xscale.ensure(sizeof(float) * (size_t)(ceil_div(rm.cap, (int64_t)R) * R), sh.device);
    DevBuf d_rows, keep, sums, src;
    d_rows.ensure(sizeof(int64_t) * (size_t)rm.m, sh.device);
    keep.ensure((size_t)cnt, sh.device);
    sums.ensure(sizeof(int64_t) * (size_t)flat_remove_scan_blocks(cnt), sh.device);
    src.ensure(sizeof(int64_t) * (size_t)std::max<int64_t>(kept, 1), sh.device);
    HIPANN_CHECK(hipMemcpyAsync(d_rows.p, rows.data(), sizeof(int64_t) * (size_t)rm.m, hipMemcpyHostToDevice, st));
    launch_flat_remove_plan(d_rows.get<int64_t>(), rm.m, first, cnt, keep.get<unsigned char>(), sums.get<int64_t>(),
                            src.get<int64_t>(), st);
    if (first > 0) {
        HIPANN_CHECK(hipMemcpyAsync(rm.xb.p, sh.xb, (size_t)first * d * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (metric == kL2)
            HIPANN_CHECK(hipMemcpyAsync(rm.xn.p, sh.xn.p, (size_t)first * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (sh.xi8_ok)
            HIPANN_CHECK(hipMemcpyAsync(rm.xscale.p, sh.xscale.p, (size_t)first * sizeof(float), hipMemcpyDeviceToDevice,
                                        st));
    }
    launch_flat_gather_rows(sh.xb + first * (int64_t)d, src.get<int64_t>(), kept, d,
                            rm.xb.get<float>() + first * (int64_t)d, st);
    if (metric == kL2)
        launch_flat_gather_f32(sh.xn.get<float>() + first, src.get<int64_t>(), kept, rm.xn.get<float>() + first, st);
    if (sh.xi8_ok)
        launch_flat_gather_f32(sh.xscale.get<float>() + first, src.get<int64_t>(), kept,
                               rm.xscale.get<float>() + first, st);
    HIPANN_CHECK(hipStreamSynchronize(st));  // the plan's scratch is freed on return
}

void flat_remove_commit(FlatShard &sh, int d, int metric, FlatRemoval &rm) {
    if (!rm.m) return;
    DeviceGuard g(sh.device);
    FenceScope fs(sh.fence, sh.stream, sh.device);
    hipStream_t st = sh.stream;
    const int R = flat_bf16_tile_rows();
    const int64_t t0 = rm.first / R, r0 = t0 * R;  // first tile with a moved row
    try {
        if (sh.xi8_ok && rm.n_new > r0)
            launch_i8_tile_rows(rm.xb.get<float>() + r0 * (int64_t)d, rm.xscale.get<float>() + r0, rm.n_new - r0, d, R,
                                static_cast<char *>(sh.xi8.p) + (size_t)t0 * flat_i8_img_bytes(R, d, R), st);
        if (sh.xb16_ok && rm.n_new > r0)
            launch_b16_tile_rows(rm.xb.get<float>() + r0 * (int64_t)d, rm.n_new - r0, d, R,
                                 static_cast<char *>(sh.xb16.p) + (size_t)t0 * flat_bf16_img_bytes(R, d, R), st);
        HIPANN_CHECK(hipStreamSynchronize(st));
    } catch (...) {  // the rows are still the old ones: the images are rebuilt from them at the next search
        sh.xi8_ok = false;
        sh.xb16_ok = false;
        throw;
    }
    auto take = [](DevBuf &dst, DevBuf &src) {
        std::swap(dst.p, src.p);
        std::swap(dst.bytes, src.bytes);
        std::swap(dst.device, src.device);
    };
    take(sh.xb_buf, rm.xb);  // rm now holds the old storage (nothing, when the table was borrowed): freed with it
    sh.xb = sh.xb_buf.get<float>();
    sh.owns = true;
    sh.cap = rm.cap;
    sh.n = rm.n_new;
    if (metric == kL2) take(sh.xn, rm.xn);
    if (sh.xi8_ok) take(sh.xscale, rm.xscale);
}

// The labels of a removal call as FAISS's IDSelectorBatch sees them: a set (sorted here, duplicates dropped).
std::vector<int64_t> sorted_unique_labels(const int64_t *labels, int64_t n) {
    std::vector<int64_t> v(labels, labels + n);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

template <typename F>
int64_t guard_i64(char *eb, int el, F &&f) {
    try {
        return f();
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return -1;
}

}  // namespace

namespace hipann {

FlatIndex::~FlatIndex() {
    for (auto &s : shards) {
        DeviceGuard g(s->device);
        if (s->done) (void)hipEventDestroy(s->done);
        if (s->stream) (void)hipStreamDestroy(s->stream);
    }
}

// k > 64: distance keys for a column chunk into HBM (GEMM or direct scan, same forms as the fused
// path), per-(row, segment) S-slot wave lists, and a running merge across chunks.
static void flat_shard_search_bigk(FlatIndex &ix, FlatShard &sh, int64_t nq, const float *xq, const float *qn, int k,
                                   int kout, float *D, int64_t *I, hipStream_t st) {
    const int d = ix.d, metric = ix.metric;
    const float out_sign = metric == kIP ? -1.f : 1.f;
    const int64_t budget = (int64_t)256 << 20;  // bytes of keys per chunk
    int64_t C = std::max<int64_t>(1024, budget / (4 * std::max<int64_t>(nq, 1)));
    C = std::min<int64_t>(C, sh.n);
    C = (C + 127) / 128 * 128;
    const int64_t seg_len = 8192;
    const int nseg = (int)ceil_div(C, seg_len);
    sh.keys.ensure((size_t)nq * C * sizeof(float), sh.device);
    sh.part_d.ensure((size_t)(nseg + 1) * nq * k * sizeof(float), sh.device);
    sh.part_i.ensure((size_t)(nseg + 1) * nq * k * sizeof(int), sh.device);
    if (sh.n <= C) {  // one chunk (an IVF coarse quantizer): the segment lists go straight to the output merge
        {
            ScopedTiming t(ix.timer_main, st);
            if (nq < kBlasThreshold)
                launch_flat_scan_keys(xq, (int)nq, sh.xb, sh.n, d, metric, sh.keys.get<float>(), C, st);
            else
                launch_flat_gemm_keys(xq, qn, nq, sh.xb, sh.xn.get<float>(), sh.n, d, metric, sh.keys.get<float>(), C,
                                      st, sh.keys_bf3);
        }
        {  // kout ≤ 256: one wave selects the whole row and writes the output (no segment lists, no merge)
            ScopedTiming t(ix.timer_merge, st);
            // (short rows only: a long row would be one wave's serial inserts — the segment path spreads it)
            if (sh.n <= kSmallTable && launch_rows_select_out(sh.keys.get<float>(), C, sh.n, nq, k, kout,
                                                              sh.label_offset, out_sign, D, I, st, sh.plan_hook))
                return;
        }
        // short rows: 256-column segments, so a 1024-centroid row is selected by 4 waves, not 1
        const int64_t sl = sh.n <= seg_len && k <= 64 ? 256 : seg_len;
        const int ns = (int)ceil_div(sh.n, sl);
        sh.part_d.ensure((size_t)ns * nq * k * sizeof(float), sh.device);
        sh.part_i.ensure((size_t)ns * nq * k * sizeof(int), sh.device);
        launch_rows_topk(sh.keys.get<float>(), C, sh.n, nq, sl, ns, k, 0, sh.part_d.get<float>(), sh.part_i.get<int>(),
                         st);
        ScopedTiming t(ix.timer_merge, st);
        launch_merge_parts<int>(sh.part_d.get<float>(), sh.part_i.get<int>(), ns, nq, k, kout, sh.label_offset, 1.f,
                                out_sign, D, I, st);
        return;
    }
    sh.run_d.ensure((size_t)nq * k * sizeof(float), sh.device);
    sh.run_i.ensure((size_t)nq * k * sizeof(int), sh.device);
    // running best starts empty: part 0 = pads
    HIPANN_CHECK(hipMemsetAsync(sh.part_i.p, 0xff, (size_t)nq * k * sizeof(int), st));
    for (int64_t c0 = 0; c0 < sh.n; c0 += C) {
        const int64_t cn = std::min<int64_t>(C, sh.n - c0);
        {
            ScopedTiming t(ix.timer_main, st);
            if (nq < kBlasThreshold)
                launch_flat_scan_keys(xq, (int)nq, sh.xb + c0 * d, cn, d, metric, sh.keys.get<float>(), C, st);
            else
                launch_flat_gemm_keys(xq, qn, nq, sh.xb + c0 * d, sh.xn.get<float>() + c0, cn, d, metric,
                                      sh.keys.get<float>(), C, st);
        }
        const int ns = (int)ceil_div(cn, seg_len);
        launch_rows_topk(sh.keys.get<float>(), C, cn, nq, seg_len, ns, k, (int)c0,
                         sh.part_d.get<float>() + (size_t)nq * k, sh.part_i.get<int>() + (size_t)nq * k, st);
        // merge [running best, ns segment partials] → running best (then back into part 0)
        launch_merge_raw(sh.part_d.get<float>(), sh.part_i.get<int>(), ns + 1, nq, k, sh.run_d.get<float>(),
                         sh.run_i.get<int>(), st);
        HIPANN_CHECK(hipMemcpyAsync(sh.part_d.p, sh.run_d.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToDevice, st));
        HIPANN_CHECK(hipMemcpyAsync(sh.part_i.p, sh.run_i.p, (size_t)nq * k * sizeof(int), hipMemcpyDeviceToDevice, st));
    }
    ScopedTiming t(ix.timer_merge, st);
    launch_merge_parts<int>(sh.run_d.get<float>(), sh.run_i.get<int>(), 1, nq, k, kout, sh.label_offset, 1.f, out_sign,
                            D, I, st);
}

// ---- the Flat shard search: its switches, the mode a call resolves to ("Flat scan modes", has the
// table), then the stages of flat_shard_launch in their order on the stream ----

// The A/B switches of the shard search, read from the environment once (flat_tuning) and passed by value into the
// resolver and the planner.  The defaults are the product's paths.
struct FlatTuning {
    int passes = 0;             // HIPANN_FLAT_PASSES: pins the bounded passes' count P (0: flat_pass_plan's choice)
    bool i8_small = true;       // HIPANN_FLAT_I8_SMALL=0: every nq < 20 call stays on the fp32 scan
    bool seed = true;           // HIPANN_FLAT_BF16_SEED=0: no seed bound on large tables, so no bounded passes
    bool i8_prep_fused = true;  // HIPANN_I8_PREP_FUSED=0: the int8 queries by row_norms + i8_row_scale + i8_tile_rows
    int64_t blocks = 0;         // HIPANN_FLAT_BF16_BLOCKS: target grid size of the image scans (0: one resident round)
    int64_t pass_a = -1;        // HIPANN_FLAT_PASS_A: two passes, 1/x of each split in pass A (< 0: flat_pass_plan)
    int64_t sample = 16384;     // HIPANN_FLAT_SAMPLE: rows of the seed sample (multiple of 256)
    bool cand_debug = false;    // HIPANN_FLAT_CAND_DEBUG (set): the candidate buffers' fill and the flagged queries to stderr
    bool b16_k64 = true;        // HIPANN_B16_K64=0: one pass of the 32-dim list kernel in place of the bounded passes
};

static const FlatTuning &flat_tuning() {
    static const FlatTuning t = [] {
        auto num = [](const char *name, long long dflt) {
            const char *e = std::getenv(name);
            return e ? std::atoll(e) : dflt;
        };
        FlatTuning v;
        v.passes = (int)num("HIPANN_FLAT_PASSES", 0);
        v.i8_small = num("HIPANN_FLAT_I8_SMALL", 1) != 0;
        v.seed = num("HIPANN_FLAT_BF16_SEED", 1) != 0;
        v.i8_prep_fused = num("HIPANN_I8_PREP_FUSED", 1) != 0;
        v.blocks = num("HIPANN_FLAT_BF16_BLOCKS", 0);
        v.pass_a = num("HIPANN_FLAT_PASS_A", -1);
        v.sample = num("HIPANN_FLAT_SAMPLE", 16384);
        v.cand_debug = std::getenv("HIPANN_FLAT_CAND_DEBUG") != nullptr;
        v.b16_k64 = num("HIPANN_B16_K64", 1) != 0;
        return v;
    }();
    return t;
}

enum FlatPath : int {
    kFlatPathNone = 0,     // no queries: nothing is written
    kFlatPathPads = 1,     // no rows: pads only
    kFlatPathKeys = 2,     // the key matrix + per-row selection (flat_shard_search_bigk)
    kFlatPathSmallI8 = 3,  // nq <= 16 on a large table: the int8 image's scan, 64 candidates, exact rerank
    kFlatPathDirect = 4,   // nq < 20: the fp32 direct scan
    kFlatPathLists = 5,    // per-split lists: the fp32 / 2-term / 3-term GEMM lists or (form 4) the bf16 list kernel
    kFlatPathBounded = 6   // the bounded passes over the bf16 or int8 image
};

// Everything flat_resolve_mode reads; no pointer, no shard, no environment.
struct FlatModeIn {
    int64_t nq = 0, n = 0;
    int d = 0, metric = kL2, k = 0, kout = 0;
    int form = kFlatI8Exact;   // the requested form (FlatForm)
    bool is_override = false;  // ... from the caller (a flagged query's re-run), not the index
    FlatTuning tune;
};

// What a call resolves to.  Every field is set once, here; a stage that needs one reads it.
struct FlatScanMode {
    int path = kFlatPathNone;
    int form = kFlatFp32;            // the scan that runs (paths Lists and Bounded; SmallI8: kFlatI8Exact)
    bool record = false;             // the index's last_* is written (never by an override call or the Keys path) ...
    int last_form = kFlatFp32, last_kfilt = 0;  // ... with these
    bool exact = false;              // a filter of kscan candidates + the exact direct-form rerank
    bool bounded = false, seeded = false;  // the bounded passes; a seed bound from a sample of the first rows
    bool i8 = false, i8_prep = false;      // the int8 image filters; its queries by the fused preparation
    int kscan = 0, k_user = 0;       // the scan's depth (kf on the exact forms), the caller's k (the re-run's)
    int pend_kind = FlatPending::kNone, rerun_form = kFlatSplit3;  // what flat_shard_finish has left to do, on which form
    bool need_qn = false;            // the path reads ‖q‖² ...
    bool prep_qn = false;            // ... and the int8 query preparation writes it (no row_norms launch)
    bool image() const { return form == kFlatBf16Exact || form == kFlatI8Exact; }
};

constexpr int64_t kFlatSeedMinRows = 8 * 65536;  // tables from here on get a seed bound (and may run bounded)
constexpr int64_t kFlatI8SmallMinRows = 65536;

// The exact forms' filter depth kf (0: not an exact form) and whether the form runs as the bounded passes.
// kout ≤ kRerankMaxK: kf = 32 (the bf16 image: at 10M × 768 the 10th and 16th distances are ≈2 apart, inside its
// rounding bound ≈1.3, the 10th and 32nd ≈5; the split scan: IP 32, L2 16).  Larger kout (request_k = k +
// |tombstones|, faiss_index.cpp:713-715): kf = min(64, max(base, 2·kout)).  The list kernels hold kf in LDS (capped
// by their launchers' LDS budget); the bounded passes take any kf ≤ 64.  The int8 rounding bound is ≈3× the bf16 one
// (E ≈ 4.4 against 1.3-1.7 at 768 dims on U(-1, 1)): a 64-deep filter keeps the 10th distance clear of it (the
// 10th-to-32nd gap is ≈5, the 10th-to-64th ≈8).
static int flat_filter_depth(const FlatModeIn &in, int form, bool sampled, bool *bounded) {
    *bounded = form == kFlatI8Exact;
    if (form == kFlatI8Exact) return 64;
    if (form != kFlatSplit2Exact && form != kFlatBf16Exact) return 0;
    const int base = in.metric == kIP || form == kFlatBf16Exact ? kFlatRerankKIP : kRerankK;
    const int kf = in.kout <= kRerankMaxK ? base : std::min(64, std::max(base, 2 * in.kout));
    if (form == kFlatSplit2Exact) return std::min(kf, flat_gemm_topk_bf_kmax(2));
    *bounded = flat_bf16_resumable(in.nq, in.d, kf, in.tune.b16_k64) && sampled;
    return *bounded ? kf : std::min(kf, flat_bf16_topk_kmax(in.nq));
}

FlatScanMode flat_resolve_mode(const FlatModeIn &in) {
    FlatScanMode m;
    const int64_t nq = in.nq, n = in.n;
    const int d = in.d, k = in.k, kout = in.kout;
    m.kscan = m.k_user = k;
    if (nq <= 0) return m;
    if (n == 0) {
        m.path = kFlatPathPads;
        return m;
    }
    // Large k, or a small table (an IVF coarse quantizer: nq x nlist keys are a few MB): the GEMM writes the key
    // matrix and one wave per query selects — the fused epilogue would spend its time filling empty lists, one query
    // tile per CU.  nq < 20 on a table of ≤ 1024 rows (the coarse quantizer of the extension's nq = 1 call):
    // direct-form keys over ≥ 16-row waves + one bitwise select per query row (the fused scan's nparts × k partial
    // lists took one wave 47 µs to merge at nlist 1024).  This path leaves last_* as it was.
    if (k > kFusedMaxK || (nq >= kBlasThreshold && n <= kSmallTable) ||
        (nq < kBlasThreshold && n <= 1024 && kout <= 64 && scan_smem_bytes((int)nq, d) <= 64 * 1024)) {
        m.path = kFlatPathKeys;
        m.need_qn = nq >= kBlasThreshold && in.metric == kL2;
        return m;
    }
    m.record = !in.is_override;
    // nq < 20 on a large table (the extension's per-query calls, faiss_index.cpp:737): form 5's int8 image as the
    // filter — flat_i8_scan (a quarter of the fp32 rows' bytes), 64 candidates per query, the exact direct-form
    // rerank with the int8 residual bound; queries it cannot certify re-run on the fp32 direct scan.
    if (nq <= flat_i8_scan_max_nq() && in.form == kFlatI8Exact && in.tune.i8_small && n >= kFlatI8SmallMinRows &&
        d <= 1024 && kout <= flat_i8_scan_k() && k <= flat_i8_scan_k()) {
        m.path = kFlatPathSmallI8;
        m.form = m.last_form = kFlatI8Exact;
        m.exact = m.i8 = true;
        m.kscan = m.last_kfilt = flat_i8_scan_k();
        m.pend_kind = FlatPending::kSmallI8;
        m.rerun_form = kFlatFp32;
        m.need_qn = in.metric == kL2;
        return m;
    }
    if (nq < kBlasThreshold) {  // the direct form (fvec_L2sqr / fvec_inner_product)
        m.path = kFlatPathDirect;
        return m;
    }
    // BLAS form: ‖q‖² + ‖x‖² − 2 q·x on the matrix cores.  kFlatI8Exact runs only as the bounded passes (256-query
    // blocks, >= 512K rows, d <= 1024 so the int32 sums convert to fp32 exactly); elsewhere the bf16 image's paths.
    const bool sampled = in.tune.seed && n >= kFlatSeedMinRows;
    const int want = in.form == kFlatI8Exact &&
                             !(flat_bf16_resumable(nq, d, 64, in.tune.b16_k64) && sampled && d <= 1024)
                         ? kFlatBf16Exact : in.form;
    bool bounded = false;
    const int kf = flat_filter_depth(in, want, sampled, &bounded);
    // the list kernels need kf ≥ kout + 4 of margin; the bounded passes take any kout ≤ kf — a query whose kout-th
    // distance is within the bound of the kf-th key goes to the all-candidate rerank, certified against the pass
    // bound.  Otherwise: the 3-term split (fp32-level).
    m.exact = kf > 0 && (kout <= kRerankMaxK || (bounded ? kout <= kf : kout + 4 <= kf));
    m.kscan = m.exact ? kf : k;
    const int lists = kf > 0 && !m.exact ? kFlatSplit3 : want;
    // the split scans' LDS lists hold fewer rows at 3 terms (k <= 56 at 8 waves): a longer list takes the fp32
    // matrix cores (exact fp32 products, lists up to 64)
    const bool too_deep = (lists == kFlatSplit3 || lists == kFlatSplit2) &&
                          m.kscan > flat_gemm_topk_bf_kmax(lists == kFlatSplit3 ? 3 : 2);
    m.form = m.last_form = too_deep ? kFlatFp32 : lists;
    m.last_kfilt = m.exact ? kf : 0;
    m.bounded = m.exact && bounded;
    m.seeded = m.image() && sampled;
    m.i8 = m.form == kFlatI8Exact;
    m.i8_prep = m.i8 && in.tune.i8_prep_fused;
    m.path = m.bounded ? kFlatPathBounded : kFlatPathLists;
    if (m.exact) m.pend_kind = FlatPending::kExact;  // flagged queries re-run on the 3-term split
    m.need_qn = in.metric == kL2;
    m.prep_qn = m.need_qn && m.i8_prep;
    return m;
}

// max over n non-negative floats on the device, on the host (their bit patterns order as the values): one launch into
// the scratch word sh.nflag (so before any flags), a 4-byte readback and a host synchronisation, counted — later
// searches may run on other streams.  sh.tmpnorm, where the callers put the values, is released.
static float device_max_to_host(FlatIndex &ix, FlatShard &sh, const float *v, int64_t n, hipStream_t st) {
    sh.nflag.ensure(sizeof(int), sh.device);
    launch_ivf_max_norm(v, n, sh.nflag.get<unsigned>(), st);
    unsigned bits = 0;
    HIPANN_CHECK(hipMemcpyAsync(&bits, sh.nflag.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));
    ++ix.host_syncs;
    sh.tmpnorm.release();
    return bits_to_float(bits);
}

// The shard's tiled int8 image (form kFlatI8Exact): per-row scales max|x|/127, the rows' int8 units in the bf16
// image's tile geometry, and the largest row residual ‖x − s·x̂‖ (the rerank bound's row term).  Built once.
static void ensure_i8_image(FlatIndex &ix, FlatShard &sh, int d, hipStream_t st) {
    if (sh.xi8_ok) return;
    sh.xi8.ensure(flat_i8_img_bytes(sh.n, d, flat_bf16_tile_rows()), sh.device);
    sh.xscale.ensure(sizeof(float) * (size_t)sh.n, sh.device);
    sh.tmpnorm.ensure(sizeof(float) * (size_t)sh.n, sh.device);
    launch_i8_row_scale(sh.xb, sh.n, d, sh.xscale.get<float>(), sh.tmpnorm.get<float>(), st);
    launch_i8_tile_rows(sh.xb, sh.xscale.get<float>(), sh.n, d, flat_bf16_tile_rows(), sh.xi8.p, st);
    sh.i8_rxmax = device_max_to_host(ix, sh, sh.tmpnorm.get<float>(), sh.n, st);
    sh.xi8_ok = true;
}

// The shard's tiled bf16 image (flat_bf16.hip: one plain bf16 product per element) and the rows' largest bf16
// rounding residual ‖x̂ − x‖ (the rerank's bound).  Built once.
static void ensure_b16_image(FlatIndex &ix, FlatShard &sh, int d, hipStream_t st) {
    if (sh.xb16_ok) return;
    sh.xb16.ensure(flat_bf16_img_bytes(sh.n, d, flat_bf16_tile_rows()), sh.device);
    launch_b16_tile_rows(sh.xb, sh.n, d, flat_bf16_tile_rows(), sh.xb16.p, st);
    sh.tmpnorm.ensure(sizeof(float) * (size_t)sh.n, sh.device);
    launch_b16_row_residual2(sh.xb, sh.n, d, sh.tmpnorm.get<float>(), st);
    sh.bf16_rxmax = std::sqrt(device_max_to_host(ix, sh, sh.tmpnorm.get<float>(), sh.n, st)) * 1.0001f;
    sh.xb16_ok = true;
}

// max‖x‖² of the shard (once per row set): the exact form's error bound
static float flat_xmax2(FlatIndex &ix, FlatShard &sh, int d, hipStream_t st) {
    if (sh.xmax2 >= 0.f) return sh.xmax2;
    const float *xn = sh.xn.get<float>();
    if (!xn) {
        sh.tmpnorm.ensure(sizeof(float) * (size_t)std::max<int64_t>(sh.n, 1), sh.device);
        launch_row_norms(sh.xb, sh.n, d, sh.tmpnorm.get<float>(), st);
        xn = sh.tmpnorm.get<float>();
    }
    sh.xmax2 = device_max_to_host(ix, sh, xn, sh.n, st);
    return sh.xmax2;
}

// ‖q‖² of the batch in sh.qn, and the shard's note of whose they are (qn_of / qn_nq: the IVF scan reads them
// afterwards).  The caller may have prepared them (qn_given: nothing to launch).  With `owed` the launch is left to
// the int8 query preparation, which writes *owed (nullptr: nothing owed).
static const float *flat_query_norms(FlatShard &sh, int64_t nq, const float *xq, int d, hipStream_t st,
                                     float **owed = nullptr) {
    const bool given = sh.qn_given == xq && sh.qn_given_nq == nq;
    if (!given) sh.qn.ensure((size_t)nq * sizeof(float), sh.device);
    if (owed) *owed = given ? nullptr : sh.qn.get<float>();
    else if (!given) launch_row_norms(xq, nq, d, sh.qn.get<float>(), st);
    sh.qn_of = xq;
    sh.qn_nq = nq;
    return sh.qn.get<float>();
}

// The bounded passes' plan: tile boundaries 0 = b₀ < b₁ < … < b_P = tps within every split.  Pass 0 admits the
// rows under the seed (the k-th of S sample keys): ≈ k·(b₁·nsplit·rows)/S candidates per query; pass p ≥ 1 runs
// under the k-th over every earlier row: ≈ k·(b_{p+1} − b_p)/b_p.  Every candidate costs a scattered store and
// the epilogue's slow path (measured ≈ 0.54 µs per candidate per query per 1024-query batch: C2 and 10M pass-A
// sweeps, profiles/r04/passa_sweep_r04.txt), every pass ≈ 55 µs (its pipeline fill + the bound kernel), so P and
// geometric boundaries b_p ≈ (S/(nsplit·rows))·g^p, g = (N/S)^{1/P}, minimise candidates·nq·0.54 ns + P·55 µs.
// forced > 0 pins P (FlatTuning::passes, A/B).
static std::vector<int64_t> flat_pass_plan(int64_t tps, int64_t nsplit, int64_t tile_rows, int64_t sample, int k,
                                           int64_t nq, int forced) {
    const double unit = (double)sample / ((double)nsplit * (double)tile_rows);  // the sample in tiles per split
    std::vector<int64_t> best{0, tps};
    double best_cost = 1e300;
    for (int P = 1; P <= 6; ++P) {
        if (forced > 0 && P != forced) continue;
        std::vector<int64_t> b{0};
        const double g = std::pow((double)tps / unit, 1.0 / P);
        for (int p = 1; p < P; ++p) {
            const int64_t t = std::llround(unit * std::pow(g, p));
            if (t > b.back() && t < tps) b.push_back(t);
        }
        b.push_back(tps);
        if ((int)b.size() != P + 1) continue;  // too few tiles for P passes
        double cand = k * (double)b[1] / unit;
        for (size_t p = 1; p + 1 < b.size(); ++p) cand += k * (double)(b[p + 1] - b[p]) / (double)b[p];
        const double cost = cand * (double)nq * 0.54e-9 + P * 55e-6;
        if (cost < best_cost) { best_cost = cost; best = b; }
    }
    return best;
}

// Per-(query, split) candidate capacity of a plan pb from its expected fill: pass 0 admits ≈ k·rows₀/S per cell
// (keys ≤ the k-th of S sample rows), pass p ≈ k·rows_p/(nsplit·rows_<p) (the k-th over all earlier rows); 3× + 32
// of headroom (clustered 12.5M IP rows peaked at 2.3× the mean), a multiple of 32, at most 2²⁰.
static int flat_pass_cap(const std::vector<int64_t> &pb, int64_t nsplit, int64_t tile_rows, int64_t sample, int k) {
    double fill = k * (double)(pb[1] * tile_rows) / (double)sample;
    for (size_t p = 1; p + 1 < pb.size(); ++p)
        fill += k * (double)(pb[p + 1] - pb[p]) / ((double)pb[p] * (double)nsplit);
    return (int)std::min<double>(1 << 20, (double)ceil_div((int64_t)(3.0 * fill + 32.0), 32) * 32);
}

// The flag count of the launch phase's bound check into the shard's pinned host word (a copy kernel through its
// device mapping, no DMA round trip), then a fresh token into the word after it; the host reads the count after
// its next synchronisation with `st` (or once the token arrives, wait_posted).
static void flag_readback(FlatShard &sh, hipStream_t st) {
    if (sh.h_nflag.ensure(2 * sizeof(unsigned), hipHostMallocCoherent)) sh.h_nflag.get<unsigned>()[1] = sh.flag_seq;
    launch_post_words(sh.nflag.p, sh.h_nflag.p, 1, ++sh.flag_seq, st);
}

// One call of flat_shard_launch: its arguments, the resolved mode and what the stages hand on.
struct FlatCall {
    FlatIndex &ix;
    FlatShard &sh;
    const int64_t nq;
    const float *const xq;
    const int kout;
    float *const D;
    int64_t *const I;
    const hipStream_t st;
    const FlatTuning tune;
    const FlatScanMode m;
    const int d, metric;
    const float out_sign;
    const float *qn = nullptr;  // ‖q‖² (L2), or nullptr
    float *qn_owed = nullptr;   // ... still to be written, by the int8 query preparation
    float xmax2 = 0.f;          // the exact forms' max ‖x‖²
    float rxmax = -1.f;         // the rerank bound's row term of the image that filtered (−1: the 2-term split's eps)
    int W = 0;                  // the image scans' waves per block (32 queries each)
    int64_t nqt = 0, nsplit = 0, tps = 0;  // query tiles, column splits, row tiles per split
};

// What the scan stage leaves in part_d / part_i for the merge or the rerank, and, from the bounded passes, the
// candidate buffers and pass bound for the flagged queries' second rerank (flat_shard_finish).
struct FlatCandRun {
    int lists = 0;             // lists per query, m.kscan entries each
    bool flags_reset = false;  // nflag is zeroed and the overflowed queries are flagged already
    const float *cd = nullptr, *bound = nullptr;
    const int *ci = nullptr, *cn = nullptr;
    int nsplit = 0, cap = 0;
};

// The exact Flat forms' rerank over the shard's rows (ivf_rerank_topk, slot lists query-major): the caller adds the
// lists (pd, pi, nprobe = lists per query) and the filter depth k.
static IvfRerankArgs flat_rerank_args(const FlatCall &c) {
    FlatShard &sh = c.sh;
    IvfRerankArgs a;
    a.nq = c.nq, a.kout = c.kout, a.metric = c.metric, a.Q = c.xq, a.codes = sh.xb, a.d = c.d, a.nrows = sh.n;
    a.label_offset = sh.label_offset, a.xmax2 = c.xmax2, a.D = c.D, a.I = c.I;
    a.nflag = sh.nflag.get<int>(), a.flagged = sh.flagged.get<int>();
    // (int8: the row term and each query's own residual from the int8 images; qres makes the rerank read them)
    a.rxmax = c.rxmax, a.qres = c.m.i8 ? sh.qres.get<float>() : nullptr;
    return a;
}

static void flat_reset_flags(FlatCall &c) {
    c.sh.nflag.ensure(sizeof(int), c.sh.device);
    c.sh.flagged.ensure(sizeof(int) * (size_t)c.nq, c.sh.device);
    HIPANN_CHECK(hipMemsetAsync(c.sh.nflag.p, 0, sizeof(int), c.st));
}

// Path SmallI8: the int8 image and max ‖x‖² (built once), ‖q‖², flat_i8_scan's per-wave lists merged to G groups of
// 64 per query, the rerank.
static void flat_small_i8(FlatCall &c) {
    FlatShard &sh = c.sh;
    const int64_t nq = c.nq;
    const int kf = c.m.kscan;
    ensure_i8_image(c.ix, sh, c.d, c.st);
    c.xmax2 = flat_xmax2(c.ix, sh, c.d, c.st);
    c.rxmax = sh.i8_rxmax;
    if (c.m.need_qn) c.qn = flat_query_norms(sh, nq, c.xq, c.d, c.st);
    const int64_t nw = flat_i8_scan_waves(sh.n);
    const int G = (int)std::min<int64_t>(64, nw);
    sh.qscale.ensure(sizeof(float) * (size_t)nq, sh.device);
    sh.qres.ensure(sizeof(float) * (size_t)nq, sh.device);
    sh.qimg.ensure((size_t)nq * flat_i8_nk(c.d) * 4 * 16, sh.device);
    sh.part_d.ensure((size_t)nw * nq * kf * sizeof(float), sh.device);
    sh.part_i.ensure((size_t)nw * nq * kf * sizeof(int), sh.device);
    sh.mid_d.ensure((size_t)G * nq * kf * sizeof(float), sh.device);
    sh.mid_i.ensure((size_t)G * nq * kf * sizeof(long long), sh.device);
    {
        ScopedTiming t(c.ix.timer_main, c.st);
        launch_flat_i8_scan(c.xq, nq, c.d, c.metric, sh.xi8.p, sh.xscale.get<float>(), sh.xn.get<float>(), sh.n,
                            sh.qscale.get<float>(), sh.qres.get<float>(), c.qn, sh.qimg.p, sh.part_d.get<float>(),
                            sh.part_i.get<int>(), nw, c.st);
    }
    flat_reset_flags(c);
    ScopedTiming t(c.ix.timer_merge, c.st);
    float *md = sh.mid_d.get<float>();
    int *mi = reinterpret_cast<int *>(sh.mid_i.p);
    launch_flat_i8_group_merge(sh.part_d.get<float>(), sh.part_i.get<int>(), (int)nw, (int)nq, G, md, mi, c.st);
    IvfRerankArgs a = flat_rerank_args(c);
    a.pd = md, a.pi = mi, a.nprobe = G, a.k = kf;
    launch_ivf_rerank(a, c.st);
}

// Path Direct (fvec_L2sqr / fvec_inner_product): per-wave lists, merged per query.
static void flat_direct_scan(FlatCall &c) {
    FlatShard &sh = c.sh;
    const int64_t nq = c.nq;
    const int d = c.d, k = c.m.kscan, kout = c.kout;
    // ≥ 512 rows per wave on large tables; small ones (the IVF coarse quantizer's 1024 centroids at
    // nq = 1) are spread over waves of ≥ 16 rows (2 waves of 512 rows took 234 us for 1024 × 768)
    const int64_t want = std::min<int64_t>(8192, std::max<int64_t>(std::min<int64_t>(256, ceil_div(sh.n, 16)),
                                                                     ceil_div(sh.n, 512)));
    const int64_t rpw = ceil_div(sh.n, want);
    const int64_t nw_alloc = ceil_div(ceil_div(sh.n, rpw), 4) * 4;
    // the scan holds its queries in ≤ 64 KiB of LDS: larger d·nq runs as several query chunks (d = 1536 fits 10
    // queries; one query up to d = 16384)
    int qc = (int)nq;
    while (qc > 1 && scan_smem_bytes(qc, d) > 64 * 1024) --qc;
    HIPANN_REQUIRE(scan_smem_bytes(qc, d) <= 64 * 1024, "dimension too large for the scan path");
    sh.part_d.ensure((size_t)nw_alloc * qc * k * sizeof(float), sh.device);
    sh.part_i.ensure((size_t)nw_alloc * qc * k * sizeof(int), sh.device);
    const int groups = (int)std::min<int64_t>(256, ceil_div(nw_alloc, 32));
    if (nw_alloc > 256) {
        sh.mid_d.ensure(sizeof(float) * (size_t)groups * qc * kout, sh.device);
        sh.mid_i.ensure(sizeof(long long) * (size_t)groups * qc * kout, sh.device);
    }
    for (int64_t q0 = 0; q0 < nq; q0 += qc) {
        const int64_t nc = std::min<int64_t>(qc, nq - q0);
        {
            ScopedTiming t(c.ix.timer_main, c.st);
            launch_flat_scan_topk(c.xq + q0 * d, (int)nc, sh.xb, sh.n, d, c.metric, k, (int)nw_alloc, rpw,
                                  sh.part_d.get<float>(), sh.part_i.get<int>(), c.st);
        }
        ScopedTiming t(c.ix.timer_merge, c.st);
        if (nw_alloc > 256) {
            // thousands of per-wave lists: groups of ~32 merged by one wave each, then the group lists by one
            // 4-wave block per query (one wave per query took ~1 ms for 8192 lists at 10M rows, nq = 1)
            launch_merge_parts_2level<int>(sh.part_d.get<float>(), sh.part_i.get<int>(), (int)nw_alloc, nc, k, kout,
                                           sh.label_offset, 1.f, c.out_sign, c.D + q0 * kout, c.I + q0 * kout,
                                           sh.mid_d.get<float>(), sh.mid_i.get<long long>(), groups, c.st);
        } else {
            launch_merge_parts<int>(sh.part_d.get<float>(), sh.part_i.get<int>(), (int)nw_alloc, nc, k, kout,
                                    sh.label_offset, 1.f, c.out_sign, c.D + q0 * kout, c.I + q0 * kout, c.st);
        }
    }
}

// The exact forms' bound terms: max ‖x‖² (cached; its first computation uses sh.nflag as scratch, so before any
// flags), the int8 image (one int8 product per element, int32 sums, per-row scales; built once) and the row residual
// of the image that filters.  The bf16 term is read here, ahead of the image's first build, as it always was: the
// first bf16 search of a row set reranks with the value from before the build.
static void flat_bound_terms(FlatCall &c) {
    if (!c.m.exact) return;
    c.xmax2 = flat_xmax2(c.ix, c.sh, c.d, c.st);
    if (c.m.i8) ensure_i8_image(c.ix, c.sh, c.d, c.st);
    c.rxmax = c.m.i8 ? c.sh.i8_rxmax : c.m.form == kFlatBf16Exact ? c.sh.bf16_rxmax : -1.f;
}

// Column splits of a table of n rows in tiles of tile_rows for about `blocks` blocks over nqt query tiles: whole
// tiles per split, no empty split.  round8 (the GEMM lists): a multiple of 8 splits before the tiles are dealt out.
struct FlatSplit {
    int64_t nsplit, tps;
};
static FlatSplit flat_split_geometry(int64_t blocks, int64_t nqt, int64_t n, int64_t tile_rows, bool round8) {
    const int64_t ntiles = ceil_div(n, tile_rows);
    const int64_t fit = std::min<int64_t>(std::max<int64_t>(1, ceil_div(blocks, nqt)), ntiles);
    const int64_t tps = ceil_div(ntiles, round8 && fit >= 8 ? fit / 8 * 8 : fit);
    const int64_t nsplit = ceil_div(ntiles, tps);
    HIPANN_REQUIRE(nqt * nsplit < (int64_t)0x7fffffff, "grid too large");
    return {nsplit, tps};
}

// The lists' geometry and scratch.  Image scans: one round of resident blocks (W = 8 / 4: one block per CU; W = 2:
// two) — fewer, longer splits admit fewer candidates into the per-split lists (≈ k·ln(rows / k) per list), the
// epilogue's slow path.  GEMM lists: ≈2048 blocks; small tables (an IVF coarse quantizer: 1024 centroids = 8 tiles)
// go down to one column tile per block rather than leaving CUs idle.
static void flat_lists_scratch(FlatCall &c) {
    FlatShard &sh = c.sh;
    FlatSplit s;
    if (c.m.image()) {
        c.W = flat_bf16_waves(c.nq);
        c.nqt = ceil_div(c.nq, 32 * c.W);
        s = flat_split_geometry(c.tune.blocks > 0 ? c.tune.blocks : (c.W == 2 ? 512 : 256), c.nqt, sh.n,
                                flat_bf16_tile_rows(), false);
        sh.qimg.ensure(c.m.i8 ? flat_i8_img_bytes(c.nq, c.d, 32 * c.W) : flat_bf16_img_bytes(c.nq, c.d, 32 * c.W),
                       sh.device);
    } else {
        c.nqt = ceil_div(c.nq, 128);
        s = flat_split_geometry(2048, c.nqt, sh.n, 128, true);
    }
    c.nsplit = s.nsplit, c.tps = s.tps;
    sh.part_d.ensure((size_t)c.nsplit * c.nq * c.m.kscan * sizeof(float), sh.device);
    sh.part_i.ensure((size_t)c.nsplit * c.nq * c.m.kscan * sizeof(int), sh.device);
}

static FlatCandRun flat_lists_run(const FlatCall &c) {
    FlatCandRun r;
    r.lists = (int)c.nsplit;
    return r;
}

// GEMM lists: fp32 matrix cores, or the 2- / 3-term split-bf16 products (query-major lists for the rerank).
static FlatCandRun flat_gemm_lists(FlatCall &c) {
    FlatShard &sh = c.sh;
    const int k = c.m.kscan;
    if (c.m.form == kFlatFp32) {
        launch_flat_gemm_topk(c.xq, c.qn, c.nq, sh.xb, sh.xn.get<float>(), sh.n, c.d, c.metric, k, (int)c.nsplit, c.tps,
                              sh.part_d.get<float>(), sh.part_i.get<int>(), c.st);
    } else {
        const int np = c.m.form == kFlatSplit3 ? 3 : 2;
        sh.qsplit.ensure(flat_bf_qsplit_bytes(c.nq, c.d, np), sh.device);
        launch_flat_gemm_topk_bf(np, c.xq, c.qn, c.nq, sh.qsplit.get<void>(), sh.xb, sh.xn.get<float>(), sh.n, c.d,
                                 c.metric, k, (int)c.nsplit, c.tps, sh.part_d.get<float>(), sh.part_i.get<int>(),
                                 c.m.exact ? 1 : 0, c.st);
    }
    return flat_lists_run(c);
}

// The bf16 list kernel.  Seeded (large tables): first the k-th best key of each query over the first 64K rows — the
// same kernel's lists over them and flat_bf16_seed (its lists start empty: every row an insert, ≈1 ms at 1024
// queries — what the bounded passes' keys mode replaces); the scan then admits only keys ≤ that bound.
static FlatCandRun flat_bf16_lists(FlatCall &c) {
    FlatShard &sh = c.sh;
    const int64_t nq = c.nq;
    const int k = c.m.kscan;
    if (c.m.seeded) {
        const int64_t seed_rows = 65536;
        const int64_t stiles = seed_rows / flat_bf16_tile_rows();
        const int64_t snsplit = std::min<int64_t>(stiles, std::max<int64_t>(1, ceil_div(256, c.nqt)));
        const int64_t stps = ceil_div(stiles, snsplit);
        sh.seed.ensure(sizeof(float) * ((size_t)snsplit * nq * k * 2 + (size_t)nq), sh.device);
        float *spd = sh.seed.get<float>() + nq;
        int *spi = reinterpret_cast<int *>(spd + (size_t)snsplit * nq * k);
        launch_flat_bf16_topk(c.xq, c.qn, nq, sh.qimg.p, sh.xb16.p, sh.xn.get<float>(), seed_rows, c.d, c.metric, k,
                              (int)ceil_div(stiles, stps), stps, spd, spi, nullptr, false, c.st);
        launch_flat_bf16_seed(spd, (int)ceil_div(stiles, stps), nq, k, sh.seed.get<float>(), c.st);
    }
    launch_flat_bf16_topk(c.xq, c.qn, nq, sh.qimg.p, sh.xb16.p, sh.xn.get<float>(), sh.n, c.d, c.metric, k,
                          (int)c.nsplit, c.tps, sh.part_d.get<float>(), sh.part_i.get<int>(),
                          c.m.seeded ? sh.seed.get<float>() : nullptr, c.m.seeded, c.st);
    return flat_lists_run(c);
}

// The bounded passes' plan for this call: the seed sample's rows, the passes' tile boundaries within every split —
// pass p scans tiles [pb[p], pb[p+1]) under the bound from everything before it (the seed for pass 0) — and the
// per-(query, split) candidate capacity.
struct FlatPassPlan {
    int64_t sample;
    std::vector<int64_t> pb;
    int cap;
};
static FlatPassPlan flat_plan_passes(const FlatCall &c) {
    FlatPassPlan p;
    const int64_t R = flat_bf16_tile_rows(), div = c.tune.pass_a;
    p.sample = std::max<int64_t>(256, std::min<int64_t>(c.tune.sample / 256 * 256, flat_keys_kth_max()));
    if (div < 0) p.pb = flat_pass_plan(c.tps, c.nsplit, R, p.sample, c.m.kscan, c.nq, c.tune.passes);
    else if (div > 1 && c.tps / div >= 1) p.pb = {0, c.tps / div, c.tps};
    else p.pb = {0, c.tps};
    p.cap = flat_pass_cap(p.pb, c.nsplit, R, p.sample, c.m.kscan);
    return p;
}

// The batch's query image in the scan's format; int8: with the queries' scales and residuals (the rerank's query
// term), by the fused preparation (which also writes the ‖q‖² still owed) or its three-launch form.
static void flat_bounded_queries(FlatCall &c) {
    FlatShard &sh = c.sh;
    if (!c.m.i8) return launch_b16_tile_rows(c.xq, c.nq, c.d, 32 * c.W, sh.qimg.p, c.st);
    sh.qscale.ensure(sizeof(float) * (size_t)c.nq, sh.device);
    sh.qres.ensure(sizeof(float) * (size_t)c.nq, sh.device);
    if (c.m.i8_prep) {
        launch_i8_query_prep(c.xq, c.nq, c.d, c.qn_owed, sh.qscale.get<float>(), sh.qres.get<float>(), 32 * c.W,
                             sh.qimg.p, c.st);
    } else {
        launch_i8_row_scale(c.xq, c.nq, c.d, sh.qscale.get<float>(), sh.qres.get<float>(), c.st);
        launch_i8_tile_rows(c.xq, sh.qscale.get<float>(), c.nq, c.d, 32 * c.W, sh.qimg.p, c.st);
    }
}

// HIPANN_FLAT_CAND_DEBUG: the candidate cells' fill after the passes (a host synchronisation of its own)
static void flat_cand_debug_print(const FlatCall &c, const FlatPassPlan &p, const FlatCandRun &r) {
    const size_t ncell = (size_t)c.nq * r.nsplit;
    std::vector<int> hn(ncell);
    std::vector<float> hb((size_t)c.nq);
    HIPANN_CHECK(hipMemcpyAsync(hn.data(), r.cn, sizeof(int) * ncell, hipMemcpyDeviceToHost, c.st));
    HIPANN_CHECK(hipMemcpyAsync(hb.data(), r.bound, sizeof(float) * c.nq, hipMemcpyDeviceToHost, c.st));
    HIPANN_CHECK(hipStreamSynchronize(c.st));
    long long tot = 0;
    int mx = 0;
    for (int v : hn) { tot += v; mx = std::max(mx, v); }
    std::fprintf(stderr, "hipann flat cand: nsplit %lld tps %lld passes %zu pass0 %lld cap %d mean %.2f max %d bound[0] %g\n",
                 (long long)r.nsplit, (long long)c.tps, p.pb.size() - 1, (long long)p.pb[1], r.cap,
                 (double)tot / (double)ncell, mx, (double)hb[0]);
}

// Bounded passes (64-dim K-step kernel, flat_b16k64.hip).  The seed: the kernel's keys mode over a sample of the
// first rows (a dense nq × S matrix, one tile per block, per chunk of 1024 queries = 4 query tiles through one 64 MB
// slab of keys) and its k-th order statistic (flat_keys_kth).  Then every row with key ≤ the bound goes to a
// per-(query, split) candidate buffer.  Pass 0 covers the first tiles of every split under the 16K-row seed bound;
// after each pass the bound is re-merged from all candidates so far (the k-th best key over every row scanned) and
// the next pass continues (flat_pass_plan: at 10M rows 4 passes over 5 / 20 / 98 / 488 tiles per split, ≈ 8.5
// candidates per query and split), no row scanned twice.  flat_cand_select keeps each query's k best for the rerank.
static FlatCandRun flat_bounded_passes(FlatCall &c) {
    FlatShard &sh = c.sh;
    const int64_t nq = c.nq, seed_qc = 1024;
    const int k = c.m.kscan, QM = 32 * c.W;
    const FlatPassPlan p = flat_plan_passes(c);
    const size_t ncell = (size_t)nq * c.nsplit;
    sh.seed.ensure(sizeof(float) * (size_t)nq, sh.device);
    sh.cand.ensure(std::max(ncell * ((size_t)p.cap * 8 + 4), (size_t)std::min(nq, seed_qc) * p.sample * sizeof(float)),
                   sh.device);
    flat_bounded_queries(c);
    float *cd = sh.cand.get<float>(), *bound = sh.seed.get<float>();
    int *ci = reinterpret_cast<int *>(cd + ncell * p.cap), *cn = ci + ncell * p.cap;
    FlatCandRun r;
    r.cd = cd, r.ci = ci, r.cn = cn, r.bound = bound, r.nsplit = (int)c.nsplit, r.cap = p.cap;
    FlatK64Args a;  // the operands: the images, their chunk count and (int8) scales, the L2 key terms
    a.qimg = sh.qimg.p, a.qn = c.qn, a.nq = nq, a.xn = sh.xn.get<float>(), a.metric = c.metric;
    a.ximg = c.m.i8 ? sh.xi8.p : sh.xb16.p, a.nk = c.m.i8 ? flat_i8_nk(c.d) : (int)ceil_div(c.d, 32);
    a.qscale = c.m.i8 ? sh.qscale.get<float>() : nullptr, a.xscale = c.m.i8 ? sh.xscale.get<float>() : nullptr;
    a.cand_d = cd;
    const size_t qtile_bytes = c.m.i8 ? flat_i8_img_bytes(QM, c.d, QM) : flat_bf16_img_bytes(QM, c.d, QM);
    for (int64_t c0 = 0; c0 < nq; c0 += seed_qc) {  // keys mode: the sample's tiles as splits of one tile
        FlatK64Args s = a;
        s.qimg = static_cast<const char *>(sh.qimg.p) + (size_t)(c0 / QM) * qtile_bytes;
        s.qn = c.qn ? c.qn + c0 : nullptr, s.qscale = a.qscale ? a.qscale + c0 : nullptr;
        s.nq = std::min(seed_qc, nq - c0), s.N = p.sample, s.keys = true;
        s.nqt = (int)ceil_div(s.nq, QM), s.nsplit = (int)(p.sample / flat_bf16_tile_rows());
        s.tiles_per_split = 1, s.tile_begin = 0, s.tile_end = 1;
        launch_flat_bf16_k64(s, c.st);
        launch_flat_keys_kth(cd, (int)p.sample, s.nq, k, bound + c0, c.st);
    }
    a.N = sh.n, a.nqt = (int)c.nqt, a.nsplit = (int)c.nsplit, a.tiles_per_split = c.tps;
    a.bound = bound, a.cand_i = ci, a.cand_n = cn, a.cap = p.cap;
    for (size_t i = 0; i + 1 < p.pb.size(); ++i) {
        a.tile_begin = p.pb[i], a.tile_end = p.pb[i + 1], a.resume = i > 0;
        launch_flat_bf16_k64(a, c.st);
        if (i + 2 < p.pb.size()) launch_flat_cand_bound(cd, cn, r.nsplit, r.cap, nq, k, bound, c.st);
    }
    // overflowed queries are flagged here, ahead of the rerank's own flags (the fallback re-runs both)
    flat_reset_flags(c);
    launch_flat_cand_select(r.cd, r.ci, r.cn, r.nsplit, r.cap, nq, k, sh.part_d.get<float>(), sh.part_i.get<int>(),
                            sh.nflag.get<int>(), sh.flagged.get<int>(), c.st);
    if (c.tune.cand_debug) flat_cand_debug_print(c, p, r);
    r.lists = 1, r.flags_reset = true;
    return r;
}

// Exact forms: each query's lists merged to the best scan keys, those rows recomputed in the direct form and
// bound-checked (ivf_rerank_topk, slot lists query-major); flagged queries re-run in flat_shard_finish.
static void flat_rerank(FlatCall &c, const FlatCandRun &r) {
    if (!r.flags_reset) flat_reset_flags(c);
    ScopedTiming t(c.ix.timer_merge, c.st);
    IvfRerankArgs a = flat_rerank_args(c);
    a.pd = c.sh.part_d.get<float>(), a.pi = c.sh.part_i.get<int>(), a.nprobe = r.lists, a.k = c.m.kscan;
    launch_ivf_rerank(a, c.st);
}

static void flat_merge_lists(FlatCall &c, const FlatCandRun &r) {
    ScopedTiming t(c.ix.timer_merge, c.st);
    launch_merge_parts<int>(c.sh.part_d.get<float>(), c.sh.part_i.get<int>(), r.lists, c.nq, c.m.kscan, c.kout,
                            c.sh.label_offset, 1.f, c.out_sign, c.D, c.I, c.st);
}

// What flat_shard_finish has left to do, from the mode and the stages' results — the one place a FlatPending is built.
static FlatPending flat_pending(const FlatCall &c, const FlatCandRun &r) {
    FlatPending p;
    p.kind = c.m.pend_kind, p.rerun_form = c.m.rerun_form, p.i8 = c.m.i8;
    p.nq = c.nq, p.xq = c.xq, p.k = c.m.k_user, p.kout = c.kout, p.D = c.D, p.I = c.I;
    p.cr_d = r.cd, p.cr_bound = r.bound, p.cr_i = r.ci, p.cr_n = r.cn, p.cr_nsplit = r.nsplit, p.cr_cap = r.cap;
    p.xmax2 = c.xmax2, p.rxmax = c.rxmax;
    return p;
}

// Launch phase of a shard search: every kernel of the search up to the exact forms' flag count, enqueued on `st`
// without a host synchronisation (queries already on the shard's device; D: nq×kout fp32 raw distances, ±inf pads;
// I: nq×kout int64 labels, −1 pads).  pend says what flat_shard_finish has left to do (kNone: the output is complete
// once `st` drains).
static void flat_shard_launch(FlatIndex &ix, FlatShard &sh, int64_t nq, const float *xq, int k, int kout, float *D,
                              int64_t *I, hipStream_t st, int form_override, FlatPending &pend) {
    pend = FlatPending{};
    DeviceGuard g(sh.device);
    HIPANN_REQUIRE(k <= HIPANN_MAX_K, "k larger than HIPANN_MAX_K");
    const FlatModeIn in{nq, sh.n, ix.d, ix.metric, k, kout, form_override >= 0 ? form_override : ix.form,
                        form_override >= 0, flat_tuning()};
    FlatCall c{ix, sh, nq, xq, kout, D, I, st, in.tune, flat_resolve_mode(in), ix.d, ix.metric,
               ix.metric == kIP ? -1.f : 1.f};
    const FlatScanMode &m = c.m;
    // sh.qn holds ‖q‖² of this batch only if the caller prepared it, until flat_query_norms says otherwise
    sh.qn_of = sh.qn_given == xq && sh.qn_given_nq == nq ? xq : nullptr;
    sh.qn_nq = nq;
    if (m.path == kFlatPathNone) return;
    if (m.path == kFlatPathPads)
        return launch_merge_parts<int>(nullptr, nullptr, 0, nq, k, kout, sh.label_offset, 1.f, c.out_sign, D, I, st);
    HIPANN_REQUIRE(sh.n <= (int64_t)0x7ffffffe, "shard larger than 2^31-2 rows");
    if (m.record) ix.last_form = m.last_form, ix.last_kfilt = m.last_kfilt, ix.last_sublists = 0;
    FlatCandRun run;
    if (m.path == kFlatPathKeys) {
        const float *qn = m.need_qn ? flat_query_norms(sh, nq, xq, c.d, st) : nullptr;
        return flat_shard_search_bigk(ix, sh, nq, xq, qn, k, kout, D, I, st);
    } else if (m.path == kFlatPathDirect) {
        return flat_direct_scan(c);
    } else if (m.path == kFlatPathSmallI8) {
        flat_small_i8(c);
    } else {
        flat_bound_terms(c);  // (host synchronisations at their first use; before ‖q‖², as ever)
        if (m.need_qn) c.qn = flat_query_norms(sh, nq, xq, c.d, st, m.prep_qn ? &c.qn_owed : nullptr);
        if (m.form == kFlatBf16Exact) ensure_b16_image(ix, sh, c.d, st);
        flat_lists_scratch(c);
        {
            ScopedTiming t(ix.timer_main, st);
            run = m.bounded ? flat_bounded_passes(c) : m.image() ? flat_bf16_lists(c) : flat_gemm_lists(c);
        }
        if (!m.exact) return flat_merge_lists(c, run);
        flat_rerank(c, run);
    }
    // the flagged count goes to the host with the results; flat_shard_finish re-runs what was not certified
    pend = flat_pending(c, run);
    flag_readback(sh, st);
}

// The second half of a shard search, once the host has synchronised with the launch phase's stream (its flag
// count read back into sh.h_nflag): nothing to do unless the exact form's bound check flagged queries.  Flagged
// queries are rare (0 on every benchmark batch); their re-runs are synchronous, on the form pend names (the fp32
// direct scan after the small-batch int8 scan, the 3-term split after the batched exact forms).
void flat_shard_finish(FlatIndex &ix, FlatShard &sh, const FlatPending &pend, hipStream_t st) {
    if (pend.kind == FlatPending::kNone) return;
    int nf = *sh.h_nflag.get<int>();
    if (nf <= 0) return;
    DeviceGuard g(sh.device);
    const int d = ix.d, kout = pend.kout;
    int *fl = sh.flagged.get<int>();
    if (pend.cr_d) {
        // bounded passes: rerank each flagged query over all its buffered candidates, certified against the pass
        // bound (launch_flat_cand_rerank); only what that cannot certify re-runs
        const bool dbg = flat_tuning().cand_debug;
        const int P = flat_cand_rerank_parts(pend.cr_nsplit);
        sh.crd.ensure(sizeof(float) * (size_t)nf * P * kout, sh.device);
        sh.cri.ensure(sizeof(long long) * (size_t)nf * P * kout, sh.device);
        sh.covf.ensure(sizeof(int) * (size_t)nf * P, sh.device);
        sh.nflag2.ensure(sizeof(int), sh.device);
        sh.flagged2.ensure(sizeof(int) * (size_t)nf, sh.device);
        HIPANN_CHECK(hipMemsetAsync(sh.nflag2.p, 0, sizeof(int), st));
        if (dbg) sh.tmpnorm.ensure(sizeof(float) * 4 * (size_t)nf, sh.device);
        FlatCandRerankArgs a;
        a.flagged = fl, a.nf = nf;
        a.cand_d = pend.cr_d, a.cand_i = pend.cr_i, a.cand_n = pend.cr_n, a.nsplit = pend.cr_nsplit, a.cap = pend.cr_cap;
        a.bound = pend.cr_bound, a.Q = pend.xq, a.X = sh.xb, a.d = d, a.nrows = sh.n, a.label_offset = sh.label_offset;
        a.xmax2 = pend.xmax2, a.rxmax = pend.rxmax, a.metric = ix.metric, a.kout = kout;
        a.part_d = sh.crd.get<float>(), a.part_i = sh.cri.get<long long>(), a.ovf = sh.covf.get<int>();
        a.D = pend.D, a.I = pend.I, a.nflag2 = sh.nflag2.get<int>(), a.flagged2 = sh.flagged2.get<int>();
        a.dbg = dbg ? sh.tmpnorm.get<float>() : nullptr, a.qres = pend.i8 ? sh.qres.get<float>() : nullptr;
        {
            ScopedTiming t(ix.timer_merge, st);
            launch_flat_cand_rerank(a, st);
        }
        ix.cand_reranked += nf;
        const int nf1 = nf;
        HIPANN_CHECK(hipMemcpyAsync(&nf, sh.nflag2.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        ++ix.host_syncs;
        if (dbg) {
            std::vector<float> h((size_t)nf1 * 4);
            HIPANN_CHECK(hipMemcpy(h.data(), sh.tmpnorm.p, h.size() * sizeof(float), hipMemcpyDeviceToHost));
            std::fprintf(stderr, "hipann flat flagged %d -> %d after the candidate rerank\n", nf1, nf);
            for (int j = 0; j < nf1 && j < 8; ++j)
                std::fprintf(stderr, "  overflow %g  dk %g  T %g  E %g\n", h[4 * j], h[4 * j + 1], h[4 * j + 2], h[4 * j + 3]);
        }
        if (nf <= 0) return;
        fl = sh.flagged2.get<int>();
    }
    ix.rerank_fallbacks += nf;
    sh.fq.ensure(sizeof(float) * (size_t)nf * d, sh.device);
    sh.fD.ensure(sizeof(float) * (size_t)nf * kout, sh.device);
    sh.fI.ensure(sizeof(int64_t) * (size_t)nf * kout, sh.device);
    launch_ivf_gather_queries(pend.xq, fl, nf, d, sh.fq.get<float>(), st);
    {
        TimerPause p0(ix.timer_main), p1(ix.timer_merge);
        flat_shard_search(ix, sh, nf, sh.fq.get<float>(), pend.k, kout, sh.fD.get<float>(), sh.fI.get<int64_t>(), st,
                          pend.rerun_form);
    }
    launch_ivf_scatter_results(sh.fD.get<float>(), sh.fI.get<int64_t>(), fl, nf, kout, pend.D, pend.I, st);
}

void flat_shard_search(FlatIndex &ix, FlatShard &sh, int64_t nq, const float *xq, int k, int kout, float *D,
                       int64_t *I, hipStream_t st, int form_override, FlatPending *pend) {
    RoctxRange r_all("hipann.flat.search_shard");
    FlatPending local;
    flat_shard_launch(ix, sh, nq, xq, k, kout, D, I, st, form_override, pend ? *pend : local);
    if (pend || local.kind == FlatPending::kNone) return;
    wait_posted(sh.h_nflag.get<unsigned>() + 1, sh.flag_seq, st);  // the flag count's token: the launch phase is done
    ++ix.host_syncs;
    flat_shard_finish(ix, sh, local, st);
}

}  // namespace hipann

// ================================================================================================
extern "C" {

int hipann_available(void) {
    try {
        if (device_count() <= 0) return 0;
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, 0) != hipSuccess) return 0;
        return std::strstr(p.gcnArchName, "gfx950") ? 1 : 0;
    } catch (...) {
        return 0;
    }
}

int hipann_device_count(void) { return device_count(); }

int hipann_peer_access(void *h, int *state, int cap, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h, "null index");
        auto *ix = static_cast<IndexBase *>(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        // single-device handles (the _device creates) carry no list: one shard, on its own device
        const std::vector<int> one{2};
        const std::vector<int> &pv = ix->peer.empty() ? one : ix->peer;
        const int n = (int)pv.size();
        HIPANN_REQUIRE(!state || cap >= n, "state buffer too small");
        if (state) for (int i = 0; i < n; ++i) state[i] = pv[(size_t)i];
        return n;
    });
}

int hipann_device_info(char *buf, int buf_len) {
    try {
        std::string s;
        const int n = device_count();
        if (n <= 0) s = "HIP: no device available";
        else {
            hipDeviceProp_t p;
            HIPANN_CHECK(hipGetDeviceProperties(&p, 0));
            char tmp[512];
            std::snprintf(tmp, sizeof tmp, "%s (%s, %d CUs, %.0f GB HBM) x%d", p.name, p.gcnArchName,
                          p.multiProcessorCount, (double)p.totalGlobalMem / 1e9, n);
            s = tmp;
        }
        set_err(buf, buf_len, s.c_str());
        return (int)s.size();
    } catch (...) {
        return -1;
    }
}

void *hipann_flat_create(int d, int metric, const float *xb, int64_t n, const int *devices, int ndev, char *eb,
                         int el) {
    return guard_ptr(eb, el, [&]() -> void * {
        require_device();
        HIPANN_REQUIRE(d > 0, "d must be > 0");
        HIPANN_REQUIRE(metric == kL2 || metric == kIP, "metric must be 0 (L2) or 1 (IP)");
        HIPANN_REQUIRE(n >= 0 && (n == 0 || xb), "invalid vectors");
        auto devs = device_list(devices, ndev);
        auto ix = std::make_unique<FlatIndex>();
        ix->d = d;
        ix->metric = metric;
        const int64_t per = ceil_div(std::max<int64_t>(n, 1), (int64_t)devs.size());
        int64_t off = 0;
        for (size_t i = 0; i < devs.size(); ++i) {
            auto sh = std::make_unique<FlatShard>();
            sh->device = devs[i];
            sh->stream = make_stream(devs[i]);
            sh->label_offset = off;
            const int64_t cnt = std::min<int64_t>(per, n - off);
            if (cnt > 0) shard_append(*sh, d, metric, xb + off * (int64_t)d, nullptr, cnt);
            off += std::max<int64_t>(cnt, 0);
            ix->shards.push_back(std::move(sh));
        }
        ix->peer = enable_peer_access(devs);
        return ix.release();
    });
}

int hipann_flat_add(void *h, const float *xb, int64_t n, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h, "null index");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::Flat, "not a Flat index");
        auto *fx = static_cast<FlatIndex *>(ix);
        std::lock_guard<std::mutex> lk(fx->mu);
        HIPANN_REQUIRE(n >= 0 && (n == 0 || xb), "invalid vectors");
        // appended rows go to the last shard (labels stay contiguous)
        auto &sh = *fx->shards.back();
        shard_append(sh, fx->d, fx->metric, xb, nullptr, n);
        return 0;
    });
}

int64_t hipann_flat_remove_ids(void *h, const int64_t *labels, int64_t n, char *eb, int el) {
    return guard_i64(eb, el, [&]() -> int64_t {
        HIPANN_REQUIRE(h, "null index");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::Flat, "not a Flat index");
        HIPANN_REQUIRE(n >= 0 && (n == 0 || labels), "invalid labels");
        if (n == 0) return 0;
        auto *fx = static_cast<FlatIndex *>(ix);
        std::lock_guard<std::mutex> lk(fx->mu);
        const std::vector<int64_t> lab = sorted_unique_labels(labels, n);
        // per shard, the local rows that leave (label − label_offset; labels outside every shard are ignored)
        const size_t ns = fx->shards.size();
        std::vector<std::vector<int64_t>> rows(ns);
        int64_t removed = 0;
        for (size_t s = 0; s < ns; ++s) {
            const FlatShard &sh = *fx->shards[s];
            auto lo = std::lower_bound(lab.begin(), lab.end(), sh.label_offset);
            auto hi = std::lower_bound(lo, lab.end(), sh.label_offset + sh.n);
            rows[s].reserve((size_t)(hi - lo));
            for (auto it = lo; it != hi; ++it) rows[s].push_back(*it - sh.label_offset);
            removed += (int64_t)rows[s].size();
        }
        if (!removed) return 0;
        // every shard's new storage first (nothing a search reads changes), then the swaps
        std::vector<FlatRemoval> rm(ns);
        for (size_t s = 0; s < ns; ++s) flat_remove_prepare(*fx->shards[s], fx->d, fx->metric, rows[s], rm[s]);
        auto relabel = [&]() {  // the later shards' labels shift down
            int64_t off = fx->shards[0]->label_offset;
            for (auto &shp : fx->shards) {
                shp->label_offset = off;
                off += shp->n;
            }
        };
        try {
            for (size_t s = 0; s < ns; ++s) flat_remove_commit(*fx->shards[s], fx->d, fx->metric, rm[s]);
        } catch (...) {  // (a failed launch with every buffer in hand: the shards already swapped keep contiguous labels)
            relabel();
            throw;
        }
        relabel();
        return removed;
    });
}

static int flat_search_host(FlatIndex &ix, int64_t nq, const float *xq, int64_t k, float *D, int64_t *I) {
    HIPANN_REQUIRE(k > 0, "k must be > 0");
    HIPANN_REQUIRE(k <= HIPANN_MAX_K, "k larger than HIPANN_MAX_K");
    HIPANN_REQUIRE(nq >= 0 && (nq == 0 || (xq && D && I)), "invalid arguments");
    const float pad = ix.metric == kIP ? -__builtin_inff() : __builtin_inff();
    const int64_t ntot = ix.ntotal();
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
    const int np = (int)ix.shards.size();
    // Launch phase: every shard's search on its own stream (devices run concurrently), no host wait.  The exact
    // forms' flag counts travel to pinned host words with the results (flat_shard_finish reads them).
    std::vector<FlatPending> pend((size_t)np);
    for (int p = 0; p < np; ++p) {
        FlatShard &sh = *ix.shards[p];
        DeviceGuard g(sh.device);
        sh.q.ensure(qbytes, sh.device);
        sh.out_d.ensure(ob * sizeof(float), sh.device);
        sh.out_i.ensure(ob * sizeof(int64_t), sh.device);
        FenceScope fs(sh.fence, sh.stream, sh.device);
        if (qbytes <= kKernelCopyMax) launch_copy_words(host_device_ptr(ix.h_q.p), sh.q.p, qbytes, sh.stream);
        else HIPANN_CHECK(hipMemcpyAsync(sh.q.p, ix.h_q.p, qbytes, hipMemcpyHostToDevice, sh.stream));
        flat_shard_search(ix, sh, nq, sh.q.get<float>(), keff, kout, sh.out_d.get<float>(), sh.out_i.get<int64_t>(),
                          sh.stream, -1, &pend[(size_t)p]);
        if (np > 1) {
            if (!sh.done) HIPANN_CHECK(hipEventCreateWithFlags(&sh.done, hipEventDisableTiming));
            HIPANN_CHECK(hipEventRecord(sh.done, sh.stream));
        }
    }
    ix.h_d.ensure(ob * sizeof(float));
    ix.h_i.ensure(ob * sizeof(int64_t));
    FlatShard &s0 = *ix.shards[0];
    // Completion: results (merged on shard 0's device when sharded) to the host, ONE host synchronisation — which
    // also covers every shard's flag count.  Only if a shard flagged queries: its re-runs, then the results again.
    auto deliver = [&]() {
        if (np == 1) {
            DeviceGuard g(s0.device);
            if (ob * sizeof(int64_t) <= kKernelCopyMax) {
                launch_copy_words(s0.out_d.p, host_device_ptr(ix.h_d.p), ob * sizeof(float), s0.stream);
                launch_copy_words(s0.out_i.p, host_device_ptr(ix.h_i.p), ob * sizeof(int64_t), s0.stream);
            } else {
                HIPANN_CHECK(hipMemcpyAsync(ix.h_d.p, s0.out_d.p, ob * sizeof(float), hipMemcpyDeviceToHost, s0.stream));
                HIPANN_CHECK(hipMemcpyAsync(ix.h_i.p, s0.out_i.p, ob * sizeof(int64_t), hipMemcpyDeviceToHost, s0.stream));
            }
        } else {
            // gather the per-device partial top-k onto shard 0's device (shard 0's stream waits for each shard's
            // launch phase on the device, not the host), then one device merge
            DeviceGuard g(s0.device);
            ix.gather_d.ensure(ob * np * sizeof(float), s0.device);
            ix.gather_i.ensure(ob * np * sizeof(int64_t), s0.device);
            ix.merged_d.ensure(ob * sizeof(float), s0.device);
            ix.merged_i.ensure(ob * sizeof(int64_t), s0.device);
            for (int p = 0; p < np; ++p) {
                FlatShard &sh = *ix.shards[p];
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
        }
        DeviceGuard g(s0.device);
        HIPANN_CHECK(hipStreamSynchronize(s0.stream));
        ++ix.host_syncs;
    };
    deliver();
    bool rerun = false;
    for (int p = 0; p < np; ++p) {
        FlatShard &sh = *ix.shards[p];
        if (pend[(size_t)p].kind == FlatPending::kNone || *sh.h_nflag.get<int>() <= 0) continue;
        FenceScope fs(sh.fence, sh.stream, sh.device);
        flat_shard_finish(ix, sh, pend[(size_t)p], sh.stream);
        if (np > 1) {
            DeviceGuard g(sh.device);
            HIPANN_CHECK(hipEventRecord(sh.done, sh.stream));
        }
        rerun = true;
    }
    if (rerun) deliver();
    std::memcpy(D, ix.h_d.p, ob * sizeof(float));
    std::memcpy(I, ix.h_i.p, ob * sizeof(int64_t));
    return 0;
}

int hipann_flat_search(void *h, int64_t nq, const float *xq, int64_t k, float *D, int64_t *I, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h, "null index");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::Flat, "not a Flat index");
        auto *fx = static_cast<FlatIndex *>(ix);
        std::lock_guard<std::mutex> lk(fx->mu);
        return flat_search_host(*fx, nq, xq, k, D, I);
    });
}

int hipann_flat_reconstruct(void *h, int64_t key, float *out, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h && out, "null argument");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::Flat, "not a Flat index");
        auto *fx = static_cast<FlatIndex *>(ix);
        std::lock_guard<std::mutex> lk(fx->mu);
        for (auto &shp : fx->shards) {
            FlatShard &sh = *shp;
            if (key >= sh.label_offset && key < sh.label_offset + sh.n) {
                DeviceGuard g(sh.device);
                HIPANN_CHECK(hipMemcpyAsync(out, sh.xb + (key - sh.label_offset) * fx->d, (size_t)fx->d * sizeof(float),
                                            hipMemcpyDeviceToHost, sh.stream));
                HIPANN_CHECK(hipStreamSynchronize(sh.stream));
                return 0;
            }
        }
        throw HipError("hipann: reconstruct key out of range");
    });
}

int hipann_flat_reconstruct_n(void *h, int64_t i0, int64_t n, float *out, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h && (n == 0 || out), "null argument");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::Flat, "not a Flat index");
        auto *fx = static_cast<FlatIndex *>(ix);
        std::lock_guard<std::mutex> lk(fx->mu);
        HIPANN_REQUIRE(i0 >= 0 && n >= 0 && i0 + n <= fx->ntotal(), "hipann: reconstruct_n range out of bounds");
        for (auto &shp : fx->shards) {  // shards hold contiguous label ranges
            FlatShard &sh = *shp;
            const int64_t lo = std::max(i0, sh.label_offset), hi = std::min(i0 + n, sh.label_offset + sh.n);
            if (lo >= hi) continue;
            DeviceGuard g(sh.device);
            HIPANN_CHECK(hipMemcpyAsync(out + (lo - i0) * fx->d, sh.xb + (lo - sh.label_offset) * fx->d,
                                        sizeof(float) * (size_t)(hi - lo) * fx->d, hipMemcpyDeviceToHost, sh.stream));
            HIPANN_CHECK(hipStreamSynchronize(sh.stream));
        }
        return 0;
    });
}

void *hipann_flat_create_device(int d, int metric, const float *xb_dev, int64_t n, int device, int copy,
                                int64_t label_offset, char *eb, int el) {
    return guard_ptr(eb, el, [&]() -> void * {
        require_device();
        HIPANN_REQUIRE(d > 0, "d must be > 0");
        HIPANN_REQUIRE(metric == kL2 || metric == kIP, "metric must be 0 (L2) or 1 (IP)");
        HIPANN_REQUIRE(device >= 0 && device < device_count(), "invalid device");
        HIPANN_REQUIRE(n >= 0 && (n == 0 || xb_dev), "invalid vectors");
        {   // the caller's writes to xb_dev may still be in flight on any of its streams
            DeviceGuard g(device);
            HIPANN_CHECK(hipDeviceSynchronize());
        }
        auto ix = std::make_unique<FlatIndex>();
        ix->d = d;
        ix->metric = metric;
        auto sh = std::make_unique<FlatShard>();
        sh->device = device;
        sh->stream = make_stream(device);
        sh->label_offset = label_offset;
        if (copy) {
            shard_append(*sh, d, metric, nullptr, xb_dev, n);
        } else {
            DeviceGuard g(device);
            sh->xb = const_cast<float *>(xb_dev);
            sh->owns = false;
            sh->n = n;
            sh->cap = n;
            if (metric == kL2 && n > 0) {
                sh->xn.ensure((size_t)n * sizeof(float), device);
                launch_row_norms(sh->xb, n, d, sh->xn.get<float>(), sh->stream);
                HIPANN_CHECK(hipStreamSynchronize(sh->stream));
            }
        }
        ix->shards.push_back(std::move(sh));
        return ix.release();
    });
}

int hipann_flat_search_device(void *h, int64_t nq, const float *xq_dev, int64_t k, float *D_dev, int64_t *I_dev,
                              void *stream, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        HIPANN_REQUIRE(h, "null index");
        auto *ix = static_cast<IndexBase *>(h);
        HIPANN_REQUIRE(ix->kind == Kind::Flat, "not a Flat index");
        auto *fx = static_cast<FlatIndex *>(ix);
        std::lock_guard<std::mutex> lk(fx->mu);
        HIPANN_REQUIRE(fx->shards.size() == 1, "device search needs a single-device index");
        HIPANN_REQUIRE(k > 0 && k <= HIPANN_MAX_K, "k out of range");
        FlatShard &sh = *fx->shards[0];
        hipStream_t st = static_cast<hipStream_t>(stream);  // NULL = the default (null) stream
        const int keff = (int)std::min<int64_t>(k, std::max<int64_t>(sh.n, 1));
        FenceScope fs(sh.fence, st, sh.device);  // the previous call's kernels may still use this shard's scratch
        flat_shard_search(*fx, sh, nq, xq_dev, keff, (int)k, D_dev, I_dev, st);
        return 0;
    });
}

int hipann_merge_topk_device(int metric, int nparts, int64_t nq, int64_t k, const float *D_parts,
                             const int64_t *I_parts, float *D_out, int64_t *I_out, void *stream, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        require_device();
        HIPANN_REQUIRE(metric == kL2 || metric == kIP, "bad metric");
        HIPANN_REQUIRE(k > 0 && k <= HIPANN_MAX_K && nparts >= 0, "bad arguments");
        const float sign = metric == kIP ? -1.f : 1.f;
        launch_merge_parts<long long>(D_parts, reinterpret_cast<const long long *>(I_parts), nparts, nq, (int)k, (int)k,
                                      0, sign, sign, D_out, I_out, static_cast<hipStream_t>(stream));
        return 0;
    });
}

int hipann_merge_topk_packed_device(int metric, int nparts, int64_t nq, int64_t k, const void *parts,
                                    int64_t part_bytes, float *D_out, int64_t *I_out, void *stream, char *eb, int el) {
    return guard_int(eb, el, [&]() -> int {
        require_device();
        HIPANN_REQUIRE(metric == kL2 || metric == kIP, "bad metric");
        HIPANN_REQUIRE(k > 0 && k <= HIPANN_MAX_K && nparts >= 0, "bad arguments");
        HIPANN_REQUIRE(part_bytes % 8 == 0 && part_bytes >= nq * k * 12, "part_bytes too small / misaligned");
        const float sign = metric == kIP ? -1.f : 1.f;
        const char *base = static_cast<const char *>(parts);
        // part p: [labels int64 nq*k][distances fp32 nq*k] at base + p * part_bytes
        launch_merge_parts<long long>(reinterpret_cast<const float *>(base + nq * k * 8),
                                      reinterpret_cast<const long long *>(base), nparts, nq, (int)k, (int)k, 0, sign,
                                      sign, D_out, I_out, static_cast<hipStream_t>(stream), part_bytes / 4,
                                      part_bytes / 8);
        return 0;
    });
}

int64_t hipann_ntotal(void *h) { return h ? static_cast<IndexBase *>(h)->ntotal() : -1; }
int hipann_dim(void *h) { return h ? static_cast<IndexBase *>(h)->d : -1; }
int hipann_metric(void *h) { return h ? static_cast<IndexBase *>(h)->metric : -1; }
int64_t hipann_memory_bytes(void *h) { return h ? static_cast<IndexBase *>(h)->memory_bytes() : -1; }

int hipann_flat_set_form(void *h, int form) {
    if (!h || form < kFlatFp32 || form > kFlatI8Exact) return -1;
    auto *ix = static_cast<IndexBase *>(h);
    if (ix->kind != Kind::Flat) return -1;
    auto *fx = static_cast<FlatIndex *>(ix);
    std::lock_guard<std::mutex> lk(fx->mu);
    fx->form = form;
    return 0;
}

int64_t hipann_flat_rerank_fallbacks(void *h) {
    if (!h) return -1;
    auto *ix = static_cast<IndexBase *>(h);
    if (ix->kind != Kind::Flat) return -1;
    return static_cast<FlatIndex *>(ix)->rerank_fallbacks;
}

int64_t hipann_flat_host_syncs(void *h) {
    if (!h) return -1;
    auto *ix = static_cast<IndexBase *>(h);
    if (ix->kind != Kind::Flat) return -1;
    std::lock_guard<std::mutex> lk(ix->mu);
    return static_cast<FlatIndex *>(ix)->host_syncs;
}

int hipann_last_search_path(void *h, int *form, int *filter_k, int *sublists) {
    if (!h) return -1;
    auto *ix = static_cast<IndexBase *>(h);
    std::lock_guard<std::mutex> lk(ix->mu);
    if (form) *form = ix->last_form;
    if (filter_k) *filter_k = ix->last_kfilt;
    if (sublists) *sublists = ix->last_sublists;
    return 0;
}

int hipann_flat_get_form(void *h) {
    if (!h) return -1;
    auto *ix = static_cast<IndexBase *>(h);
    if (ix->kind != Kind::Flat) return -1;
    return static_cast<FlatIndex *>(ix)->form;
}

void hipann_free(void *h) {
    if (!h) return;
    try {
        delete static_cast<IndexBase *>(h);
    } catch (...) {
    }
}

int hipann_set_kernel_timing(void *h, int on) {
    try {
        if (!h) return -1;
        auto *ix = static_cast<IndexBase *>(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        ix->timer_main.reset(on != 0, 0);
        ix->timer_merge.reset(on != 0, 0);
        return 0;
    } catch (...) {
        return -1;
    }
}

double hipann_last_kernel_ms(void *h, int which) {
    try {
        if (!h) return 0.0;
        auto *ix = static_cast<IndexBase *>(h);
        std::lock_guard<std::mutex> lk(ix->mu);
        return which == 0 ? ix->timer_main.average_ms() : ix->timer_merge.average_ms();
    } catch (...) {
        return 0.0;
    }
}

}  // extern "C"

// test hook (tests/test_flat_pass_cases.py): the bounded passes' plan for tps tiles per split — its boundaries into
// bounds[0 .. *nb) (at most 7) and the candidate capacity flat_shard_launch derives from them (no device needed);
// 0 on success, -1 on a bad shape
extern "C" int hipann_debug_flat_pass_plan(int64_t tps, int64_t nsplit, int64_t sample, int k, int64_t nq,
                                           int64_t *bounds, int *nb, int *cap) {
    try {
        if (tps < 1 || nsplit < 1 || sample < 256 || k < 1 || nq < 1 || !bounds || !nb || !cap) return -1;
        const std::vector<int64_t> pb = hipann::flat_pass_plan(tps, nsplit, hipann::flat_bf16_tile_rows(), sample, k, nq,
                                                               hipann::flat_tuning().passes);
        if (pb.size() < 2 || pb.size() > 7) return -1;
        for (size_t i = 0; i < pb.size(); ++i) bounds[i] = pb[i];
        *nb = (int)pb.size();
        *cap = hipann::flat_pass_cap(pb, nsplit, hipann::flat_bf16_tile_rows(), sample, k);
        return 0;
    } catch (...) {
        return -1;
    }
}

// test hook (tests/test_flat_scan_mode.py): the mode of a shard search as flat_shard_launch resolves it, with no
// device.  in[0..12): nq, n (the shard's rows), d, metric, k, kout, the requested form, is_override, then the switches
// the decision reads: HIPANN_FLAT_I8_SMALL, HIPANN_FLAT_BF16_SEED, HIPANN_I8_PREP_FUSED, HIPANN_B16_K64 (0 / 1).
// out[0..16): path (FlatPath), form, record, last_form, last_kfilt, exact, bounded, seeded, i8, i8_prep, kscan,
// k_user, pending kind, re-run form, need_qn, prep_qn.  0, or -1 on short arrays or a value out of range.
extern "C" int hipann_debug_flat_scan_mode(const int *in, int nin, int *out, int nout) {
    using namespace hipann;
    if (!in || !out || nin < 12 || nout < 16 || in[0] < 0 || in[1] < 0 || in[2] < 1 || in[4] < 1 || in[5] < 1) return -1;
    if ((in[3] != kL2 && in[3] != kIP) || in[6] < kFlatFp32 || in[6] > kFlatI8Exact) return -1;
    FlatModeIn mi;
    mi.nq = in[0], mi.n = in[1], mi.d = in[2], mi.metric = in[3], mi.k = in[4], mi.kout = in[5];
    mi.form = in[6], mi.is_override = in[7] != 0;
    mi.tune.i8_small = in[8] != 0, mi.tune.seed = in[9] != 0, mi.tune.i8_prep_fused = in[10] != 0;
    mi.tune.b16_k64 = in[11] != 0;
    const FlatScanMode m = flat_resolve_mode(mi);
    const int o[16] = {m.path, m.form, m.record, m.last_form, m.last_kfilt, m.exact, m.bounded, m.seeded,
                       m.i8, m.i8_prep, m.kscan, m.k_user, m.pend_kind, m.rerun_form, m.need_qn, m.prep_qn};
    std::copy(o, o + 16, out);
    return 0;
}
