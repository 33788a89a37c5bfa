// diskann_quantize.cpp — the entry point and the SQ8 search copy of a registered fp32 DiskANN DB, computed on the device
// (include/hip_diskann_bridge.h): diskann_hip_medoid, diskann_hip_quantize_sq8, diskann_hip_export_sq8.
// Host orchestration only: the kernels are in diskann_sq8.hip (diskann_kernels.hpp).  Both device calls hold the
// source's mutex, run on its stream and read its rows 0 .. n−1 only (`data` is a capacity after add_rows).
#include "diskann_db.hpp"
#include "diskann_kernels.hpp"

#include <chrono>
#include <memory>
#include <vector>

using namespace hipann;

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); }

// the body of diskann_hip_quantize_sq8 (throws; the entry point turns that into NULL + message)
DiskDB *quantize_sq8(void *h) {
    HIPANN_REQUIRE(h, "quantize_sq8: null db");
    auto *src = static_cast<DiskDB *>(h);
    std::lock_guard<std::mutex> lk(src->mu);
    HIPANN_REQUIRE(src->fmt == DISKANN_HIP_FMT_F32, "quantize_sq8: an fp32 DB is required (the source is SQ8)");
    HIPANN_REQUIRE(src->n > 0, "quantize_sq8: the DB has no rows");
    DeviceGuard g(src->device);
    RoctxRange rr("hipann.diskann.quantize_sq8");
    const hipStream_t st = src->stream;
    const int64_t n = src->n;
    const int d = src->dim, dev = src->device, R = src->R;
    const float *x = src->data.get<float>();
    double secs[3] = {0.0, 0.0, 0.0};
    auto t_rest = clk::now();

    // ---- every allocation, before any device work ----
    auto q = std::make_unique<DiskDB>();
    q->device = dev;
    HIPANN_CHECK(hipStreamCreateWithFlags(&q->stream, hipStreamNonBlocking));
    q->n = n;
    q->dim = d;
    q->fmt = DISKANN_HIP_FMT_SQ8;
    q->graph_metric = src->graph_metric;
    q->data.ensure((size_t)n * d + 16, dev);
    q->ab.ensure((size_t)d * 8, dev);
    q->ab_raw.ensure((size_t)d * 8, dev);
    const int64_t slabs = sq8_stat_slabs(n);
    DevBuf pmin, pmax, ms, flag;
    pmin.ensure((size_t)slabs * d * 4, dev);
    pmax.ensure((size_t)slabs * d * 4, dev);
    ms.ensure((size_t)d * 8, dev);
    flag.ensure(4, dev);
    std::vector<float> hms((size_t)d * 2);
    const size_t adj_words = (size_t)n * R, dup_bytes = (size_t)((n + 31) / 32) * 4;
    const bool with_dupw = R > 0 && src->dupw.p;
    if (R > 0) {
        q->adj_dev.ensure(adj_words * 4 + 16, dev);
        if (with_dupw) q->dupw.ensure(dup_bytes + 16, dev);
        q->adj_host.reserve(adj_words);
    }

    // ---- the finite check (the oracle's cast of a NaN is undefined, so such rows are refused) ----
    int bad = 0;
    HIPANN_CHECK(hipMemsetAsync(flag.p, 0, 4, st));
    launch_vamana_check_finite(x, n * (int64_t)d, flag.get<int>(), st);
    HIPANN_CHECK(hipMemcpyAsync(&bad, flag.p, 4, hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));
    HIPANN_REQUIRE(!bad, "quantize_sq8: the rows hold a non-finite value");
    secs[2] += since(t_rest);

    // ---- column statistics: min[d], scale[d] ----
    auto t0 = clk::now();
    launch_sq8_col_stats(x, n, d, true, false, pmin.get<float>(), pmax.get<float>(), nullptr, ms.get<float>(), nullptr,
                         st);
    HIPANN_CHECK(hipMemcpyAsync(hms.data(), ms.p, hms.size() * 4, hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));
    secs[0] = since(t0);

    // ---- encode ----
    t0 = clk::now();
    launch_sq8_encode(x, n, d, ms.get<float>(), q->data.get<uint8_t>(), st);
    HIPANN_CHECK(hipStreamSynchronize(st));
    secs[1] = since(t0);

    // ---- the decode tables (as diskann_hip_register_db fills them) and the graph, copied on the device ----
    t_rest = clk::now();
    sq8_fill_decode_tables(*q, hms.data(), hms.data() + d, st);
    if (R > 0) {
        HIPANN_CHECK(hipMemcpyAsync(q->adj_dev.p, src->adj_dev.p, adj_words * 4, hipMemcpyDeviceToDevice, st));
        if (with_dupw) HIPANN_CHECK(hipMemcpyAsync(q->dupw.p, src->dupw.p, dup_bytes, hipMemcpyDeviceToDevice, st));
    }
    HIPANN_CHECK(hipStreamSynchronize(st));
    if (R > 0) {
        // the host copy is read back only if a flagged query needs the host BFS (resident_search_locked)
        q->adj_host_stale = true;
        q->R = R;
    }
    secs[2] += since(t_rest);
    for (int i = 0; i < 3; ++i) src->quantize_s[i] = secs[i];
    return q.release();
}

}  // namespace

extern "C" {

int diskann_hip_medoid(void *h, uint32_t *row_out, char *eb, int el) {
    return abi_call(eb, el, [&] {
        HIPANN_REQUIRE(h && row_out, "medoid: null argument");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        HIPANN_REQUIRE(db->fmt == DISKANN_HIP_FMT_F32, "medoid: an fp32 DB is required (SQ8 is not supported)");
        HIPANN_REQUIRE(db->n > 0, "medoid: the DB has no rows");
        HIPANN_REQUIRE(db->n <= (int64_t)UINT32_MAX, "medoid: n must be below 2^32");
        DeviceGuard g(db->device);
        RoctxRange rr("hipann.diskann.medoid");
        const hipStream_t st = db->stream;
        const int64_t n = db->n, slabs = sq8_stat_slabs(n);
        const int d = db->dim, dev = db->device, nb = medoid_nearest_blocks(n);
        DevBuf psum, mean, bd, bi;
        psum.ensure((size_t)slabs * d * 8, dev);
        mean.ensure((size_t)d * 8, dev);
        bd.ensure((size_t)nb * 8, dev);
        bi.ensure((size_t)(nb + 1) * 4, dev);  // the blocks' ids, then the result
        const float *x = db->data.get<float>();
        launch_sq8_col_stats(x, n, d, false, true, nullptr, nullptr, psum.get<double>(), nullptr, mean.get<double>(),
                             st);
        launch_medoid_nearest(x, n, d, mean.get<double>(), bd.get<double>(), bi.get<uint32_t>(),
                              bi.get<uint32_t>() + nb, st);
        uint32_t row = 0;
        HIPANN_CHECK(hipMemcpyAsync(&row, bi.get<uint32_t>() + nb, 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        *row_out = row;
        return 0;
    });
}

void *diskann_hip_quantize_sq8(void *h, char *eb, int el) {
    try {
        return quantize_sq8(h);
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return nullptr;
}

int diskann_hip_export_sq8(void *h, void *codes, float *sq8_min, float *sq8_scale, char *eb, int el) {
    return abi_call(eb, el, [&] {
        HIPANN_REQUIRE(h, "export_sq8: null db");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        HIPANN_REQUIRE(db->fmt == DISKANN_HIP_FMT_SQ8, "export_sq8: an SQ8 DB is required (the handle is fp32)");
        DeviceGuard g(db->device);
        const hipStream_t st = db->stream;
        const int d = db->dim;
        const size_t bytes = (size_t)db->n * d;
        std::vector<float> abr((size_t)d * 2);  // (scale, min) per dimension
        if (codes && bytes) HIPANN_CHECK(hipMemcpyAsync(codes, db->data.p, bytes, hipMemcpyDeviceToHost, st));
        if (sq8_min || sq8_scale)
            HIPANN_CHECK(hipMemcpyAsync(abr.data(), db->ab_raw.p, abr.size() * 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        for (int j = 0; j < d; ++j) {
            if (sq8_scale) sq8_scale[j] = abr[2 * j];
            if (sq8_min) sq8_min[j] = abr[2 * j + 1];
        }
        return 0;
    });
}

int diskann_hip_quantize_phase_seconds(void *h, double *seconds) {
    return phase_seconds(h, seconds, &DiskDB::quantize_s);
}

}  // extern "C"
