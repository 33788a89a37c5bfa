// diskann_db.hpp — (internal) what diskann.hip (bridge, launchers, DB registry, resident search), diskann_host_bfs.cpp
// (the lock-step host BFS), diskann_graph.cpp (graph build, add, remove, prune) and diskann_quantize.cpp (medoid, SQ8 copy)
// share on the host: the HBM-resident DB, the id-gather launcher, the two searches, and the C ABI's error epilogue.
#pragma once
#include "../../include/hip_diskann_bridge.h"
#include "common.hpp"
#include "runtime.hpp"

#include <cstring>
#include <exception>

namespace hipann {

struct DiskDB {
    int device = 0;
    int64_t n = 0;
    int dim = 0;
    int fmt = DISKANN_HIP_FMT_F32;
    DevBuf data;  // fp32 rows or u8 codes
    DevBuf ab;    // float2 per dim (SQ8): (scale/255, min), the traversal's fused decode
    DevBuf ab_raw;  // float2 per dim (SQ8): (scale, min), the id-gather kernels' exact decode
    hipStream_t stream = nullptr;
    std::mutex mu;
    DevBuf q, ids, m, out;
    HostBuf hids, hm, hout;
    KernelTimer timer;
    // resident graph + BFS scratch (diskann_hip_register_graph / _search_batch_resident)
    int R = 0;
    // the metric of the graph this handle builds and maintains (diskann_hip_set_graph_metric): kL2 unless told
    // otherwise.  The graph-writing calls require their `metric` argument to equal it; the searches do not read it.
    int graph_metric = kL2;
    DevBuf adj_dev, dupw, visited, flags, bstats, eps_dev;
    DevBuf vbits;  // host BFS: the queries' visited bits on the device (one bit per row and query)
    std::vector<uint32_t> adj_host;
    // diskann_hip_build_graph: adj_dev is ahead of adj_host (the resident search refreshes the host copy before it
    // re-runs a flagged query on it); the last build's seconds in search / out-edge prunes / back-edges
    bool adj_host_stale = false;
    double build_s[3] = {0.0, 0.0, 0.0};
    double remove_s[3] = {0.0, 0.0, 0.0};  // the last diskann_hip_remove_ids: pool build, prune, compact
    double add_s[4] = {0.0, 0.0, 0.0, 0.0};  // the last diskann_hip_add_rows: searches, mates, out-edge prunes, back-edges
    double quantize_s[3] = {0.0, 0.0, 0.0};  // the last diskann_hip_quantize_sq8 from this DB: statistics, encode, rest
    ~DiskDB() {
        if (stream) { DeviceGuard g(device); (void)hipStreamDestroy(stream); }
    }
};

// Resident search: queries / outputs in HBM, asynchronous launch on `st`, then a wait for the per-query flags (the
// rare flagged queries and unsupported shapes go through the host BFS).  The caller holds db->mu and the device; the
// graph build and add_rows search their own frozen graph through this.
void resident_search_locked(DiskDB *db, const uint32_t *eps, int n_ep, const float *queries_dev, int nq, int k,
                            int l_search, int metric, int64_t *out_ids_dev, float *out_d_dev, int64_t *stats,
                            hipStream_t st);

// The id-gather launch (diskann.hip): out[i] = the distance of query m[i] to row ids[i] of the DB, for total_n
// candidates; an id ≥ db.n is an empty slot and leaves out[i] alone.  With vbits (the host BFS's visited sets on the
// device, vwords words per query) a candidate whose bit is already set comes back as kVisitedBits instead.
void launch_ids(DiskDB &db, const float *q, const unsigned *ids, const unsigned *m, int total_n, int metric,
                float *out, hipStream_t st, unsigned *vbits = nullptr, int64_t vwords = 0);

// Host-driven lock-step BFS (diskann_host_bfs.cpp; the reference's structure: host state, one id-gather launch per
// step) over the host adjacency adj (db->n × R): the body of diskann_hip_search_batch, whose outputs and stats it
// fills, and the fallback of the resident search for flagged queries.  The caller holds db->mu and the device.
void host_bfs(DiskDB *db, const uint32_t *adj, int R, const uint32_t *eps, int n_ep, const float *queries, int nq,
              int k, int l_search, int metric, int64_t *out_ids, float *out_d, int64_t *stats);

// An SQ8 DB's decode tables from the codec's per-dimension min / scale (host, db.dim each), queued on st: ab =
// (scale/255, min), the traversal's fused form, and ab_raw = (scale, min), the id-gather kernels' exact decode.  The
// one place they are computed: diskann_hip_register_db and diskann_hip_quantize_sq8 fill a handle through it.
void sq8_fill_decode_tables(DiskDB &db, const float *sq8_min, const float *sq8_scale, hipStream_t st);

// the last call's phase clocks (DiskDB::build_s / add_s / remove_s / quantize_s) for the *_phase_seconds entry points
template <int N> int phase_seconds(void *h, double *seconds, double (DiskDB::*phases)[N]) {
    if (!h || !seconds) return -1;
    auto *db = static_cast<DiskDB *>(h);
    std::lock_guard<std::mutex> lk(db->mu);
    for (int i = 0; i < N; ++i) seconds[i] = (db->*phases)[i];
    return 0;
}

inline void set_err(char *buf, int len, const char *msg) {
    if (!buf || len <= 0) return;
    std::strncpy(buf, msg, (size_t)len - 1);
    buf[len - 1] = '\0';
}

// The epilogue of a C entry point with an error buffer: the body's value, or −1 with the exception's text in (eb, el).
template <typename F>
auto abi_call(char *eb, int el, F &&body) -> decltype(body()) {
    try {
        return body();
    } catch (const std::exception &e) {
        set_err(eb, el, e.what());
    } catch (...) {
        set_err(eb, el, "hipann: unknown error");
    }
    return -1;
}

}  // namespace hipann
