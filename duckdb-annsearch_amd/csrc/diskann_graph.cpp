// diskann_graph.cpp — DiskANN graph maintenance on the device, host side (include/hip_diskann_bridge.h): graph build
// (DESIGN.md §6), row insertion (§6.3), row removal (§6.2) and the stand-alone RobustPrune / batch-mates entry points.
// Host orchestration only: the kernels are in diskann_build.hip, diskann_add.hip and diskann_remove.hip
// (diskann_kernels.hpp), the searches go through the resident search of diskann.hip (diskann_db.hpp).
//
// The build and add_rows insert a batch the same way — VamanaInsert::step: out-edge prune, back-edges, overflow prune —
// and differ in what surrounds it: the build's entry-point gap and slot rollback, add_rows' growth, finite check and
// batch mates.
#include "diskann_db.hpp"
#include "diskann_kernels.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

using namespace hipann;

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); }

void swap_buf(DevBuf &a, DevBuf &b) {
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
    std::swap(a.device, b.device);
}

// the shapes the build entry points and remove_ids refuse (a message, never a slow path); `who` names the call.  The
// call's metric must be the handle's graph metric (diskann_hip_set_graph_metric; L2 unless the handle was told otherwise).
void build_shape_check(const DiskDB *db, int R, float alpha, int metric, const char *who = "graph build") {
    const std::string w = std::string(who) + ": ";
    if (db->graph_metric == kL2) {
        HIPANN_REQUIRE(metric != kIP, w + "IP is not supported (the crate prunes IP by a different rule)");
        HIPANN_REQUIRE(metric == kL2, w + "metric must be 0 (L2)");
    } else {
        HIPANN_REQUIRE(metric == kIP, w + "metric must be 1 (IP): the handle's graph metric is IP "
                                          "(diskann_hip_set_graph_metric)");
    }
    HIPANN_REQUIRE(db->fmt == DISKANN_HIP_FMT_F32, w + "an fp32 DB is required (SQ8 is not supported)");
    HIPANN_REQUIRE(R >= 1 && R <= 64, w + "R must be in [1, 64]");
    HIPANN_REQUIRE(db->dim % 4 == 0 && db->dim <= 2048, w + "d must be a multiple of 4 and at most 2048");
    HIPANN_REQUIRE(db->n < ((int64_t)1 << 31), w + "n must be below 2^31");
    HIPANN_REQUIRE(alpha >= 1.0f, w + "alpha must be >= 1");  // (a NaN fails the comparison)
}

// the host copy of the adjacency brought level with the device's (the caller holds db->mu and the device)
void refresh_adj_host(DiskDB *db, hipStream_t st) {
    db->adj_host.resize((size_t)db->n * db->R);
    HIPANN_CHECK(hipMemcpyAsync(db->adj_host.data(), db->adj_dev.p, db->adj_host.size() * 4, hipMemcpyDeviceToHost, st));
    HIPANN_CHECK(hipStreamSynchronize(st));
    db->adj_host_stale = false;
}

// rows a walk from entry_point over the host adjacency does not reach (rows end at the first UINT32_MAX)
int64_t unreached_rows(const std::vector<uint32_t> &a, int64_t n, int R, uint32_t entry_point) {
    std::vector<uint8_t> seen((size_t)n, 0);
    std::vector<uint32_t> stack{entry_point};
    seen[entry_point] = 1;
    int64_t reached = 1;
    while (!stack.empty()) {
        const uint32_t v = stack.back();
        stack.pop_back();
        for (int r = 0; r < R; ++r) {
            const uint32_t w = a[(size_t)v * R + r];
            if (w == kNone) break;
            if (w < (uint64_t)n && !seen[w]) { seen[w] = 1; ++reached; stack.push_back(w); }
        }
    }
    return n - reached;
}

// `buf` with room for `need` bytes and its first `keep` bytes preserved: in place when the capacity suffices, else
// a new buffer a quarter larger than the old one (at least `need`) in `grown`, for the caller to swap in.
void *grow_keep(DevBuf &buf, DevBuf &grown, size_t need, size_t keep, int dev, hipStream_t st) {
    if (buf.p && need <= buf.bytes) return buf.p;
    grown.ensure(std::max(need, buf.bytes + buf.bytes / 4), dev);
    if (keep) HIPANN_CHECK(hipMemcpyAsync(grown.p, buf.p, keep, hipMemcpyDeviceToDevice, st));
    return grown.p;
}

// The insert step the graph build and add_rows share: a batch of rows, already searched against the frozen graph
// (their lists in sid / sd), gets its out-edges and the graph its back-edges.  The scratch is sized once per call.
struct VamanaInsert {
    // set by the caller before the first step, the same for every batch
    const float *x = nullptr;
    uint32_t *adj = nullptr;
    int d = 0, R = 0;
    int T = 0;  // batch mates per row (0: the out-edge prune reads the traversal's lists in place)
    float alpha = 0.f;
    int metric = kL2;  // the handle's graph metric
    uint32_t ep = 0;
    hipStream_t st = nullptr;

    DevBuf sid, sd;  // the batch's search results: bmax × K labels and distances
    DevBuf tg, cnt, slot, touched, off, fill, src, pool, ptgt, pbeg, plen, ctr, gram;
    DevBuf mates, nrm, opool, obeg, olen;  // T > 0: the mates and the out-edge prune's concatenated pools
    DevBuf pctr;  // u64 [0..3]: the prunes' counters — overflow prunes at 0, out-edge prunes at 2 (the caller clears it)
    int blocks = 0;
    unsigned long long pc[5] = {0, 0, 0, 0, 0};  // pctr on the host (queue_counters)

    // batches of at most bmax rows, lists of at most K ids, a graph of at most n_max rows, pctr_bytes of counters
    void size(const char *who, int bmax, int K, int64_t n_max, size_t pctr_bytes, int dev) {
        const int64_t pairs = (int64_t)bmax * R;
        const int64_t rows_max = std::min<int64_t>(pairs, n_max);  // rows one batch's back-edges can touch
        const int64_t pool_words = rows_max * R + pairs;
        HIPANN_REQUIRE(pairs < INT32_MAX && pool_words < INT32_MAX, std::string(who) + ": batch_max too large");
        sid.ensure((size_t)bmax * K * 8, dev);
        sd.ensure((size_t)bmax * K * 4, dev);
        tg.ensure((size_t)bmax * 4, dev);
        for (DevBuf *w : {&cnt, &slot}) w->ensure((size_t)n_max * 4, dev);
        for (DevBuf *w : {&touched, &off, &fill, &src}) w->ensure((size_t)pairs * 4, dev);
        pool.ensure((size_t)pool_words * 4, dev);
        for (DevBuf *w : {&ptgt, &pbeg, &plen}) w->ensure((size_t)rows_max * 4, dev);
        ctr.ensure(16, dev);
        pctr.ensure(pctr_bytes, dev);
        if (T > 0) {
            mates.ensure((size_t)bmax * T * 4, dev);
            opool.ensure((size_t)bmax * (K + T) * 4, dev);
            for (DevBuf *w : {&nrm, &obeg, &olen}) w->ensure((size_t)bmax * 4, dev);
        }
        blocks = vamana_prune_blocks(std::max<int64_t>(bmax, rows_max));
        gram.ensure(vamana_gram_bytes(blocks), dev);
    }

    // The batch of b rows at insertion orders o0 .. o0 + b − 1, their K-wide lists in sid / sd; `rows` bounds the ids
    // (the graph's rows once the batch is in).  secs[0] += the out-edge prunes' seconds, secs[1] += the back-edges'.
    void step(uint32_t o0, int b, int K, int64_t rows, bool with_mates, double *secs) {
        PruneArgs p;  // what the two prunes share
        p.x = x; p.d = d; p.n = (uint32_t)rows; p.R = R; p.alpha = alpha; p.metric = metric;
        p.out = adj; p.out_by_target = 1; p.gram = gram.get<float>();
        // out-edges: N(p) = prune(p, the traversal's list [+ the row's batch mates])
        auto t1 = clk::now();
        launch_vamana_fill_targets(tg.get<uint32_t>(), b, o0, ep, st);
        PruneArgs o = p;
        o.targets = tg.get<uint32_t>(); o.m = b; o.counters = pctr.get<unsigned long long>() + 2;
        if (T == 0) {
            o.pool64 = sid.get<int64_t>(); o.pool_d = sd.get<float>(); o.pool_cap = K;
        } else {
            launch_vamana_concat_pool(sid.get<int64_t>(), K, with_mates ? mates.get<uint32_t>() : nullptr, T, b,
                                      opool.get<uint32_t>(), obeg.get<int>(), olen.get<int>(), st);
            o.pool32 = opool.get<uint32_t>(); o.pool_beg = obeg.get<int>(); o.pool_len = olen.get<int>();
        }
        launch_vamana_prune(o, blocks, st);
        HIPANN_CHECK(hipStreamSynchronize(st));
        secs[0] += since(t1);
        // back-edges, grouped per target row on the device; rows that overflow are pruned (a target may be a batch row:
        // the stream puts every read of the out-edges before be_merge)
        auto t2 = clk::now();
        HIPANN_CHECK(hipMemsetAsync(cnt.p, 0, (size_t)rows * 4, st));
        HIPANN_CHECK(hipMemsetAsync(ctr.p, 0, 16, st));
        launch_vamana_backedges(adj, R, tg.get<uint32_t>(), b, cnt.get<int>(), slot.get<int>(), touched.get<uint32_t>(),
                                off.get<int>(), fill.get<int>(), src.get<uint32_t>(), ctr.get<int>(),
                                pool.get<uint32_t>(), ptgt.get<uint32_t>(), pbeg.get<int>(), plen.get<int>(), st);
        PruneArgs v = p;  // ctr[3] targets (at most min(b·R, rows)), their pools in `pool`
        v.targets = ptgt.get<uint32_t>(); v.m = (int)std::min<int64_t>((int64_t)b * R, rows); v.m_ptr = ctr.get<int>() + 3;
        v.pool32 = pool.get<uint32_t>(); v.pool_beg = pbeg.get<int>(); v.pool_len = plen.get<int>();
        v.counters = pctr.get<unsigned long long>();
        launch_vamana_prune(v, blocks, st);
        HIPANN_CHECK(hipStreamSynchronize(st));
        secs[1] += since(t2);
    }

    // after the last step: the first `words` counters of pctr on their way into pc (the caller synchronises) ...
    void queue_counters(int words) {
        HIPANN_CHECK(hipMemcpyAsync(pc, pctr.p, (size_t)words * 8, hipMemcpyDeviceToHost, st));
    }
    // ... and the prunes' share of them in the call's stats: back-edge prunes, pools truncated to 256
    void counters_to_stats(int64_t *s8) const {
        s8[3] = (int64_t)pc[0];
        s8[5] = (int64_t)(pc[1] + pc[3]);
    }
};

}  // namespace

extern "C" {

// ---- graph build on the device (kernels in diskann_build.hip) ----
int diskann_hip_build_graph(void *h, int R, int l_build, float alpha, int metric, uint32_t entry_point, int batch_max,
                            uint32_t *adjacency_out, int64_t *stats, char *eb, int el) {
    return abi_call(eb, el, [&] {
        HIPANN_REQUIRE(h, "graph build: null db");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        build_shape_check(db, R, alpha, metric);
        HIPANN_REQUIRE(l_build >= 1 && l_build <= 256, "graph build: L must be in [1, 256]");
        HIPANN_REQUIRE(batch_max >= 1, "graph build: batch_max must be >= 1");
        HIPANN_REQUIRE((int64_t)entry_point < db->n, "graph build: entry_point must be below n");
        DeviceGuard g(db->device);
        RoctxRange rr("hipann.diskann.build_graph");
        const hipStream_t st = db->stream;
        const int64_t n = db->n;
        const int d = db->dim, dev = db->device;
        int64_t s8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        // The graph under construction sits in the DB's own graph slots (the traversal reads them); the slots' former
        // contents come back if the build fails.  No built row repeats an id, so dupw stays zero.
        DevBuf nadj, ndupw;
        std::vector<uint32_t> nhost;
        int nR = R;
        nadj.ensure((size_t)n * R * 4 + 16, dev);
        ndupw.ensure((size_t)((n + 31) / 32) * 4 + 16, dev);
        HIPANN_CHECK(hipMemsetAsync(nadj.p, 0xff, (size_t)n * R * 4, st));
        HIPANN_CHECK(hipMemsetAsync(ndupw.p, 0, (size_t)((n + 31) / 32) * 4, st));
        struct Slots {
            DiskDB *db;
            DevBuf &a, &w;
            std::vector<uint32_t> &hst;
            int &R;
            bool keep = false;
            bool stale0;  // whether the former graph's host copy was behind its device copy (after add_rows)
            void exchange() {
                swap_buf(db->adj_dev, a);
                swap_buf(db->dupw, w);
                db->adj_host.swap(hst);
                std::swap(db->R, R);
            }
            ~Slots() {
                if (!keep) exchange();
                db->adj_host_stale = keep ? false : stale0;
            }
        } slots{db, nadj, ndupw, nhost, nR, false, db->adj_host_stale};
        slots.exchange();
        db->adj_host_stale = false;
        double secs[3] = {0.0, 0.0, 0.0};
        if (n > 1) {
            const uint32_t ep = entry_point;
            const int K = (int)std::min<int64_t>(l_build, n);
            const int bmax = (int)std::min<int64_t>(batch_max, n - 1);
            VamanaInsert ins;
            ins.x = db->data.get<float>(); ins.adj = db->adj_dev.get<uint32_t>();
            ins.d = d; ins.R = R; ins.alpha = alpha; ins.metric = metric; ins.ep = ep; ins.st = st;
            ins.size("graph build", bmax, K, n, 32, dev);
            HIPANN_CHECK(hipMemsetAsync(ins.pctr.p, 0, 32, st));
            const uint32_t eps1[1] = {ep};
            int64_t o0 = 0;  // rows inserted so far in insertion order (row order, the entry point left out)
            while (o0 < n - 1) {
                const int b = (int)std::min<int64_t>(std::min<int64_t>(bmax, std::max<int64_t>(1, o0 + 1)), n - 1 - o0);
                const int64_t o1 = o0 + b;
                // search the frozen graph: the batch's rows are contiguous but for the entry point's gap
                auto t0 = clk::now();
                const int64_t seg[2][2] = {{o0, std::min<int64_t>(o1, ep)}, {std::max<int64_t>(o0, ep), o1}};
                for (int sgi = 0; sgi < 2; ++sgi) {
                    const int64_t oa = seg[sgi][0], ob = seg[sgi][1];
                    if (ob <= oa) continue;
                    const int64_t row0 = sgi == 0 ? oa : oa + 1;
                    int64_t sst[4] = {0, 0, 0, 0};
                    resident_search_locked(db, eps1, 1, ins.x + row0 * d, (int)(ob - oa), K, l_build, metric,
                                           ins.sid.get<int64_t>() + (oa - o0) * K, ins.sd.get<float>() + (oa - o0) * K,
                                           sst, st);
                    s8[0] += sst[0];
                    s8[4] += sst[3];
                }
                secs[0] += since(t0);
                ins.step((uint32_t)o0, b, K, n, false, secs + 1);
                db->adj_host_stale = true;
                s8[1] += 1;
                s8[2] += b;
                o0 = o1;
            }
            ins.queue_counters(4);
            HIPANN_CHECK(hipStreamSynchronize(st));
            ins.counters_to_stats(s8);
        }
        // registered as after diskann_hip_register_graph: the host copy and the repeated-id row bits
        launch_diskann_dup_rows(db->adj_dev.get<uint32_t>(), R, n, db->dupw.get<uint32_t>(), st);
        db->adj_host.resize((size_t)n * R);
        HIPANN_CHECK(hipMemcpyAsync(db->adj_host.data(), db->adj_dev.p, (size_t)n * R * 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        s8[6] = unreached_rows(db->adj_host, n, R, entry_point);
        if (adjacency_out) std::memcpy(adjacency_out, db->adj_host.data(), (size_t)n * R * 4);
        if (stats) std::memcpy(stats, s8, sizeof(s8));
        for (int i = 0; i < 3; ++i) db->build_s[i] = secs[i];
        slots.keep = true;
        return 0;
    });
}

int diskann_hip_build_phase_seconds(void *h, double *seconds) { return phase_seconds(h, seconds, &DiskDB::build_s); }

// ---- row insertion into the device graph (kernels in diskann_add.hip and diskann_build.hip) ----
int64_t diskann_hip_add_rows(void *h, const float *rows, int64_t m, int l_build, float alpha, int metric,
                             uint32_t entry_point, int batch_max, int batch_mates, uint32_t *adjacency_out,
                             int64_t *stats, char *eb, int el) {
    return abi_call(eb, el, [&]() -> int64_t {
        HIPANN_REQUIRE(h, "add_rows: null db");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        HIPANN_REQUIRE(db->R > 0, "add_rows: no graph registered (diskann_hip_register_graph / _build_graph)");
        build_shape_check(db, db->R, alpha, metric, "add_rows");
        HIPANN_REQUIRE(l_build >= 1 && l_build <= 256, "add_rows: L must be in [1, 256]");
        HIPANN_REQUIRE(batch_max >= 1, "add_rows: batch_max must be >= 1");
        HIPANN_REQUIRE(batch_mates >= 0 && batch_mates <= 64, "add_rows: batch_mates must be in [0, 64]");
        HIPANN_REQUIRE(l_build + batch_mates <= 512, "add_rows: L + batch_mates must be at most 512");
        HIPANN_REQUIRE((int64_t)entry_point < db->n, "add_rows: entry_point must be below n");
        HIPANN_REQUIRE(m >= 0 && (m == 0 || rows), "add_rows: null rows");
        HIPANN_REQUIRE(db->n + m < ((int64_t)1 << 31), "add_rows: n + m must be below 2^31");
        DeviceGuard g(db->device);
        const hipStream_t st = db->stream;
        const int64_t n0 = db->n, n1 = n0 + m;
        const int R = db->R, d = db->dim, dev = db->device, T = batch_mates, L = l_build;
        int64_t s8[8] = {0, 0, 0, 0, 0, 0, -1, 0};
        if (m == 0) {  // nothing moves
            if (adjacency_out) {
                if (db->adj_host_stale) refresh_adj_host(db, st);
                s8[6] = unreached_rows(db->adj_host, n0, R, entry_point);
                std::memcpy(adjacency_out, db->adj_host.data(), (size_t)n0 * R * 4);
            }
            if (stats) std::memcpy(stats, s8, sizeof(s8));
            return 0;
        }
        RoctxRange rr("hipann.diskann.add_rows");
        double secs[4] = {0.0, 0.0, 0.0, 0.0};
        const uint32_t ep = entry_point;

        // ---- everything that can refuse or allocate, before anything a search reads changes ----
        const int bmax = (int)std::min<int64_t>(batch_max, m);
        VamanaInsert ins;
        ins.d = d; ins.R = R; ins.T = T; ins.alpha = alpha; ins.metric = metric; ins.ep = ep; ins.st = st;
        // (x and adj: once grown, below)
        // (L + T: the pool slots of an out-edge prune with mates)
        HIPANN_REQUIRE((int64_t)bmax * (L + T) < INT32_MAX, "add_rows: batch_max too large");
        // pctr: [0..3] the prunes' counters, [4] mate ids written, [5] (int) the non-finite flag
        ins.size("add_rows", bmax, L, n1, 48, dev);
        {  // the traversal's own scratch at its largest (resident_search_locked sizes it the same way)
            const int64_t vwords = (n1 + 31) / 32;
            const int64_t per = std::max<int64_t>(1, std::min<int64_t>(bmax, ((int64_t)2 << 30) / (vwords * 4)));
            db->visited.ensure((size_t)per * vwords * 4, dev);
            db->flags.ensure((size_t)bmax * 4, dev);
            db->bstats.ensure(72, dev);
            db->eps_dev.ensure(4, dev);
        }
        db->adj_host.reserve((size_t)n1 * R);
        // rows, adjacency and repeated-id bits with room for n1 rows: in place, or grown copies swapped in below
        DevBuf gdata, gadj, gdupw;
        const size_t w0 = (size_t)((n0 + 31) / 32), w1 = (size_t)((n1 + 31) / 32);
        float *x = static_cast<float *>(grow_keep(db->data, gdata, (size_t)n1 * d * 4 + 16, (size_t)n0 * d * 4, dev, st));
        uint32_t *adj =
            static_cast<uint32_t *>(grow_keep(db->adj_dev, gadj, (size_t)n1 * R * 4 + 16, (size_t)n0 * R * 4, dev, st));
        uint32_t *dupw = static_cast<uint32_t *>(grow_keep(db->dupw, gdupw, w1 * 4 + 16, w0 * 4, dev, st));
        ins.x = x; ins.adj = adj;
        // the tails no search reads yet: the new rows, empty adjacency rows, clear bits (the bits past n0 in word
        // w0 − 1 are clear already)
        HIPANN_CHECK(hipMemcpyAsync(x + (size_t)n0 * d, rows, (size_t)m * d * 4, hipMemcpyHostToDevice, st));
        HIPANN_CHECK(hipMemsetAsync(adj + (size_t)n0 * R, 0xff, (size_t)m * R * 4, st));
        if (w1 > w0) HIPANN_CHECK(hipMemsetAsync(dupw + w0, 0, (w1 - w0) * 4, st));
        HIPANN_CHECK(hipMemsetAsync(ins.pctr.p, 0, 48, st));
        launch_vamana_check_finite(x + (size_t)n0 * d, m * (int64_t)d, ins.pctr.get<int>() + 10, st);
        int bad = 0;
        HIPANN_CHECK(hipMemcpyAsync(&bad, ins.pctr.get<int>() + 10, 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        HIPANN_REQUIRE(!bad, "add_rows: rows hold a non-finite value");

        // ---- from here on the handle changes; a failure leaves it without a graph (it cannot be rolled back) ----
        struct Guard {
            DiskDB *db;
            int64_t n0;
            bool armed = true;
            ~Guard() {
                if (!armed) return;
                db->n = n0;
                db->R = 0;
                db->adj_host.clear();
                db->adj_host_stale = false;
            }
        } guard{db, n0};
        if (gdata.p) swap_buf(db->data, gdata);
        if (gadj.p) swap_buf(db->adj_dev, gadj);
        if (gdupw.p) swap_buf(db->dupw, gdupw);
        gdata.release();
        gadj.release();
        gdupw.release();
        const uint32_t eps1[1] = {ep};
        int64_t c = n0;  // rows in the graph
        while (c < n1) {
            const int b = (int)std::min<int64_t>(std::min<int64_t>(bmax, c), n1 - c);
            const int K = (int)std::min<int64_t>(L, c);
            db->n = c;  // the searches see the graph as it stands at the batch's start
            // search
            auto t0 = clk::now();
            int64_t sst[4] = {0, 0, 0, 0};
            resident_search_locked(db, eps1, 1, x + (size_t)c * d, b, K, K, metric, ins.sid.get<int64_t>(),
                                   ins.sd.get<float>(), sst, st);
            s8[0] += sst[0];
            s8[4] += sst[3];
            secs[0] += since(t0);
            // mates
            const bool with_mates = T > 0 && b > 1;
            if (with_mates) {
                auto tm = clk::now();
                launch_vamana_batch_mates(x + (size_t)c * d, b, d, (uint32_t)c, T, metric, ins.nrm.get<float>(),
                                          ins.mates.get<uint32_t>(), ins.pctr.get<unsigned long long>() + 4, st);
                HIPANN_CHECK(hipStreamSynchronize(st));
                secs[1] += since(tm);
            }
            // (the targets are rows c .. c + b − 1: insertion order c − 1 + i with the entry point below)
            ins.step((uint32_t)(c - 1), b, K, c + b, with_mates, secs + 2);
            db->adj_host_stale = true;
            s8[1] += 1;
            s8[2] += b;
            c += b;
        }
        ins.queue_counters(5);
        // the repeated-id row bits of all rows (one pass over the adjacency; no pruned or appended row repeats an id)
        launch_diskann_dup_rows(adj, R, n1, dupw, st);
        HIPANN_CHECK(hipStreamSynchronize(st));
        ins.counters_to_stats(s8);
        s8[7] = (int64_t)ins.pc[4];
        db->adj_host.resize((size_t)n1 * R);  // (reserved above: cannot throw)
        db->n = n1;
        guard.armed = false;
        // the host copy stays behind (the next host re-run refreshes it) unless the caller wants the graph
        if (adjacency_out) {
            refresh_adj_host(db, st);
            s8[6] = unreached_rows(db->adj_host, n1, R, ep);
            std::memcpy(adjacency_out, db->adj_host.data(), (size_t)n1 * R * 4);
        }
        if (stats) std::memcpy(stats, s8, sizeof(s8));
        for (int i = 0; i < 4; ++i) db->add_s[i] = secs[i];
        return n1;
    });
}

int diskann_hip_batch_mates(void *h, int64_t row0, int b, int T, uint32_t *out, char *eb, int el) {
    return abi_call(eb, el, [&] {
        HIPANN_REQUIRE(h, "batch_mates: null db");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        build_shape_check(db, 1, 1.0f, db->graph_metric, "batch_mates");
        HIPANN_REQUIRE(T >= 1 && T <= 64, "batch_mates: T must be in [1, 64]");
        HIPANN_REQUIRE(row0 >= 0 && b >= 0 && row0 + b <= db->n, "batch_mates: rows out of range");
        HIPANN_REQUIRE(b == 0 || out, "batch_mates: null out");
        if (b == 0) return 0;
        DeviceGuard g(db->device);
        const hipStream_t st = db->stream;
        DevBuf nrm, od;
        nrm.ensure((size_t)b * 4, db->device);
        od.ensure((size_t)b * T * 4, db->device);
        launch_vamana_batch_mates(db->data.get<float>() + (size_t)row0 * db->dim, b, db->dim, (uint32_t)row0, T,
                                  db->graph_metric, nrm.get<float>(), od.get<uint32_t>(), nullptr, st);
        HIPANN_CHECK(hipMemcpyAsync(out, od.p, (size_t)b * T * 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}

int diskann_hip_add_phase_seconds(void *h, double *seconds) { return phase_seconds(h, seconds, &DiskDB::add_s); }

// ---- row removal from the device graph (kernels in diskann_remove.hip) ----
int64_t diskann_hip_remove_ids(void *h, const int64_t *labels, int64_t n_labels, float alpha, int metric,
                               uint32_t *entry_point, int64_t scratch_words, uint32_t *adjacency_out, int64_t *stats,
                               char *eb, int el) {
    return abi_call(eb, el, [&]() -> int64_t {
        HIPANN_REQUIRE(h, "remove_ids: null db");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        HIPANN_REQUIRE(db->R > 0, "remove_ids: no graph registered (diskann_hip_register_graph / _build_graph)");
        build_shape_check(db, db->R, alpha, metric, "remove_ids");
        HIPANN_REQUIRE(entry_point, "remove_ids: null entry_point");
        HIPANN_REQUIRE(n_labels >= 0 && (n_labels == 0 || labels) && scratch_words >= 0, "remove_ids: bad arguments");
        HIPANN_REQUIRE((int64_t)*entry_point < db->n, "remove_ids: entry_point must be below n");
        const int64_t n = db->n;
        const int R = db->R, d = db->dim, dev = db->device;
        const uint32_t ep = *entry_point;
        int64_t s8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        // D: the distinct labels in range
        std::vector<uint32_t> dead;
        for (int64_t i = 0; i < n_labels; ++i)
            if (labels[i] >= 0 && labels[i] < n) dead.push_back((uint32_t)labels[i]);
        std::sort(dead.begin(), dead.end());
        dead.erase(std::unique(dead.begin(), dead.end()), dead.end());
        const int64_t nd = (int64_t)dead.size(), n2 = n - nd;
        if (nd == 0) {  // nothing moves
            if (db->adj_host_stale) {  // (add_rows leaves the host copy behind)
                DeviceGuard g(db->device);
                refresh_adj_host(db, db->stream);
            }
            s8[6] = unreached_rows(db->adj_host, n, R, ep);
            if (adjacency_out) std::memcpy(adjacency_out, db->adj_host.data(), (size_t)n * R * 4);
            if (stats) std::memcpy(stats, s8, sizeof(s8));
            return 0;
        }
        HIPANN_REQUIRE(n2 > 0, "remove_ids: every row would be removed");
        DeviceGuard g(db->device);
        RoctxRange rr("hipann.diskann.remove_ids");
        const hipStream_t st = db->stream;
        double secs[3] = {0.0, 0.0, 0.0};
        KernelTimer fill_ev, prune_ev;  // device time of the slabs' pool fills and prunes (read after the last sync)
        fill_ev.reset(true, db->device);
        prune_ev.reset(true, db->device);
        const auto t_call = clk::now();
        const float *x = db->data.get<float>();
        const uint32_t *adj = db->adj_dev.get<uint32_t>();

        // 1. mark, rank, and every live row's count of removed neighbours
        auto t0 = clk::now();
        const int64_t words = (n + 31) / 32;
        DevBuf lab, bits, wpre, sums, nrem, radj, ctr;
        lab.ensure((size_t)n_labels * 8, dev);
        bits.ensure((size_t)words * 4, dev);
        wpre.ensure((size_t)words * 4, dev);
        sums.ensure((size_t)diskann_remove_scan_blocks(n) * 4, dev);
        nrem.ensure((size_t)n, dev);
        radj.ensure((size_t)n * R * 4 + 16, dev);
        ctr.ensure(32, dev);
        HIPANN_CHECK(hipMemcpyAsync(lab.p, labels, (size_t)n_labels * 8, hipMemcpyHostToDevice, st));
        launch_diskann_remove_mark(lab.get<int64_t>(), n_labels, n, bits.get<uint32_t>(), wpre.get<uint32_t>(),
                                   sums.get<uint32_t>(), st);
        launch_diskann_remove_pool_len(adj, R, n, bits.get<uint32_t>(), nrem.get<uint8_t>(), st);
        // the repaired graph in the old id space: the stored rows, the pruned ones written over them
        HIPANN_CHECK(hipMemcpyAsync(radj.p, adj, (size_t)n * R * 4, hipMemcpyDeviceToDevice, st));
        HIPANN_CHECK(hipMemsetAsync(ctr.p, 0, 32, st));
        std::vector<uint8_t> hrem((size_t)n);
        HIPANN_CHECK(hipMemcpyAsync(hrem.data(), nrem.p, (size_t)n, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        // slabs of affected rows whose pool slots fit the budget (a row over the budget takes a slab alone)
        const int64_t budget = std::min<int64_t>(scratch_words > 0 ? scratch_words : (int64_t)1 << 28, 0x7fff0000);
        std::vector<uint32_t> tg;
        std::vector<int> pbeg, plen;
        std::vector<int64_t> slab_at{0};
        int64_t used = 0, pool_words = 0, slab_rows = 0;
        for (int64_t p = 0; p < n; ++p) {
            if (!hrem[p]) continue;
            const int len = R * (1 + (int)hrem[p]);
            if (used > 0 && used + len > budget) {
                slab_at.push_back((int64_t)tg.size());
                used = 0;
            }
            tg.push_back((uint32_t)p);
            pbeg.push_back((int)used);
            plen.push_back(len);
            used += len;
            pool_words = std::max(pool_words, used);
        }
        slab_at.push_back((int64_t)tg.size());
        const int64_t na = (int64_t)tg.size();
        for (size_t s = 0; s + 1 < slab_at.size(); ++s) slab_rows = std::max(slab_rows, slab_at[s + 1] - slab_at[s]);
        secs[0] += since(t0);
        if (na > 0) {
            DevBuf dtg, dbeg, dlen, pool, gram;
            dtg.ensure((size_t)na * 4, dev);
            dbeg.ensure((size_t)na * 4, dev);
            dlen.ensure((size_t)na * 4, dev);
            pool.ensure((size_t)pool_words * 4, dev);
            const int blocks = vamana_prune_blocks(slab_rows);
            gram.ensure(vamana_gram_bytes(blocks), dev);
            HIPANN_CHECK(hipMemcpyAsync(dtg.p, tg.data(), (size_t)na * 4, hipMemcpyHostToDevice, st));
            HIPANN_CHECK(hipMemcpyAsync(dbeg.p, pbeg.data(), (size_t)na * 4, hipMemcpyHostToDevice, st));
            HIPANN_CHECK(hipMemcpyAsync(dlen.p, plen.data(), (size_t)na * 4, hipMemcpyHostToDevice, st));
            unsigned long long *c64 = ctr.get<unsigned long long>();
            PruneArgs pa;  // every slab's prune: its pools in `pool`, the pruned rows written over radj's
            pa.x = x; pa.d = d; pa.n = (uint32_t)n; pa.R = R; pa.alpha = alpha; pa.metric = metric;
            pa.pool32 = pool.get<uint32_t>();
            pa.out = radj.get<uint32_t>(); pa.out_by_target = 1; pa.gram = gram.get<float>(); pa.counters = c64;
            // the stream orders fill, prune and the next slab's reuse of `pool`; events split the device time
            for (size_t s = 0; s + 1 < slab_at.size(); ++s) {
                const int64_t a0 = slab_at[s];
                const int cnt = (int)(slab_at[s + 1] - a0);
                if (cnt <= 0) continue;
                {
                    ScopedTiming tm(fill_ev, st);
                    launch_diskann_remove_pool_fill(adj, R, n, bits.get<uint32_t>(), dtg.get<uint32_t>() + a0,
                                                    dbeg.get<int>() + a0, dlen.get<int>() + a0, cnt,
                                                    pool.get<uint32_t>(), c64 + 2, st);
                }
                {
                    ScopedTiming tm(prune_ev, st);
                    pa.targets = dtg.get<uint32_t>() + a0; pa.m = cnt;
                    pa.pool_beg = dbeg.get<int>() + a0; pa.pool_len = dlen.get<int>() + a0;
                    launch_vamana_prune(pa, blocks, st);
                }
                s8[4] += 1;
            }
        }
        // 2. the entry point: relabelled, or replaced by the nearest live row before the rows move
        uint32_t nep = ep;
        unsigned long long hc[4] = {0, 0, 0, ~0ull};
        if (std::binary_search(dead.begin(), dead.end(), ep)) {
            HIPANN_CHECK(hipMemsetAsync(ctr.get<unsigned long long>() + 3, 0xff, 8, st));
            launch_diskann_remove_nearest(x, d, n, bits.get<uint32_t>(), ep, metric,
                                          ctr.get<unsigned long long>() + 3, st);
            s8[5] = 1;
        }
        // 3. compact into fresh buffers: rows, adjacency (ids replaced by their ranks), repeated-id row bits
        DevBuf src, nx, nadj, ndupw;
        std::vector<uint32_t> nhost((size_t)n2 * R);
        src.ensure((size_t)n2 * 8, dev);
        nx.ensure((size_t)n2 * d * 4 + 16, dev);
        nadj.ensure((size_t)n2 * R * 4 + 16, dev);
        ndupw.ensure((size_t)((n2 + 31) / 32) * 4 + 16, dev);
        launch_diskann_remove_sources(bits.get<uint32_t>(), wpre.get<uint32_t>(), n, src.get<int64_t>(), st);
        launch_flat_gather_rows(x, src.get<int64_t>(), n2, d, nx.get<float>(), st);
        launch_diskann_remove_compact_adj(radj.get<uint32_t>(), R, n, bits.get<uint32_t>(), wpre.get<uint32_t>(),
                                          nadj.get<uint32_t>(), st);
        launch_diskann_dup_rows(nadj.get<uint32_t>(), R, n2, ndupw.get<uint32_t>(), st);
        HIPANN_CHECK(hipMemcpyAsync(nhost.data(), nadj.p, (size_t)n2 * R * 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipMemcpyAsync(hc, ctr.p, 32, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        if (s8[5]) {
            HIPANN_REQUIRE(hc[3] != ~0ull, "remove_ids: no live row found for the entry point");
            nep = (uint32_t)(hc[3] & 0xffffffffull);
        }
        nep -= (uint32_t)(std::lower_bound(dead.begin(), dead.end(), nep) - dead.begin());
        s8[0] = nd;
        s8[1] = (int64_t)hc[0];
        s8[2] = (int64_t)hc[1];
        s8[3] = (int64_t)hc[2];
        s8[6] = unreached_rows(nhost, n2, R, nep);
        // phases: host time up to the slab plan plus the fills' device time; the prunes' device time; the rest
        secs[0] += fill_ev.average_ms() * (double)fill_ev.used * 1e-3;
        secs[1] = prune_ev.average_ms() * (double)prune_ev.used * 1e-3;
        secs[2] = std::max(0.0, since(t_call) - secs[0] - secs[1]);
        // everything is built: swap it in
        swap_buf(db->data, nx);
        swap_buf(db->adj_dev, nadj);
        swap_buf(db->dupw, ndupw);
        db->adj_host.swap(nhost);
        db->adj_host_stale = false;
        db->n = n2;
        *entry_point = nep;
        if (adjacency_out) std::memcpy(adjacency_out, db->adj_host.data(), (size_t)n2 * R * 4);
        if (stats) std::memcpy(stats, s8, sizeof(s8));
        for (int i = 0; i < 3; ++i) db->remove_s[i] = secs[i];
        return nd;
    });
}

int diskann_hip_remove_phase_seconds(void *h, double *seconds) { return phase_seconds(h, seconds, &DiskDB::remove_s); }

int diskann_hip_robust_prune(void *h, const uint32_t *targets, int m, const uint32_t *pools, int pool_cap, int R,
                             float alpha, int metric, uint32_t *out, char *eb, int el) {
    return abi_call(eb, el, [&] {
        HIPANN_REQUIRE(h, "robust prune: null db");
        auto *db = static_cast<DiskDB *>(h);
        std::lock_guard<std::mutex> lk(db->mu);
        build_shape_check(db, R, alpha, metric);
        HIPANN_REQUIRE(m >= 0 && pool_cap >= 1 && (m == 0 || (targets && pools && out)), "robust prune: bad arguments");
        for (int i = 0; i < m; ++i) HIPANN_REQUIRE((int64_t)targets[i] < db->n, "robust prune: target id out of range");
        if (m == 0) return 0;
        DeviceGuard g(db->device);
        const hipStream_t st = db->stream;
        const int dev = db->device;
        DevBuf tg, pl, od, gram;
        const size_t pw = (size_t)m * pool_cap;
        tg.ensure((size_t)m * 4, dev);
        pl.ensure(pw * 4, dev);
        od.ensure((size_t)m * R * 4, dev);
        const int blocks = vamana_prune_blocks(m);
        gram.ensure(vamana_gram_bytes(blocks), dev);
        HIPANN_CHECK(hipMemcpyAsync(tg.p, targets, (size_t)m * 4, hipMemcpyHostToDevice, st));
        HIPANN_CHECK(hipMemcpyAsync(pl.p, pools, pw * 4, hipMemcpyHostToDevice, st));
        PruneArgs pa;  // target t's pool is pools[t·pool_cap ..], its row out[t·R ..]
        pa.x = db->data.get<float>(); pa.d = db->dim; pa.n = (uint32_t)db->n; pa.R = R; pa.alpha = alpha;
        pa.metric = metric;
        pa.targets = tg.get<uint32_t>(); pa.m = m; pa.pool32 = pl.get<uint32_t>(); pa.pool_cap = pool_cap;
        pa.out = od.get<uint32_t>(); pa.gram = gram.get<float>();
        launch_vamana_prune(pa, blocks, st);
        HIPANN_CHECK(hipMemcpyAsync(out, od.p, (size_t)m * R * 4, hipMemcpyDeviceToHost, st));
        HIPANN_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}

}  // extern "C"
