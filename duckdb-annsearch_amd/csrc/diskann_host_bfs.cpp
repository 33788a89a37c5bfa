// diskann_host_bfs.cpp — the host-driven lock-step BFS of DiskProvider::search_batch (disk_provider.rs:470-652): the
// body of diskann_hip_search_batch and the fallback of the resident search for the queries it flags (diskann.hip).
// Host state (heaps, result lists, visited sets) as in the reference; one id-gather launch per lock-step iteration
// (launch_ids, diskann.hip).  host_bfs resolves a plan once and runs the stages below; no stage reads the environment.
#include "diskann_db.hpp"
#include "diskann_kernels.hpp"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>

namespace hipann {
namespace {

struct Cand {
    float d;
    uint32_t id;
};
struct CandGreater {  // min-heap on (d, id): BinaryHeap<Reverse<(FloatOrd, u32)>>
    bool operator()(const Cand &a, const Cand &b) const { return a.d > b.d || (a.d == b.d && a.id > b.id); }
};

// Rust slice::binary_search_by (std ≥ 1.82) with partial_cmp on distance; returns the insert position.
size_t rust_binary_search(const std::vector<Cand> &res, float dist) {
    size_t size = res.size();
    if (size == 0) return 0;
    size_t base = 0;
    while (size > 1) {
        const size_t half = size / 2, mid = base + half;
        base = (res[mid].d > dist) ? base : mid;
        size -= half;
    }
    const float p = res[base].d;
    if (!(p < dist) && !(p > dist)) return base;
    return base + (p < dist ? 1 : 0);
}

// Visited set: open addressing over u32 ids (linear probing, power-of-two capacity, load ≤ 1/2).
// Same membership semantics as the reference's hashbrown::HashSet<u32>; only speed differs.
struct VisitedSet {
    std::vector<uint32_t> slot;  // kEmpty = unused
    uint32_t mask = 0;
    size_t count = 0;
    static constexpr uint32_t kEmpty = 0xffffffffu;
    void init(size_t expect) {
        size_t cap = 64;
        while (cap < 2 * expect) cap <<= 1;
        slot.assign(cap, kEmpty);
        mask = (uint32_t)(cap - 1);
        count = 0;
    }
    static uint32_t hash(uint32_t v) { return (v * 0x9E3779B1u) ^ (v >> 15); }
    void prefetch(uint32_t v) const { __builtin_prefetch(slot.data() + (hash(v) & mask), 1); }
    // Returns true if v was newly inserted (HashSet::insert).  v == kEmpty is stored out of band.
    bool insert(uint32_t v) {
        if (v == kEmpty) {
            const bool fresh = !has_max;
            has_max = true;
            return fresh;
        }
        if (2 * (count + 1) > slot.size()) grow();
        uint32_t i = hash(v) & mask;
        for (;;) {
            const uint32_t x = slot[i];
            if (x == v) return false;
            if (x == kEmpty) { slot[i] = v; ++count; return true; }
            i = (i + 1) & mask;
        }
    }
    bool has_max = false;

  private:
    void grow() {
        std::vector<uint32_t> old;
        old.swap(slot);
        slot.assign(old.size() * 2, kEmpty);
        mask = (uint32_t)(slot.size() - 1);
        for (uint32_t v : old) {
            if (v == kEmpty) continue;
            uint32_t i = hash(v) & mask;
            while (slot[i] != kEmpty) i = (i + 1) & mask;
            slot[i] = v;
        }
    }
};

struct QState {
    VisitedSet visited;
    std::vector<Cand> cands;  // binary min-heap on (d, id) (CandGreater): BinaryHeap<Reverse<..>>
    std::vector<Cand> result;  // sorted by d, at most l entries
    bool active = true;
    int nnew = 0;  // candidates this query put into the current lock-step batch
};

// insert_result (disk_provider.rs:656-678).  (d, id) pairs in `cands` are unique (ids pass the
// visited set once), so any binary heap pops them in the same order as Rust's BinaryHeap.
void insert_result(QState &s, size_t l, float dist, uint32_t nb) {
    if (s.result.size() < l || dist < s.result.back().d) {
        const size_t pos = rust_binary_search(s.result, dist);
        s.result.insert(s.result.begin() + (ptrdiff_t)pos, Cand{dist, nb});
        if (s.result.size() > l) s.result.resize(l);
        s.cands.push_back(Cand{dist, nb});
        std::push_heap(s.cands.begin(), s.cands.end(), CandGreater());
    }
}

// Fork-join pool for the per-step host phases of the lock-step BFS: the calling thread is worker 0,
// the others spin on a generation counter (the phases are ~0.1 ms apart, too short for a futex
// round trip) and exit when the search returns.
class SpinPool {
  public:
    explicit SpinPool(int nthreads) : n_(nthreads < 1 ? 1 : nthreads) {
        for (int t = 1; t < n_; ++t) th_.emplace_back([this, t] { worker(t); });
    }
    ~SpinPool() {
        stop_.store(true, std::memory_order_release);
        gen_.fetch_add(1, std::memory_order_acq_rel);
        for (auto &t : th_) t.join();
    }
    int size() const { return n_; }
    // Runs fn(tid) on every worker and returns when all have finished.  Exceptions must not escape fn.
    template <typename F> void run(F &&fn) {
        if (n_ == 1) { fn(0); return; }
        std::function<void(int)> job(fn);
        job_ = &job;
        pending_.store(n_ - 1, std::memory_order_release);
        gen_.fetch_add(1, std::memory_order_acq_rel);
        fn(0);
        while (pending_.load(std::memory_order_acquire) != 0) spin_pause();
        job_ = nullptr;
    }

  private:
    static void spin_pause() { __builtin_ia32_pause(); }
    void worker(int tid) {
        uint64_t seen = 0;
        for (;;) {
            uint64_t g;
            int idle = 0;
            while ((g = gen_.load(std::memory_order_acquire)) == seen) {
                spin_pause();
                if (++idle > 4096) { std::this_thread::yield(); idle = 0; }
            }
            seen = g;
            if (stop_.load(std::memory_order_acquire)) return;
            (*job_)(tid);
            pending_.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
    int n_;
    std::vector<std::thread> th_;
    std::atomic<uint64_t> gen_{0};
    std::atomic<int> pending_{0};
    std::atomic<bool> stop_{false};
    std::function<void(int)> *job_ = nullptr;
};

int bfs_threads(int nq) {
    int t = 16;  // the GPU box's CPU share per GPU
    if (const char *e = std::getenv("HIPANN_BFS_THREADS")) t = std::atoi(e);
    const int hw = (int)std::thread::hardware_concurrency();
    if (hw > 0) t = std::min(t, hw);
    t = std::min(t, std::max(1, nq / 16));  // ≥ 16 queries per thread
    return std::max(1, t);
}

int bfs_groups(int nq) {
    // two pipelined groups: the GPU gathers one group's distances while the host threads run the other's inserts and
    // expansions (C4 host path, 16 threads: 1 group 34.8K QPS with 9.6 ms of GPU waits per batch, 2 groups 39.9K with
    // 0.5 ms, profiles/r05/diskann_host_bfs_r05.txt); HIPANN_BFS_GROUPS=1..8 for A/B
    int g = 2;
    if (const char *e = std::getenv("HIPANN_BFS_GROUPS")) g = std::atoi(e);
    g = std::min(g, std::max(1, nq / 64));  // ≥ 64 queries per group
    return std::max(1, std::min(g, 8));
}

// What one batch runs with, resolved once.
// Fixed per-query slot layout: query qi owns slots [qi*S, qi*S + S) of every lock-step batch, S = max(R, n_ep); unused
// slots hold UINT32_MAX and the kernel skips them.  The query map is therefore constant (uploaded once) and the host
// phases run per query in parallel with no compaction step.  Per query the candidate order is the reference's
// (neighbour order).
struct BfsPlan {
    size_t l;        // result-list length, max(l_search, k)
    size_t S, cap;   // slots per query, slots per batch (nq * S)
    int T, G;        // host threads, pipelined groups
    int64_t vwords;  // visited words per query (device sets)
    // The visited sets live on the device (default): the id-gather kernel sets each candidate's bit and skips the ones
    // already set, so the host phases never probe a per-query hash set (≈ 6K ids, 32-64 KB per query: a cache miss
    // per neighbour).  The host hands over every valid neighbour of the expanded row; an already-visited one comes
    // back as kVisitedBits and is dropped.  HIPANN_BFS_GPU_VISITED=0 (A/B), or more than 1 GiB of bits: the host sets.
    bool gv;
    bool prof;  // HIPANN_BFS_PROF=1 (tuning): host time in the GPU waits, the host phases and the launches, on stderr
};

BfsPlan resolve_plan(const DiskDB &db, int R, int n_ep, int nq, int k, int l_search) {
    static const bool gv_env = [] { const char *e = std::getenv("HIPANN_BFS_GPU_VISITED"); return !e || std::atoi(e); }();
    static const bool prof = std::getenv("HIPANN_BFS_PROF") != nullptr;
    BfsPlan p;
    p.l = (size_t)std::max(l_search, k);
    p.S = (size_t)std::max(R, n_ep);
    p.cap = (size_t)nq * p.S;
    HIPANN_REQUIRE(p.cap <= (size_t)INT32_MAX, "nq * max(R, n_ep) exceeds INT32_MAX");
    p.T = bfs_threads(nq);
    p.G = bfs_groups(nq);
    p.vwords = ((int64_t)(uint32_t)db.n + 31) / 32;
    p.gv = gv_env && (int64_t)nq * p.vwords * 4 <= ((int64_t)1 << 30);
    p.prof = prof;
    return p;
}

bool visited_mark(float v) { return __builtin_bit_cast(uint32_t, v) == kVisitedBits; }

// The device marks each slot's candidate with one atomic, in no order among the slots of a launch: of an id that a
// row (or the entry points) holds twice, either slot could come back as the fresh one.  The reference's visited
// insert runs in neighbour order — the first occurrence wins, and with it the candidate's place among this step's
// inserts — so a repeated id goes over once, in its first slot.
// (`seen`: a 256-bit filter over the ids already in `slot`; a clear bit proves the id new, a set one is checked.)
void push_once(uint32_t *slot, int &cnt, uint32_t id, uint64_t (&seen)[4]) {
    const uint32_t h = (id * 0x9E3779B1u) >> 24;
    uint64_t &w = seen[h >> 6];
    const uint64_t bit = 1ull << (h & 63);
    if (w & bit)
        for (int j = 0; j < cnt; ++j)
            if (slot[j] == id) return;
    w |= bit;
    slot[cnt++] = id;
}

// The queries run in G groups (2 by default), each its own lock-step loop, pipelined: while the GPU gathers group
// g's distances, the host threads insert and expand group g+1's.  A query's trajectory depends only on its own
// state, so grouping changes no result; the batch's step count (the reference's loop iterations) is the largest
// group's.
struct Group {
    int q0 = 0, q1 = 0;
    bool seed = true, done = false, launched = false;
    int64_t steps = 0;
    hipEvent_t ev = nullptr;
};

struct HostBfs {
    DiskDB *db;
    const uint32_t *adj, *eps;
    const int R, n_ep, nq, metric;
    const uint32_t N;
    const BfsPlan p;
    const hipStream_t st;
    uint32_t *hid = nullptr;            // the step's ids, pinned; the gather reads them through hid_dev
    const unsigned *hid_dev = nullptr;
    float *hout = nullptr, *hout_dev = nullptr;  // the step's distances, pinned; the gather writes through hout_dev
    unsigned *vbits = nullptr;
    std::vector<QState> Sq;
    std::vector<Group> grp;
    SpinPool pool;
    std::vector<int64_t> red;  // per-thread head counts and evaluations, padded against false sharing
    int64_t nevals = 0, ncalls = 0;

    HostBfs(DiskDB *db_, const uint32_t *adj_, int R_, const uint32_t *eps_, int n_ep_, int nq_, int metric_,
            const BfsPlan &plan)
        : db(db_), adj(adj_), eps(eps_), R(R_), n_ep(n_ep_), nq(nq_), metric(metric_), N((uint32_t)db_->n), p(plan),
          st(db_->stream), Sq((size_t)nq_), grp((size_t)plan.G), pool(plan.T), red((size_t)plan.T * 8, 0) {}
    ~HostBfs() {
        for (auto &g : grp)
            if (g.ev) (void)hipEventDestroy(g.ev);
    }

    // Staging: the queries and the constant query map on the device, the pinned id and distance buffers with their
    // device mappings, the visited bits, the groups with their events.
    void stage(const float *queries) {
        const size_t cap = p.cap;
        db->q.ensure((size_t)nq * db->dim * 4 + 16, db->device);
        HIPANN_CHECK(hipMemcpyAsync(db->q.p, queries, (size_t)nq * db->dim * 4, hipMemcpyHostToDevice, st));
        db->m.ensure(cap * 4, db->device);
        db->hids.ensure(cap * 4);
        db->hm.ensure(cap * 4);
        db->hout.ensure(cap * 4);
        hid = db->hids.get<uint32_t>();
        uint32_t *hm = db->hm.get<uint32_t>();
        hout = db->hout.get<float>();
        // the distances go straight into the pinned host buffer through its device mapping (posted writes: no
        // device-to-host copy and its round trip per step), and the kernel reads the step's ids from theirs
        hout_dev = static_cast<float *>(host_device_ptr(hout));
        hid_dev = static_cast<const unsigned *>(host_device_ptr(hid));
        for (size_t i = 0; i < cap; ++i) hm[i] = (uint32_t)(i / p.S);
        HIPANN_CHECK(hipMemcpyAsync(db->m.p, hm, cap * 4, hipMemcpyHostToDevice, st));
        if (p.gv) {
            db->vbits.ensure((size_t)nq * p.vwords * 4, db->device);
            HIPANN_CHECK(hipMemsetAsync(db->vbits.p, 0, (size_t)nq * p.vwords * 4, st));
            vbits = db->vbits.get<unsigned>();
        }
        for (int g = 0; g < p.G; ++g) {
            grp[g].q0 = (int)((int64_t)nq * g / p.G);
            grp[g].q1 = (int)((int64_t)nq * (g + 1) / p.G);
            HIPANN_CHECK(hipEventCreateWithFlags(&grp[g].ev, hipEventDisableTiming));
        }
    }

    // Seeding: the entry points into every query's slots (disk_provider.rs:524-538).
    void seed() {
        pool.run([&](int t) {
            const int q0 = (int)((int64_t)nq * t / p.T), q1 = (int)((int64_t)nq * (t + 1) / p.T);
            for (int qi = q0; qi < q1; ++qi) {
                QState &s = Sq[qi];
                if (!p.gv) s.visited.init(std::max<size_t>(p.l * 2, 1024));
                s.cands.reserve(p.l * 2);
                s.result.reserve(p.l + 1);
                uint32_t *slot = hid + (size_t)qi * p.S;
                int cnt = 0;
                uint64_t seen[4] = {0, 0, 0, 0};
                for (int e = 0; e < n_ep; ++e) {
                    const uint32_t ep = eps[e];
                    if (p.gv) {
                        if (ep < N) push_once(slot, cnt, ep, seen);
                    } else if (s.visited.insert(ep) && ep < N) {
                        slot[cnt++] = ep;
                    }
                }
                for (size_t j = (size_t)cnt; j < p.S; ++j) slot[j] = kNone;
                s.nnew = cnt;
            }
        });
    }

    // One group's launch: its slots with work (up to its last query with new candidates) through the id-gather kernel,
    // and the event the pipelined loop waits on.
    void launch(Group &g) {
        int last = g.q0;
        int64_t tot = 0;
        for (int qi = g.q0; qi < g.q1; ++qi)
            if (Sq[qi].nnew) { last = qi + 1; tot += Sq[qi].nnew; }
        g.launched = tot > 0;
        if (!tot) return;
        const size_t o = (size_t)g.q0 * p.S, span = (size_t)(last - g.q0) * p.S;
        {
            ScopedTiming tm(db->timer, st);
            launch_ids(*db, db->q.get<float>(), hid_dev + o, db->m.get<unsigned>() + o, (int)span, metric, hout_dev + o,
                       st, vbits, p.vwords);
        }
        HIPANN_CHECK(hipEventRecord(g.ev, st));
        ncalls++;
        if (!p.gv) nevals += tot;  // (gv: the first visits, counted as the phases read them)
    }

    // One query's absorb step: the results of its last GPU call — the seeds' into cands + result (disk_provider.rs:
    // 524-538), later steps' through insert_result (:656-678).  A slot that comes back as kVisitedBits (a repeated
    // entry point, an already-visited neighbour) is dropped.  Returns the distances taken.
    int64_t absorb(QState &s, const uint32_t *slot, const float *dd, bool seeds) const {
        int64_t evals = 0;
        for (int j = 0; j < s.nnew; ++j) {
            if (p.gv && visited_mark(dd[j])) continue;
            ++evals;
            if (seeds) {
                s.cands.push_back(Cand{dd[j], slot[j]});
                std::push_heap(s.cands.begin(), s.cands.end(), CandGreater());
                s.result.push_back(Cand{dd[j], slot[j]});
            } else {
                insert_result(s, p.l, dd[j], slot[j]);
            }
        }
        if (seeds)
            std::stable_sort(s.result.begin(), s.result.end(), [](const Cand &x, const Cand &y) { return x.d < y.d; });
        return evals;
    }

    // One query's loop head (disk_provider.rs:545-652): pop, stop rule, expansion of the popped row into the query's
    // slots (s.nnew of them).  The fork is how a neighbour is admitted: with device visited sets every valid neighbour
    // goes over once (push_once); with host sets a neighbour goes over when VisitedSet::insert takes it, the row's
    // valid neighbours first with their set slots prefetched — the set (≈ 6K ids, 32-64 KB per query) misses cache on
    // nearly every probe, and 64 overlapped misses cost about one.
    void head(QState &s, uint32_t *slot) const {
        if (s.cands.empty()) {
            s.active = false;
            return;
        }
        std::pop_heap(s.cands.begin(), s.cands.end(), CandGreater());
        const Cand c = s.cands.back();
        s.cands.pop_back();
        if (s.result.size() >= p.l && c.d > s.result[p.l - 1].d) {
            s.active = false;
            return;
        }
        const uint32_t *nbr = adj + (size_t)c.id * R;
        uint32_t nv[256];
        uint64_t seen[4] = {0, 0, 0, 0};
        int cnt = 0;
        bool end = false;
        for (int r0 = 0; r0 < R && !end; r0 += 256) {  // (rows wider than 256 in pieces)
            int m = 0;
            for (int r = r0; r < R && r < r0 + 256; ++r) {
                const uint32_t nb = nbr[r];
                if (nb == kNone) {  // get_neighbors trims at the first sentinel
                    end = true;
                    break;
                }
                if (nb >= N) continue;
                if (p.gv) {
                    push_once(slot, cnt, nb, seen);
                } else {
                    nv[m++] = nb;
                    s.visited.prefetch(nb);
                }
            }
            for (int j = 0; j < m; ++j)
                if (s.visited.insert(nv[j])) slot[cnt++] = nv[j];
        }
        s.nnew = cnt;
    }

    // One host phase of a group: every query absorbs its last results and runs its loop head, a static 1/T range of
    // the group per thread (a query's state stays in one core's caches only when the same thread keeps it).
    // Returns the loop-head active count.
    int64_t phase(Group &g) {
        const int n = g.q1 - g.q0;
        const bool seeds = g.seed;
        pool.run([&](int t) {
            int64_t heads = 0, evals = 0;
            const int q0 = g.q0 + (int)((int64_t)n * t / p.T), q1 = g.q0 + (int)((int64_t)n * (t + 1) / p.T);
            for (int qi = q0; qi < q1; ++qi) {
                QState &s = Sq[qi];
                uint32_t *slot = hid + (size_t)qi * p.S;
                evals += absorb(s, slot, hout + (size_t)qi * p.S, seeds);
                const int prev = s.nnew;  // slots >= prev are already empty
                s.nnew = 0;
                heads += s.active ? 1 : 0;  // the reference's loop-head active count
                if (s.active) head(s, slot);
                for (int j = s.nnew; j < prev; ++j) slot[j] = kNone;
                // the adjacency row the next pop most likely takes (the heap's top now; the next step's inserts rarely
                // change it), into cache while the GPU computes this step's distances
                if (s.active && !s.cands.empty()) __builtin_prefetch(adj + (size_t)s.cands.front().id * R);
            }
            red[(size_t)t * 8] = heads;
            red[(size_t)t * 8 + 1] = evals;
        });
        g.seed = false;
        int64_t heads = 0;
        for (int t = 0; t < p.T; ++t) {
            heads += red[(size_t)t * 8];
            if (p.gv) nevals += red[(size_t)t * 8 + 1];
        }
        return heads;
    }

    // The pipelined loop: each live group in turn waits for its gather, runs its host phase and launches its next
    // step, until no query of it is active.  Returns the batch's step count.
    int64_t run() {
        using clk = std::chrono::steady_clock;
        auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        double t_wait = 0, t_phase = 0, t_launch = 0;
        const auto t_all = clk::now();
        for (int live = p.G; live > 0;) {
            for (auto &g : grp) {
                if (g.done) continue;
                const auto t0 = clk::now();
                if (g.launched) wait_event(g.ev);
                const auto t1 = clk::now();
                const int64_t heads = phase(g);
                const auto t2 = clk::now();
                if (p.prof) {
                    t_wait += us(t0, t1);
                    t_phase += us(t1, t2);
                }
                if (!heads) {
                    g.done = true;
                    --live;
                    continue;
                }
                g.steps++;
                launch(g);  // (nothing when no query of the group expanded new neighbours)
                if (p.prof) t_launch += us(t2, clk::now());
            }
        }
        if (p.prof)
            std::fprintf(stderr, "hipann bfs: nq %d groups %d threads %d calls %lld: total %.0f us, waits %.0f, phases %.0f, "
                                 "launches %.0f\n", nq, p.G, p.T, (long long)ncalls, us(t_all, clk::now()), t_wait, t_phase,
                         t_launch);
        int64_t nsteps = 0;
        for (auto &g : grp) nsteps = std::max(nsteps, g.steps);
        return nsteps;
    }

    // The copy-out: the first k of every result list, ids −1 / distances FLT_MAX past its end.
    void copy_out(int k, int64_t *out_ids, float *out_d) const {
        for (int qi = 0; qi < nq; ++qi) {
            const auto &r = Sq[qi].result;
            for (int j = 0; j < k; ++j) {
                const bool has = (size_t)j < r.size();
                out_ids[(size_t)qi * k + j] = has ? (int64_t)r[j].id : -1;
                out_d[(size_t)qi * k + j] = has ? r[j].d : FLT_MAX;
            }
        }
    }
};

}  // namespace

// (described where it is declared, diskann_db.hpp)
void host_bfs(DiskDB *db, const uint32_t *adj, int R, const uint32_t *eps, int n_ep, const float *queries, int nq,
              int k, int l_search, int metric, int64_t *out_ids, float *out_d, int64_t *stats) {
    if (stats) { stats[0] = stats[1] = stats[2] = stats[3] = 0; }
    if (nq == 0) return;
    HostBfs b(db, adj, R, eps, n_ep, nq, metric, resolve_plan(*db, R, n_ep, nq, k, l_search));
    b.stage(queries);
    b.seed();
    for (auto &g : b.grp) b.launch(g);
    const int64_t nsteps = b.run();
    b.copy_out(k, out_ids, out_d);
    if (stats) { stats[0] = b.nevals; stats[1] = nsteps; stats[2] = b.ncalls; }
}

}  // namespace hipann
