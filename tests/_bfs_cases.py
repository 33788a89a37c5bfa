"""Inputs for the exact tests of the GPU-resident DiskANN traversal (diskann_bfs.hip), and a Python model of the
search.  Pure numpy: nothing here touches the GPU, so tests/test_bfs_cases.py can hold every input to the oracle
on the CPU before tests/test_diskann_bfs_shapes_gpu.py relies on it.

Every builder makes small-integer (or dyadic) data: each term of a distance is a non-negative value that fp32 holds
exactly and every sum stays below 2^24, so a distance is the same float in any summation order — the oracle's
sequential sum, the kernel's lane-strided partials and its reduce-scatter butterfly must agree bit for bit.

A case is a dict: x (n, d) fp32 rows, qs (nq, d) fp32 queries, adj (n, R) uint32 adjacency (u32::MAX padding),
eps the entry points; rows 0..31 of the traversal cases are SQ8 calibration rows (see calibration_rows).
"""
from __future__ import annotations

import functools
import heapq

import numpy as np

NONE = 0xFFFFFFFF

# The shapes the GPU tests run, shared with the CPU checks of the same inputs.  launch_diskann_bfs picks the row
# template by chunks per lane (64 lanes x 8 SQ8 codes or 4 floats per chunk): fmt 1 (SQ8) T = 1..4 per 512 dims,
# fmt 0 (fp32) T = 1, 2, 4, 6, 8 at 256, 512, 1024, 1536, 2048 dims.
N, NQ = 2048, 48
WIDE_DIMS = {1: (520, 1024, 1544, 2048), 0: (260, 768, 1028, 1536, 1540, 2048)}
ONE_HOT_DIMS = {1: (8, 504, 512, 520, 1024, 1032, 1536, 1544, 2048),
                0: (4, 252, 256, 260, 512, 516, 768, 1024, 1028, 1536, 1540, 2048)}
DEPTH_D = 64


def calibration_rows(d):
    """32 rows, row r = 255 in the dims ≡ r (mod 32) and 0 elsewhere: with them in the data SQ8 training gives
    min 0 and range 255 in every dim (codes == values), and no single row is farther than (d/32)·255² away."""
    c = np.zeros((32, d), np.float32)
    for r in range(32):
        c[r, r::32] = 255.0
    return c


def knn_graph(x, kn):
    """The kn nearest other rows of every row (L2, exact integers in fp64; ties by id), from one x @ x.T."""
    x64 = x.astype(np.float64)
    n2 = (x64 * x64).sum(1)
    dm = n2[:, None] + n2[None, :] - 2.0 * (x64 @ x64.T)
    np.fill_diagonal(dm, np.inf)
    return np.argsort(dm, axis=1, kind="stable")[:, :kn]


def ragged_from_nn(nn, R, rng, extra_random=2):
    """A ragged adjacency over the neighbour table nn (n, ≥ R − extra_random − 2): sentinel padding after a varying
    degree, out-of-range ids, repeated ids — the visited / skip rules of disk_provider.rs:556-577."""
    n = len(nn)
    adj = np.full((n, R), NONE, np.uint32)
    adj[:, : R - extra_random - 2] = nn[:, : R - extra_random - 2]
    adj[:, R - extra_random - 2: R - 2] = rng.integers(0, n, (n, extra_random))
    adj[::7, R - 2] = n + 5          # out of range: skipped, not a sentinel
    adj[::5, 3] = adj[::5, 2]        # duplicate neighbour
    deg = rng.integers(R // 2, R + 1, n)
    adj[np.arange(R)[None, :] >= deg[:, None]] = NONE
    return adj


def _ragged_graph(oracle, x, R, rng, extra_random=2):
    _, nn = oracle.flat_search(x, x, R - extra_random - 2 + 1, 0)
    return ragged_from_nn(nn[:, 1:], R, rng, extra_random)


def repeat_first_last(adj, n, winner="first"):
    """Every row's first id again in its last slot before the sentinel (rows of degree ≥ 3): the same id twice in one
    expansion, far apart.  The reference's visited insert keeps the first occurrence.  winner="last" is the graph a
    search would see if the later occurrence won instead (the first one made an out-of-range id, which is skipped):
    the CPU checks use it to show that the two orders give different results on this input."""
    out = adj.copy()
    deg = np.where((adj == NONE).any(1), (adj == NONE).argmax(1), adj.shape[1])
    rows = np.flatnonzero((deg >= 3) & (adj[:, 0] < n))
    out[rows, deg[rows] - 1] = adj[rows, 0]
    if winner == "last":
        out[rows, 0] = n + 5
    return out


def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _sparse_rows(rng, m, d, nnz=12):
    out = np.zeros((m, d), np.float32)
    for i in range(m):
        out[i, rng.choice(d, min(nnz, d), replace=False)] = rng.integers(1, 256, min(nnz, d))
    return out


@functools.lru_cache(maxsize=None)
def wide_sparse(n, d, nq, seed):
    """No-tie regime: 12 random dims of 1..255 per row and per query, so nearly every L2 distance is distinct and a
    correct kernel takes the bulk insert.  Graph: 24 nearest neighbours + 8 random ids, R = 32.
    Under IP the sparse queries are no such regime: a row shares a dim or two with a query at most, so products
    collide and most are 0 (up to 110 boundary ties outstanding, past the kernel's spill list).  qs_ip are the same
    queries plus 1 + (dim mod 32) in every dim, which spreads the products (and the calibration rows) apart: the
    no-tie regime of the IP kernels."""
    rng = np.random.default_rng(seed)
    x = _sparse_rows(rng, n, d)
    x[:32] = calibration_rows(d)
    qs = _sparse_rows(rng, nq, d)
    adj = np.empty((n, 32), np.uint32)
    adj[:, :24] = knn_graph(x, 24)
    adj[:, 24:] = rng.integers(0, n, (n, 8))
    qs_ip = (qs + 1 + (np.arange(d) % 32)).astype(np.float32)
    return _frozen(dict(x=x, qs=qs, qs_ip=qs_ip, adj=adj, eps=[40, 47]))


@functools.lru_cache(maxsize=None)
def dense_ties(n, d, nq, seed):
    """Tie-heavy regime: values 0..3, every row present 4 times, on a ragged graph (R = 24): the Rust binary-search
    probe, the boundary evictions and the spill list decide the result."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, (n // 4, d)).astype(np.float32)
    x = np.repeat(base, 4, axis=0)[rng.permutation(4 * (n // 4))]
    x[:32] = calibration_rows(d)
    qs = rng.integers(0, 4, (nq, d)).astype(np.float32)
    adj = ragged_from_nn(knn_graph(x, 24), 24, rng, extra_random=4)
    return _frozen(dict(x=x, qs=qs, adj=adj, eps=[40, 47]))


def boundary_dims(d, fmt):
    """The dims on either side of every boundary of the kernel's row layout below d: the first chunk (a lane's 8
    codes or 4 floats), every 64-lane round (512 codes / 256 floats) and the row's last chunk."""
    dc, per = (8, 512) if fmt == 1 else (4, 256)
    s = set(range(min(dc + 1, d)))
    for b in range(per, d + 1, per):
        s.update((b - 1, b))
    s.update((d // 3, d // 2, d - dc, d - 1))
    return sorted(v for v in s if 0 <= v < d)


def one_hot_complete(d, dims):
    """Row i is (i + 1) at dims[i] and 0 elsewhere, on a complete graph (R = n − 1); two calibration rows (all 0,
    all 255) follow the graph rows and are not reachable.  The query 0 is at L2 distance (i + 1)² of row i, the
    all-ones query at IP distance −(i + 1): a kernel that drops, doubles or misplaces one dimension changes
    exactly that row."""
    n = len(dims)
    assert 2 <= n <= 64
    x = np.zeros((n + 2, d), np.float32)
    x[np.arange(n), dims] = np.arange(1, n + 1)
    x[n + 1] = 255.0
    adj = np.full((n + 2, n - 1), NONE, np.uint32)
    adj[:n] = np.array([[j for j in range(n) if j != i] for i in range(n)], np.uint32)
    qs = np.stack([np.zeros(d, np.float32), np.ones(d, np.float32)])
    return _frozen(dict(x=x, qs=qs, adj=adj, eps=[0], n_graph=n))


def spill_overflow():
    """One query whose boundary ties overflow the kernel's 64-entry spill list (L = 200): the list fills with 200
    rows at distance exactly 100, then 80 nearer rows evict unexpanded ties one by one while the threshold stays
    100.  Every evicted tie stays in the reference's heap."""
    d, R = 8, 64
    x = np.zeros((281, d), np.float32)
    x[0, 0] = 30.0                                   # the entry point, 900
    x[1:201, 0] = 10.0                               # A: 100 each
    x[201:281, 0] = (159 - np.arange(80)) / 16.0     # B: distinct, all below 100
    adj = np.full((281, R), NONE, np.uint32)
    adj[0] = np.arange(1, 65)
    adj[1] = np.arange(65, 129)
    adj[2] = np.arange(129, 193)
    adj[3, :8] = np.arange(193, 201)
    adj[4] = np.arange(201, 265)
    adj[201:281, :16] = np.arange(265, 281)
    return _frozen(dict(x=x, qs=np.zeros((1, d), np.float32), adj=adj, eps=[0], L=200))


def few_reachable():
    """40 rows of which the entry point reaches 5 (a chain 0 → 1 → 2 → 3 → 4); every other row points at the
    chain but nothing points back."""
    rng = np.random.default_rng(3)
    x = rng.integers(0, 4, (40, 8)).astype(np.float32)
    adj = np.full((40, 4), NONE, np.uint32)
    for i in range(4):
        adj[i, 0] = i + 1
    adj[4, 0] = 0
    adj[5:, 0] = rng.integers(0, 5, 35)
    qs = rng.integers(0, 4, (3, 8)).astype(np.float32)
    return _frozen(dict(x=x, qs=qs, adj=adj, eps=[0]))


def worst_sum(case, rows=None, qs="qs"):
    """An fp64 bound on every partial sum of every distance of the case: max Σx² + max Σq² (all values are ≥ 0,
    so (q − x)² ≤ q² + x² and q·x ≤ q² + x² term by term)."""
    x = case["x"] if rows is None else case["x"][:rows]
    return float((x.astype(np.float64) ** 2).sum(1).max() + (case[qs].astype(np.float64) ** 2).sum(1).max())


def tie_share(dists):
    """Share of neighbouring equal distances in sorted result rows (padding excluded)."""
    real = dists[:, 1:] < np.finfo(np.float32).max
    return float(((dists[:, 1:] == dists[:, :-1]) & real).sum() / max(int(real.sum()), 1))


def _rust_pos(res, dist):
    """slice::binary_search_by(partial_cmp) of std ≥ 1.82: the probe sequence decides among equal elements."""
    if not res:
        return 0
    size, base = len(res), 0
    while size > 1:
        half = size >> 1
        mid = base + half
        if not res[mid][0] > dist:
            base = mid
        size -= half
    p = res[base][0]
    if p == dist:
        return base
    return base + (1 if p < dist else 0)


def model_search(x, adj, eps, q, k, L, metric=0):
    """DiskProvider::search_batch for one query, as a heap and a sorted list (disk_provider.rs:524-678).
    Returns (ids, dists, outstanding): outstanding is the largest number of heap entries that are outside the
    result list and equal to its last distance — what the kernel has to keep in its spill list."""
    n = len(x)
    k = min(k, n)
    L = max(L, k)
    x32, q32 = x.astype(np.float32), q.astype(np.float32)

    def dist(i):
        if metric == 1:
            return np.float32(-np.sum(q32 * x32[i], dtype=np.float32))
        t = q32 - x32[i]
        return np.float32(np.sum(t * t, dtype=np.float32))

    visited, heap, res = set(), [], []
    for ep in eps:
        if ep in visited:
            continue
        visited.add(ep)
        if ep < n:
            c = (dist(ep), int(ep))
            heapq.heappush(heap, c)
            res.append(c)
    res.sort(key=lambda c: c[0])  # stable
    outstanding = 0
    while heap:
        cd, cid = heapq.heappop(heap)
        if len(res) >= L and cd > res[L - 1][0]:
            break
        for nb in adj[cid]:
            nb = int(nb)
            if nb == NONE:
                break
            if nb >= n or nb in visited:
                continue
            visited.add(nb)
            dn = dist(nb)
            if len(res) < L or dn < res[-1][0]:
                res.insert(_rust_pos(res, dn), (dn, nb))
                del res[L:]
                heapq.heappush(heap, (dn, nb))
        if len(res) >= L:
            inside = {i for _, i in res}
            thr = res[L - 1][0]
            outstanding = max(outstanding, sum(1 for dd, i in heap if dd == thr and i not in inside))
    ids = np.full(k, -1, np.int64)
    ds = np.full(k, np.finfo(np.float32).max, np.float32)
    m = min(k, len(res))
    ids[:m] = [i for _, i in res[:m]]
    ds[:m] = [dd for dd, _ in res[:m]]
    return ids, ds, outstanding
