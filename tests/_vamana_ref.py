"""The graph build of DESIGN §6 restated in numpy: `prune` (the crate's occlude_list for the triangle-inequality kind,
rust_lib/diskann-patch/src/graph/index.rs:3329-3500), `build` (prefix-doubling batches searched against the frozen
graph, out-edges, back-edges) and `reachable`.  The searches come from oracle.diskann_search_batch, the existing
restatement of the traversal.  On data whose partial sums are exact in fp32 the GPU build reproduces this bit for bit.
"""
from __future__ import annotations

import numpy as np

NONE = 0xFFFFFFFF
POOL_MAX = 256
F32_MAX = np.finfo(np.float32).max


def dist_to(x: np.ndarray, i: int, ids) -> np.ndarray:
    """d(x[i], x[ids]) = Σ(a−b)² in fp32."""
    diff = x[np.asarray(ids, np.int64)] - x[int(i)]
    return (diff * diff).sum(axis=1, dtype=np.float32)


def prune(x: np.ndarray, p: int, ids, dists, R: int, alpha: float, pair=None):
    """prune(p, pool) of the spec.  ids: pool ids (any integer type; p itself, ids outside [0, n) and repeats are
    dropped); dists: their distances to p, or None to compute them.  pair (optional): the n x n fp32 matrix of
    dist_to's values, for callers that prune many pools over a small DB.  Returns (selected ids in selection order,
    whether the pool was truncated to POOL_MAX)."""
    dist = dist_to if pair is None else (lambda _x, i, js: pair[int(i), np.asarray(js, np.int64)])
    n = x.shape[0]
    ids = np.asarray(ids, np.int64).reshape(-1)
    keep = (ids >= 0) & (ids < n) & (ids != p)
    if dists is not None:
        dists = np.asarray(dists, np.float32).reshape(-1)[keep]
    ids = ids[keep]
    ids, first = np.unique(ids, return_index=True)
    dists = dist(x, p, ids) if dists is None else dists[first]
    order = np.lexsort((ids, dists))  # (dist, id) ascending
    truncated = order.size > POOL_MAX
    order = order[:POOL_MAX]
    ids, dists = ids[order], dists[order].astype(np.float32)
    M = ids.size
    f = np.zeros(M, np.float32)  # occlusion factors; F32_MAX marks a selected position
    alpha = np.float32(alpha)
    step = min(alpha, np.float32(1.2))
    t = np.float32(1.0)
    out = []
    while True:
        for i in range(M):
            if len(out) >= R:
                break
            if f[i] > t:
                continue
            out.append(int(ids[i]))
            f[i] = F32_MAX
            later = np.arange(i + 1, M)
            later = later[f[later] <= alpha]  # neither selected nor dead
            if later.size:
                dj = dist(x, ids[i], ids[later])
                with np.errstate(divide="ignore", invalid="ignore"):
                    fac = np.where(dj == 0, F32_MAX, dists[later] / dj).astype(np.float32)
                f[later] = np.maximum(f[later], fac)
        if len(out) >= R or t == alpha:
            break
        t = min(np.float32(t * step), alpha)
    return np.asarray(out, np.uint32), truncated


def build(x: np.ndarray, R: int, L: int, alpha: float = 1.2, entry_point: int = 0, batch_max: int = 4096):
    """The whole build.  Returns (adjacency (n, R) uint32, counts) with counts = {batches, out_prunes, back_prunes,
    pools_truncated}."""
    from oracle import oracle

    x = np.ascontiguousarray(x, np.float32)
    n = x.shape[0]
    adj = np.full((n, R), NONE, np.uint32)
    counts = {"batches": 0, "out_prunes": 0, "back_prunes": 0, "pools_truncated": 0}
    order = [i for i in range(n) if i != entry_point]
    o0 = 0
    while o0 < n - 1:
        b = min(batch_max, max(1, o0 + 1), n - 1 - o0)
        batch = order[o0:o0 + b]
        ids, dd, _ = oracle.diskann_search_batch(adj, [entry_point], x[batch], L, L, 0, vecs=x)
        for bi, p in enumerate(batch):
            m = ids[bi] >= 0
            sel, tr = prune(x, p, ids[bi][m], dd[bi][m], R, alpha)
            adj[p] = NONE
            adj[p, :sel.size] = sel
            counts["out_prunes"] += 1
            counts["pools_truncated"] += int(tr)
        sources = {}
        for p in batch:
            for q in adj[p]:
                if q == NONE:
                    break
                sources.setdefault(int(q), []).append(p)
        for q, ps in sources.items():
            row = adj[q]
            deg = int(np.argmax(row == NONE)) if (row == NONE).any() else R
            have = set(int(v) for v in row[:deg])
            cand = [int(v) for v in row[:deg]] + [p for p in sorted(ps) if p not in have]
            if len(cand) <= R:
                adj[q, :len(cand)] = cand
            else:
                sel, tr = prune(x, q, cand, None, R, alpha)
                adj[q] = NONE
                adj[q, :sel.size] = sel
                counts["back_prunes"] += 1
                counts["pools_truncated"] += int(tr)
        counts["batches"] += 1
        o0 += b
    return adj, counts


def reachable(adj: np.ndarray, entry_point: int) -> np.ndarray:
    """Boolean mask of the rows a walk from entry_point reaches (rows end at the first NONE)."""
    n = adj.shape[0]
    seen = np.zeros(n, bool)
    seen[entry_point] = True
    stack = [int(entry_point)]
    while stack:
        v = stack.pop()
        for w in adj[v]:
            if w == NONE:
                break
            if w < n and not seen[w]:
                seen[w] = True
                stack.append(int(w))
    return seen


def check_structure(adj, R):
    n = adj.shape[0]
    assert adj.shape == (n, R) and adj.dtype == np.uint32
    valid = adj != NONE
    assert (adj[valid] < n).all()
    deg = valid.sum(axis=1)
    assert (valid == (np.arange(R)[None, :] < deg[:, None])).all(), "padding is not contiguous"
    assert not (adj == np.arange(n, dtype=np.uint32)[:, None]).any(), "self loop"
    s = np.sort(adj.astype(np.int64), axis=1)
    assert not ((s[:, 1:] == s[:, :-1]) & (s[:, 1:] != NONE)).any(), "repeated id in a row"


def knn_random_graph(x, R, seed=11):
    """The yardstick: the exact R − 4 nearest rows plus 4 random edges."""
    n = x.shape[0]
    x64 = x.astype(np.float64)
    nn = (x64 ** 2).sum(1)
    d2 = nn[:, None] + nn[None, :] - 2.0 * (x64 @ x64.T)
    np.fill_diagonal(d2, np.inf)
    near = np.argsort(d2, axis=1, kind="stable")[:, :R - 4]
    rnd = np.random.default_rng(seed).integers(0, n, (n, 4))
    return np.concatenate([near, rnd], axis=1).astype(np.uint32)
