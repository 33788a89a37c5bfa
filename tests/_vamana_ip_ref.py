"""The inner-product graph lifecycle of DESIGN §6.5 restated in numpy: `prune_ip` (the crate's occlude_list for
PruneKind::Occluding, rust_lib/diskann-patch/src/graph/index.rs:3329-3500 with config/mod.rs:44-101, no slack and no
saturation), and `build_ip`, `mates_ip`, `add_ip`, `consolidate_ip`: the loops of _vamana_ref.build, _vamana_add_ref.add
and _vamana_remove_ref.consolidate with prune_ip, d(a, b) = −Σ a_j·b_j and the oracle's traversal at metric = 1.  On data
whose partial sums are exact in fp32 the GPU reproduces all of it bit for bit.

prune_ip follows the crate's lazy loop literally — one position at a time, each with its own count of the selected
entries it has met — because its result depends on that order.  `stateless=True` is the variant that forgets the counts
and re-tests every selected entry at the current threshold; the two agree for a single pass (alpha = 1) and differ for
most pools otherwise, which tests/test_vamana_ip_ref.py holds the GPU tests' inputs to.
"""
from __future__ import annotations

import numpy as np

from _vamana_ref import F32_MAX, NONE, POOL_MAX
from _vamana_remove_ref import stored_row

IP = 1
OCCLUDED_STEP = np.float32(0.01)


def canon(d) -> np.ndarray:
    """fp32 with −0.0 counted as +0.0."""
    return np.asarray(d, np.float32) + np.float32(0.0)


def dist_ip(x: np.ndarray, i: int, ids) -> np.ndarray:
    """d(x[i], x[ids]) = −Σ a_j·b_j in fp32."""
    prod = x[np.asarray(ids, np.int64)] * x[int(i)]
    return canon(-prod.sum(axis=1, dtype=np.float32))


def pair_ip(x: np.ndarray) -> np.ndarray:
    """The n x n fp32 matrix of dist_ip's values (for callers that prune many pools over a small DB)."""
    x = np.ascontiguousarray(x, np.float32)
    return canon(-(x @ x.T).astype(np.float32))


def occlude_update(d_pi, d_ji, f, t):
    """The rule's one comparison: position i (d_pi from the target, current factor f) meets the selected entry j at the
    threshold t.  Strict, the product a plain fp32 multiply.  Returns the new factor: t + 0.01 when j occludes i."""
    t = np.float32(t)
    if np.float32(d_ji) < np.float32(t * np.float32(d_pi)):
        return np.float32(t + OCCLUDED_STEP)
    return np.float32(f)


def thresholds(alpha):
    """1.0, then t·min(alpha, 1.2) capped at alpha, up to and including alpha."""
    alpha = np.float32(alpha)
    step = min(alpha, np.float32(1.2))
    t = np.float32(1.0)
    out = [t]
    while t != alpha:
        t = min(np.float32(t * step), alpha)
        out.append(t)
    return out


def prune_ip(x: np.ndarray, p: int, ids, dists, R: int, alpha: float, pair=None, stateless: bool = False):
    """prune_ip(p, pool) of the spec.  ids: pool ids (p itself, ids outside [0, n) and repeats are dropped); dists:
    their distances to p, or None to compute them; pair (optional): pair_ip(x).  Returns (selected ids in selection
    order, whether the pool was truncated to POOL_MAX)."""
    n = x.shape[0]
    ids = np.asarray(ids, np.int64).reshape(-1)
    keep = (ids >= 0) & (ids < n) & (ids != p)
    if dists is not None:
        dists = canon(np.asarray(dists, np.float32).reshape(-1)[keep])
    ids = ids[keep]
    ids, first = np.unique(ids, return_index=True)
    if dists is None:
        dists = dist_ip(x, p, ids) if pair is None else pair[int(p), ids]
    else:
        dists = dists[first]
    order = np.lexsort((ids, dists))  # (dist, id) ascending, negatives first
    truncated = order.size > POOL_MAX
    order = order[:POOL_MAX]
    ids, dists = ids[order], canon(dists[order])
    M = ids.size
    if pair is None:
        D = canon(-(x[ids] @ x[ids].T).astype(np.float32))
    else:
        D = pair[np.ix_(ids, ids)]
    # fp32 values as Python floats (exact), for a loop that visits one position at a time
    Dl = D.tolist()
    f = [0.0] * M
    c = [0] * M
    sel = []
    fmax = float(F32_MAX)
    for t in thresholds(alpha):
        tf = float(t)
        occ = float(np.float32(t + OCCLUDED_STEP))
        bound = (t * dists).astype(np.float32).tolist()  # t · d(p, i), one fp32 multiply each
        for i in range(M):
            if len(sel) >= R:
                break
            if f[i] > tf:
                continue
            ci = 0 if stateless else c[i]
            hit = False
            while ci < len(sel):
                j = sel[ci]
                ci += 1
                if j >= i:
                    continue
                if Dl[j][i] < bound[i]:
                    hit = True
                    break
            c[i] = ci
            if hit:
                f[i] = 0.0 if stateless else occ
            else:
                f[i] = fmax
                sel.append(i)
        if len(sel) >= R:
            break
    return ids[np.asarray(sel, np.int64)].astype(np.uint32), truncated


def _set_row(adj, p, sel):
    adj[p] = NONE
    adj[p, :sel.size] = sel


def _back_edges(x, adj, batch, R, alpha, counts):
    """The batch's back-edges: appended where the row has room, else the row is pruned (pool: row + new sources)."""
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
            sel, tr = prune_ip(x, q, cand, None, R, alpha)
            _set_row(adj, q, sel)
            counts["back_prunes"] += 1
            counts["pools_truncated"] += int(tr)


def build_ip(x: np.ndarray, R: int, L: int, alpha: float = 1.2, entry_point: int = 0, batch_max: int = 4096):
    """_vamana_ref.build for IP.  Returns (adjacency (n, R) uint32, counts)."""
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
        ids, dd, _ = oracle.diskann_search_batch(adj, [entry_point], x[batch], L, L, IP, vecs=x)
        for bi, p in enumerate(batch):
            m = ids[bi] >= 0
            sel, tr = prune_ip(x, p, ids[bi][m], dd[bi][m], R, alpha)
            _set_row(adj, p, sel)
            counts["out_prunes"] += 1
            counts["pools_truncated"] += int(tr)
        _back_edges(x, adj, batch, R, alpha, counts)
        counts["batches"] += 1
        o0 += b
    return adj, counts


def mates_ip(xb: np.ndarray, T: int) -> np.ndarray:
    """_vamana_add_ref.mates for IP: (b, T) uint32 positions of each batch row's min(T, b − 1) other batch rows by
    (−G_ij, position) ascending, NONE-padded."""
    xb = np.ascontiguousarray(xb, np.float32)
    b = xb.shape[0]
    D = canon(-(xb @ xb.T).astype(np.float32))
    out = np.full((b, T), NONE, np.uint32)
    pos = np.arange(b)
    for i in range(b):
        other = pos[pos != i]
        order = other[np.lexsort((other, D[i, other]))][:T]
        out[i, :order.size] = order
    return out


def add_ip(x: np.ndarray, adj0: np.ndarray, n0: int, R: int, L: int, alpha: float = 1.2, entry_point: int = 0,
           batch_max: int = 4096, T: int = 0):
    """_vamana_add_ref.add for IP: rows n0 .. n − 1 of x inserted into the graph adj0 over rows 0 .. n0 − 1."""
    from oracle import oracle

    x = np.ascontiguousarray(x, np.float32)
    n = x.shape[0]
    adj = np.full((n, R), NONE, np.uint32)
    adj[:n0] = adj0[:n0]
    counts = {"batches": 0, "out_prunes": 0, "back_prunes": 0, "pools_truncated": 0, "mate_ids": 0}
    c = n0
    while c < n:
        b = min(batch_max, c, n - c)
        batch = list(range(c, c + b))
        K = min(L, c)
        ids, dd, _ = oracle.diskann_search_batch(adj[:c], [entry_point], x[batch], K, K, IP, vecs=x[:c])
        mt = mates_ip(x[batch], T) if T > 0 and b > 1 else None
        for bi, p in enumerate(batch):
            m = ids[bi] >= 0
            if T == 0:
                sel, tr = prune_ip(x[:c + b], p, ids[bi][m], dd[bi][m], R, alpha)
            else:
                pool = ids[bi][m].astype(np.int64)
                if mt is not None:
                    mm = mt[bi][mt[bi] != NONE].astype(np.int64) + c
                    counts["mate_ids"] += int(mm.size)
                    pool = np.concatenate([pool, mm])
                sel, tr = prune_ip(x[:c + b], p, pool, None, R, alpha)
            _set_row(adj, p, sel)
            counts["out_prunes"] += 1
            counts["pools_truncated"] += int(tr)
        _back_edges(x[:c + b], adj, batch, R, alpha, counts)
        counts["batches"] += 1
        c += b
    return adj, counts


def consolidate_ip(x: np.ndarray, adj: np.ndarray, labels, entry_point: int, alpha: float = 1.2, pair=None):
    """_vamana_remove_ref.consolidate for IP; a removed entry point is replaced by the live row with the smallest
    (−dot, id).  Returns (new_adj, new_entry_point, live_ids, counts)."""
    x = np.ascontiguousarray(x, np.float32)
    adj = np.ascontiguousarray(adj, np.uint32)
    n, R = adj.shape
    labels = np.asarray(labels, np.int64).reshape(-1)
    dead = np.zeros(n, bool)
    dead[labels[(labels >= 0) & (labels < n)]] = True
    live_ids = np.nonzero(~dead)[0].astype(np.int64)
    assert live_ids.size > 0, "every row would be removed"
    counts = {"removed": int(dead.sum()), "repaired": 0, "pools_truncated": 0, "pool_ids": 0, "entry_replaced": 0}

    def live_of(row):
        row = row[row < n].astype(np.int64)
        return row[~dead[row]]

    within = np.cumsum(adj == NONE, axis=1) == 0
    rep = np.where(within, adj, np.uint32(NONE))
    gone_slot = within & (adj < n) & dead[np.minimum(adj, n - 1)]
    for p in np.nonzero(~dead & gone_slot.any(axis=1))[0]:
        row = stored_row(adj, p)
        gone = row[gone_slot[p, :row.size]]
        pool = np.concatenate([live_of(row)] + [live_of(stored_row(adj, v)) for v in gone])
        sel, tr = prune_ip(x, int(p), pool, None, R, alpha, pair=pair)
        _set_row(rep, p, sel)
        counts["repaired"] += 1
        counts["pools_truncated"] += int(tr)
        counts["pool_ids"] += int(pool.size)

    ep = int(entry_point)
    if dead[ep]:
        dd = dist_ip(x, ep, live_ids) if pair is None else pair[ep, live_ids]
        ep = int(live_ids[dd == dd.min()].min())
        counts["entry_replaced"] = 1

    rank = np.arange(n, dtype=np.int64) - (np.cumsum(dead) - dead)
    new_adj = rep[live_ids]
    inside = new_adj < n
    new_adj[inside] = rank[new_adj[inside].astype(np.int64)].astype(np.uint32)
    return new_adj, int(rank[ep]), live_ids, counts


def knn_random_graph_ip(x, R, seed=11):
    """The yardstick: the exact R − 4 largest-dot rows plus 4 random edges."""
    n = x.shape[0]
    x64 = x.astype(np.float64)
    dd = -(x64 @ x64.T)
    np.fill_diagonal(dd, np.inf)
    near = np.argsort(dd, axis=1, kind="stable")[:, :R - 4]
    rnd = np.random.default_rng(seed).integers(0, n, (n, 4))
    return np.concatenate([near, rnd], axis=1).astype(np.uint32)


# ---- the inputs the CPU and the GPU prune tests share ----
PRUNE_SIZES = [1, 2, 63, 64, 65, 128, 129, 255, 256, 300]
PRUNE_N, PRUNE_M, PRUNE_CAP = 600, 40, 300


def dup4_rows(rng, base, d):
    """`base` rows of values 0..3, every row four times (all dots >= 0, zero dots, masses of ties), shuffled."""
    x = np.repeat(rng.integers(0, 4, (base, d)), 4, axis=0).astype(np.float32)
    return np.ascontiguousarray(x[rng.permutation(x.shape[0])])


def prune_inputs(kind: str, d: int):
    """(x, targets, pools) of test_prune_ip_exact: 600 rows — "dup4" (values 0..3, every row four times) or "ints"
    (integers −8..8: distances of both signs and exact zeros) —, 40 targets, pools of every size in PRUNE_SIZES with
    repeats, the target itself, ids outside the DB and padding inside and around."""
    rng = np.random.default_rng((2000 if kind == "dup4" else 3000) + d)
    n, m, cap = PRUNE_N, PRUNE_M, PRUNE_CAP
    if kind == "dup4":
        x = dup4_rows(rng, n // 4, d)
    else:
        x = rng.integers(-8, 9, (n, d)).astype(np.float32)
    targets = rng.integers(0, n, m).astype(np.uint32)
    sizes = rng.choice(PRUNE_SIZES, m)
    sizes[:len(PRUNE_SIZES)] = PRUNE_SIZES  # each size at least once
    pools = np.full((m, cap), NONE, np.uint32)
    for t in range(m):
        s = int(sizes[t])
        ids = rng.integers(0, n, s).astype(np.uint32)  # with replacement: repeats
        if t < len(PRUNE_SIZES) and s >= 255:
            ids = rng.permutation(n)[:s].astype(np.uint32)  # distinct: 255 and 256 kept whole, 300 truncated to 256
        if s >= 2:
            ids[rng.integers(0, s)] = targets[t]
            ids[rng.integers(0, s)] = n + rng.integers(0, 5)
        if s >= 63:
            ids[rng.integers(0, s, 3)] = NONE
        pools[t, rng.permutation(cap)[:s]] = ids
    return x, targets, pools
