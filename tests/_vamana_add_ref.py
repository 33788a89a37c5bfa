"""Row insertion into an existing graph restated in numpy: `mates` (each batch row's nearest other batch
rows from the batch's Gram matrix) and `add` (the build's batches continued: search against the graph as it stood at the
batch's start, out-edges from the traversal's list — joined with the mates when T > 0 —, back-edges).  `prune` is the
build's; the searches come from oracle.diskann_search_batch, as in _vamana_ref.build.  On data whose partial sums are
exact in fp32 the GPU reproduces this bit for bit.
"""
from __future__ import annotations

import numpy as np

from _vamana_ref import NONE, prune


def mates(xb: np.ndarray, T: int) -> np.ndarray:
    """(b, T) uint32: for batch row i the positions (0-based, within the batch) of its min(T, b − 1) nearest other
    batch rows by (distance, position) ascending, NONE-padded.  d(i, j) = max(0, (G_ii + G_jj) − 2·G_ij) in fp32 with
    G = X_b·X_bᵀ."""
    xb = np.ascontiguousarray(xb, np.float32)
    b = xb.shape[0]
    G = (xb @ xb.T).astype(np.float32)
    nn = np.diagonal(G).copy()
    D = np.maximum(np.float32(0), (nn[:, None] + nn[None, :]).astype(np.float32) - np.float32(2) * G)
    out = np.full((b, T), NONE, np.uint32)
    pos = np.arange(b)
    for i in range(b):
        other = pos[pos != i]
        order = other[np.lexsort((other, D[i, other]))][:T]
        out[i, :order.size] = order
    return out


def add(x: np.ndarray, adj0: np.ndarray, n0: int, R: int, L: int, alpha: float = 1.2, entry_point: int = 0,
        batch_max: int = 4096, T: int = 0):
    """Insert rows n0 .. n − 1 of x into the graph adj0 over rows 0 .. n0 − 1.  Returns (adjacency (n, R) uint32,
    counts) with counts = {batches, out_prunes, back_prunes, pools_truncated, mate_ids}."""
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
        # the graph as it stands: rows c.. are not in it (their adjacency rows are empty and nothing points at them)
        ids, dd, _ = oracle.diskann_search_batch(adj[:c], [entry_point], x[batch], K, K, 0, vecs=x[:c])
        mt = mates(x[batch], T) if T > 0 and b > 1 else None
        for bi, p in enumerate(batch):
            m = ids[bi] >= 0
            if T == 0:
                sel, tr = prune(x[:c + b], p, ids[bi][m], dd[bi][m], R, alpha)
            else:
                pool = ids[bi][m].astype(np.int64)
                if mt is not None:
                    mm = mt[bi][mt[bi] != NONE].astype(np.int64) + c
                    counts["mate_ids"] += int(mm.size)
                    pool = np.concatenate([pool, mm])
                sel, tr = prune(x[:c + b], p, pool, None, R, alpha)
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
                sel, tr = prune(x[:c + b], q, cand, None, R, alpha)
                adj[q] = NONE
                adj[q, :sel.size] = sel
                counts["back_prunes"] += 1
                counts["pools_truncated"] += int(tr)
        counts["batches"] += 1
        c += b
    return adj, counts


# ---- the inputs the CPU and the GPU tests share ----
def cont_rows():
    """The continuation input: small integers, every partial sum exact in fp32."""
    return np.random.default_rng(77).integers(-8, 9, (1500, 16)).astype(np.float32)


def burst_data():
    """An old distribution of 32 clusters and a burst of rows from 4 new cluster centres."""
    rng = np.random.default_rng(5)
    d = 32
    c_old = (4 * rng.standard_normal((32, d))).astype(np.float32)
    c_new = (4 * rng.standard_normal((4, d))).astype(np.float32)
    x_old = (c_old[rng.integers(0, 32, 2048)] + rng.standard_normal((2048, d))).astype(np.float32)
    x_new = (c_new[rng.integers(0, 4, 512)] + rng.standard_normal((512, d))).astype(np.float32)
    q_new = (c_new[rng.integers(0, 4, 200)] + rng.standard_normal((200, d))).astype(np.float32)
    return x_old, x_new, q_new
