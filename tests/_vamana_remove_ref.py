"""Row removal from a DiskANN graph (FreshDiskANN's delete consolidation) restated in numpy: the repair of
the rows that point at a removed row, the entry-point replacement, and the compaction with relabelling.  `prune` is the
build's (tests/_vamana_ref.py).  On data whose partial sums are exact in fp32 diskann_hip_remove_ids reproduces this
bit for bit."""
from __future__ import annotations

import numpy as np

from _vamana_ref import NONE, dist_to, prune


def stored_row(adj: np.ndarray, p: int) -> np.ndarray:
    """N(p): the ids of row p up to the first NONE."""
    row = adj[p]
    pad = np.nonzero(row == NONE)[0]
    return row[:pad[0]] if pad.size else row


def consolidate(x: np.ndarray, adj: np.ndarray, labels, entry_point: int, alpha: float = 1.2, pair=None):
    """Remove the rows `labels` (any order; repeats and labels outside [0, n) are ignored) from the graph `adj` over the
    rows `x`.  pair (optional): the n x n fp32 matrix of dist_to's values, as for `prune`.  Returns (new_adj (n', R)
    uint32, new_entry_point, live_ids (n',) int64: the old id of every new row, counts) with counts = {removed, repaired, pools_truncated, pool_ids: live ids gathered into pools, repeats and the
    target itself included, entry_replaced}."""
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

    # 1. repair, in the old id space: every row reads `adj` and writes `rep`
    within = np.cumsum(adj == NONE, axis=1) == 0          # the slots of N(p)
    rep = np.where(within, adj, np.uint32(NONE))          # rows that keep their ids
    gone_slot = within & (adj < n) & dead[np.minimum(adj, n - 1)]
    for p in np.nonzero(~dead & gone_slot.any(axis=1))[0]:
        row = stored_row(adj, p)
        gone = row[gone_slot[p, :row.size]]  # per slot: a removed id stored twice is gathered twice
        pool = np.concatenate([live_of(row)] + [live_of(stored_row(adj, v)) for v in gone])
        sel, tr = prune(x, int(p), pool, None, R, alpha, pair=pair)
        rep[p] = NONE
        rep[p, :sel.size] = sel
        counts["repaired"] += 1
        counts["pools_truncated"] += int(tr)
        counts["pool_ids"] += int(pool.size)

    # 2. the entry point: the live row nearest the removed one by (dist, id)
    ep = int(entry_point)
    if dead[ep]:
        dd = dist_to(x, ep, live_ids) if pair is None else pair[ep, live_ids]
        ep = int(live_ids[dd == dd.min()].min())
        counts["entry_replaced"] = 1

    # 3. compact: survivors keep their order, new id = old id − removed rows below it
    rank = np.arange(n, dtype=np.int64) - (np.cumsum(dead) - dead)
    new_adj = rep[live_ids]
    inside = new_adj < n  # (NONE and ids ≥ n stay as they are)
    new_adj[inside] = rank[new_adj[inside].astype(np.int64)].astype(np.uint32)
    return new_adj, int(rank[ep]), live_ids, counts
