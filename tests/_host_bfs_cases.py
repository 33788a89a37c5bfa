"""The cases of tests/test_diskann_host_bfs_gpu.py, shared with the child process that answers them with
HIPANN_BFS_GPU_VISITED=0 (the host BFS keeps its visited sets on the host, csrc/diskann_host_bfs.cpp): run as a script,
it writes every case's ids, distances, evaluation count and step count to the .npz named on its command line.

ragged_case is also the graph of test_bfs_many_queries_parallel_host (tests/test_diskann_gpu.py).
"""
from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "duckdb-annsearch_amd", ROOT, Path(__file__).resolve().parent):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

from _bfs_cases import NONE, ragged_from_nn  # noqa: E402

FIELDS = ("ids", "dists", "evals", "steps")


def _oracle():
    from oracle import oracle as O

    O.build()
    return O


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def ragged_case():
    """n 4000, d 48, R 24, 600 queries (a case takes the first nq): u32::MAX padding after a varying degree,
    out-of-range ids, a duplicated neighbour, and a repeated entry point — the visited / skip rules of
    disk_provider.rs:556-577.  Returns (x, qs, adj, eps)."""
    O = _oracle()
    rng = np.random.default_rng(11)
    n, d, R = 4000, 48, 24
    x = rng.standard_normal((n, d)).astype(np.float32)
    qs = (x[rng.integers(0, n, 600)] + 0.1 * rng.standard_normal((600, d))).astype(np.float32)
    _, nn = O.flat_search(x, x, R - 4 + 1, 0)
    adj = np.full((n, R), NONE, np.uint32)
    adj[:, : R - 4] = nn[:, 1:]
    adj[:, R - 4: R - 2] = rng.integers(0, n, (n, 2))
    adj[::7, R - 2] = n + 5          # out of range: skipped, not a sentinel
    adj[::5, 3] = adj[::5, 2]        # duplicate neighbour
    deg = rng.integers(R // 2, R + 1, n)
    adj[np.arange(R)[None, :] >= deg[:, None]] = NONE
    return _frozen(x, qs, adj) + ([17, 17, 2500],)


@functools.lru_cache(maxsize=None)
def ragged_sq8():
    """The ragged case's SQ8 database: (codes, mins, scale)."""
    O = _oracle()
    x = ragged_case()[0]
    mins, scale = O.sq8_train(x)
    return _frozen(O.sq8_encode(x, mins, scale), mins, scale)


@functools.lru_cache(maxsize=None)
def complete6_case():
    """A complete graph on rows 0..5 of a 12-row database (rows 6..11 have no edge in or out): k = 10 asks for more
    than the 6 rows a search can reach, so every result row ends in four −1 / FLT_MAX pads."""
    rng = np.random.default_rng(6)
    x = rng.integers(-4, 5, (12, 3)).astype(np.float32)
    qs = rng.integers(-4, 5, (3, 3)).astype(np.float32)
    adj = np.full((12, 5), NONE, np.uint32)
    adj[:6] = np.array([[j for j in range(6) if j != i] for i in range(6)], np.uint32)
    return _frozen(x, qs, adj) + ([0],)


@functools.lru_cache(maxsize=None)
def wide_case():
    """R = 300 on 400 rows of 16 dims, rows built as the ragged ones: wider than the host-set expansion's 256-id
    pieces and than the resident kernel's 64-id rows."""
    O = _oracle()
    rng = np.random.default_rng(13)
    n, d, R = 400, 16, 300
    x = rng.standard_normal((n, d)).astype(np.float32)
    qs = (x[rng.integers(0, n, 20)] + 0.1 * rng.standard_normal((20, d))).astype(np.float32)
    _, nn = O.flat_search(x, x, R - 4 + 1, 0)
    adj = ragged_from_nn(nn[:, 1:], R, rng)
    return _frozen(x, qs, adj) + ([17, 17, 250],)


# name -> (kind, fmt, metric, nq)
CASES = {}
for _nq in (130, 5):  # two groups and eight threads; one group, one thread
    for _fmt in (0, 1):
        for _metric in (0, 1):
            CASES[f"ragged_nq{_nq}_{'sq8' if _fmt else 'f32'}_{'ip' if _metric else 'l2'}"] = ("ragged", _fmt, _metric, _nq)
CASES["complete6_padding"] = ("complete6", 0, 0, 3)
CASES["nq0"] = ("ragged", 0, 0, 0)
CASES["wide_R300"] = ("wide", 0, 0, 20)
CASES["wide_R300_resident_fallback"] = ("wide_resident", 0, 0, 20)


def run_case(hipann, name):
    """Answer the case on the GPU: {"ids", "dists", "evals", "steps"}."""
    kind, fmt, metric, nq = CASES[name]
    if kind == "ragged":
        x, qs, adj, eps = ragged_case()
        qs = qs[:nq]
        k, L = 10, 40
    elif kind == "complete6":
        x, qs, adj, eps = complete6_case()
        k, L = 10, 8
    else:
        x, qs, adj, eps = wide_case()
        k, L = 10, 40
    if fmt == 0:
        db = hipann.DiskannDeviceDB(x, 0)
    else:
        codes, mins, scale = ragged_sq8()
        db = hipann.DiskannDeviceDB(codes, 1, mins, scale)
    if kind == "wide_resident":  # every query flagged (R > 64): the resident search's host fallback
        db.register_graph(adj)
        ids, dists, st = db.search_batch_resident(eps, qs, k, L, metric)
        assert st["pops"] == 0 and st["host_requeries"] == nq, st
    else:
        ids, dists, st = db.search_batch(adj, eps, qs, k, L, metric)
    db.close()
    return {"ids": ids, "dists": dists, "evals": np.int64(st["evals"]), "steps": np.int64(st["steps"])}


if __name__ == "__main__":
    import hipann

    out = {}
    for name in CASES:
        r = run_case(hipann, name)
        for f in FIELDS:
            out[f"{name}.{f}"] = r[f]
    np.savez(sys.argv[1], **out)
