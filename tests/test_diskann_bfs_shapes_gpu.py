"""Exact tests of every template instantiation and edge path of the GPU-resident DiskANN traversal
(diskann_bfs.hip: 9 row widths x 2 list depths x 2 metrics), against oracle.diskann_search_batch, the restatement of
DiskProvider::search_batch.

The inputs (tests/_bfs_cases.py) are small integers, so every distance is one float in any summation order; "exact"
below is np.array_equal on ids and on distances and == on the evaluation and step counts.  tests/test_bfs_cases.py
holds the same inputs to the oracle alone on the CPU (exactness, SQ8 codes == values, tie shares, the spill
overflow), so none of these cases can pass vacuously.
"""
from __future__ import annotations

import numpy as np
import pytest

import _bfs_cases as B

pytestmark = pytest.mark.gpu
FMAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def dbs(gpu, oracle):
    """(case name, fmt) → (device DB with the graph registered, the oracle's keyword arguments): one upload per
    module, released at its end."""
    made = {}

    def get(name, case, fmt):
        key = (name, fmt)
        if key not in made:
            x = case["x"]
            if fmt == 0:
                db, kw = gpu.DiskannDeviceDB(x, 0), dict(vecs=x)
            else:
                mins, scale = oracle.sq8_train(x)
                assert np.all(mins == 0) and np.all(scale == 255)
                codes = oracle.sq8_encode(x, mins, scale)
                db, kw = gpu.DiskannDeviceDB(codes, 1, mins, scale), dict(codes=codes, mins=mins, scale=scale)
            db.register_graph(case["adj"])
            made[key] = (db, kw)
        return made[key]

    yield get
    for db, _ in made.values():
        db.close()


def check_exact(oracle, db, kw, adj, eps, qs, k, L, metric=0, on_device=True):
    ids, dists, st = db.search_batch_resident(eps, qs, k, L, metric)
    oi, od, ost = oracle.diskann_search_batch(adj, eps, qs, k, L, metric, **kw)
    print(f"gpu {st} oracle {ost} ids equal {(ids == oi).mean():.4f}")
    assert ids.shape == oi.shape and dists.shape == od.shape
    assert np.array_equal(ids, oi)
    assert np.array_equal(dists, od)
    assert st["evals"] == ost["evals"]
    assert st["steps"] == ost["steps"]
    assert np.all(np.diff(dists, axis=1) >= 0)
    if on_device:
        assert st["host_requeries"] == 0 and st["pops"] > 0
    return ids, dists, st


def run_case(oracle, dbs, name, case, fmt, k, L, metric=0, eps=None, on_device=True, qs="qs"):
    db, kw = dbs(name, case, fmt)
    return check_exact(oracle, db, kw, case["adj"], case["eps"] if eps is None else eps, case[qs], k, L, metric,
                       on_device)


ONE_HOT = [(fmt, d) for fmt in (1, 0) for d in B.ONE_HOT_DIMS[fmt]]
WIDE = [(fmt, d) for fmt in (1, 0) for d in B.WIDE_DIMS[fmt]]


# ---- 1. every dimension counts -------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("fmt,d", ONE_HOT)
def test_every_dimension_counts(gpu, oracle, dbs, fmt, d, metric):
    """One row per boundary dimension of the lane layout, each at its own distance: a dimension that is dropped,
    counted twice or credited to another row changes exactly that row's distance."""
    case = B.one_hot_complete(d, B.boundary_dims(d, fmt))
    n = case["n_graph"]
    ids, dists, st = run_case(oracle, dbs, f"one_hot{d}", case, fmt, n, 64, metric)
    want = np.arange(1, n + 1, dtype=np.float32)
    q = metric                                       # L2: the query 0; IP: the query of all ones
    if metric == 0:
        assert ids[q].tolist() == list(range(n)) and np.array_equal(dists[q], want ** 2)
    else:
        assert ids[q].tolist() == list(range(n))[::-1] and np.array_equal(dists[q], -want[::-1])
    assert st["evals"] == 2 * n


# ---- 2. no-tie exact traversal -------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [128, 129])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("fmt,d", WIDE)
def test_no_tie_traversal(gpu, oracle, dbs, fmt, d, metric, L):
    """wide_sparse has next to no equal distances (L2: the sparse queries; IP: the dense-offset queries): a correct
    kernel merges each step's candidates at once (bulk_insert), at both list depths (S = 2 at L = 128, S = 4 at
    L = 129)."""
    run_case(oracle, dbs, f"wide{d}", B.wide_sparse(B.N, d, B.NQ, d), fmt, 10, L, metric,
             qs="qs_ip" if metric == 1 else "qs")


@pytest.mark.parametrize("L", [128, 129])
@pytest.mark.parametrize("fmt,d", WIDE)
def test_sparse_ip_ties(gpu, oracle, dbs, fmt, d, L):
    """The sparse queries under IP: most products are 0, so the list's tail is one long tie and up to 110 evicted
    boundary ties are outstanding at once.  Queries that overflow the 64-entry spill list are re-run on the host;
    either way every result and both counts are the oracle's."""
    _, _, st = run_case(oracle, dbs, f"wide{d}", B.wide_sparse(B.N, d, B.NQ, d), fmt, 10, L, 1, on_device=False)
    assert st["pops"] > 0


# ---- 3. tie-heavy exact traversal ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,d", WIDE)
def test_tie_heavy_traversal(gpu, oracle, dbs, fmt, d):
    run_case(oracle, dbs, f"dense{d}", B.dense_ties(B.N, d, B.NQ, d), fmt, 10, 128)


# ---- 4. list-depth edges -------------------------------------------------------------------------------------------
def _depth_case(builder):
    return builder.__name__, builder(B.N, B.DEPTH_D, B.NQ, 5)


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256])
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("builder", [B.dense_ties, B.wide_sparse])
def test_list_depth_edges(gpu, oracle, dbs, builder, fmt, L):
    """k = L returns the whole list: every slot crossing of insert_at / get_d / clear_at and the last element."""
    name, case = _depth_case(builder)
    if L == 1:  # the case's two seeds are more than L (flagged, re-run on the host): one seed stays on the device
        _, _, st = run_case(oracle, dbs, name, case, fmt, L, L, on_device=False)
        assert st["host_requeries"] == B.NQ
        run_case(oracle, dbs, name, case, fmt, L, L, eps=case["eps"][:1])
        return
    run_case(oracle, dbs, name, case, fmt, L, L)
    if L > 10:
        run_case(oracle, dbs, name, case, fmt, 10, L)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("builder", [B.dense_ties, B.wide_sparse])
def test_list_depth_beyond_kernel(gpu, oracle, dbs, builder, fmt):
    name, case = _depth_case(builder)
    _, _, st = run_case(oracle, dbs, name, case, fmt, 10, 257, on_device=False)
    assert st["pops"] == 0 and st["host_requeries"] == B.NQ


# ---- 5. k edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,L", [(1, 128), (64, 128), (65, 128), (100, 128), (150, 40)])
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("builder", [B.dense_ties, B.wide_sparse])
def test_k_edges(gpu, oracle, dbs, builder, fmt, k, L):
    """The output loop's second round (k > 64) and k > L (L is raised to k)."""
    name, case = _depth_case(builder)
    ids, _, _ = run_case(oracle, dbs, name, case, fmt, k, L)
    assert ids.shape == (B.NQ, k) and np.all(ids >= 0)


def test_k_beyond_reachable(gpu, oracle, dbs):
    ids, dists, st = run_case(oracle, dbs, "few", B.few_reachable(), 0, 10, 16)
    assert np.all(ids[:, :5] >= 0) and np.all(ids[:, 5:] == -1) and np.all(dists[:, 5:] == FMAX)


def _tiny_graph(n, seed=1):
    rng = np.random.default_rng(seed)
    R = max(min(n - 1, 6), 1)
    x = rng.integers(0, 4, (n, 16)).astype(np.float32)
    adj = np.full((n, R), B.NONE, np.uint32)
    for i in range(n):
        others = rng.permutation(np.delete(np.arange(n), i))[:R]
        adj[i, : len(others)] = others
    adj[:: 4, R - 1] = B.NONE
    qs = rng.integers(0, 4, (5, 16)).astype(np.float32)
    return dict(x=x, qs=qs, adj=adj, eps=[0, n - 1])


def test_k_beyond_n(gpu, oracle, dbs):
    ids, _, _ = run_case(oracle, dbs, "tiny7", _tiny_graph(7), 0, 10, 4)
    assert ids.shape == (5, 7)


# ---- 6. seeds ------------------------------------------------------------------------------------------------------
SEEDS = {
    "one": [40],
    "64_distinct": list(range(32, 96)),
    "64_repeats_and_out_of_range": list(range(40, 72)) + [40, B.N, B.N + 7, 0xFFFFFFFE] + list(range(60, 88)),
}


@pytest.mark.parametrize("which", sorted(SEEDS))
@pytest.mark.parametrize("fmt", [0, 1])
def test_seeds(gpu, oracle, dbs, fmt, which):
    """The seed phase: visited insert in order (first occurrence wins, ids ≥ N skipped), the stable sort."""
    name, case = _depth_case(B.dense_ties)
    assert len(SEEDS[which]) in (1, 64)
    run_case(oracle, dbs, name, case, fmt, 10, 128, eps=SEEDS[which])
    run_case(oracle, dbs, name, case, fmt, 64, 64, eps=SEEDS[which])


@pytest.mark.parametrize("fmt", [0, 1])
def test_no_seeds(gpu, oracle, dbs, fmt):
    name, case = _depth_case(B.dense_ties)
    db, kw = dbs(name, case, fmt)
    ids, dists, st = check_exact(oracle, db, kw, case["adj"], np.zeros(0, np.uint32), case["qs"], 10, 32)
    assert np.all(ids == -1) and np.all(dists == FMAX) and st["evals"] == 0


@pytest.mark.parametrize("fmt", [0, 1])
def test_65_seeds_run_on_the_host(gpu, oracle, dbs, fmt):
    name, case = _depth_case(B.dense_ties)
    _, _, st = run_case(oracle, dbs, name, case, fmt, 10, 128, eps=list(range(32, 97)), on_device=False)
    assert st["pops"] == 0 and st["host_requeries"] == B.NQ


@pytest.mark.parametrize("fmt", [0, 1])
def test_more_seeds_than_L_are_flagged(gpu, oracle, dbs, fmt):
    """20 distinct seeds at L = 8: the kernel flags every query after the seed phase and the host re-runs it.  A
    flagged query's evaluations are the host re-run's alone (check_exact: evals == the oracle's)."""
    name, case = _depth_case(B.dense_ties)
    _, _, st = run_case(oracle, dbs, name, case, fmt, 5, 8, eps=list(range(40, 60)), on_device=False)
    assert st["host_requeries"] == B.NQ


# ---- 7. graph shape ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65])
def test_n_around_visited_words(gpu, oracle, dbs, n):
    """The visited bitmap has (N + 31) / 32 words per query: the last id of a word, the first of the next."""
    case = _tiny_graph(n)
    ids, _, st = run_case(oracle, dbs, f"tiny{n}", case, 0, 10, 16)
    assert st["evals"] <= len(case["qs"]) * n


@pytest.mark.parametrize("R", [1, 2, 63, 64])
@pytest.mark.parametrize("fmt", [0, 1])
def test_degree_edges(gpu, oracle, dbs, fmt, R):
    _, base = _depth_case(B.dense_ties)
    case = dict(base, adj=np.ascontiguousarray(B.knn_graph(base["x"], R).astype(np.uint32)))
    run_case(oracle, dbs, f"deg{R}", case, fmt, 10, 64)


@pytest.mark.parametrize("fmt", [0, 1])
def test_empty_and_repeated_rows(gpu, oracle, dbs, fmt):
    """Rows whose first slot is u32::MAX expand nothing (an entry point among them); rows with a repeated id before
    their first sentinel take the dedupe."""
    _, base = _depth_case(B.dense_ties)
    adj = base["adj"].copy()
    assert adj[40, 2] == adj[40, 3] != B.NONE and adj[45, 2] == adj[45, 3] != B.NONE   # _ragged_graph's repeats
    adj[47] = B.NONE
    adj[3::11, 0] = B.NONE
    case = dict(base, adj=adj)
    assert adj[36, 0] == B.NONE
    for eps in ([40, 47], [45, 47, 36]):
        run_case(oracle, dbs, "empty_rows", case, fmt, 10, 64, eps=eps)
    _, _, st = run_case(oracle, dbs, "empty_rows", case, fmt, 10, 64, eps=[47])
    assert st["evals"] == B.NQ and st["steps"] == 2   # the seed, one empty expansion, the empty heap


@pytest.mark.parametrize("fmt", [0, 1])
def test_host_bfs_repeated_ids_first_occurrence(gpu, oracle, dbs, fmt):
    """The host BFS (search_batch, and the resident search's host path at L = 257) keeps its visited sets on the
    device, one atomic per slot of a step's gather in no particular order: an id a row holds twice, far apart, must
    still count at its first occurrence.  (The results of the two orders differ on this input, test_bfs_cases.py.)"""
    _, base = _depth_case(B.dense_ties)
    case = dict(base, adj=B.repeat_first_last(base["adj"], B.N))
    db, kw = dbs("repeat_first_last", case, fmt)
    for eps, L in (([40, 47], 64), ([40, 47, 60, 40, 47], 257)):
        oi, od, ost = oracle.diskann_search_batch(case["adj"], eps, case["qs"], 10, L, 0, **kw)
        ids, dists, st = db.search_batch(case["adj"], eps, case["qs"], 10, L)
        assert np.array_equal(ids, oi) and np.array_equal(dists, od)
        assert st["evals"] == ost["evals"] and st["steps"] == ost["steps"]
        check_exact(oracle, db, kw, case["adj"], eps, case["qs"], 10, L, on_device=L <= 256)


# ---- 8. spill overflow ---------------------------------------------------------------------------------------------
def test_spill_overflow_is_rerun_on_the_host(gpu, oracle, dbs):
    """More boundary ties outstanding than the 64-entry spill list holds: the query is flagged, re-run by the host
    BFS, and counted once — its evaluations and steps are the oracle's, not the oracle's plus the device's partial
    run."""
    case = B.spill_overflow()
    L = case["L"]
    for k in (10, L):
        _, _, st = run_case(oracle, dbs, "spill", case, 0, k, L, on_device=False)
        assert st["host_requeries"] == 1 and st["pops"] > 0


# ---- 9. float data at the new widths -------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("fmt,d", [(1, 1024), (1, 2048), (0, 512), (0, 768), (0, 1536), (0, 2048)])
def test_float_rows_match_oracle(gpu, oracle, fmt, d, metric):
    """Gaussian rows at one width per template no other test runs, under the contract of
    test_resident_bfs_matches_oracle."""
    rng = np.random.default_rng(d + fmt)
    n, nq, R, L = 2048, 64, 32, 128
    x = rng.standard_normal((n, d)).astype(np.float32)
    qs = (x[rng.integers(0, n, nq)] + 0.1 * rng.standard_normal((nq, d))).astype(np.float32)
    adj = B._ragged_graph(oracle, x, R, rng)
    eps = [17, 17, 1500, n + 3]
    if fmt == 0:
        db, kw = gpu.DiskannDeviceDB(x, 0), dict(vecs=x)
    else:
        mins, scale = oracle.sq8_train(x)
        codes = oracle.sq8_encode(x, mins, scale)
        db, kw = gpu.DiskannDeviceDB(codes, 1, mins, scale), dict(codes=codes, mins=mins, scale=scale)
    db.register_graph(adj)
    ids, dists, st = db.search_batch_resident(eps, qs, 10, L, metric)
    db.close()
    assert st["pops"] > 0 and st["host_requeries"] == 0
    oi, od, ost = oracle.diskann_search_batch(adj, eps, qs, 10, L, metric, **kw)
    same = ids == oi
    print(f"ids equal {same.mean():.4f} evals {st['evals']} / {ost['evals']} steps {st['steps']} / {ost['steps']}")
    assert same.mean() >= 0.99
    assert np.allclose(dists[same], od[same], rtol=1e-5, atol=1e-4)
    assert abs(st["evals"] - ost["evals"]) <= 0.01 * ost["evals"]
    assert abs(st["steps"] - ost["steps"]) <= 2
    assert np.all(np.diff(dists, axis=1) >= 0)
