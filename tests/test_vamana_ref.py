"""CPU tests of the graph-build restatement (tests/_vamana_ref.py) and of the two build entry points'
behaviour without a DB handle."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import _vamana_ref as V
from _vamana_ref import check_structure, knn_random_graph


def pts(*rows):
    return np.asarray(rows, np.float32)


def test_prune_one_candidate():
    x = pts([0, 0], [1, 0])
    sel, tr = V.prune(x, 0, [1], None, 4, 1.2)
    assert sel.tolist() == [1] and not tr
    # the target itself, ids outside the DB, padding and repeats leave the pool
    sel, tr = V.prune(x, 0, [0, 1, 1, 7, V.NONE], None, 4, 1.2)
    assert sel.tolist() == [1] and not tr


def test_prune_zero_distance_pair():
    # rows 1 and 2 coincide: (dist, id) order puts 1 first, d(1, 2) = 0 makes 2's factor the largest float
    x = pts([0, 0], [1, 0], [1, 0], [0, 5])
    for alpha in (1.0, 1.2, 2.0):
        sel, _ = V.prune(x, 0, [2, 1, 3], None, 4, alpha)
        assert sel.tolist() == [1, 3]


def test_prune_rejected_at_1_admitted_at_1_2():
    # d(p, a) = 9, d(p, c) = 20, d(a, c) = 17: c's factor is 20/17 = 1.176, above 1.0 and below 1.2
    x = pts([0, 0], [3, 0], [2, 4])
    assert V.prune(x, 0, [1, 2], None, 4, 1.0)[0].tolist() == [1]
    assert V.prune(x, 0, [1, 2], None, 4, 1.2)[0].tolist() == [1, 2]
    # the traversal's distances are used as given
    assert V.prune(x, 0, [2, 1], [20.0, 9.0], 4, 1.2)[0].tolist() == [1, 2]


def test_prune_truncates_pool_to_256():
    # rows 1..299 on a line: row 1 is selected and gives every later row i the factor i² / (i − 1)² > 1.  Row 300 is
    # far off the line: selected whenever it is in the pool, but it is the 300th by distance
    x = np.zeros((301, 4), np.float32)
    x[1:300, 0] = np.arange(1, 300)
    x[300, 1] = 1000.0
    sel, tr = V.prune(x, 0, [1, 300], None, 8, 1.0)
    assert sel.tolist() == [1, 300] and not tr
    sel, tr = V.prune(x, 0, np.arange(1, 301), None, 8, 1.0)
    assert sel.tolist() == [1] and tr
    sel, tr = V.prune(x, 0, np.arange(1, 257), None, 8, 1.0)
    assert not tr


def test_prune_R_reached_mid_pass():
    # candidates on four axes: every pairwise distance exceeds the distances to p, so all pass at t = 1.0
    x = pts([0, 0, 0, 0], [1, 0, 0, 0], [0, 2, 0, 0], [0, 0, 3, 0], [0, 0, 0, 4])
    assert V.prune(x, 0, [4, 3, 2, 1], None, 8, 1.2)[0].tolist() == [1, 2, 3, 4]
    assert V.prune(x, 0, [4, 3, 2, 1], None, 2, 1.2)[0].tolist() == [1, 2]


@pytest.fixture(scope="module")
def ref_build(oracle):
    x = np.random.default_rng(3).standard_normal((2048, 32)).astype(np.float32)
    adj, counts = V.build(x, 16, 32, 1.2, 0, 256)
    return x, adj, counts


def recall_at_10(oracle, x, adj, queries, L, ep=0):
    ids, _, _ = oracle.diskann_search_batch(adj, [ep], queries, 10, L, 0, vecs=x)
    _, truth = oracle.flat_search(x, queries, 10)
    return float(np.mean([len(set(ids[i]) & set(truth[i])) / 10.0 for i in range(queries.shape[0])]))


def test_reference_build_structure(ref_build):
    x, adj, counts = ref_build
    check_structure(adj, 16)
    assert counts["out_prunes"] == 2047 and counts["batches"] == 9 + 6  # 1, 2, 4, ..., 256 (511 rows), then 6 x 256
    assert V.reachable(adj, 0).sum() >= 0.99 * 2048


def test_reference_build_recall_not_below_knn_graph(ref_build, oracle):
    x, adj, _ = ref_build
    q = np.random.default_rng(4).standard_normal((200, 32)).astype(np.float32)
    r_build = recall_at_10(oracle, x, adj, q, 32)
    r_knn = recall_at_10(oracle, x, knn_random_graph(x, 16), q, 32)
    print(f"recall@10 at L=32: build {r_build:.4f}, kNN+random {r_knn:.4f}")
    assert r_build >= r_knn


def test_build_entry_points_without_a_db(hipann_mod):
    """Both calls validate the handle before anything else: -1 and a message, with or without a device."""
    L = hipann_mod.lib()
    eb = C.create_string_buffer(256)
    assert L.diskann_hip_build_graph(None, 16, 32, 1.2, 0, 0, 256, None, None, eb, 256) == -1
    assert eb.value
    eb2 = C.create_string_buffer(256)
    t = (C.c_uint32 * 1)(0)
    assert L.diskann_hip_robust_prune(None, t, 1, t, 1, 16, 1.2, 0, t, eb2, 256) == -1
    assert eb2.value
    s = (C.c_double * 3)()
    assert L.diskann_hip_build_phase_seconds(None, s) == -1
