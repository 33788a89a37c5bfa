"""CPU tests of the row-removal restatement (tests/_vamana_remove_ref.py) and of diskann_hip_remove_ids's
behaviour without a DB handle."""
from __future__ import annotations

import ctypes as C

import numpy as np

import _vamana_ref as V
import _vamana_remove_ref as VR

NONE = V.NONE


def pts(*rows):
    return np.asarray(rows, np.float32)


def graph(rows, R):
    adj = np.full((len(rows), R), NONE, np.uint32)
    for i, r in enumerate(rows):
        adj[i, :len(r)] = r
    return adj


# six points on a line at 0, 1, 2, 3, 4, 10
LINE = pts([0, 0], [1, 0], [2, 0], [3, 0], [4, 0], [10, 0])


def test_row_without_removed_neighbour_is_only_relabelled():
    # row 4 keeps its order, its repeat and its self loop; rows 0 and 5 point at the removed row 2 and are pruned
    adj = graph([[1, 2], [0, 3], [1, 3], [4, 1], [5, 3, 3, 4], [2, 4]], 4)
    new, ep, live, counts = VR.consolidate(LINE, adj, [2], 0, 1.2)
    assert live.tolist() == [0, 1, 3, 4, 5] and ep == 0
    assert new[1].tolist() == [0, 2, NONE, NONE]        # old row 1: [0, 3]
    assert new[2].tolist() == [3, 1, NONE, NONE]        # old row 3: [4, 1]
    assert new[3].tolist() == [4, 2, 2, 3]              # old row 4: [5, 3, 3, 4]
    # old row 0: pool {1} ∪ N(2) = {1, 3}; 3 is occluded by 1 (9 / 4 > 1.2)
    assert new[0].tolist() == [1, NONE, NONE, NONE]
    # old row 5: pool {4} ∪ {1, 3}: 4 first, then 3 (49 / 1) and 1 (81 / 9) are occluded
    assert new[4].tolist() == [3, NONE, NONE, NONE]
    assert counts == {"removed": 1, "repaired": 2, "pools_truncated": 0, "pool_ids": 6, "entry_replaced": 0}


def test_row_whose_pool_is_all_removed_becomes_empty():
    # row 0 points at 1 and 2 only, both removed, and their rows hold removed ids, row 0 itself excepted
    adj = graph([[1, 2], [2, 0], [1], [0], [3], [4]], 2)
    new, ep, live, counts = VR.consolidate(LINE, adj, [1, 2], 3, 1.2)
    assert live.tolist() == [0, 3, 4, 5] and ep == 1
    assert new[0].tolist() == [NONE, NONE]  # (the target itself leaves the pool)
    assert new[1].tolist() == [0, NONE] and new[2].tolist() == [1, NONE] and new[3].tolist() == [2, NONE]
    assert counts["repaired"] == 1 and counts["pool_ids"] == 1


def test_always_pruned_even_when_the_pool_fits():
    # row 0's pool {1, 3} has 2 ≤ R ids, yet 3 is occluded by 1: the row is pruned, not merely filtered
    adj = graph([[1, 2, 3], [0], [0], [0], [0], [0]], 3)
    new, _, _, counts = VR.consolidate(LINE, adj, [2], 0, 1.2)
    assert new[0].tolist() == [1, NONE, NONE] and counts["repaired"] == 1


def test_entry_point_replaced_by_nearest_live_row_ties_by_id():
    adj = graph([[1], [2], [3], [4], [5], [0]], 1)
    # rows 1 and 3 are both at distance 1 from the removed entry point 2: the smaller id wins
    new, ep, live, counts = VR.consolidate(LINE, adj, [2], 2, 1.2)
    assert live[ep] == 1 and counts["entry_replaced"] == 1
    # with 1 removed as well, 3 is the nearest
    _, ep, live, _ = VR.consolidate(LINE, adj, [1, 2], 2, 1.2)
    assert live[ep] == 3
    # an entry point that stays is only relabelled
    _, ep, live, counts = VR.consolidate(LINE, adj, [0, 1], 4, 1.2)
    assert ep == 2 and live[ep] == 4 and counts["entry_replaced"] == 0


def test_duplicate_and_out_of_range_labels_are_ignored():
    adj = graph([[1, 2], [0, 3], [1, 3], [4, 1], [5, 3], [2, 4]], 2)
    a = VR.consolidate(LINE, adj, [2, 4], 0, 1.2)
    b = VR.consolidate(LINE, adj, [4, 2, 2, -1, 6, 9, 4, 2 ** 40, -2 ** 40], 0, 1.2)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert a[3]["removed"] == 2
    # no label in range: nothing moves
    new, ep, live, counts = VR.consolidate(LINE, adj, [-1, 6], 5, 1.2)
    assert np.array_equal(new, adj) and ep == 5 and live.tolist() == list(range(6)) and counts["repaired"] == 0


def test_matches_a_rebuild_free_walk_on_a_built_graph(oracle):
    """On a built graph the result keeps the build's invariants and relabels exactly like np.delete."""
    x = np.random.default_rng(5).integers(-8, 9, (400, 8)).astype(np.float32)
    adj, _ = V.build(x, 8, 16, 1.2, 0, 64)
    labels = np.random.default_rng(6).permutation(400)[:100]
    new, ep, live, counts = VR.consolidate(x, adj, labels, 0, 1.2)
    assert np.array_equal(x[live], np.delete(x, labels, axis=0))
    V.check_structure(new, 8)
    assert counts["removed"] == 100 and 0 < counts["repaired"] <= 300 and 0 <= ep < 300


def test_remove_entry_point_without_a_db(hipann_mod):
    """The call validates the handle before anything else: -1 and a message, with or without a device."""
    L = hipann_mod.lib()
    eb = C.create_string_buffer(256)
    lab = (C.c_int64 * 2)(0, 1)
    ep = C.c_uint32(0)
    assert L.diskann_hip_remove_ids(None, lab, 2, 1.2, 0, C.byref(ep), 0, None, None, eb, 256) == -1
    assert eb.value
    s = (C.c_double * 3)()
    assert L.diskann_hip_remove_phase_seconds(None, s) == -1
