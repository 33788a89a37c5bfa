"""CPU tests of the row-insertion restatement (tests/_vamana_add_ref.py), before the GPU is held to it:
an add without mates continues the build exactly when it starts at one of the build's batch boundaries, and on a burst
of mutually similar rows the mates are what makes the new rows findable."""
from __future__ import annotations

import numpy as np
import pytest

import _vamana_add_ref as A
from _vamana_add_ref import burst_data, cont_rows
import _vamana_ref as V

NONE = V.NONE


@pytest.fixture(scope="module")
def cont_full(oracle):
    x = cont_rows()
    return x, V.build(x, 16, 32, 1.2, 0, 256)


@pytest.mark.parametrize("n0", [512, 768, 1024])
def test_add_continues_build_at_batch_boundaries(oracle, cont_full, n0):
    x, (full, fc) = cont_full
    base, bc = V.build(x[:n0], 16, 32, 1.2, 0, 256)
    adj, ac = A.add(x, base, n0, 16, 32, 1.2, 0, 256, 0)
    assert np.array_equal(adj, full)
    for k in ("batches", "out_prunes", "back_prunes", "pools_truncated"):
        assert ac[k] == fc[k] - bc[k], k
    assert ac["mate_ids"] == 0


def test_add_off_a_boundary_differs(oracle, cont_full):
    # negative control: 300 is inside the build's batch 256..511, so the rows 300..511 see rows 256..299 already linked
    x, (full, _) = cont_full
    base, _ = V.build(x[:300], 16, 32, 1.2, 0, 256)
    adj, _ = A.add(x, base, 300, 16, 32, 1.2, 0, 256, 0)
    assert not np.array_equal(adj, full)
    V.check_structure(adj, 16)


def test_mates_small():
    x = np.asarray([[0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [5, 0, 0, 0]], np.float32)
    m = A.mates(x, 2)
    # rows 1 and 2 coincide (distance 0: the position decides among equals); row 0 sees both at 1
    assert m.tolist() == [[1, 2], [2, 0], [1, 0], [1, 2]]
    assert A.mates(x[:1], 3).tolist() == [[NONE, NONE, NONE]]
    assert A.mates(x[:2], 3).tolist() == [[1, NONE, NONE], [0, NONE, NONE]]


def recall_at_10(oracle, x, adj, q, L, ep=0):
    ids, _, _ = oracle.diskann_search_batch(adj, [ep], q, 10, L, 0, vecs=x)
    _, truth = oracle.flat_search(x, q, 10)
    return float(np.mean([len(set(ids[i]) & set(truth[i])) / 10.0 for i in range(q.shape[0])]))


def test_mates_make_a_burst_findable(oracle):
    R, L = 16, 32
    x_old, x_new, q_new = burst_data()
    x = np.ascontiguousarray(np.concatenate([x_old, x_new]))
    base, _ = V.build(x_old, R, L, 1.2, 0, 256)
    adj0, _ = A.add(x, base, 2048, R, L, 1.2, 0, 512, 0)
    adj16, c16 = A.add(x, base, 2048, R, L, 1.2, 0, 512, 16)
    rebuilt, _ = V.build(x, R, L, 1.2, 0, 256)
    V.check_structure(adj16, R)
    assert c16["mate_ids"] == 512 * 16
    r0, r16, rb = (recall_at_10(oracle, x, a, q_new, L) for a in (adj0, adj16, rebuilt))
    u0, u16 = (int((~V.reachable(a, 0)).sum()) for a in (adj0, adj16))
    print(f"recall@10 at L={L} on q_new: T=0 {r0:.4f} (unreachable {u0}), T=16 {r16:.4f} (unreachable {u16}), "
          f"rebuild {rb:.4f}")
    assert r16 >= 0.95
    assert r16 > rb
    assert r0 < 0.5
    assert u16 <= 26  # 1 % of the rows
