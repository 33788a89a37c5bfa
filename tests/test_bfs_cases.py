"""CPU checks of the inputs of tests/test_diskann_bfs_shapes_gpu.py (tests/_bfs_cases.py), against the oracle alone:
they are what keeps the GPU tests from passing vacuously.  For every (builder, d) pair the GPU tests run, every
distance is exact in fp32 in any summation order (sums below 2^24), SQ8 codes equal the values (min 0, range 255),
and the fp32 and SQ8 oracles agree bit for bit; the no-tie inputs have no ties, the tie-heavy inputs have many, the
spill input overflows a 64-entry spill list, and the Python model of the search equals the oracle.
"""
from __future__ import annotations

import numpy as np
import pytest

import _bfs_cases as B

WIDE = [(fmt, d) for fmt in (1, 0) for d in B.WIDE_DIMS[fmt]]
ONE_HOT = [(fmt, d) for fmt in (1, 0) for d in B.ONE_HOT_DIMS[fmt]]


def _sq8(oracle, x):
    mins, scale = oracle.sq8_train(x)
    codes = oracle.sq8_encode(x, mins, scale)
    assert np.all(mins == 0) and np.all(scale == 255)
    assert np.array_equal(codes.astype(np.float32), x)
    assert np.array_equal(oracle.sq8_decode(codes, mins, scale), x)
    return dict(codes=codes, mins=mins, scale=scale)


def _both_oracles(oracle, case, k, L, metric, rows=None, qs="qs"):
    """The fp32 and the SQ8 oracle on one case: exact data, codes == values, bit-identical results."""
    assert B.worst_sum(case, rows, qs) < 2 ** 24
    f = oracle.diskann_search_batch(case["adj"], case["eps"], case[qs], k, L, metric, vecs=case["x"])
    s = oracle.diskann_search_batch(case["adj"], case["eps"], case[qs], k, L, metric, **_sq8(oracle, case["x"]))
    assert np.array_equal(f[0], s[0])
    assert np.array_equal(f[1].view(np.uint32), s[1].view(np.uint32))
    assert f[2] == s[2]
    return f


@pytest.mark.parametrize("d", sorted({d for _, d in WIDE}))
def test_wide_sparse_inputs(oracle, d):
    case = B.wide_sparse(B.N, d, B.NQ, d)
    _, dists, st = _both_oracles(oracle, case, 128, 128, 0)
    assert B.tie_share(dists) <= 0.01              # ten times the largest share seen (0.001)
    assert st["evals"] >= 300 * B.NQ               # a traversal, not a handful of rows
    # IP, the dense-offset queries: the same bound
    _, dists, st = _both_oracles(oracle, case, 128, 128, 1, qs="qs_ip")
    assert B.tie_share(dists) <= 0.01
    assert st["evals"] >= 300 * B.NQ
    # IP, the sparse queries: exact and identical in both oracles, but tie-heavy (products collide, most are 0)
    _, dists, _ = _both_oracles(oracle, case, 128, 128, 1)
    assert B.tie_share(dists) > 0.01


@pytest.mark.parametrize("d", sorted({d for _, d in WIDE}))
def test_dense_ties_inputs(oracle, d):
    case = B.dense_ties(B.N, d, B.NQ, d)
    _, dists, st = _both_oracles(oracle, case, 128, 128, 0)
    assert B.tie_share(dists) >= 0.25              # every row is there 4 times
    assert st["evals"] >= 300 * B.NQ


@pytest.mark.parametrize("builder", [B.wide_sparse, B.dense_ties])
def test_depth_inputs(oracle, builder):
    case = builder(B.N, B.DEPTH_D, B.NQ, 5)
    for L in (1, 64, 256):
        _, dists, _ = _both_oracles(oracle, case, L, L, 0)
        if L > 1:
            assert (B.tie_share(dists) <= 0.01) if builder is B.wide_sparse else (B.tie_share(dists) >= 0.25)


@pytest.mark.parametrize("fmt,d", ONE_HOT)
def test_one_hot_inputs(oracle, fmt, d):
    dims = B.boundary_dims(d, fmt)
    dc, per = (8, 512) if fmt == 1 else (4, 256)
    assert 0 in dims and d - 1 in dims and len(set(dims)) == len(dims) <= 64
    for b in range(per, d, per):                   # both sides of every 64-lane round below d
        assert b - 1 in dims and b in dims
    assert all(v in dims for v in range(min(dc + 1, d)))
    case = B.one_hot_complete(d, dims)
    n = case["n_graph"]
    for metric in (0, 1):
        ids, dists, st = _both_oracles(oracle, case, n, 64, metric, rows=n)
        assert st["evals"] == 2 * n                # every graph row once per query, no calibration row
    ids, dists, _ = oracle.diskann_search_batch(case["adj"], [0], case["qs"][:1], n, 64, 0, vecs=case["x"])
    assert ids[0].tolist() == list(range(n)) and dists[0].tolist() == [(i + 1.0) ** 2 for i in range(n)]
    ids, dists, _ = oracle.diskann_search_batch(case["adj"], [0], case["qs"][1:], n, 64, 1, vecs=case["x"])
    assert ids[0].tolist() == list(range(n))[::-1] and dists[0].tolist() == [-(i + 1.0) for i in range(n)][::-1]


def test_spill_overflow_input(oracle):
    case = B.spill_overflow()
    L = case["L"]
    assert B.worst_sum(case) < 2 ** 24
    oi, od, _ = oracle.diskann_search_batch(case["adj"], case["eps"], case["qs"], L, L, 0, vecs=case["x"])
    mi, md, outstanding = B.model_search(case["x"], case["adj"], case["eps"], case["qs"][0], L, L)
    assert np.array_equal(mi, oi[0]) and np.array_equal(md, od[0])
    assert outstanding >= 65                       # the kernel's spill list holds 64
    assert np.sum(od[0] == 100.0) == L - 80 and np.all(np.diff(od[0]) >= 0)


def test_few_reachable_input(oracle):
    case = B.few_reachable()
    ids, dists, st = oracle.diskann_search_batch(case["adj"], case["eps"], case["qs"], 10, 16, 0, vecs=case["x"])
    assert np.all(ids[:, :5] >= 0) and np.all(ids[:, 5:] == -1)
    assert np.all(dists[:, 5:] == np.finfo(np.float32).max) and st["evals"] == 5 * len(case["qs"])
    assert sorted(ids[0, :5].tolist()) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("builder", [B.wide_sparse, B.dense_ties])
@pytest.mark.parametrize("metric", [0, 1])
def test_model_equals_oracle(oracle, builder, metric):
    case = builder(B.N, 260, B.NQ, 260)
    for L, k in ((128, 10), (20, 20)):
        oi, od, _ = oracle.diskann_search_batch(case["adj"], case["eps"], case["qs"][:3], k, L, metric,
                                                vecs=case["x"])
        for qi in range(3):
            mi, md, _ = B.model_search(case["x"], case["adj"], case["eps"], case["qs"][qi], k, L, metric)
            assert np.array_equal(mi, oi[qi]) and np.array_equal(md, od[qi])


def test_model_seed_rules(oracle):
    """Repeated and out-of-range entry points, more seeds than L (the list is truncated by the first insert)."""
    case = B.dense_ties(B.N, B.DEPTH_D, B.NQ, 5)
    for eps, L, k in (([40, 40, 5000, 47], 16, 5), (list(range(40, 60)), 8, 4)):
        oi, od, _ = oracle.diskann_search_batch(case["adj"], eps, case["qs"][:3], k, L, 0, vecs=case["x"])
        for qi in range(3):
            mi, md, _ = B.model_search(case["x"], case["adj"], eps, case["qs"][qi], k, L)
            assert np.array_equal(mi, oi[qi]) and np.array_equal(md, od[qi])


def test_repeated_ids_decide_the_result(oracle):
    """The host-path test of the GPU file gives every row its first id again in its last slot.  Which occurrence
    wins changes the order of that step's inserts, hence the place of tied rows: on this input the oracle's results
    differ between the two, so a search that let the later occurrence win would fail the exact comparison."""
    case = B.dense_ties(B.N, B.DEPTH_D, B.NQ, 5)
    first = B.repeat_first_last(case["adj"], B.N)
    last = B.repeat_first_last(case["adj"], B.N, winner="last")
    a = oracle.diskann_search_batch(first, case["eps"], case["qs"], 10, 64, 0, vecs=case["x"])
    b = oracle.diskann_search_batch(last, case["eps"], case["qs"], 10, 64, 0, vecs=case["x"])
    assert a[2]["evals"] > 300 * B.NQ
    assert not np.array_equal(a[0], b[0])
    for qi in range(3):
        mi, md, _ = B.model_search(case["x"], first, case["eps"], case["qs"][qi], 10, 64)
        assert np.array_equal(mi, a[0][qi]) and np.array_equal(md, a[1][qi])
