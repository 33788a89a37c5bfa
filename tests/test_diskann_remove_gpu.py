"""GPU tests of diskann_hip_remove_ids against its numpy restatement (tests/_vamana_remove_ref.py).  On
small-integer rows every partial sum is exact in fp32, so the whole adjacency, the entry point and the counters are
compared exactly; on real-valued rows the repaired graph is held to the build's invariants, to run-to-run identity and
to the recall of the exact kNN + random graph of the survivors at the same degree."""
from __future__ import annotations

import numpy as np
import pytest

import _vamana_ref as V
import _vamana_remove_ref as VR
from _vamana_ref import check_structure, knn_random_graph

pytestmark = pytest.mark.gpu
NONE = V.NONE

CASES = {  # the inputs of test_diskann_build_gpu.py::test_build_exact
    "ints": dict(n=1500, d=16, R=16, L=32, batch_max=256),
    "dup4": dict(n=1200, d=16, R=24, L=24, batch_max=128),
}
_built = {}


def exact_pair(x):
    """dist_to's values for integer rows: exact (integers below 2^24)."""
    xi = x.astype(np.int64)
    nn = (xi * xi).sum(1)
    return (nn[:, None] + nn[None, :] - 2 * (xi @ xi.T)).astype(np.float32)


def built(gpu, case):
    """(x, the graph the GPU builds, the removed labels as passed, the restatement's result), once per case."""
    if case not in _built:
        c = CASES[case]
        rng = np.random.default_rng(77)
        if case == "ints":
            x = rng.integers(-8, 9, (c["n"], c["d"])).astype(np.float32)
        else:
            x = np.repeat(rng.integers(0, 4, (c["n"] // 4, c["d"])), 4, axis=0).astype(np.float32)
            x = np.ascontiguousarray(x[rng.permutation(x.shape[0])])
        db = gpu.DiskannDeviceDB(x)
        adj, _ = db.build_graph(R=c["R"], L=c["L"], alpha=1.2, entry_point=0, batch_max=c["batch_max"])
        db.close()
        n = c["n"]
        r2 = np.random.default_rng(78)
        gone = np.concatenate([[0], 1 + r2.permutation(n - 1)[:n // 4 - 1]])  # 25 %, the entry point among them
        labels = np.concatenate([gone, gone[:7], [-1, n + 3]])  # duplicates and labels outside the DB
        labels = labels[r2.permutation(labels.size)].astype(np.int64)
        ref = VR.consolidate(x, adj, labels, 0, 1.2, pair=exact_pair(x))
        _built[case] = (x, adj, labels, ref)
    return _built[case]


def removed_handle(gpu, x, adj, labels, ep, **kw):
    db = gpu.DiskannDeviceDB(x)
    db.register_graph(adj)
    out = db.remove_ids(labels, ep, **kw)
    return db, out


def assert_matches(out, ref, n_before):
    adj, ep, st = out
    radj, rep, live, counts = ref
    print(st, counts)
    assert adj.shape == radj.shape and np.array_equal(adj, radj), np.nonzero((adj != radj).any(axis=1))[0][:10]
    assert ep == rep
    assert (st["removed"], st["repaired"], st["pools_truncated"]) == \
        (counts["removed"], counts["repaired"], counts["pools_truncated"])
    assert st["pool_ids"] == counts["pool_ids"]
    assert st["entry_replaced"] == counts["entry_replaced"]
    assert st["unreachable"] == int((~V.reachable(radj, rep)).sum())
    assert live.size == n_before - st["removed"]


@pytest.mark.parametrize("case", ["ints", "dup4"])
def test_remove_exact_built_graph(gpu, case):
    x, adj, labels, ref = built(gpu, case)
    db, out = removed_handle(gpu, x, adj, labels, 0)
    assert db.n == ref[2].size and out[2]["entry_replaced"] == 1
    db.close()
    assert_matches(out, ref, x.shape[0])


@pytest.mark.parametrize("d", [16, 100, 1536])
def test_remove_exact_full_degree_truncated_pools(gpu, d):
    """R = 64 rows of random ids (repeats and self loops kept, about 50 rows shortened by padding), half of the rows
    removed: pools of about a thousand ids, most of them cut to the 256 smallest."""
    n, R = 600, 64
    rng = np.random.default_rng(2000 + d)
    x = rng.integers(-8, 9, (n, d)).astype(np.float32)
    adj = rng.integers(0, n, (n, R)).astype(np.uint32)
    for p in rng.permutation(n)[:50]:
        adj[p, rng.integers(0, R):] = NONE
    ep = int(rng.integers(0, n))
    gone = np.concatenate([[ep], rng.permutation(np.delete(np.arange(n), ep))[:n // 2 - 1]]).astype(np.int64)
    ref = VR.consolidate(x, adj, gone, ep, 1.2, pair=exact_pair(x))
    db, out = removed_handle(gpu, x, adj, gone, ep)
    db.close()
    assert_matches(out, ref, n)
    assert out[2]["pools_truncated"] > 0, "the > 256 path went untested"


def test_remove_slab_independence(gpu):
    x, adj, labels, ref = built(gpu, "ints")
    R = adj.shape[1]
    db, base = removed_handle(gpu, x, adj, labels, 0)
    db.close()
    assert base[2]["slabs"] == 1
    for words in (R * (R + 1), 20000):
        db, out = removed_handle(gpu, x, adj, labels, 0, scratch_words=words)
        db.close()
        assert np.array_equal(out[0], base[0]) and out[1] == base[1]
        skip = ("slabs", "pool_s", "prune_s", "compact_s")
        assert {k: v for k, v in out[2].items() if k not in skip} == {k: v for k, v in base[2].items() if k not in skip}
        assert out[2]["slabs"] > 1 and out[2]["slabs"] != base[2]["slabs"]
        print(words, "words:", out[2]["slabs"], "slabs")


def test_remove_handle_afterwards(gpu):
    x, adj, labels, ref = built(gpu, "ints")
    radj, rep, live, _ = ref
    q = np.random.default_rng(79).integers(-8, 9, (40, x.shape[1])).astype(np.float32)
    db, (nadj, nep, _) = removed_handle(gpu, x, adj, labels, 0)
    fresh = gpu.DiskannDeviceDB(x[live])
    fresh.register_graph(nadj)
    assert db.n == fresh.n == live.size
    ids, dist, _ = db.search_batch_resident([nep], q, 10, 32)
    ids2, dist2, _ = fresh.search_batch_resident([nep], q, 10, 32)
    assert np.array_equal(ids, ids2) and np.array_equal(dist, dist2)
    every = np.arange(db.n, dtype=np.uint32)
    qm = np.zeros(db.n, np.uint32)
    assert np.array_equal(db.distances_ids(q[:1], every, qm), fresh.distances_ids(q[:1], every, qm))  # the rows moved
    fresh.close()
    # a second removal on the same handle: the restatement applied twice
    labels2 = np.random.default_rng(80).permutation(live.size)[:200].astype(np.int64)
    ref2 = VR.consolidate(x[live], radj, labels2, rep, 1.2, pair=exact_pair(x[live]))
    out2 = db.remove_ids(labels2, nep)
    assert_matches(out2, ref2, live.size)
    # build_graph -> remove_ids -> build_graph on one handle: a build of the survivors
    live2 = live[ref2[2]]
    assert db.n == live2.size
    again, _ = db.build_graph(R=16, L=32, alpha=1.2, entry_point=0, batch_max=256)
    db.close()
    fresh = gpu.DiskannDeviceDB(x[live2])
    want, _ = fresh.build_graph(R=16, L=32, alpha=1.2, entry_point=0, batch_max=256)
    fresh.close()
    assert np.array_equal(again, want)


def recall_resident(db, x, oracle, q, L, ep):
    ids, _, _ = db.search_batch_resident([ep], q, 10, L)
    _, truth = oracle.flat_search(x, q, 10)
    return float(np.mean([len(set(ids[i]) & set(truth[i])) / 10.0 for i in range(q.shape[0])]))


def test_remove_real_valued(gpu, oracle):
    n, d, R, L = 4096, 64, 32, 64  # the shape and seeds of test_build_real_valued
    x = np.random.default_rng(3).standard_normal((n, d)).astype(np.float32)
    q = np.random.default_rng(4).standard_normal((200, d)).astype(np.float32)
    gone = np.concatenate([[0], 1 + np.random.default_rng(5).permutation(n - 1)[:n // 4 - 1]]).astype(np.int64)
    live = np.setdiff1d(np.arange(n), gone)
    db = gpu.DiskannDeviceDB(x)
    adj, _ = db.build_graph(R=R, L=L, alpha=1.2, entry_point=0, batch_max=512)
    # the prune's own (dist, id) order names the row that must replace the removed entry point: with R = 1 it keeps
    # the first of the 256 smallest of the pool, here every live row
    nearest = int(db.robust_prune([0], live[None, :].astype(np.uint32), 1)[0, 0])
    nadj, nep, st = db.remove_ids(gone, 0)
    assert live[nep] == nearest, "the nearest live row is not the prune's"
    n2 = live.size
    assert db.n == n2 and nadj.shape == (n2, R) and st["removed"] == n // 4 and st["entry_replaced"] == 1
    check_structure(nadj, R)
    unreached = int((~V.reachable(nadj, nep)).sum())
    print("remove stats", st, "unreachable (numpy)", unreached)
    assert st["unreachable"] == unreached
    assert unreached <= n2 // 100
    xl = np.ascontiguousarray(x[live])
    r_removed = recall_resident(db, xl, oracle, q, L, nep)  # the graph remove_ids left registered
    db.close()
    # the same call on a second handle: identical
    db2, (nadj2, nep2, st2) = removed_handle(gpu, x, adj, gone, 0)
    assert np.array_equal(nadj, nadj2) and nep == nep2
    assert {k: v for k, v in st.items() if not k.endswith("_s")} == {k: v for k, v in st2.items() if not k.endswith("_s")}
    db2.register_graph(knn_random_graph(xl, R))
    r_knn = recall_resident(db2, xl, oracle, q, L, nep)
    db2.build_graph(R=R, L=L, alpha=1.2, entry_point=nep, batch_max=512)
    r_rebuilt = recall_resident(db2, xl, oracle, q, L, nep)  # recorded, not asserted
    db2.close()
    print(f"recall@10 at L={L}: removed {r_removed:.4f}, rebuilt {r_rebuilt:.4f}, kNN+random {r_knn:.4f}")
    assert r_removed >= r_knn


def small_graph(rng, n, d, R):
    x = rng.integers(-8, 9, (n, d)).astype(np.float32)
    adj = rng.integers(0, n, (n, R)).astype(np.uint32)
    return x, adj


@pytest.mark.parametrize("R", [1, 8])
def test_remove_small_degrees(gpu, R):
    rng = np.random.default_rng(90 + R)
    x, adj = small_graph(rng, 300, 16, R)
    gone = rng.permutation(300)[:90].astype(np.int64)
    ep = int(gone[0])
    ref = VR.consolidate(x, adj, gone, ep, 1.2, pair=exact_pair(x))
    db, out = removed_handle(gpu, x, adj, gone, ep)
    db.close()
    assert_matches(out, ref, 300)


@pytest.mark.parametrize("n", [3 * 32768 + 77, 257 * 32768 + 5])
def test_remove_rank_across_scan_blocks(gpu, n):
    """The rank (an exclusive prefix popcount over the removed-row bitmap) past one scan block (32768 rows) and past one
    chunk of the carry pass (256 blocks).  Few rows leave, spread over the whole range with the block edges among
    them, so the restatement prunes a few hundred rows while every surviving id is relabelled.  The removed entry point
    has many live rows at equal (integer) distance: the smallest id must win."""
    d, R = 4, 2
    rng = np.random.default_rng(n)
    x = rng.integers(-8, 9, (n, d)).astype(np.float32)
    adj = rng.integers(0, n, (n, R)).astype(np.uint32)
    ep = n - 1
    gone = np.concatenate([[ep, 0, 31, 32, 32767, 32768, 2 * 32768 - 1], rng.integers(0, n, 300)]).astype(np.int64)
    radj, rep, live, counts = VR.consolidate(x, adj, gone, ep, 1.2)
    db, (nadj, nep, st) = removed_handle(gpu, x, adj, gone, ep)
    print(st, counts)
    assert np.array_equal(nadj, radj) and nep == rep and db.n == live.size
    assert (st["removed"], st["repaired"], st["pools_truncated"], st["pool_ids"], st["entry_replaced"]) == \
        (counts["removed"], counts["repaired"], 0, counts["pool_ids"], 1)
    ids = np.concatenate([[0, live.size - 1], rng.integers(0, live.size, 1000)]).astype(np.uint32)
    got = db.distances_ids(x[:1], ids, np.zeros(ids.size, np.uint32))
    db.close()
    assert np.array_equal(got, V.dist_to(x, 0, live[ids]))  # the rows moved with their ids


def test_remove_rejections_and_edges(gpu):
    rng = np.random.default_rng(10)
    x = rng.standard_normal((300, 16)).astype(np.float32)
    q = rng.standard_normal((20, 16)).astype(np.float32)
    db = gpu.DiskannDeviceDB(x)
    with pytest.raises(gpu.HipAnnError) as e:  # no graph registered
        db.remove_ids([1, 2], 0)
    assert str(e.value) and db.n == 300
    adj, _ = db.build_graph(R=8, L=16, entry_point=0, batch_max=64)
    want = db.search_batch_resident([0], q, 5, 16)[0]
    bad = [dict(metric=1), dict(alpha=0.99), dict(alpha=float("nan")), dict(entry_point=300),
           dict(labels=np.arange(300)), dict(labels=np.arange(-5, 400))]  # the last two remove every row
    for kw in bad:
        args = dict(labels=[1, 2, 3], entry_point=0, alpha=1.2)
        args.update(kw)
        with pytest.raises(gpu.HipAnnError) as e:
            db.remove_ids(**args)
        assert str(e.value).startswith("hipann: remove_ids:"), (kw, str(e.value))  # the message names this call
        assert db.n == 300
        assert np.array_equal(db.search_batch_resident([0], q, 5, 16)[0], want), kw  # the old graph still serves
    # no label, or none in range: 0 removed, nothing moves, the current graph comes back
    for labels in ([], [-1, 300, 2 ** 40]):
        a0, ep0, s0 = db.remove_ids(labels, 7)
        assert np.array_equal(a0, adj) and ep0 == 7 and s0["removed"] == 0 and s0["slabs"] == 0 and db.n == 300
        assert np.array_equal(db.search_batch_resident([0], q, 5, 16)[0], want)
    # one survivor: a single all-padding row, and the removed entry point becomes row 0
    a1, ep1, s1 = db.remove_ids(np.delete(np.arange(300), 123), 5)
    assert a1.shape == (1, 8) and (a1 == NONE).all() and ep1 == 0 and db.n == 1
    assert s1["removed"] == 299 and s1["entry_replaced"] == 1 and s1["unreachable"] == 0
    ids, dist, _ = db.search_batch_resident([0], q[:3], 1, 4)
    assert (ids == 0).all() and np.allclose(dist[:, 0], ((q[:3] - x[123]) ** 2).sum(1), rtol=1e-5)
    db.close()
    # shapes of the DB and of the graph: SQ8 codes, d not a multiple of 4, d above 2048, R above 64
    ring = lambda n, R: ((np.arange(n)[:, None] + 1 + np.arange(R)[None, :]) % n).astype(np.uint32)  # noqa: E731
    sq = gpu.DiskannDeviceDB(np.zeros((10, 16), np.uint8), fmt=1, sq8_min=np.zeros(16), sq8_scale=np.ones(16))
    odd = gpu.DiskannDeviceDB(rng.standard_normal((10, 18)).astype(np.float32))
    wide = gpu.DiskannDeviceDB(rng.standard_normal((10, 2052)).astype(np.float32))
    fat = gpu.DiskannDeviceDB(rng.standard_normal((100, 16)).astype(np.float32))
    for bad_db, R in ((sq, 4), (odd, 4), (wide, 4), (fat, 65)):
        n0 = bad_db.n
        bad_db.register_graph(ring(n0, R))
        qb = rng.standard_normal((5, bad_db.dim)).astype(np.float32)
        before = bad_db.search_batch_resident([0], qb, 3, 8)
        with pytest.raises(gpu.HipAnnError) as e:
            bad_db.remove_ids([1], 0)
        assert str(e.value).startswith("hipann: remove_ids:") and bad_db.n == n0
        after = bad_db.search_batch_resident([0], qb, 3, 8)  # the old graph still serves
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        bad_db.close()
