"""GPU tests of the DiskANN graph build (diskann_hip_build_graph / diskann_hip_robust_prune) against its
numpy restatement (tests/_vamana_ref.py).  On small-integer rows every partial sum is exact in fp32, so the pruned rows
and the whole adjacency are compared with array_equal; on real-valued rows the graph is held to its invariants, to
run-to-run identity and to the recall of the exact kNN + random graph at the same degree."""
from __future__ import annotations

import numpy as np
import pytest

import _vamana_ref as V
from _vamana_ref import check_structure, knn_random_graph

pytestmark = pytest.mark.gpu
NONE = V.NONE


def dup4_rows(rng, base, d):
    """`base` rows of values 0..3, every row four times (zero distances and ties everywhere), shuffled."""
    x = np.repeat(rng.integers(0, 4, (base, d)), 4, axis=0).astype(np.float32)
    return np.ascontiguousarray(x[rng.permutation(x.shape[0])])


@pytest.mark.parametrize("d", [16, 100, 1536])
def test_prune_exact(gpu, d):
    rng = np.random.default_rng(1000 + d)
    n, m, cap = 600, 200, 300
    x = dup4_rows(rng, n // 4, d)
    xi = x.astype(np.int64)
    nn = (xi * xi).sum(1)
    pair = (nn[:, None] + nn[None, :] - 2 * (xi @ xi.T)).astype(np.float32)  # exact: integers below 2^24
    targets = rng.integers(0, n, m).astype(np.uint32)
    sizes = rng.choice([1, 2, 63, 64, 65, 128, 129, 255, 256, 300], m)
    sizes[:10] = [1, 2, 63, 64, 65, 128, 129, 255, 256, 300]  # each size at least once
    pools = np.full((m, cap), NONE, np.uint32)
    for t in range(m):
        s = int(sizes[t])
        ids = rng.integers(0, n, s).astype(np.uint32)  # with replacement: repeats
        if s >= 2:
            ids[rng.integers(0, s)] = targets[t]          # the target itself
            ids[rng.integers(0, s)] = n + rng.integers(0, 5)  # an id outside the DB
        if s >= 63:
            ids[rng.integers(0, s, 3)] = NONE  # padding inside the pool
        pools[t, rng.permutation(cap)[:s]] = ids  # ... and around it
    db = gpu.DiskannDeviceDB(x)
    for R in (1, 8, 32, 64):
        for alpha in (1.0, 1.2, 2.0):
            out = db.robust_prune(targets, pools, R, alpha)
            assert out.shape == (m, R)
            ref = np.full((m, R), NONE, np.uint32)
            for t in range(m):
                sel, _ = V.prune(x, int(targets[t]), pools[t], None, R, alpha, pair=pair)
                ref[t, :sel.size] = sel
            assert np.array_equal(out, ref), (d, R, alpha, np.nonzero((out != ref).any(axis=1))[0][:5])
    db.close()


def sparse_rows(rng, d=16):
    """Every row of values 0..3 with at most two non-zero coordinates (1129 distinct rows at d = 16), shuffled: from
    any row, hundreds of distinct rows sit at the same distance (e.g. 240 at a² + b² = 5 from the zero row)."""
    rows = [np.zeros(d)]
    for i in range(d):
        for a in (1, 2, 3):
            v = np.zeros(d)
            v[i] = a
            rows.append(v)
    for i in range(d):
        for j in range(i + 1, d):
            for a in (1, 2, 3):
                for b in (1, 2, 3):
                    v = np.zeros(d)
                    v[i], v[j] = a, b
                    rows.append(v)
    x = np.asarray(rows, np.float32)
    return np.ascontiguousarray(x[rng.permutation(x.shape[0])])


# "dup4" is the second input as specified.  It cannot overflow the traversal's spill list at any duplication: the list
# takes 64 entries evicted on a tie with result[L-1] while that threshold stands, at most L - 1 = 23 of them here, and
# a row's later copies are occluded by the first (zero distance), so most copies never enter a traversal (measured:
# host re-runs 0 for 4x, 20x, 60x and 100x at L 24..256).  "ties" is the input chosen so that searches do overflow
# (L = 256, whole distance classes larger than the spill list): 8 searches of that build are re-run on the host.
BUILD_CASES = {
    "ints": dict(n=1500, d=16, R=16, L=32, batch_max=256),
    "dup4": dict(n=1200, d=16, R=24, L=24, batch_max=128),
    "ties": dict(n=1129, d=16, R=24, L=256, batch_max=128),
}


@pytest.mark.parametrize("case", ["ints", "dup4", "ties"])
def test_build_exact(gpu, oracle, case):
    c = BUILD_CASES[case]
    rng = np.random.default_rng(77)
    if case == "ints":
        x = rng.integers(-8, 9, (c["n"], c["d"])).astype(np.float32)
    elif case == "dup4":
        x = dup4_rows(rng, c["n"] // 4, c["d"])
    else:
        x = sparse_rows(rng, c["d"])  # drives boundary-tie overflows of the traversal's spill list
        assert x.shape[0] == c["n"]
    db = gpu.DiskannDeviceDB(x)
    adj, st = db.build_graph(R=c["R"], L=c["L"], alpha=1.2, entry_point=0, batch_max=c["batch_max"])
    db.close()
    print(case, st)
    ref, counts = V.build(x, c["R"], c["L"], 1.2, 0, c["batch_max"])
    assert np.array_equal(adj, ref), np.nonzero((adj != ref).any(axis=1))[0][:10]
    assert (st["batches"], st["out_prunes"], st["back_prunes"], st["pools_truncated"]) == \
        (counts["batches"], counts["out_prunes"], counts["back_prunes"], counts["pools_truncated"])
    assert st["unreachable"] == int((~V.reachable(adj, 0)).sum())
    if case == "ties":
        assert st["host_requeries"] > 0, "the input no longer overflows the spill list: the host re-run went untested"


@pytest.mark.parametrize("ep", [137, 299])
def test_build_exact_entry_point_gap(gpu, ep):
    """The entry point inside the insertion order: a batch's rows are searched in two segments around it.  Row 137 falls
    inside the 64-row batch of insertion orders 127..190 (both segments non-empty); row 299 is the last row (the second
    segment always empty).  With entry_point=0, as in test_build_exact, the first segment never runs."""
    x = np.random.default_rng(77).integers(-8, 9, (300, 16)).astype(np.float32)
    db = gpu.DiskannDeviceDB(x)
    adj, st = db.build_graph(R=8, L=16, alpha=1.2, entry_point=ep, batch_max=64)
    db.close()
    print(ep, st)
    ref, counts = V.build(x, 8, 16, 1.2, ep, 64)
    assert np.array_equal(adj, ref), np.nonzero((adj != ref).any(axis=1))[0][:10]
    assert (st["batches"], st["out_prunes"], st["back_prunes"], st["pools_truncated"]) == \
        (counts["batches"], counts["out_prunes"], counts["back_prunes"], counts["pools_truncated"])
    assert st["unreachable"] == int((~V.reachable(ref, ep)).sum())


def recall_resident(db, x, oracle, q, L, ep):
    ids, _, _ = db.search_batch_resident([ep], q, 10, L)
    _, truth = oracle.flat_search(x, q, 10)
    return float(np.mean([len(set(ids[i]) & set(truth[i])) / 10.0 for i in range(q.shape[0])]))


def test_build_real_valued(gpu, oracle):
    n, d, R, L = 4096, 64, 32, 64
    x = np.random.default_rng(3).standard_normal((n, d)).astype(np.float32)
    q = np.random.default_rng(4).standard_normal((200, d)).astype(np.float32)
    db = gpu.DiskannDeviceDB(x)
    adj, st = db.build_graph(R=R, L=L, alpha=1.2, entry_point=0, batch_max=512)
    check_structure(adj, R)
    unreached = int((~V.reachable(adj, 0)).sum())
    print("build stats", st, "unreachable (numpy)", unreached)
    assert st["unreachable"] == unreached
    assert unreached <= n // 100
    r_build = recall_resident(db, x, oracle, q, L, 0)  # the graph build_graph left registered
    adj2, st2 = db.build_graph(R=R, L=L, alpha=1.2, entry_point=0, batch_max=512)
    assert np.array_equal(adj, adj2)
    assert {k: v for k, v in st.items() if not k.endswith("_s")} == {k: v for k, v in st2.items() if not k.endswith("_s")}
    db.register_graph(knn_random_graph(x, R))
    r_knn = recall_resident(db, x, oracle, q, L, 0)
    db.close()
    print(f"recall@10 at L={L}: build {r_build:.4f}, kNN+random {r_knn:.4f}")
    assert r_build >= r_knn


def test_build_round_trip(gpu, tmp_path):
    import diskann_format as F

    x = np.random.default_rng(8).standard_normal((1000, 32)).astype(np.float32)
    q = np.random.default_rng(9).standard_normal((50, 32)).astype(np.float32)
    db = gpu.DiskannDeviceDB(x)
    ep = gpu.medoid(x)
    assert ep == int(np.argmin(((x.astype(np.float64) - x.mean(0, dtype=np.float64)) ** 2).sum(1)))
    adj, _ = db.build_graph(R=16, L=32, alpha=1.2, entry_point=ep, batch_max=128)
    ids, dist, _ = db.search_batch_resident([ep], q, 10, 32)
    db.close()
    path = tmp_path / "built.diskann"
    F.write_index(path, x, adj, [ep], metric=0, build_complexity=32)
    f = F.open_index(path)
    assert f.max_degree == 16 and f.build_complexity == 32 and f.entry_points.tolist() == [ep]
    assert np.array_equal(f.adjacency, adj)
    db2 = gpu.DiskannDeviceDB(np.asarray(f.vectors))
    db2.register_graph(np.asarray(f.adjacency))
    ids2, dist2, _ = db2.search_batch_resident(f.entry_points, q, 10, 32)
    db2.close()
    assert np.array_equal(ids, ids2) and np.array_equal(dist, dist2)


def test_build_rejections(gpu):
    rng = np.random.default_rng(10)
    x = rng.standard_normal((300, 16)).astype(np.float32)
    q = rng.standard_normal((20, 16)).astype(np.float32)
    db = gpu.DiskannDeviceDB(x)
    adj, _ = db.build_graph(R=8, L=16, entry_point=0, batch_max=64)
    want = db.search_batch_resident([0], q, 5, 16)[0]
    bad = [dict(metric=1), dict(R=65), dict(R=0), dict(L=257), dict(L=0), dict(alpha=0.99), dict(alpha=float("nan")),
           dict(entry_point=300), dict(batch_max=0)]
    for kw in bad:
        args = dict(R=8, L=16, alpha=1.2, entry_point=0, batch_max=64)
        args.update(kw)
        with pytest.raises(gpu.HipAnnError) as e:
            db.build_graph(**args)
        assert str(e.value), kw
        assert np.array_equal(db.search_batch_resident([0], q, 5, 16)[0], want), kw  # the old graph still serves
    pools = np.zeros((1, 4), np.uint32)
    for kw in (dict(metric=1), dict(R=65), dict(alpha=0.5)):
        args = dict(R=8, alpha=1.2)
        args.update(kw)
        with pytest.raises(gpu.HipAnnError):
            db.robust_prune([1], pools, **args)
    with pytest.raises(gpu.HipAnnError):
        db.robust_prune([300], pools, 8)  # a target outside the DB
    db.close()
    # shapes of the DB itself: SQ8 codes, d not a multiple of 4, d above 2048
    sq = gpu.DiskannDeviceDB(np.zeros((10, 16), np.uint8), fmt=1, sq8_min=np.zeros(16), sq8_scale=np.ones(16))
    odd = gpu.DiskannDeviceDB(rng.standard_normal((10, 18)).astype(np.float32))
    wide = gpu.DiskannDeviceDB(rng.standard_normal((10, 2052)).astype(np.float32))
    for bad_db in (sq, odd, wide):
        with pytest.raises(gpu.HipAnnError) as e:
            bad_db.build_graph(R=4, L=8)
        assert str(e.value)
        with pytest.raises(gpu.HipAnnError):
            bad_db.robust_prune([1], pools, 4)
        bad_db.close()
    one = gpu.DiskannDeviceDB(x[:1])
    a1, s1 = one.build_graph(R=8, L=16)
    assert a1.shape == (1, 8) and (a1 == NONE).all() and s1["batches"] == 0 and s1["unreachable"] == 0
    one.close()
