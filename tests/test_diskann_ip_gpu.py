"""GPU tests of the inner-product graph lifecycle: a handle whose graph metric is IP builds, prunes, grows
and shrinks its graph on the device by the crate's occluding rule.  The reference is tests/_vamana_ip_ref.py.  On
small-integer rows every partial sum and every t·d product is the same fp32 value in numpy and on the device, so pruned
rows and whole adjacencies are compared with array_equal; on real-valued rows the graph is held to its invariants, to
run-to-run identity and to the recall of the exact kNN-by-dot + random graph at the same degree."""
from __future__ import annotations

import numpy as np
import pytest

import _vamana_add_ref as A
import _vamana_ip_ref as VI
import _vamana_ref as V
from _vamana_ref import check_structure

pytestmark = pytest.mark.gpu
NONE = V.NONE
IP = 1
COUNTS = ("batches", "out_prunes", "back_prunes", "pools_truncated")

BUILD_CASES = {  # the "ints" and "dup4" shapes of test_diskann_build_gpu.py, and one entry-point-gap case
    "ints": dict(n=1500, d=16, R=16, L=32, batch_max=256, ep=0),
    "dup4": dict(n=1200, d=16, R=24, L=24, batch_max=128, ep=0),
    "gap": dict(n=300, d=16, R=8, L=16, batch_max=64, ep=137),
}


def ip_db(gpu, x):
    return gpu.DiskannDeviceDB(x, graph_metric=IP)


@pytest.mark.parametrize("d", [16, 100, 1536])
@pytest.mark.parametrize("kind", ["dup4", "ints"])
def test_prune_ip_exact(gpu, kind, d):
    x, targets, pools = VI.prune_inputs(kind, d)
    pair = VI.pair_ip(x)  # exact: integers below 2^24
    m = targets.size
    db = ip_db(gpu, x)
    for R in (1, 8, 32, 64):
        for alpha in (1.0, 1.2, 2.0):
            out = db.robust_prune(targets, pools, R, alpha)
            assert out.shape == (m, R)
            ref = np.full((m, R), NONE, np.uint32)
            for t in range(m):
                sel, _ = VI.prune_ip(x, int(targets[t]), pools[t], None, R, alpha, pair=pair)
                ref[t, :sel.size] = sel
            assert np.array_equal(out, ref), (kind, d, R, alpha, np.nonzero((out != ref).any(axis=1))[0][:5])
    db.close()


def build_rows(case):
    c = BUILD_CASES[case]
    rng = np.random.default_rng(77)
    if case == "dup4":
        return VI.dup4_rows(rng, c["n"] // 4, c["d"])
    return rng.integers(-8, 9, (c["n"], c["d"])).astype(np.float32)


@pytest.mark.parametrize("case", ["ints", "dup4", "gap"])
def test_build_ip_exact(gpu, oracle, case):
    c = BUILD_CASES[case]
    x = build_rows(case)
    db = ip_db(gpu, x)
    adj, st = db.build_graph(R=c["R"], L=c["L"], alpha=1.2, entry_point=c["ep"], batch_max=c["batch_max"])
    db.close()
    print(case, st)
    ref, counts = VI.build_ip(x, c["R"], c["L"], 1.2, c["ep"], c["batch_max"])
    assert np.array_equal(adj, ref), np.nonzero((adj != ref).any(axis=1))[0][:10]
    assert tuple(st[k] for k in COUNTS) == tuple(counts[k] for k in COUNTS)
    assert st["unreachable"] == int((~V.reachable(adj, c["ep"])).sum())


@pytest.fixture(scope="module")
def cont(gpu):
    """cont_rows(): the IP graph of the first 1000 rows, built once on the GPU."""
    x = A.cont_rows()
    db = ip_db(gpu, x[:1000])
    base, _ = db.build_graph(R=16, L=32, alpha=1.2, entry_point=0, batch_max=128)
    db.close()
    return {"x": x, "base": base}


@pytest.mark.parametrize("T", [0, 16])
def test_add_ip_exact(gpu, oracle, cont, T):
    x, base = cont["x"], cont["base"]
    db = ip_db(gpu, x[:1000])
    db.register_graph(base)
    adj, st = db.add_rows(x[1000:], 0, L=32, alpha=1.2, batch_max=128, batch_mates=T)
    assert db.n == 1500
    db.close()
    ref, counts = VI.add_ip(x, base, 1000, 16, 32, 1.2, 0, 128, T)
    print(T, st, counts)
    assert np.array_equal(adj, ref), np.nonzero((adj != ref).any(axis=1))[0][:10]
    for k in COUNTS + ("mate_ids",):
        assert st[k] == counts[k], k
    assert st["unreachable"] == int((~V.reachable(adj, 0)).sum())


@pytest.mark.parametrize("b,d,T", [(2, 16, 8), (65, 100, 16), (300, 1536, 64)])
def test_batch_mates_ip_exact(gpu, b, d, T):
    row0 = 5
    x = np.random.default_rng(500 + b).integers(-8, 9, (row0 + b + 3, d)).astype(np.float32)
    db = ip_db(gpu, x)
    out = db.batch_mates(row0, b, T)
    db.close()
    ref = VI.mates_ip(x[row0:row0 + b], T)
    ref = np.where(ref == NONE, ref, ref + np.uint32(row0)).astype(np.uint32)
    assert np.array_equal(out, ref), np.nonzero((out != ref).any(axis=1))[0][:5]


def test_remove_ip_exact(gpu, oracle):
    n, R = 600, 16
    x = np.random.default_rng(91).integers(-8, 9, (n, 16)).astype(np.float32)
    db = ip_db(gpu, x)
    adj, _ = db.build_graph(R=R, L=32, alpha=1.2, entry_point=0, batch_max=128)
    r2 = np.random.default_rng(92)
    gone = np.concatenate([[0], 1 + r2.permutation(n - 1)[:59]])  # 60 rows, the entry point among them
    labels = np.concatenate([gone, gone[:5], [-1, n + 3]])
    labels = labels[r2.permutation(labels.size)].astype(np.int64)
    radj, rep, live, counts = VI.consolidate_ip(x, adj, labels, 0, 1.2, pair=VI.pair_ip(x))
    nadj, nep, st = db.remove_ids(labels, 0)
    assert db.n == live.size == n - 60
    db.close()
    print(st, counts)
    assert nadj.shape == radj.shape and np.array_equal(nadj, radj), np.nonzero((nadj != radj).any(axis=1))[0][:10]
    assert nep == rep
    for k in ("removed", "repaired", "pools_truncated", "pool_ids", "entry_replaced"):
        assert st[k] == counts[k], k
    assert st["entry_replaced"] == 1 and st["repaired"] > 0
    assert st["unreachable"] == int((~V.reachable(radj, rep)).sum())


def recall_resident_ip(db, x, oracle, q, L, ep):
    ids, _, _ = db.search_batch_resident([ep], q, 10, L, metric=IP)
    _, truth = oracle.flat_search(x, q, 10, metric=IP)
    return float(np.mean([len(set(ids[i]) & set(truth[i])) / 10.0 for i in range(q.shape[0])]))


def test_build_ip_real_valued(gpu, oracle):
    n, d, R, L = 2048, 32, 32, 64
    x = np.random.default_rng(3).standard_normal((n, d)).astype(np.float32)
    q = np.random.default_rng(4).standard_normal((200, d)).astype(np.float32)
    db = ip_db(gpu, x)
    adj, st = db.build_graph(R=R, L=L, alpha=1.2, entry_point=0, batch_max=256)
    check_structure(adj, R)
    unreached = int((~V.reachable(adj, 0)).sum())
    print("build stats", st, "unreachable (numpy)", unreached)
    assert st["unreachable"] == unreached
    r_build = recall_resident_ip(db, x, oracle, q, L, 0)  # the graph build_graph left registered
    adj2, st2 = db.build_graph(R=R, L=L, alpha=1.2, entry_point=0, batch_max=256)
    assert np.array_equal(adj, adj2)
    assert {k: v for k, v in st.items() if not k.endswith("_s")} == {k: v for k, v in st2.items() if not k.endswith("_s")}
    db.register_graph(VI.knn_random_graph_ip(x, R))
    r_knn = recall_resident_ip(db, x, oracle, q, L, 0)
    db.close()
    print(f"recall@10 at L={L}: build {r_build:.4f}, kNN-by-dot+random {r_knn:.4f}")
    assert r_build >= r_knn


def test_graph_metric_contract(gpu):
    rng = np.random.default_rng(10)
    x = rng.standard_normal((300, 16)).astype(np.float32)
    q = rng.standard_normal((20, 16)).astype(np.float32)
    plain = gpu.DiskannDeviceDB(x)
    assert plain.graph_metric == 0  # the default handle is L2 ...
    plain.build_graph(R=8, L=16, entry_point=0, batch_max=64)  # ... and metric=None follows it
    with pytest.raises(gpu.HipAnnError) as e:
        plain.build_graph(R=8, L=16, entry_point=0, batch_max=64, metric=IP)
    assert "IP is not supported" in str(e.value)  # the L2 handle's message, word for word
    for bad in (2, -1, 7):
        with pytest.raises(gpu.HipAnnError):
            plain.graph_metric = bad
        assert plain.graph_metric == 0
    plain.graph_metric = IP  # after a graph is registered
    assert plain.graph_metric == IP
    plain.graph_metric = 0
    plain.close()
    with pytest.raises(gpu.HipAnnError):
        gpu.DiskannDeviceDB(x, graph_metric=2)

    db = ip_db(gpu, x)
    assert db.graph_metric == IP
    adj, _ = db.build_graph(R=8, L=16, entry_point=0, batch_max=64)  # metric=None: IP
    adj1, _ = db.build_graph(R=8, L=16, entry_point=0, batch_max=64, metric=IP)
    assert np.array_equal(adj, adj1)
    want = db.search_batch_resident([0], q, 5, 16, metric=IP)[0]
    pools = np.zeros((1, 4), np.uint32)
    calls = [lambda: db.build_graph(R=8, L=16, entry_point=0, batch_max=64, metric=0),
             lambda: db.robust_prune([1], pools, 8, 1.2, metric=0),
             lambda: db.add_rows(x[:4], 0, L=16, batch_max=64, metric=0),
             lambda: db.remove_ids([3], 0, metric=0)]
    for call in calls:
        with pytest.raises(gpu.HipAnnError) as e:
            call()
        assert "IP" in str(e.value)  # the message names the handle's metric
        assert db.n == 300
        assert np.array_equal(db.search_batch_resident([0], q, 5, 16, metric=IP)[0], want)  # the graph still serves
    assert db.robust_prune([1], pools, 8, 1.2).shape == (1, 8)  # metric=None: IP
    sq = db.quantize_sq8()
    assert sq.graph_metric == IP and sq.R == 8  # the metric survives quantize_sq8 ...
    with pytest.raises(gpu.HipAnnError) as e:
        sq.add_rows(x[:4], 0, L=16, batch_max=64)  # ... and the SQ8 handle still refuses the maintenance calls
    assert "SQ8" in str(e.value)
    sq.close()
    db.close()


def test_ip_round_trip(gpu, tmp_path):
    import diskann_format as F

    x = np.random.default_rng(8).standard_normal((1000, 32)).astype(np.float32)
    q = np.random.default_rng(9).standard_normal((50, 32)).astype(np.float32)
    db = ip_db(gpu, x)
    ep = db.medoid()
    adj, _ = db.build_graph(R=16, L=32, alpha=1.2, entry_point=ep, batch_max=128)
    ids, dist, _ = db.search_batch_resident([ep], q, 10, 32, metric=IP)
    db.close()
    path = tmp_path / "built_ip.diskann"
    F.write_index(path, x, adj, [ep], metric=IP, build_complexity=32)
    f = F.open_index(path)
    assert f.metric == IP and f.max_degree == 16 and f.entry_points.tolist() == [ep]
    assert np.array_equal(f.adjacency, adj)
    db2 = gpu.DiskannDeviceDB(np.asarray(f.vectors), graph_metric=int(f.metric))
    db2.register_graph(np.asarray(f.adjacency))
    ids2, dist2, _ = db2.search_batch_resident(f.entry_points, q, 10, 32, metric=int(f.metric))
    db2.close()
    assert np.array_equal(ids, ids2) and np.array_equal(dist, dist2)
