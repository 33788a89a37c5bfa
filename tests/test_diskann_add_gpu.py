"""GPU tests of row insertion into the device DiskANN graph (diskann_hip_add_rows / diskann_hip_batch_mates, DESIGN
§6.3) against its numpy restatement (tests/_vamana_add_ref.py).  On small-integer rows every partial sum is exact in
fp32, so mates and whole adjacencies are compared with array_equal; on real-valued rows the graph is held to its
invariants, to run-to-run identity and to the recall margins of the restatement (tests/test_vamana_add_ref.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import _vamana_add_ref as A
import _vamana_ref as V
from _vamana_add_ref import burst_data, cont_rows
from _vamana_ref import check_structure

pytestmark = pytest.mark.gpu
NONE = V.NONE
COUNTS = ("batches", "out_prunes", "back_prunes", "pools_truncated")


def dup4_rows(rng, base, d):
    """`base` rows of values 0..3, every row four times (zero distances and ties everywhere), shuffled."""
    x = np.repeat(rng.integers(0, 4, (base, d)), 4, axis=0).astype(np.float32)
    return np.ascontiguousarray(x[rng.permutation(x.shape[0])])


def sparse_rows(rng, d=16):
    """Every row of values 0..3 with at most two non-zero coordinates (1129 distinct rows at d = 16), shuffled: whole
    distance classes larger than the traversal's spill list (tests/test_diskann_build_gpu.py, "ties")."""
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


def mates_ref(xb, T, row0):
    m = A.mates(xb, T)
    return np.where(m == NONE, NONE, m + np.uint32(row0)).astype(np.uint32)


MATES_SHAPES = [(1, 16, 8), (2, 16, 8), (33, 4, 1), (65, 100, 16), (300, 1536, 64), (257, 2048, 64)]


@pytest.mark.parametrize("b,d,T", MATES_SHAPES)
def test_mates_exact(gpu, b, d, T):
    rng = np.random.default_rng(3000 + b + d)
    for kind in ("ints", "dup4"):
        if kind == "ints":
            xb = rng.integers(-8, 9, (b, d)).astype(np.float32)
        else:
            xb = dup4_rows(rng, (b + 3) // 4, d)[:b]
        for row0 in (0, 37):
            x = np.concatenate([rng.integers(-8, 9, (row0, d)).astype(np.float32), xb])
            db = gpu.DiskannDeviceDB(x)
            out = db.batch_mates(row0, b, T)
            db.close()
            ref = mates_ref(xb, T, row0)
            assert out.shape == (b, T)
            assert np.array_equal(out, ref), (kind, row0, np.nonzero((out != ref).any(axis=1))[0][:5])
            assert ((out != NONE).sum(axis=1) == min(T, b - 1)).all()
    # real-valued rows: the same answer from run to run, and a sane one
    xr = rng.standard_normal((b, d)).astype(np.float32)
    db = gpu.DiskannDeviceDB(xr)
    o1 = db.batch_mates(0, b, T)
    o2 = db.batch_mates(0, b, T)
    db.close()
    assert np.array_equal(o1, o2)
    assert not (o1 == np.arange(b, dtype=np.uint32)[:, None]).any()
    if b > 1 and b * b * d < 4e7:
        # the nearest mate is a nearest row, up to the Gram form's rounding: 3 sums of d products, each within
        # d·2^-24 of its magnitude (at most the larger squared norm)
        x64 = xr.astype(np.float64)
        nn = (x64 ** 2).sum(1)
        d2 = ((x64[:, None, :] - x64[None, :, :]) ** 2).sum(-1)
        np.fill_diagonal(d2, np.inf)
        tol = 4.0 * d * 2.0 ** -24 * (nn + nn.max())
        assert (d2[np.arange(b), o1[:, 0]] <= d2.min(axis=1) + tol).all()


def test_mates_rejections(gpu):
    x = np.zeros((10, 16), np.float32)
    db = gpu.DiskannDeviceDB(x)
    for row0, b, T in ((0, 10, 0), (0, 10, 65), (-1, 5, 4), (5, 6, 4)):
        with pytest.raises(gpu.HipAnnError) as e:
            db.batch_mates(row0, b, T)
        assert str(e.value)
    assert db.batch_mates(3, 0, 4).shape == (0, 4)
    db.close()
    odd = gpu.DiskannDeviceDB(np.zeros((10, 18), np.float32))
    with pytest.raises(gpu.HipAnnError):
        odd.batch_mates(0, 10, 4)
    odd.close()


@pytest.fixture(scope="module")
def cont(gpu, oracle):
    """The continuation input (tests/test_vamana_add_ref.py item 1): rows, the restatement's full build and the
    device's, shared by the tests below and left unchanged."""
    x = cont_rows()
    ref, ref_counts = V.build(x, 16, 32, 1.2, 0, 256)
    db = gpu.DiskannDeviceDB(x)
    full, full_st = db.build_graph(R=16, L=32, alpha=1.2, entry_point=0, batch_max=256)
    db.close()
    assert np.array_equal(full, ref)
    return dict(x=x, ref=ref, ref_counts=ref_counts, full=full, full_st=full_st)


def prefix_db(gpu, x, n0, R=16, L=32, batch_max=256):
    db = gpu.DiskannDeviceDB(x[:n0])
    base, st = db.build_graph(R=R, L=L, alpha=1.2, entry_point=0, batch_max=batch_max)
    return db, base, st


@pytest.mark.parametrize("n0", [512, 768, 1024])
def test_add_equals_build(gpu, cont, n0):
    x = cont["x"]
    db, _, st0 = prefix_db(gpu, x, n0)
    adj, st = db.add_rows(x[n0:], 0, L=32, alpha=1.2, batch_max=256, batch_mates=0)
    assert db.n == 1500 and adj.shape == (1500, 16)
    db.close()
    print(n0, st)
    assert np.array_equal(adj, cont["full"]), np.nonzero((adj != cont["full"]).any(axis=1))[0][:10]
    assert np.array_equal(adj, cont["ref"])
    for k in COUNTS:
        assert st[k] == cont["full_st"][k] - st0[k], k
    assert st["mate_ids"] == 0 and st["mates_s"] == 0.0
    assert st["unreachable"] == int((~V.reachable(adj, 0)).sum())


def test_add_equals_build_in_two_calls(gpu, cont):
    x = cont["x"]
    db, _, st0 = prefix_db(gpu, x, 768)
    a1, s1 = db.add_rows(x[768:1024], 0, L=32, batch_max=256, batch_mates=0)
    assert a1.shape == (1024, 16) and db.n == 1024
    a2, s2 = db.add_rows(x[1024:], 0, L=32, batch_max=256, batch_mates=0)
    db.close()
    assert np.array_equal(a2, cont["full"])
    for k in COUNTS:
        assert s1[k] + s2[k] == cont["full_st"][k] - st0[k], k


@pytest.mark.parametrize("T", [1, 8])
def test_add_exact_with_mates(gpu, oracle, cont, T):
    x = cont["x"]
    db, base, _ = prefix_db(gpu, x, 768)
    adj, st = db.add_rows(x[768:], 0, L=32, alpha=1.2, batch_max=256, batch_mates=T)
    db.close()
    ref, counts = A.add(x, base, 768, 16, 32, 1.2, 0, 256, T)
    print(T, st, counts)
    assert np.array_equal(adj, ref), np.nonzero((adj != ref).any(axis=1))[0][:10]
    for k in COUNTS + ("mate_ids",):
        assert st[k] == counts[k], k
    assert not np.array_equal(adj, cont["full"])  # the mates do change the graph
    assert st["unreachable"] == int((~V.reachable(adj, 0)).sum())


def test_add_exact_with_mates_ties(gpu, oracle):
    """The input that overflows the traversal's spill list: flagged searches are re-run by the host BFS on a host
    adjacency that add_rows left behind the device's, so the refresh is exercised."""
    R, L, bm, n0, T = 24, 256, 128, 512, 8
    x = sparse_rows(np.random.default_rng(77), 16)
    db, base, _ = prefix_db(gpu, x, n0, R=R, L=L, batch_max=bm)
    adj, st = db.add_rows(x[n0:], 0, L=L, alpha=1.2, batch_max=bm, batch_mates=T)
    db.close()
    print("ties", st)
    ref, counts = A.add(x, base, n0, R, L, 1.2, 0, bm, T)
    assert np.array_equal(adj, ref), np.nonzero((adj != ref).any(axis=1))[0][:10]
    for k in COUNTS + ("mate_ids",):
        assert st[k] == counts[k], k
    assert st["host_requeries"] > 0, "the input no longer overflows the spill list: the host re-run went untested"


def recall_resident(db, x, oracle, q, L, ep=0):
    ids, _, _ = db.search_batch_resident([ep], q, 10, L)
    _, truth = oracle.flat_search(x, q, 10)
    return float(np.mean([len(set(ids[i]) & set(truth[i])) / 10.0 for i in range(q.shape[0])]))


def test_add_real_valued(gpu, oracle):
    R, L = 16, 32
    x_old, x_new, q_new = burst_data()
    x = np.ascontiguousarray(np.concatenate([x_old, x_new]))

    def added(T):
        db = gpu.DiskannDeviceDB(x_old)
        db.build_graph(R=R, L=L, alpha=1.2, entry_point=0, batch_max=256)
        adj, st = db.add_rows(x_new, 0, L=L, alpha=1.2, batch_max=512, batch_mates=T)
        return db, adj, st

    db, adj, st = added(16)
    check_structure(adj, R)
    unreached = int((~V.reachable(adj, 0)).sum())
    r16 = recall_resident(db, x, oracle, q_new, L)
    db.close()
    db2, adj2, st2 = added(16)
    db2.close()
    db0, adj0, st0 = added(0)
    r0 = recall_resident(db0, x, oracle, q_new, L)
    db0.close()
    dbb = gpu.DiskannDeviceDB(x)
    dbb.build_graph(R=R, L=L, alpha=1.2, entry_point=0, batch_max=256)
    rb = recall_resident(dbb, x, oracle, q_new, L)
    dbb.close()
    print(f"recall@10 at L={L} on q_new: batch_mates=16 {r16:.4f} (unreachable {unreached}), batch_mates=0 {r0:.4f} "
          f"(unreachable {st0['unreachable']}), build_graph over all rows {rb:.4f}")
    assert st["unreachable"] == unreached
    assert unreached <= 26
    assert r16 >= 0.95
    assert r16 >= rb
    assert r0 < 0.5
    assert np.array_equal(adj, adj2)
    assert {k: v for k, v in st.items() if not k.endswith("_s")} == {k: v for k, v in st2.items() if not k.endswith("_s")}


def fresh_answers(gpu, x, adj, q, ids, L):
    db = gpu.DiskannDeviceDB(x)
    db.register_graph(adj)
    out = (db.search_batch_resident([0], q, 5, L)[:2], db.distances_ids(q[:1], ids, np.zeros(len(ids), np.uint32)))
    db.close()
    return out


def test_add_growth_and_state(gpu, oracle, tmp_path):
    import diskann_format as F

    rng = np.random.default_rng(21)
    d, R, L, n0 = 16, 8, 16, 64
    sizes = [1, 1]
    while len(sizes) < 20:
        sizes.append(sizes[-1] + sizes[-2])
    total = n0 + sum(sizes)
    x = rng.integers(-8, 9, (total, d)).astype(np.float32)
    q = rng.integers(-8, 9, (20, d)).astype(np.float32)
    db = gpu.DiskannDeviceDB(x[:n0])
    adj, _ = db.build_graph(R=R, L=L, alpha=1.2, entry_point=0, batch_max=32)
    ref = adj
    n = n0
    for step, m in enumerate(sizes):
        want = step % 3 != 1  # every third call leaves the graph on the device
        got, st = db.add_rows(x[n:n + m], 0, L=L, alpha=1.2, batch_max=1024, batch_mates=4, want_adjacency=want)
        if step < 8:  # the first calls also against the restatement (54 rows)
            ref, _ = A.add(x[:n + m], ref, n, R, L, 1.2, 0, 1024, 4)
        n += m
        assert db.n == n and int(gpu.lib().diskann_hip_db_size(db._h)) == n
        if not want:
            assert got is None and st["unreachable"] == -1
            continue
        assert got.shape == (n, R) and st["unreachable"] == int((~V.reachable(got, 0)).sum())
        check_structure(got, R)
        if step < 8:
            assert np.array_equal(got, ref), step
        ids = np.asarray([0, n0 - 1, n - m, n - 1], np.uint32)  # old and new ids
        mine = (db.search_batch_resident([0], q, 5, L)[:2], db.distances_ids(q[:1], ids, np.zeros(4, np.uint32)))
        theirs = fresh_answers(gpu, x[:n], got, q, ids, L)
        assert np.array_equal(mine[0][0], theirs[0][0]) and np.array_equal(mine[0][1], theirs[0][1]), step
        assert np.array_equal(mine[1], theirs[1]), step
        adj = got
    assert n == total
    # add -> remove_ids -> add: ids stay dense and the handle answers as a fresh one
    dead = np.arange(10, n, 7)
    radj, ep, _ = db.remove_ids(dead, 0)
    keep = np.setdiff1d(np.arange(n), dead)
    extra = rng.integers(-8, 9, (50, d)).astype(np.float32)
    got, st = db.add_rows(extra, ep, L=L, batch_max=1024, batch_mates=4)
    xs = np.ascontiguousarray(np.concatenate([x[keep], extra]))
    assert db.n == xs.shape[0] and got.shape == (xs.shape[0], R)
    assert radj.shape == (keep.size, R)
    check_structure(got, R)
    ids = np.asarray([0, keep.size - 1, keep.size, xs.shape[0] - 1], np.uint32)
    i1, d1, _ = db.search_batch_resident([ep], q, 5, L)
    dd1 = db.distances_ids(q[:1], ids, np.zeros(4, np.uint32))
    db.close()
    db2 = gpu.DiskannDeviceDB(xs)
    db2.register_graph(got)
    i2, d2, _ = db2.search_batch_resident([ep], q, 5, L)
    dd2 = db2.distances_ids(q[:1], ids, np.zeros(4, np.uint32))
    db2.close()
    assert np.array_equal(i1, i2) and np.array_equal(d1, d2) and np.array_equal(dd1, dd2)
    # .diskann round trip of the grown graph
    path = tmp_path / "added.diskann"
    F.write_index(path, xs, got, [ep], metric=0, build_complexity=L)
    f = F.open_index(path)
    assert np.array_equal(f.adjacency, got) and f.max_degree == R
    db3 = gpu.DiskannDeviceDB(np.asarray(f.vectors))
    db3.register_graph(np.asarray(f.adjacency))
    i3, d3, _ = db3.search_batch_resident(f.entry_points, q, 5, L)
    db3.close()
    assert np.array_equal(i1, i3) and np.array_equal(d1, d3)


def test_add_rejections(gpu):
    rng = np.random.default_rng(10)
    x = rng.standard_normal((300, 16)).astype(np.float32)
    q = rng.standard_normal((20, 16)).astype(np.float32)
    new = rng.standard_normal((40, 16)).astype(np.float32)
    db = gpu.DiskannDeviceDB(x)
    with pytest.raises(gpu.HipAnnError) as e:  # no graph registered
        db.add_rows(new, 0, L=16)
    assert "graph" in str(e.value) and db.n == 300
    base, _ = db.build_graph(R=8, L=16, entry_point=0, batch_max=64)
    want = db.search_batch_resident([0], q, 5, 16)[:2]

    def unchanged(what):
        assert db.n == 300 and int(gpu.lib().diskann_hip_db_size(db._h)) == 300, what
        got = db.search_batch_resident([0], q, 5, 16)[:2]
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what

    nan_rows, inf_rows = new.copy(), new.copy()
    nan_rows[17, 3] = np.nan
    inf_rows[39, 15] = -np.inf
    bad = [dict(metric=1), dict(metric=2), dict(alpha=0.99), dict(alpha=float("nan")), dict(L=0), dict(L=257),
           dict(batch_max=0), dict(batch_mates=-1), dict(batch_mates=65), dict(entry_point=300),
           dict(rows=nan_rows), dict(rows=inf_rows)]
    for kw in bad:
        args = dict(rows=new, entry_point=0, L=16, alpha=1.2, batch_max=64, batch_mates=4)
        args.update(kw)
        with pytest.raises(gpu.HipAnnError) as e:
            db.add_rows(**args)
        assert str(e.value), kw
        unchanged(kw)
    # through the C ABI: rows NULL with m > 0, and n + m at 2^31 (refused before a row is read)
    lib, eb = gpu.lib(), C.create_string_buffer(1024)
    u32p = C.POINTER(C.c_uint32)
    rc = lib.diskann_hip_add_rows(db._h, None, 5, 16, 1.2, 0, 0, 64, 4, C.cast(None, u32p), None, eb, 1024)
    assert rc == -1 and eb.value
    unchanged("null rows")
    eb = C.create_string_buffer(1024)
    rc = lib.diskann_hip_add_rows(db._h, new.ctypes.data_as(C.POINTER(C.c_float)), 2 ** 31 - 300, 16, 1.2, 0, 0, 64, 4,
                                  C.cast(None, u32p), None, eb, 1024)
    assert rc == -1 and b"2^31" in eb.value
    unchanged("n + m = 2^31")
    # m = 0: nothing moves, the graph comes back as it is
    same, st = db.add_rows(np.zeros((0, 16), np.float32), 0, L=16)
    assert np.array_equal(same, base) and st["batches"] == 0 and st["out_prunes"] == 0
    unchanged("m = 0")
    # ... and the handle still takes rows
    adj, st = db.add_rows(new, 0, L=16, batch_max=64, batch_mates=4)
    assert db.n == 340 and adj.shape == (340, 8) and st["out_prunes"] == 40
    db.close()
    # shapes of the DB itself: SQ8 codes, d not a multiple of 4, d above 2048 (each with a graph registered)
    sq = gpu.DiskannDeviceDB(np.zeros((10, 16), np.uint8), fmt=1, sq8_min=np.zeros(16), sq8_scale=np.ones(16))
    odd = gpu.DiskannDeviceDB(rng.standard_normal((10, 18)).astype(np.float32))
    wide = gpu.DiskannDeviceDB(rng.standard_normal((10, 2052)).astype(np.float32))
    for bad_db in (sq, odd, wide):
        bad_db.register_graph(np.full((10, 4), NONE, np.uint32))
        with pytest.raises(gpu.HipAnnError) as e:
            bad_db.add_rows(np.zeros((2, bad_db.dim), np.float32), 0, L=8)
        assert str(e.value) and bad_db.n == 10
        bad_db.close()
