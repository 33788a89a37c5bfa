"""GPU tests of the entry point and the SQ8 search copy computed on the device (diskann_hip_medoid,
diskann_hip_quantize_sq8, diskann_hip_export_sq8).

The codec is held to the committed restatement of Provider::quantize_sq8 (oracle.sq8_train / sq8_encode) value for
value: min / max are exact, and every step of a code is one IEEE fp32 operation, so equality is the bar.  A handle made
by quantize_sq8 holds the same bytes as one registered with the oracle's codes and runs the same kernels, so its
searches are compared with array_equal too.  The medoid is held to hipann.medoid: on small-integer rows every fp64 sum
is exact; on real-valued rows the test first shows in numpy that the runner-up is further than any summation order
can move a distance."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
L2, IP = 0, 1


def planted_rows(rng, n, d):
    """Standard-normal rows with four planted columns: constant; constant but for an outlier in the last row;
    all-negative; the integers 0..510 cycled with 0 and 510 present (normalized * 255 = v / 2: exact halves)."""
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[:, 0] = 1.5
    x[:, 1] = 0.25
    x[-1, 1] = 7.0
    x[:, 2] = -np.abs(x[:, 2]) - 0.5
    x[:, 3] = (np.arange(n) % 511).astype(np.float32)
    if n >= 2:
        x[0, 3], x[-1, 3] = 0.0, 510.0
    return np.ascontiguousarray(x)


def dup4_rows(rng, base, d):
    """`base` rows of values 0..3, every row four times (zero distances and ties everywhere), shuffled."""
    x = np.repeat(rng.integers(0, 4, (base, d)), 4, axis=0).astype(np.float32)
    return np.ascontiguousarray(x[rng.permutation(x.shape[0])])


def oracle_codec(x):
    mins, scale = O.sq8_train(x)
    return O.sq8_encode(x, mins, scale), mins, scale


def assert_codec(q8, x):
    codes, mins, scale = q8.export_sq8()
    rc, rm, rs = oracle_codec(x)
    assert np.array_equal(mins, rm), np.nonzero(mins != rm)[0][:5]  # (by value: a zero minimum may carry either sign)
    assert np.array_equal(scale, rs), np.nonzero(scale != rs)[0][:5]
    bad = np.argwhere(codes != rc)
    assert bad.size == 0, (len(bad), bad[:5])
    return rc, rm, rs


# d: the 16-dimension path, the 4-dimension path, the scalar path, a non-power-of-two d, the C4 width; n = 5000 is
# nine slabs of 512 rows and a remainder
@pytest.mark.parametrize("n", [1, 257, 5000])
@pytest.mark.parametrize("d", [16, 20, 18, 100, 1536])
def test_quantize_equals_codec(gpu, d, n):
    x = planted_rows(np.random.default_rng(100 * d + n), n, d)
    db = gpu.DiskannDeviceDB(x)
    q8 = db.quantize_sq8()
    assert (q8.n, q8.dim, q8.fmt, q8.R) == (n, d, gpu.DiskannDeviceDB.FMT_SQ8, 0)
    _, _, rs = assert_codec(q8, x)
    assert rs[0] == 1.0  # the constant column
    assert set(db.quantize_seconds) == {"stats_s", "encode_s", "rest_s"}
    assert all(v >= 0.0 for v in db.quantize_seconds.values())
    q8.close()
    db.close()


def same_search(a, b, adj, eps, q, k, L, metric):
    """ids, distances and stats of the resident search, the host BFS and the id gather, equal between two handles"""
    ia, da, sa = a.search_batch_resident(eps, q, k, L, metric)
    ib, dbb, sb = b.search_batch_resident(eps, q, k, L, metric)
    assert np.array_equal(ia, ib) and np.array_equal(da, dbb) and sa == sb, ("resident", metric, sa, sb)
    assert (ia >= 0).all()
    ia, da, sa = a.search_batch(adj, eps, q, k, L, metric)
    ib, dbb, sb = b.search_batch(adj, eps, q, k, L, metric)
    assert np.array_equal(ia, ib) and np.array_equal(da, dbb) and sa == sb, ("host bfs", metric, sa, sb)


def same_gather(a, b, rng, q, n, metric):
    ids = rng.integers(0, n, 500).astype(np.uint32)
    qm = rng.integers(0, q.shape[0], 500).astype(np.uint32)
    assert np.array_equal(a.distances_ids(q, ids, qm, metric), b.distances_ids(q, ids, qm, metric))


def test_quantized_handle_searches_like_registered_codes(gpu):
    rng = np.random.default_rng(11)
    n, d, R, L, nq, k = 3000, 64, 16, 32, 64, 10
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    db = gpu.DiskannDeviceDB(x)
    # a source without a graph: a handle without one, which still serves the id gather
    bare = db.quantize_sq8()
    codes, mins, scale = oracle_codec(x)
    ref = gpu.DiskannDeviceDB(codes, 1, mins, scale)
    assert bare.R == 0
    for metric in (L2, IP):
        same_gather(bare, ref, rng, q, n, metric)
    with pytest.raises(gpu.HipAnnError):
        bare.search_batch_resident([0], q, k, L, L2)
    bare.close()
    ep = db.medoid()
    adj, _ = db.build_graph(R=R, L=L, entry_point=ep)
    q8 = db.quantize_sq8()
    assert (q8.n, q8.dim, q8.fmt, q8.R) == (n, d, 1, R)
    ref.register_graph(adj)
    for metric in (L2, IP):
        same_search(q8, ref, adj, [ep], q, k, L, metric)
        same_gather(q8, ref, rng, q, n, metric)
    # L beyond the traversal kernel's 256: every query goes through the host BFS over the handle's own host copy of
    # the adjacency, which the quantized handle reads back from its device copy only now
    ia, da, sa = q8.search_batch_resident([ep], q[:8], k, 300, L2)
    ib, db_, sb = ref.search_batch_resident([ep], q[:8], k, 300, L2)
    assert sa["host_requeries"] == 8 and sa == sb
    assert np.array_equal(ia, ib) and np.array_equal(da, db_)
    for h in (q8, ref, db):
        h.close()


def test_source_unchanged(gpu):
    rng = np.random.default_rng(12)
    n, d, R, L, k = 2000, 32, 16, 32, 10
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((32, d)).astype(np.float32)
    db = gpu.DiskannDeviceDB(x)
    adj, _ = db.build_graph(R=R, L=L, entry_point=0)
    i0, d0, s0 = db.search_batch_resident([0], q, k, L)
    q8 = db.quantize_sq8()
    db.medoid()
    i1, d1, s1 = db.search_batch_resident([0], q, k, L)
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1) and s0 == s1
    assert (db.n, db.R, db.fmt) == (n, R, 0)
    assert int(gpu.lib().diskann_hip_db_size(db._h)) == n
    # the graph was copied, not borrowed: the copy outlives its source
    codes, mins, scale = oracle_codec(x)
    ref = gpu.DiskannDeviceDB(codes, 1, mins, scale)
    ref.register_graph(adj)
    db.close()
    del db
    same_search(q8, ref, adj, [0], q, k, L, L2)
    q8.close()
    ref.close()


def test_requantize_after_add_and_remove(gpu):
    rng = np.random.default_rng(13)
    n, d, R, L, k = 1200, 32, 16, 32, 10
    x = rng.standard_normal((n, d)).astype(np.float32)
    extra = (rng.standard_normal((300, d)) * 1.5 + 0.5).astype(np.float32)  # (moves the columns' min / max)
    q = rng.standard_normal((32, d)).astype(np.float32)
    db = gpu.DiskannDeviceDB(x)
    ep = 5
    adj, _ = db.build_graph(R=R, L=L, entry_point=ep)

    def check(rows, adj_now, ep_now):
        q8 = db.quantize_sq8()
        assert (q8.n, q8.R) == (rows.shape[0], R)
        codes, mins, scale = assert_codec(q8, rows)
        ref = gpu.DiskannDeviceDB(codes, 1, mins, scale)
        ref.register_graph(adj_now)
        same_search(q8, ref, adj_now, [ep_now], q, k, L, L2)
        q8.close()
        ref.close()

    check(x, adj, ep)
    adj1, _ = db.add_rows(extra, ep, L=L, batch_mates=8)  # (the rows now sit in a capacity larger than n)
    x1 = np.concatenate([x, extra])
    assert db.n == 1500
    check(x1, adj1, ep)
    labels = np.concatenate([[3, 3, 1499, 5000, -1], rng.choice(np.arange(16, 1499), 197, replace=False)])
    adj2, ep2, st = db.remove_ids(labels, ep)
    gone = np.unique(labels[(labels >= 0) & (labels < 1500)])
    assert st["removed"] == gone.size == 199 and db.n == 1500 - 199
    x2 = np.ascontiguousarray(np.delete(x1, gone, axis=0))
    check(x2, adj2, ep2)
    db.close()


def test_quantize_rejections(gpu):
    rng = np.random.default_rng(14)
    x = rng.standard_normal((600, 16)).astype(np.float32)
    q = rng.standard_normal((4, 16)).astype(np.float32)
    ids = np.arange(0, 590, dtype=np.uint32)
    qm = (ids % 4).astype(np.uint32)
    # an SQ8 source
    db = gpu.DiskannDeviceDB(x)
    q8 = db.quantize_sq8()
    before = q8.distances_ids(q, ids, qm)
    with pytest.raises(gpu.HipAnnError, match="SQ8"):
        q8.quantize_sq8()
    assert np.array_equal(q8.distances_ids(q, ids, qm), before)
    q8.close()
    db.close()
    # no rows
    empty = gpu.DiskannDeviceDB(np.empty((0, 16), np.float32))
    with pytest.raises(gpu.HipAnnError, match="no rows"):
        empty.quantize_sq8()
    empty.close()
    # a non-finite value (the last row, which the gather below leaves out)
    for bad in (np.nan, -np.inf):
        y = x.copy()
        y[599, 7] = bad
        db = gpu.DiskannDeviceDB(y)
        before = db.distances_ids(q, ids, qm)
        with pytest.raises(gpu.HipAnnError, match="non-finite"):
            db.quantize_sq8()
        assert np.array_equal(db.distances_ids(q, ids, qm), before)
        assert db.n == 600
        db.close()


@pytest.mark.parametrize("n", [1, 257, 5000])
@pytest.mark.parametrize("d", [16, 18, 100])
def test_medoid_integer_rows(gpu, d, n):
    """rows of small integers: the column sums and the mean's division are the same fp64 values on both sides"""
    x = np.random.default_rng(7 * d + n).integers(-8, 9, (n, d)).astype(np.float32)
    db = gpu.DiskannDeviceDB(x)
    assert db.medoid() == gpu.medoid(x)
    db.close()


@pytest.mark.parametrize("base,d", [(1, 16), (150, 16), (700, 18)])
def test_medoid_duplicated_rows(gpu, base, d):
    """every row four times: the smallest index among the equal rows wins"""
    x = dup4_rows(np.random.default_rng(base + d), base, d)
    want = gpu.medoid(x)
    assert want == int(np.nonzero((x == x[want]).all(axis=1))[0][0])
    db = gpu.DiskannDeviceDB(x)
    assert db.medoid() == want
    db.close()


# (n, d, seed): the seeds were checked on the CPU for the margin asserted below
@pytest.mark.parametrize("n,d,seed", [(257, 18, 1), (5000, 100, 2), (1100, 1536, 3), (3000, 64, 4)])
def test_medoid_real_rows(gpu, n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    c = x.mean(axis=0, dtype=np.float64)
    dd = np.sort(((x.astype(np.float64) - c) ** 2).sum(axis=1))
    # n + d fp64 additions per distance move it by less than (n + d) * 2^-52 relative: far inside this margin
    assert dd[1] - dd[0] > 1e-9 * dd[0]
    db = gpu.DiskannDeviceDB(x)
    assert db.medoid() == gpu.medoid(x)
    db.close()


def test_medoid_rejections(gpu):
    x = np.random.default_rng(15).standard_normal((100, 16)).astype(np.float32)
    db = gpu.DiskannDeviceDB(x)
    q8 = db.quantize_sq8()
    with pytest.raises(gpu.HipAnnError, match="SQ8"):
        q8.medoid()
    with pytest.raises(gpu.HipAnnError, match="SQ8|fp32"):
        db.export_sq8()
    q8.close()
    db.close()
    empty = gpu.DiskannDeviceDB(np.empty((0, 16), np.float32))
    with pytest.raises(gpu.HipAnnError, match="no rows"):
        empty.medoid()
    empty.close()


def test_run_to_run_identity(gpu):
    x = np.random.default_rng(16).standard_normal((5000, 100)).astype(np.float32)
    db = gpu.DiskannDeviceDB(x)
    a, b = db.quantize_sq8(), db.quantize_sq8()
    for u, v in zip(a.export_sq8(), b.export_sq8()):
        assert u.tobytes() == v.tobytes()
    assert db.medoid() == db.medoid()
    for h in (a, b, db):
        h.close()
