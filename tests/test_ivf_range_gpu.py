"""IVF range search (hipann_ivf_range_search*) against numpy in float64: per query the ids of the rows of its probed
lists passing the strict comparison (Σ(q−x)² < radius, IP: q·x > radius), in probe order, then list order.

Every index is built from a CSR with chosen list lengths and shuffled int64 ids, some above 2³².  Integer-valued data
(entries in −4..4) are exact in fp16 and fp32, so lims, ids, distances and the probe lists — float64 centroid
distances ordered by (distance, list id), the quantizer's tie rule — must equal the reference exactly, rows sitting
exactly on the radius included.  The Gaussian case runs the fp16 filter with real residuals; for its fixed seed no
row of the judged queries lies within 1e-4 relative of its radius and no adjacent coarse distances among a query's
first five lie that close (asserted below), so float64 alone decides membership and probe lists.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
LENS = (0, 1, 31, 32, 33, 2047, 2048, 2049, 4097)  # pass and chunk edges, an empty list


def dist64(x, q, metric):
    x, q = x.astype(np.float64), q.astype(np.float64)
    ip = q @ x.T
    return ip if metric == IP else (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * ip


def build(gpu, seed, d, lens, metric, nprobe=1, devices=None):
    rng = np.random.default_rng(seed)
    n, nlist = int(sum(lens)), len(lens)
    cen = rng.integers(-4, 5, (nlist, d)).astype(np.float32)
    codes = rng.integers(-4, 5, (n, d)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64) + np.where(rng.random(n) < 0.5, 1 << 33, 0)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return gpu.HipIndexIVFFlat(cen, off, ids, codes, nprobe=nprobe, metric=metric, devices=devices), cen, off, ids, codes


def ref_range(cen, off, ids, codes, xq, radius, metric, nprobe, pre=None):
    """(lims, D, I, probes) of the reference, in probe order and then list order.  pre: (centroid, row) distances."""
    cd, dist = pre if pre else (dist64(cen, xq, metric), dist64(codes, xq, metric))
    np_eff = min(nprobe, len(cen))
    probes = np.stack([np.lexsort((np.arange(len(cen)), -c if metric == IP else c))[:np_eff] for c in cd])
    D, I, lims = [], [], [0]
    for q, pl in enumerate(probes):
        rows = np.concatenate([np.arange(off[l], off[l + 1]) for l in pl]).astype(np.int64)
        keep = dist[q, rows] > radius if metric == IP else dist[q, rows] < radius
        D.append(dist[q, rows[keep]]), I.append(ids[rows[keep]]), lims.append(lims[-1] + int(keep.sum()))
    return np.array(lims), np.concatenate(D).astype(np.float32), np.concatenate(I), probes


def check_exact(got, ref):
    assert got[0].tolist() == ref[0].tolist()
    assert np.array_equal(got[2], ref[2])
    assert np.array_equal(got[1], ref[1])


def attained(codes, xq, metric):
    return float(np.sort(dist64(codes, xq[:1], metric)[0])[len(codes) // 3])


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [1, 31, 32, 33, 100, 768])
def test_range_shapes_exact(gpu, d, metric):
    ix, cen, off, ids, codes = build(gpu, 100 + d, d, LENS, metric)
    xq = np.random.default_rng(7 + d).integers(-4, 5, (130, d)).astype(np.float32)
    radius = attained(codes, xq, metric)  # an attained distance of query 0: those rows stay out
    cd, dist = dist64(cen, xq, metric), dist64(codes, xq, metric)
    for nprobe in (1, 3, len(LENS), len(LENS) + 5):  # (the last is clamped)
        for nq in (1, 19, 20, 130):  # at 130 with every list probed, more queries than the 96 of one wide item
            ref = ref_range(cen, off, ids, codes, xq[:nq], radius, metric, nprobe, (cd[:nq], dist[:nq]))
            check_exact(ix.range_search(xq[:nq], radius, nprobe=nprobe), ref)
            assert np.array_equal(ix.last_probes(nq, nprobe), ref[3])


@pytest.mark.parametrize("metric", [L2, IP])
def test_range_radius_edges(gpu, metric):
    d, nprobe = 32, 4
    ix, cen, off, ids, codes = build(gpu, 1, d, LENS, metric, nprobe=nprobe)
    xq = np.random.default_rng(2).integers(-4, 5, (40, d)).astype(np.float32)
    dist = dist64(codes, xq, metric)
    everything, nothing = (dist.min() - 1, dist.max() + 1) if metric == IP else (dist.max() + 1, dist.min() - 1)
    for radius in (attained(codes, xq, metric), float(nothing), float(everything), np.inf, -np.inf):
        check_exact(ix.range_search(xq, radius), ref_range(cen, off, ids, codes, xq, radius, metric, nprobe))
    lims, _, _ = ix.range_search(xq, float(everything))
    probed = np.diff(off)[ix.last_probes(len(xq))].sum(1)
    assert np.array_equal(np.diff(lims), probed) and probed.max() > 2048  # beyond HIPANN_MAX_K
    radius = attained(codes, xq, metric)
    assert all(np.array_equal(a, b) for a, b in zip(ix.range_search(xq, radius), ix.range_search(xq, radius)))


@pytest.mark.parametrize("nq", [3, 64])
@pytest.mark.parametrize("metric", [L2, IP])
def test_range_gaussian(gpu, metric, nq):
    rng = np.random.default_rng(20261127)
    xb = rng.standard_normal((20000, 96)).astype(np.float32)
    xq = rng.standard_normal((64, 96)).astype(np.float32)[:nq]
    cen = xb[rng.choice(20000, 16, replace=False)]
    cd = dist64(cen, xb, metric)
    assign = np.argmax(cd, 1) if metric == IP else np.argmin(cd, 1)
    order = np.argsort(assign, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=16))]).astype(np.int64)
    ids, codes = order.astype(np.int64), xb[order]
    ix = gpu.HipIndexIVFFlat(cen, off, ids, codes, nprobe=4, metric=metric)
    cq = np.sort(dist64(cen, xq, metric), 1)
    cq = cq[:, ::-1][:, :5] if metric == IP else cq[:, :5]
    assert (np.abs(np.diff(cq, axis=1)) > 1e-4 * np.abs(cq[:, 1:])).all()  # the probe lists are unambiguous
    Ds, Is = ix.search(xq, 32)
    pre = (dist64(cen, xq, metric), dist64(codes, xq, metric))
    dist, probes = pre[1], ref_range(cen, off, ids, codes, xq, 0.0, metric, 4, pre)[3]
    for qi in (0, 1, 2):
        rows = np.concatenate([np.arange(off[l], off[l + 1]) for l in probes[qi]])
        s = np.sort(dist[qi, rows])
        radius = float(np.float32((s[-20] + s[-21]) / 2 if metric == IP else (s[19] + s[20]) / 2))
        assert (np.abs(s - radius) > 1e-4 * abs(radius)).all()  # the reference alone decides membership
        ref = ref_range(cen, off, ids, codes, xq, radius, metric, 4, pre)
        lims, D, I = ix.range_search(xq, radius)  # the whole batch; query qi is judged
        assert np.array_equal(ix.last_probes(nq), ref[3])
        want = ref[2][ref[0][qi]:ref[0][qi + 1]]
        assert len(want) == 20 and np.array_equal(I[lims[qi]:lims[qi + 1]], want)
        for q in range(nq):  # the same bits as the top-k call returns for the same rows
            top = dict(zip(Is[q].tolist(), Ds[q].tolist()))
            got = zip(I[lims[q]:lims[q + 1]].tolist(), D[lims[q]:lims[q + 1]].tolist())
            assert all(top[lab] == v for lab, v in got if lab in top)
    if metric == L2:
        assert {2733, 3137, 4529} <= set(np.diff(off).tolist())  # multi-chunk lists


@pytest.mark.parametrize("metric", [L2, IP])
def test_range_after_add_and_remove(gpu, metric):
    d, nprobe = 33, 3
    ix, cen, _, _, codes = build(gpu, 3, d, (40, 2100, 0, 70, 2500), metric, nprobe=nprobe)
    rng = np.random.default_rng(4)
    more, xq = rng.integers(-4, 5, (300, d)).astype(np.float32), rng.integers(-4, 5, (40, d)).astype(np.float32)
    radius = attained(codes, xq, metric)

    def check():
        e = ix.export()
        for nq in (3, 40):
            ref = ref_range(cen, e["list_offsets"], e["ids"], e["codes"], xq[:nq], radius, metric, nprobe)
            check_exact(ix.range_search(xq[:nq], radius), ref)
        return e

    check()  # builds the image the add and the remove maintain
    ix.add(more, np.arange(300, dtype=np.int64) + (1 << 40))
    e = check()
    o, ids = e["list_offsets"], e["ids"]
    gone = [ids[o[1]], ids[o[2] - 1], ids[o[1] + 2050], ids[o[4]], ids[o[5] - 1], ids[o[0] + 5]]
    assert ix.remove_ids(np.array(gone)) == len(gone)
    check()


@pytest.mark.parametrize("metric", [L2, IP])
def test_range_nonfinite_codes_take_the_direct_kernel(gpu, metric):
    d, nprobe, lens = 33, 3, (40, 2100, 0, 70)
    rng = np.random.default_rng(5)
    cen, codes = rng.integers(-4, 5, (4, d)).astype(np.float32), rng.integers(-4, 5, (sum(lens), d)).astype(np.float32)
    codes[45, 7] = np.inf
    ids = rng.permutation(sum(lens)).astype(np.int64) + (1 << 33)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    xq = rng.integers(-4, 5, (25, d)).astype(np.float32)
    xq[:, 7] = np.abs(xq[:, 7]) + 1  # IP: q·x = +inf for the inf row (inside every radius); L2: +inf (outside)
    ix = gpu.HipIndexIVFFlat(cen, off, ids, codes, nprobe=nprobe, metric=metric)
    radius = attained(np.delete(codes, 45, 0), xq, metric)
    with np.errstate(invalid="ignore"):
        ref = ref_range(cen, off, ids, codes, xq, radius, metric, nprobe)
    check_exact(ix.range_search(xq, radius), ref)
    assert (ids[45] in ref[2]) == (metric == IP)


def test_range_device_variant_cap(gpu):
    import torch

    d, nprobe, nq = 32, 3, 40
    ix, cen, off, ids, codes = build(gpu, 8, d, (40, 2100, 0, 70, 2500), L2, nprobe=nprobe)
    xq = np.random.default_rng(9).integers(-4, 5, (nq, d)).astype(np.float32)
    radius = attained(codes, xq, L2)
    rl, rD, rI, _ = ref_range(cen, off, ids, codes, xq, radius, L2, nprobe)
    tq = torch.from_numpy(xq).cuda()
    lims = torch.full((nq + 1,), -7, dtype=torch.int64, device="cuda")
    D = torch.full((int(rl[-1]),), -7.0, dtype=torch.float32, device="cuda")
    I = torch.full((int(rl[-1]),), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert not ix.range_search_device(nq, tq.data_ptr(), radius, lims.data_ptr(), D.data_ptr(), I.data_ptr(), 1)
    torch.cuda.synchronize()
    assert lims.cpu().numpy().tolist() == rl.tolist()
    assert (D == -7).all() and (I == -7).all()  # too small a cap: the sentinels stay
    assert ix.range_search_device(nq, tq.data_ptr(), radius, lims.data_ptr(), D.data_ptr(), I.data_ptr(), int(rl[-1]))
    torch.cuda.synchronize()
    assert np.array_equal(I.cpu().numpy(), rI) and np.array_equal(D.cpu().numpy(), rD)


@pytest.mark.parametrize("metric", [L2, IP])
def test_range_two_shards(gpu, metric):
    d, nprobe = 33, 4
    one, cen, off, ids, codes = build(gpu, 10, d, LENS, metric, nprobe=nprobe)
    two = build(gpu, 10, d, LENS, metric, nprobe=nprobe, devices=[0, 0])[0]
    xq = np.random.default_rng(11).integers(-4, 5, (40, d)).astype(np.float32)
    radius = attained(codes, xq, metric)
    for nq in (3, 40):
        got = two.range_search(xq[:nq], radius)
        check_exact(got, ref_range(cen, off, ids, codes, xq[:nq], radius, metric, nprobe))
        assert all(np.array_equal(a, b) for a, b in zip(got, one.range_search(xq[:nq], radius)))


def test_range_arguments(gpu):
    ix, cen, off, _, codes = build(gpu, 12, 8, (5, 0, 45), L2)
    lims, D, I = ix.range_search(np.zeros((0, 8), np.float32), 1.0)
    assert lims.tolist() == [0] and D.size == 0 and I.size == 0
    empty = gpu.HipIndexIVFFlat(cen, np.zeros(4, np.int64), np.zeros(0, np.int64), np.zeros((0, 8), np.float32))
    assert empty.range_search(codes[:3], 1.0)[0].tolist() == [0, 0, 0, 0]
    with pytest.raises(gpu.HipAnnError):
        ix.range_search(codes[:3], float("nan"))
