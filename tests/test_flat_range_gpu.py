"""Flat range search (hipann_flat_range_search*) against numpy in float64: per query the labels passing the strict
comparison (Σ(q−x)² < radius, IP: q·x > radius), in ascending label order.

Integer-valued data (entries in −4..4) make every form exact in fp32, so lims, labels and distances must equal the
reference exactly, rows sitting exactly on the radius included.  The Gaussian cases run the bf16 filter with real
residuals; each radius is the midpoint between the 20th and 21st neighbour of one test query, and for the fixed seed
no row of that query lies within 1e-4 relative of it (checked on the CPU when the cases were chosen, and asserted
below), so the float64 reference alone decides that query's membership.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
NQS = (1, 19, 20, 129)  # direct kernel, the threshold between the two kernels, a second query tile with a tail


def ints(seed, n, d):
    return np.random.default_rng(seed).integers(-4, 5, (n, d)).astype(np.float32)


def ref_dist(xb, xq, metric):
    x, q = xb.astype(np.float64), xq.astype(np.float64)
    ip = q @ x.T
    return ip if metric == IP else (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * ip


def ref_range(xb, xq, radius, metric):
    dist = ref_dist(xb, xq, metric)
    keep = dist > radius if metric == IP else dist < radius
    lims = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    return lims, dist[keep], np.nonzero(keep)[1].astype(np.int64)


def check_exact(got, xb, xq, radius, metric):
    lims, D, I = got
    rl, rD, rI = ref_range(xb, xq, radius, metric)
    assert lims.tolist() == rl.tolist()
    assert np.array_equal(I, rI)
    assert np.array_equal(D, rD.astype(np.float32))


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [1, 31, 32, 33, 100, 768])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_range_shapes_exact(gpu, n, d, metric):
    xb, xq = ints(n * 1000 + d, n, d), ints(7 + d, max(NQS), d)
    ix = gpu.HipIndexFlat(d, metric, xb)
    radius = float(np.sort(ref_dist(xb, xq[:1], metric)[0])[n // 2])  # an attained distance: those rows stay out
    for nq in NQS:
        check_exact(ix.range_search(xq[:nq], radius), xb, xq[:nq], radius, metric)


@pytest.mark.parametrize("nq", [3, 40])
@pytest.mark.parametrize("metric", [L2, IP])
def test_range_radius_edges(gpu, metric, nq):
    n, d = 3000, 32
    xb, xq = ints(1, n, d), ints(2, nq, d)
    ix = gpu.HipIndexFlat(d, metric, xb)
    dist = ref_dist(xb, xq, metric)
    attained = float(np.sort(dist[0])[n // 3])
    assert (dist == attained).any()
    everything, nothing = (dist.min() - 1, dist.max() + 1) if metric == IP else (dist.max() + 1, dist.min() - 1)
    for radius in (attained, float(nothing), float(everything), np.inf, -np.inf):
        check_exact(ix.range_search(xq, radius), xb, xq, radius, metric)
    lims, _, _ = ix.range_search(xq, float(everything))
    assert (np.diff(lims) == n).all()  # far beyond HIPANN_MAX_K
    again = ix.range_search(xq, attained)
    assert all(np.array_equal(a, b) for a, b in zip(again, ix.range_search(xq, attained)))


@pytest.mark.parametrize("nq", [3, 64])
@pytest.mark.parametrize("metric", [L2, IP])
def test_range_gaussian(gpu, metric, nq):
    n, d = 20000, 96
    rng = np.random.default_rng(20261126)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((64, d)).astype(np.float32)[:nq]
    ix = gpu.HipIndexFlat(d, metric, xb)
    dist = ref_dist(xb, xq, metric)
    Ds, Is = ix.search(xq, 32)
    for qi in (0, 1, 2):
        s = np.sort(dist[qi])
        radius = float(np.float32((s[-20] + s[-21]) / 2 if metric == IP else (s[19] + s[20]) / 2))
        assert (np.abs(dist[qi] - radius) > 1e-4 * abs(radius)).all()  # the reference alone is unambiguous
        lims, D, I = ix.range_search(xq, radius)  # the whole batch, so nq picks the kernel; query qi is judged
        want = np.nonzero(dist[qi] > radius if metric == IP else dist[qi] < radius)[0]
        assert len(want) == 20 and np.array_equal(I[lims[qi]:lims[qi + 1]], want)
        assert set(want) <= set(Is[qi].tolist())
        for q in range(nq):  # the same bits as the top-k call returns for the same rows
            got = dict(zip(I[lims[q]:lims[q + 1]].tolist(), D[lims[q]:lims[q + 1]].tolist()))
            top = dict(zip(Is[q].tolist(), Ds[q].tolist()))
            assert all(top[lab] == v for lab, v in got.items() if lab in top)


@pytest.mark.parametrize("metric", [L2, IP])
def test_range_after_add_and_remove(gpu, metric):
    d = 33
    xb, more, xq = ints(3, 600, d), ints(4, 300, d), ints(5, 40, d)
    ix = gpu.HipIndexFlat(d, metric, xb)
    radius = float(np.sort(ref_dist(xb, xq[:1], metric)[0])[len(xb) // 2])
    check_exact(ix.range_search(xq, radius), xb, xq, radius, metric)  # builds the image the add re-tiles
    ix.add(more)
    xb = np.concatenate([xb, more])
    gone = np.array([0, 5, 255, 256, 600, 899])
    for step in range(2):
        for nq in (3, 40):
            check_exact(ix.range_search(xq[:nq], radius), xb, xq[:nq], radius, metric)
        if step == 0:
            assert ix.remove_ids(gone) == len(gone)
            xb = np.delete(xb, gone, axis=0)


@pytest.mark.parametrize("nq", [3, 40])
def test_range_device_variant_cap(gpu, nq):
    import torch

    n, d = 1000, 32
    xb, xq = ints(8, n, d), ints(9, nq, d)
    radius = float(np.sort(ref_dist(xb, xq[:1], L2)[0])[n // 2])
    rl, rD, rI = ref_range(xb, xq, radius, L2)
    tb, tq = torch.from_numpy(xb).cuda(), torch.from_numpy(xq).cuda()
    ix = gpu.HipIndexFlatDevice(d, L2, tb.data_ptr(), n)
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
    assert np.array_equal(I.cpu().numpy(), rI) and np.array_equal(D.cpu().numpy(), rD.astype(np.float32))


@pytest.mark.parametrize("metric", [L2, IP])
def test_range_two_shards(gpu, metric):
    n, d = 1000, 33
    xb, xq = ints(10, n, d), ints(11, 40, d)
    ix = gpu.HipIndexFlat(d, metric, xb, devices=[0, 0])
    radius = float(np.sort(ref_dist(xb, xq[:1], metric)[0])[len(xb) // 2])
    for nq in (3, 40):
        check_exact(ix.range_search(xq[:nq], radius), xb, xq[:nq], radius, metric)


def test_range_arguments(gpu):
    xb = ints(12, 50, 8)
    ix = gpu.HipIndexFlat(8, L2, xb)
    lims, D, I = ix.range_search(np.zeros((0, 8), np.float32), 1.0)
    assert lims.tolist() == [0] and D.size == 0 and I.size == 0
    assert gpu.HipIndexFlat(8, L2).range_search(xb[:3], 1.0)[0].tolist() == [0, 0, 0, 0]
    with pytest.raises(gpu.HipAnnError):
        ix.range_search(xb[:3], float("nan"))
