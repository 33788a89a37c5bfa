"""IVF SQ8 for 17 <= k <= 64: the 32-deep code scan (two gate classes above k = 32) and its rerank against the float64
references of test_ivf_sq8_gpu.  "filter_depth": the last call's scan depth (16 | 32), 0 for the direct kernel."""
import numpy as np
import pytest

from test_ivf_sq8_add_gpu import info  # hipann_debug_ivfsq_info(handle, name)
from test_ivf_sq8_gpu import IP, L2, LENS, build, decode64, dist64, exact_ref, ref_topk, tol_rows

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d", [1, 33, 100, 768])
@pytest.mark.parametrize("by_res", [0, 1])
@pytest.mark.parametrize("metric", [L2, IP])
def test_sq8_deep_shapes_exact(gpu, metric, by_res, d):
    ix, p, xh = build(gpu, d, metric, by_res)
    lim = 64 if d <= 100 else 4
    xq = np.random.default_rng(7 + d).integers(-lim, lim + 1, (130, d)).astype(np.float32)
    cd, dist = exact_ref(p, xh, xq, metric)
    for nprobe in (1, 3, len(LENS)):
        for k in (17, 32, 33, 64):  # 33 and 64: two gate classes
            rD, rI, rP = ref_topk(cd, dist, p["list_offsets"], p["ids"], metric, nprobe, k)
            for nq in (1, 20, 130):  # at 130 with every list probed, more queries than one scan item holds
                D, I = ix.search(xq[:nq], k, nprobe=nprobe)
                assert np.array_equal(I, rI[:nq]) and np.array_equal(D, rD[:nq].astype(np.float32))
                assert info(gpu, ix, "filter_depth") == 32 and np.array_equal(ix.last_probes(nq, nprobe), rP[:nq])
    for k, depth in ((16, 16), (65, 0)):
        ix.search(xq[:20], k, nprobe=3)
        assert info(gpu, ix, "filter_depth") == depth


@pytest.mark.parametrize("k", [30, 64])
@pytest.mark.parametrize("metric", [L2, IP])
def test_sq8_deep_scan_answers(gpu, metric, k):
    """40 lists of at most 31 rows: no sub-list fills, nothing is gated or flagged, every result row is rechecked."""
    rng = np.random.default_rng(23)
    d, nlist, nq = 33, 40, 20
    lens = np.concatenate([[0, 31], rng.integers(0, 32, nlist - 2)])
    n, off = int(lens.sum()), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cen, codes = rng.integers(-4, 5, (nlist, d)).astype(np.float32), rng.integers(0, 256, (n, d)).astype(np.uint8)
    vmin, vdiff = rng.integers(-130, -125, d).astype(np.float32), np.full(d, 255, np.float32)
    ids, xq = rng.permutation(n).astype(np.int64), rng.integers(-64, 65, (nq, d)).astype(np.float32)
    ix = gpu.HipIndexIVFSQ8(cen, vmin, vdiff, off, ids, codes, nprobe=nlist, metric=metric, by_residual=True)
    cd, dist = exact_ref(dict(centroids=cen), decode64(cen, vmin, vdiff, off, codes, 1), xq, metric)
    rD, rI, _ = ref_topk(cd, dist, off, ids, metric, nlist, k)
    fb0, re0 = ix.rerank_fallbacks(), info(gpu, ix, "rechecked")
    D, I = ix.search(xq, k)
    assert np.array_equal(I, rI) and np.array_equal(D, rD.astype(np.float32))
    assert ix.rerank_fallbacks() == fb0 and info(gpu, ix, "rechecked") - re0 >= nq * min(k, n)


@pytest.mark.parametrize("by_res", [0, 1])
@pytest.mark.parametrize("metric", [L2, IP])
def test_sq8_deep_trained(gpu, metric, by_res):
    """test_sq8_trained's construction and judgement; at most a tenth of the queries may take the fallback."""
    n, d, nlist, nprobe, nq = 20000, 96, 16, 4, 64
    rng = np.random.default_rng(11 + d + by_res)
    x = rng.standard_normal((n, d)).astype(np.float32)
    cen = x[rng.choice(n, nlist, replace=False)].copy()
    assign = np.argmin(dist64(cen, x, L2), axis=1)
    order = np.argsort(assign, kind="stable")
    x, assign = x[order], assign[order]
    off = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=nlist))]).astype(np.int64)
    xe = x - cen[assign] if by_res else x
    vmin = xe.min(0)
    vdiff = xe.max(0) - vmin
    codes = (np.clip((xe - vmin) / vdiff, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.int32).astype(np.uint8)
    ids = rng.permutation(n).astype(np.int64)
    ix = gpu.HipIndexIVFSQ8(cen, vmin, vdiff, off, ids, codes, nprobe=nprobe, metric=metric, by_residual=bool(by_res))
    dec = decode64(cen, vmin, vdiff, off, codes, 0)
    xh = dec + cen[assign].astype(np.float64) if by_res else dec
    sgn = -1.0 if metric == IP else 1.0
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    cd, dist = dist64(cen, xq, metric), dist64(xh, xq, metric)
    cs = np.sort(sgn * cd, axis=1)[:, :nprobe + 1]
    judged = np.flatnonzero((np.diff(cs, axis=1) > 1e-4 * np.abs(cs[:, 1:])).all(1))  # unambiguous probe lists
    assert len(judged) >= 0.9 * nq
    aD, aI, rP = ref_topk(cd, dist, off, ids, metric, nprobe, 65)
    row_of = np.argsort(ids)  # (ids are a permutation of the rows)
    for k in (30, 64):
        rD, rI, fb0 = aD[:, :k + 1], aI[:, :k + 1], ix.rerank_fallbacks()
        D, I = ix.search(xq, k)
        assert info(gpu, ix, "filter_depth") == 32 and ix.rerank_fallbacks() - fb0 <= nq // 10
        assert np.array_equal(ix.last_probes(nq)[judged], rP[judged])
        decided = 0
        for q in judged:
            rows = np.concatenate([np.arange(off[l], off[l + 1]) for l in rP[q]])
            tol = np.zeros(n)
            tol[rows] = tol_rows(xq[q].astype(np.float64), cen[assign[rows]].astype(np.float64) * by_res, dec[rows],
                                 vmin.astype(np.float64), metric, d)
            got, kth = row_of[I[q]], sgn * rD[q, k - 1]
            assert (np.abs(D[q] - dist[q, got]) <= tol[got]).all()
            assert (sgn * dist[q, got] <= kth + tol[got]).all()  # every returned row is within tol of the k-th
            assert np.isin(rows[sgn * dist[q, rows] < kth - tol[rows]], got).all()  # no better row is missing
            rt = tol[row_of[rI[q]]]
            gap = np.diff(sgn * rD[q]) > 2 * np.maximum(rt[:-1], rt[1:])  # rank r to r + 1, r < k
            ok = gap & np.concatenate([[True], gap[:-1]])  # both neighbours farther than 2·tol: the id is decided
            assert np.array_equal(I[q][ok], rI[q, :k][ok])
            decided += int(gap.sum())
        assert decided >= 0.9 * k * len(judged)  # a property of the reference alone: float64 gaps decide the ids
