"""IVF SQ8 (hipann_ivfsq_*) against numpy in float64: per query the k best rows of its probed lists by (distance, id),
the decode dec = vmin + (c + 0.5) / 255 · vdiff taken from the same fp32 vmin / vdiff, probe lists from float64 centroid
distances with ties by list id.

Exact cases: vdiff = 255·2^j makes the fp32 decode exactly vmin + (c + 0.5)·2^j; with integer vmin, centroids and
queries every partial sum is a multiple of 2⁻⁴ below 2²⁴, so fp32 and float64 agree bit for bit.  Their reference
decodes as vmin + (c + 0.5)·2^j, which float64 holds exactly (the formula's (c + 0.5) / 255 · 255 is off by float64's
last bit; build asserts the two agree to 1e-12), and the grid property is asserted on its untouched distances.
Trained cases: min/max quantizer, FAISS's encode in numpy fp32,
judged under tol_rows' forward bound of the fp32 direct form (derived there; tighter than (d + 8)·2⁻²³·Σ(|t_i| + |dec_i|)²,
under which only 80 % of the 4000 × 768 residual L2 case's float64 gaps exceed 2·tol, whatever the seed).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
LENS = (0, 1, 31, 32, 33, 2047, 2048, 2049, 4097)  # pass and chunk edges, an empty list


def build(gpu, d, metric, by_res, seed=5):
    """The exact-case index: (handle, pieces, x̂ in float64)."""
    rng = np.random.default_rng(seed + d)
    n, nlist = int(sum(LENS)), len(LENS)
    cen = rng.integers(-4, 5, (nlist, d)).astype(np.float32)
    if d <= 100:
        codes, j, vmin = rng.integers(0, 256, (n, d)), np.zeros(d), rng.integers(-130, -125, d)
    else:
        codes, j, vmin = rng.integers(0, 8, (n, d)), rng.integers(-1, 2, d), rng.integers(-4, 5, d)
    codes, vmin, vdiff = codes.astype(np.uint8), vmin.astype(np.float32), (255.0 * 2.0 ** j).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64) + np.where(rng.random(n) < 0.5, 1 << 33, 0)
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    ix = gpu.HipIndexIVFSQ8(cen, vmin, vdiff, off, ids, codes, nprobe=1, metric=metric, by_residual=bool(by_res))
    xh = vmin.astype(np.float64) + (codes + 0.5) * 2.0 ** j + (np.repeat(cen, np.diff(off), axis=0) if by_res else 0.0)
    assert np.abs(xh - decode64(cen, vmin, vdiff, off, codes, by_res)).max() < 1e-12
    return ix, dict(centroids=cen, vmin=vmin, vdiff=vdiff, list_offsets=off, ids=ids, codes=codes), xh


def decode64(cen, vmin, vdiff, off, codes, by_res):
    dec = vmin.astype(np.float64) + (codes.astype(np.float64) + 0.5) / 255.0 * vdiff.astype(np.float64)
    return dec + np.repeat(cen.astype(np.float64), np.diff(off), axis=0) if by_res else dec


def dist64(x, q, metric):
    x, q = x.astype(np.float64), q.astype(np.float64)
    ip = q @ x.T
    return ip if metric == IP else (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * ip


def ref_topk(cd, dist, off, ids, metric, nprobe, k):
    """(D, I, probes): per query the k best (distance, id) of the probed lists' rows, pads (±inf, −1)."""
    sgn = -1.0 if metric == IP else 1.0
    probes = np.stack([np.lexsort((np.arange(len(c)), sgn * c))[:min(nprobe, len(c))] for c in cd])
    D = np.full((len(cd), k), sgn * np.inf)
    I = np.full((len(cd), k), -1, np.int64)
    for q, pl in enumerate(probes):
        rows = np.concatenate([np.arange(off[l], off[l + 1]) for l in pl]).astype(np.int64)
        best = rows[np.lexsort((ids[rows], sgn * dist[q, rows]))[:k]]
        D[q, :len(best)], I[q, :len(best)] = dist[q, best], ids[best]
    return D, I, probes


def tol_rows(q, g, dec, vmin, metric, d):
    """Forward bound of the fp32 direct form against float64, u = 2⁻²⁴, any summation order, per row.  The decode's
    three roundings move dec_i by <= 3u·m_i, m_i = |vmin_i| + |dec_i − vmin_i|.  L2: t̃_i = fl(q_i − g_i) is off by
    u|t_i| and the subtraction by u|δ_i|, δ = t − dec, so each δ̃_i² is off by 2|δ_i|(u|t_i| + 3u·m_i + u|δ_i|) and the d
    additions by d·u·Σδ_i²: tol = 1.01·u·((d + 2)·Σδ_i² + 2Σ|δ_i|(|t_i| + 3m_i)).  IP: tol = 1.01·u·((d + 2)·(Σ|q_i·dec_i| +
    Σ|q_i·g_i|) + 3Σ|q_i|·m_i).  For this data both lie below (d + 8)·2⁻²³·Σ(|t_i| + |dec_i|)² (IP: products)."""
    m = np.abs(vmin) + np.abs(dec - vmin)
    if metric == IP:
        return 1.01 * 2.0 ** -24 * ((d + 2) * (np.abs(q * dec).sum(1) + np.abs(q * g).sum(1)) + 3 * (np.abs(q) * m).sum(1))
    t = q - g
    dl = np.abs(t - dec)
    return 1.01 * 2.0 ** -24 * ((d + 2) * (dl * dl).sum(1) + 2 * (dl * (np.abs(t) + 3 * m)).sum(1))


def exact_ref(p, xh, xq, metric):
    cd, dist = dist64(p["centroids"], xq, metric), dist64(xh, xq, metric)
    assert np.array_equal(dist * 16.0, np.round(dist * 16.0)) and np.abs(dist).max() < 2 ** 24  # multiples of 2⁻⁴ below 2²⁴
    return cd, dist


@pytest.mark.parametrize("d", [1, 31, 32, 33, 64, 100, 768])
@pytest.mark.parametrize("by_res", [0, 1])
@pytest.mark.parametrize("metric", [L2, IP])
def test_sq8_shapes_exact(gpu, metric, by_res, d):
    ix, p, xh = build(gpu, d, metric, by_res)
    lim = 64 if d <= 100 else 4
    xq = np.random.default_rng(7 + d).integers(-lim, lim + 1, (130, d)).astype(np.float32)
    cd, dist = exact_ref(p, xh, xq, metric)
    for nprobe in (1, 3, len(LENS), len(LENS) + 5):  # (the last is clamped)
        for k in (1, 10, 16, 64):  # 16: the scan's filter depth; 64: above it, the direct kernel
            rD, rI, rP = ref_topk(cd, dist, p["list_offsets"], p["ids"], metric, nprobe, k)
            for nq in (1, 19, 20, 130):  # at 130 with every list probed, more queries than one scan item holds
                D, I = ix.search(xq[:nq], k, nprobe=nprobe)
                assert np.array_equal(I, rI[:nq]) and np.array_equal(D, rD[:nq].astype(np.float32))
                assert np.array_equal(ix.last_probes(nq, nprobe), rP[:nq])


@pytest.mark.parametrize("metric", [L2, IP])
def test_sq8_large_k_and_pads(gpu, metric):
    ix, p, xh = build(gpu, 33, metric, 1)
    xq = np.random.default_rng(40).integers(-64, 65, (5, 33)).astype(np.float32)
    cd, dist = exact_ref(p, xh, xq, metric)
    for nprobe in (1, len(LENS)):
        for k in (65, 200, 2048):
            rD, rI, _ = ref_topk(cd, dist, p["list_offsets"], p["ids"], metric, nprobe, k)
            D, I = ix.search(xq, k, nprobe=nprobe)
            assert np.array_equal(I, rI) and np.array_equal(D, rD.astype(np.float32))
            assert nprobe > 1 or k < 2048 or (I == -1).any()  # fewer rows probed than k: pads


@pytest.mark.parametrize("n,d", [(20000, 96), (4000, 768)])
@pytest.mark.parametrize("by_res", [0, 1])
@pytest.mark.parametrize("metric", [L2, IP])
def test_sq8_trained(gpu, metric, by_res, n, d):
    rng = np.random.default_rng(11 + d + by_res)
    nlist, nprobe, k = 16, 4, 10
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
    assert codes.max() >= 128
    ids = rng.permutation(n).astype(np.int64)
    ix = gpu.HipIndexIVFSQ8(cen, vmin, vdiff, off, ids, codes, nprobe=nprobe, metric=metric, by_residual=bool(by_res))
    dec = decode64(cen, vmin, vdiff, off, codes, 0)
    xh = dec + cen[assign].astype(np.float64) if by_res else dec
    sgn = -1.0 if metric == IP else 1.0
    decided = total = 0
    for nq in (3, 64):
        xq = rng.standard_normal((nq, d)).astype(np.float32)
        cd, dist = dist64(cen, xq, metric), dist64(xh, xq, metric)
        cs = np.sort(sgn * cd, axis=1)[:, :nprobe + 1]
        judged = np.flatnonzero((np.diff(cs, axis=1) > 1e-4 * np.abs(cs[:, 1:])).all(1))  # unambiguous probe lists
        assert len(judged) >= 0.9 * nq
        rD, rI, rP = ref_topk(cd, dist, off, ids, metric, nprobe, k + 1)
        D, I = ix.search(xq, k)
        assert np.array_equal(ix.last_probes(nq)[judged], rP[judged])
        row_of = np.empty(n, np.int64)
        row_of[ids] = np.arange(n)
        for q in judged:
            rows = np.concatenate([np.arange(off[l], off[l + 1]) for l in rP[q]])
            tol = np.zeros(n)
            tol[rows] = tol_rows(xq[q].astype(np.float64), cen[assign[rows]].astype(np.float64) * by_res, dec[rows],
                                 vmin.astype(np.float64), metric, d)
            got = row_of[I[q]]
            kth = sgn * rD[q, k - 1]
            assert (np.abs(D[q] - dist[q, got]) <= tol[got]).all()
            assert (sgn * dist[q, got] <= kth + tol[got]).all()  # every returned row is within tol of the k-th
            must = rows[sgn * dist[q, rows] < kth - tol[rows]]
            assert np.isin(must, got).all()  # every row that beats the k-th by more than tol is present
            rt = tol[row_of[rI[q]]]
            gap = np.diff(sgn * rD[q]) > 2 * np.maximum(rt[:-1], rt[1:])  # rank r to r + 1, r < k
            ok = gap & np.concatenate([[True], gap[:-1]])  # both neighbours farther than 2·tol: the id is decided
            assert np.array_equal(I[q][ok], rI[q, :k][ok])
            decided, total = decided + int(gap.sum()), total + k
    assert decided >= 0.9 * total  # a property of the reference alone: float64 gaps decide the ids
    assert ix.rerank_fallbacks() >= 0


@pytest.mark.parametrize("metric", [L2, IP])
def test_sq8_empty_index(gpu, metric):
    cen = np.arange(12, dtype=np.float32).reshape(3, 4)
    ix = gpu.HipIndexIVFSQ8(cen, np.zeros(4, np.float32), np.full(4, 255, np.float32), np.zeros(4, np.int64),
                            np.zeros(0, np.int64), np.zeros((0, 4), np.uint8), nprobe=2, metric=metric)
    for k in (3, 70):
        D, I = ix.search(np.ones((2, 4), np.float32), k)
        assert (I == -1).all() and (D == (-np.inf if metric == IP else np.inf)).all()
    assert ix.ntotal == 0


def test_sq8_round_trip_and_refusals(gpu):
    ix, p, _ = build(gpu, 33, L2, 1)
    ex = ix.export()
    for name, val in p.items():
        assert ex[name].dtype == val.dtype and np.array_equal(ex[name], val), name
    xq = np.random.default_rng(3).integers(-64, 65, (20, 33)).astype(np.float32)
    ix2 = gpu.GpuBackend().cpu_to_gpu(dict(p, type="IVFSQ8", nprobe=3))
    for a, b in zip(ix2.search(xq, 10), ix.search(xq, 10, nprobe=3)):
        assert np.array_equal(a, b)
    assert gpu.GpuBackend().gpu_to_cpu(ix2)["type"] == "IVFSQ8"
    eb, D, I = C.create_string_buffer(256), np.empty(1, np.float32), np.empty(1, np.int64)
    assert gpu.lib().hipann_flat_search(ix.handle, 1, xq.ctypes.data_as(C.POINTER(C.c_float)), 1,
                                        D.ctypes.data_as(C.POINTER(C.c_float)), I.ctypes.data_as(C.POINTER(C.c_int64)),
                                        eb, 256) == -1
    bad_vdiff = p["vdiff"].copy()
    bad_vdiff[0] = np.nan
    bad_off = p["list_offsets"].copy()
    bad_off[3] = bad_off[2] - 1
    with pytest.raises(gpu.HipAnnError, match="finite"):
        gpu.HipIndexIVFSQ8(**dict(p, vdiff=bad_vdiff))
    with pytest.raises(gpu.HipAnnError, match="ascending"):
        gpu.HipIndexIVFSQ8(**dict(p, list_offsets=bad_off))
    with pytest.raises(gpu.HipAnnError, match="k must be"):
        ix.search(xq, 0)
