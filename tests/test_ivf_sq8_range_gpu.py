"""IVF SQ8 range search (hipann_ivfsq_range_search*) against numpy in float64: per query the rows of its probed lists
whose decoded distance passes the strict comparison (L2: < radius, IP: > radius), in probe order, then list order.  The
decode is vmin + (c + 0.5) / 255 · vdiff from the same fp32 vmin / vdiff, probe lists come from float64 centroid distances
with ties by list id.

Exact cases use test_ivf_sq8_gpu's grid (vdiff = 255·2^j, integer vmin / centroids / queries): every distance is a
multiple of 2⁻⁴ below 2²⁴, asserted on the reference, so lims, ids, distances and probe lists must equal it array for
array, rows sitting exactly on the radius included.  Trained cases are judged under tol_rows, the forward bound of the
fp32 direct form derived in test_ivf_sq8_gpu.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from test_ivf_range_gpu import check_exact, ref_range
from test_ivf_sq8_gpu import LENS, build, decode64, dist64, exact_ref, tol_rows

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
LENS5 = (40, 2100, 0, 70, 2500)


def grid_index(gpu, d, metric, by_res, lens, seed, nprobe=1):
    """An exact-grid index with chosen list lengths: (handle, centroids)."""
    rng = np.random.default_rng(seed)
    n, nlist = int(sum(lens)), len(lens)
    cen = rng.integers(-4, 5, (nlist, d)).astype(np.float32)
    hi, j, vmin = (256, np.zeros(d), rng.integers(-130, -125, d)) if d <= 100 else (8, rng.integers(-1, 2, d), rng.integers(-4, 5, d))
    codes = rng.integers(0, hi, (n, d), dtype=np.uint8)
    ids = rng.permutation(n).astype(np.int64) + np.where(rng.random(n) < 0.5, 1 << 33, 0)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return gpu.HipIndexIVFSQ8(cen, vmin.astype(np.float32), (255.0 * 2.0 ** j).astype(np.float32), off, ids, codes,
                              nprobe=nprobe, metric=metric, by_residual=bool(by_res)), cen


def export_ref(ix, xq, metric, by_res):
    """(pieces, (centroid, row) float64 distances) of the index as it is now, decoded exactly on the grid."""
    p = ix.export()
    xh = p["vmin"].astype(np.float64) + (p["codes"] + 0.5) * (p["vdiff"].astype(np.float64) / 255.0)
    if by_res:
        xh = xh + np.repeat(p["centroids"].astype(np.float64), np.diff(p["list_offsets"]), axis=0)
    return p, exact_ref(p, xh, xq, metric)


def check_export(ix, xq, radius, metric, by_res, nprobe):
    p, pre = export_ref(ix, xq, metric, by_res)
    ref = ref_range(p["centroids"], p["list_offsets"], p["ids"], None, xq, radius, metric, nprobe, pre)
    check_exact(ix.range_search(xq, radius, nprobe=nprobe), ref)
    return ref


def attained(dist):
    return float(np.sort(dist[0])[dist.shape[1] // 3])


@pytest.mark.parametrize("d", [1, 31, 32, 33, 64, 100, 768])
@pytest.mark.parametrize("by_res", [0, 1])
@pytest.mark.parametrize("metric", [L2, IP])
def test_sq8_range_shapes_exact(gpu, metric, by_res, d):
    ix, p, xh = build(gpu, d, metric, by_res)
    lim = 64 if d <= 100 else 4
    xq = np.random.default_rng(7 + d).integers(-lim, lim + 1, (130, d)).astype(np.float32)
    cd, dist = exact_ref(p, xh, xq, metric)
    radius = attained(dist)  # an attained distance of query 0: those rows stay out
    for nprobe in (1, 3, len(LENS), len(LENS) + 5):  # (the last is clamped)
        for nq in (1, 19, 20, 130):  # at 130 with every list probed, more queries than one item holds
            ref = ref_range(p["centroids"], p["list_offsets"], p["ids"], None, xq[:nq], radius, metric, nprobe,
                            (cd[:nq], dist[:nq]))
            check_exact(ix.range_search(xq[:nq], radius, nprobe=nprobe), ref)
            assert np.array_equal(ix.last_probes(nq, nprobe), ref[3])


@pytest.mark.parametrize("metric", [L2, IP])
def test_sq8_range_radius_edges(gpu, metric):
    d, nprobe = 32, 4
    ix, p, xh = build(gpu, d, metric, 1)
    xq = np.random.default_rng(2).integers(-64, 65, (40, d)).astype(np.float32)
    pre = exact_ref(p, xh, xq, metric)
    dist, off = pre[1], p["list_offsets"]
    everything, nothing = (dist.min() - 1, dist.max() + 1) if metric == IP else (dist.max() + 1, dist.min() - 1)
    for radius in (attained(dist), float(nothing), float(everything), np.inf, -np.inf):
        check_exact(ix.range_search(xq, radius, nprobe=nprobe),
                    ref_range(p["centroids"], off, p["ids"], None, xq, radius, metric, nprobe, pre))
    lims, _, _ = ix.range_search(xq, float(everything), nprobe=nprobe)
    probed = np.diff(off)[ix.last_probes(len(xq), nprobe)].sum(1)
    assert np.array_equal(np.diff(lims), probed) and probed.max() > 2048  # beyond HIPANN_MAX_K
    radius = attained(dist)
    a, b = ix.range_search(xq, radius, nprobe=nprobe), ix.range_search(xq, radius, nprobe=nprobe)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n,d", [(20000, 96), (4000, 768)])
@pytest.mark.parametrize("by_res", [0, 1])
@pytest.mark.parametrize("metric", [L2, IP])
def test_sq8_range_trained(gpu, metric, by_res, n, d):
    rng = np.random.default_rng(11 + d + by_res)  # the index of test_sq8_trained
    nlist, nprobe = 16, 4
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
    row_of = np.empty(n, np.int64)
    row_of[ids] = np.arange(n)
    xq = rng.standard_normal((64, d)).astype(np.float32)
    cd, dist = dist64(cen, xq, metric), dist64(xh, xq, metric)
    probes = ref_range(cen, off, ids, None, xq, 0.0, metric, nprobe, (cd, dist))[3]
    prow = [np.concatenate([np.arange(off[l], off[l + 1]) for l in pl]) for pl in probes]
    radius = float(np.float32(np.median([sgn * np.sort(sgn * dist[q, r])[49] for q, r in enumerate(prow)])))
    cs = np.sort(sgn * cd, axis=1)[:, :nprobe + 1]
    clear = (np.diff(cs, axis=1) > 1e-4 * np.abs(cs[:, 1:])).all(1)  # unambiguous probe lists
    near = must_n = 0
    for nq in (3, 64):
        judged = np.flatnonzero(clear[:nq])
        assert len(judged) >= 0.9 * nq
        lims, D, I = ix.range_search(xq[:nq], radius)
        assert np.array_equal(ix.last_probes(nq)[judged], probes[:nq][judged])
        Ds, Is = ix.search(xq[:nq], 32)
        for q in range(nq):
            gD, gI = D[lims[q]:lims[q + 1]], I[lims[q]:lims[q + 1]]
            both, at, bt = np.intersect1d(gI, Is[q], return_indices=True)
            assert np.array_equal(gD[at].view(np.uint32), Ds[q][bt].view(np.uint32))  # the top-k paths' bits
        for q in judged:
            rows, got = prow[q], row_of[I[lims[q]:lims[q + 1]]]
            tol = tol_rows(xq[q].astype(np.float64), cen[assign[rows]].astype(np.float64) * by_res, dec[rows],
                           vmin.astype(np.float64), metric, d)
            sd, sr = sgn * dist[q, rows], sgn * radius
            pos = np.full(n, -1)
            pos[rows] = np.arange(len(rows))
            assert (pos[got] >= 0).all() and (np.diff(pos[got]) > 0).all()  # (probe rank, list position) ascending
            assert np.isin(rows[sd < sr - tol], got).all()  # inside by more than tol: returned
            assert not np.isin(rows[sd > sr + tol], got).any()  # outside by more than tol: not returned
            assert (np.abs(D[lims[q]:lims[q + 1]] - dist[q, got]) <= tol[pos[got]]).all()
            near, must_n = near + int((np.abs(sd - sr) <= tol).sum()), must_n + int((sd < sr - tol).sum())
    assert near <= 0.05 * must_n  # a property of the reference alone: float64 decides nearly every membership


@pytest.mark.parametrize("metric", [L2, IP])
def test_sq8_range_after_add_and_remove(gpu, metric):
    d, nprobe = 33, 3
    ix, cen = grid_index(gpu, d, metric, 1, LENS5, 21)
    rng = np.random.default_rng(22)
    xq = rng.integers(-64, 65, (40, d)).astype(np.float32)
    radius = attained(export_ref(ix, xq, metric, 1)[1][1])
    check_export(ix, xq, radius, metric, 1, nprobe)
    add = cen[rng.integers(0, len(LENS5), 300)] + rng.integers(-128, 128, (300, d)).astype(np.float32)
    ix.add(add, (1 << 40) + np.arange(300, dtype=np.int64))
    check_export(ix, xq, radius, metric, 1, nprobe)
    p = ix.export()
    off = p["list_offsets"]
    gone = np.concatenate([p["ids"][off[l]:off[l + 1]][[0, -1, 2060]] for l in (1, 4)])  # first, last, mid-chunk rows
    assert ix.remove_ids(gone) == len(gone)
    ref = check_export(ix, xq, radius, metric, 1, nprobe)
    assert not np.isin(gone, ref[2]).any() and ref[0][-1] > 0


def test_sq8_range_direct_kernel(gpu):
    """d above 4352: the query terms do not fit the LDS, every slot takes ivf_sq_range_direct."""
    for metric in (L2, IP):
        ix, _ = grid_index(gpu, 4400, metric, 1, (33, 0, 2081), 31 + metric)
        xq = np.random.default_rng(32).integers(-4, 5, (3, 4400)).astype(np.float32)
        radius = attained(export_ref(ix, xq, metric, 1)[1][1])
        assert check_export(ix, xq, radius, metric, 1, 3)[0][-1] > 0


@pytest.mark.parametrize("budget", [0, 7 * 5 * 256])  # the default, and query slices of 7 (5 slots a query at most)
def test_sq8_range_device_variant_cap(gpu, budget):
    import torch

    d, nprobe, nq = 32, 3, 40
    ix, _ = grid_index(gpu, d, L2, 1, LENS5, 8, nprobe=nprobe)
    f = gpu.lib().hipann_debug_ivfsq_info
    f.argtypes, f.restype = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)], C.c_int
    assert f(ix.handle, b"range_mask_budget", C.byref(C.c_double(budget))) == 0
    xq = np.random.default_rng(9).integers(-64, 65, (nq, d)).astype(np.float32)
    p, pre = export_ref(ix, xq, L2, 1)
    radius = attained(pre[1])
    rl, rD, rI, _ = ref_range(p["centroids"], p["list_offsets"], p["ids"], None, xq, radius, L2, nprobe, pre)
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
    check_exact(ix.range_search(xq, radius), (rl, rD, rI))  # the host variant under the same slicing
    assert np.array_equal(ix.last_probes(nq), ref_range(p["centroids"], p["list_offsets"], p["ids"], None, xq, radius, L2,
                                                        nprobe, pre)[3])


def test_sq8_range_arguments(gpu):
    ix, cen = grid_index(gpu, 8, L2, 1, (5, 0, 45), 12)
    lims, D, I = ix.range_search(np.zeros((0, 8), np.float32), 1.0)
    assert lims.tolist() == [0] and D.size == 0 and I.size == 0
    empty = gpu.HipIndexIVFSQ8(cen, np.zeros(8, np.float32), np.full(8, 255, np.float32), np.zeros(4, np.int64),
                               np.zeros(0, np.int64), np.zeros((0, 8), np.uint8))
    assert empty.range_search(cen, 1.0)[0].tolist() == [0, 0, 0, 0]
    with pytest.raises(gpu.HipAnnError):
        ix.range_search(cen, float("nan"))
    nanq = cen.copy()
    nanq[1, 3] = np.nan
    lims, _, _ = ix.range_search(nanq, np.inf, nprobe=3)
    assert lims[2] == lims[1] and lims[1] == 50 and lims[3] == 100  # a query holding a NaN returns no rows
    flat = gpu.HipIndexIVFFlat(cen, np.array([0, 1, 2, 3], np.int64), np.arange(3, dtype=np.int64), cen)
    L = gpu.lib()
    eb, out = C.create_string_buffer(256), np.zeros(4, np.int64)
    dp, ip = C.POINTER(C.c_float)(), C.POINTER(C.c_int64)()
    args = (0, 3, cen.ctypes.data_as(C.POINTER(C.c_float)), 1.0, out.ctypes.data_as(C.POINTER(C.c_int64)),
            C.byref(dp), C.byref(ip), eb, 256)
    assert L.hipann_ivf_range_search(ix.handle, *args) == -1
    assert L.hipann_ivfsq_range_search(flat.handle, *args) == -1
