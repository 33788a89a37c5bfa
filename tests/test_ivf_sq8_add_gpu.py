"""IVF SQ8 train and add on the device (hipann_ivfsq_train / hipann_ivfsq_add) against numpy: the assignment and the
distances in float64, FAISS's encode in fp32.

Grid data: vdiff = 255·2^j and rows x = g + vmin + (c + 0.5)·2^j with integer g and vmin, so the fp32 encode returns c,
every coarse and row distance is a multiple of 2⁻⁴ below 2²⁴ (asserted on the reference) and fp32 equals float64 bit
for bit.  All centroids share their entries except dimension 0, where they are 40 apart (300 for d = 1): the L2
assignment is decided there, far from any tie; for IP only the two extreme lists take rows.  Rows of the created part
have codes < 8, added rows up to 255 (for d = 768 in dimensions 1 and 2 only, which keeps the sums below 2²⁴)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
LENS = (0, 1, 31, 32, 33, 2047, 2048, 2049, 4097)  # the created lists of the existing exact test
NL = len(LENS)


def quantizer(d, rng):
    cen = np.tile(rng.integers(-4, 5, d), (NL, 1)).astype(np.float32)
    cen[:, 0] = (300 if d == 1 else 40) * (np.arange(NL) - 4)
    if d <= 100:
        j, vmin, big = np.zeros(d), rng.integers(-130, -125, d), np.arange(d > 1, d)
    else:
        j, vmin, big = rng.integers(-1, 2, d), rng.integers(-4, 5, d), np.arange(1, 3)
        j[:3] = 0
    if d > 1:
        vmin[0] = rng.integers(-4, 5)
    return cen, vmin.astype(np.float32), (255.0 * 2.0 ** j).astype(np.float32), big


def grid_rows(rng, own, cen, vmin, vdiff, big, top):
    c = rng.integers(0, 8, (len(own), cen.shape[1]))
    c[:, big] = rng.integers(0, top, (len(own), len(big)))
    x = cen[own].astype(np.float64) + vmin + (c + 0.5) * (vdiff.astype(np.float64) / 255.0)
    assert np.array_equal(x.astype(np.float32), x)
    return x.astype(np.float32)


def assign64(x, cen, metric):
    x, g = x.astype(np.float64), cen.astype(np.float64)
    ip = x @ g.T
    return np.argmax(ip, 1) if metric == IP else np.argmin((g * g).sum(1)[None, :] - 2.0 * ip, 1)  # ties: lowest list


def encode32(x, g, vmin, vdiff):
    e = x - g if g is not None else x
    ok = vdiff != 0
    xi = np.where(ok, (e - vmin) / np.where(ok, vdiff, np.float32(1)), np.float32(0)).astype(np.float32)
    return (np.float32(255) * np.clip(xi, np.float32(0), np.float32(1))).astype(np.int32).astype(np.uint8)


class RefLists:
    """The index in numpy: per list the labels and codes in insertion order."""

    def __init__(self, cen, vmin, vdiff, metric, by_res):
        self.cen, self.vmin, self.vdiff, self.metric, self.by_res = cen, vmin, vdiff, metric, by_res
        self.ids = [np.zeros(0, np.int64) for _ in range(NL)]
        self.codes = [np.zeros((0, cen.shape[1]), np.uint8) for _ in range(NL)]

    def add(self, x, ids):
        a = assign64(x, self.cen, self.metric)
        c = encode32(x, self.cen[a] if self.by_res else None, self.vmin, self.vdiff)
        for l in np.unique(a):
            self.ids[l] = np.concatenate([self.ids[l], ids[a == l]])
            self.codes[l] = np.concatenate([self.codes[l], c[a == l]])

    def csr(self):
        off = np.concatenate([[0], np.cumsum([len(i) for i in self.ids])]).astype(np.int64)
        return off, np.concatenate(self.ids), np.concatenate(self.codes)

    def check(self, ix, xq, ks=(1, 16, 64, 200), nqs=(1, 20, 130)):
        off, ids, codes = self.csr()
        ex = ix.export()
        assert np.array_equal(ex["list_offsets"], off) and np.array_equal(ex["ids"], ids)
        assert np.array_equal(ex["codes"], codes) and ix.ntotal == len(ids)
        xh = self.vmin.astype(np.float64) + (codes + 0.5) * (self.vdiff.astype(np.float64) / 255.0)
        if self.by_res:
            xh = xh + np.repeat(self.cen.astype(np.float64), np.diff(off), axis=0)
        sgn = -1.0 if self.metric == IP else 1.0
        q = xq.astype(np.float64)
        cd, dist = q @ self.cen.astype(np.float64).T, q @ xh.T
        if self.metric == L2:
            cd = (q * q).sum(1)[:, None] + (self.cen.astype(np.float64) ** 2).sum(1)[None, :] - 2.0 * cd
            dist = (q * q).sum(1)[:, None] + (xh * xh).sum(1)[None, :] - 2.0 * dist
        for m in (cd, dist):
            assert np.array_equal(m * 16.0, np.round(m * 16.0)) and np.abs(m).max() < 2 ** 24
        for nprobe in (1, NL):
            D = np.full((len(xq), max(ks)), sgn * np.inf)
            I = np.full((len(xq), max(ks)), -1, np.int64)
            for qi, c in enumerate(cd):
                pl = np.lexsort((np.arange(NL), sgn * c))[:nprobe]
                rows = np.concatenate([np.arange(off[l], off[l + 1]) for l in pl]).astype(np.int64)
                best = rows[np.lexsort((ids[rows], sgn * dist[qi, rows]))[:max(ks)]]
                D[qi, :len(best)], I[qi, :len(best)] = dist[qi, best], ids[best]
            for k in ks:
                for nq in nqs:
                    gD, gI = ix.search(xq[:nq], k, nprobe=nprobe)
                    assert np.array_equal(gI, I[:nq, :k]) and np.array_equal(gD, D[:nq, :k].astype(np.float32))
        return codes


def info(gpu, ix, name):
    f, out = gpu.lib().hipann_debug_ivfsq_info, C.c_double()
    f.argtypes, f.restype = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)], C.c_int
    assert f(ix.handle, name.encode(), C.byref(out)) == 0
    return out.value


def grown_cap(cap, need):
    return -(-max(cap, need + max(need // 4, 64)) // 32) * 32


@pytest.mark.parametrize("d", [1, 33, 100, 768])
@pytest.mark.parametrize("by_res", [0, 1])
@pytest.mark.parametrize("metric", [L2, IP])
def test_add_exact(gpu, metric, by_res, d):
    rng = np.random.default_rng(17 + d)
    cen, vmin, vdiff, big = quantizer(d, rng)
    ref = RefLists(cen, vmin, vdiff, metric, by_res)
    x0 = grid_rows(rng, np.repeat(np.arange(NL), LENS), cen, vmin, vdiff, big, 8)
    x0 = x0[assign64(x0, cen, metric) != 0]  # list 0 starts empty (IP sends the low lists' rows there)
    ref.add(x0, rng.permutation(len(x0)).astype(np.int64) + (1 << 33))
    off, ids, codes = ref.csr()
    ix = gpu.HipIndexIVFSQ8(cen, vmin, vdiff, off, ids, codes, nprobe=1, metric=metric, by_residual=bool(by_res))
    # the pool of rows to add, by the list they go to: E = 0 (empty) and F = 8 (the longest) take rows under both metrics
    pool = grid_rows(rng, np.repeat([0, NL - 1], [100, 7900]), cen, vmin, vdiff, big, 256)
    pa, used, E, F = assign64(pool, cen, metric), np.zeros(len(pool), bool), 0, NL - 1

    def take(l, m):
        rows = np.flatnonzero((pa == l) & ~used)[:m]
        assert len(rows) == m
        used[rows] = True
        return rows

    xq = rng.integers(-4, 5, (130, d)).astype(np.float32) * (16 if d <= 100 else 1)
    lenF = len(ref.ids[F])
    capF = grown_cap(lenF, lenF)  # after the first step's regroup (no row of it goes to F)
    capF2 = grown_cap(capF, capF + 1)
    steps = [take(E, 3),                                   # into the empty list: the dense lists regroup
             take(F, 1),                                   # one row
             take(F, capF - lenF - 1),                     # fills F's slack exactly: no regroup
             take(F, 1),                                   # one row more: regroup
             np.concatenate([take(F, capF2 - capF - 41), take(E, 5)])]  # most of the new slack, both lists
    assert (capF + 1) // 2048 != (capF2 - 40) // 2048  # the last step takes F across a 2048-row chunk edge
    mem = ix.memory_bytes
    for s, rows in enumerate(steps):
        lab = None if s == 1 else rng.permutation(len(rows)).astype(np.int64) + 1000000 * (s + 1)
        n0 = ix.ntotal
        ix.add(pool[rows], lab)
        ref.add(pool[rows], np.arange(n0, n0 + len(rows), dtype=np.int64) if lab is None else lab)
        codes = ref.check(ix, xq)  # every (k, nq, nprobe) after every step
        assert (ix.memory_bytes > mem) == (s in (0, 3)), s  # the regroups, and only they, change the footprint
        mem = ix.memory_bytes
    cn = np.sqrt((codes.astype(np.float64) ** 2).sum(1).max())
    assert cn > 200 and cn <= info(gpu, ix, "cmax") <= 1.001 * cn


def test_add_from_empty_and_blocks(gpu):
    d, rng = 8, np.random.default_rng(5)
    cen, vmin, vdiff, big = quantizer(d, rng)
    ref = RefLists(cen, vmin, vdiff, L2, 1)
    ix = gpu.HipIndexIVFSQ8(cen, vmin, vdiff, np.zeros(NL + 1, np.int64), np.zeros(0, np.int64),
                            np.zeros((0, d), np.uint8), nprobe=2, metric=L2)
    x = grid_rows(rng, rng.integers(0, NL, 70000), cen, vmin, vdiff, big, 256)  # two assignment blocks
    ix.add(x)
    ref.add(x, np.arange(70000, dtype=np.int64))
    xq = rng.integers(-64, 65, (20, d)).astype(np.float32)
    ref.check(ix, xq, (10,), (20,))
    ex = ix.export()
    ix2 = gpu.HipIndexIVFSQ8(ex["centroids"], ex["vmin"], ex["vdiff"], ex["list_offsets"], ex["ids"], ex["codes"],
                             nprobe=2, metric=L2)
    for k in (10, 100):
        for a, b in zip(ix.search(xq, k, nprobe=3), ix2.search(xq, k, nprobe=3)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("metric", [L2, IP])
def test_device_entry_points(gpu, metric):
    """hipann_ivfsq_train_device / _add_device: rows, centroids and labels in HBM, on the caller's stream."""
    import torch

    d, rng = 33, np.random.default_rng(9)
    cen, vmin, vdiff, big = quantizer(d, rng)
    x = grid_rows(rng, rng.integers(0, NL, 3000), cen, vmin, vdiff, big, 256)
    lab = rng.permutation(3000).astype(np.int64) + (1 << 40)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        xt, ct, lt = torch.from_numpy(x).cuda(), torch.from_numpy(cen).cuda(), torch.from_numpy(lab).cuda()
        out = torch.empty((2, d), device="cuda")
        gpu.ivfsq_train_device(d, NL, 3000, xt.data_ptr(), ct.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), metric,
                               True, stream=st.cuda_stream)
        e = x - cen[assign64(x, cen, metric)]
        assert np.array_equal(out.cpu().numpy(), np.stack([e.min(0), e.max(0) - e.min(0)]))
        ref = RefLists(cen, vmin, vdiff, metric, 1)
        ix = gpu.HipIndexIVFSQ8(cen, vmin, vdiff, np.zeros(NL + 1, np.int64), np.zeros(0, np.int64),
                                np.zeros((0, d), np.uint8), metric=metric)
        for r0, ids_ptr in ((0, lt.data_ptr()), (2000, 0)):  # device labels, then ntotal + i
            ix.add_device(1000 if r0 else 2000, xt[r0:].data_ptr(), ids_ptr, st.cuda_stream)
        ref.add(x[:2000], lab[:2000])
        ref.add(x[2000:], np.arange(2000, 3000, dtype=np.int64))
        ref.check(ix, rng.integers(-64, 65, (20, d)).astype(np.float32), (10, 100), (20,))


@pytest.mark.parametrize("d", [1, 33, 768])
@pytest.mark.parametrize("by_res", [0, 1])
def test_train(gpu, by_res, d):
    rng = np.random.default_rng(23 + d)
    if by_res:
        cen, vmin, vdiff, big = quantizer(d, rng)
        x = grid_rows(rng, rng.integers(0, NL, 5000), cen, vmin, vdiff, big, 256)
        e = x - cen[assign64(x, cen, L2)]
    else:
        cen = rng.standard_normal((NL, d)).astype(np.float32)
        e = x = rng.standard_normal((5000, d)).astype(np.float32)
    gmin, gdiff = gpu.ivfsq_train(x, cen, L2, bool(by_res))
    assert np.array_equal(gmin, e.min(0)) and np.array_equal(gdiff, e.max(0) - e.min(0))


@pytest.mark.parametrize("n,d", [(20000, 96), (4000, 768)])
@pytest.mark.parametrize("metric", [L2, IP])
def test_add_trained_encode(gpu, metric, n, d):
    rng = np.random.default_rng(11 + d)
    nlist = 16
    x = rng.standard_normal((n, d)).astype(np.float32)
    cen = x[rng.choice(n, nlist, replace=False)].copy()
    vmin, vdiff = gpu.ivfsq_train(x, cen, metric, True)
    ix = gpu.HipIndexIVFSQ8(cen, vmin, vdiff, np.zeros(nlist + 1, np.int64), np.zeros(0, np.int64),
                            np.zeros((0, d), np.uint8), metric=metric)
    perm = rng.permutation(n).astype(np.int64)
    ix.add(x, perm)
    ex = ix.export()
    row = np.argsort(perm)[ex["ids"]]  # the row each exported entry came from
    lst = np.repeat(np.arange(nlist), np.diff(ex["list_offsets"]))
    assert len(row) == n and all((np.diff(row[lst == l]) > 0).all() for l in range(nlist))  # insertion order
    assert np.array_equal(ex["codes"], encode32(x[row], cen[lst], vmin, vdiff)) and ex["codes"].max() == 255
    sgn = -1.0 if metric == IP else 1.0
    q, g = x[row].astype(np.float64), cen.astype(np.float64)
    cd = sgn * (q @ g.T if metric == IP else (g * g).sum(1)[None, :] - 2.0 * (q @ g.T) + (q * q).sum(1)[:, None])
    two = np.sort(cd, 1)[:, :2]
    clear = two[:, 1] - two[:, 0] > 1e-4 * np.abs(two[:, 1])
    assert clear.mean() >= 0.99  # a property of the reference alone
    assert np.array_equal(lst[clear], np.argmin(cd, 1)[clear])


def test_add_refusals(gpu):
    rng = np.random.default_rng(3)
    cen, vmin, vdiff, big = quantizer(33, rng)
    ref = RefLists(cen, vmin, vdiff, L2, 1)
    x = grid_rows(rng, rng.integers(0, NL, 500), cen, vmin, vdiff, big, 256)
    ref.add(x[:300], np.arange(300, dtype=np.int64))
    off, ids, codes = ref.csr()
    ix = gpu.HipIndexIVFSQ8(cen, vmin, vdiff, off, ids, codes, metric=L2)
    xq = rng.integers(-64, 65, (20, 33)).astype(np.float32)
    bad = x[300:].copy()
    bad[150, 7] = np.nan
    with pytest.raises(gpu.HipAnnError, match="finite"):
        ix.add(bad)
    ref.check(ix, xq, (10,), (20,))  # unchanged
    ix.add(x[300:300])  # n = 0
    assert ix.ntotal == 300
    with pytest.raises(gpu.HipAnnError):
        gpu.ivfsq_train(x[:0], cen)
    with pytest.raises(ValueError):
        ix.add(np.zeros((2, 32), np.float32))
