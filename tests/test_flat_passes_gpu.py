"""The Flat bounded passes' kernels (flat_b16k64.hip) against the exact numpy model of _flat_pass_cases.py.

flat_shard_launch takes this path only for tables of 512K rows and more, and what it computes then passes through
the exact rerank and the fallback, which repair a filter that drops or invents a row.  These tests run the pieces
themselves through the library's test hooks — the image builders, one launch of flat_bf16_k64 in its keys and
filter modes, flat_cand_bound / flat_cand_select in both variants — on inputs whose every intermediate is exact in
fp32, and compare bit for bit: image bytes with the documented layout, dense keys, per-cell counts and admitted
(key, row) sets, untouched slots and guard regions, bounds, selected lists and flags.

Decision recorded here (T = +inf): the padding rows of a last tile carry s = -inf and pass a bound of +inf
(cth = -inf); the append path now skips rows >= N, so they are neither counted nor stored, and the filter test
asserts exact counts and no id >= N for such queries too.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import _flat_pass_cases as M

pytestmark = pytest.mark.gpu

GUARD = 1024  # sentinel words before and after every output buffer
SENT = 0x7FC0BEEF  # a NaN as float, a large positive id as int: never a legitimate output here
R = M.TILE


# ---- plumbing ---------------------------------------------------------------------------------------------------
class Guarded:
    """A device buffer of n 32-bit words between two sentinel-filled guard regions."""

    def __init__(self, n: int, init: np.ndarray | None = None):
        import torch

        host = np.full(n + 2 * GUARD, SENT, dtype=np.uint32)
        if init is not None:
            host[GUARD : GUARD + n] = np.ascontiguousarray(init).view(np.uint32).ravel()
        self.n = n
        self.t = torch.from_numpy(host.view(np.int32)).cuda()

    @property
    def ptr(self) -> int:
        return self.t.data_ptr() + 4 * GUARD

    def read(self) -> np.ndarray:
        a = self.t.cpu().numpy().view(np.uint32)
        assert np.all(a[:GUARD] == SENT) and np.all(a[GUARD + self.n :] == SENT), "guard region overwritten"
        return a[GUARD : GUARD + self.n].copy()


def _dev(a: np.ndarray):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Hooks:
    def __init__(self, lib):
        p, i, l = C.c_void_p, C.c_int, C.c_int64
        self.img8 = lib.hipann_debug_flat_i8_img_bytes
        self.img16 = lib.hipann_debug_flat_bf16_img_bytes
        for f in (self.img8, self.img16):
            f.restype, f.argtypes = l, [l, i, i]
        self.nk8 = lib.hipann_debug_flat_i8_nk
        self.nk8.restype, self.nk8.argtypes = i, [i]
        self.prep = lib.hipann_debug_flat_image_prep
        self.prep.restype, self.prep.argtypes = i, [p, l, i, i, i, p, p, p, p, p]
        self.scan = lib.hipann_debug_flat_pass
        self.scan.restype, self.scan.argtypes = i, [p, l, p, l, i, i, i, i, i, l, l, l, p, p, p, p, i, i]
        self.bound = lib.hipann_debug_flat_cand_bound
        self.bound.restype, self.bound.argtypes = i, [p, p, i, i, l, i, p, i]
        self.select = lib.hipann_debug_flat_cand_select
        self.select.restype, self.select.argtypes = i, [p, p, p, i, i, l, i, p, p, p, p, i]
        self.kth = lib.hipann_debug_flat_keys_kth
        self.kth.restype, self.kth.argtypes = i, [p, i, l, i, p, i]


@pytest.fixture(scope="module")
def hk(gpu):
    return Hooks(gpu.lib())


def run_keys(hk, Q, X, metric, i8, nsplit, tps, rc=0):
    nq, N = len(Q), len(X)
    out = Guarded(nq * N)
    dq, dx = _dev(Q), _dev(X)
    got = hk.scan(dq.data_ptr(), nq, dx.data_ptr(), N, Q.shape[1], metric, int(i8), 1, nsplit, tps, 0, tps, None,
                  out.ptr, None, None, 0, 0)
    assert got == rc
    return out.read().view(np.float32).reshape(nq, N)


class Cells:
    """Candidate buffers of nq x nsplit cells of cap slots on the device, sentinel-filled."""

    def __init__(self, nq, nsplit, cap, cd=None, ci=None, cn=None):
        self.nq, self.nsplit, self.cap = nq, nsplit, cap
        self.d = Guarded(nq * nsplit * cap, cd)
        self.i = Guarded(nq * nsplit * cap, ci)
        self.n = Guarded(nq * nsplit, cn)

    def read(self):
        s = (self.nq, self.nsplit, self.cap)
        return (self.d.read().view(np.float32).reshape(s), self.i.read().view(np.int32).reshape(s),
                self.n.read().view(np.int32).reshape(s[:2]))


def run_pass(hk, cells: Cells, dq, dx, nq, N, d, metric, i8, tps, tb, te, T, resume):
    dT = _dev(np.asarray(T, dtype=np.float32))
    assert hk.scan(dq.data_ptr(), nq, dx.data_ptr(), N, d, metric, int(i8), 0, cells.nsplit, tps, tb, te,
                   dT.data_ptr(), cells.d.ptr, cells.i.ptr, cells.n.ptr, cells.cap, int(resume)) == 0
    return cells.read()


def run_bound(hk, cells: Cells, k, bound, narrow):
    b = Guarded(cells.nq, np.asarray(bound, dtype=np.float32))
    assert hk.bound(cells.d.ptr, cells.n.ptr, cells.nsplit, cells.cap, cells.nq, k, b.ptr, narrow) == 0
    return b.read().view(np.float32)


def run_select(hk, cells: Cells, k, narrow):
    od, oi = Guarded(cells.nq * k), Guarded(cells.nq * k)
    nflag, flagged = Guarded(1), Guarded(cells.nq)
    assert hk.select(cells.d.ptr, cells.i.ptr, cells.n.ptr, cells.nsplit, cells.cap, cells.nq, k, od.ptr, oi.ptr,
                     nflag.ptr, flagged.ptr, narrow) == 0
    nf = int(nflag.read().view(np.int32)[0])
    fl = flagged.read().view(np.int32)
    assert 0 <= nf <= cells.nq and np.all(fl[nf:].view(np.uint32) == SENT)
    return (od.read().view(np.float32).reshape(cells.nq, k), oi.read().view(np.int32).reshape(cells.nq, k), fl[:nf])


def check_bound_select(hk, cells: Cells, k, bound_in):
    """Both variants of bound and select over the device buffers against the model on their downloaded content."""
    cd, ci, cn = cells.read()
    want_b = M.bound_model(cd, cn, k, bound_in)
    want_d, want_i, want_f = M.select_model(cd, ci, cn, k)
    for narrow in (1, 0):
        b = run_bound(hk, cells, k, bound_in, narrow)
        np.testing.assert_array_equal(b, want_b, err_msg=f"bound narrow={narrow} k={k}")
        with np.errstate(invalid="ignore"):
            assert np.all(b <= np.asarray(bound_in, dtype=np.float32)), "bound raised"
        od, oi, fl = run_select(hk, cells, k, narrow)
        np.testing.assert_array_equal(oi, want_i, err_msg=f"select rows narrow={narrow} k={k}")
        np.testing.assert_array_equal(od, want_d, err_msg=f"select keys narrow={narrow} k={k}")
        np.testing.assert_array_equal(np.sort(fl), want_f, err_msg=f"flagged narrow={narrow} k={k}")
    c2 = cells.read()  # neither kernel writes the buffers
    for a, b_ in zip((cd, ci, cn), c2):
        np.testing.assert_array_equal(a.view(np.uint32), b_.view(np.uint32))


def check_cells(got, K, admit, nsplit, tps, cap, exact=True):
    """cand_n exact; the stored (key, row) of every cell the admitted set (a subset of it of min(count, cap) distinct
    rows when a cell overflows); every other slot still the sentinel; no id >= N; rows in their own split's cell."""
    cd, ci, cn = got
    nq, N = K.shape
    want_n = M.cell_counts(admit, nsplit, tps)
    np.testing.assert_array_equal(cn, want_n)
    stored = np.minimum(want_n, cap)
    valid = np.arange(cap)[None, None, :] < stored[:, :, None]
    assert np.all(cd.view(np.uint32)[~valid] == SENT) and np.all(ci.view(np.uint32)[~valid] == SENT)
    qq, ss, _ = np.nonzero(valid)
    rows, keys = ci[valid], cd[valid]
    assert np.all((rows >= 0) & (rows < N)), "row id out of range"
    np.testing.assert_array_equal(M.split_of_rows(N, tps)[rows], ss)
    seen = np.zeros((nq, N), dtype=np.int64)
    np.add.at(seen, (qq, rows), 1)
    if exact:
        assert np.all(want_n <= cap)
        np.testing.assert_array_equal(seen, admit.astype(np.int64))
    else:
        assert seen.max(initial=0) <= 1 and np.all(seen <= admit)
    np.testing.assert_array_equal(keys, K[qq, rows])


# ---- images -----------------------------------------------------------------------------------------------------
def _image_rows(rng, n, d):
    X = (rng.standard_normal((n, d)) * np.exp2(rng.integers(-6, 7, size=(n, 1)))).astype(np.float32)
    kinds = np.zeros(n, dtype=np.int64)  # 0 finite, 1 zero row, 2 inf, 3 NaN
    if n >= 16:
        X[3] = 0.0
        kinds[3] = 1
        X[5, d // 2] = np.inf
        X[7, 0] = -np.inf
        kinds[[5, 7]] = 2
        if d >= 2:  # one NaN element among finite ones
            X[9, d - 1] = np.nan
            kinds[9] = 3
    return X, kinds


def _prep(hk, X, fused):
    n, d = X.shape
    nb8, nb16 = hk.img8(n, d, R), hk.img16(n, d, R)
    nk8 = hk.nk8(d)
    ntiles = (n + R - 1) // R
    assert nk8 == M.i8_nk(d) and nb8 == ntiles * nk8 * 4 * R * 16 and nb16 == ntiles * M.b16_nk(d) * 4 * R * 16
    norm, scale, resid = Guarded(n), Guarded(n), Guarded(n)
    i8, b16 = Guarded(nb8 // 4), Guarded(nb16 // 4)
    dx = _dev(X)
    assert hk.prep(dx.data_ptr(), n, d, R, fused, norm.ptr, scale.ptr, resid.ptr, i8.ptr, b16.ptr) == 0
    return norm.read(), scale.read(), resid.read(), i8.read(), b16.read()


@pytest.mark.parametrize("d", M.IMAGE_D)
def test_images(hk, d):
    rng = np.random.default_rng(1000 + d)
    for n in M.IMAGE_N:
        X, kinds = _image_rows(rng, n, d)
        two = _prep(hk, X, 0)
        fused = _prep(hk, X, 1)
        finite = kinds <= 1
        # the fused route and the two-kernel route: the same bytes
        for name, a, b in zip(("norm", "scale", "resid", "int8 image", "bf16 image"), two, fused):
            if name == "norm":
                a, b = a[finite], b[finite]
                assert not np.isfinite(two[0].view(np.float32)[~finite]).any()
                assert not np.isfinite(fused[0].view(np.float32)[~finite]).any()
            np.testing.assert_array_equal(a, b, err_msg=f"{name} n={n} d={d}")
        norm, scale, resid = (a.view(np.float32) for a in two[:3])
        x64 = X.astype(np.float64)
        np.testing.assert_allclose(norm[finite], (x64[finite] ** 2).sum(1), rtol=1e-5)
        # scales and codes: numpy's float32 max / 127 and clip(rint(x / s))
        s = M.i8_scale(X)
        np.testing.assert_array_equal(scale.view(np.uint32), s.view(np.uint32))
        codes = M.i8_codes(X, s)
        want8 = M.tiled_image(codes, n, d, R, 16, M.i8_nk(d))
        np.testing.assert_array_equal(two[3].view(np.int8), want8.ravel(), err_msg=f"int8 image n={n} d={d}")
        assert np.all(scale[kinds == 1] == 0) and np.all(scale[kinds == 2] == 0) and np.all(scale[kinds == 3] > 0)
        # residuals: the certificate's safe direction, within 0.1 %; +inf for rows that are not entirely finite
        true = np.sqrt(((x64[finite] - s[finite, None].astype(np.float64) * codes[finite]) ** 2).sum(1))
        r = resid[finite].astype(np.float64)
        print(f"n={n} d={d} resid/true min {np.min(r[true > 0] / true[true > 0], initial=np.inf):.7f} "
              f"max {np.max(r[true > 0] / true[true > 0], initial=0):.7f}")
        assert np.all(r >= true), f"resid below the true residual n={n} d={d}: {np.min(r - true)}"
        assert np.all(r <= 1.001 * true), f"resid above 1.001 x n={n} d={d}"
        assert np.all(resid[kinds == 1] == 0)
        assert np.all(np.isposinf(resid[~finite])), f"non-finite rows must get resid = +inf: {resid[~finite]}"
        # bf16 image: RNE bf16 in the same layout (NaN elements: any bf16 NaN)
        nan = np.isnan(X)
        want16 = M.tiled_image(M.bf16_bits(np.where(nan, np.float32(0), X)).reshape(n, d), n, d, R, 8, M.b16_nk(d)).ravel()
        nan16 = M.tiled_image(nan, n, d, R, 8, M.b16_nk(d)).ravel()
        got16 = two[4].view(np.uint16)
        np.testing.assert_array_equal(got16[~nan16], want16[~nan16], err_msg=f"bf16 image n={n} d={d}")
        assert np.all((got16[nan16] & 0x7FFF) > 0x7F80)


# ---- keys mode --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i8,d", [(True, d) for d in M.KEYS_D_I8] + [(False, d) for d in M.KEYS_D_B16])
def test_keys_mode(hk, i8, d):
    rng = np.random.default_rng(2000 + d + int(i8))
    Q = M.exact_rows(rng, max(M.KEYS_NQ), d, i8)
    X = M.exact_rows(rng, max(M.KEYS_N), d, i8)
    X[10], X[300], X[1279] = Q[20], Q[256], Q[319]  # rows equal to a query: L2 key exactly 0
    X[11] = M.clamp_row(d, i8)  # and one whose L2 expression is negative before the clamp
    Q[21] = X[11]
    for metric in (M.L2, M.IP):
        K = M.keys_model(Q, X, metric, i8)
        if metric == M.L2:
            assert K[20, 10] == 0 and K[21, 11] == 0 and K.min() == 0
        for nq in M.KEYS_NQ:
            for N in M.KEYS_N:
                nt = N // R
                geoms = [(nt, 1)] + ([(1, nt), (2, (nt + 1) // 2)] if N == max(M.KEYS_N) else [])
                for nsplit, tps in geoms:  # (nt, 1): the seed pass's own geometry
                    got = run_keys(hk, Q[:nq], X[:N], metric, i8, nsplit, tps)
                    np.testing.assert_array_equal(got, K[:nq, :N], err_msg=f"metric={metric} nq={nq} N={N} {nsplit}x{tps}")


def test_pass_hook_rejects_what_the_product_rejects(hk):
    rng = np.random.default_rng(5)
    Q, X = M.exact_bf16_rows(rng, 256, 65), M.exact_bf16_rows(rng, 256, 65)
    got = run_keys(hk, Q, X, M.L2, False, 1, 1, rc=-1)  # ceil(65 / 32) = 3 chunks: odd
    assert np.all(got.view(np.uint32) == SENT)
    Q, X = M.exact_i8_rows(rng, 256, 64), M.exact_i8_rows(rng, 256, 64)
    out = Guarded(256 * 256)
    dq, dx = _dev(Q), _dev(X)
    assert hk.scan(dq.data_ptr(), 256, dx.data_ptr(), 256, 64, M.L2, 2, 1, 1, 1, 0, 1, None, out.ptr, None, None, 0, 0) == -1
    assert np.all(out.read() == SENT)  # int8 rows without the query scales: refused by the launcher
    assert hk.scan(dq.data_ptr(), 256, dx.data_ptr(), 256, 64, M.L2, 1, 0, 1, 1, 0, 1, None, out.ptr, None, None, 0, 0) == -1


# ---- filter mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [M.L2, M.IP])
@pytest.mark.parametrize("i8,d", [(True, d) for d in M.FILTER_D[True]] + [(False, d) for d in M.FILTER_D[False]])
def test_filter_mode(hk, i8, d, metric):
    rng = np.random.default_rng(3000 + d + 7 * int(i8) + metric)
    nq = 257
    Q = M.exact_rows(rng, nq, d, i8)
    Xall = M.with_ties(rng, M.exact_rows(rng, max(M.FILTER_N), d, i8), max(M.FILTER_N))
    Xall[0] = M.clamp_row(d, i8)  # query 21 (T = one of its keys) admits it with the append path's clamp at 0
    Q[21] = Xall[0]
    Kall = M.keys_model(Q, Xall, metric, i8)
    if metric == M.L2:
        assert Kall[21, 0] == 0 and Kall[21].min() == 0
    dq = _dev(Q)
    for N in M.FILTER_N:
        K = Kall[:, :N]
        T = M.filter_bounds(K)
        dx = _dev(Xall[:N])
        for nsplit, tps in M.filter_geometries(N):
            tag = f"N={N} {nsplit}x{tps}"
            cap = tps * R + 3  # a split's rows: no cell can overflow
            admit = M.pass_mask(K, T, nsplit, tps, 0, tps)
            cells = Cells(nq, nsplit, cap)
            got = run_pass(hk, cells, dq, dx, nq, N, d, metric, i8, tps, 0, tps, T, False)
            check_cells(got, K, admit, nsplit, tps, cap)
            # the four kinds of bound do what they say
            assert admit[4::5].all() and not admit[2::5].any() and not admit[3::5].any(), tag
            assert all(K[q][admit[q]].max() == T[q] for q in range(1, nq, 5)), tag  # the boundary row is admitted
            if N in (257, 1793):  # bound and select over these buffers, both variants
                check_bound_select(hk, cells, 10, np.full(nq, np.inf, dtype=np.float32))
                check_bound_select(hk, cells, 64, T)
            # overflow: the count is still the true count, the first cap slots a subset of the admitted set
            small = Cells(nq, nsplit, 5)
            got = run_pass(hk, small, dq, dx, nq, N, d, metric, i8, tps, 0, tps, T, False)
            check_cells(got, K, admit, nsplit, tps, 5, exact=False)
            if N == 1793:
                assert (got[2] > 5).any()
                check_bound_select(hk, small, 10, np.full(nq, np.inf, dtype=np.float32))
            # resume: [0, b) then [b, tps) continues the buffers; the first pass's entries stay as a prefix
            for b in {1, tps // 2, tps - 1} - {0, tps}:
                cells = Cells(nq, nsplit, cap)
                first = run_pass(hk, cells, dq, dx, nq, N, d, metric, i8, tps, 0, b, T, False)
                check_cells(first, K, M.pass_mask(K, T, nsplit, tps, 0, b), nsplit, tps, cap)
                both = run_pass(hk, cells, dq, dx, nq, N, d, metric, i8, tps, b, tps, T, True)
                check_cells(both, K, admit, nsplit, tps, cap)
                pre = np.arange(cap)[None, None, :] < first[2][:, :, None]
                np.testing.assert_array_equal(both[0].view(np.uint32)[pre], first[0].view(np.uint32)[pre], err_msg=tag)
                np.testing.assert_array_equal(both[1][pre], first[1][pre], err_msg=tag)


# ---- bound and select on synthetic buffers ----------------------------------------------------------------------
def _synthetic(rng, nsplit, cap, k):
    """One query per pattern: totals around k, 64 and 256 with distinct, all-equal and few-valued keys (all-equal
    keys all lie at the narrowing threshold: list lengths <= 64, <= 256 and the wave-list fallback), a tie run
    straddling k with rows out of order across splits, +-0 and negative keys, empty cells, one overflowed cell."""
    slots = nsplit * cap
    totals = sorted({0, k - 1, k, 64, 65, 256, 257, min(290, slots)})
    pats = []
    for t in totals:
        pats.append(rng.standard_normal(t).astype(np.float32) * 50)  # distinct, signed (IP keys)
        pats.append(np.full(t, 2.5, dtype=np.float32))
        pats.append(np.full(t, -1.0, dtype=np.float32))
        pats.append(rng.integers(0, 3, size=t).astype(np.float32))
    lo = np.arange(max(k - 3, 0), dtype=np.float32) - 100
    pats.append(np.concatenate([lo, np.full(10, 7.0, np.float32), 8 + rng.random(90).astype(np.float32)]))
    pats.append(np.concatenate([np.full(35, -0.0, np.float32), np.zeros(35, np.float32), -rng.random(5).astype(np.float32)]))
    pats.append(rng.standard_normal(40).astype(np.float32))  # (the overflowed query)
    nq = len(pats)
    cd = np.full((nq, nsplit, cap), np.nan, dtype=np.float32)
    ci = np.full((nq, nsplit, cap), -7, dtype=np.int32)
    cn = np.zeros((nq, nsplit), dtype=np.int32)
    for q, keys in enumerate(pats):
        t = len(keys)
        cell = np.sort(rng.permutation(slots)[:t] // cap)  # entries per cell, at most cap each
        rows = M.distinct_rows(rng, t)
        if q == nq - 3:  # the tie run: rows descending while the split index ascends
            rows = np.sort(rows)[::-1].copy()
        else:
            keys = keys[rng.permutation(t)]
        for s in range(nsplit):
            sel = cell == s
            n = int(sel.sum())
            cn[q, s] = n
            cd[q, s, :n] = keys[sel]
            ci[q, s, :n] = rows[sel]
    s_over = int(np.argmax(cn[nq - 1]))
    cn[nq - 1, s_over] = cap + 3  # counted past its capacity: the first cap slots are what it holds
    cd[nq - 1, s_over] = rng.standard_normal(cap).astype(np.float32)
    ci[nq - 1, s_over] = M.distinct_rows(rng, cap)
    bound = np.array([np.inf, -1e30, 1e30, 0.0, 2.5], dtype=np.float32)[np.arange(nq) % 5]
    return cd, ci, cn, bound


@pytest.mark.parametrize("nsplit", [1, 3, 64, 65, 130])
@pytest.mark.parametrize("k", [1, 10, 32, 64])
def test_bound_select_synthetic(hk, nsplit, k):
    rng = np.random.default_rng(4000 + 10 * nsplit + k)
    cap = max(8, -(-300 // nsplit))
    cd, ci, cn, bound = _synthetic(rng, nsplit, cap, k)
    nq = len(cd)
    assert (cn[:-1] <= cap).all() and (cn[-1] > cap).sum() == 1 and (cn == 0).any()
    cells = Cells(nq, nsplit, cap, cd, ci, cn)
    check_bound_select(hk, cells, k, bound)
    _, _, fl = run_select(hk, cells, k, 1)
    assert list(fl) == [nq - 1]  # the overflowed query, once


# ---- composition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [M.L2, M.IP])
@pytest.mark.parametrize("i8,d", [(True, 300), (False, 128)])
@pytest.mark.parametrize("bounds", [[0, 1, 3], [0, 1, 2, 3]])
def test_composition(hk, i8, d, metric, bounds):
    """Seed keys on the first 256 rows -> flat_keys_kth -> pass 0 -> bound -> pass 1 (resume) ... -> select equals the
    brute-force top-64 by (key, row) of the exact keys for every query; no query is flagged."""
    rng = np.random.default_rng(5000 + d + metric)
    nq, N, k, nsplit, tps, cap = 257, 2304, 64, 3, 3, 768
    Q = M.exact_rows(rng, nq, d, i8)
    X = M.with_ties(rng, M.exact_rows(rng, N, d, i8), N)
    K = M.keys_model(Q, X, metric, i8)
    want_d, want_i = M.brute_topk(K, k)
    dq, dx = _dev(Q), _dev(X)
    seed_keys = Guarded(nq * R)
    assert hk.scan(dq.data_ptr(), nq, dx.data_ptr(), R, d, metric, int(i8), 1, 1, 1, 0, 1, None, seed_keys.ptr, None,
                   None, 0, 0) == 0
    np.testing.assert_array_equal(seed_keys.read().view(np.float32).reshape(nq, R), K[:, :R])
    bound = Guarded(nq)
    assert hk.kth(seed_keys.ptr, R, nq, k, bound.ptr, 1) == 0
    T = bound.read().view(np.float32)
    np.testing.assert_array_equal(T, M.kth_bound(K[:, :R], k))
    cells = Cells(nq, nsplit, cap)
    for p in range(len(bounds) - 1):
        dT = _dev(T)
        assert hk.scan(dq.data_ptr(), nq, dx.data_ptr(), N, d, metric, int(i8), 0, nsplit, tps, bounds[p], bounds[p + 1],
                       dT.data_ptr(), cells.d.ptr, cells.i.ptr, cells.n.ptr, cap, int(p > 0)) == 0
        if p + 2 < len(bounds):
            T2 = run_bound(hk, cells, k, T, 1)
            assert np.all(T2 <= T)
            T = T2
    for narrow in (1, 0):
        od, oi, fl = run_select(hk, cells, k, narrow)
        assert len(fl) == 0
        np.testing.assert_array_equal(oi, want_i)
        np.testing.assert_array_equal(od, want_d)
    # the composition of the model agrees (same plan), and the kernels admitted no more than it predicts
    md, mi, mf, mn = M.compose_model(K, k, nsplit, tps, bounds, R, cap)
    np.testing.assert_array_equal(mi, want_i)
    assert len(mf) == 0
