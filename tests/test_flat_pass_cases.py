"""CPU tests of the Flat bounded passes' cases and model (tests/_flat_pass_cases.py) and of the pass plan hook.

The GPU tests (test_flat_passes_gpu.py) compare kernels with this model bit for bit; that only means something if
the model's inputs are exact in fp32 and the model itself is right.  Here: every intermediate of the exact builders
fits 24 significant bits and the float32 restatement of the kernel's arithmetic equals the int64 / float64 value;
the multi-pass composition equals brute-force top-k by (key, row); the tie cases tie across the k-th boundary; the
overflow cases overflow; and hipann_debug_flat_pass_plan's boundaries and capacity are sane over a sweep.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import _flat_pass_cases as M


@pytest.mark.parametrize("i8,d", [(True, d) for d in (1, 64, 129, 300, 1024)] + [(False, d) for d in (33, 64, 192, 256)])
@pytest.mark.parametrize("metric", [M.L2, M.IP])
def test_exact_builders_are_exact(i8, d, metric):
    rng = np.random.default_rng(100 + d)
    Q = M.exact_rows(rng, 40, d, i8)
    X = M.exact_rows(rng, 300, d, i8)
    if i8:
        for A in (Q, X):
            s = M.i8_scale(A)
            c = M.i8_codes(A, s).astype(np.float64)
            e = np.log2(s.astype(np.float64))
            assert np.all(e == np.rint(e)) and set(e) <= {-1.0, 0.0, 1.0}  # the scale is 2^e exactly
            assert np.all(c * s[:, None] == A.astype(np.float64))  # codes are the integers, residual 0
            assert np.all(np.abs(c).max(1) == 127)
            small = np.sort(np.abs(c), axis=1)[:, :-1]
            assert small.size == 0 or small.max() <= 3
    else:
        assert np.all(M.bf16_round(X) == X) and np.all(M.bf16_round(Q) == Q) and max(np.abs(Q).max(), np.abs(X).max()) <= 8
    X[7] = Q[3]  # a row equal to a query
    X[8] = M.clamp_row(d, i8)
    Q[5] = X[8]
    parts: dict = {}
    K = M.keys_exact(Q, X, metric, i8, parts)
    for name in ("acc", "dot", "qn", "xn", "s", "key"):
        assert M.fits24(parts[name]), name
    # the unclamped L2 expression too (what the kernel forms before the clamp)
    if metric == M.L2:
        raw = parts["qn"][:, None] - parts["s"]
        assert M.fits24(raw)
        assert raw[3, 7] == 0.0  # a row equal to its query: exactly 0
        assert (raw[5, 8] < 0.0 or d == 1) and K[5, 8] == 0.0  # the clamp row: negative before the clamp
    K32 = M.keys_fp32(Q, X, metric, i8)
    np.testing.assert_array_equal(K32.astype(np.float64), K)
    np.testing.assert_array_equal(M.keys_model(Q, X, metric, i8).view(np.uint32), (K32 + np.float32(0)).view(np.uint32))


def test_bf16_round_is_rne():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3.0 * 2.0 ** -8, 1.0 + 3.0 * 2.0 ** -9, -2.5, 0.0, 3.0e38], dtype=np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -2.5, 0.0, 2.9908e38], dtype=np.float32)
    got = M.bf16_round(x)
    np.testing.assert_array_equal(got[:6], want[:6])
    assert got[6].view(np.uint32) & 0xFFFF == 0 and abs(got[6] / x[6] - 1) < 2.0 ** -8


def test_tiled_image_layout():
    n, d, R, nk = 300, 70, 256, M.i8_nk(70)
    V = (np.arange(n * d).reshape(n, d) % 251 - 125).astype(np.int8)
    img = M.tiled_image(V, n, d, R, 16, nk).reshape(-1, 16)
    for t, kc, c, row in [(0, 0, 0, 0), (0, 1, 0, 5), (1, 0, 3, 43), (1, 1, 2, 255), (0, 0, 1, 2)]:
        u = ((t * nk + kc) * 4 + c) * R + (row ^ (2 * c))
        g = t * R + row
        want = np.zeros(16, dtype=np.int8)
        if g < n:
            lo = 64 * kc + 16 * c
            seg = V[g, lo : min(lo + 16, d)] if lo < d else V[g, :0]
            want[: len(seg)] = seg
        np.testing.assert_array_equal(img[u], want)
    assert img.shape[0] == 2 * nk * 4 * R


def _case(rng, nq, N, d, i8, metric, ties):
    Q = M.exact_rows(rng, nq, d, i8)
    X = M.exact_rows(rng, N, d, i8)
    if ties:
        X = M.with_ties(rng, X, N)
    return M.keys_model(Q, X, metric, i8)


@pytest.mark.parametrize("i8", [True, False])
@pytest.mark.parametrize("metric", [M.L2, M.IP])
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("k", [1, 10, 32, 64])
def test_composition_equals_brute_force(i8, metric, ties, k):
    rng = np.random.default_rng(7 + k)
    N, nsplit, tps = 2304, 3, 3
    K = _case(rng, 33, N, 129 if i8 else 64, i8, metric, ties)
    want_d, want_i = M.brute_topk(K, k)
    if ties:  # the k-th and (k+1)-th keys tie for (nearly) every query: rows decide
        srt = np.sort(K, axis=1)
        share = float(np.mean(srt[:, k - 1] == srt[:, k]))
        assert share >= 0.9, share
    for bounds in ([0, 3], [0, 1, 3], [0, 1, 2, 3]):
        od, oi, fl, cn = M.compose_model(K, k, nsplit, tps, bounds, sample=256, cap=768)
        assert len(fl) == 0
        np.testing.assert_array_equal(oi, want_i)
        np.testing.assert_array_equal(od.view(np.uint32), want_d.view(np.uint32))


def test_overflow_cases_overflow_and_others_do_not():
    """The cap condition of the GPU overflow test, checked on the reference: a cell overflows iff its admitted count
    exceeds cap; select then flags exactly the queries with such a cell."""
    rng = np.random.default_rng(3)
    K = _case(rng, 40, 1793, 64, False, M.L2, False)
    T = M.filter_bounds(K)
    nsplit, tps = 2, 4
    admit = M.pass_mask(K, T, nsplit, tps, 0, tps)
    cnt = M.cell_counts(admit, nsplit, tps)
    big = 4 * M.TILE
    assert cnt.max() <= big  # the no-overflow capacity of the GPU filter tests: a split's rows
    cd, ci, cn = M.cells_from_mask(K, admit, nsplit, tps, big)
    assert len(M.select_model(cd, ci, cn, 10)[2]) == 0
    cap = 5
    over = (cnt > cap).any(1)
    assert over[4::5].all()  # T = +inf admits every row: always an overflow at cap 5
    assert not over[2::5].any() and not over[3::5].any()  # nothing admitted
    assert 0 < over.sum() < len(over)
    cd, ci, cn = M.cells_from_mask(K, admit, nsplit, tps, cap)
    np.testing.assert_array_equal(cn, cnt)  # counts keep counting past cap
    od, oi, fl = M.select_model(cd, ci, cn, 10)
    np.testing.assert_array_equal(fl, np.flatnonzero(over))
    assert np.all(oi[over] == M.PAD_ROW) and np.all(np.isinf(od[over]))
    # admitted sets: boundary rows in (T equal to a key), nothing below the smallest key, everything at +inf
    assert all(admit[q].sum() >= 1 and K[q][admit[q]].max() == T[q] for q in range(1, 40, 5))
    assert admit[4::5].all()


def test_bound_model():
    cd = np.array([[[1.0, 5.0, np.nan], [3.0, -2.0, 4.0]]], dtype=np.float32)
    cn = np.array([[2, 3]], dtype=np.int32)
    b = M.bound_model(cd, cn, 3, np.array([np.inf], dtype=np.float32))
    assert b[0] == np.float32(3.0) * np.float32(1.0 + 2.0 ** -20)
    assert M.bound_model(cd, cn, 3, np.array([2.0], dtype=np.float32))[0] == 2.0  # never raised
    assert np.isinf(M.bound_model(cd, cn, 6, np.array([np.inf], dtype=np.float32))[0])  # fewer than k: unchanged
    assert M.widen(np.array([0.0], dtype=np.float32))[0] == np.float32(2.0 ** -100)
    assert M.widen(np.array([-4.0], dtype=np.float32))[0] == np.float32(-4.0)  # t (1 + 2^-20) < t: the sum wins
    cn[0, 0] = 7  # an overflowed cell offers its first cap entries
    cd[0, 0, 2] = 0.5
    assert M.bound_model(cd, cn, 1, np.array([np.inf], dtype=np.float32))[0] == np.float32(-2.0)


def test_filter_case_tables_cover_every_ring_residue():
    """G = (tiles of a block) x (K-steps per tile) over the filter cases covers every residue of the 3-slot fragment
    ring and the 5-stage LDS ring, and ns = 1 .. 8 (int8) / 1 .. 4 (bf16) over the keys cases."""
    G = set()
    for i8 in (True, False):
        for d in M.FILTER_D[i8]:
            for N in M.FILTER_N:
                for nsplit, tps in M.filter_geometries(N):
                    nt = (N + M.TILE - 1) // M.TILE
                    for s in range(nsplit):
                        G.add((min((s + 1) * tps, nt) - s * tps) * M.steps_per_tile(d, i8))
    assert {g % 3 for g in G} == {0, 1, 2} and {g % 5 for g in G} == {0, 1, 2, 3, 4}
    assert sorted({M.steps_per_tile(d, True) for d in M.KEYS_D_I8}) == list(range(1, 9))
    assert sorted({M.steps_per_tile(d, False) for d in M.KEYS_D_B16}) == [1, 2, 3, 4]
    assert all(M.b16_nk(d) % 2 == 0 for d in M.KEYS_D_B16)
    assert any(nsplit * tps > (N + 255) // 256 for N in M.FILTER_N for nsplit, tps in M.filter_geometries(N))  # short last split


def test_pass_plan_hook(hipann_mod):
    L = hipann_mod.lib()
    f = L.hipann_debug_flat_pass_plan
    f.restype = C.c_int
    f.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    b = (C.c_int64 * 8)()
    nb, cap = C.c_int(0), C.c_int(0)
    sample = 16384
    npass = set()
    for nsplit in (1, 8, 64, 256):
        for k in (32, 64):
            for nq in (256, 1024, 8192):
                for tps in range(1, 601):
                    assert f(tps, nsplit, sample, k, nq, b, C.byref(nb), C.byref(cap)) == 0
                    pb = [int(b[i]) for i in range(nb.value)]
                    assert 2 <= len(pb) <= 7 and pb[0] == 0 and pb[-1] == tps, (tps, nsplit, pb)
                    assert all(x < y for x, y in zip(pb, pb[1:])), (tps, nsplit, pb)
                    c = cap.value
                    assert c % 32 == 0 and 32 <= c <= 1 << 20, (tps, nsplit, pb, c)
                    assert c >= M.expected_fill(pb, nsplit, sample, k), (tps, nsplit, pb, c)
                    npass.add(len(pb) - 1)
    assert len(npass) >= 3  # the sweep reaches single- and multi-pass plans
    assert f(0, 1, sample, 64, 256, b, C.byref(nb), C.byref(cap)) == -1
    assert f(10, 0, sample, 64, 256, b, C.byref(nb), C.byref(cap)) == -1
