"""The inputs and the numpy model of tests/_ivf_scan_cases.py, checked on the CPU: the exact family is exact (every
key recomputed in int64 / fp64 equals the staged fp32 model bit for bit and fits fp32), the model's selections equal
brute force, every case reaches what its name claims, and the plan tables equal the library's own plan arithmetic
(hipann_debug_ivf_seed_items / _slots, host-only)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import _ivf_scan_cases as M

F = np.float32


def _exact32(v64):
    v64 = np.asarray(v64, np.float64)
    return np.array_equal(v64.astype(F).astype(np.float64), v64)


@pytest.mark.parametrize("name", sorted(M.SCAN_CASES))
@pytest.mark.parametrize("metric", [M.L2, M.IP])
def test_exact_int8_family_is_exact(name, metric):
    lists, Q, _ = M.scan_case(name, M.I8)
    X = lists.rows
    keys, pl = M.keys_i8(Q, X, metric)
    # s = 2^e, the units are the integers, the residuals vanish
    for V, s, u in ((X, pl["xs8"], pl["xu"]), (Q, pl["qs8"], pl["qu"])):
        assert np.all(np.log2(s) == np.round(np.log2(s))) and np.all(np.abs(u).max(axis=1) == 127)
        assert np.array_equal(s[:, None].astype(np.float64) * u, V.astype(np.float64))
    assert not pl["xr8"].any()
    # int64 in units of 2^-2 per element: norms, dots and keys
    Xi, Qi = np.rint(X.astype(np.float64) * 4).astype(np.int64), np.rint(Q.astype(np.float64) * 4).astype(np.int64)
    assert np.array_equal(Xi / 4.0, X) and np.array_equal(Qi / 4.0, Q)
    xn, qn, dot = (Xi * Xi).sum(1), (Qi * Qi).sum(1), Qi @ Xi.T
    assert np.array_equal(pl["xnorm"].astype(np.float64) * 16, xn) and np.array_equal(pl["qhn2"].astype(np.float64) * 16, qn)
    if metric == M.L2:
        want = qn[:, None] + xn[None, :] - 2 * dot
        assert want.min() >= 0 and (want == 0).any() == (X.shape[1] >= 20)  # the planted row: key 0
        assert _exact32((qn[:, None] + xn[None, :]) / 16.0)  # the key's first sum
    else:
        want = -dot
        assert want.size < 32 or ((want < 0).any() and (want > 0).any())  # negative and positive dots
    assert np.abs(want).max() < 2 ** 24 and _exact32(want / 16.0)
    assert np.array_equal(keys.astype(np.float64) * 16, want)
    # the int32 sums and their scaled products
    su = pl["qu"].astype(np.int64) @ pl["xu"].astype(np.int64).T
    assert np.abs(su).max() < 2 ** 24 and _exact32(su * (pl["qs8"][:, None].astype(np.float64) * pl["xs8"][None, :]))


@pytest.mark.parametrize("name", sorted(M.SCAN_CASES))
@pytest.mark.parametrize("metric", [M.L2, M.IP])
def test_exact_fp16_family_is_exact(name, metric):
    lists, Q, _ = M.scan_case(name, M.HALF)
    X = lists.rows
    ok, es = M.half_es(X)
    assert ok
    ns = M.nsup_half(X.shape[1])
    img = M.half_val(M.half_bits((X * F(2.0 ** es)).astype(F)))
    assert np.array_equal(img.astype(np.float64) * 2.0 ** -es, X)  # the image is the rows
    hs, its, r2, r1, okq = M.split_queries_h(Q, ns, es)
    assert okq.all() and not r1.any() and not r2.any() and not hs[:, 1].any()  # one term holds the query
    keys, pl = M.keys_half(Q, X, metric, es)
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    dot = Q64 @ X64.T
    want = (Q64 ** 2).sum(1)[:, None] + (X64 ** 2).sum(1)[None, :] - 2 * dot if metric == M.L2 else -dot
    # every partial sum of the MFMA is a sum of integer products (in units of 2^-6) below 2^24
    assert (np.abs(np.rint(Q64 * 8)).astype(np.int64) @ np.abs(np.rint(X64 * 8)).astype(np.int64).T).max() < 2 ** 24
    assert _exact32(want) and _exact32(pl["av"])
    assert np.array_equal(keys.astype(np.float64), want)
    if metric == M.L2:
        assert want.min() >= 0 and (want == 0).any() == (X.shape[1] >= 20)


def _brute(keys, rows, n):
    t = sorted((int(M.sortable(np.array([k], F))[0]), int(r)) for k, r in zip(keys, rows))[:n]
    return [r for _, r in t]


@pytest.mark.parametrize("name", ["lists_d64", "chunk2049_d64", "wave7_share16_d20", "share15_d20"])
@pytest.mark.parametrize("sub", [0, 1])
def test_scan_model_equals_brute_force(name, sub):
    lists, Q, probes = M.scan_case(name, M.I8)
    keys, _ = M.keys_i8(Q, lists.rows, M.L2)
    slots, bound = M.scan_model(keys, lists, probes, sub)
    for q in range(0, len(Q), 5):
        want_b = np.inf
        for p, l in enumerate(probes[q]):
            rows = np.arange(lists.off[l], lists.off[l + 1])
            for c in range(-(-len(rows) // M.CH)):
                kd, ki = slots[(q, p, c)]
                cr = rows[c * M.CH:(c + 1) * M.CH]
                for w in range(M.WAVES if sub else 1):
                    mine = np.concatenate([cr[i:i + 32] for i in range(32 * w, len(cr), 256)] + [cr[:0]]) if sub else cr
                    want = _brute(keys[q, mine], mine, M.K)
                    assert list(ki[w][:len(want)]) == want and np.all(ki[w][len(want):] == M.PAD_ID)
                    assert np.array_equal(kd[w][:len(want)], keys[q, want]) and np.all(np.isinf(kd[w][len(want):]))
                    if len(want) == M.K:
                        want_b = min(want_b, float(keys[q, want[-1]]))
        assert M.decode_bound(bound[q]) == F(want_b)
    sd, si, b2 = M.seed_model(keys, lists, probes, bound)
    for q in range(0, len(Q), 5):
        ent = [(k, r) for (qq, p, c), (kd, ki) in slots.items() if qq == q and c == 0
               for k, r in zip(kd.ravel(), ki.ravel()) if r != M.PAD_ID and k <= M.decode_bound(bound[q])] if sub else []
        if sub:
            want = _brute([k for k, _ in ent], [r for _, r in ent], M.SEED_K)
            assert list(si[q][:len(want)]) == want and np.all(si[q][len(want):] == M.PAD_ID)


def test_rerank_select_equals_brute_force():
    rng = np.random.default_rng(5)
    for total, k in ((0, 16), (1, 16), (15, 16), (16, 16), (700, 64), (4096, 64), (4097, 64), (6000, 20)):
        pd = rng.permutation(total).astype(F) * F(0.5)  # distinct keys: no tie rule involved
        pi = rng.integers(0, 1000, total)
        kd, ki = M.rerank_select(pd, pi, k, 1000, M.INF, 0)
        o = np.argsort(pd, kind="stable")[:k]
        assert np.array_equal(kd, pd[o]) and np.array_equal(ki, pi[o])
    # ties at the k-th key: the wave select keeps the first in (wave, position) order, the lists the smallest rows
    pd = np.ones(512, F)
    pi = np.arange(512)[::-1].copy()
    kd, ki = M.rerank_select(pd, pi, 16, 1000, M.INF, 0)
    assert np.array_equal(np.sort(ki), np.sort(pi[:16]))  # wave 0's first strip
    pd = np.ones(5000, F)
    pi = np.arange(5000)[::-1].copy()
    kd, ki = M.rerank_select(pd, pi, 16, 5000, M.INF, 0)
    assert np.array_equal(ki, np.arange(16))


def test_scan_order_rule():
    # four rows tied at the 2nd distance over two probe ranks: the first two in scan order are admitted (one slot is
    # left after the one below T), of which the smallest label stays
    dist = np.array([1, 2, 2, 2, 2, 3], F)
    labels = np.array([9, 50, 40, 30, 20, 1])
    pos = np.array([5, 3, 1, 4, 2, 0])  # scan order: label 40 (pos 1), 20 (pos 2), 50, 30, then the one below T
    sel = M.scan_order_topk(dist, labels, pos, 2)
    assert list(labels[sel]) == [9, 20]  # first two at <= T in scan order: labels 40, 20 -> the smallest label
    sel = M.scan_order_topk(dist, labels, pos, 3)
    assert list(labels[sel]) == [9, 20, 40]


def test_cases_reach_what_they_claim():
    S = M.SCAN_CASES
    nch = lambda name: [-(-s // M.CH) for s in S[name][0]]
    assert nch("chunk2048_d832") == [1] and nch("chunk2049_d64") == [2] and max(nch("lists_d64")) == 3
    assert S["tile33_d192"][0][0] % 32 == 1 and S["chunk2049_d64"][0][0] % M.CH == 1  # a last pass / chunk of one row
    assert S["groups97_d20"][1] > 96 and S["groups100_chunks_d100"][1] > 96
    assert M.nsup_i8(832) > M.MH_P and M.nsup_i8(64) == M.MH_P and M.nsup_half(20) == M.MH_P
    assert {S[n][2] for n in S} >= {1, 20, 64, 100, 192, 832}
    assert {S[n][1] for n in S} >= {1, 15, 17, 40, 97, 100}
    sizes = {s for n in S for s in S[n][0]}
    assert sizes >= {0, 1, 15, 16, 17, 33, 256, 2048, 2049} and any(4100 <= s <= 4300 for s in sizes)
    for name, want in (("wave7_share16_d20", 16), ("wave7_share15_d20", 15), ("share16_d64", 16), ("share15_d20", 15)):
        lists, _, _ = M.scan_case(name, M.I8)
        sh = M.shares(lists, 0)
        assert len(sh[(0, max(w for _, w in sh))]) == want, name
    assert set(M.SINGLE_ITEM) | set(M.MULTI_ITEM) == set(S) and "lists_d64" in M.MULTI_ITEM
    # the planted rows: an all-equal list and duplicates of query 0's row in other passes, waves, chunks and lists
    lists, Q, _ = M.scan_case("lists_d64", M.I8)
    off = lists.off
    assert np.all(lists.rows[off[4]:off[5]] == lists.rows[off[4]])
    dup = np.nonzero((lists.rows == Q[0]).all(1))[0]
    assert len({int(np.searchsorted(off, r, side="right")) for r in dup}) >= 3
    big = dup[dup >= off[5]] - off[5]
    assert len(set(big // M.CH)) >= 2 and len(set((big % M.CH) // 32 % 8)) >= 2, big


@pytest.mark.parametrize("name", sorted(M.SCAN_CASES))
def test_plan_tables_equal_the_library(hipann_mod, name):
    L = hipann_mod.lib()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    lists, Q, probes = M.scan_case(name, M.I8)
    cnt, item_off, goff, slot_off = M.plan_model(lists, probes, 96)
    nl = lists.nlist
    io, go = np.zeros(nl + 1, np.int32), np.zeros(nl + 1, np.int32)
    a, b = np.full((256, 3), -1, np.int32), np.full((256, 3), -1, np.int32)
    assert L.hipann_debug_ivf_seed_items(ip(lists.lens.astype(np.int32)), ip(cnt.astype(np.int32)), nl, 96 << 8, ip(io),
                                         ip(go), 256, ip(a), ip(b)) == 0
    assert np.array_equal(io, item_off) and np.array_equal(go, goff)
    nq, npr = probes.shape
    cslot, bcnt = np.zeros(nq * npr, np.int64), np.zeros(nq, np.int32)
    L.hipann_debug_ivf_seed_slots(ip(slot_off.astype(np.int32)), npr, C.c_int64(nq),
                                  cslot.ctypes.data_as(C.POINTER(C.c_int64)), ip(bcnt))
    nch = -(-lists.lens // M.CH)
    assert np.all(bcnt == np.maximum(nch - 1, 0).sum())
    assert np.array_equal(cslot[::npr], slot_off[:-1:npr] + np.arange(nq) + 1)
