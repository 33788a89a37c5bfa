"""The IVF image scans' kernels (csrc/ivf_mfma.hip, csrc/ivf_kernels.hip) against the numpy model of
_ivf_scan_cases.py: the tiled fp16 / int8 images and their per-row planes, the query preparation, one launch of the
scan (slot by slot), the seeded scan's two launches around ivf_seed_bound, and ivf_rerank_topk alone with each of its
three certificates decided on both sides of the threshold.

Every other test of this path is end to end, where the exact rerank and the device fallback repair a filter that drops
or invents a row and a certificate that is too lenient returns the right answer whenever the filter did not miss.
These tests run the stages themselves through the library's test hooks: hipann_debug_ivf_set stops ivf_shard_search
after its scan step (and forces the seeded path on or off), hipann_debug_ivf_read / _info read the shard's buffers back
by name, hipann_debug_ivf_rerank calls launch_ivf_rerank over caller-owned arrays with no fallback behind it.  The
probes come from the caller (nprobe = nlist, hand-made lists), so the coarse step is no part of them.

Found by these tests (both fixed with them): the int8 builders' residual x - fl(s * code) fell below the true residual
(d = 1: 0), and a row with a NaN element kept the int8 image.  Recorded, not changed: a candidate whose row id is out
of range is never offered, so it cannot be selected and raises no flag (the `sel_bad` flag of ivf_rerank_topk is never
set); with sub-lists the wave select offers keys <= T_sub and the wave lists keys < T_sub.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import _ivf_scan_cases as M

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 1024            # sentinel words before and after every output buffer the test owns
SENT = 0x7FC0BEEF       # a NaN as float, a large positive id as int: never a legitimate output here
FILL = 0xEF             # the byte a shard buffer is filled with before a launch
FILLW = 0xEFEFEFEF
PAD = M.PAD_ID


# ---- plumbing ------------------------------------------------------------------------------------------------------
class Guarded:
    """A device buffer of n 32-bit words between two sentinel-filled guard regions."""

    def __init__(self, n: int, init: np.ndarray | None = None):
        import torch

        host = np.full(n + 2 * GUARD, SENT, dtype=np.uint32)
        if init is not None:
            host[GUARD:GUARD + n] = np.ascontiguousarray(init).view(np.uint32).ravel()
        self.n = n
        self.t = torch.from_numpy(host.view(np.int32)).cuda()

    @property
    def ptr(self) -> int:
        return self.t.data_ptr() + 4 * GUARD

    def read(self) -> np.ndarray:
        a = self.t.cpu().numpy().view(np.uint32)
        assert np.all(a[:GUARD] == SENT) and np.all(a[GUARD + self.n:] == SENT), "guard region overwritten"
        return a[GUARD:GUARD + self.n].copy()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Hooks:
    def __init__(self, lib):
        p, i, l, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
        self.set_ = lib.hipann_debug_ivf_set
        self.set_.restype, self.set_.argtypes = i, [p, i, i]
        self.info_ = lib.hipann_debug_ivf_info
        self.info_.restype, self.info_.argtypes = i, [p, C.c_char_p, C.POINTER(C.c_double)]
        self.read_ = lib.hipann_debug_ivf_read
        self.read_.restype, self.read_.argtypes = l, [p, C.c_char_p, p, l, i]
        self.rerank = lib.hipann_debug_ivf_rerank
        self.rerank.restype = i
        self.rerank.argtypes = [p, p, p, i, l, i, i, i, p, p, i, p, l, l, f, p, p, p, p, f, f, p, p, p, i, p, p, i, i,
                                i, p]

    def set(self, ix, stop, seed):
        assert self.set_(ix.handle, stop, seed) == 0

    def info(self, ix, name):
        v = C.c_double()
        assert self.info_(ix.handle, name.encode(), C.byref(v)) == 0, name
        return v.value

    def read(self, ix, name, dtype, count=None):
        n = self.read_(ix.handle, name.encode(), None, 0, -1)
        assert n >= 0, name
        buf = np.zeros(n, np.uint8)
        if n:
            assert self.read_(ix.handle, name.encode(), buf.ctypes.data, n, -1) == n
        a = buf.view(dtype)
        if count is None:
            return a
        assert len(a) >= count, (name, len(a), count)
        return a[:count].copy()

    def fill(self, ix, name):
        assert self.read_(ix.handle, name.encode(), None, 0, FILL) >= 0, name


@pytest.fixture(scope="module")
def hk(gpu):
    h = Hooks(gpu.lib())
    # the hooks reject what they cannot serve
    assert h.set_(None, 1, 0) == -1 and h.read_(None, b"xs8", None, 0, -1) == -1
    return h


# mode -> (image, metric, request k): fp16 merged lists, fp16 sub-lists, int8 L2, int8 IP
MODES = {"h_sub0": (M.HALF, M.L2, 10), "h_sub1": (M.HALF, M.L2, 30), "i8_l2": (M.I8, M.L2, 10),
         "i8_ip": (M.I8, M.IP, 10)}


class Scan:
    """An IVF handle over hand-made lists whose searches stop after the scan step."""

    def __init__(self, gpu, hk, lists: M.Lists, mode, seed=0, nprobe=None, stop=1, hand=None):
        self.kind, self.metric, self.k = MODES[mode]
        self.hk, self.lists = hk, lists
        cen, off, ids, codes = hand or lists.hand()
        self.ix = gpu.HipIndexIVFFlat(cen, off, ids, codes, nprobe or lists.nlist, self.metric)
        self.ix.form = 7 if self.kind == M.I8 else 6
        if self.kind == M.HALF:
            self.ix.filter_image = self.ix.FILTER_FP16
        hk.set(self.ix, stop, seed)

    def run(self, Q, probes, k=None):
        import torch

        k = k or self.k
        nq = len(Q)
        self.dq, self.dp = _dev(Q), _dev(np.asarray(probes, np.int64))
        self.D = torch.zeros(nq * k, dtype=torch.float32, device="cuda")
        self.I = torch.zeros(nq * k, dtype=torch.int64, device="cuda")
        self.ix.search_probes_device(nq, self.dq.data_ptr(), self.dp.data_ptr(), k, self.D.data_ptr(), self.I.data_ptr())
        torch.cuda.synchronize()
        self.nq, self.np_ = nq, np.asarray(probes).shape[1]
        return self

    def info(self, name):
        return self.hk.info(self.ix, name)

    def read(self, name, dtype, count=None):
        return self.hk.read(self.ix, name, dtype, count)

    def outputs(self):
        """(part_d, part_i, qbound, slot_off) of the last run, the whole allocation of the two part buffers."""
        assert self.info("image") == self.kind and self.info("nq") == self.nq and self.info("nprobe") == self.np_
        so = self.read("slot_off", np.int32, self.nq * self.np_ + 1)
        return self.read("part_d", F), self.read("part_i", np.int32), self.read("qbound", np.uint32, self.nq), so

    def close(self):
        self.ix.close()


def _keys(kind, metric, Q, lists, es=None):
    if kind == M.I8:
        return M.keys_i8(Q, lists.rows, metric)
    return M.keys_half(Q, lists.rows, metric, es)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- images and query preparation, exact family: bit for bit ---------------------------------------------------------
def check_images_exact(s: Scan, Q, pl):
    lists, nq, d = s.lists, len(Q), Q.shape[1]
    n, npass = len(lists.rows), int(lists.tpass[-1])
    assert np.array_equal(s.read("tpass_off", np.int64, lists.nlist + 1), lists.tpass)
    if s.metric == M.L2:
        assert np.array_equal(_bits(s.read("xnorm", F, n)), _bits(M.row_norms(lists.rows)))
        assert np.array_equal(_bits(s.read("qn", F, nq)), _bits(M.row_norms(Q)))
    if s.kind == M.HALF:
        ns = int(s.info("half_nsup"))
        ok, es = M.half_es(lists.rows)
        assert ok and s.info("half_state") == 1 and s.info("half_es") == es and s.info("half_rxmax") == 0.0
        assert np.array_equal(s.read("codes_h", np.uint16, npass * ns * 1024), M.half_image(lists, ns, es).ravel())
        hs, its, r2, r1, okq = M.split_queries_h(Q, ns, es)
        assert np.array_equal(s.read("hsplit", np.uint16, hs.size), hs.ravel())
        assert np.array_equal(_bits(s.read("hits", F, nq)), _bits(its))
        assert not s.read("hres", F, 2 * nq).any()
    else:
        ns = int(s.info("i8_nsup"))
        assert s.info("i8_state") == 1
        assert np.array_equal(s.read("codes_i8", np.int8, npass * ns * 2048), M.i8_image(lists, ns, pl["xu"]).ravel())
        assert np.array_equal(_bits(s.read("xs8", F, n)), _bits(pl["xs8"])) and not s.read("xr8", F, n).any()
        qi, qs, fin, _ = M.split_queries_i8(Q, ns)
        assert fin.all() and np.array_equal(s.read("qi8", np.int8, qi.size), qi.ravel())
        assert np.array_equal(_bits(s.read("qs8", F, nq)), _bits(qs)) and not s.read("qres8", F, nq).any()
        assert np.array_equal(_bits(s.read("qhn2", F, nq)), _bits(pl["qhn2"]))
        assert np.array_equal(_bits(s.read("qhn", F, nq)), _bits(pl["qhn"]))


# ---- one scan launch -------------------------------------------------------------------------------------------------
def check_slots(s: Scan, keys, probes, out, exact_slots):
    """The slots of one launch against the model.  exact_slots: bit for bit (a single item: every bound starts at
    +inf); else the invariant of a launch whose items start under each other's bounds."""
    pd, pi, qb, so = out
    lists = s.lists
    sub = int(s.info("sub"))
    kslot = int(s.info("kslot"))
    W = M.WAVES if sub else 1
    assert kslot == W * M.K and np.array_equal(so, M.slot_prefix(lists, probes))
    # the plan: queries per list, the lists' first items and chunk-0 items, and every list's (query, probe) pairs
    nl = lists.nlist
    cnt, item_off, goff, _ = M.plan_model(lists, probes, int(s.info("group")) >> 8)
    assert np.array_equal(s.read("cnt", np.int32, nl), cnt)
    assert np.array_equal(s.read("item_off", np.int32, nl + 1), item_off)
    assert np.array_equal(s.read("goff", np.int32, nl + 1), goff)
    boff = s.read("bucket_off", np.int32, nl)
    assert np.array_equal(boff, np.concatenate([[0], np.cumsum(cnt)])[:nl])
    bucket = s.read("bucket", np.int32, s.nq * s.np_)
    pairs = np.asarray(probes).ravel()
    for l in range(nl):
        want = np.nonzero(pairs == l)[0] if lists.lens[l] else np.zeros(0, np.int64)
        assert np.array_equal(np.sort(bucket[boff[l]:boff[l] + cnt[l]]), want), l
    slots, bound = M.scan_model(keys, lists, probes, sub)
    assert np.array_equal(qb, bound), "final per-query bound"
    for (q, p, c), (kd, ki) in slots.items():
        a = (int(so[q * s.np_ + p]) + c) * kslot
        gd, gi = pd[a:a + kslot].reshape(W, M.K), pi[a:a + kslot].reshape(W, M.K)
        if exact_slots:
            assert np.array_equal(_bits(gd), _bits(kd)) and np.array_equal(gi, ki.astype(np.int32)), (q, p, c)
            continue
        for w in range(W):
            n = int(np.count_nonzero(gi[w] != PAD))
            assert np.all(gi[w][n:] == PAD) and np.all(_bits(gd[w][n:]) == 0x7F800000), (q, p, c, w)  # pads last
            nm = int(np.count_nonzero(ki[w] != PAD))
            want = dict(zip(ki[w][:nm].tolist(), _bits(kd[w][:nm]).tolist()))
            got = dict(zip(gi[w][:n].tolist(), _bits(gd[w][:n]).tolist()))
            assert len(got) == n and got.items() <= want.items(), (q, p, c, w)  # real rows of the share's 16 smallest
            pk = M.packed(gd[w][:n], gi[w][:n])
            assert np.all(pk[1:] > pk[:-1]), (q, p, c, w)  # ascending by (key, row)
            need = {r for r, k in zip(ki[w][:nm].tolist(), M.sortable(kd[w][:nm]).tolist()) if k <= int(qb[q])}
            assert need <= got.keys(), (q, p, c, w)  # nothing at or below the final bound is missing
    return int(so[-1]) * kslot


def run_scan_case(gpu, hk, name, mode, exact_slots):
    kind, metric, _ = MODES[mode]
    lists, Q, probes = M.scan_case(name, kind)
    s = Scan(gpu, hk, lists, mode)
    try:
        s.run(Q, probes)
        assert s.info("seeded") == 0 and s.info("cand_off") == -1
        es = int(s.info("half_es")) if kind == M.HALF else None
        keys, pl = _keys(kind, metric, Q, lists, es)
        check_images_exact(s, Q, pl)
        check_slots(s, keys, probes, s.outputs(), exact_slots)
        # again into sentinel-filled buffers: the same rule, and nothing written outside the slots
        for b in ("part_d", "part_i"):
            hk.fill(s.ix, b)
        s.run(Q, probes)
        out = s.outputs()
        used = check_slots(s, keys, probes, out, exact_slots)
        assert np.all(out[0][used:].view(np.uint32) == FILLW) and np.all(out[1][used:].view(np.uint32) == FILLW)
    finally:
        s.close()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", M.SINGLE_ITEM)
def test_scan_single_item(gpu, hk, name, mode):
    """One list, one chunk, at most 96 queries: images, planes and query preparation bit for bit, every sub-list bit
    for bit (keys, rows, pads, order; lists of <= 16 rows hold every (query, row) key), the bounds' bits, and for fp16
    the split residual overwritten by the one-term one (0 here)."""
    run_scan_case(gpu, hk, name, mode, True)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", M.MULTI_ITEM)
def test_scan_multi_item(gpu, hk, name, mode):
    """Several chunks, query groups and lists: an item's starting bound depends on which items finished first, so the
    slots are compared by the invariant (check_slots); the final bound is exact; a repeat obeys the same rule."""
    run_scan_case(gpu, hk, name, mode, False)


# ---- float family ----------------------------------------------------------------------------------------------------
def _two_sided(got, exact, d, what):
    """got >= exact (soundness, no tolerance) and got <= exact * 1.0001 * (1 + (d + 2) * 2^-23)."""
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    assert np.all(got >= exact), (what, float(np.max(exact - got)))
    assert np.all(got <= exact * 1.0001 * (1 + (d + 2) * 2.0 ** -23)), what


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("d", [1, 20, 100, 832])
def test_float_family(gpu, hk, d, mode):
    """Low-rank gaussian rows at scales 1e-3 .. 50: image bytes equal the numpy fp32 model; every residual plane is a
    bound of what it claims to bound, measured in fp64 from the GPU's own units and scales, and no looser than its
    own arithmetic explains; every key the scan returns lies within the certificate's E of the fp64 distance (fp16,
    int8 IP) or below the int8 L2 lower bound's limit.  List 1 is empty and nprobe = 1: the queries that probe it are
    not scanned and keep their two-term split residual."""
    kind, metric, _ = MODES[mode]
    n, nq = 333, 17
    X, Q = M.float_case(n, d, nq, 900 + d)
    X[5, d // 2] = X[5].max() if d > 1 else X[5, 0]  # (a row whose maximum appears twice)
    X[7] = Q[0]  # a row equal to a scanned query: the int8 lower-bound key falls below 0 and is clamped
    lists = M.Lists(X, np.array([0, n, n], np.int64))
    probes = (np.arange(nq, dtype=np.int64) % 2).reshape(nq, 1)
    scanned = probes[:, 0] == 0
    s = Scan(gpu, hk, lists, mode, nprobe=1)
    try:
        s.run(Q, probes)
        pd, pi, qb, so = s.outputs()
        X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
        qq, xx = (Q64 ** 2).sum(1), (X64 ** 2).sum(1)
        rel = (d + 2) * 2.0 ** -24
        if metric == M.L2:
            assert np.all(np.abs(s.read("qn", F, nq) - qq) <= rel * qq)
            assert np.all(np.abs(s.read("xnorm", F, n) - xx) <= rel * xx)
        npass = int(lists.tpass[-1])
        if kind == M.HALF:
            ns, es = int(s.info("half_nsup")), int(s.info("half_es"))
            assert M.half_es(X) == (True, es)
            img = s.read("codes_h", np.uint16, npass * ns * 1024)
            assert np.array_equal(img, M.half_image(lists, ns, es).ravel())
            xh = M.half_val(M.half_bits((X * F(2.0 ** es)).astype(F))).astype(np.float64) * 2.0 ** -es
            _two_sided(s.info("half_rxmax"), np.sqrt(((X64 - xh) ** 2).sum(1)).max(), d, "half_rxmax")
            hs, its, r2, r1, okq = M.split_queries_h(Q, ns, es)
            assert okq.all() and np.array_equal(s.read("hsplit", np.uint16, hs.size), hs.ravel())
            assert np.array_equal(_bits(s.read("hits", F, nq)), _bits(its))
            hres = s.read("hres", F, 2 * nq)
            _two_sided(hres[nq:], r1, d, "one-term split residual")
            _two_sided(hres[:nq][~scanned], r2[~scanned], d, "two-term split residual")
            assert np.array_equal(_bits(hres[:nq][scanned]), _bits(hres[nq:][scanned]))  # the scan's overwrite
            rxmax, rq = s.info("half_rxmax"), hres[nq:].astype(np.float64)
        else:
            ns = int(s.info("i8_nsup"))
            xs = M.i8_scale(X)
            xu = M.i8_units(X, xs)
            assert np.array_equal(s.read("codes_i8", np.int8, npass * ns * 2048), M.i8_image(lists, ns, xu).ravel())
            gxs = s.read("xs8", F, n)
            assert np.array_equal(_bits(gxs), _bits(xs)) and np.abs(xu).max() == 127
            xr8 = s.read("xr8", F, n)
            xhat = gxs.astype(np.float64)[:, None] * xu
            _two_sided(xr8, np.sqrt(((X64 - xhat) ** 2).sum(1)), d, "xr8")
            qi, qs, fin, qu = M.split_queries_i8(Q, ns)
            assert np.array_equal(s.read("qi8", np.int8, qi.size), qi.ravel())
            gqs = s.read("qs8", F, nq)
            assert np.array_equal(_bits(gqs), _bits(qs))
            qhat = gqs.astype(np.float64)[:, None] * qu
            qres8 = s.read("qres8", F, nq)
            _two_sided(qres8, np.sqrt(((Q64 - qhat) ** 2).sum(1)), d, "qres8")
            _two_sided(s.read("qhn", F, nq), np.sqrt((qhat ** 2).sum(1)), d, "qhn")
            assert np.all(np.abs(s.read("qhn2", F, nq) - (qhat ** 2).sum(1)) <= rel * (qhat ** 2).sum(1))
            rxmax, rq = float(xr8.max()), qres8.astype(np.float64)
        # every returned entry's key
        kslot = int(s.info("kslot"))
        worst, seen = 0.0, 0
        for q in np.nonzero(scanned)[0]:
            a = int(so[q]) * kslot
            gd, gi = pd[a:a + kslot], pi[a:a + kslot]
            real = gi != PAD
            assert np.all((gi[real] >= 0) & (gi[real] < n)) and np.all(np.isinf(gd[~real]))
            rows, key = gi[real], gd[real].astype(np.float64)
            seen += len(rows)
            if metric == M.L2:
                assert np.all(gd[real].view(np.uint32) < 0x7F800000), (q, "a negative or non-finite L2 key")
                if q == 0 and mode == "i8_l2" and d > 1:
                    assert gd[real][rows == 7].view(np.uint32).tolist() == [0], "the clamp at 0"
            fp = (d + 8) * 2.0 ** -24 * 2.0 * (qq[q] + xx.max())
            if mode == "i8_l2":
                lim = ((qhat[q] - X64[rows]) ** 2).sum(1) + fp
                assert np.all(key <= lim), (q, float(np.max(key - lim)))
                worst = max(worst, float(np.max((key - ((qhat[q] - X64[rows]) ** 2).sum(1)) / fp)))
            else:
                exact = ((Q64[q] - X64[rows]) ** 2).sum(1) if metric == M.L2 else -(X64[rows] @ Q64[q])
                E = M.cert_E("cs", metric, d, qq[q], xx.max(), rxmax=rxmax, rq=rq[q], have_qres=True)
                worst = max(worst, float(np.max(np.abs(key - exact)) / E))
                assert np.all(np.abs(key - exact) <= E), (q, worst)
        assert seen >= min(n, 16) * int(scanned.sum())
        print(f"ivf_scan_ratio mode={mode} d={d} max|key-exact|/E={worst:.4f} entries={seen}")
    finally:
        s.close()


# ---- non-finite inputs -------------------------------------------------------------------------------------------------
NEG_NAN = np.array([0xFFC00000], np.uint32).view(F)[0]
BAD = {"pinf": F(np.inf), "ninf": F(-np.inf), "nan": F(np.nan), "neg_nan": NEG_NAN}


@pytest.mark.parametrize("what", sorted(BAD) + ["all_nan"])
def test_nonfinite_row_refuses_the_images(gpu, hk, what):
    """A row holding one +-inf, +NaN or -NaN (sign bit set) among finite elements, or all NaN: the int8 image is
    refused (its builder reports the row), so is the fp16 image, and the search takes form 5 — and answers the
    finite queries as the direct form does."""
    X, Q = M.float_case(200, 20, 17, 77)
    if what == "all_nan":
        X[70] = np.nan
    else:
        X[70, 3] = BAD[what]
    lists = M.Lists(X, np.array([0, 120, 200], np.int64))
    probes = np.tile(np.arange(2, dtype=np.int64), (17, 1))
    for mode in ("i8_l2", "i8_ip", "h_sub0"):
        s = Scan(gpu, hk, lists, mode, stop=0)
        try:
            s.run(Q, probes)
            assert s.ix.last_search_path()["form"] == 5, (mode, s.ix.last_search_path())
            if mode == "h_sub0":
                assert s.info("half_state") == -1
            else:
                assert s.info("i8_state") == -1 and len(s.read("codes_i8", np.int8)) == 0
            D = s.D.cpu().numpy().reshape(17, -1)
            I = s.I.cpu().numpy().reshape(17, -1)
            for q in range(17):
                dist = M.direct_dist(Q[q], X, MODES[mode][1]).astype(np.float64)
                kth = np.sort(np.delete(dist, 70))[9]
                got = I[q][(I[q] != 70) & (I[q] >= 0)]
                assert len(got) >= 9 and np.all(dist[got] <= kth + 1e-5 * abs(kth) + 1e-6), (mode, q)
        finally:
            s.close()


@pytest.mark.parametrize("mode", ["i8_l2", "h_sub0"])
def test_nonfinite_query_residual_is_inf(gpu, hk, mode):
    """Queries holding +-inf, +NaN, -NaN among finite elements: their split residual is +inf (the rerank re-runs
    them), the others' are finite."""
    X, Q = M.float_case(100, 20, 8, 78)
    for j, v in enumerate(BAD.values()):
        Q[2 * j, 5] = v
    lists = M.Lists(X, np.array([0, 100], np.int64))
    s = Scan(gpu, hk, lists, mode)
    try:
        s.run(Q, np.zeros((8, 1), np.int64))
        res = s.read("qres8", F, 8) if mode == "i8_l2" else s.read("hres", F, 16)
        bad = np.arange(8) % 2 == 0
        assert np.all(res[:8][bad] == np.inf) and np.all(np.isfinite(res[:8][~bad]))
        if mode == "h_sub0":
            assert np.all(res[8:][bad] == np.inf)
    finally:
        s.close()


# ---- the incremental re-tile -------------------------------------------------------------------------------------------
def _image_state(s: Scan, d):
    off = s.read("list_off", np.int64, s.lists.nlist + 1)
    ln = s.read("list_len", np.int32, s.lists.nlist)
    tp = s.read("tpass_off", np.int64, s.lists.nlist + 1)
    if s.kind == M.I8:
        per = int(s.info("i8_nsup")) * 2048
        img = s.read("codes_i8", np.int8, int(tp[-1]) * per).reshape(-1, per)
        planes = [s.read("xs8", F, int(off[-1])), s.read("xr8", F, int(off[-1]))]
    else:
        per = int(s.info("half_nsup")) * 1024
        img = s.read("codes_h", np.uint16, int(tp[-1]) * per).reshape(-1, per)
        planes = []
    return off, ln, tp, img, planes


@pytest.mark.parametrize("mode", ["i8_l2", "h_sub0"])
def test_retile_after_add_and_remove(gpu, hk, mode):
    """After an add and after a remove the touched passes are re-tiled in place (pass_ids): every list's image passes
    and planes equal, bit for bit, a fresh build over the same lists; passes and rows past a list's live length are
    zero units, scale 0, residual 0."""
    d = 20
    X, Q = M.float_case(143 + 60, d, 5, 79)
    lists = M.Lists(X[:143], np.array([0, 40, 110, 143], np.int64))
    cen = np.stack([X[0:40].mean(0), X[40:110].mean(0), X[110:143].mean(0)]).astype(F)
    probes = np.tile(np.arange(3, dtype=np.int64), (5, 1))

    def build(cen, off, ids, codes):
        return Scan(gpu, hk, M.Lists(codes, off), mode, hand=(cen, off, ids, codes))

    a = build(cen, lists.off, np.arange(143, dtype=np.int64), lists.rows)
    try:
        a.run(Q, probes)  # builds the image
        steps = [lambda: a.ix.add(X[143:], np.arange(143, 203, dtype=np.int64)),
                 lambda: a.ix.remove_ids(np.arange(30, 90, 2, dtype=np.int64))]
        for step in steps:
            step()
            a.run(Q, probes)
            ex = a.ix.export()
            b = build(ex["centroids"], ex["list_offsets"], ex["ids"], ex["codes"])
            try:
                b.run(Q, probes)
                oa, la, ta, ia, pa = _image_state(a, d)
                ob, lb, tb, ib, pb = _image_state(b, d)
                assert np.array_equal(la, lb) and np.array_equal(la, np.diff(ex["list_offsets"]))
                for l in range(3):
                    npl = -(-int(la[l]) // 32)
                    assert np.array_equal(ia[ta[l]:ta[l] + npl], ib[tb[l]:tb[l] + npl]), (l, "image passes")
                    assert not ia[ta[l] + npl:ta[l + 1]].any(), (l, "slack passes")
                    for x, y in zip(pa, pb):
                        assert np.array_equal(_bits(x[oa[l]:oa[l] + la[l]]), _bits(y[ob[l]:ob[l] + la[l]])), (l, "planes")
                        assert not x[oa[l] + la[l]:oa[l + 1]].any(), (l, "slack rows")
                if mode == "h_sub0":
                    assert a.info("half_es") == b.info("half_es") and a.info("half_rxmax") >= b.info("half_rxmax")
            finally:
                b.close()
    finally:
        a.close()


# ---- the seeded two launches -------------------------------------------------------------------------------------------
def seed_none_case():
    """One list of 2048 + 300 rows whose second chunk lies far from every query: every row and query has its
    127 * 2^e at dim 0, the second chunk's rows -127 * 2^2 there, so the second launch appends nothing for any query
    (exact-family inputs: keys below 2^24 units of 2^-4)."""
    rng = np.random.default_rng(31)

    def make(m):
        v = rng.integers(-1, 2, (m, 20)) * (rng.random((m, 20)) < 1 / 3)
        v[:, 0] = 127
        return (v * 2.0 ** rng.integers(-2, 3, m)[:, None]).astype(F)

    X, Q = make(2348), make(17)
    X[2048:] = 0
    X[2048:, 0] = -508.0
    return M.Lists(np.ascontiguousarray(X), np.array([0, 2348], np.int64)), Q, np.zeros((17, 1), np.int64)


def seed_ties_case():
    """One list of 2100 identical rows: every key of a query is equal, so the seed list's 64th key — the bound of the
    second launch — ties with every row of the second chunk, which must be admitted at `<=`."""
    X, Q = M.exact_i8(1, 20, 17, 32)
    X = np.ascontiguousarray(np.repeat(X, 2100, axis=0))
    return M.Lists(X, np.array([0, 2100], np.int64)), Q, np.zeros((17, 1), np.int64)


@pytest.mark.parametrize("name", ["chunk2049_d64", "lists_d64", "groups100_chunks_d100", "seed_none", "seed_ties"])
def test_seeded_two_launches(gpu, hk, name):
    """int8 L2, lists of two and more chunks, the seeded path forced on: the chunk-0 slots obey the scan's invariant;
    after ivf_seed_bound the last 64 entries of a query's seed slot are the 64 smallest chunk-0 entries at or below
    its bound (pads when fewer; the bound min'ed only with a real 64th); run_cnt starts from zero and counts exactly
    the entries the second launch appended, each a real row of its share's 16 smallest with the model's key bits and
    none at or below the final bound missing; nothing is written past them; the final bound is the single launch's."""
    lists, Q, probes = (seed_none_case() if name == "seed_none" else seed_ties_case() if name == "seed_ties"
                        else M.scan_case(name, M.I8))
    keys, _ = M.keys_i8(Q, lists.rows, M.L2)
    nq, npr = probes.shape
    s = Scan(gpu, hk, lists, "i8_l2", seed=1)
    try:
        s.run(Q, probes)
        assert s.info("seeded") == 1 and s.ix.last_search_path(seeded=True)["seeded"] == 1
        for b in ("part_d", "part_i", "run_cnt"):
            hk.fill(s.ix, b)
        s.run(Q, probes)
        pd, pi, qb, so = s.outputs()
        kslot, co = int(s.info("kslot")), int(s.info("cand_off"))
        assert kslot == 128 and co == npr * nq * kslot and np.array_equal(so, M.slot_prefix(lists, probes))
        slots, bound = M.scan_model(keys, lists, probes, True)
        run_cnt = s.read("run_cnt", np.int32, nq)
        b1 = np.full(nq, M.QB_INF, np.uint32)  # the bound after the chunk-0 items
        for (q, p, c), (kd, ki) in slots.items():
            if c == 0:
                full = ki[:, M.K - 1] != PAD
                if full.any():
                    b1[q] = min(b1[q], M.sortable(kd[full, M.K - 1]).min())
        sd, si, b2 = M.seed_model(keys, lists, probes, b1)
        # the bound word also takes the seed list's 64th key; the rerank's bound B — the smaller of the 64th
        # candidate key and T_sub — is the single launch's (checked per query below)
        assert np.array_equal(qb, np.minimum(bound, b2)), "final per-query bound"
        used = np.zeros(len(pd), bool)
        appended_any = must_append = False
        for q in range(nq):
            # chunk-0 slots: one per pair, at the head of the buffers
            for p in range(npr):
                a = (q * npr + p) * kslot
                if (q, p, 0) not in slots:
                    continue  # an empty list: no item wrote the pair's slot
                used[a:a + kslot] = True
                kd, ki = slots[(q, p, 0)]
                gd, gi = pd[a:a + kslot].reshape(8, 16), pi[a:a + kslot].reshape(8, 16)
                for w in range(8):
                    n = int(np.count_nonzero(gi[w] != PAD))
                    assert np.all(gi[w][n:] == PAD) and np.all(_bits(gd[w][n:]) == 0x7F800000)
                    nm = int(np.count_nonzero(ki[w] != PAD))
                    want = dict(zip(ki[w][:nm].tolist(), _bits(kd[w][:nm]).tolist()))
                    got = dict(zip(gi[w][:n].tolist(), _bits(gd[w][:n]).tolist()))
                    assert len(got) == n and got.items() <= want.items()
                    need = {r for r, k in zip(ki[w][:nm].tolist(), M.sortable(kd[w][:nm]).tolist()) if k <= int(b1[q])}
                    assert need <= got.keys(), (q, p, w)
            # the seed list
            a = co + (int(so[q * npr]) + q + 1) * kslot - M.SEED_K
            used[a:a + M.SEED_K] = True
            gd, gi = pd[a:a + M.SEED_K], pi[a:a + M.SEED_K]
            n = int(np.count_nonzero(si[q] != PAD))
            assert np.array_equal(_bits(gd), _bits(sd[q])), (q, "seed keys")
            assert np.all(gi[n:] == PAD)
            last = _bits(sd[q][n - 1:n])
            lt = _bits(sd[q][:n]) != (last[0] if n else 0)
            assert np.array_equal(gi[:n][lt], si[q][:n][lt].astype(np.int32)), (q, "seed rows below the last key")
            pool = {int(r) for (qq, p, c), (kd, ki) in slots.items() if qq == q and c == 0
                    for r, k in zip(ki.ravel(), _bits(kd.ravel())) if n and k == last[0] and r != PAD}
            assert set(gi[:n][~lt].tolist()) <= pool and len(set(gi[:n].tolist())) == n, (q, "seed rows at the last key")
            # the appended run
            cnt = int(run_cnt[q])
            cap = sum(max(int(-(-lists.lens[l] // M.CH)) - 1, 0) for l in probes[q]) * kslot
            assert 0 <= cnt <= cap, (q, cnt)
            appended_any |= cnt > 0
            r0 = a + M.SEED_K
            used[r0:r0 + cnt] = True
            got = dict(zip(pi[r0:r0 + cnt].tolist(), _bits(pd[r0:r0 + cnt]).tolist()))
            assert len(got) == cnt, (q, "a row appended twice")
            want, need = {}, set()
            for (qq, p, c), (kd, ki) in slots.items():
                if qq == q and c >= 1:
                    m = ki.ravel() != PAD
                    want.update(zip(ki.ravel()[m].tolist(), _bits(kd.ravel()[m]).tolist()))
                    need |= {r for r, k in zip(ki.ravel()[m].tolist(), M.sortable(kd.ravel()[m]).tolist()) if k <= int(qb[q])}
            assert got.items() <= want.items() and need <= got.keys(), q
            must_append |= bool(need)
            # B of the rerank: this run under T_sub = qb[q] against the single launch's slots under its own bound
            def rerank_bound(kbits, t):
                kb = np.sort(kbits[kbits <= t])
                return min(int(kb[M.SEED_K - 1]) if len(kb) >= M.SEED_K else M.QB_INF, int(t))
            mine = M.sortable(pd[a:r0 + cnt][pi[a:r0 + cnt] != PAD])
            single = np.concatenate([M.sortable(kd.ravel()[ki.ravel() != PAD])
                                     for (qq, p, c), (kd, ki) in slots.items() if qq == q])
            assert rerank_bound(mine, qb[q]) == rerank_bound(single, bound[q]), (q, "the rerank's bound B")
        # (an entry between a query's final bound and the bound its item started under may or may not be appended)
        assert appended_any or not must_append
        assert (must_append or name not in ("lists_d64", "seed_ties")) and not (name == "seed_none" and appended_any)
        assert np.all(pd[~used].view(np.uint32) == FILLW) and np.all(pi[~used].view(np.uint32) == FILLW)
    finally:
        s.close()


def test_seed_override_off_and_hooks_leave_search_alone(gpu, hk):
    """Override off: the single launch on a shape the seeded path would take.  And with the stop cleared the handle
    searches as a fresh one does."""
    lists, Q, probes = M.scan_case("chunk2049_d64", M.I8)
    s = Scan(gpu, hk, lists, "i8_l2", seed=0)
    ref = Scan(gpu, hk, lists, "i8_l2", seed=-1, stop=0)
    try:
        s.run(Q, probes)
        assert s.info("seeded") == 0
        hk.set(s.ix, 0, -1)
        s.run(Q, probes)
        ref.run(Q, probes)
        assert np.array_equal(s.D.cpu().numpy().view(np.uint32), ref.D.cpu().numpy().view(np.uint32))
        assert np.array_equal(s.I.cpu().numpy(), ref.I.cpu().numpy())
    finally:
        s.close()
        ref.close()


# ---- ivf_rerank_topk alone ---------------------------------------------------------------------------------------------
class Table:
    """A small integer table (exact direct-form distances) in three lists, with scattered labels."""

    def __init__(self, d=8, nrows=200, seed=11):
        rng = np.random.default_rng(seed)
        self.codes = rng.integers(-4, 5, (nrows, d)).astype(F)
        self.ids = rng.permutation(nrows).astype(np.int64) * 3 + 1
        self.list_off = np.array([0, 70, 130, nrows], np.int64)
        self.nrows, self.d = nrows, d
        self.dcodes, self.dids, self.dloff = _dev(self.codes), _dev(self.ids), _dev(self.list_off)


@pytest.fixture(scope="module")
def table():
    return Table()


def rerank(hk, tb: Table, runs, Q, k, kout, metric=M.L2, *, use_ids=True, label_offset=0, xmax2=0.0, cert="eps",
           eps=0.0, rxmax=-1.0, qres=None, qnorm=None, qbound=None, sub=0, probes=None, seed_layout=None, rc=0,
           f32=False):
    """Run hipann_debug_ivf_rerank over per-query candidate runs [(keys, rows)] and compare D, I, the flags and their
    bookkeeping with the model.  The runs are laid out with one slot entry per candidate (kslot = 1, nprobe = 1), or
    nprobe slots of equal size when probes are given (the tie rule reads the probe ranks), or as seeded candidate
    runs (seed_layout = kslot: the run's first 64 entries end the query's first slot)."""
    nq = len(runs)
    seed_cnt = None
    if seed_layout:
        kslot, npr = seed_layout, 1
        slots = np.array([2 + (len(r[0]) - 64 + kslot - 1) // kslot for r in runs])
        so = np.concatenate([[0], np.cumsum(slots)]).astype(np.int32)
        pd = np.full((int(so[-1]) + nq + 1) * kslot, np.nan, F)
        pi = np.full(len(pd), 5, np.int32)  # stale memory: NaN keys on a valid row
        for q, (kd, ki) in enumerate(runs):
            a = (int(so[q]) + q + 1) * kslot - 64
            pd[a:a + len(kd)], pi[a:a + len(kd)] = kd, ki
        seed_cnt = np.array([len(r[0]) - 64 for r in runs], np.int32)
    elif probes is not None:
        npr = probes.shape[1]
        kslot = len(runs[0][0]) // npr
        assert all(len(r[0]) == kslot * npr for r in runs)
        so = None
        pd = np.concatenate([r[0] for r in runs]).astype(F)
        pi = np.concatenate([r[1] for r in runs]).astype(np.int32)
    else:
        kslot, npr = 1, 1
        so = np.concatenate([[0], np.cumsum([len(r[0]) for r in runs])]).astype(np.int32)
        pd = np.concatenate([np.asarray(r[0], F) for r in runs] + [np.zeros(1, F)])
        pi = np.concatenate([np.asarray(r[1], np.int32) for r in runs] + [np.zeros(1, np.int32)])
    dpd, dpi, dq = _dev(pd), _dev(pi), _dev(np.ascontiguousarray(Q, F))
    dso = _dev(so) if so is not None else None
    dqres = _dev(np.asarray(qres, F)) if qres is not None else None
    dqn = _dev(np.asarray(qnorm, F)) if qnorm is not None else None
    dqb = _dev(np.asarray(qbound, np.uint32)) if qbound is not None else None
    dpr = _dev(np.asarray(probes, np.int64)) if probes is not None else None
    dsc = _dev(seed_cnt) if seed_cnt is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    D, I = Guarded(nq * kout), Guarded(2 * nq * kout)
    nflag, flagged = Guarded(1), Guarded(nq)
    got = hk.rerank(ptr(dpd), ptr(dpi), ptr(dso), npr, nq, k, kout, metric, ptr(dq), ptr(tb.dcodes), tb.d,
                    ptr(tb.dids) if use_ids else None, tb.nrows, label_offset, xmax2, D.ptr, I.ptr, nflag.ptr,
                    flagged.ptr, eps, rxmax, ptr(dqres), ptr(dpr), ptr(tb.dloff) if probes is not None else None,
                    3 if probes is not None else 0, ptr(dqb), ptr(dqn), kslot, sub, 1 if cert == "i8_l2" else 0,
                    ptr(dsc))
    assert got == rc
    if rc:
        return None
    gD = D.read().view(F).reshape(nq, kout)
    gI = I.read().view(np.int64).reshape(nq, kout)
    nf = int(nflag.read().view(np.int32)[0])
    fl = flagged.read().view(np.int32)
    assert 0 <= nf <= nq and np.all(fl[nf:].view(np.uint32) == SENT)
    assert len(set(fl[:nf].tolist())) == nf, "a query listed twice"
    want_flag, infos = [], []
    for q in range(nq):
        wD, wI, wf, info = M.rerank_model(
            runs[q][0], runs[q][1], k, kout, metric, Q[q], tb.codes, tb.nrows, tb.ids if use_ids else None,
            label_offset, xmax2, cert, eps, rxmax, None if qres is None else qres[q],
            None if qnorm is None else qnorm[q], None if qbound is None else qbound[q], sub,
            None if probes is None else probes[q], tb.list_off, f32)
        assert np.array_equal(_bits(gD[q]), _bits(wD)), (q, gD[q], wD, info)
        assert np.array_equal(gI[q], wI), (q, gI[q], wI, info)
        if wf:
            want_flag.append(q)
        infos.append(info)
    assert sorted(fl[:nf].tolist()) == want_flag, (sorted(fl[:nf].tolist()), want_flag)
    return set(want_flag), infos


def _run_of(rng, total, nrows, lo=1.0):
    """A run of `total` distinct keys with everything a run may hold besides candidates."""
    kd = (lo + rng.permutation(total) * 0.25).astype(F)
    ki = rng.integers(0, nrows, total).astype(np.int32)
    for j, (key, row) in enumerate(((np.inf, PAD), (np.inf, 3), (0.5, -1), (0.5, nrows), (0.25, nrows + 7),
                                    (np.nan, 4), (0.125, -(2 ** 31)))):
        if total > 40:
            pos = (j * 37 + 5) % total
            kd[pos], ki[pos] = key, row
    return kd, ki


@pytest.mark.parametrize("metric", [M.L2, M.IP])
@pytest.mark.parametrize("k,kout", [(16, 10), (64, 30), (20, 20)])
def test_rerank_selection_and_output(hk, table, k, kout, metric):
    """Totals of 0, 1, k - 1, k, a few hundred, 4096 (the wave select's last) and 4097, 6000 (the wave lists), with
    pads, +inf and NaN keys, rows < 0 and >= nrows under small keys (never offered: no flag, no output), key ties at
    the k-th key (broken as modelled), labels through ids and through label_offset, L2 and IP signs, (-1, +-inf) pads."""
    rng = np.random.default_rng(100 * k + metric)
    totals = [0, 1, k - 1, k, 300, 700, 4096, 4097, 6000, 512, 5000]
    runs = [_run_of(rng, t, table.nrows) for t in totals]
    for j in (-2, -1):  # ties across the k-th key: 3k entries share one key, rows in descending order
        kd, ki = runs[j]
        kd[40:40 + 3 * k] = 0.75
        ki[40:40 + 3 * k] = np.arange(3 * k, 0, -1)
    Q = rng.integers(-3, 4, (len(runs), table.d)).astype(F)
    for use_ids, lo in ((True, 0), (False, 1000)):
        rerank(hk, table, runs, Q, k, kout, metric, use_ids=use_ids, label_offset=lo, eps=0.0)


def test_rerank_tsub_and_seed_runs(hk, table):
    """Sub-lists: keys >= T_sub are not offered (the wave lists; the wave select offers the key equal to it), and
    the seeded layout reads exactly 64 + seed_cnt[q] entries from the end of the query's first slot."""
    rng = np.random.default_rng(7)
    k, kout = 64, 10
    runs, qb = [], []
    totals = (200, 4096, 4500, 6000)
    Q = rng.integers(-3, 4, (len(totals), table.d)).astype(F)
    for q, total in enumerate(totals):
        kd, ki = _run_of(rng, total, table.nrows)
        t = F(np.sort(kd[np.isfinite(kd)])[30])  # a key of the run: fewer than k candidates lie below it
        ki[np.nonzero(kd == t)[0][0]] = 20 + q   # ... and the entry at it is the query's own row (distance 0)
        Q[q] = table.codes[20 + q]
        runs.append((kd, ki))
        qb.append(M.sortable(np.array([t], F))[0])
    flagged, infos = rerank(hk, table, runs, Q, k, kout, eps=0.0, qbound=np.array(qb, np.uint32), sub=1)
    assert all(i["ncand"] < k and i["keys"].max() <= i["tsub"] for i in infos)
    at = [bool((i["keys"] == i["tsub"]).any()) for i in infos]
    assert at == [True, True, False, False]  # offered by the wave select (<= T_sub), not by the wave lists (<)
    # seeded runs: 64 + n entries, n = 0, 1, 130, 5000
    runs = [_run_of(rng, 64 + n, table.nrows) for n in (0, 1, 130, 5000)]
    rerank(hk, table, runs, Q, k, kout, eps=0.0, qbound=np.full(4, M.QB_INF, np.uint32), sub=1, seed_layout=128)
    # the launcher refuses candidate runs without the slot table's companions, and a depth outside 16 .. 64
    assert hk.rerank(None, None, None, 1, 1, 16, 10, 0, None, None, 8, None, 10, 0, 0.0, None, None, None, None, 0.0,
                     -1.0, None, None, None, 0, None, None, 1, 0, 0, None) == -1
    rerank(hk, table, runs[:1], Q[:1], 8, 4, rc=-1)
    rerank(hk, table, runs[:1], Q[:1], 16, 17, rc=-1)
    rerank(hk, table, runs[:1], Q[:1], 16, 10, sub=1, rc=-1)  # sub-lists without the bound


def test_rerank_tie_rule(hk, table):
    """More rows tied at the kout-th distance than slots remain, spread over probe ranks and list positions:
    membership follows FAISS's scan order (probe rank, then row), the output is ordered by (distance, label)."""
    tb = Table(seed=12)
    q = np.zeros(tb.d, F)
    codes = tb.codes.copy()
    tied = [5, 60, 69, 75, 100, 129, 140, 150, 199]  # rows of all three lists at distance 9
    for r in tied:
        codes[r] = 0
        codes[r, r % tb.d] = 3 if r % 2 else -3
    for r in (80, 170):  # two below the tie
        codes[r] = 0
        codes[r, 0] = 1
    far = [r for r in range(tb.nrows) if r not in tied + [80, 170]]
    codes[far] = 4  # everything else is far
    tb.codes, tb.dcodes = codes, _dev(codes)
    runs, probes = [], []
    for perm in ([2, 0, 1], [0, 1, 2], [1, 2, 0]):
        rows = np.array(tied + [80, 170] + far[:9], np.int32)
        rng = np.random.default_rng(perm[0])
        rows = rows[rng.permutation(len(rows))]
        kd = np.arange(1, len(rows) + 1, dtype=F)
        pad = 21 - len(rows)  # three slots of seven entries
        runs.append((np.concatenate([kd, np.full(pad, np.inf, F)]), np.concatenate([rows, np.full(pad, PAD, np.int32)])))
        probes.append(perm)
    Q = np.stack([q] * 3)
    for kout in (4, 5, 8):
        _, infos = rerank(hk, tb, runs, Q, 32, kout, eps=0.0, probes=np.array(probes, np.int64))
        assert all(i["ncand"] == 20 for i in infos)


CERTS = {
    # name: (cert, metric, with qres, sub)
    "eps_kk": ("eps", M.L2, False, 0), "eps_tsub": ("eps", M.L2, False, 1),
    "cs_qres_kk": ("cs", M.L2, True, 0), "cs_qres_tsub": ("cs", M.L2, True, 1), "cs_qres_ip": ("cs", M.IP, True, 0),
    "cs_accum": ("cs", M.L2, True, 0), "cs_noqres_kk": ("cs", M.L2, False, 0),
    "i8_kk": ("i8_l2", M.L2, True, 0), "i8_tsub": ("i8_l2", M.L2, True, 1),
}


@pytest.mark.parametrize("name", sorted(CERTS))
def test_rerank_decision(hk, table, name):
    """Pairs of queries identical except the bound B (the k-th key, or T_sub), set to the certificate's threshold
    +- 2^-9 of E: the lower one must be flagged, the upper one must not.  2^-9 lies above the fp32 evaluation error
    of E (a dozen roundings, below 2^-20) and below the formula's own 1 % factor, so a dropped 1.01, d for 2d, a
    missing term or a missing clause flips a pair.  E is evaluated in fp64 from the header's formula; xmax2 and the
    residuals are inputs chosen so that E is within a factor of 8 of the kout-th distance."""
    cert, metric, with_qres, sub = CERTS[name]
    k, kout, nq = 16, 10, 12
    rng = np.random.default_rng(sorted(CERTS).index(name))
    Q = rng.integers(-3, 4, (nq, table.d)).astype(F)
    Q[:, 0] = 3
    if name == "cs_noqres_kk":
        Q[:, 1] = F(1 + 2.0 ** -9)  # not a bf16 value: the kernel's own query residual is 2^-9
    Q[1::2] = Q[0::2]  # pairs
    n = k if not sub else kout + 2
    rows = [((np.arange(n) * 7 + 5 * (q // 2)) % table.nrows).astype(np.int32) for q in range(nq)]
    dk = np.array([np.sort(M.direct_dist(Q[q], table.codes[rows[q]], metric).astype(np.float64))[kout - 1] for q in range(nq)])
    qq = (Q.astype(np.float64) ** 2).sum(1)
    qres = qnorm = None
    eps, rxmax, xmax2 = 0.0, -1.0, 400.0
    if cert == "eps":
        eps, xmax2 = 2.0 ** -12, 2.0e5
    elif name == "cs_accum":  # no residuals: E is the fp32 accumulation of 2d products and the rounding term
        rxmax, qres, qnorm, xmax2 = 0.0, np.zeros(nq, F), np.full(nq, 2.5e7, F), 2.5e7
    elif cert == "cs":
        rxmax = 2.0 if metric == M.L2 else 4.0
        if with_qres:
            qres, qnorm = np.full(nq, 0.5, F), qq.astype(F)
    else:
        qres, qnorm, xmax2 = np.full(nq, 1.5, F), qq.astype(F), 1.6e7
    B = np.zeros(nq)
    for q in range(nq):
        rq = float(qres[q]) if qres is not None else float(np.sqrt(np.sum(
            (Q[q].astype(np.float64) - M.bf16_round(Q[q])) ** 2)))
        E = M.cert_E(cert, metric, table.d, float(qnorm[q]) if qnorm is not None else qq[q], xmax2, eps,
                     max(rxmax, 0.0), rq, qres is not None)
        assert abs(dk[q]) / 8 <= E <= 8 * max(abs(dk[q]), 16.0), (name, q, dk[q], E)  # (IP: d_k may be near 0)
        thr = dk[q] if cert != "i8_l2" else ((np.sqrt(dk[q]) + rq) * (1 + 2.0 ** -20)) ** 2 / (1 - 2.0 ** -20)
        B[q] = thr + E * (1 + (2.0 ** -9 if q % 2 else -2.0 ** -9))
    runs = []
    for q in range(nq):
        lo = min(dk[q], 0.0) - 50.0  # keys below the bound (IP: distances are negative)
        kd = (lo + (B[q] - lo) * np.arange(n) / n).astype(F)
        if not sub:
            kd[-1] = F(B[q])
        runs.append((kd, rows[q]))
    qb = M.sortable(B.astype(F)) if sub else None
    flagged, infos = rerank(hk, table, runs, Q, k, kout, metric, xmax2=xmax2, cert=cert, eps=eps, rxmax=rxmax, qres=qres,
                            qnorm=qnorm, qbound=qb, sub=sub)
    assert flagged == set(range(0, nq, 2)), (name, flagged)


def test_rerank_decision_at_the_threshold(hk, table):
    """The comparisons themselves.  eps: E and B are exact and B - E == d_k: `d_k < B - E` is false, the query is
    flagged, and one ulp more of B certifies it.  i8_l2: the kernel's own fp32 expression, step for step, finds the
    smallest certifying B; that B certifies on the GPU and the float below it does not (the (1 +- 2^-20) factors move
    the threshold by some fifty ulps)."""
    k, kout = 16, 10
    rng = np.random.default_rng(3)
    Q = rng.integers(-3, 4, (8, table.d)).astype(F)
    Q[1::2] = Q[0::2]
    rows = [((np.arange(k) * 7 + 5 * (q // 2)) % table.nrows).astype(np.int32) for q in range(8)]
    dk = [float(np.sort(M.direct_dist(Q[q], table.codes[rows[q]], M.L2))[kout - 1]) for q in range(8)]
    qq = (Q.astype(np.float64) ** 2).sum(1)

    def runs_for(B):
        out = []
        for q in range(8):
            kd = (np.arange(k) * 0.01).astype(F)
            kd[-1] = B[q]
            out.append((kd, rows[q]))
        return out

    # eps = 2^-12 and ||q||^2 + xmax2 = 2^16: E = 16
    assert len(set(qq)) >= 1
    for q0 in range(0, 8, 2):
        xmax2 = 65536.0 - qq[q0]
        B = np.array([F(dk[q]) + F(16) if q % 2 == 0 else np.nextafter(F(dk[q]) + F(16), F(np.inf)) for q in range(8)], F)
        flagged, _ = rerank(hk, table, runs_for(B), Q, k, kout, xmax2=xmax2, eps=2.0 ** -12, f32=True)
        assert (q0 in flagged) and (q0 + 1 not in flagged), (q0, flagged)
    # i8_l2: bisect the kernel's fp32 expression for the smallest certifying B
    qres, qnorm, xmax2 = np.full(8, 1.5, F), qq.astype(F), 1.6e7
    B = np.zeros(8, F)
    for q in range(8):
        E = M.cert_E_f32("i8_l2", M.L2, table.d, qnorm[q], xmax2)
        lo, hi = F(dk[q]), F(dk[q] * 4 + 100)
        assert not M.clears("i8_l2", dk[q], lo, E, 1.5, True) and M.clears("i8_l2", dk[q], hi, E, 1.5, True)
        while np.nextafter(lo, F(np.inf)) < hi:
            mid = F((np.float64(lo) + np.float64(hi)) / 2)
            if M.clears("i8_l2", dk[q], mid, E, 1.5, True):
                hi = mid
            else:
                lo = mid
        B[q] = lo if q % 2 == 0 else hi
    flagged, _ = rerank(hk, table, runs_for(B), Q, k, kout, xmax2=xmax2, cert="i8_l2", qres=qres, qnorm=qnorm, f32=True)
    assert flagged == {0, 2, 4, 6}, flagged


def test_rerank_never_and_always_flagged(hk, table):
    """Fewer candidates than k are never flagged on K_k (whatever E), no candidate at all is never flagged (even
    with a non-finite bound), a non-finite residual or E with candidates always is; fewer candidates than kout pad
    the output with (-1, +-inf)."""
    rng = np.random.default_rng(9)
    k, kout = 16, 10
    Q = rng.integers(-3, 4, (4, table.d)).astype(F)
    mk = lambda n: ((np.arange(n) + 1).astype(F), ((np.arange(n) * 11) % table.nrows).astype(np.int32))
    runs = [mk(15), mk(5), mk(0), (np.full(20, np.inf, F), np.full(20, PAD, np.int32))]
    qn = (Q ** 2).sum(1).astype(F)
    for metric in (M.L2, M.IP):
        f, infos = rerank(hk, table, runs, Q, k, kout, metric, xmax2=1e30, eps=1.0)  # a huge, finite E
        assert f == set() and [i["ncand"] for i in infos] == [15, 5, 0, 0]
        f, _ = rerank(hk, table, runs, Q, k, kout, metric, xmax2=np.inf, eps=1.0)  # E = +inf
        assert f == {0, 1}
        f, _ = rerank(hk, table, runs, Q, k, kout, metric, xmax2=10.0, cert="cs", rxmax=1.0,
                      qres=np.full(4, np.inf, F), qnorm=qn)
        assert f == {0, 1}
    f, _ = rerank(hk, table, runs, Q, k, kout, M.L2, xmax2=10.0, cert="i8_l2", qres=np.full(4, np.inf, F), qnorm=qn)
    assert f == {0, 1}
    f, _ = rerank(hk, table, runs, Q, k, kout, M.L2, xmax2=np.nan, cert="i8_l2", qres=np.zeros(4, F), qnorm=qn)
    assert f == {0, 1}
