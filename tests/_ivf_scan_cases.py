"""Inputs and a plain numpy model of the IVF image scans (csrc/ivf_mfma.hip, csrc/ivf_kernels.hip): the tiled fp16 and
int8 images, the query preparation, the scan's keys and per-wave 16-lists, the per-query bound, the seeded scan's
seed list, and ivf_rerank_topk with its three certificates.  Shared by tests/test_ivf_scan_cases.py (CPU) and
tests/test_ivf_scan_gpu.py.

Two input families:

  * exact: every quantity the kernels form is exact in fp32, so any summation order gives the same bits and the GPU
    tests compare bit for bit.
      int8: rows and queries are small integers (|v| <= 1, a third of the dims) with one element of magnitude 127,
      times a per-row 2^e, e in -2..2.  max|x| = 127 * 2^e, so s = max|x| / 127 = 2^e exactly, the units are the
      integers and the residual is 0.  Norms, sums and keys are integer multiples of 2^-4 (2^-8 for the products of
      two scales) below 2^24 of those units; test_ivf_scan_cases.py recomputes them in int64 and checks.
      fp16: integers |v| <= 15 times one power of two: the image, the queries' one-term h (l = 0, residual 0) and
      every MFMA sum are exact.
  * float: low-rank gaussian rows (_i8cert.lowrank_case) at scales 1e-3 .. 50; the kernels are compared with fp64
    references under bounds derived from their documented arithmetic.

Layouts (ivf_mfma.hip): a list's rows in 32-row passes, two 16-row tiles per pass.
  fp16 image [pass][32-dim super-step S][tile r][lane (g, m)][8 halves]: row 16r + m, dims 32S + 4g + j and
  32S + 16 + 4g + j (j < 4); RNE, subnormal results flushed to zero, zero past the live rows and past d.
  int8 image [pass][64-dim super-step S][tile r][lane (g, m)][16 units]: row 16r + m, dims 64S + 16g + i.
  Super-step counts are rounded up to the scan's ring depth (MH_P = 6).
The scan: a list's 2048-row chunk is one item per query group; wave w of its 8 takes the passes w, w + 8, ... and
keeps the 16 smallest (key, row); with sub-lists every wave's list is written to the (query, probe, chunk) slot, else
their merged 16.  A list of 16 real entries publishes its 16th key to the query's bound (atomicMin).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F = np.float32
L2, IP = 0, 1
HALF, I8 = 1, 2  # image kinds (hipann_debug_ivf_info "image")
PASS, CH, WAVES, K, SEED_K = 32, 2048, 8, 16, 64
MH_P = 6
PAD_ID = 0x7FFFFFFF
INF = F(np.inf)
QB_INF = 0xFF800000  # a bound of +inf in the scan's order-preserving bits
UP = F(1.0001)


def nsup_half(d, p=MH_P):
    return -(-(-(-d // 32)) // p) * p


def nsup_i8(d, p=MH_P):
    return -(-(-(-d // 64)) // p) * p


# ---- number formats ------------------------------------------------------------------------------------------------
def sortable(f):
    """mf_sortable: float32 -> uint32 whose unsigned order is the float order (-0 below +0)."""
    u = np.ascontiguousarray(f, dtype=F).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def unsortable(s):
    s = np.asarray(s, dtype=np.uint32)
    return np.where(s & 0x80000000, s & 0x7FFFFFFF, ~s).astype(np.uint32).view(F)


def half_bits(v):
    """mh_half_bits: fp32 -> fp16 bits, round to nearest even, subnormal results (and -0) flushed to +0."""
    with np.errstate(over="ignore"):
        h = np.asarray(v, dtype=F).astype(np.float16)
    b = h.view(np.uint16).copy()
    b[np.abs(h.astype(F)) < F(2.0 ** -14)] = 0
    return b


def half_val(b):
    return np.asarray(b, dtype=np.uint16).view(np.float16).astype(F)


def max_exp(x):
    """(ok, e): max|x| = f * 2^e, f in [1/2, 1) (e = 0 for an all-zero array); ok False when non-finite."""
    bits = int(np.max(np.ascontiguousarray(x, dtype=F).view(np.uint32) & 0x7FFFFFFF, initial=0))
    if bits >= 0x7F800000:
        return False, 0
    return True, (int(np.frexp(np.array([bits], np.uint32).view(F)[0])[1]) if bits else 0)


def i8_scale(X):
    """mi_row_scale: max|x| / 127 (fmaxf drops NaNs); 0 for a zero row; -1 for a row with a +-inf element."""
    X = np.asarray(X, dtype=F)
    with np.errstate(invalid="ignore"):
        m = np.fmax.reduce(np.abs(X), axis=1, initial=F(0)).astype(F)
    with np.errstate(over="ignore"):
        s = (m / F(127.0)).astype(F)
    return np.where((m > 0) & (m < F(3.0e38)), s, np.where(m == 0, F(0), F(-1))).astype(F)


def i8_units(X, s):
    """mi_quant: clamp(rint(x / s), +-127) with the fp32 division the kernel performs; 0 where s <= 0."""
    X = np.asarray(X, dtype=F)
    sd = np.where(s > 0, s, F(1)).astype(F)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.clip(np.rint((X / sd).astype(F)), -127, 127)
    c = np.where(np.isnan(c), -127, c)  # fminf(fmaxf(NaN, -127), 127)
    return np.where(s[:, None] > 0, c, 0).astype(np.int8)


# ---- lists ---------------------------------------------------------------------------------------------------------
@dataclass
class Lists:
    rows: np.ndarray  # n x d fp32 in CSR order
    off: np.ndarray   # nlist + 1 int64 (capacity = length here)

    @property
    def nlist(self):
        return len(self.off) - 1

    @property
    def lens(self):
        return np.diff(self.off)

    @property
    def tpass(self):
        return np.concatenate([[0], np.cumsum(-(-self.lens // PASS))]).astype(np.int64)

    def hand(self):
        """(centroids, offsets, ids, codes) for HipIndexIVFFlat: any centroids do, the probes come from the caller."""
        d = self.rows.shape[1]
        cen = np.zeros((self.nlist, d), F)
        cen[:, 0] = np.arange(self.nlist)
        return cen, self.off.astype(np.int64), np.arange(len(self.rows), dtype=np.int64), np.ascontiguousarray(self.rows)


def _padded(V, lists: Lists, width, lens=None):
    """V's rows laid out pass by pass (32 rows each, lists padded to whole passes), zero past the live rows and past
    d: [total passes * 32, width]."""
    tp = lists.tpass
    lens = lists.lens if lens is None else lens
    out = np.zeros((int(tp[-1]) * PASS, width), V.dtype)
    for l in range(lists.nlist):
        n = int(lens[l])
        out[int(tp[l]) * PASS:int(tp[l]) * PASS + n, :V.shape[1]] = V[int(lists.off[l]):int(lists.off[l]) + n]
    return out


def half_image(lists: Lists, nsup, es, lens=None):
    """uint16 [pass][S][r][lane][8] of the fp16 image of rows * 2^es."""
    with np.errstate(over="ignore", invalid="ignore"):
        b = half_bits((lists.rows * F(2.0 ** es)).astype(F))
    P = _padded(b, lists, nsup * 32, lens)
    npass = len(P) // PASS
    P = P.reshape(npass, 2, 16, nsup, 2, 4, 4)      # [pass, r, m, S, half, g, j]
    P = P.transpose(0, 3, 1, 5, 2, 4, 6)            # [pass, S, r, g, m, half, j]
    return np.ascontiguousarray(P).reshape(npass, nsup, 2, 64, 8)


def i8_image(lists: Lists, nsup, units, lens=None):
    """int8 [pass][S][r][lane][16] of the rows' units."""
    P = _padded(units, lists, nsup * 64, lens)
    npass = len(P) // PASS
    P = P.reshape(npass, 2, 16, nsup, 4, 16)        # [pass, r, m, S, g, i]
    P = P.transpose(0, 3, 1, 4, 2, 5)               # [pass, S, r, g, m, i]
    return np.ascontiguousarray(P).reshape(npass, nsup, 2, 64, 16)


def half_es(rows):
    ok, e = max_exp(rows)
    return ok and -100 <= e <= 100, 14 - e


# ---- query preparation ---------------------------------------------------------------------------------------------
def split_queries_h(Q, nsup, es):
    """ivf_split_queries_h: (hsplit uint16 [q][term][S][g][8], its, r2, r1, ok) with r2 / r1 the two-term / one-term
    split residuals in fp64 (the kernel's carry x1.0001 on an fp32 sum); a query outside the safe range: zero terms."""
    Q = np.asarray(Q, dtype=F)
    nq, d = Q.shape
    out = np.zeros((nq, 2, nsup, 4, 8), np.uint16)
    its = np.ones(nq, F)
    r2, r1, okv = np.zeros(nq), np.zeros(nq), np.zeros(nq, bool)
    for q in range(nq):
        ok, eq = max_exp(Q[q])
        et = 14 - eq
        eits = -(et + es)
        ok = ok and -100 <= eq <= 100 and -120 <= eits <= 120
        okv[q] = ok
        if not ok:
            r2[q] = r1[q] = np.inf
            continue
        a = np.zeros(nsup * 32, F)
        a[:d] = Q[q] * F(2.0 ** et)
        h = half_bits(a)
        m = a - half_val(h)  # exact
        lo = half_bits(m)
        its[q] = F(2.0 ** eits)
        r1[q] = np.sqrt(np.sum((m.astype(np.float64) * 2.0 ** -et) ** 2))
        r2[q] = np.sqrt(np.sum(((m - half_val(lo)).astype(np.float64) * 2.0 ** -et) ** 2))
        for t, w in enumerate((h, lo)):
            out[q, t] = w.reshape(nsup, 2, 4, 4).transpose(0, 2, 1, 3).reshape(nsup, 4, 8)
    return out, its, r2, r1, okv


def split_queries_i8(Q, nsup):
    """ivf_split_queries_i8: (units int8 [q][S][g][16], scale, finite) — residuals and norms come from these."""
    Q = np.asarray(Q, dtype=F)
    s = i8_scale(Q)
    fin = s >= 0
    s = np.where(fin, s, F(0)).astype(F)
    u = i8_units(Q, s)
    P = np.zeros((len(Q), nsup * 64), np.int8)
    P[:, :Q.shape[1]] = u
    return P.reshape(len(Q), nsup, 4, 16), s, fin, u


# ---- keys ----------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf in fp32 through fp64 (products of two fp32 are exact in fp64; the exact family never rounds)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def row_norms(X):
    return np.sum(np.asarray(X, np.float64) ** 2, axis=1).astype(F)


def keys_i8(Q, X, metric):
    """The int8 scan's key of every (query, row), following the kernel's fp32 operations (exact-family inputs:
    residuals 0): (keys [nq, n], dict of the planes)."""
    qs = i8_scale(Q)
    xs = i8_scale(X)
    qu, xu = i8_units(Q, qs), i8_units(X, xs)
    av = (qu.astype(np.int64) @ xu.astype(np.int64).T).astype(F)  # int32 sums, converted
    sc = (qs[:, None] * xs[None, :]).astype(F)
    qh = (qs[:, None] * qu.astype(F)).astype(F)
    qhn2 = row_norms(qh)
    qhn = (np.sqrt(qhn2) * UP).astype(F)
    xr = np.sqrt(np.sum((X.astype(np.float64) - xs[:, None].astype(np.float64) * xu) ** 2, axis=1))
    xr8 = (xr * float(UP)).astype(F)  # (0 in the exact family)
    xn = row_norms(X)
    planes = dict(qs8=qs, xs8=xs, qhn2=qhn2, qhn=qhn, xr8=xr8, xnorm=xn, qu=qu, xu=xu)
    if metric == IP:
        return (-av * sc).astype(F), planes
    key = _fma(F(-2) * sc, av, (qhn2[:, None] + xn[None, :]).astype(F))
    key = _fma(-(F(2) * qhn)[:, None], xr8[None, :], key)
    return np.where(key < 0, F(0), key).astype(F), planes


def keys_half(Q, X, metric, es):
    """The fp16 scan's key (one query term) of every (query, row) for exact-family inputs."""
    nq, d = Q.shape
    ns = nsup_half(d)
    hs, its, _, _, ok = split_queries_h(Q, ns, es)
    assert ok.all()
    xh = half_val(half_bits((X * F(2.0 ** es)).astype(F))).astype(np.float64)
    qh = np.zeros((nq, d))
    for q in range(nq):
        qh[q] = half_val(hs[q, 0].reshape(ns, 4, 2, 4).transpose(0, 2, 1, 3).reshape(-1))[:d]
    av = (qh @ xh.T).astype(F)
    if metric == IP:
        return (-av * its[:, None]).astype(F), dict(its=its, av=av)
    key = _fma((F(-2) * its)[:, None], av, (row_norms(Q)[:, None] + row_norms(X)[None, :]).astype(F))
    return np.where(key < 0, F(0), key).astype(F), dict(its=its, av=av)


# ---- the scan's lists ----------------------------------------------------------------------------------------------
def packed(keys, rows):
    return (sortable(keys).astype(np.uint64) << np.uint64(32)) | np.asarray(rows, np.uint64)


def smallest(keys, rows, n=K):
    """The n smallest (key, row) as (keys, rows), ascending."""
    o = np.argsort(packed(keys, rows), kind="stable")[:n]
    return np.asarray(keys, F)[o], np.asarray(rows, np.int64)[o]


def shares(lists: Lists, l):
    """List l's rows by (chunk, wave): {(chunk, wave): CSR rows}; wave w of a chunk takes its passes w, w + 8, ..."""
    j = np.arange(int(lists.lens[l]))
    ch, wv = j // CH, ((j % CH) // PASS) % WAVES
    return {(int(c), int(w)): int(lists.off[l]) + j[(ch == c) & (wv == w)]
            for c in np.unique(ch) for w in np.unique(wv[ch == c])}


def slot_prefix(lists: Lists, probes):
    """slot_off of the plan: one slot per (query, probe, chunk), query-major."""
    nch = -(-lists.lens // CH)
    return np.concatenate([[0], np.cumsum(nch[np.asarray(probes).ravel()])]).astype(np.int64)


def plan_model(lists: Lists, probes, group_wide=96):
    """The plan's tables: (cnt, item_off, goff, slot_off) — queries per non-empty list, the lists' first items
    (ng * nch each), their first chunk-0 items (ng each) and the slot prefixes."""
    cnt = np.bincount(np.asarray(probes).ravel(), minlength=lists.nlist)
    cnt[lists.lens == 0] = 0  # the plan counts no pair of an empty list: it gets no slot, no item and no bucket entry
    ng, nch = -(-cnt // group_wide), -(-lists.lens // CH)
    return (cnt, np.concatenate([[0], np.cumsum(ng * nch)]), np.concatenate([[0], np.cumsum(ng)]),
            slot_prefix(lists, probes))


def scan_model(keys, lists: Lists, probes, sub):
    """Ungated slot contents: {(q, p, chunk): (keys [W, 16], rows [W, 16])} with W = 8 sub-lists (sub) or 1 merged
    list, pads (+inf, PAD_ID); and every query's final bound (order-preserving bits)."""
    nq = len(keys)
    out, bound = {}, np.full(nq, QB_INF, np.uint32)
    for q in range(nq):
        for p, l in enumerate(np.asarray(probes)[q]):
            sh = shares(lists, int(l))
            for c in range(int(-(-lists.lens[l] // CH))):
                W = WAVES if sub else 1
                kd, ki = np.full((W, K), INF, F), np.full((W, K), PAD_ID, np.int64)
                if sub:
                    parts = [(w, sh[(c, w)]) for w in range(WAVES) if (c, w) in sh]
                else:
                    parts = [(0, np.concatenate([sh[(c, w)] for w in range(WAVES) if (c, w) in sh]))]
                for w, rows in parts:
                    a, b = smallest(keys[q, rows], rows)
                    kd[w, :len(a)], ki[w, :len(a)] = a, b
                    if len(a) == K:
                        bound[q] = min(bound[q], sortable(a[-1:])[0])
                out[(q, p, c)] = (kd, ki)
    return out, bound


def seed_model(keys, lists: Lists, probes, bound1):
    """ivf_seed_bound: per query the SEED_K smallest (key, row) of its chunk-0 sub-list entries at or below bound1[q]
    (the bound after the chunk-0 items), pads last, and the bound after the min with a real 64th key."""
    slots, _ = scan_model(keys, lists, probes, True)
    nq = len(keys)
    sd, si = np.full((nq, SEED_K), INF, F), np.full((nq, SEED_K), PAD_ID, np.int64)
    bound = np.array(bound1, np.uint32)
    for q in range(nq):
        ks = [slots[(q, p, 0)] for p in range(np.asarray(probes).shape[1]) if (q, p, 0) in slots]
        if not ks:
            continue
        kd = np.concatenate([a.ravel() for a, _ in ks])
        ki = np.concatenate([b.ravel() for _, b in ks])
        m = (ki != PAD_ID) & (sortable(kd) <= bound[q])
        a, b = smallest(kd[m], ki[m], SEED_K)
        sd[q, :len(a)], si[q, :len(a)] = a, b
        if len(a) == SEED_K:
            bound[q] = min(bound[q], sortable(a[-1:])[0])
    return sd, si, bound


# ---- exact-family inputs -------------------------------------------------------------------------------------------
def exact_i8(n, d, nq, seed, e_lo=-2, e_hi=2):
    """Integer rows / queries for the int8 image (module docstring); returns (X, Q) fp32."""
    rng = np.random.default_rng(seed)

    def make(m):
        v = rng.integers(-1, 2, (m, d)) * (rng.random((m, d)) < 1 / 3)
        v[np.arange(m), rng.integers(0, d, m)] = 127 * rng.choice([-1, 1], m)
        return (v * 2.0 ** rng.integers(e_lo, e_hi + 1, m)[:, None]).astype(F)

    return make(n), make(nq)


def exact_half(n, d, nq, seed, p=-3):
    rng = np.random.default_rng(seed)
    X = (rng.integers(-15, 16, (n, d)) * 2.0 ** p).astype(F)
    Q = (rng.integers(-15, 16, (nq, d)) * 2.0 ** p).astype(F)
    X[0, 0] = F(15 * 2.0 ** p)  # the table's and a query's maximum are known
    Q[0, 0] = F(-15 * 2.0 ** p)
    return X, Q


def plant(X, Q, lists_sizes, kind):
    """Edge rows planted into exact inputs: row 0 of the first list = query 0 (key 0 for L2: the clamp), the same row
    duplicated across passes, waves, chunks and lists (ties on key), and — when a list has exactly 40 rows — that
    list all equal."""
    off = np.concatenate([[0], np.cumsum(lists_sizes)])
    n = len(X)
    X[0] = Q[0]
    for r in (1, 17, 33, 32 * 8 + 2, 2048 + 5, 2049 + 40):  # next tile, next pass, next wave round, next chunk
        if r < n:
            X[r] = X[0]
    for l in range(1, len(lists_sizes)):
        if lists_sizes[l] > 2:
            X[off[l] + 1] = X[0]
        for r in (32 * 9 + 3, 2048 + 64 + 7, 4096 + 9):  # ... of a later list's chunks too
            if r < lists_sizes[l]:
                X[off[l] + r] = X[0]
        if lists_sizes[l] == 40:
            X[off[l]:off[l + 1]] = X[off[l]]
    return X


# The case table of the scan tests: name -> (list sizes, nq, d).  nprobe = nlist, every query probes every list.
SCAN_CASES = {
    # single item: one list, one chunk, nq <= 96 — the slot contents are deterministic
    "one_row_d1": ([1], 1, 1),
    "share15_d20": ([15], 15, 20),
    "share16_d64": ([16], 17, 64),
    "share17_d100": ([17], 40, 100),
    "tile33_d192": ([33], 17, 192),            # a last pass of one row
    "waves256_d64": ([256], 40, 64),           # every wave one pass
    "wave7_share16_d20": ([32 * 7 + 16], 15, 20),  # the last wave's share is exactly 16 rows
    "wave7_share15_d20": ([32 * 7 + 15], 15, 20),  # ... and 15: it publishes no bound
    "chunk2048_d832": ([2048], 17, 832),       # a full chunk, more than MH_P int8 super-steps
    # multi item: chunks, groups, lists — compared by the invariant
    "chunk2049_d64": ([2049], 40, 64),         # the second chunk has one row
    "groups97_d20": ([300], 97, 20),           # more than 96 queries on a list: two query groups
    "lists_d64": ([0, 1, 15, 16, 40, 4200], 17, 64),  # an empty list, an all-equal list, three chunks
    "groups100_chunks_d100": ([2049, 33], 100, 100),
}
SINGLE_ITEM = [n for n, (s, nq, _) in SCAN_CASES.items() if len(s) == 1 and s[0] <= CH and nq <= 96]
MULTI_ITEM = [n for n in SCAN_CASES if n not in SINGLE_ITEM]


def scan_case(name, kind):
    sizes, nq, d = SCAN_CASES[name]
    n = int(sum(sizes))
    seed = sorted(SCAN_CASES).index(name) + (100 if kind == I8 else 200)
    X, Q = exact_i8(n, d, nq, seed) if kind == I8 else exact_half(n, d, nq, seed)
    if d >= 20:
        X = plant(X, Q, sizes, kind)
    lists = Lists(np.ascontiguousarray(X), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    probes = np.tile(np.arange(len(sizes), dtype=np.int64), (nq, 1))
    return lists, np.ascontiguousarray(Q), probes


def float_case(n, d, nq, seed):
    """Low-rank gaussian rows at per-row scales 1e-3 .. 50 (the float family)."""
    import _i8cert as C8

    xb, xq = C8.lowrank_case(n, d, min(4, d), 0.02, nq, seed)
    rng = np.random.default_rng(seed + 1)
    sc = np.array([1e-3, 0.05, 1.0, 7.0, 50.0], F)
    xb = (xb * sc[rng.integers(0, len(sc), n)][:, None]).astype(F)
    xq = (xq * sc[rng.integers(0, len(sc), nq)][:, None]).astype(F)
    return np.ascontiguousarray(xb), np.ascontiguousarray(xq)


# ---- ivf_rerank_topk -----------------------------------------------------------------------------------------------
RR_WAVES, RR_J = 4, 16  # the launcher's kernel: a 4-wave block per query, the wave select up to 64 * 4 * 16 candidates


def _take(kd, ki, k):
    """rws_kth_bits + rws_take over a run in order: the keys below the k-th smallest key's bits, then the first
    entries at it, in run order."""
    if len(kd) <= k:
        return kd, ki
    b = sortable(np.where(kd == 0, F(0), kd))
    T = np.sort(b)[k - 1]
    lt, eq = np.nonzero(b < T)[0], np.nonzero(b == T)[0]
    o = np.concatenate([lt, eq])[:k]
    return kd[o], ki[o]


def rerank_select(pd, pi, k, nrows, tsub, sub, bound=np.inf):
    """The k candidates ivf_rerank_topk<.., 4> selects from a query's run (pd, pi), ascending by (key, row).
    Up to 4096 entries: rerank_wave_select (wave w takes the 64-entry strips w, w + 4, ...; entries with key <= the
    bound — T_sub with sub-lists — finite, row in range; ties at a k-th key keep the first in run order).  More: the
    wave lists (key < T_sub; the k smallest by (key, row))."""
    pd, pi = np.asarray(pd, F), np.asarray(pi, np.int64)
    total = len(pd)
    valid = (pi >= 0) & (pi < nrows) & ~(pd == INF)
    with np.errstate(invalid="ignore"):
        if total <= 64 * RR_WAVES * RR_J:
            a = valid & (pd <= (tsub if sub else bound))
            c = np.arange(total)
            runs = []
            for w in range(RR_WAVES):
                m = a & ((c // 64) % RR_WAVES == w)
                runs.append(_take(pd[m], pi[m], k))
            kd, ki = _take(np.concatenate([r[0] for r in runs]), np.concatenate([r[1] for r in runs]), k)
        else:
            a = valid & (pd < tsub)
            kd, ki = pd[a], pi[a]
            o = np.lexsort((ki, kd))[:k]
            kd, ki = kd[o], ki[o]
    o = np.argsort(packed(np.where(kd == 0, F(0), kd), ki), kind="stable")
    return kd[o], ki[o]


def decode_bound(b):
    t = unsortable(np.array([b], np.uint32))[0]
    return INF if np.isnan(t) else t


def direct_dist(q, X, metric):
    q64, X64 = np.asarray(q, np.float64), np.asarray(X, np.float64)
    return (np.sum((X64 - q64) ** 2, axis=1) if metric == L2 else -(X64 @ q64)).astype(F)


def bf16_round(x):
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    return (((u + ((u >> 16) & 1) + 0x7FFF) >> 16).astype(np.uint32) << 16).view(F)


def cert_E(cert, metric, d, qq, xmax2, eps=0.0, rxmax=0.0, rq=0.0, have_qres=False):
    """E of the three certificates in fp64, as the header of ivf_rerank_topk and DESIGN.md section 2 state them."""
    fp = (d + 8) * 2.0 ** -24 * 2.0 * (qq + xmax2)
    if cert == "i8_l2":
        return 1.01 * fp
    if cert == "eps":
        return eps * (qq + xmax2)
    qn, xh = np.sqrt(qq), np.sqrt(xmax2) + rxmax
    g = (2 * d if have_qres else d) * 2.0 ** -24
    eip = qn * rxmax + rq * xh + g * (qn + rq) * xh
    return 1.01 * ((1.0 if metric == IP else 2.0) * eip + fp)


def cert_E_f32(cert, metric, d, qq, xmax2, eps=0.0, rxmax=0.0, rq=0.0, have_qres=False):
    """The same in the kernel's own fp32 operations and order (no contraction in the build)."""
    qq, xmax2, rxmax, rq, eps = F(qq), F(xmax2), F(rxmax), F(rq), F(eps)
    fp = F(d + 8) * F(2.0 ** -24) * F(2) * (qq + xmax2)
    if cert == "i8_l2":
        return F(1.01) * F(d + 8) * F(2.0 ** -24) * F(2) * (qq + xmax2)
    if cert == "eps":
        return eps * (qq + xmax2)
    qn, xh = np.sqrt(qq), np.sqrt(xmax2) + rxmax
    g = F(2 * d if have_qres else d) * F(2.0 ** -24)
    eip = qn * rxmax + rq * xh + g * (qn + rq) * xh
    return F(1.01) * ((F(1) if metric == IP else F(2)) * eip + fp)


def clears(cert, dk, B, E, rq=0.0, f32=False):
    """clear(B): the kout-th exact distance lies below every row pruned under the bound B."""
    if f32:
        dk, B, E, rq = F(dk), F(B), F(E), F(rq)
        if cert == "i8_l2":
            lhs = (np.sqrt(np.maximum(dk, F(0))) + rq) * (F(1) + F(2.0 ** -20))
            return bool(lhs < np.sqrt(np.maximum((B - E) * (F(1) - F(2.0 ** -20)), F(0))))
        return bool(dk < B - E)
    if cert == "i8_l2":
        return (np.sqrt(max(dk, 0.0)) + rq) * (1 + 2.0 ** -20) < np.sqrt(max((B - E) * (1 - 2.0 ** -20), 0.0))
    return dk < B - E


def scan_order_topk(dist, labels, pos, kout):
    """FAISS IndexIVFFlat's tie membership (ivf_scan_order_topk): every candidate below the kout-th distance T, and
    of those at T the ones among the first kout candidates with distance <= T in scan order (pos), of which the
    smallest labels; as (distance, label) ascending."""
    T = np.sort(dist)[kout - 1]
    lt = np.nonzero(dist < T)[0]
    le = np.nonzero(dist <= T)[0]
    first = le[np.argsort(pos[le], kind="stable")][:kout]
    eq = first[dist[first] == T]
    eq = eq[np.argsort(labels[eq], kind="stable")][:kout - len(lt)]
    sel = np.concatenate([lt, eq])
    return sel[np.lexsort((labels[sel], dist[sel]))]


def rerank_model(pd, pi, k, kout, metric, q, codes, nrows, ids=None, label_offset=0, xmax2=0.0, cert="eps", eps=0.0,
                 rxmax=-1.0, qres=None, qnorm=None, qbound=None, sub=0, probes=None, list_off=None, f32=False):
    """One query of ivf_rerank_topk: (D [kout], I [kout], flag, info).  pd / pi: the query's candidate run."""
    d = codes.shape[1]
    tsub = decode_bound(qbound) if (sub and qbound is not None) else INF
    bound = tsub if sub else (decode_bound(qbound) if qbound is not None else INF)
    kd, ki = rerank_select(pd, pi, k, nrows, tsub, sub, bound)
    ncand = len(kd)
    k16 = kd[k - 1] if ncand == k else INF
    dist = direct_dist(q, codes[ki], metric) if ncand else np.zeros(0, F)
    lab = (np.asarray(ids)[ki] if ids is not None else label_offset + ki).astype(np.int64)
    o = np.lexsort((lab, dist))
    if probes is not None and ncand:
        T = dist[o[kout - 1]] if ncand >= kout else INF
        if T != INF and np.count_nonzero(dist <= T) > kout:
            lst = np.searchsorted(np.asarray(list_off), ki, side="right") - 1
            rank = np.array([int(np.nonzero(np.asarray(probes) == l)[0][0]) for l in lst], np.int64)
            o = scan_order_topk(dist, lab, (rank << 32) | ki, kout)
    pad_d = -INF if metric == IP else INF
    D, I = np.full(kout, pad_d, F), np.full(kout, -1, np.int64)
    n = min(kout, len(o))
    D[:n] = -dist[o[:n]] if metric == IP else dist[o[:n]]
    I[:n] = lab[o[:n]]
    sd = np.sort(dist)
    dk = sd[kout - 1] if ncand >= kout else INF
    if qres is not None and qnorm is not None:
        qq, rq = float(qnorm), float(qres)
    else:
        qq = float(np.sum(np.asarray(q, np.float64) ** 2))
        rq = float(qres) if qres is not None else float(np.sqrt(np.sum(
            (np.asarray(q, np.float64) - bf16_round(q).astype(np.float64)) ** 2)))
    Efn = cert_E_f32 if f32 else cert_E
    with np.errstate(invalid="ignore", over="ignore"):
        E = Efn(cert, metric, d, qq, xmax2, eps, max(rxmax, 0.0), rq, qres is not None)
        fin = bool(E <= 3.4e38) and (cert != "i8_l2" or rq <= 3.4e38)
        flag = (ncand > 0 and not fin) or (ncand == k and not clears(cert, dk, k16, E, rq, f32)) or \
               (bool(sub) and tsub < INF and not clears(cert, dk, tsub, E, rq, f32))
    return D, I, bool(flag), dict(ncand=ncand, k16=k16, dk=dk, E=E, tsub=tsub, rows=ki, keys=kd)
