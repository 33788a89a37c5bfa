"""An independent reference for IVF training (hipann_ivf_train, oracle_kmeans_train) that needs no summation order.

`ref_train_int` restates the trainer for integer-valued fp32 rows, L2 (or IP at niter = 0), niter <= 1, in int64 and
Python integers only.  The initial centroids are training rows, so with small integer values (|v| <= 3, d <= 768:
‖x‖² <= 6912) every fp32 product, norm and sum on the GPU, in the oracle and here is an integer far below 2^24, and
every fp64 D² of k-means++ is exact: no rounding happens anywhere, the order of a sum cannot matter, a tie between
two centroids is a real tie (resolved towards the lower label, as the Flat search is required to), and the three
implementations must agree bit for bit.  After the first iteration the centroids stop being integers, which is why
the reference stops at niter = 1.

`assignment_margin` is the condition under which float rows train bit-equal as well: the smallest relative gap,
over the rows, between the nearest and the second nearest centroid.

`TIER_A_CASES` is the case table the CPU test (reference == oracle) and the GPU test (GPU == reference == oracle)
share."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

_M64 = (1 << 64) - 1
KM_SEED = 77  # the k-means seed of every Tier A run


class SplitMix64:
    """The trainer's random stream (km_next / km_rand_float)."""

    def __init__(self, seed: int):
        self.s = seed & _M64

    def next(self) -> int:
        self.s = (self.s + 0x9E3779B97F4A7C15) & _M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)

    def rand_float(self) -> np.float32:
        return np.float32(self.next() >> 40) * np.float32(2.0 ** -24)


def training_rows(n: int, train_sample: int, nlist: int, rng: SplitMix64) -> np.ndarray:
    """The stride sample (0 < train_sample < n), then above 256·nlist rows a uniform subset in ascending order."""
    if 0 < train_sample < n:
        stride = float(n) / float(train_sample)
        rows = [int(float(i) * stride) for i in range(train_sample)]
    else:
        rows = list(range(n))
    m, maxp = len(rows), 256 * nlist
    if m > maxp:
        perm = list(range(m))
        for i in range(maxp):
            j = i + rng.next() % (m - i)
            perm[i], perm[j] = perm[j], perm[i]
        rows = [rows[i] for i in sorted(perm[:maxp])]
    return np.array(rows, np.int64)


def init_rows(Ti: np.ndarray, nlist: int, init: int, rng: SplitMix64) -> list:
    """The indices (into the training rows Ti, int64) of the initial centroids: init 0 the first nlist entries of a
    partial Fisher-Yates, init 1 k-means++ with exact integer D², weights uint64(float64(D²)·(2^32/float64(max)))
    and the first row whose running weight exceeds r mod Σw (every D² zero: r mod m)."""
    m = len(Ti)
    if init == 0:
        perm, pick = list(range(m)), []
        for i in range(nlist):
            j = i + rng.next() % (m - i)
            perm[i], perm[j] = perm[j], perm[i]
            pick.append(perm[i])
        return pick
    assert init == 1
    pick, d2 = [rng.next() % m], None
    for _ in range(1, nlist):
        v = ((Ti - Ti[pick[-1]]) ** 2).sum(1)
        d2 = v if d2 is None else np.minimum(d2, v)
        r, mx = rng.next(), int(d2.max())
        if mx > 0:
            scale = np.float64(4294967296.0) / np.float64(mx)
            w = (d2.astype(np.float64) * scale).astype(np.uint64)
            t = r % int(w.sum(dtype=np.uint64))  # at most m · 2^32 < 2^64
            cs = np.cumsum(w, dtype=np.uint64)
            pick.append(int(np.searchsorted(cs, np.uint64(t), side="right")))
        else:
            pick.append(r % m)
    return pick


def _assign_int(Ti: np.ndarray, ci: np.ndarray) -> np.ndarray:
    """argmin over the centroids of the exact integer ‖x‖² + ‖c‖² − 2x·c; the first minimum is the lowest label."""
    cn = (ci ** 2).sum(1)[None]
    a = np.empty(len(Ti), np.int64)
    for r0 in range(0, len(Ti), 16384):
        t = Ti[r0:r0 + 16384]
        a[r0:r0 + 16384] = ((t ** 2).sum(1)[:, None] + cn - 2 * (t @ ci.T)).argmin(1)
    return a


def ref_init(x: np.ndarray, nlist: int, train_sample: int, seed: int, init: int):
    """Sampling and init, the part niter does not change: (training row indices into x, the init's indices into
    those, the state of the random stream afterwards)."""
    rng = SplitMix64(seed)
    rows = training_rows(len(x), train_sample, nlist, rng)
    pick = init_rows(np.asarray(x)[rows].astype(np.int64), nlist, init, rng)
    return rows, pick, rng.s


def ref_train_int(x: np.ndarray, nlist: int, train_sample: int, niter: int, seed: int, init: int, metric: int = 0,
                  info: dict | None = None, start=None):
    """(centroids nlist × d fp32, list_sizes int64) of hipann_ivf_train on integer-valued rows.  `info`, when given,
    receives what the tests assert as preconditions: "m", "pick" (the init's row indices into the training rows),
    "distinct" (distinct training rows), "empty" (clusters the first assignment left empty).  `start` is a
    ref_init result of the same arguments, to share one between niter 0 and 1."""
    x = np.asarray(x)
    assert niter in (0, 1) and np.array_equal(x, np.rint(x)) and (metric == 0 or niter == 0)
    rows, pick, state = start if start is not None else ref_init(x, nlist, train_sample, seed, init)
    rng = SplitMix64(state)
    d = x.shape[1]
    T = x[rows]
    m = len(T)
    Ti = T.astype(np.int64)
    cen = T[pick].astype(np.float32).copy()
    sizes = np.zeros(nlist, np.int64)
    if info is not None:
        info.update(m=m, pick=list(pick), distinct=len(np.unique(Ti, axis=0)), empty=0)
    if niter == 0:
        if metric == 1:  # spherical: unit-norm centroids (an exact fp64 sum of integer squares)
            s = (cen.astype(np.int64) ** 2).sum(1).astype(np.float64)
            inv = np.where(s > 0, 1.0 / np.sqrt(np.maximum(s, 1.0)), 1.0).astype(np.float32)
            cen = cen * inv[:, None]
        return cen, sizes
    a = _assign_int(Ti, cen.astype(np.int64))
    sizes = np.bincount(a, minlength=nlist).astype(np.int64)
    S = np.zeros((nlist, d), np.int64)
    np.add.at(S, a, Ti)
    nz = sizes > 0
    cen[nz] = (S[nz].astype(np.float64) / sizes[nz, None].astype(np.float64)).astype(np.float32)
    if info is not None:
        info["empty"] = int((~nz).sum())
    # FAISS split_clusters: float sizes, EPS = 1/1024, even dims of the new centroid up and of the donor down
    hs = sizes.astype(np.float32)
    one, eps = np.float32(1), np.float32(1 / 1024)
    even = np.arange(d) % 2 == 0
    for c in range(nlist):
        if hs[c] != 0:
            continue
        cj = 0
        while True:
            p = np.float32((np.float64(hs[cj]) - 1.0) / np.float64(np.float32(m - nlist)))
            if rng.rand_float() < p:
                break
            cj = (cj + 1) % nlist
        src = cen[cj].copy()
        cen[c] = np.where(even, src * (one + eps), src * (one - eps))
        cen[cj] = np.where(even, src * (one - eps), src * (one + eps))
        hs[c] = hs[cj] / np.float32(2)
        hs[cj] -= hs[c]
    return cen, sizes


def assignment_margin(x: np.ndarray, centroids: np.ndarray, metric: int) -> float:
    """min over the rows of (second-best − best centroid distance) / scale in fp64, where scale is the larger of the
    two distances' scales: ‖x‖² + ‖c‖² for L2, Σ|x_e||c_e| for IP.  inf for a single centroid."""
    if centroids.shape[0] == 1:
        return float("inf")
    x64, c64 = np.asarray(x, np.float64), np.asarray(centroids, np.float64)
    if metric == 0:
        sc = (x64 ** 2).sum(1)[:, None] + (c64 ** 2).sum(1)[None]
        D = sc - 2 * x64 @ c64.T
    else:
        D = -(x64 @ c64.T)
        sc = np.abs(x64) @ np.abs(c64.T)
    idx = np.argsort(D, axis=1, kind="stable")[:, :2]
    b = np.take_along_axis(D, idx, 1)
    s = np.take_along_axis(sc, idx, 1).max(1)
    return float(((b[:, 1] - b[:, 0]) / s).min())


def int_rows(n: int, d: int, hi: int, seed: int) -> np.ndarray:
    """n × d fp32 rows of integers uniform in [−hi, hi]."""
    return np.ascontiguousarray(np.random.default_rng(seed).integers(-hi, hi + 1, (n, d)).astype(np.float32))


# (n, d, nlist, train_sample, hi); the data seed of a case is n + d
D_SWEEP = (1, 2, 3, 5, 63, 64, 65, 129, 257, 300, 768)
NLIST_SWEEP = (1, 2, 3, 255, 256, 257, 1024)
CASE_BATCH2 = (65541, 4, 260, 0, 2)      # second assignment batch of 5 rows, nb = 257, 34 splits with the random init
CASE_BATCH3 = (131073, 4, 513, 0, 2)     # three batches, the last of 1 row, 160 splits (random init)
CASE_STRIDE_SUBSET = (3000, 20, 4, 2500, 3)  # stride sample, then the 256·nlist subset: m = 1024
CASE_SUBSET_ODD_D = (3000, 5, 4, 0, 1)
CASE_FEW_DISTINCT = (400, 2, 40, 0, 1)   # 9 distinct rows for 40 centres: mx == 0 in kpp_pick, 31 empty clusters
CASE_STRIDE_DUP = (2000, 3, 64, 1999, 1)  # stride n/(n−1), 27 distinct rows
TIER_A_CASES = ([(1031, d, 7, 0, 3) for d in D_SWEEP] +
                [(max(5 * nl + 3, 300), 16, nl, 0, 3) for nl in NLIST_SWEEP] +
                [CASE_BATCH2, CASE_BATCH3, CASE_STRIDE_SUBSET, CASE_SUBSET_ODD_D, CASE_FEW_DISTINCT, CASE_STRIDE_DUP])


def mixture_rows(m: int, d: int, nc: int, seed: int) -> np.ndarray:
    """A separated mixture of float rows: nc centres uniform(−1, 1)·10, row i = centre[i mod nc] + uniform(−1, 1)·0.5."""
    r = np.random.default_rng(seed)
    cen = r.uniform(-1, 1, (nc, d)).astype(np.float32) * np.float32(10.0)
    x = cen[np.arange(m) % nc] + r.uniform(-1, 1, (m, d)).astype(np.float32) * np.float32(0.5)
    return np.ascontiguousarray(x.astype(np.float32))


def margin_tau(d: int) -> float:
    """The margin above which an fp32 assignment cannot differ from the exact one: an fp32 distance in either form
    carries at most about (d + 3)·2^-24·scale of rounding error, on each of the two distances compared; τ is twice
    the sum of the two."""
    return 4.0 * (d + 4) * 2.0 ** -24


def training_margin(kmeans_train, x: np.ndarray, nlist: int, metric: int, niter: int, seed: int, init: int) -> float:
    """min over t < niter of assignment_margin on the centroids `kmeans_train` (the oracle's) gives after t
    iterations, over the training rows (train_sample = 0): the margin of every assignment a niter-iteration run
    makes."""
    T = x[training_rows(len(x), 0, nlist, SplitMix64(seed))]
    return min(assignment_margin(T, kmeans_train(x, nlist, metric, 0, t, seed, init)[0], metric) for t in range(niter))


# Tier B: (m, d, nlist, metric, data seed) — float rows of mixture_rows(m, d, nlist, seed), k-means++ init, k-means
# seed 1234, 6 iterations.  The data seed is 1000 + d unless the margin of that seed is below 10·τ (d = 3: 9× for L2,
# 1.5× for IP) or below τ (d = 300: k-means++ puts two centres into one component); then 2000 + d, 3000 + d.
TIER_B_NITER, TIER_B_SEED = 6, 1234
_TIER_B_DATA_SEED = {3: 3003, 300: 2300}
TIER_B_CASES = ([(1031, d, 7, metric, _TIER_B_DATA_SEED.get(d, 1000 + d))
                 for d in (3, 5, 63, 64, 65, 129, 257, 300, 768) for metric in (0, 1)] +
                [(4000, 100, 24, 0, 1100), (4000, 100, 24, 1, 1100),
                 (1031, 1, 3, 0, 1001), (1031, 1, 5, 0, 1001), (1031, 2, 3, 0, 1002), (1031, 2, 5, 0, 1002)])


def tier_b_id(case) -> str:
    m, d, nlist, metric, seed = case
    return f"m{m}-d{d}-nlist{nlist}-{'ip' if metric else 'l2'}-seed{seed}"


def case_id(case) -> str:
    n, d, nlist, ts, hi = case
    return f"n{n}-d{d}-nlist{nlist}-ts{ts}-hi{hi}"


def case_inits(case) -> tuple:
    """Both inits, except the 131073-row case: its k-means++ run costs the oracle several seconds and reaches
    nothing the 65541-row case does not."""
    return (0,) if case == CASE_BATCH3 else (0, 1)


@lru_cache(maxsize=None)
def case_rows(case) -> np.ndarray:
    n, d, _, _, hi = case
    x = int_rows(n, d, hi, n + d)
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def _case_init(case, init: int, seed: int):
    _, _, nlist, ts, _ = case
    return ref_init(case_rows(case), nlist, ts, seed, init)


@lru_cache(maxsize=None)
def case_ref(case, niter: int, init: int, seed: int = KM_SEED):
    """(centroids, sizes, info) of the reference on a Tier A case, computed once and read-only."""
    _, _, nlist, ts, _ = case
    info: dict = {}
    cen, sizes = ref_train_int(case_rows(case), nlist, ts, niter, seed, init, info=info,
                               start=_case_init(case, init, seed))
    cen.setflags(write=False)
    sizes.setflags(write=False)
    return cen, sizes, info
