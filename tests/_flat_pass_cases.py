"""Exact inputs and a plain numpy model of the Flat bounded passes (flat_b16k64.hip).

The bounded passes scan a tiled bf16 or int8 image of the table under a per-query bound T and append every row
with key <= T to a per-(query, split) candidate buffer; flat_cand_bound tightens T from the candidates so far and
flat_cand_select keeps each query's k best by (key, row).  On general data the scan's keys carry fp32 rounding
in an order the MFMA fixes, so a model can only agree within a tolerance.  The builders here make every quantity
the kernels form exact in fp32 instead — then any summation order gives the same bits and the GPU tests
(test_flat_passes_gpu.py) compare bit for bit:

  * int8: small integers (|v| <= 3) with one element of magnitude 127 per row, times a per-row 2^e, e in
    {-1, 0, 1}.  max|x| = 127 * 2^e, so scale = max|x| / 127 = 2^e exactly, the codes are the integers and the
    residual is 0.  |sum of code products| < 2^15 and every norm, 2 q.x - |x|^2 and key is an integer multiple of
    1/4 below 2^22: all within fp32's 24 bits.
  * bf16: integers |v| <= 8 (exact in bf16), d <= 256: every dot product and norm is an integer below 2^15.
  * clamp rows: a row equal to its query whose rounded image is longer than the row itself, so the scan's
    |q|^2 + |x|^2 - 2 q^.x^ is negative (still exact) and the L2 clamp at 0 decides the key.

The model restates the kernels' arithmetic twice: in float64 / int64 (exact by construction) and in float32
following the kernel's operations; test_flat_pass_cases.py asserts they agree bit for bit and that every
intermediate fits 24 significant bits.
"""
from __future__ import annotations

import numpy as np

L2, IP = 0, 1
TILE = 256  # rows per database tile and queries per block
PAD_KEY = np.float32(np.inf)
PAD_ROW = np.int32(0x7FFFFFFF)
F32 = np.float32


# ---- number formats ---------------------------------------------------------------------------------------------
def bf16_bits(x: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even bf16 of finite float32 values, as uint16 bit patterns."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u >> 16) & 1) + 0x7FFF
    return ((u + r) >> 16).astype(np.uint16)


def bf16_round(x: np.ndarray) -> np.ndarray:
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32).reshape(np.shape(x))


def i8_scale(X: np.ndarray) -> np.ndarray:
    """Per-row scale max|x| / 127 in float32 (0 for a zero row or one with a non-finite maximum)."""
    X = np.asarray(X, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        m = np.fmax.reduce(np.abs(X), axis=1, initial=np.float32(0)).astype(np.float32)
    s = (m / np.float32(127.0)).astype(np.float32)
    return np.where((m > 0) & (m < np.float32(3.0e38)), s, np.float32(0)).astype(np.float32)


def i8_codes(X: np.ndarray, s: np.ndarray) -> np.ndarray:
    """clip(rint(x / s), +-127) with the float32 division the kernel performs; 0 where s = 0; -127 for a NaN."""
    X = np.asarray(X, dtype=np.float32)
    sd = np.where(s > 0, s, np.float32(1)).astype(np.float32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.clip(np.rint((X / sd).astype(np.float32)), -127, 127)
    c = np.where(np.isnan(c), -127, c)  # fminf(fmaxf(NaN, -127), 127): the NaN operand is dropped
    return np.where(s[:, None] > 0, c, 0).astype(np.int8)


def i8_nk(d: int) -> int:
    nk = (d + 63) // 64
    return nk + (nk & 1)


def b16_nk(d: int) -> int:
    return (d + 31) // 32


def tiled_image(V: np.ndarray, n: int, d: int, R: int, per_unit: int, nk: int) -> np.ndarray:
    """The documented layout: unit u = ((t*nk + kc)*4 + c)*R + (row ^ 2c) holds dims (4*kc + c)*per_unit .. of
    row t*R + row, zero past n and past d.  V: n x d values; returns [ntiles, nk, 4, R, per_unit]."""
    ntiles = max((n + R - 1) // R, 1)
    P = np.zeros((ntiles * R, nk * 4 * per_unit), dtype=V.dtype)
    P[:n, :d] = V
    P = P.reshape(ntiles, R, nk, 4, per_unit).transpose(0, 2, 3, 1, 4)  # [t, kc, c, row, i]
    out = np.zeros_like(P)
    rows = np.arange(R)
    for c in range(4):
        out[:, :, c, rows ^ (2 * c), :] = P[:, :, c, rows, :]
    return np.ascontiguousarray(out)


# ---- builders of exact data -------------------------------------------------------------------------------------
def exact_i8_rows(rng: np.random.Generator, n: int, d: int) -> np.ndarray:
    V = rng.integers(-3, 4, size=(n, d)).astype(np.int64)
    V[np.arange(n), rng.integers(0, d, size=n)] = 127 * rng.choice([-1, 1], size=n)
    e = rng.integers(-1, 2, size=n)
    return (V * np.exp2(e)[:, None]).astype(np.float32)


def exact_bf16_rows(rng: np.random.Generator, n: int, d: int) -> np.ndarray:
    return rng.integers(-8, 9, size=(n, d)).astype(np.float32)


def exact_rows(rng, n: int, d: int, i8: bool) -> np.ndarray:
    return exact_i8_rows(rng, n, d) if i8 else exact_bf16_rows(rng, n, d)


def clamp_row(d: int, i8: bool) -> np.ndarray:
    """A row whose image is longer than the row: against itself the scan's L2 expression is negative and exact."""
    x = np.zeros(d, dtype=np.float32)
    if i8:  # 1.5 quantises to 2 (scale 1): q^.x^ = 127^2 + 4j against |x|^2 = 127^2 + 2.25j (needs d >= 2)
        x[: min(d, 9)] = 1.5
        x[0] = 127.0
    else:  # 259 rounds to 260 in bf16 (8 significant bits, ties to even): integers still
        x[: min(d, 4)] = 259.0
    return x


def distinct_rows(rng: np.random.Generator, t: int) -> np.ndarray:
    """t distinct row ids below 2^31 - 1, in random order."""
    r = np.unique(rng.integers(0, 2 ** 31 - 2, size=2 * t + 16))
    assert len(r) >= t
    return rng.permutation(r)[:t].astype(np.int32)


def with_ties(rng: np.random.Generator, base: np.ndarray, n: int) -> np.ndarray:
    """n rows drawn as three copies of each of ceil(n/3) base rows, shuffled: every key value occurs in runs of
    three, so the k-th and (k+1)-th smallest tie for every k that is not a multiple of 3."""
    m = (n + 2) // 3
    X = np.concatenate([base[:m]] * 3)[:n]
    return X[rng.permutation(n)]


# ---- keys -------------------------------------------------------------------------------------------------------
def fits24(x: np.ndarray) -> bool:
    x = np.asarray(x, dtype=np.float64)
    return bool(np.all(x.astype(np.float32).astype(np.float64) == x))


def operands(X: np.ndarray, i8: bool):
    """(integer-or-bf16 image values as float64, per-row scale as float64) of the scan's operand."""
    if i8:
        s = i8_scale(X)
        return i8_codes(X, s).astype(np.float64), s.astype(np.float64)
    return bf16_round(X).astype(np.float64), np.ones(len(X))


def keys_exact(Q: np.ndarray, X: np.ndarray, metric: int, i8: bool, parts: dict | None = None) -> np.ndarray:
    """The scan's keys in float64: L2 max(0, |q|^2 - (2 q^.x^ - |x|^2)), IP -q^.x^, with the norms of the fp32 rows
    and the product of the images.  parts (optional) receives every intermediate for the 24-bit check."""
    qv, qs = operands(Q, i8)
    xv, xs = operands(X, i8)
    acc = qv @ xv.T
    dot = acc * qs[:, None] * xs[None, :]
    qn = (Q.astype(np.float64) ** 2).sum(1)
    xn = (X.astype(np.float64) ** 2).sum(1)
    if metric == L2:
        s = 2.0 * dot - xn[None, :]
        key = np.maximum(0.0, qn[:, None] - s)
    else:
        s = 2.0 * dot
        key = -0.5 * s
    if parts is not None:
        parts.update(acc=acc, dot=dot, qn=qn, xn=xn, s=s, key=key, qscale=qs, xscale=xs)
    return key


def keys_fp32(Q: np.ndarray, X: np.ndarray, metric: int, i8: bool) -> np.ndarray:
    """The same keys by the kernel's own float32 operations (the epilogue of flat_bf16_k64): v = float(acc),
    s = fma(2 s_q s_x, v, -|x|^2), key = |q|^2 - s clamped at 0 (L2) or -0.5 s (IP).  Every product and sum below is
    exact on the builders' data, so the fma's single rounding and this two-step form agree."""
    qv, qs = operands(Q, i8)
    xv, xs = operands(X, i8)
    v = (qv @ xv.T).astype(np.float32)
    qn = np.zeros(len(Q), dtype=np.float32)
    xn = np.zeros(len(X), dtype=np.float32)
    if metric == L2:
        for e in range(Q.shape[1]):  # a sequential float32 sum (any order is exact here)
            qn = (qn + Q[:, e] * Q[:, e]).astype(np.float32)
            xn = (xn + X[:, e] * X[:, e]).astype(np.float32)
    c = ((F32(2.0) * qs.astype(np.float32))[:, None] * xs.astype(np.float32)[None, :]).astype(np.float32)
    s = (c * v - xn[None, :]).astype(np.float32)
    if metric == L2:
        key = (qn[:, None] - s).astype(np.float32)
        return np.where(key < 0, F32(0), key).astype(np.float32)
    return (F32(-0.5) * s).astype(np.float32)


def keys_model(Q, X, metric: int, i8: bool) -> np.ndarray:
    """float32 keys of exact data (asserts they are exact)."""
    k = keys_exact(Q, X, metric, i8)
    assert fits24(k)
    return (k + 0.0).astype(np.float32)


# ---- one pass ---------------------------------------------------------------------------------------------------
def pass_rows(N: int, nsplit: int, tps: int, tile_begin: int, tile_end: int, split: int):
    """Row range [r0, r1) that a pass scans in `split`: tiles [ts + tile_begin, min(ts + tile_end, ts + tps,
    ntiles)), rows below N."""
    ntiles = (N + TILE - 1) // TILE
    ts = split * tps
    t0 = ts + tile_begin
    t1 = min(ts + min(tile_end, tps), ntiles)
    if t1 <= t0:
        return 0, 0
    return min(t0 * TILE, N), min(t1 * TILE, N)


def pass_mask(K: np.ndarray, T: np.ndarray, nsplit: int, tps: int, tile_begin: int, tile_end: int) -> np.ndarray:
    """admit[q, row]: the rows a pass appends for query q (key <= T inclusive, inside the pass's tiles)."""
    nq, N = K.shape
    inside = np.zeros(N, dtype=bool)
    for s in range(nsplit):
        r0, r1 = pass_rows(N, nsplit, tps, tile_begin, tile_end, s)
        inside[r0:r1] = True
    with np.errstate(invalid="ignore"):
        return (K <= np.asarray(T, dtype=np.float32)[:, None]) & inside[None, :]


def split_of_rows(N: int, tps: int) -> np.ndarray:
    return (np.arange(N) // TILE) // tps


def cell_counts(admit: np.ndarray, nsplit: int, tps: int) -> np.ndarray:
    """cand_n[q, split] of an admitted mask: counts keep counting whatever the capacity."""
    nq, N = admit.shape
    so = split_of_rows(N, tps)
    out = np.zeros((nq, nsplit), dtype=np.int64)
    for s in range(nsplit):
        out[:, s] = admit[:, so == s].sum(1)
    return out


def cells_from_mask(K: np.ndarray, admit: np.ndarray, nsplit: int, tps: int, cap: int):
    """Candidate buffers (cand_d, cand_i, cand_n) holding the admitted rows in row order (one valid order of many)."""
    nq, N = K.shape
    so = split_of_rows(N, tps)
    cd = np.full((nq, nsplit, cap), np.nan, dtype=np.float32)
    ci = np.full((nq, nsplit, cap), -1, dtype=np.int32)
    cn = cell_counts(admit, nsplit, tps).astype(np.int32)
    for q in range(nq):
        rows = np.flatnonzero(admit[q])
        for s in np.unique(so[rows]):
            r = rows[so[rows] == s][:cap]
            cd[q, s, : len(r)] = K[q, r]
            ci[q, s, : len(r)] = r
    return cd, ci, cn


# ---- bound and select -------------------------------------------------------------------------------------------
def widen(t: np.ndarray) -> np.ndarray:
    """The bound's margin: max(t (1 + 2^-20), t + 2^-100) in float32; +inf stays +inf."""
    t = np.asarray(t, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.maximum((t * F32(1.0 + 2.0 ** -20)).astype(np.float32), (t + F32(2.0 ** -100)).astype(np.float32))
    return np.where(np.isinf(t) & (t > 0), t, w).astype(np.float32)


def kth_bound(keys: np.ndarray, k: int) -> np.ndarray:
    """widen(k-th smallest of each row of keys) — the seed bound of a sample's dense keys."""
    return widen(np.sort(keys, axis=1)[:, k - 1])


def _entries(cd, ci, cn, q, cap):
    ks, rs = [], []
    for s in range(cd.shape[1]):
        n = min(int(cn[q, s]), cap)
        ks.append(cd[q, s, :n])
        if ci is not None:
            rs.append(ci[q, s, :n])
    k = np.concatenate(ks) if ks else np.zeros(0, np.float32)
    r = np.concatenate(rs) if rs else None
    return k, r


def bound_model(cd: np.ndarray, cn: np.ndarray, k: int, bound: np.ndarray) -> np.ndarray:
    """flat_cand_bound: min(bound, widen(k-th smallest buffered key)); fewer than k entries leave the bound."""
    nq, nsplit, cap = cd.shape
    out = np.array(bound, dtype=np.float32, copy=True)
    for q in range(nq):
        keys, _ = _entries(cd, None, cn, q, cap)
        if len(keys) >= k:
            t = widen(np.sort(keys + F32(0.0))[k - 1 : k])[0]
            out[q] = np.fmin(out[q], t)
    return out


def select_model(cd: np.ndarray, ci: np.ndarray, cn: np.ndarray, k: int):
    """flat_cand_select: the k best (key, row) ascending with (+inf, 0x7fffffff) pads; a query with an overflowed
    cell gets an all-pad list and one entry in flagged.  Returns (out_d, out_i, sorted flagged queries)."""
    nq, nsplit, cap = cd.shape
    od = np.full((nq, k), PAD_KEY, dtype=np.float32)
    oi = np.full((nq, k), PAD_ROW, dtype=np.int32)
    flagged = []
    for q in range(nq):
        if (cn[q] > cap).any():
            flagged.append(q)
            continue
        keys, rows = _entries(cd, ci, cn, q, cap)
        keys = keys + F32(0.0)  # -0 and +0 are one key
        o = np.lexsort((rows, keys))[:k]
        od[q, : len(o)] = keys[o]
        oi[q, : len(o)] = rows[o]
    return od, oi, np.array(flagged, dtype=np.int32)


def brute_topk(K: np.ndarray, k: int):
    nq, N = K.shape
    od = np.full((nq, k), PAD_KEY, dtype=np.float32)
    oi = np.full((nq, k), PAD_ROW, dtype=np.int32)
    rows = np.arange(N)
    for q in range(nq):
        o = np.lexsort((rows, K[q] + F32(0.0)))[:k]
        od[q, : len(o)] = K[q, o] + F32(0.0)
        oi[q, : len(o)] = o
    return od, oi


def compose_model(K: np.ndarray, k: int, nsplit: int, tps: int, bounds, sample: int, cap: int):
    """The bounded passes end to end on a key matrix: seed = widen(k-th of the first `sample` rows' keys), then for
    each pass [bounds[p], bounds[p+1]) of every split: admit under the bound (resuming the buffers), re-bound.
    Returns (out_d, out_i, flagged, cand_n)."""
    nq, N = K.shape
    T = kth_bound(K[:, :sample], k)
    admit = np.zeros((nq, N), dtype=bool)
    for p in range(len(bounds) - 1):
        admit |= pass_mask(K, T, nsplit, tps, bounds[p], bounds[p + 1])
        cd, ci, cn = cells_from_mask(K, admit, nsplit, tps, cap)
        if p + 2 < len(bounds):
            T = bound_model(cd, cn, k, T)
    od, oi, fl = select_model(cd, ci, cn, k)
    return od, oi, fl, cn


# ---- the plan ---------------------------------------------------------------------------------------------------
def expected_fill(bounds, nsplit: int, sample: int, k: int) -> float:
    """Expected candidates per (query, split) cell of a plan: pass 0 admits k rows0 / S, pass p k rows_p /
    (nsplit rows_<p)."""
    fill = k * bounds[1] * TILE / sample
    for p in range(1, len(bounds) - 1):
        fill += k * (bounds[p + 1] - bounds[p]) / (bounds[p] * nsplit)
    return fill


# ---- case tables (shared by the CPU and GPU tests) -------------------------------------------------------------
IMAGE_D = [1, 15, 16, 17, 63, 64, 65, 128, 129, 150, 300, 1024]
IMAGE_N = [1, 255, 256, 257, 700]
KEYS_NQ = [256, 257, 320]
KEYS_N = [256, 512, 1280]
KEYS_D_I8 = [64, 129, 300, 448, 640, 768, 832, 900, 1024]  # ns = 1 .. 8 (832: ns = 7)
KEYS_D_B16 = [33, 64, 97, 128, 161, 192, 256]  # ceil(d / 32) even, ns = 1 .. 4
FILTER_N = [1, 255, 256, 257, 700, 1280, 1793]
FILTER_D = {True: [64, 129, 300], False: [64, 128, 192]}  # ns = 1, 2, 3 for either image


def steps_per_tile(d: int, i8: bool) -> int:
    return (i8_nk(d) if i8 else b16_nk(d)) // 2


def filter_geometries(N: int):
    """(nsplit, tps) of a table: one split, one tile per split, two splits with a short last one."""
    nt = (N + TILE - 1) // TILE
    g = [(1, nt), (nt, 1), (2, (nt + 1) // 2)]
    out = []
    for x in g:
        if x not in out:
            out.append(x)
    return out


def filter_bounds(K: np.ndarray) -> np.ndarray:
    """Per-query T by kind q % 5: a low quantile plus 1/8 (between two keys), exactly a key, below every key, -inf,
    +inf.  The kernel compares s >= |q|^2 - T; every finite T here is a multiple of 1/8 below 2^19 (the third kind
    is the smallest key minus 1), so that difference is exact and the compare is key <= T."""
    nq, N = K.shape
    srt = np.sort(K, axis=1)
    T = np.empty(nq, dtype=np.float32)
    for q in range(nq):
        kind = q % 5
        if kind == 0:
            T[q] = srt[q, min(N - 1, max(N // 16, 1))] + F32(0.125)
        elif kind == 1:
            T[q] = srt[q, min(N - 1, 3 + q % 7)]
        elif kind == 2:
            T[q] = srt[q, 0] - F32(1.0)
        elif kind == 3:
            T[q] = -np.inf
        else:
            T[q] = np.inf
    return T
