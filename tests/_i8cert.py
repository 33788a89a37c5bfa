"""The IVF int8 image's L2 certificate restated in numpy (csrc/ivf_mfma.hip, csrc/ivf_kernels.hip): the quantiser
(one scale per row, s = max|x| / 127, units clamp(rint(x / s), ±127)), the scan's lower-bound key and the rerank's
certificate, with the scan's sub-list structure (8 waves per 2048-row chunk, each keeping its 16 best keys, a 64-deep
merged filter).  Shared by tests/test_ivf_i8_cert.py (CPU) and tests/test_ivf_i8_cert_gpu.py.

Data generator of both: rows on a random r-dimensional subspace of R^d plus isotropic noise,
B = qr(normal(d, r))[0].T · sqrt(d / r) / 3, rows = normal(n, r) @ B + eta · normal(n, d) (fp32), the queries drawn
the same way after the rows; lists as tests/test_request_k_gpu.py::_ivf builds them.
"""
from __future__ import annotations

import numpy as np

from _data import build_ivf_lists

F = np.float32
UP = F(1.0001)            # the fp32 residual / norm sums' margin (the kernels' ×1.0001)
MARGIN = 2.0 ** -20       # the certificate's multiplicative margin
SUBLISTS, SUB_K, FILTER_K, CHUNK, PASS = 8, 16, 64, 2048, 32


def lowrank_case(n, d, r, eta, nq, seed):
    rng = np.random.default_rng(seed)
    B = np.linalg.qr(rng.standard_normal((d, r)))[0].T * (np.sqrt(d / r) / 3)
    xb = (rng.standard_normal((n, r)) @ B + eta * rng.standard_normal((n, d))).astype(F)
    xq = (rng.standard_normal((nq, r)) @ B + eta * rng.standard_normal((nq, d))).astype(F)
    return np.ascontiguousarray(xb), np.ascontiguousarray(xq)


def ivf_lists(xb, nlist, metric=0):
    cen = np.ascontiguousarray(xb[:: len(xb) // nlist][:nlist])
    off, ids, codes = build_ivf_lists(xb, cen, metric)
    return cen, off, ids, codes


def quantise(x):
    """Rows → (units as fp32 integers, scale, residual ‖x − s·x̂‖·1.0001 (+inf for a non-finite row), ‖s·x̂‖²)."""
    x = np.ascontiguousarray(x, F)
    mx = np.max(np.abs(x), axis=1)
    fin = np.isfinite(mx)
    s = np.where(fin & (mx > 0), mx / F(127), F(0)).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(s[:, None] > 0, np.clip(np.rint(x / s[:, None]), -127, 127), 0).astype(F)
    deq = (s[:, None] * u).astype(F)
    res = np.where(fin, np.sqrt(np.sum((x - deq) ** 2, axis=1, dtype=F)) * UP, F(np.inf)).astype(F)
    return u, s, res, np.sum(deq * deq, axis=1, dtype=F)


def lower_bound_keys(qu, qs, qh2, xu, xs, xres, xn2):
    """The scan's L2 key of every (query, row) pair in fp32:
    max(0, ‖q̂‖² + ‖x‖² − 2·s_q·s_x·Σq̂₈x̂₈ − 2‖q̂‖·r_x), the sum exact (int32 on the device)."""
    dot = (qu.astype(np.float64) @ xu.astype(np.float64).T).astype(F)  # exact: |sum| < 2^24 for d <= 1040
    qhn = (np.sqrt(qh2) * UP).astype(F)
    key = (qh2[:, None] + xn2[None, :]).astype(F)
    key = (F(-2) * (qs[:, None] * xs[None, :]) * dot + key).astype(F)
    key = (-(F(2) * qhn)[:, None] * xres[None, :] + key).astype(F)
    return np.maximum(key, F(0))


def fp_slack(d, qn2, xmax2):
    """The certificate's rounding term: fp32 rounding of the key's norms and sums and of the reranked direct
    distance, (d + 8)·2⁻²⁴·2(‖q‖² + max‖x‖²)·1.01 (the bound every exact form of ivf_rerank_topk carries)."""
    return 1.01 * (d + 8) * 2.0 ** -24 * 2.0 * (qn2 + xmax2)


def certified(dk, rq, bound, slack):
    """sqrt(d_k) + ‖q − q̂‖ < sqrt((B − E)·(1 − margin)), with the device's guard factor on the left side."""
    return (np.sqrt(max(dk, 0.0)) + rq) * (1 + MARGIN) < np.sqrt(max((bound - slack) * (1 - MARGIN), 0.0))


def emulate(cen, off, codes, xq, k, nprobe):
    """Per query: whether the device would certify it.  The probe lists are the exact nearest centroids; the scan
    keeps, per (probed list, 2048-row chunk, wave), the 16 smallest keys of the wave's 32-row passes; T_sub is the
    smallest 16th key of a full sub-list, the candidates are the sub-list entries below it, the filter their 64
    smallest, B = min(64th key, T_sub)."""
    xu, xs, xres, _ = quantise(codes)
    xn2 = np.sum(codes * codes, axis=1, dtype=F)
    qu, qs, qres, qh2 = quantise(xq)
    xmax2 = float(xn2.max())
    d = codes.shape[1]
    c2 = np.sum(cen.astype(np.float64) ** 2, 1)
    out = np.zeros(len(xq), bool)
    for qi in range(len(xq)):
        q64 = xq[qi].astype(np.float64)
        probes = np.argsort(c2 - 2.0 * (cen.astype(np.float64) @ q64), kind="stable")[:nprobe]
        keys, rows, tsub = [], [], np.inf
        for l in probes:
            r0, r1 = int(off[l]), int(off[l + 1])
            if r1 == r0:
                continue
            kl = lower_bound_keys(qu[qi:qi + 1], qs[qi:qi + 1], qh2[qi:qi + 1], xu[r0:r1], xs[r0:r1], xres[r0:r1],
                                  xn2[r0:r1])[0]
            j = np.arange(r1 - r0)
            sub = (j // CHUNK) * SUBLISTS + ((j % CHUNK) // PASS) % SUBLISTS
            for sl in np.unique(sub):
                m = np.nonzero(sub == sl)[0]
                o = m[np.argsort(kl[m], kind="stable")[:SUB_K]]
                if len(m) >= SUB_K:
                    tsub = min(tsub, float(kl[o[-1]]))
                keys.append(kl[o])
                rows.append(r0 + o)
        if not keys:
            out[qi] = True
            continue
        keys, rows = np.concatenate(keys), np.concatenate(rows)
        keep = keys < tsub
        keys, rows = keys[keep], rows[keep]
        o = np.argsort(keys, kind="stable")[:FILTER_K]
        bound = min(float(keys[o[-1]]) if len(o) == FILTER_K else np.inf, tsub)
        ex = np.sort(np.sum((codes[rows[o]].astype(np.float64) - q64) ** 2, 1))
        if len(ex) < k:  # fewer candidates than k: nothing below the bounds was pruned iff they are infinite
            out[qi] = not np.isfinite(bound)
            continue
        out[qi] = not np.isfinite(bound) or certified(float(ex[k - 1]), float(qres[qi]), bound,
                                                      fp_slack(d, float(q64 @ q64), xmax2))
    return out
