"""CPU checks of the IVF int8 image's L2 certificate (tests/_i8cert.py: the numpy restatement of the quantiser, the
scan's lower-bound key and the rerank's certificate).

Soundness: the scan key is a lower bound of ‖q̂ − x‖² for the dequantised query q̂, and sqrt(key) − ‖q − q̂‖ is a lower
bound of ‖q − x‖ — the two facts the certificate rests on — on random, widely scaled, zero and duplicate rows.
Input check: the emulation certifies the dense-but-certifying input of tests/test_ivf_i8_cert_gpu.py within the cap
that test puts on the device's flag count, so a failure there is the device's, not the input's.
"""
from __future__ import annotations

import numpy as np
import pytest

import _i8cert as C

# key_lb ≤ ‖q̂ − x‖²·(1 + margin): the key's fp32 roundings (two norm sums of d terms, two fmas) relative to the
# distance.  The residual and norm factors carry ×1.0001 each, so the key sits below the exact bound by about
# 2·10⁻⁴·2‖q̂‖·r_x, which absorbs the roundings' absolute part wherever the norms cancel (q ≈ x).
KEY_MARGIN = 1e-5


def _rows(kind, rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    if kind == "scaled":
        x *= (10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)
    elif kind == "zero":
        x[::5] = 0
    elif kind == "duplicate":
        x[1::2] = x[::2]
    return x


@pytest.mark.parametrize("kind", ["random", "scaled", "zero", "duplicate"])
@pytest.mark.parametrize("d", [100, 128, 768])
def test_lower_bound_key_is_sound(kind, d):
    rng = np.random.default_rng(d + len(kind))
    xb = _rows(kind, rng, 600, d)
    xq = rng.standard_normal((40, d)).astype(np.float32)
    if kind == "scaled":
        xq *= (10.0 ** rng.uniform(-2, 2, (40, 1))).astype(np.float32)
    if kind == "duplicate":
        xq[:20] = xb[:40:2]  # queries equal to stored rows
    if kind == "zero":
        xq[3] = 0
    xu, xs, xres, _ = C.quantise(xb)
    xn2 = np.sum(xb * xb, axis=1, dtype=np.float32)
    qu, qs, qres, qh2 = C.quantise(xq)
    key = C.lower_bound_keys(qu, qs, qh2, xu, xs, xres, xn2).astype(np.float64)
    qhat = qs.astype(np.float64)[:, None] * qu.astype(np.float64)
    x64, q64 = xb.astype(np.float64), xq.astype(np.float64)
    d_hat = ((qhat[:, None, :] - x64[None, :, :]) ** 2).sum(-1)
    d_true = np.sqrt(((q64[:, None, :] - x64[None, :, :]) ** 2).sum(-1))
    assert (key <= d_hat * (1 + KEY_MARGIN)).all(), float(np.max(key - d_hat * (1 + KEY_MARGIN)))
    # the residual the device keeps is an upper bound of the true one
    assert (qres >= np.sqrt(((q64 - qhat) ** 2).sum(-1))).all()
    lhs = np.sqrt(key) - qres.astype(np.float64)[:, None]
    assert (lhs <= d_true * (1 + KEY_MARGIN)).all(), float(np.max(lhs - d_true))


def test_certificate_passes_on_the_gpu_tests_certifying_input():
    """n 60 000, d 128, intrinsic dimension 4, noise 0.02, nlist 64, nprobe 8, 128 queries, k 10: at least 126 of
    the 128 queries certify in the emulation (the GPU test allows the device 2 flagged queries)."""
    xb, xq = C.lowrank_case(60_000, 128, 4, 0.02, 128, seed=5)
    cen, off, ids, codes = C.ivf_lists(xb, 64)
    ok = C.emulate(cen, off, codes, xq, 10, 8)
    print("certified", int(ok.sum()), "of", len(ok))
    assert ok.sum() >= 126, int(ok.sum())
