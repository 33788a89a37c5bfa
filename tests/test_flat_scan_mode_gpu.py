"""What a real Flat search reports (hipann_last_search_path) equals what the host-only resolver hook returns for the
same inputs (tests/test_flat_scan_mode.py checks the hook against a hand-written table), one shape per path at the
smallest size that reaches it, d = 64; and every result equals the fp32 direct form's on the same index (form 0 in
chunks of 16 queries).

The data make that comparison an equality.  Rows and queries are small integers (rows in [-8, 8], queries of magnitude
4..8), so every product, norm and distance is an integer below 2^24: the direct form, the decomposed form and the split
forms all compute it exactly, in any order.  Each query has 12 planted rows: row t equals the query with its first t
coordinates one nearer to zero, so its L2 distance is t and its inner product ‖q‖² − Σ_{i<t}|q_i| — distinct and far
better than any random row (L2 ≈ ‖q‖² + ‖x‖² ≈ 4000; IP: ‖q‖² ≈ 2400 less at most 96, against a standard deviation of
≈ 240 for a random row).  The ten best are therefore planted rows without ties, the same for every form.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

from test_flat_scan_mode import BOUNDED, DIRECT, KEYS, LISTS, OUT, SMALL_I8

pytestmark = pytest.mark.gpu

D_, K, PLANT = 64, 10, 12
L2, IP = 0, 1
BIG = 8 * 65536


def planted_case(seed: int, n: int, nq: int):
    rng = np.random.default_rng(seed)
    xb = rng.integers(-8, 9, size=(n, D_)).astype(np.float32)
    xq = (rng.integers(4, 9, size=(nq, D_)) * rng.choice([-1, 1], size=(nq, D_))).astype(np.float32)
    rows = rng.permutation(n)[: nq * PLANT].reshape(nq, PLANT)
    for t in range(PLANT):
        x = xq.copy()
        x[:, :t] -= np.sign(x[:, :t])
        xb[rows[:, t]] = x
    return xb, xq, rows


def resolved(lib, nq, n, metric, form):
    env = lambda name: int(os.environ.get(name) or 1) != 0
    a = np.array([nq, n, D_, metric, K, K, form, 0, env("HIPANN_FLAT_I8_SMALL"), env("HIPANN_FLAT_BF16_SEED"),
                  env("HIPANN_I8_PREP_FUSED"), env("HIPANN_B16_K64")], np.int32)
    o = np.zeros(len(OUT), np.int32)
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.hipann_debug_flat_scan_mode(ip(a), len(a), ip(o), len(o)) == 0
    return dict(zip(OUT, (int(v) for v in o)))


def direct_reference(ix, xq):
    """The fp32 direct form on the same index: form 0, fewer than 20 queries per call."""
    form = ix.form
    ix.form = ix.FORM_FP32
    parts = [ix.search(xq[s:s + 16], K) for s in range(0, len(xq), 16)]
    ix.form = form
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def run_case(gpu, ix, xq, rows, metric, form, path):
    """One search on form `form`: the path is `path`, the report is the resolver's, the result the direct form's."""
    n, nq = ix.ntotal, len(xq)
    m = resolved(gpu.lib(), nq, n, metric, form)
    assert m["path"] == path, m
    ix.form = form
    before, fb0 = ix.last_search_path(), ix.rerank_fallbacks()
    D, I = ix.search(xq, K)
    if m["record"]:
        assert ix.last_search_path() == {"form": m["last_form"], "filter_k": m["last_kfilt"], "sublists": 0}, m
    else:
        assert ix.last_search_path() == before, m
    assert ix.rerank_fallbacks() == fb0  # planted neighbours stand clear of every filter's bound
    s0 = ix.host_syncs()
    D2, I2 = ix.search(xq, K)  # images built: one synchronisation, for the results
    assert ix.host_syncs() - s0 == 1, (m, ix.host_syncs() - s0)
    assert np.array_equal(I2, I) and np.array_equal(D2, D)
    assert np.array_equal(I, rows[:, :K]), m
    if path != DIRECT or form != 0:
        Dd, Id = direct_reference(ix, xq)
        assert np.array_equal(I, Id) and np.array_equal(D, Dd), m
    return m


@pytest.fixture(scope="module", params=[L2, IP], ids=["l2", "ip"])
def big(request, gpu):
    """524288 rows (134 MB), one index per metric for the module."""
    xb, xq, rows = planted_case(5, BIG, 256)
    ix = gpu.HipIndexFlat(D_, request.param, xb)
    yield ix, xq, rows, request.param
    ix.close()


@pytest.mark.parametrize("form", [4, 5])
def test_bounded_passes(gpu, big, form):
    ix, xq, rows, metric = big
    m = run_case(gpu, ix, xq, rows, metric, form, BOUNDED)
    assert (m["form"], m["last_kfilt"], m["i8"]) == (form, 64 if form == 5 else 32, int(form == 5))


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 32])
def test_keys_path_leaves_the_report_untouched(gpu, metric, nq):
    xb, xq, rows = planted_case(1, 1024, nq)
    ix = gpu.HipIndexFlat(D_, metric, xb)
    run_case(gpu, ix, xq, rows, metric, ix.form, KEYS)
    assert ix.last_search_path() == {"form": -1, "filter_k": 0, "sublists": 0}  # as at creation
    ix.close()


@pytest.mark.parametrize("metric", [L2, IP])
def test_direct_and_small_int8(gpu, metric):
    xb, xq, rows = planted_case(2, 2048, 4)
    ix = gpu.HipIndexFlat(D_, metric, xb)
    run_case(gpu, ix, xq, rows, metric, ix.form, DIRECT)
    ix.close()
    xb, xq, rows = planted_case(3, 65536, 4)
    ix = gpu.HipIndexFlat(D_, metric, xb)
    m = run_case(gpu, ix, xq, rows, metric, 5, SMALL_I8)
    assert (m["last_form"], m["last_kfilt"], m["rerun_form"]) == (5, 64, 0)
    run_case(gpu, ix, xq, rows, metric, 4, DIRECT)  # the int8 scan is form 5's only
    ix.close()


@pytest.mark.parametrize("metric", [L2, IP])
def test_list_paths(gpu, metric):
    xb, xq, rows = planted_case(4, 20000, 64)
    ix = gpu.HipIndexFlat(D_, metric, xb)
    for form in (0, 1, 2, 3):  # the GEMM lists
        m = run_case(gpu, ix, xq[:32], rows[:32], metric, form, LISTS)
        assert m["form"] == form and m["exact"] == int(form == 3)
    m = run_case(gpu, ix, xq, rows, metric, 4, LISTS)  # the bf16 list kernel
    assert (m["form"], m["last_kfilt"], m["seeded"]) == (4, 32, 0)
    ix.close()
