"""The oracle's k-means (oracle_kmeans_train) against the summation-order-free integer reference (_kmeans_ref.py).

On integer-valued rows nothing rounds, so the two must agree bit for bit, centroids and sizes, over the whole Tier A
case table (d 1 … 768 — beyond one term per lane of km_dist64 —, nlist 1 … 1024, more than 65536 training rows, the
stride sample and the 256·nlist subset, fewer distinct rows than centres), at niter 0 and 1 and both inits.  This ties
the oracle, to which tests/test_ivf_train_shapes_gpu.py and the committed fixtures pin the GPU, to something that
shares no code with it."""
from __future__ import annotations

import numpy as np
import pytest

from _kmeans_ref import (CASE_FEW_DISTINCT, KM_SEED, TIER_A_CASES, TIER_B_CASES, TIER_B_NITER, TIER_B_SEED, SplitMix64,
                         assignment_margin, case_id, case_inits, case_ref, case_rows, margin_tau, mixture_rows,
                         ref_train_int, tier_b_id, training_margin, training_rows)


@pytest.mark.parametrize("niter", [0, 1])
@pytest.mark.parametrize("case", TIER_A_CASES, ids=case_id)
def test_reference_equals_oracle(oracle, case, niter):
    _, _, nlist, ts, _ = case
    x = case_rows(case)
    for init in case_inits(case):
        cen_r, sizes_r, info = case_ref(case, niter, init)
        cen_o, sizes_o = oracle.kmeans_train(x, nlist, 0, ts, niter, KM_SEED, init)
        assert np.array_equal(sizes_o, sizes_r), (init, sizes_o, sizes_r)
        assert np.array_equal(cen_o, cen_r), (init, float(np.abs(cen_o - cen_r).max()))
        assert sizes_r.sum() == (info["m"] if niter else 0)


def test_reference_ip_init_equals_oracle(oracle):
    """niter = 0 with IP: the renormalised init."""
    case = (1031, 65, 7, 0, 3)
    for init in (0, 1):
        cen_r, sizes_r = ref_train_int(case_rows(case), 7, 0, 0, KM_SEED, init, metric=1)
        cen_o, sizes_o = oracle.kmeans_train(case_rows(case), 7, 1, 0, 0, KM_SEED, init)
        assert np.array_equal(cen_o, cen_r) and np.array_equal(sizes_o, sizes_r)
        assert np.allclose((cen_r.astype(np.float64) ** 2).sum(1), 1.0, atol=1e-6)


@pytest.mark.parametrize("case", TIER_B_CASES, ids=tier_b_id)
def test_tier_b_margin_holds(oracle, case):
    """The float-row cases of test_ivf_train_shapes_gpu.py keep their margin above τ (checked here without a GPU, so
    a change of the data or of the oracle shows before the GPU run), with the 10× room asked of a chosen seed."""
    m, d, nlist, metric, seed = case
    x = mixture_rows(m, d, nlist, seed)
    margin = training_margin(oracle.kmeans_train, x, nlist, metric, TIER_B_NITER, TIER_B_SEED, 1)
    assert margin >= 10 * margin_tau(d), (margin, margin_tau(d))


def test_tier_b_margin_rejects_a_doubled_component(oracle):
    """What the margin assertion guards against: with data seed 1300 at d = 300 k-means++ puts two centres into one
    component, rows sit between them, and the margin falls below τ."""
    x = mixture_rows(1031, 300, 7, 1300)
    assert training_margin(oracle.kmeans_train, x, 7, 0, TIER_B_NITER, TIER_B_SEED, 1) < margin_tau(300)


def test_training_rows_sampling():
    rows = training_rows(2000, 1999, 64, SplitMix64(1))  # stride 2000/1999: floor(i·stride) = i for every i < 1999
    assert np.array_equal(rows, np.arange(1999))
    rows = training_rows(50_000, 1000, 3, SplitMix64(1))  # stride 50, then 768 of the 1000
    assert len(rows) == 768 and np.all(rows % 50 == 0) and np.all(np.diff(rows) > 0) and rows[-1] > 40_000
    rows = training_rows(3000, 2500, 4, SplitMix64(1))  # the stride sample, then 1024 of its 2500 rows, ascending
    assert len(rows) == 1024 and np.all(np.diff(rows) > 0)
    assert np.isin(rows, (np.arange(2500) * (3000 / 2500)).astype(np.int64)).all()
    for ts in (0, 300, 301):  # 0, n and n + 1 all mean every row
        assert np.array_equal(training_rows(300, ts, 7, SplitMix64(1)), np.arange(300))


def test_few_distinct_rows_reach_zero_weights():
    """The k-means++ run on 9 distinct rows for 40 centres: after the distinct rows are used up every D² is 0 and the
    pick is r mod m, which the reference must take like the oracle (covered above); here the precondition itself."""
    _, _, info = case_ref(CASE_FEW_DISTINCT, 1, 1)
    assert info["distinct"] == 9 and info["empty"] == 31


def test_assignment_margin():
    x = np.array([[0.0, 0.0], [3.0, 0.0], [1.25, 0.0]], np.float32)
    cen = np.array([[0.0, 0.0], [2.0, 0.0]], np.float32)
    # L2: row 2 is the closest call: distances 1.5625 and 0.5625, scale max(1.5625 + 0, 1.5625 + 4)
    assert assignment_margin(x, cen, 0) == pytest.approx(1.0 / 5.5625)
    assert assignment_margin(x, cen[:1], 0) == float("inf")
    assert assignment_margin(x, np.vstack([cen, cen[1:]]), 0) == 0.0  # a duplicated centroid is a tie
    xi = np.array([[1.0, 2.0], [2.0, -1.0]], np.float32)
    ci = np.array([[1.0, 0.0], [0.0, 1.0]], np.float32)
    # IP: row 0 products 1 and 2, scales 1 and 2 → 1/2; row 1 products 2 and −1, scales 2 and 1 → 3/2
    assert assignment_margin(xi, ci, 1) == pytest.approx(0.5)
