"""GPU IVF training (hipann_ivf_train / _device, csrc/ivf_train.hip) against exact references, across d, nlist and
batch edges — the shapes beyond the committed fixtures of test_ivf_train_gpu.py (all 6000 × 48).

Tier A — integer-valued rows, L2, niter 0 and 1, both inits: nothing rounds (tests/_kmeans_ref.py), so the GPU's
centroids and list sizes must be array_equal to the integer reference and to the oracle, ties included.  The table
(_kmeans_ref.TIER_A_CASES) reaches d >= 64 (a second lane-strided term in kpp_update), d > 256 (a second pass of the
row loops in km_sums / kpp_pick), odd d, nlist 1, 2, 3 and at and around 2^b (the radix sort's end_bit), more than
65536 training rows (a second and a third assignment batch), the stride sample and the 256·nlist subset, k-means++
with fewer distinct rows than centres (every D² zero: the pick is r mod m) and FAISS's split of up to 160 empty
clusters.  Each test recomputes the property of the data it depends on (distinct rows, empty clusters, the block a
k-means++ pick lands in) and asserts it, so a change of data cannot quietly stop it from reaching its path.

Tier B — float rows of a separated mixture, both metrics, k-means++ init, 6 iterations: bit-equal to the oracle under
an asserted margin.  On the oracle's centroids after every t < 6 iterations the relative gap between each row's
nearest and second nearest centroid (_kmeans_ref.assignment_margin) must be at least τ = 4·(d + 4)·2^-24, twice the
rounding error two fp32 distances can carry; then no assignment can differ, and the sums (fp64, row order) and the
finish are the same arithmetic on both sides.  τ is derived, not measured.  Data seeds and minimum margins (k-means
seed 1234; the seed is 1000 + d unless noted):

    m     d    nlist  seed   margin L2   margin IP   τ
    1031  3    7      3003   1.06e-01    4.19e-05    1.67e-06   (1003: 1.5e-05 / 2.4e-06, IP too thin;
                                                                  2003: 4.3e-06 / 3.4e-07, IP fails)
    1031  5    7      1005   7.95e-02    7.93e-02    2.15e-06
    1031  63   7      1063   7.25e-01    7.85e-01    1.60e-05
    1031  64   7      1064   5.74e-01    6.05e-01    1.62e-05
    1031  65   7      1065   6.01e-01    6.79e-01    1.65e-05
    1031  129  7      1129   6.53e-01    7.18e-01    3.17e-05
    1031  257  7      1257   8.62e-01    8.69e-01    6.22e-05
    1031  300  7      2300   8.69e-01    8.96e-01    7.25e-05   (1300: 6.9e-07 / 4.8e-07, two centres in one
                                                                  component: fails, as the assertion is there to show)
    1031  768  7      1768   8.75e-01    8.90e-01    1.84e-04
    4000  100  24     1100   5.75e-01    6.02e-01    2.48e-05
    1031  1    3      1001   4.57e-02    —           1.19e-06   (768 of the 1031 rows are trained on)
    1031  1    5      1001   1.37e-03    —           1.19e-06
    1031  2    3      1002   4.06e-01    —           1.43e-06   (768 of the 1031 rows are trained on)
    1031  2    5      1002   1.38e-02    —           1.43e-06

Tier C — the API surface: the device-pointer entry against the host one (stride sample far past m, a non-default
stream, niter 0), niter 0 (the init, renormalised for IP; sizes zero), and the argument errors, each followed by a
valid call that must still give the reference's result."""
from __future__ import annotations

import numpy as np
import pytest

from _kmeans_ref import (CASE_BATCH2, CASE_BATCH3, CASE_FEW_DISTINCT, CASE_STRIDE_DUP, CASE_STRIDE_SUBSET,
                         CASE_SUBSET_ODD_D, KM_SEED, TIER_A_CASES, TIER_B_CASES, TIER_B_NITER, TIER_B_SEED, case_id,
                         case_inits, case_ref, case_rows, margin_tau, mixture_rows, ref_train_int, tier_b_id,
                         training_margin)

pytestmark = pytest.mark.gpu

_ORACLE = {}


def oracle_train(oracle, case, niter, init):
    """The oracle on a Tier A case, computed once."""
    key = (case, niter, init)
    if key not in _ORACLE:
        _, _, nlist, ts, _ = case
        _ORACLE[key] = oracle.kmeans_train(case_rows(case), nlist, 0, ts, niter, KM_SEED, init)
    return _ORACLE[key]


def assert_exact(got, want, what):
    cen, sizes = got
    cen_w, sizes_w = want[0], want[1]
    assert np.array_equal(sizes, sizes_w), (what, "sizes", np.flatnonzero(sizes != sizes_w)[:8])
    assert np.array_equal(cen, cen_w), (what, "centroids", np.argwhere(cen != cen_w)[:8])


# what the table in the issue says each case reaches, recomputed from the reference: (init, key) -> value
PRECONDITIONS = {
    CASE_BATCH2: {(0, "m"): 65541, (0, "empty"): 34},
    CASE_BATCH3: {(0, "m"): 131073, (0, "empty"): 160},
    CASE_STRIDE_SUBSET: {(0, "m"): 1024, (1, "m"): 1024},
    CASE_SUBSET_ODD_D: {(0, "m"): 1024, (1, "m"): 1024},
    CASE_FEW_DISTINCT: {(0, "distinct"): 9, (0, "empty"): 31, (1, "empty"): 31},
    CASE_STRIDE_DUP: {(0, "m"): 1999, (0, "distinct"): 27, (0, "empty"): 40, (1, "empty"): 37},
}


# ---- Tier A ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("niter", [0, 1])
@pytest.mark.parametrize("case", TIER_A_CASES, ids=case_id)
def test_tier_a_exact(gpu, oracle, case, niter):
    _, _, nlist, ts, _ = case
    x = case_rows(case)
    for init in case_inits(case):
        ref = case_ref(case, niter, init)
        info = case_ref(case, 1, init)[2]
        for (i, key), want in PRECONDITIONS.get(case, {}).items():
            if i == init:
                assert info[key] == want, (init, key, info[key], want)
        got = gpu.ivf_train(x, nlist, 0, ts, niter, KM_SEED, init)
        assert_exact(got, ref, f"init {init}: GPU vs reference")
        assert_exact(got, oracle_train(oracle, case, niter, init), f"init {init}: GPU vs oracle")


def test_tier_a_zero_weights_pick(gpu):
    """k-means++ with 9 distinct rows for 40 centres: once every distinct row is a centre every D² is 0 (mx == 0 in
    kpp_pick) and the remaining centres are rows r mod m — duplicates of earlier ones."""
    cen, _, info = case_ref(CASE_FEW_DISTINCT, 0, 1)
    assert info["distinct"] == 9 and len(np.unique(cen, axis=0)) == 9
    first_dup = next(j for j in range(1, 40) if any(np.array_equal(cen[j], c) for c in cen[:j]))
    assert len(np.unique(cen[:first_dup], axis=0)) == 9  # the first duplicate comes only after all nine: D² all zero
    assert_exact(gpu.ivf_train(case_rows(CASE_FEW_DISTINCT), 40, 0, 0, 0, KM_SEED, 1), (cen, np.zeros(40, np.int64)),
                 "GPU vs reference")


def test_tier_a_train_sample_n_and_beyond(gpu):
    """train_sample = n and n + 1 both mean every row, like 0."""
    case = (300, 16, 3, 0, 3)
    for init in (0, 1):
        ref = case_ref(case, 1, init)
        for ts in (300, 301):
            assert_exact(gpu.ivf_train(case_rows(case), 3, 0, ts, 1, KM_SEED, init), ref, f"init {init} ts {ts}")


def test_tier_a_kpp_pick_every_block(gpu):
    """k-means++ picks over 8 seeds on 1031 × 65 (5 blocks of kpp_weights, the last with 7 rows): the picks made by
    kpp_pick land in every block, the last one included."""
    case = (1031, 65, 7, 0, 3)
    blocks = set()
    for seed in (24, 25, 26, 27, 28, 29, 30, 34):
        cen, sizes, info = case_ref(case, 0, 1, seed)
        blocks |= {p // 256 for p in info["pick"][1:]}  # pick[0] is drawn on the host
        assert_exact(gpu.ivf_train(case_rows(case), 7, 0, 0, 0, seed, 1), (cen, sizes), f"seed {seed}")
    assert blocks == {0, 1, 2, 3, 4}, blocks  # block 4: a row index >= 1024


# ---- Tier B ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TIER_B_CASES, ids=tier_b_id)
def test_tier_b_bit_equal_under_margin(gpu, oracle, case):
    m, d, nlist, metric, seed = case
    x = mixture_rows(m, d, nlist, seed)
    margin = training_margin(oracle.kmeans_train, x, nlist, metric, TIER_B_NITER, TIER_B_SEED, 1)
    print(f"{tier_b_id(case)}: margin {margin:.3e} tau {margin_tau(d):.3e}")
    assert margin >= margin_tau(d), (margin, margin_tau(d))
    want = oracle.kmeans_train(x, nlist, metric, 0, TIER_B_NITER, TIER_B_SEED, 1)
    assert want[1].min() > 0  # no empty cluster: every centroid is a mean
    assert_exact(gpu.ivf_train(x, nlist, metric, 0, TIER_B_NITER, TIER_B_SEED, 1), want, "GPU vs oracle")


# ---- Tier C ---------------------------------------------------------------------------------------------------
DEVICE_CASE = (50_000, 8, 3, 1000, 3)  # stride 50 to 1000 rows, then 768 of them: km_gather reads rows far past m


def _train_device(gpu, x, nlist, ts, niter, init, stream=None, metric=0):
    import torch

    xt = torch.from_numpy(np.array(x, np.float32)).cuda()  # a copy: the shared rows are read-only
    ct = torch.full((nlist, x.shape[1]), float("nan"), device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    gpu.ivf_train_device(x.shape[1], nlist, x.shape[0], xt.data_ptr(), ct.data_ptr(), metric, ts, niter, KM_SEED, init,
                         0, 0 if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return ct.cpu().numpy()


@pytest.mark.parametrize("niter", [0, 1])
@pytest.mark.parametrize("init", [0, 1])
def test_tier_c_device_api_equals_host_api(gpu, init, niter):
    import torch

    n, d, nlist, ts, hi = DEVICE_CASE
    x = case_rows(DEVICE_CASE)
    cen_r, sizes_r, info = case_ref(DEVICE_CASE, niter, init)
    assert info["m"] == 768
    host = gpu.ivf_train(x, nlist, 0, ts, niter, KM_SEED, init)
    assert_exact(host, (cen_r, sizes_r), "host API vs reference")
    assert np.array_equal(_train_device(gpu, x, nlist, ts, niter, init), host[0])  # the null stream
    assert np.array_equal(_train_device(gpu, x, nlist, ts, niter, init, torch.cuda.Stream()), host[0])


def test_tier_c_device_api_float_rows_on_a_stream(gpu):
    """The device entry on a caller's stream over float rows and 6 iterations equals the host entry bit for bit
    (the same kernels on the same training rows)."""
    import torch

    m, d, nlist, metric = 1031, 64, 7, 1
    x = mixture_rows(m, d, nlist, 1064)
    host, _ = gpu.ivf_train(x, nlist, metric, 0, TIER_B_NITER, KM_SEED, 1)
    assert np.array_equal(_train_device(gpu, x, nlist, 0, TIER_B_NITER, 1, torch.cuda.Stream(), metric), host)


@pytest.mark.parametrize("metric", [0, 1])
def test_tier_c_niter_zero_is_the_init(gpu, oracle, metric):
    """niter = 0: the centroids are the init's rows (for IP renormalised to unit length), the sizes all zero."""
    case = (1031, 65, 7, 0, 3)
    x = case_rows(case)
    for init in (0, 1):
        info: dict = {}
        cen_r, sizes_r = ref_train_int(x, 7, 0, 0, KM_SEED, init, metric=metric, info=info)
        got = gpu.ivf_train(x, 7, metric, 0, 0, KM_SEED, init)
        assert not got[1].any()
        assert_exact(got, (cen_r, sizes_r), "GPU vs reference")
        assert_exact(got, oracle.kmeans_train(x, 7, metric, 0, 0, KM_SEED, init), "GPU vs oracle")
        if metric == 0:
            assert np.array_equal(got[0], x[info["pick"]])
        else:
            assert np.allclose((got[0].astype(np.float64) ** 2).sum(1), 1.0, atol=1e-6)


ERROR_CALLS = {
    "d=0": dict(x=np.zeros((300, 0), np.float32)),
    "nlist=0": dict(nlist=0),
    "niter=-1": dict(niter=-1),
    "metric=2": dict(metric=2),
    "train_sample<nlist": dict(nlist=7, train_sample=5),  # 0 < train_sample < nlist <= n
    "device=99": dict(device=99),
}


@pytest.mark.parametrize("name", list(ERROR_CALLS))
def test_tier_c_errors_leave_the_library_usable(gpu, name):
    case = (300, 16, 3, 0, 3)
    args = dict(x=case_rows(case), nlist=3, metric=0, train_sample=0, niter=1, seed=KM_SEED, init=1, device=0)
    with pytest.raises(gpu.HipAnnError):
        gpu.ivf_train(**{**args, **ERROR_CALLS[name]})
    assert_exact(gpu.ivf_train(**args), case_ref(case, 1, 1), "a valid call after the error")
