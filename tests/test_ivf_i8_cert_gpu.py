"""IVF form 7 (the int8 image) with the L2 certificate of per-row residuals: results equal the oracle's whether the
certificate passes (few or no re-runs) or not (the device fallback), on the shapes where the scan takes another
path, and the image is kept across adds and removes (only the touched 32-row passes are tiled again).

Inputs: tests/_i8cert.py (rows on an r-dimensional subspace plus noise; the CPU test checks that the numpy
restatement certifies the first input within the cap asserted here).
"""
from __future__ import annotations

import numpy as np
import pytest

import _i8cert as C
from _data import build_ivf_lists, check_topk_parity
from test_remove_ids import remove_from_csr

pytestmark = pytest.mark.gpu

NLIST, NPROBE, K = 64, 8, 10


def _index(gpu, xb, metric=0, nlist=NLIST, nprobe=NPROBE):
    cen, off, ids, codes = C.ivf_lists(xb, nlist, metric)
    ix = gpu.HipIndexIVFFlat(cen, off, ids, codes, nprobe, metric)
    ix.form = 7
    return ix, (cen, off, ids, codes)


def _check(oracle, ix, lists, xb, xq, metric=0, k=K, nprobe=NPROBE):
    cen, off, ids, codes = lists
    fb0 = ix.rerank_fallbacks()
    D, I = ix.search(xq, k)
    assert ix.last_search_path() == {"form": 7, "filter_k": 64, "sublists": 8}, ix.last_search_path()
    Do, Io, Po = oracle.ivf_search(cen, off, ids, codes, xq, k, nprobe, metric)
    assert np.array_equal(ix.last_probes(len(xq)), Po)
    st = check_topk_parity(xb, xq, D, I, Do, Io, metric)
    v = I >= 0
    assert np.allclose(D[v], Do[v], rtol=2e-6, atol=1e-6)  # the exact forms' tolerances (test_request_k_gpu.py)
    flagged = ix.rerank_fallbacks() - fb0
    print("flagged", flagged, "of", len(xq), "exact fraction", st["exact_fraction"])
    return flagged, D, I


def test_dense_but_certifying(gpu, oracle):
    """n 60 000, d 128, intrinsic dimension 4, noise 0.02: distances of about the quantisation scale apart, which the
    whole-table bound could not certify (5 % in the emulation) and the per-row bound does."""
    xb, xq = C.lowrank_case(60_000, 128, 4, 0.02, 128, seed=5)
    ix, lists = _index(gpu, xb)
    flagged, _, _ = _check(oracle, ix, lists, xb, xq)
    assert flagged <= 2, flagged
    ix.close()


def test_not_certifying_falls_back(gpu, oracle):
    """The same at intrinsic dimension 2 (the emulation certifies 12 %): the flagged queries re-run in the direct form
    and the results still equal the oracle's."""
    xb, xq = C.lowrank_case(60_000, 128, 2, 0.02, 128, seed=5)
    ix, lists = _index(gpu, xb)
    _check(oracle, ix, lists, xb, xq)
    ix.close()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("shape", ["d100", "d768", "zero_row", "query_is_row", "near_copies"])
def test_other_shapes(gpu, oracle, shape, metric):
    rng = np.random.default_rng(3)
    nlist = NLIST
    if shape == "d100":  # d no multiple of the 64-dim super-step
        xb, xq = C.lowrank_case(20_000, 100, 4, 0.02, 64, seed=6)
    elif shape == "d768":
        xb, xq = C.lowrank_case(40_000, 768, 16, 0.02, 64, seed=7)
    elif shape == "zero_row":
        xb, xq = C.lowrank_case(20_000, 128, 4, 0.02, 64, seed=8)
        xb[12_345] = 0
    elif shape == "query_is_row":
        xb, xq = C.lowrank_case(20_000, 128, 4, 0.02, 64, seed=9)
        xq[:16] = xb[rng.choice(len(xb), 16, replace=False)]
    else:  # 40 near-copies of every row: ties and flags
        base, xq = C.lowrank_case(1_500, 128, 4, 0.02, 64, seed=10)
        xb = np.repeat(base, 40, axis=0)
        xb += np.float32(1e-3) * rng.standard_normal(xb.shape, dtype=np.float32)
        xb = np.ascontiguousarray(xb[rng.permutation(len(xb))])
    ix, lists = _index(gpu, xb, metric, nlist)
    _check(oracle, ix, lists, xb, xq, metric)
    ix.close()


def test_add_and_remove_keep_the_image(gpu, oracle):
    """With the int8 image built: 2048 rows arrive and 100 leave.  Results equal the oracle's on the new lists, the
    tiled-pass counter grows by the touched passes only and memory_bytes counts the image and both per-row planes."""
    xb, xq = C.lowrank_case(60_000, 128, 4, 0.02, 128, seed=5)
    xnew, _ = C.lowrank_case(2048, 128, 4, 0.02, 1, seed=11)
    d = xb.shape[1]
    ix, (cen, off, ids, codes) = _index(gpu, xb)
    mem0 = ix.memory_bytes
    assert ix.i8_passes_tiled() == 0
    ix.search(xq, K)
    p0 = ix.i8_passes_tiled()
    assert p0 == int(np.sum(-(-np.diff(off) // 32)))  # every pass once
    img = ix.memory_bytes - mem0
    # the image: whole passes of 32 rows x (d padded to whole super-steps) bytes, plus a scale and a residual per row
    assert img >= len(xb) * (d + 8) and (img - 8 * len(xb)) % p0 == 0 and (img - 8 * len(xb)) // p0 >= 32 * d, img
    # add: the passes from each touched list's first partly filled pass to its new end
    idnew = np.arange(len(xb), len(xb) + len(xnew), dtype=np.int64)
    ix.add(xnew, ids=idnew)
    a = oracle.flat_search(cen, xnew, 1)[1][:, 0]
    cnt, ln = np.bincount(a, minlength=NLIST), np.diff(off)
    touched = int(sum(-(-(ln[l] + cnt[l]) // 32) - ln[l] // 32 for l in range(NLIST) if cnt[l]))
    p1 = ix.i8_passes_tiled()
    assert p1 - p0 == touched, (p1 - p0, touched)
    lists_i = [np.concatenate([ids[off[l]:off[l + 1]], idnew[a == l]]) for l in range(NLIST)]
    lists_c = [np.concatenate([codes[off[l]:off[l + 1]], xnew[a == l]]) for l in range(NLIST)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists_i])]).astype(np.int64)
    ids, codes = np.concatenate(lists_i), np.ascontiguousarray(np.concatenate(lists_c))
    xall = np.concatenate([xb, xnew])
    flagged, _, _ = _check(oracle, ix, (cen, off, ids, codes), xall, xq)
    assert flagged <= 2, flagged
    assert ix.i8_passes_tiled() == p1  # the search tiled nothing
    # remove: each removed row touches its own pass and the pass of the row that fills its hole
    gone = np.random.default_rng(12).choice(ids, 100, replace=False)
    assert ix.remove_ids(gone) == 100
    p2 = ix.i8_passes_tiled()
    assert 1 <= p2 - p1 <= 200, p2 - p1
    off, ids, codes = remove_from_csr(off, ids, codes, gone)
    flagged, _, I = _check(oracle, ix, (cen, off, ids, codes), xall, xq)
    assert flagged <= 2 and not np.isin(I, gone).any()
    assert ix.i8_passes_tiled() == p2
    assert ix.memory_bytes - mem0 >= ix.ntotal * (d + 8)
    ix.close()


def _form6(gpu, xb, metric=0):
    cen, off, ids, codes = C.ivf_lists(xb, NLIST, metric)
    ix = gpu.HipIndexIVFFlat(cen, off, ids, codes, NPROBE, metric)
    assert ix.form == ix.FORM_HALF_EXACT and ix.filter_image == ix.FILTER_AUTO
    return ix, (cen, off, ids, codes)


def _search6(oracle, ix, lists, xb, xq, k=K, metric=0):
    cen, off, ids, codes = lists
    D, I = ix.search(xq, k)
    Do, Io, Po = oracle.ivf_search(cen, off, ids, codes, xq, k, NPROBE, metric)
    assert np.array_equal(ix.last_probes(len(xq)), Po)
    check_topk_parity(xb, xq, D, I, Do, Io, metric)
    return D, I


def test_auto_switches_to_int8_after_probation(gpu, oracle):
    """Form 6 under auto, nq 256, L2, the certifying input: the first batch is answered through the fp16 image (and
    probed), the second through the int8 image; both equal the oracle and each other bit for bit."""
    xb, xq = C.lowrank_case(60_000, 128, 4, 0.02, 256, seed=5)
    ix, lists = _form6(gpu, xb)
    D1, I1 = _search6(oracle, ix, lists, xb, xq)
    assert ix.last_filter_image() == 0 and ix.last_search_path() == {"form": 6, "filter_k": 16, "sublists": 0}
    D2, I2 = _search6(oracle, ix, lists, xb, xq)
    assert ix.last_filter_image() == 1 and ix.last_search_path()["form"] == 6
    assert np.array_equal(I1, I2) and np.array_equal(D1, D2)
    assert ix.i8_passes_tiled() > 0
    ix.close()


def test_auto_stays_on_fp16_where_int8_does_not_certify(gpu, oracle):
    xb, xq = C.lowrank_case(60_000, 128, 2, 0.02, 256, seed=5)
    ix, lists = _form6(gpu, xb)
    for _ in range(3):
        _search6(oracle, ix, lists, xb, xq)
        assert ix.last_filter_image() == 0 and ix.last_search_path() == {"form": 6, "filter_k": 16, "sublists": 0}
    ix.close()


@pytest.mark.parametrize("case", ["ip", "nq8", "k30"])
def test_auto_leaves_other_requests_alone(gpu, oracle, case):
    """IP, a small batch and a sub-list request keep today's path (and its dict) exactly."""
    metric = 1 if case == "ip" else 0
    nq = 8 if case == "nq8" else 256
    k = 30 if case == "k30" else K
    xb, xq = C.lowrank_case(60_000, 128, 4, 0.02, nq, seed=5)
    ix, lists = _form6(gpu, xb, metric)
    want = {"form": 6, "filter_k": 60, "sublists": 8} if case == "k30" else {"form": 6, "filter_k": 16, "sublists": 0}
    for _ in range(2):
        _search6(oracle, ix, lists, xb, xq, k, metric)
        assert ix.last_search_path() == want and ix.last_filter_image() == 0
    assert ix.i8_passes_tiled() == 0
    ix.close()


def test_filter_image_modes_are_honoured(gpu, oracle):
    xb, xq = C.lowrank_case(60_000, 128, 4, 0.02, 256, seed=5)
    ix, lists = _form6(gpu, xb)
    ix.filter_image = ix.FILTER_FP16
    for _ in range(2):
        D0, I0 = _search6(oracle, ix, lists, xb, xq)
        assert ix.last_filter_image() == 0
    assert ix.i8_passes_tiled() == 0
    ix.filter_image = ix.FILTER_INT8
    D1, I1 = _search6(oracle, ix, lists, xb, xq)  # at once, no probation
    assert ix.last_filter_image() == 1 and ix.last_search_path() == {"form": 6, "filter_k": 64, "sublists": 8}
    assert np.array_equal(I0, I1) and np.array_equal(D0, D1)
    with pytest.raises(gpu.HipAnnError):
        ix.filter_image = 3
    ix.close()
