"""The fp16 / int8 list scan's selection (csrc/ivf_mfma.hip mh_item: per step, the admitted rows are inserted one by
one or sorted and merged): results equal the oracle's under the parity rule on the shapes where the bounds cross items,
waves and query groups and where keys tie, a batch repeats bit for bit, and the certificate's flag count stays put.

d is 64 unless a case names another.  With nprobe = nlist every list is probed by every query, so the lists are laid
out by hand (any partition of the rows is a valid IVF index) to get the chunk and pass counts each case needs.
"""
from __future__ import annotations

import numpy as np
import pytest

import _i8cert as C
from _data import check_topk_parity

pytestmark = pytest.mark.gpu

D64 = 64


def _hand_lists(xb, sizes):
    """Lists of the given sizes over xb's rows in order (ids = row numbers); centroids = the lists' means (an empty
    list's: a far corner, it is probed all the same at nprobe = nlist)."""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert off[-1] == len(xb)
    cen = np.stack([xb[off[l]:off[l + 1]].mean(0) if sizes[l] else np.full(xb.shape[1], 9.0, np.float32)
                    for l in range(len(sizes))]).astype(np.float32)
    return np.ascontiguousarray(cen), off, np.arange(len(xb), dtype=np.int64), xb


def _run(gpu, oracle, lists, xq, k, form, metric=0, fp16=False, want_sub=None):
    cen, off, ids, codes = lists
    nprobe = len(cen)
    ix = gpu.HipIndexIVFFlat(cen, off, ids, codes, nprobe, metric)
    ix.form = form
    if fp16:
        ix.filter_image = ix.FILTER_FP16
    D, I = ix.search(xq, k)
    if want_sub is not None:
        assert ix.last_search_path()["sublists"] == want_sub, ix.last_search_path()
    Do, Io, Po = oracle.ivf_search(cen, off, ids, codes, xq, k, nprobe, metric)
    assert np.array_equal(np.sort(ix.last_probes(len(xq)), axis=1), np.sort(Po, axis=1))
    check_topk_parity(codes, xq, D, I, Do, Io, metric)
    D2, I2 = ix.search(xq, k)  # repeat: the same batch on the same index, bit for bit
    assert np.array_equal(I, I2) and np.array_equal(D, D2)
    ix.close()
    return D, I


@pytest.fixture(scope="module")
def cross_item():
    """nlist 4, nprobe 4, about 6000 rows per list (3 chunks of 2048), nq 40: three query tiles, the last with 8."""
    xb, xq = C.lowrank_case(24_000, D64, 4, 0.02, 40, seed=21)
    return _hand_lists(xb, [6000, 5990, 6100, 5910]), xq


@pytest.mark.parametrize("case", ["form7_l2", "form7_ip", "form6_fp16_k10", "form6_fp16_k30"])
def test_cross_item_partial_tile(gpu, oracle, cross_item, case):
    lists, xq = cross_item
    if case == "form7_l2":
        _run(gpu, oracle, lists, xq, 10, 7, 0, want_sub=8)
    elif case == "form7_ip":
        _run(gpu, oracle, lists, xq, 10, 7, 1)
    elif case == "form6_fp16_k10":  # one merged list per slot
        _run(gpu, oracle, lists, xq, 10, 6, 0, fp16=True, want_sub=0)
    else:  # a sub-list request
        _run(gpu, oracle, lists, xq, 30, 6, 0, fp16=True, want_sub=8)


@pytest.mark.parametrize("form", [7, 6])
def test_ragged_chunks(gpu, oracle, form):
    """A list of 2049 rows (its second chunk has one row: seven waves have no pass), one of 100 rows, an empty one."""
    xb, xq = C.lowrank_case(2049 + 100 + 1000, D64, 4, 0.02, 40, seed=22)
    _run(gpu, oracle, _hand_lists(xb, [2049, 100, 0, 1000]), xq, 10, form, fp16=form == 6)


@pytest.mark.parametrize("form", [7, 6])
def test_more_than_one_group(gpu, oracle, form):
    """One list, 3000 rows, 100 queries: over the 96 a group holds, so the list is scanned by two groups."""
    xb, xq = C.lowrank_case(3000, D64, 4, 0.02, 100, seed=23)
    _run(gpu, oracle, _hand_lists(xb, [3000]), xq, 10, form, fp16=form == 6)


@pytest.mark.parametrize("form", [7, 6])
@pytest.mark.parametrize("shape", ["identical", "near_copies"])
def test_ties(gpu, oracle, shape, form):
    """Every key equal (3000 identical rows), and 40 near-copies of every row: admission at `<=` and the shared gate
    must agree."""
    rng = np.random.default_rng(24)
    if shape == "identical":
        base, xq = C.lowrank_case(1, D64, 4, 0.02, 40, seed=24)
        xb = np.ascontiguousarray(np.repeat(base, 3000, axis=0))
        lists = _hand_lists(xb, [3000])
    else:
        base, xq = C.lowrank_case(150, D64, 4, 0.02, 40, seed=25)
        xb = np.repeat(base, 40, axis=0)
        xb += np.float32(1e-3) * rng.standard_normal(xb.shape, dtype=np.float32)
        xb = np.ascontiguousarray(xb[rng.permutation(len(xb))])
        lists = _hand_lists(xb, [2500, 3500])
    _run(gpu, oracle, lists, xq, 10, form, fp16=form == 6)


def test_d768(gpu, oracle):
    """d 768, nq 64, as test_ivf_i8_cert_gpu.py::test_other_shapes builds it."""
    xb, xq = C.lowrank_case(40_000, 768, 16, 0.02, 64, seed=7)
    cen, off, ids, codes = C.ivf_lists(xb, 64, 0)
    ix = gpu.HipIndexIVFFlat(cen, off, ids, codes, 8, 0)
    ix.form = 7
    D, I = ix.search(xq, 10)
    Do, Io, Po = oracle.ivf_search(cen, off, ids, codes, xq, 10, 8, 0)
    assert np.array_equal(ix.last_probes(len(xq)), Po)
    check_topk_parity(xb, xq, D, I, Do, Io, 0)
    D2, I2 = ix.search(xq, 10)
    assert np.array_equal(I, I2) and np.array_equal(D, D2)
    ix.close()


def test_certificate_and_images_agree(gpu):
    """The dense certifying input of test_ivf_i8_cert_gpu.py, form 7: the flag count stays within that test's cap, and
    form 6 answers the same batch bit for bit through the fp16 and through the int8 image (the selection keeps the
    same rows whichever of its two merge paths a step takes)."""
    xb, xq = C.lowrank_case(60_000, 128, 4, 0.02, 128, seed=5)
    cen, off, ids, codes = C.ivf_lists(xb, 64, 0)
    ix = gpu.HipIndexIVFFlat(cen, off, ids, codes, 8, 0)
    ix.form = 7
    fb0 = ix.rerank_fallbacks()
    D7, I7 = ix.search(xq, 10)
    flagged = ix.rerank_fallbacks() - fb0
    print("flagged", flagged, "of", len(xq))
    assert flagged <= 2, flagged
    ix.form = 6
    ix.filter_image = ix.FILTER_FP16
    D0, I0 = ix.search(xq, 10)
    ix.filter_image = ix.FILTER_INT8
    D1, I1 = ix.search(xq, 10)
    assert ix.last_filter_image() == 1
    assert np.array_equal(I0, I1) and np.array_equal(D0, D1)
    assert np.array_equal(I7, I1) and np.array_equal(D7, D1)
    ix.close()
