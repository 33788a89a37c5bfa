"""GPU tests of hipann_flat_remove_ids / hipann_ivf_remove_ids: rows leave the resident copy in place, and what is
left equals what FAISS leaves on the CPU — IndexFlatCodes::remove_ids (a stable compaction, labels shifted down:
np.delete) and IndexIVF::remove_ids (the sequential fill-with-the-last-entry loop restated in
tests/test_remove_ids.py) — and searches like an index built from scratch over those rows."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from _data import build_ivf_lists, check_topk_parity, faiss_metal_case
from test_remove_ids import remove_from_csr

pytestmark = pytest.mark.gpu

N_FLAT = 3000


def _flat_sets(n):
    rng = np.random.default_rng(5)
    return {
        "first": np.array([0]),
        "last": np.array([n - 1]),
        "tile": np.arange(256, 512),
        "tile_edge": np.array([255, 256, 257]),
        "random10": rng.choice(n, n // 10, replace=False),
        "dups_and_outside": np.array([7, 7, 300, -1, n + 5, 300, 2999, 7]),
        "empty": np.zeros(0, np.int64),
        "all": rng.permutation(n),
    }


def _kept(n, labels):
    lab = np.unique(np.asarray(labels, np.int64))
    lab = lab[(lab >= 0) & (lab < n)]
    return np.delete(np.arange(n), lab), len(lab)


def _check_flat(gpu, oracle, ix, rows, xq, metric, nqs=(1, 40), fresh=True):
    """ix holds exactly `rows` (labels 0..len-1): size, bit-equal rows, oracle parity, equality with a fresh build."""
    n, d = rows.shape
    assert ix.ntotal == n
    assert np.array_equal(ix.reconstruct_n(0, n).view(np.uint32), rows.view(np.uint32))
    pad = -np.inf if metric == 1 else np.inf
    fr = gpu.HipIndexFlat(d, metric, rows) if fresh and n else None
    for nq in nqs:
        D, I = ix.search(xq[:nq], 10)
        if n == 0:
            assert (I == -1).all() and (D == pad).all()
            continue
        Do, Io = oracle.flat_search(rows, xq[:nq], 10, metric)
        check_topk_parity(rows, xq[:nq], D, I, Do, Io, metric)
        if fr is not None:
            D2, I2 = fr.search(xq[:nq], 10)
            assert np.array_equal(I, I2) and np.array_equal(D, D2), nq
    if fr is not None:
        fr.close()


@pytest.mark.parametrize("which", list(_flat_sets(N_FLAT)))
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [32, 33])
def test_flat_remove_small(gpu, oracle, d, metric, which):
    """One removal on a 3000-row table (12 tiles of 256 rows; d = 33 takes the scalar gather): first / last row, a
    whole tile, the rows around a tile edge, a random tenth, duplicates with labels outside the table, nothing, all."""
    n = N_FLAT
    xb, xq = faiss_metal_case(n, 40, d)
    labels = _flat_sets(n)[which]
    ix = gpu.HipIndexFlat(d, metric, xb)
    ix.search(xq, 10)
    keep, nrem = _kept(n, labels)
    mem0 = ix.memory_bytes
    assert ix.remove_ids(labels) == nrem
    assert ix.memory_bytes <= mem0 and (nrem == 0 or ix.memory_bytes < mem0)
    _check_flat(gpu, oracle, ix, np.ascontiguousarray(xb[keep]), xq, metric)
    if len(keep):
        assert np.array_equal(ix.reconstruct(len(keep) - 1), xb[keep[-1]])
    ix.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_flat_remove_add_remove(gpu, oracle, metric):
    d = 32
    xb, xq = faiss_metal_case(3500, 40, d)
    rng = np.random.default_rng(11)
    ix = gpu.HipIndexFlat(d, metric, xb[:3000])
    ix.search(xq, 10)
    r1 = rng.choice(3000, 300, replace=False)
    assert ix.remove_ids(r1) == 300
    rows = np.delete(xb[:3000], r1, 0)
    ix.add(xb[3000:])
    rows = np.ascontiguousarray(np.concatenate([rows, xb[3000:]]))
    _check_flat(gpu, oracle, ix, rows, xq, metric, nqs=(40,), fresh=False)
    r2 = np.concatenate([rng.choice(len(rows), 200, replace=False), np.arange(len(rows) - 40, len(rows))])
    keep, nrem = _kept(len(rows), r2)
    assert ix.remove_ids(r2) == nrem
    _check_flat(gpu, oracle, ix, np.ascontiguousarray(rows[keep]), xq, metric)
    ix.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_flat_remove_multi_shard(gpu, oracle, metric):
    """Three shards of 1000 rows: a removal across a shard boundary, one that empties the middle shard, one in the
    last shard after its labels have shifted twice."""
    d = 32
    xb, xq = faiss_metal_case(3000, 40, d)
    ix = gpu.HipIndexFlat(d, metric, xb, devices=[0, 0, 0])
    ix.search(xq, 10)
    rows = xb
    for labels in (np.arange(990, 1011), np.arange(990, 990 + 989), np.array([990, 995, 5]), np.array([0])):
        keep, nrem = _kept(len(rows), labels)
        assert ix.remove_ids(labels) == nrem
        rows = np.ascontiguousarray(rows[keep])
        _check_flat(gpu, oracle, ix, rows, xq, metric, nqs=(40,), fresh=False)
    ix.add(xb[:10])  # appended rows go to the last shard, labels continue from ntotal
    _check_flat(gpu, oracle, ix, np.ascontiguousarray(np.concatenate([rows, xb[:10]])), xq, metric, nqs=(1, 40),
                fresh=False)
    ix.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_flat_remove_int8_and_bf16_images(gpu, oracle, metric):
    """600 000 x 64 with the int8 and bf16 images built: a random 1 % plus the whole first tile leave; the int8
    bounded passes (nq 256), the bf16 passes (form 4) and the small-batch int8 scan (nq 4) run on the re-tiled images
    and agree with the oracle and with one fresh build (whose bound terms are the survivors' own maxima, at most the
    ones this index kept)."""
    rng = np.random.default_rng(71 + metric)
    d, n = 64, 600_000
    xb = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    xq = rng.uniform(-1, 1, (256, d)).astype(np.float32)
    ix = gpu.HipIndexFlat(d, metric, xb)
    ix.search(xq, 10)          # int8 image (bounded passes)
    ix.form = ix.FORM_BF16_EXACT
    ix.search(xq, 10)          # bf16 image
    ix.form = ix.FORM_I8_EXACT
    ix.search(xq[:4], 10)      # small-batch int8 scan
    labels = np.concatenate([np.arange(256), rng.choice(n, n // 100, replace=False)])
    keep, nrem = _kept(n, labels)
    assert ix.remove_ids(labels) == nrem and ix.ntotal == n - nrem
    rows = np.ascontiguousarray(xb[keep])
    Do, Io = oracle.flat_search(rows, xq[:64], 10, metric)
    Do4, Io4 = oracle.flat_search(rows, xq[:4], 10, metric)
    fresh = gpu.HipIndexFlat(d, metric, rows)
    for form, nq in ((ix.FORM_I8_EXACT, 256), (ix.FORM_BF16_EXACT, 256), (ix.FORM_I8_EXACT, 4)):
        ix.form = form
        fresh.form = form
        D, I = ix.search(xq[:nq], 10)
        assert ix.last_search_path()["form"] == form, (form, nq)
        m = min(nq, 64)
        ref = (Do4, Io4) if nq == 4 else (Do, Io)
        check_topk_parity(rows, xq[:m], D[:m], I[:m], ref[0][:m], ref[1][:m], metric)
        D2, I2 = fresh.search(xq[:nq], 10)
        assert np.array_equal(I, I2), (form, nq)
    fresh.close()
    ix.close()


# ---------------------------------------------------------------------------------------------------------------
# IVF
# ---------------------------------------------------------------------------------------------------------------
IVF_N, IVF_D, IVF_NLIST, IVF_NPROBE = 9000, 48, 30, 6
_IVF = {}


def _ivf_case():
    if not _IVF:
        xb, xq = faiss_metal_case(IVF_N, 30, IVF_D)
        cen = np.ascontiguousarray(xb[::300][:IVF_NLIST])
        off, ids, codes = build_ivf_lists(xb, cen)
        for a in (xb, xq, cen, off, ids, codes):
            a.setflags(write=False)
        _IVF.update(xb=xb, xq=xq, cen=cen, off=off, ids=ids, codes=codes)
    return _IVF


def _ivf_sets(off, ids):
    rng = np.random.default_rng(9)
    big = int(np.argmax(np.diff(off)))
    return {
        "random10": rng.choice(IVF_N, IVF_N // 10, replace=False),
        "whole_list": ids[off[3]:off[4]],
        "list_tail": ids[off[big + 1] - 3:off[big + 1]],
        "first_of_every_list": ids[off[:-1][np.diff(off) > 0]],
        "absent": np.array([IVF_N + 7, -5, 10 ** 12]),
        "all": rng.permutation(IVF_N),
    }


def _check_export(ix, cen, off, ids, codes):
    ex = ix.export()
    assert np.array_equal(ex["list_offsets"], off)
    assert np.array_equal(ex["ids"], ids)
    assert np.array_equal(ex["codes"].view(np.uint32), codes.view(np.uint32))
    assert np.array_equal(ex["centroids"], cen)
    assert ix.ntotal == len(ids)


@pytest.mark.parametrize("which", ["random10", "whole_list", "list_tail", "first_of_every_list", "absent", "all"])
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_ivf_remove_export_order(gpu, oracle, devices, which):
    """hipann_ivf_export after a removal equals FAISS's sequential loop applied to every list, bit for bit."""
    c = _ivf_case()
    labels = _ivf_sets(c["off"], c["ids"])[which]
    ix = gpu.HipIndexIVFFlat(c["cen"], c["off"], c["ids"], c["codes"], IVF_NPROBE, devices=devices)
    ix.search(c["xq"], 10)  # the fp16 image exists: the removal re-tiles its touched passes
    off, ids, codes = remove_from_csr(c["off"], c["ids"], c["codes"], labels)
    assert ix.remove_ids(labels) == IVF_N - len(ids)
    _check_export(ix, c["cen"], off, ids, codes)
    if which == "all":
        D, I = ix.search(c["xq"], 10)
        assert (I == -1).all() and np.isinf(D).all()
    ix.close()


@pytest.mark.parametrize("form,devices", [(5, None), (6, None), (0, None), (6, [0, 0])])
def test_ivf_search_after_remove(gpu, oracle, form, devices):
    c = _ivf_case()
    xb, xq, cen = c["xb"], c["xq"], c["cen"]
    labels = _ivf_sets(c["off"], c["ids"])["random10"]
    ix = gpu.HipIndexIVFFlat(cen, c["off"], c["ids"], c["codes"], IVF_NPROBE, devices=devices)
    ix.form = form
    ix.search(xq, 10)  # the form's tiled image exists
    ix.remove_ids(labels)
    off, ids, codes = remove_from_csr(c["off"], c["ids"], c["codes"], labels)
    D, I = ix.search(xq, 10)
    Do, Io, Po = oracle.ivf_search(cen, off, ids, codes, xq, 10, IVF_NPROBE)
    assert np.array_equal(ix.last_probes(len(xq)), Po)
    assert not np.isin(I, labels).any()
    st = check_topk_parity(xb, xq, D, I, Do, Io)
    if form in (5, 6):
        assert st["exact_fraction"] == 1.0, st
    fresh = gpu.HipIndexIVFFlat(cen, off, ids, codes, IVF_NPROBE, devices=devices)
    fresh.form = form
    D2, I2 = fresh.search(xq, 10)
    assert np.array_equal(I, I2) and np.array_equal(D, D2)
    fresh.close()
    ix.close()


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_ivf_remove_add_remove(gpu, oracle, devices):
    """2000 rows leave, 2000 arrive with explicit ids (into the freed slack), 1500 leave again."""
    c = _ivf_case()
    xb, xq, cen = c["xb"], c["xq"], c["cen"]
    rng = np.random.default_rng(13)
    ix = gpu.HipIndexIVFFlat(cen, c["off"], c["ids"], c["codes"], IVF_NPROBE, devices=devices)
    ix.search(xq, 10)
    r1 = rng.choice(IVF_N, 2000, replace=False)
    assert ix.remove_ids(r1) == 2000
    off, ids, codes = remove_from_csr(c["off"], c["ids"], c["codes"], r1)
    # the new rows: fresh vectors, labels IVF_N.., appended to their nearest centroid's list in insertion order
    xnew = rng.uniform(-1, 1, (2000, IVF_D)).astype(np.float32)
    idnew = np.arange(IVF_N, IVF_N + 2000, dtype=np.int64)
    ix.add(xnew, ids=idnew)
    a = oracle.flat_search(cen, xnew, 1)[1][:, 0]
    lists_i = [np.concatenate([ids[off[l]:off[l + 1]], idnew[a == l]]) for l in range(IVF_NLIST)]
    lists_c = [np.concatenate([codes[off[l]:off[l + 1]], xnew[a == l]]) for l in range(IVF_NLIST)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists_i])]).astype(np.int64)
    ids, codes = np.concatenate(lists_i), np.ascontiguousarray(np.concatenate(lists_c))
    _check_export(ix, cen, off, ids, codes)
    r2 = rng.choice(ids, 1500, replace=False)
    assert ix.remove_ids(r2) == 1500
    off, ids, codes = remove_from_csr(off, ids, codes, r2)
    _check_export(ix, cen, off, ids, codes)
    xall = np.concatenate([xb, xnew])
    D, I = ix.search(xq, 10)
    Do, Io, Po = oracle.ivf_search(cen, off, ids, codes, xq, 10, IVF_NPROBE)
    assert np.array_equal(ix.last_probes(len(xq)), Po)
    st = check_topk_parity(xall, xq, D, I, Do, Io)
    assert st["exact_fraction"] == 1.0, st
    ix.close()


def test_remove_failure_leaves_the_handle_intact(gpu, oracle):
    c = _ivf_case()
    xq = c["xq"]
    L = gpu.lib()
    lab = np.arange(10, dtype=np.int64)
    p = lab.ctypes.data_as(C.POINTER(C.c_int64))
    fx = gpu.HipIndexFlat(IVF_D, 0, c["xb"])
    vx = gpu.HipIndexIVFFlat(c["cen"], c["off"], c["ids"], c["codes"], IVF_NPROBE)
    for ix, good, bad in ((fx, L.hipann_flat_remove_ids, L.hipann_ivf_remove_ids),
                          (vx, L.hipann_ivf_remove_ids, L.hipann_flat_remove_ids)):
        D0, I0 = ix.search(xq, 10)
        for fn, args in ((good, (p, -1)), (good, (None, 3)), (bad, (p, 10))):
            eb = C.create_string_buffer(256)
            assert fn(ix._h, *args, eb, 256) == -1 and eb.value
        assert good(ix._h, p, 0, None, 0) == 0
        assert ix.ntotal == IVF_N
        D1, I1 = ix.search(xq, 10)
        assert np.array_equal(I0, I1) and np.array_equal(D0, D1)
        ix.close()


def test_remove_on_borrowed_device_tables(gpu, oracle):
    """copy = 0 handles (hipann_*_create_device) move into owned storage at their first removal, as at their first
    add: the caller's tensors are left untouched, a Flat shard keeps its label_offset."""
    import torch

    c = _ivf_case()
    xb, xq, cen = c["xb"], c["xq"], c["cen"]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    xq_t = torch.from_numpy(xq.copy()).to(dev)
    Dt = torch.empty((len(xq), 10), device=dev)
    It = torch.empty((len(xq), 10), device=dev, dtype=torch.int64)
    # Flat, labels 100 + row
    xb_t = torch.from_numpy(xb.copy()).to(dev)
    fx = gpu.HipIndexFlatDevice(IVF_D, 0, xb_t.data_ptr(), IVF_N, 0, copy=False, label_offset=100)
    lab = np.array([100, 105, 100 + IVF_N - 1, 99, 5000, 5000], np.int64)
    eb = C.create_string_buffer(256)
    assert gpu.lib().hipann_flat_remove_ids(fx._h, lab.ctypes.data_as(C.POINTER(C.c_int64)), len(lab), eb, 256) == 4
    torch.cuda.synchronize()
    assert np.array_equal(xb_t.cpu().numpy(), xb)
    rows = np.ascontiguousarray(np.delete(xb, [0, 5, IVF_N - 1, 4900], 0))
    assert fx.ntotal == len(rows)
    fx.search_device(len(xq), xq_t.data_ptr(), 10, Dt.data_ptr(), It.data_ptr(), stream)
    torch.cuda.synchronize()
    Do, Io = oracle.flat_search(rows, xq, 10)
    check_topk_parity(rows, xq, Dt.cpu().numpy(), It.cpu().numpy() - 100, Do, Io)
    fx.close()
    # IVF
    c_t, i_t = torch.from_numpy(cen.copy()).to(dev), torch.from_numpy(c["ids"].copy()).to(dev)
    x_t = torch.from_numpy(c["codes"].copy()).to(dev)
    vx = gpu.HipIndexIVFFlat.from_device(IVF_D, 0, IVF_NLIST, IVF_NPROBE, c_t.data_ptr(), c["off"], i_t.data_ptr(),
                                         x_t.data_ptr(), 0)
    labels = _ivf_sets(c["off"], c["ids"])["random10"]
    off, ids, codes = remove_from_csr(c["off"], c["ids"], c["codes"], labels)
    assert vx.remove_ids(labels) == IVF_N - len(ids)
    torch.cuda.synchronize()
    assert np.array_equal(x_t.cpu().numpy(), c["codes"]) and np.array_equal(i_t.cpu().numpy(), c["ids"])
    _check_export(vx, cen, off, ids, codes)
    vx.search_device(len(xq), xq_t.data_ptr(), 10, Dt.data_ptr(), It.data_ptr(), stream)
    torch.cuda.synchronize()
    Do, Io, _ = oracle.ivf_search(cen, off, ids, codes, xq, 10, IVF_NPROBE)
    check_topk_parity(xb, xq, Dt.cpu().numpy(), It.cpu().numpy(), Do, Io)
    vx.close()
