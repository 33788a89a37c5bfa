"""IVF SQ8 remove_ids on the device (hipann_ivfsq_remove_ids) against numpy: FAISS's swap loop on Python lists, the
export byte for byte and every search in float64 (the grid data of test_ivf_sq8_add_gpu.py: array_equal throughout).

The lists are created with the lengths LENS whatever the metric (a row's list is the one it was generated around, not
its coarse assignment: any CSR is a valid index), so the pass and chunk edges are there for IP too."""
from __future__ import annotations

import copy

import numpy as np
import pytest

from test_ivf_sq8_add_gpu import LENS, NL, RefLists, assign64, encode32, grid_rows, quantizer

pytestmark = pytest.mark.gpu
L2, IP = 0, 1
F = NL - 1  # the longest list


class Ref(RefLists):
    def remove(self, labels):
        """faiss::IndexIVF::remove_ids with an IDSelectorBatch, list by list; the rows removed"""
        s, n = set(np.asarray(labels).tolist()), 0
        for l in range(NL):
            ids, codes = self.ids[l].copy(), self.codes[l].copy()
            j, e = 0, len(ids)
            while j < e:
                if int(ids[j]) in s:
                    e -= 1
                    ids[j], codes[j] = ids[e], codes[e]
                else:
                    j += 1
            n += len(ids) - e
            self.ids[l], self.codes[l] = ids[:e], codes[:e]
        return n


def pattern(s, ref):
    """the labels step s takes, chosen per list by position"""
    pick = [lambda i, l: i[:1],                                                      # one hole, filled by the last row
            lambda i, l: i[-1:],                                                     # no move, one vacated row
            lambda i, l: i[[p for p in (15, 16, 31, 32, 2047, 2048) if p < len(i)]],  # tile halves, pass and chunk edges
            lambda i, l: i[::2],                                                     # holes and sources interleave
            lambda i, l: i[:-(-7 * len(i) // 10)],                                   # most removed rows are above L'
            lambda i, l: i if l == F else i[:0]][s]                                  # L' = 0
    return np.concatenate([pick(ref.ids[l], l) for l in range(NL)])


def make_ref(rng, d, metric, by_res):
    cen, vmin, vdiff, big = quantizer(d, rng)
    ref = Ref(cen, vmin, vdiff, metric, by_res)
    own = np.repeat(np.arange(NL), LENS)
    x = grid_rows(rng, own, cen, vmin, vdiff, big, 8)
    ids = rng.permutation(len(x)).astype(np.int64) + (1 << 33)
    codes = encode32(x, cen[own] if by_res else None, vmin, vdiff)
    ref.ids, ref.codes = [ids[own == l] for l in range(NL)], [codes[own == l] for l in range(NL)]
    xq = rng.integers(-4, 5, (130, d)).astype(np.float32) * (16 if d <= 100 else 1)
    return ref, xq, (cen, vmin, vdiff, big)


def make_index(gpu, ref):
    off, ids, codes = ref.csr()
    return gpu.HipIndexIVFSQ8(ref.cen, ref.vmin, ref.vdiff, off, ids, codes, nprobe=1, metric=ref.metric,
                              by_residual=bool(ref.by_res))


def noisy(rng, lab):
    """shuffled, with duplicates and with ids the index does not hold"""
    lab = np.concatenate([lab, lab[:len(lab) // 3 + 1], np.arange(40, dtype=np.int64) + (1 << 50)])
    return lab[rng.permutation(len(lab))]


@pytest.mark.parametrize("d", [1, 33, 768])
@pytest.mark.parametrize("by_res", [0, 1])
@pytest.mark.parametrize("metric", [L2, IP])
def test_remove_exact(gpu, metric, by_res, d):
    rng = np.random.default_rng(29 + d)
    ref, xq, _ = make_ref(rng, d, metric, by_res)
    # every step's labels also hold one id that sits in two lists: a dry run of the (positional) steps picks, per step,
    # a row of list F - 1 and one of list F that are alive then and outside the step's pattern; they share an id
    dry, twins = copy.deepcopy(ref), []
    for s in range(6):
        lab = set(pattern(s, dry).tolist())
        a, b = (next((i for i in dry.ids[l].tolist() if i not in lab), int(dry.ids[l][0])) for l in (F - 1, F))
        twins.append(a)
        ref.ids[F][ref.ids[F] == b] = a
        dry.remove(list(lab) + [a, b])
    ix = make_index(gpu, ref)
    mem = ix.memory_bytes
    for s in range(6):
        assert sum(int((ref.ids[l] == twins[s]).sum()) for l in (F - 1, F)) == 2
        lab = noisy(rng, np.append(pattern(s, ref), twins[s]))
        assert ix.remove_ids(lab) == ref.remove(lab)
        ref.check(ix, xq)
        assert ix.memory_bytes == mem
    assert len(ref.ids[F]) == 0 and ix.ntotal == sum(len(i) for i in ref.ids) > 0


def test_remove_then_add_reuses_slack(gpu):
    rng = np.random.default_rng(41)
    ref, xq, (cen, vmin, vdiff, big) = make_ref(rng, 33, L2, 1)
    ix = make_index(gpu, ref)
    mem = ix.memory_bytes
    x = grid_rows(rng, np.repeat(F, 100), cen, vmin, vdiff, big, 256)
    assert (assign64(x, cen, L2) == F).all()
    lab = ref.ids[F][100:200].copy()
    assert ix.remove_ids(lab) == ref.remove(lab) == 100
    ref.check(ix, xq)
    new = np.arange(100, dtype=np.int64) + (1 << 40)
    ix.add(x, new)
    ref.add(x, new)
    ref.check(ix, xq)
    assert ix.memory_bytes == mem  # the freed rows took the added ones: no regroup
    ex = ix.export()
    ix2 = gpu.HipIndexIVFSQ8(ex["centroids"], ex["vmin"], ex["vdiff"], ex["list_offsets"], ex["ids"], ex["codes"],
                             nprobe=1, metric=L2)
    for k in (10, 100):
        for a, b in zip(ix.search(xq, k, nprobe=3), ix2.search(xq, k, nprobe=3)):
            assert np.array_equal(a, b)
    everything = np.concatenate(ref.ids)
    assert ix.remove_ids(everything) == ref.remove(everything) == len(everything) and ix.ntotal == 0
    D, I = ix.search(xq, 10, nprobe=NL)
    assert np.isposinf(D).all() and (I == -1).all()
    ix.add(x, new)
    ref.add(x, new)
    ref.check(ix, xq, (10, 200), (20,))


def test_remove_refusals(gpu):
    rng = np.random.default_rng(43)
    ref, xq, _ = make_ref(rng, 33, IP, 0)
    ix = make_index(gpu, ref)
    assert ix.remove_ids(np.zeros(0, np.int64)) == 0
    assert ix.remove_ids(np.arange(1000, dtype=np.int64)) == 0  # all absent
    ref.check(ix, xq, (10,), (20,))
    off, ids, _ = ref.csr()
    flat = gpu.HipIndexIVFFlat(ref.cen, off, ids, rng.standard_normal((len(ids), 33)).astype(np.float32), nprobe=1)
    for f, h in ((gpu.lib().hipann_ivfsq_remove_ids, flat), (gpu.lib().hipann_ivf_remove_ids, ix)):
        eb = gpu._err()
        assert f(h.handle, gpu._ptr(ids, gpu.C.c_int64), 1, eb, 1024) == -1 and b"not an" in eb.value
    assert ix.ntotal == flat.ntotal == len(ids)
