"""The cases of tests/test_ivf_compact_run_gpu.py: the seeded int8 scan whose second launch appends only the admitted
rows to each query's candidate run (csrc/ivf_mfma.hip mf_finish_item).  Shared with the child process
that answers them with HIPANN_IVF_SEED=0 (the single launch): run as a script, this file writes every case's ids,
distances and flag count to the .npz named on its command line.

Every index has hand-laid lists with the centroids given, so the layouts below decide which rows fall into a list's
first 2048 rows (chunk 0: the first launch, the seed) and which into the chunks the second launch scans.
"""
from __future__ import annotations

import sys

import numpy as np

import _seed_cases as S  # (puts the package and the repository on sys.path)
import _i8cert as C

F = np.float32
D64 = 64
CH = 2048            # rows per scan item
WAVES, PASS = 8, 32  # a chunk's rows are dealt to the item's 8 waves in passes of 32
SUBLIST = 16         # entries a wave keeps per query
SELECT_MAX = 4096    # longest run the rerank's block select takes


def _lists(cen, parts):
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    xb = np.ascontiguousarray(np.concatenate(parts).astype(F))
    return np.ascontiguousarray(cen.astype(F)), off, np.arange(len(xb), dtype=np.int64), xb


def _nearest_lists(cen, xq, nprobe):
    d2 = ((xq[:, None, :].astype(np.float64) - cen[None].astype(np.float64)) ** 2).sum(-1)
    return np.argsort(d2, axis=1, kind="stable")[:, :nprobe]


def _clusters(sizes, d, nq, seed, rank=4, sep=8.0):
    """len(sizes) well separated clusters of low-rank rows, one list each; query i sits in cluster i % nlist."""
    rng = np.random.default_rng(seed)
    nl = len(sizes)
    cen = sep * rng.standard_normal((nl, d)) / np.sqrt(d)
    xb, xq = C.lowrank_case(int(sum(sizes)), d, rank, 0.02, nq, seed=seed + 1)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    parts = [xb[offs[l]:offs[l + 1]] + cen[l].astype(F) for l in range(nl)]
    xq = np.ascontiguousarray(xq + cen[np.arange(nq) % nl].astype(F))
    return cen, parts, xq


def _one_row_tail():
    """Lists of 2049 rows: chunk 1 is one row, so seven of the item's waves append nothing.  In lists 0 and 1 that row
    is the nearest row of queries 0 and 1."""
    cen, parts, xq = _clusters([2049, 2049, 3000, 2100], D64, 64, seed=101)
    rng = np.random.default_rng(102)
    for l in (0, 1):
        parts[l][2048] = xq[l] + F(1e-3) * rng.standard_normal(D64, dtype=F)
    return _lists(cen, parts), xq, 2


def _empty_run():
    """Every row past a list's first 2048 lies far from every query: the second launch admits nothing, every cursor
    stays 0 and the rerank answers from the seed lists alone."""
    cen, parts, xq = _clusters([3000, 2600, 4100, 2049], D64, 64, seed=111)
    rng = np.random.default_rng(112)
    for p in parts:
        u = rng.standard_normal((len(p) - CH, D64))
        p[CH:] += (40.0 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(F)
    return _lists(cen, parts), xq, 2


def _full_run():
    """Near-copies (75 base rows, copies with 1e-3 noise, as tests/_seed_cases.py ties_near_copies), 8 lists of 8 chunks,
    every query probing every list.  The chunk 0s hold 40 copies of each of the 69 base rows of P among far filler
    rows; the other chunks hold only copies of the 6 base rows of R, the nearest base rows of the first six queries.
    A query whose nearest base row is in R gets a loose seed bound (the P copies are all farther) under which every
    wave of the second launch fills its 16 entries: 56 slots x 128 = 7168 appended entries, past the rerank's
    block select.  A query near P appends only the R copies that happen to lie under its bound.  Checked below on
    exact distances (the scan's keys are lower bounds within a few percent)."""
    base, xq = C.lowrank_case(75, D64, 4, 0.02, 64, seed=25)
    rng = np.random.default_rng(121)
    d2b = ((xq[:, None, :].astype(np.float64) - base[None].astype(np.float64)) ** 2).sum(-1)
    nearest = np.argmin(d2b, axis=1)
    R = np.unique(nearest[:6])
    P = np.setdiff1d(np.arange(75), R)
    nl, nch = 8, 8
    pc = np.repeat(base[P], 40, axis=0)
    pc = pc + F(1e-3) * rng.standard_normal(pc.shape, dtype=F)
    pc = pc[rng.permutation(len(pc))]
    per = len(pc) // nl  # P copies per chunk 0 (the remainder is dropped)
    fill, _ = C.lowrank_case(nl * (CH - per), D64, 4, 0.02, 1, seed=122)
    u = rng.standard_normal(fill.shape)
    fill = 3.0 * fill + (12.0 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(F)
    parts = []
    for l in range(nl):
        c0 = np.concatenate([pc[l * per:(l + 1) * per], fill[l * (CH - per):(l + 1) * (CH - per)]])
        c0 = c0[rng.permutation(CH)]
        rc = base[R][rng.integers(0, len(R), (nch - 1) * CH)]
        rc = rc + F(1e-3) * rng.standard_normal(rc.shape, dtype=F)
        parts.append(np.concatenate([c0, rc]).astype(F))
    lists = _lists(np.stack([p.mean(0) for p in parts]), parts)
    # the runs these rows make, on exact distances: the seed bound is the 64th smallest chunk-0 distance; a wave
    # appends min(16, its rows under the bound).  hi / lo: with the bound 25 % looser / tighter.
    xb = lists[3].astype(np.float64)
    d2 = ((xq.astype(np.float64) ** 2).sum(1)[:, None] + (xb ** 2).sum(1)[None] - 2.0 * xq.astype(np.float64) @ xb.T)
    d2 = d2.reshape(len(xq), nl, nch, CH // (WAVES * PASS), WAVES, PASS)
    bound = np.sort(d2[:, :, 0].reshape(len(xq), -1), axis=1)[:, 63]
    later = d2[:, :, 1:].transpose(0, 1, 2, 4, 3, 5).reshape(len(xq), nl * (nch - 1) * WAVES, -1)
    hi = np.minimum(SUBLIST, (later <= 1.25 * bound[:, None, None]).sum(-1)).sum(-1)
    lo = np.minimum(SUBLIST, (later <= 0.75 * bound[:, None, None]).sum(-1)).sum(-1)
    assert 64 + lo.max() > SELECT_MAX + 1024, lo.max()  # some query's run takes the rerank's serial path
    assert 64 + hi.min() < SELECT_MAX - 1024, hi.min()  # and some query's the block select
    return lists, xq, nl


def _two_groups():
    """120 queries all probing both lists: list 0 (three chunks) is scanned by two query groups, so two items of
    different blocks (its chunks 1 and 2) append to each of its queries' cursors."""
    cen, parts, xq = _clusters([5000, 300], D64, 120, seed=131, sep=2.0)
    return _lists(cen, parts), xq, 2


def _nprobe32():
    """nprobe 32 with 128-entry slots: the most chunk-0 entries the seed kernel's select holds."""
    rng = np.random.default_rng(141)
    sizes = [int(s) for s in rng.choice([900, 2048, 2049, 2600, 4097, 4300], 40)]
    cen, parts, xq = _clusters(sizes, D64, 64, seed=142, sep=3.0)
    return _lists(cen, parts), xq, 32


def _d100():
    cen, parts, xq = _clusters([4100, 2049, 5000, 100], 100, 64, seed=151, sep=4.0)
    return _lists(cen, parts), xq, 3


def _d768():
    cen, parts, xq = _clusters([3 * CH + 5, 300], 768, 64, seed=161, rank=16, sep=4.0)
    return _lists(cen, parts), xq, 2


def _last_query_single_chunk():
    """Lists 0 and 1 have two chunks, lists 2 and 3 one; the batch's last query probes only lists 2 and 3, so no item
    of the second launch touches its cursor, which the seed kernel zeroed."""
    rng = np.random.default_rng(171)
    u, v, w = (x / np.linalg.norm(x) for x in rng.standard_normal((3, D64)))
    cen = np.stack([8 * u, 8 * u + 3 * v, -8 * u, -8 * u + 3 * w])
    sizes = [3000, 2500, 1500, 900]
    xb, xq = C.lowrank_case(sum(sizes), D64, 4, 0.02, 64, seed=172)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    parts = [xb[offs[l]:offs[l + 1]] + cen[l].astype(F) for l in range(4)]
    home = np.arange(64) % 2
    home[63] = 2
    xq = np.ascontiguousarray(xq + cen[home].astype(F))
    lists = _lists(cen, parts)
    near = _nearest_lists(lists[0], xq, 2)
    assert set(near[63]) == {2, 3} and all(set(near[i]) == {0, 1} for i in range(63))
    return lists, xq, 2


# name -> (builder of (lists, xq, nprobe), k)
CASES = {
    "one_row_tail": (_one_row_tail, 12),
    "empty_run": (_empty_run, 10),
    "full_run_near_copies": (_full_run, 10),
    "two_groups_one_list": (_two_groups, 1),
    "nprobe32": (_nprobe32, 10),
    "d100": (_d100, 10),
    "d768_three_chunks_and_5": (_d768, 10),
    "last_query_single_chunk": (_last_query_single_chunk, 10),
}


def run_case(hipann, name):
    """Answer the case on the GPU three times.  Returns a dict: D, I of the first search and of the two repeats, the
    first search's flag count, the path, the probes and the case's data."""
    build, k = CASES[name]
    (cen, off, ids, codes), xq, nprobe = build()
    ix = hipann.HipIndexIVFFlat(cen, off, ids, codes, nprobe, 0)
    ix.form = 7
    fb0 = ix.rerank_fallbacks()
    D, I = ix.search(xq, k)
    flagged = ix.rerank_fallbacks() - fb0
    path = ix.last_search_path(seeded=True)
    probes = ix.last_probes(len(xq))
    repeats = [ix.search(xq, k) for _ in range(2)]
    ix.close()
    return {"D": D, "I": I, "repeats": repeats, "flagged": flagged, "path": path, "probes": probes,
            "lists": (cen, off, ids, codes), "xq": xq, "k": k, "nprobe": nprobe}


if __name__ == "__main__":
    import hipann

    out = {}
    for name in CASES:
        r = run_case(hipann, name)
        assert r["path"]["seeded"] == 0, (name, r["path"])  # the switch is off in this process
        out[name + ".D"], out[name + ".I"] = r["D"], r["I"]
        out[name + ".flagged"] = np.int64(r["flagged"])
    np.savez(sys.argv[1], **out)
