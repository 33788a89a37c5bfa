"""The cases of tests/test_ivf_seed_bound_gpu.py, shared with the child process that answers them with
HIPANN_IVF_SEED=0 (the single-launch int8 scan): run as a script, it writes every case's ids, distances, flag count and
path to the .npz named on its command line.

Every index has hand-laid lists (tests/test_ivf_scan_bounds_gpu.py) and nprobe = nlist, so each query probes each list.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "duckdb-annsearch_amd", ROOT, Path(__file__).resolve().parent):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import _i8cert as C  # noqa: E402

D64 = 64


def hand_lists(xb, sizes):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert off[-1] == len(xb)
    cen = np.stack([xb[off[l]:off[l + 1]].mean(0) if sizes[l] else np.full(xb.shape[1], 9.0, np.float32)
                    for l in range(len(sizes))]).astype(np.float32)
    return np.ascontiguousarray(cen), off, np.arange(len(xb), dtype=np.int64), xb


def _first_layout(nq):
    xb, xq = C.lowrank_case(24_000, D64, 4, 0.02, nq, seed=21)
    return hand_lists(xb, [6000, 5990, 6100, 5910]), xq


def _short_list():
    """A list of 40 rows and one of 5000: the first 20 queries sit on rows of the short list (its 40 rows are all that
    list's chunk-0 slots hold), the other 20 are ordinary."""
    xb, xq = C.lowrank_case(5040, D64, 4, 0.02, 40, seed=31)
    rng = np.random.default_rng(32)
    xq = xq.copy()
    xq[:20] = xb[:20] + np.float32(1e-3) * rng.standard_normal((20, D64), dtype=np.float32)
    return hand_lists(xb, [40, 5000]), np.ascontiguousarray(xq)


def _ties(shape):
    rng = np.random.default_rng(24)
    if shape == "identical":
        base, xq = C.lowrank_case(1, D64, 4, 0.02, 40, seed=24)
        xb = np.ascontiguousarray(np.repeat(base, 3000, axis=0))
        return hand_lists(xb, [3000]), xq
    base, xq = C.lowrank_case(75, D64, 4, 0.02, 40, seed=25)
    xb = np.repeat(base, 40, axis=0)
    xb += np.float32(1e-3) * rng.standard_normal(xb.shape, dtype=np.float32)
    xb = np.ascontiguousarray(xb[rng.permutation(len(xb))])
    return hand_lists(xb, [3000]), xq


def _ragged():
    xb, xq = C.lowrank_case(2048 + 2049 + 100, D64, 4, 0.02, 40, seed=22)
    return hand_lists(xb, [2048, 2049, 100, 0]), xq


def _d768():
    xb, xq = C.lowrank_case(4200 + 300, 768, 16, 0.02, 64, seed=7)
    return hand_lists(xb, [4200, 300]), xq


# name -> (builder of (lists, xq), k, form, metric, fp16 image, remove-and-add first, seeded path expected)
CASES = {}
for _nq in (40, 97):
    for _k in (1, 10, 12):
        CASES[f"first_nq{_nq}_k{_k}"] = (lambda nq=_nq: _first_layout(nq), _k, 7, 0, False, False, 1)
CASES["ragged_2048_2049_100_0"] = (_ragged, 10, 7, 0, False, False, 1)
CASES["short_list"] = (_short_list, 10, 7, 0, False, False, 1)
CASES["ties_identical"] = (lambda: _ties("identical"), 10, 7, 0, False, False, 1)
CASES["ties_near_copies"] = (lambda: _ties("near_copies"), 10, 7, 0, False, False, 1)
CASES["d768_three_chunks"] = (_d768, 10, 7, 0, False, False, 1)
CASES["first_ip"] = (lambda: _first_layout(40), 10, 7, 1, False, False, 0)
CASES["first_fp16_image"] = (lambda: _first_layout(40), 10, 6, 0, True, False, 0)
CASES["first_remove_add"] = (lambda: _first_layout(40), 10, 7, 0, False, True, 1)


def run_case(hipann, name):
    """Answer the case on the GPU.  Returns a dict: D, I (and D2, I2 of a repeat), the flag count of the first search,
    the path, the lists searched (after the removal and the add, where the case has them) and the rows by label."""
    build, k, form, metric, fp16, churn, _ = CASES[name]
    (cen, off, ids, codes), xq = build()
    ix = hipann.HipIndexIVFFlat(cen, off, ids, codes, len(cen), metric)
    ix.form = form
    if fp16:
        ix.filter_image = ix.FILTER_FP16
    rows = codes
    if churn:
        rng = np.random.default_rng(41)
        gone = rng.choice(len(codes), 500, replace=False)
        assert ix.remove_ids(gone) == 500
        new = codes[rng.choice(len(codes), 500, replace=False)] + np.float32(5e-3) * rng.standard_normal(
            (500, codes.shape[1]), dtype=np.float32)
        ix.add(np.ascontiguousarray(new), np.arange(len(codes), len(codes) + 500, dtype=np.int64))
        rows = np.ascontiguousarray(np.concatenate([codes, new]))
        ex = ix.export()
        cen, off, ids, codes = ex["centroids"], ex["list_offsets"], ex["ids"], ex["codes"]
    fb0 = ix.rerank_fallbacks()
    D, I = ix.search(xq, k)
    flagged = ix.rerank_fallbacks() - fb0
    path = ix.last_search_path(seeded=True)
    probes = ix.last_probes(len(xq))
    D2, I2 = ix.search(xq, k)
    ix.close()
    return {"D": D, "I": I, "D2": D2, "I2": I2, "flagged": flagged, "path": path, "probes": probes,
            "lists": (cen, off, ids, codes), "rows": rows, "xq": xq, "k": k, "metric": metric}


if __name__ == "__main__":
    import hipann

    out = {}
    for name in CASES:
        r = run_case(hipann, name)
        assert r["path"]["seeded"] == 0, (name, r["path"])  # the switch is off in this process
        out[name + ".D"], out[name + ".I"] = r["D"], r["I"]
        out[name + ".flagged"] = np.int64(r["flagged"])
    np.savez(sys.argv[1], **out)
