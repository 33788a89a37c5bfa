#!/usr/bin/env python3
"""What does removing rows on the resident GPU copy buy against the path it replaces?

The replaced path (parent commit): the copy is dropped and the next search pays a create from host rows over the
surviving rows plus its own first search (the lazy re-upload).  The new path: hipann_*_remove_ids on
the resident copy (its search images built) plus the first search after it.  Both are timed in this one process on the
same device, median of --reps after one warm-up, with the extension's per-query call shape (nq = 1 by default):

  flat  1M x 768, a random 1 % removed
  ivf   nlist 1024 over 2M x 768, nprobe 32, a random 1 % removed

One JSON line per case: remove_ms, rebuild_ms and their ratio, as measured — nothing is tuned.  Run it under a
`timeout`; --alarm also ends the process from inside after that many seconds.

    timeout 900 python tools/remove_timing.py --case flat --case ivf
"""
from __future__ import annotations

import argparse
import json
import signal
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "duckdb-annsearch_amd"))


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def _median(setup, run, reps):
    """run(setup()) timed reps + 1 times; the first is the warm-up.  Returns (median ms, all ms, last result)."""
    ms, res = [], None
    for _ in range(reps + 1):
        state = setup()
        t, res = _timed(lambda: run(state))
        ms.append(t)
        close = getattr(state, "close", None)
        if close:
            close()
    return statistics.median(ms[1:]), ms, res


def _rows(rng, n, d):
    out = np.empty((n, d), np.float32)
    for r0 in range(0, n, 1 << 18):
        out[r0:r0 + (1 << 18)] = rng.random((min(1 << 18, n - r0), d), dtype=np.float32) * 2 - 1
    return out


def case_flat(hipann, n, d, frac, nq, reps, seed):
    rng = np.random.default_rng(seed)
    xb = _rows(rng, n, d)
    xq = _rows(rng, max(nq, 1), d)
    labels = rng.choice(n, int(n * frac), replace=False).astype(np.int64)
    kept = np.ascontiguousarray(np.delete(xb, labels, 0))

    def resident():
        ix = hipann.HipIndexFlat(d, hipann.METRIC_L2, xb)
        ix.search(xq, 10)  # the copy a running extension holds: search images built
        return ix

    def remove(ix):
        removed = ix.remove_ids(labels)
        return removed, ix.search(xq, 10)

    def rebuild(_):
        ix = hipann.HipIndexFlat(d, hipann.METRIC_L2, kept)
        out = ix.search(xq, 10)
        ix.close()
        return out

    rm_ms, rm_all, (removed, (_, I1)) = _median(resident, remove, reps)
    rb_ms, rb_all, (_, I2) = _median(lambda: None, rebuild, reps)
    return {"case": "flat", "n": n, "d": d, "removed": int(removed), "nq": nq, "remove_ms": round(rm_ms, 3),
            "rebuild_ms": round(rb_ms, 3), "rebuild_over_remove": round(rb_ms / rm_ms, 2),
            "ids_equal": bool(np.array_equal(I1, I2)), "remove_all_ms": [round(v, 2) for v in rm_all],
            "rebuild_all_ms": [round(v, 2) for v in rb_all]}


def case_ivf(hipann, n, d, nlist, nprobe, frac, nq, reps, seed):
    rng = np.random.default_rng(seed)
    xb = _rows(rng, n, d)
    xq = _rows(rng, max(nq, 1), d)
    cen = np.ascontiguousarray(xb[:: n // nlist][:nlist])
    # list assignment on the GPU (k = 1 over the centroids), CSR in insertion order
    cq = hipann.HipIndexFlat(d, hipann.METRIC_L2, cen)
    a = np.concatenate([cq.search(xb[r0:r0 + 65536], 1)[1][:, 0] for r0 in range(0, n, 65536)])
    cq.close()
    order = np.argsort(a, kind="stable").astype(np.int64)
    off = np.zeros(nlist + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(a, minlength=nlist))
    codes = np.ascontiguousarray(xb[order])
    del xb
    labels = rng.choice(n, int(n * frac), replace=False).astype(np.int64)
    keep = ~np.isin(order, labels)
    koff = np.zeros(nlist + 1, np.int64)
    koff[1:] = np.cumsum(np.bincount(np.repeat(np.arange(nlist), np.diff(off))[keep], minlength=nlist))
    kids, kcodes = order[keep], np.ascontiguousarray(codes[keep])

    def resident():
        ix = hipann.HipIndexIVFFlat(cen, off, order, codes, nprobe)
        ix.search(xq, 10)  # fp16 image built
        return ix

    def remove(ix):
        removed = ix.remove_ids(labels)
        return removed, ix.search(xq, 10)

    def rebuild(_):
        ix = hipann.HipIndexIVFFlat(cen, koff, kids, kcodes, nprobe)
        out = ix.search(xq, 10)
        ix.close()
        return out

    rm_ms, rm_all, (removed, (_, I1)) = _median(resident, remove, reps)
    rb_ms, rb_all, (_, I2) = _median(lambda: None, rebuild, reps)
    return {"case": "ivf", "n": n, "d": d, "nlist": nlist, "nprobe": nprobe, "removed": int(removed), "nq": nq,
            "remove_ms": round(rm_ms, 3), "rebuild_ms": round(rb_ms, 3), "rebuild_over_remove": round(rb_ms / rm_ms, 2),
            "ids_equal": bool(np.array_equal(I1, I2)), "remove_all_ms": [round(v, 2) for v in rm_all],
            "rebuild_all_ms": [round(v, 2) for v in rb_all]}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", action="append", choices=["flat", "ivf"])
    ap.add_argument("--flat-n", type=int, default=1_000_000)
    ap.add_argument("--ivf-n", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--frac", type=float, default=0.01)
    ap.add_argument("--nq", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--alarm", type=int, default=900, help="seconds after which the process ends itself")
    args = ap.parse_args()
    signal.alarm(args.alarm)
    import hipann

    if not hipann.is_available():
        print("remove_timing: no gfx950 device", file=sys.stderr)
        return 1
    print(json.dumps({"device": hipann.device_info(), "reps": args.reps, "frac": args.frac}), flush=True)
    for c in args.case or ["flat", "ivf"]:
        if c == "flat":
            r = case_flat(hipann, args.flat_n, args.d, args.frac, args.nq, args.reps, args.seed)
        else:
            r = case_ivf(hipann, args.ivf_n, args.d, args.nlist, args.nprobe, args.frac, args.nq, args.reps, args.seed)
        print(json.dumps(r), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
