"""Removing rows from an IVF SQ8 index in place on one MI355X: 2M x 768 L2, nlist 1024, by_residual 1, U(-1, 1) rows
(the data of tools/ivfsq_add_bench.py: trained and added on the device, then exported — the CSR every handle below is
created from).  One process; a failed step ends the run.  Per removal set — a uniformly random 1 % and 10 % of the ids,
and every id of the longest list — `--repeats` alternating rounds of

  remove   hipann_ivfsq_remove_ids on a freshly created handle over the whole CSR (wall time of the call; the creation
           is not timed); its return value and ntotal are checked
  rebuild  what a caller without remove_ids does for the same event: hipann_ivfsq_create over the surviving rows' CSR
           (wall time of the call: upload, tiling, row terms; the host walk that makes that CSR is NOT timed, which
           favours the rebuild)

and, once per set with kernel timing on, the removal kernel's own time (HIP events around the launch) beside the
bytes it has to touch — 8 per live row for the id lookup, 2·(32·nstep + 12) per moved row, 32·nstep + 12 per vacated
row — over 8 TB/s.  After the 10 % set: nq = 1024, k = 10, nprobe 32 searches on the handle the rows were removed from
and on the handle rebuilt over the survivors, alternating (device events), to show what shorter lists in unchanged
capacity cost the scan.  One JSON line per measurement on stdout (and in --out, when given): median, min, max in ms.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "duckdb-annsearch_amd"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch

    import hipann

    n, d, nlist = args.n, args.d, args.nlist
    g = torch.Generator(device="cuda").manual_seed(1234)
    xb = torch.rand((n, d), generator=g, device="cuda") * 2 - 1
    xq = (torch.rand((1024, d), generator=g, device="cuda") * 2 - 1).contiguous()
    cen = xb[:: n // nlist][:nlist].contiguous()
    vmin, vdiff = torch.empty(d, device="cuda"), torch.empty(d, device="cuda")
    torch.cuda.synchronize()
    hipann.ivfsq_train_device(d, nlist, n, xb.data_ptr(), cen.data_ptr(), vmin.data_ptr(), vdiff.data_ptr(),
                              hipann.METRIC_L2, True)
    cen_h, vmin_h, vdiff_h = cen.cpu().numpy(), vmin.cpu().numpy(), vdiff.cpu().numpy()
    sq = hipann.HipIndexIVFSQ8(cen_h, vmin_h, vdiff_h, np.zeros(nlist + 1, np.int64), np.zeros(0, np.int64),
                               np.zeros((0, d), np.uint8), metric=hipann.METRIC_L2)
    sq.add_device(n, xb.data_ptr())
    ex = sq.export()
    sq.close()
    del xb
    off, ids, codes = ex["list_offsets"], ex["ids"], ex["codes"]
    lens = np.diff(off)
    lst = np.repeat(np.arange(nlist), lens)
    pos = np.arange(n) - off[lst]
    raw = -(-d // 32)
    nstep = -(-raw // (4 if raw <= 4 else 8)) * (4 if raw <= 4 else 8)
    row_bytes = 32 * nstep + 12
    lines = []

    def emit(name, ms, **kw):
        rec = dict(measure=name, n=n, d=d, nlist=nlist, repeats=len(ms), median_ms=statistics.median(ms), min_ms=min(ms),
                   max_ms=max(ms), **kw)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def create(o, i, c):
        return hipann.HipIndexIVFSQ8(cen_h, vmin_h, vdiff_h, o, i, c, nprobe=args.nprobe, metric=hipann.METRIC_L2)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    rng = np.random.default_rng(7)
    longest = int(np.argmax(lens))
    sets = [("1pct", rng.choice(ids, n // 100, replace=False)), ("10pct", rng.choice(ids, n // 10, replace=False)),
            ("one_list", ids[off[longest]:off[longest + 1]].copy())]
    create(off, ids, codes).close()  # warm-up: code load, allocator
    for name, lab in sets:
        gone = np.isin(ids, lab)
        keep = ~gone
        s_off = np.concatenate([[0], np.cumsum(np.bincount(lst[keep], minlength=nlist))]).astype(np.int64)
        s_ids, s_codes = ids[keep], codes[keep]
        # the kernel's bytes: holes are the removed positions below the list's new length
        newlen = lens - np.bincount(lst[gone], minlength=nlist)
        moved = int((gone & (pos < newlen[lst])).sum())
        need = 8 * n + 2 * row_bytes * moved + row_bytes * int(gone.sum())
        rm, rb, kern = [], [], None
        kept_pair = None
        for r in range(args.repeats):
            h = create(off, ids, codes)
            if r == 0:
                h.set_kernel_timing(True)
            t, cnt = timed(lambda: h.remove_ids(lab))
            assert cnt == len(lab) and h.ntotal == n - len(lab), (cnt, h.ntotal)
            if r == 0:
                kern = h.kernel_ms(0)
                h.set_kernel_timing(False)
            rm.append(t)
            t, h2 = timed(lambda: create(s_off, s_ids, s_codes))
            rb.append(t)
            if name == "10pct" and r == args.repeats - 1:
                kept_pair = (h, h2)
            else:
                h.close()
                h2.close()
        emit(f"remove_{name}", rm, labels=len(lab), rows_moved=moved, kernel_ms=kern, kernel_bytes=need,
             bound_ms=need / 8e12 * 1e3, fraction_of_8TBps=need / (kern * 1e-3) / 8e12 if kern else None)
        emit(f"rebuild_{name}", rb, note="hipann_ivfsq_create over the survivors' CSR; the host walk is not timed")
        if kept_pair:
            k, nq = 10, 1024
            D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            I = [torch.empty((nq, k), dtype=torch.int64, device="cuda") for _ in range(2)]
            ms = ([], [])
            for r in range(args.repeats + 1):  # (the first round is the warm-up)
                for w, hh in enumerate(kept_pair):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    hh.search_device(nq, xq.data_ptr(), k, D.data_ptr(), I[w].data_ptr())
                    e1.record()
                    torch.cuda.synchronize()
                    if r:
                        ms[w].append(e0.elapsed_time(e1))
            emit("search_after_remove_10pct", ms[0], nq=nq, k=k, nprobe=args.nprobe,
                 same_ids_as_rebuilt=bool(torch.equal(I[0], I[1])))
            emit("search_rebuilt_10pct", ms[1], nq=nq, k=k, nprobe=args.nprobe)
            for hh in kept_pair:
                hh.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
