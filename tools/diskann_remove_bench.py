#!/usr/bin/env python3
"""Time DiskannDeviceDB.remove_ids against the only alternative without it: registering the survivors
and running a full build_graph.

The graph is built once on the GPU.  Per removed fraction, one JSON line: remove_ids' seconds in total and per phase
(pool build, prune, the rest: entry point, compaction, copies) and its counters; the seconds of
DiskannDeviceDB(survivors) + build_graph; for both graphs recall@10 at L against brute force over the survivors through
the resident traversal, and the rows their entry point does not reach; and the ratio of the two times.  The entry point
(the medoid) is always among the removed rows, so every timed call also finds its replacement.  The two sides alternate
--repeat times; the times reported are the medians, the counters and per-phase seconds are those of the median call,
and the recalls are the last repetition's (the results are the same in every repetition: nothing in either call depends
on timing).  With --out-dir the lines also go to <dir>/remove_bench.jsonl and a README.md with the table, the prune's
share and the ratios is written beside them.

    python tools/diskann_remove_bench.py --shape 100000x128 --R 64 --L 128 --out-dir profiles/diskann_remove

Rows are synthetic (diskann_build_bench.make_rows); nothing outside the repository is read.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "duckdb-annsearch_amd"))
sys.path.insert(0, str(ROOT / "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="100000x128", help="NxD")
    ap.add_argument("--R", type=int, default=64)
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--alpha", type=float, default=1.2)
    ap.add_argument("--batch-max", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--fraction", type=float, action="append", help="removed fraction, repeatable (default 0.01 0.1 0.3)")
    ap.add_argument("--dist", choices=["clustered", "gaussian"], default="clustered")
    ap.add_argument("--scratch-words", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3, help="timed repetitions of each side (the median is reported)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--metric", choices=["l2", "ip"], default="l2", help="the handles' graph metric (DESIGN §6.5)")
    ap.add_argument("--out-dir", default=None, help="write remove_bench.jsonl and README.md here")
    a = ap.parse_args()
    fractions = a.fraction or [0.01, 0.1, 0.3]
    gm = 1 if a.metric == "ip" else 0

    import torch

    import diskann_build as B
    import hipann
    from diskann_build_bench import make_rows, recall10

    n, d = (int(v) for v in a.shape.lower().split("x"))
    x, q = make_rows(torch, n, d, a.nq, a.dist, a.seed)
    xh, qh = x.cpu().numpy(), q.cpu().numpy()
    ep = hipann.medoid(xh)
    db = hipann.DiskannDeviceDB(xh, graph_metric=gm)
    t0 = time.perf_counter()
    adj, bst = db.build_graph(R=a.R, L=a.L, alpha=a.alpha, entry_point=ep, batch_max=a.batch_max)
    build_s = time.perf_counter() - t0
    print(f"[{a.shape}] built in {build_s:.2f} s (unreachable {bst['unreachable']})", file=sys.stderr,
          flush=True)
    db.close()
    lines = []
    for frac in fractions:
        m = max(1, int(round(frac * n)))
        others = np.random.default_rng(a.seed + int(frac * 1e6)).permutation(n)
        gone = np.concatenate([[ep], others[others != ep][:m - 1]]).astype(np.int64)  # the entry point leaves too
        live = np.setdiff1d(np.arange(n), gone)
        xl = np.ascontiguousarray(xh[live])
        truth = B.exact_topk(torch, x[torch.from_numpy(live).cuda()], q, 10, metric=gm).cpu().numpy()
        rem, reb = [], []
        for _ in range(a.repeat):
            h = hipann.DiskannDeviceDB(xh, graph_metric=gm)
            h.register_graph(adj)
            t0 = time.perf_counter()
            nadj, nep, st = h.remove_ids(gone, ep, alpha=a.alpha, scratch_words=a.scratch_words)
            rem.append((time.perf_counter() - t0, st))
            rec_rem, sst_rem = recall10(h, nep, qh, truth, a.L, gm)
            h.close()
            t0 = time.perf_counter()
            h = hipann.DiskannDeviceDB(xl, graph_metric=gm)
            _, rst = h.build_graph(R=a.R, L=a.L, alpha=a.alpha, entry_point=nep, batch_max=a.batch_max)
            reb.append((time.perf_counter() - t0, rst))
            rec_reb, sst_reb = recall10(h, nep, qh, truth, a.L, gm)
            h.close()
        rem.sort(key=lambda r: r[0])
        reb.sort(key=lambda r: r[0])
        (rs, st), (bs, rst) = rem[len(rem) // 2], reb[len(reb) // 2]
        deg = (nadj != 0xFFFFFFFF).sum(1)
        out = {"shape": a.shape, "metric": a.metric, "dist": a.dist, "R": a.R, "L": a.L, "alpha": a.alpha, "fraction": frac,
               "removed": st["removed"], "repeat": a.repeat,
               "remove_s": round(rs, 4), "remove_s_all": [round(r[0], 4) for r in rem],
               "pool_s": round(st["pool_s"], 4), "prune_s": round(st["prune_s"], 4),
               "compact_s": round(st["compact_s"], 4), "prune_share": round(st["prune_s"] / rs, 4),
               "stats": {k: v for k, v in st.items() if not k.endswith("_s")},
               "mean_degree": round(float(deg.mean()), 2),
               "remove_recall_at_10": round(rec_rem, 4), "remove_evals_per_query": round(sst_rem["evals"] / a.nq, 1),
               "rebuild_s": round(bs, 4), "rebuild_s_all": [round(r[0], 4) for r in reb],
               "rebuild_recall_at_10": round(rec_reb, 4), "rebuild_unreachable": rst["unreachable"],
               "rebuild_evals_per_query": round(sst_reb["evals"] / a.nq, 1),
               "remove_over_rebuild": round(rs / bs, 4)}
        lines.append(out)
        print(json.dumps(out), flush=True)
    if a.out_dir:
        write_report(Path(a.out_dir), a, lines, build_s, bst)


def write_report(out_dir, a, lines, build_s, bst):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "remove_bench.jsonl").write_text("".join(json.dumps(o) + "\n" for o in lines))
    t = [f"# Removing rows from the device DiskANN graph (`diskann_hip_remove_ids`, DESIGN §6.2)", "",
         f"Written by `tools/diskann_remove_bench.py --shape {a.shape} --R {a.R} --L {a.L}` on one GPU, one process: "
         f"{a.dist} rows, {a.nq} queries, entry point = the medoid (always among the removed rows), alpha {a.alpha}. "
         f"The graph is built once ({build_s:.2f} s, {bst['unreachable']} rows unreachable). Per removed fraction "
         f"`remove_ids` on a fresh handle holding that graph alternates {a.repeat} times with the alternative: a new "
         "`DiskannDeviceDB` of the survivors plus a full `build_graph` from the same entry point. Call times are host "
         "clocks around the synchronous calls (the Python wrapper included), medians, all repetitions in "
         "`remove_bench.jsonl`. Pool build = host time of mark, rank, pool lengths and the slab plan plus the pool "
         "fills' device time (events); prune = `vamana_prune`'s device time (events); rest = entry point, compaction, "
         "copies to the host. `resource_usage.txt`: registers, LDS and scratch of the new kernels; `NOTES.md`: what "
         "the numbers of the committed run say.", "",
         "| removed | `remove_ids` s | pool build s | prune s | rest s | prune share | rows repaired | pools over 256 | "
         "slabs | rebuild s | remove / rebuild | recall@10 removed / rebuilt | unreachable removed / rebuilt |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for o in lines:
        st = o["stats"]
        t.append(f"| {100 * o['fraction']:g} % | {o['remove_s']} | {o['pool_s']} | {o['prune_s']} | {o['compact_s']} | "
                 f"{o['prune_share']} | {st['repaired']} | {st['pools_truncated']} | {st['slabs']} | {o['rebuild_s']} | "
                 f"{o['remove_over_rebuild']} | {o['remove_recall_at_10']} / {o['rebuild_recall_at_10']} | "
                 f"{st['unreachable']} / {o['rebuild_unreachable']} |")
    lost = [o for o in lines if o["remove_over_rebuild"] >= 1.0]
    t += ["", ("`remove_ids` was the faster call at every fraction above." if not lost else
               "`remove_ids` was SLOWER than the rebuild at: " +
               ", ".join(f"{100 * o['fraction']:g} %" for o in lost) + ".")]
    (out_dir / "README.md").write_text("\n".join(t) + "\n")


if __name__ == "__main__":
    main()
