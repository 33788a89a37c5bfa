#!/usr/bin/env python3
"""Time DiskannDeviceDB.add_rows against the only alternative without it: registering all rows and
running a full build_graph.

Per data set and added fraction f the graph of the first (1 − f)·N rows is built once on the GPU; then, alternating
--repeat times: add_rows of the remaining rows onto a fresh handle holding that graph, once with batch_mates = 0 and
once with --mates (16), and DiskannDeviceDB(all rows) + build_graph from the same entry point.  One JSON line per data
set and fraction: the seconds of each call (medians; add_rows also per phase: searches, mates, out-edge prunes,
back-edges — the phases and counters are those of the median call), recall@10 at L of the three graphs through the
resident traversal against brute force over all rows, for queries drawn like the old rows and like the added rows, the
rows the entry point does not reach, and the cost of a one-row call into the finished graph with and without the
adjacency read back.  Data sets: "iid" (every row N(0, 1): the added rows are like the old ones) and "burst" (old rows
around many cluster centres, added rows around --new-centres new ones: a new document or tenant).  With --out-dir the
lines also go to <dir>/add_bench.jsonl and a README.md with the tables is written beside them.

    python tools/diskann_add_bench.py --shape 100000x128 --R 64 --L 128 --out-dir profiles/diskann_add

Rows are synthetic; nothing outside the repository is read.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "duckdb-annsearch_amd"))
sys.path.insert(0, str(ROOT / "tools"))


def make_sets(torch, kind, n0, m, d, nq, new_centres, seed):
    """(old rows, added rows, queries like the old rows, queries like the added rows) on the device."""
    from diskann_build_bench import make_rows

    g = torch.Generator(device="cuda")
    g.manual_seed(seed + 1000)
    if kind == "iid":
        x_old, q_old = make_rows(torch, n0, d, nq, "gaussian", seed)
        x_new = torch.randn((m, d), generator=g, device="cuda")
        q_new = torch.randn((nq, d), generator=g, device="cuda")
        return x_old, x_new, q_old, q_new
    x_old, q_old = make_rows(torch, n0, d, nq, "clustered", seed)
    cen = torch.randn((new_centres, d), generator=g, device="cuda")
    x_new = cen[torch.randint(0, new_centres, (m,), generator=g, device="cuda")]
    x_new = x_new + 0.5 * torch.randn((m, d), generator=g, device="cuda")
    q_new = cen[torch.randint(0, new_centres, (nq,), generator=g, device="cuda")]
    q_new = q_new + 0.5 * torch.randn((nq, d), generator=g, device="cuda")
    return x_old, x_new, q_old, q_new


def median(runs):
    runs = sorted(runs, key=lambda r: r[0])
    return runs[len(runs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="100000x128", help="NxD (N: rows after the add)")
    ap.add_argument("--R", type=int, default=64)
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--alpha", type=float, default=1.2)
    ap.add_argument("--batch-max", type=int, default=4096)
    ap.add_argument("--mates", type=int, default=16)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--fraction", type=float, action="append", help="added fraction, repeatable (default 0.01 0.1 0.3)")
    ap.add_argument("--dataset", action="append", choices=["iid", "burst"], help="repeatable (default both)")
    ap.add_argument("--new-centres", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3, help="timed repetitions of each side (the median is reported)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out-dir", default=None, help="write add_bench.jsonl and README.md here")
    a = ap.parse_args()
    fractions = a.fraction or [0.01, 0.1, 0.3]
    datasets = a.dataset or ["iid", "burst"]

    import torch

    import diskann_build as B
    import hipann
    from diskann_build_bench import recall10

    n, d = (int(v) for v in a.shape.lower().split("x"))
    lines = []
    for kind in datasets:
        for frac in fractions:
            m = max(1, int(round(frac * n)))
            n0 = n - m
            x_old, x_new, q_old, q_new = make_sets(torch, kind, n0, m, d, a.nq, a.new_centres, a.seed)
            x_all = torch.cat([x_old, x_new])
            truth = {"old": B.exact_topk(torch, x_all, q_old, 10).cpu().numpy(),
                     "new": B.exact_topk(torch, x_all, q_new, 10).cpu().numpy()}
            qs = {"old": q_old.cpu().numpy(), "new": q_new.cpu().numpy()}
            xo, xn, xa = x_old.cpu().numpy(), x_new.cpu().numpy(), x_all.cpu().numpy()
            ep = hipann.medoid(xo)
            h = hipann.DiskannDeviceDB(xo)
            base, bst = h.build_graph(R=a.R, L=a.L, alpha=a.alpha, entry_point=ep, batch_max=a.batch_max)
            h.close()
            runs = {0: [], a.mates: [], "rebuild": []}
            rec, one = {}, {}
            for rep in range(a.repeat):
                for T in (0, a.mates):
                    h = hipann.DiskannDeviceDB(xo)
                    h.register_graph(base)
                    t0 = time.perf_counter()
                    _, st = h.add_rows(xn, ep, L=a.L, alpha=a.alpha, batch_max=a.batch_max, batch_mates=T)
                    runs[T].append((time.perf_counter() - t0, st))
                    if rep == a.repeat - 1:
                        rec[T] = {w: round(recall10(h, ep, qs[w], truth[w], a.L)[0], 4) for w in ("old", "new")}
                        if T == a.mates:  # one more row into the finished graph, the adjacency left on the device / read back
                            for want in (False, True):
                                ts = []
                                for i in range(5):
                                    t0 = time.perf_counter()
                                    h.add_rows(xn[i:i + 1], ep, L=a.L, alpha=a.alpha, batch_max=a.batch_max,
                                               batch_mates=T, want_adjacency=want)
                                    ts.append(time.perf_counter() - t0)
                                one["with_adjacency_s" if want else "s"] = round(sorted(ts)[2], 6)
                    h.close()
                t0 = time.perf_counter()
                h = hipann.DiskannDeviceDB(xa)
                _, rst = h.build_graph(R=a.R, L=a.L, alpha=a.alpha, entry_point=ep, batch_max=a.batch_max)
                runs["rebuild"].append((time.perf_counter() - t0, rst))
                if rep == a.repeat - 1:
                    rec["rebuild"] = {w: round(recall10(h, ep, qs[w], truth[w], a.L)[0], 4) for w in ("old", "new")}
                h.close()
            out = {"shape": a.shape, "dataset": kind, "R": a.R, "L": a.L, "alpha": a.alpha, "batch_max": a.batch_max,
                   "fraction": frac, "added": m, "repeat": a.repeat, "base_build_s": round(bst["search_s"] +
                   bst["out_prune_s"] + bst["back_edge_s"], 4)}
            bs, rst = median(runs["rebuild"])
            out["rebuild"] = {"s": round(bs, 4), "s_all": [round(r[0], 4) for r in sorted(runs["rebuild"], key=lambda r: r[0])],
                              "unreachable": rst["unreachable"], "recall_at_10": rec["rebuild"]}
            for T in (0, a.mates):
                s, st = median(runs[T])
                out[f"add_mates_{T}"] = {
                    "s": round(s, 4), "s_all": [round(r[0], 4) for r in sorted(runs[T], key=lambda r: r[0])],
                    "search_s": round(st["search_s"], 4), "mates_s": round(st["mates_s"], 4),
                    "out_prune_s": round(st["out_prune_s"], 4), "back_edge_s": round(st["back_edge_s"], 4),
                    "mates_share": round(st["mates_s"] / s, 4), "add_over_rebuild": round(s / bs, 4),
                    "stats": {k: v for k, v in st.items() if not k.endswith("_s")}, "recall_at_10": rec[T]}
            out["one_row"] = one
            lines.append(out)
            print(json.dumps(out), flush=True)
    if a.out_dir:
        write_report(Path(a.out_dir), a, lines)


def write_report(out_dir, a, lines):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "add_bench.jsonl").write_text("".join(json.dumps(o) + "\n" for o in lines))
    T = a.mates
    t = ["# Inserting rows into the device DiskANN graph (`diskann_hip_add_rows`, DESIGN §6.3)", "",
         f"Written by `tools/diskann_add_bench.py --shape {a.shape} --R {a.R} --L {a.L}` on one GPU, one process: "
         f"{a.nq} queries per kind, entry point = the medoid of the old rows, alpha {a.alpha}, batch_max {a.batch_max}. "
         f"Per data set and added fraction the graph of the old rows is built once; `add_rows` of the added rows onto a "
         f"fresh handle holding that graph (batch_mates 0 and {T}) alternates {a.repeat} times with the alternative: a "
         "new `DiskannDeviceDB` of all rows plus a full `build_graph` from the same entry point. Call times are host "
         "clocks around the synchronous calls (the Python wrapper and the read-back of the adjacency included), medians, "
         "all repetitions in `add_bench.jsonl`; the phases are the call's own host clocks around its stream "
         "synchronisations. `iid`: every row N(0, 1). `burst`: old rows around many centres, added rows around "
         f"{a.new_centres} new centres. Recall@10 at L = {a.L} is over all rows, for queries like the old rows / like "
         "the added rows.", "",
         f"| data | added | add s (mates 0) | add s (mates {T}) | searches s | mates s | out-edge prunes s | back-edges s | "
         f"mates share | rebuild s | add / rebuild | recall old/new: mates 0 | mates {T} | rebuild | unreachable: "
         f"mates 0 / {T} / rebuild |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for o in lines:
        a0, aT, rb = o["add_mates_0"], o[f"add_mates_{T}"], o["rebuild"]
        rc = lambda r: f"{r['recall_at_10']['old']} / {r['recall_at_10']['new']}"  # noqa: E731
        t.append(f"| {o['dataset']} | {100 * o['fraction']:g} % | {a0['s']} | {aT['s']} | {aT['search_s']} | "
                 f"{aT['mates_s']} | {aT['out_prune_s']} | {aT['back_edge_s']} | {aT['mates_share']} | {rb['s']} | "
                 f"{aT['add_over_rebuild']} | {rc(a0)} | {rc(aT)} | {rc(rb)} | {a0['stats']['unreachable']} / "
                 f"{aT['stats']['unreachable']} / {rb['unreachable']} |")
    t += ["", f"The phase columns are those of the mates-{T} call.", "",
          "One more row into the finished graph (median of 5 calls): " +
          "; ".join(f"{o['dataset']} {100 * o['fraction']:g} %: {1e3 * o['one_row']['s']:.2f} ms without the adjacency, "
                    f"{1e3 * o['one_row']['with_adjacency_s']:.2f} ms with it read back" for o in lines) + "."]
    lost = [o for o in lines if o[f"add_mates_{T}"]["add_over_rebuild"] >= 1.0]
    t += ["", ("`add_rows` was the faster call at every data set and fraction above." if not lost else
               "`add_rows` was SLOWER than the rebuild at: " +
               ", ".join(f"{o['dataset']} {100 * o['fraction']:g} %" for o in lost) + ".")]
    big = [o for o in lines if o[f"add_mates_{T}"]["mates_s"] > o[f"add_mates_{T}"]["out_prune_s"]]
    t += ["", ("The mates step cost less than the out-edge prunes in every run above." if not big else
               "The mates step cost MORE than the out-edge prunes at: " +
               ", ".join(f"{o['dataset']} {100 * o['fraction']:g} %" for o in big) + ".")]
    (out_dir / "README.md").write_text("\n".join(t) + "\n")


if __name__ == "__main__":
    main()
