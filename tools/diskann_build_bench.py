#!/usr/bin/env python3
"""Time the GPU DiskANN graph build (DiskannDeviceDB.build_graph) and measure what it buys.

One JSON line per shape: build seconds in total and per phase (searches, out-edge prunes, back-edges), the build's
counters, recall@10 at L against brute force through the resident traversal, and beside it the setup time and the
recall of diskann_build.knn_graph (the benchmark's stand-in graph) at the same R, L and entry point.

    python tools/diskann_build_bench.py --shape 100000x128 --R 64 --L 128
    python tools/diskann_build_bench.py --shape 1000000x1536 --R 64 --L 128 --batch-max 4096

Rows are synthetic (clustered Gaussians by default, --dist gaussian for one isotropic blob); nothing outside the
repository is read.
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


def make_rows(torch, n, d, nq, dist, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    if dist == "gaussian":
        x = torch.randn((n, d), generator=g, device="cuda")
        q = torch.randn((nq, d), generator=g, device="cuda")
        return x, q
    nc = max(1, min(1024, n // 256))
    cen = torch.randn((nc, d), generator=g, device="cuda")
    x = cen[torch.randint(0, nc, (n,), generator=g, device="cuda")]
    x += 0.5 * torch.randn((n, d), generator=g, device="cuda")
    q = cen[torch.randint(0, nc, (nq,), generator=g, device="cuda")] + 0.5 * torch.randn((nq, d), generator=g, device="cuda")
    return x, q


def recall10(db, ep, q, truth, L):
    ids, _, st = db.search_batch_resident([ep], q, 10, L)
    hit = sum(len(set(ids[i]) & set(truth[i])) for i in range(q.shape[0]))
    return hit / (10.0 * q.shape[0]), st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", required=True, help="NxD, repeatable")
    ap.add_argument("--R", type=int, default=64)
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--alpha", type=float, default=1.2)
    ap.add_argument("--batch-max", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dist", choices=["clustered", "gaussian"], default="clustered")
    ap.add_argument("--entry", choices=["medoid", "zero"], default="medoid")
    ap.add_argument("--skip-knn", action="store_true", help="leave out the knn_graph comparison")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch

    import diskann_build as B
    import hipann

    for shape in a.shape:
        n, d = (int(v) for v in shape.lower().split("x"))
        x, q = make_rows(torch, n, d, a.nq, a.dist, a.seed)
        truth = B.exact_topk(torch, x, q, 10).cpu().numpy()
        xh = x.cpu().numpy()
        qh = q.cpu().numpy()
        ep = hipann.medoid(xh) if a.entry == "medoid" else 0
        db = hipann.DiskannDeviceDB(xh)
        print(f"[{shape}] rows resident, building (R {a.R}, L {a.L}, batch_max {a.batch_max}, entry {ep})",
              file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        adj, st = db.build_graph(R=a.R, L=a.L, alpha=a.alpha, entry_point=ep, batch_max=a.batch_max)
        build_s = time.perf_counter() - t0
        rec, sst = recall10(db, ep, qh, truth, a.L)
        deg = (adj != 0xFFFFFFFF).sum(1)
        out = {"shape": shape, "dist": a.dist, "R": a.R, "L": a.L, "alpha": a.alpha, "batch_max": a.batch_max,
               "entry_point": int(ep), "build_s": round(build_s, 4), "search_s": round(st["search_s"], 4),
               "out_prune_s": round(st["out_prune_s"], 4), "back_edge_s": round(st["back_edge_s"], 4),
               "search_share": round(st["search_s"] / build_s, 4), "rows_per_s": round(n / build_s, 1),
               "stats": {k: v for k, v in st.items() if not k.endswith("_s")}, "mean_degree": round(float(deg.mean()), 2),
               "recall_at_10": round(rec, 4), "search_evals_per_query": round(sst["evals"] / a.nq, 1)}
        if not a.skip_knn:
            print(f"[{shape}] built in {build_s:.1f} s; knn_graph for comparison", file=sys.stderr, flush=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kadj, kmed = B.knn_graph(torch, x, R=a.R)
            torch.cuda.synchronize()
            out["knn_graph_setup_s"] = round(time.perf_counter() - t0, 4)
            db.register_graph(B.adjacency_u32(torch, kadj))
            krec, kst = recall10(db, kmed, qh, truth, a.L)
            out["knn_graph_recall_at_10"] = round(krec, 4)
            out["knn_graph_evals_per_query"] = round(kst["evals"] / a.nq, 1)
        db.close()
        del x, q
        torch.cuda.empty_cache()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
