#!/usr/bin/env python3
"""Time the device-side SQ8 copy and entry point of a DiskANN DB (DiskannDeviceDB.quantize_sq8 / .medoid)
against what a caller does without them, in one process:

  quantize_sq8 (three phases)  vs  oracle.sq8_train + sq8_encode on the host's threads, then DiskannDeviceDB(codes, 1,
                                   mins, scale) + register_graph(adjacency) — the upload of n*d codes and of the
                                   adjacency a second time (the read-back of the rows, or keeping a host copy of them,
                                   is not counted: this tool has the host copy anyway)
                               vs  diskann_build.sq8_encode, the benchmark's torch encoder on the device (codec only:
                                   no handle, no graph)
  medoid                       vs  hipann.medoid on the host

One JSON line per shape: the seconds of every side (device calls: the median of --repeat and all repetitions; the
host sides run --host-repeat times and count with their fastest repetition), the phases of the median quantize call and the bandwidths they imply (bytes:
n*d*4 for the statistics, n*d*5 for the encode, n*d*4 for each of the medoid's two passes).  The adjacency is random
ids of degree --R: the copy's cost does not depend on its contents.  Every GPU step runs under its own time limit; a
step that overruns it ends the process, and nothing more is started.  With --out-dir the lines also go to
<dir>/sq8_bench.jsonl and a README.md with the tables is written beside them.

    python tools/diskann_sq8_bench.py --shape 100000x128 --shape 1000000x1536 --out-dir profiles/diskann_sq8

Rows are synthetic; nothing outside the repository is read.
"""
from __future__ import annotations

import argparse
import json
import os
import signal
import sys
import time
from contextlib import contextmanager
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "duckdb-annsearch_amd"))
sys.path.insert(0, str(ROOT))

HBM_PEAK_TBS = 8.0      # HBM3E, data sheet
HBM_STREAM_TBS = 6.3    # what a float4 copy kernel reaches on this part


@contextmanager
def step(name, limit_s):
    """One GPU step under its own time limit: when it overruns, say so and end the process at once."""
    def over(signum, frame):
        sys.stderr.write(f"[sq8-bench] step '{name}' passed its limit of {limit_s} s: stopping\n")
        sys.stderr.flush()
        os._exit(124)

    old = signal.signal(signal.SIGALRM, over)
    signal.alarm(int(limit_s))
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def med(ts):
    return sorted(ts)[len(ts) // 2]


def tbs(nbytes, s):
    return round(nbytes / s / 1e12, 3) if s > 0 else None


def run_shape(a, shape):
    import numpy as np
    import torch

    import diskann_build as B
    import hipann
    from oracle import oracle as O

    n, d = (int(v) for v in shape.lower().split("x"))
    nd = n * d
    limit = a.step_limit
    with step("rows", limit):
        g = torch.Generator(device="cuda")
        g.manual_seed(a.seed)
        xt = torch.randn((n, d), generator=g, device="cuda")
        x = xt.cpu().numpy()
        adj = torch.randint(0, n, (n, a.R), generator=g, device="cuda", dtype=torch.int64).to(torch.int32).cpu().numpy()
        adj = adj.view(np.uint32)
    with step("register", limit):
        db = hipann.DiskannDeviceDB(x)
        db.register_graph(adj)

    # ---- device: quantize_sq8 and medoid ----
    qruns, mruns = [], []
    codes_dev = None
    for rep in range(a.repeat + 1):  # (the first repetition warms up: code objects, allocations)
        with step("quantize_sq8", limit):
            t0 = time.perf_counter()
            q8 = db.quantize_sq8()
            dt = time.perf_counter() - t0
            if rep:
                qruns.append((dt, dict(db.quantize_seconds)))
            if rep == a.repeat:
                codes_dev = q8.export_sq8()
            q8.close()
        with step("medoid", limit):
            t0 = time.perf_counter()
            row = db.medoid()
            dt = time.perf_counter() - t0
            if rep:
                mruns.append(dt)
    db.close()
    qruns.sort(key=lambda r: r[0])
    qs, qph = qruns[len(qruns) // 2]

    # ---- today: the codec on the host, then a second handle with a second upload of the adjacency ----
    hruns = []
    for rep in range(a.host_repeat):
        t0 = time.perf_counter()
        mins, scale = O.sq8_train(x)
        t1 = time.perf_counter()
        codes = O.sq8_encode(x, mins, scale)
        t2 = time.perf_counter()
        with step("register codes", limit):
            h = hipann.DiskannDeviceDB(codes, 1, mins, scale)
            h.register_graph(adj)
            t3 = time.perf_counter()
            h.close()
        hruns.append((t3 - t0, {"train_s": t1 - t0, "encode_s": t2 - t1, "register_s": t3 - t2}))
    hruns.sort(key=lambda r: r[0])
    hs, hph = hruns[0]  # (the host sides count with their fastest repetition)
    same = bool(np.array_equal(codes, codes_dev[0]) and np.array_equal(mins, codes_dev[1]) and
                np.array_equal(scale, codes_dev[2]))

    # ---- the benchmark's torch encoder on the device (codec only) ----
    truns = []
    for rep in range(a.repeat + 1):
        with step("torch encoder", limit):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tc, tm, ts = B.sq8_encode(torch, xt)
            torch.cuda.synchronize()
            if rep:
                truns.append(time.perf_counter() - t0)
            del tc, tm, ts

    # ---- hipann.medoid on the host ----
    hm = []
    for rep in range(a.host_repeat):
        t0 = time.perf_counter()
        row_host = hipann.medoid(x)
        hm.append(time.perf_counter() - t0)

    out = {
        "shape": shape, "n": n, "d": d, "R": a.R, "repeat": a.repeat, "host_repeat": a.host_repeat,
        "host_threads": int(O.lib().oracle_num_threads()),
        "quantize_sq8": {"s": round(qs, 6), "s_all": [round(r[0], 6) for r in qruns],
                         "stats_s": round(qph["stats_s"], 6), "encode_s": round(qph["encode_s"], 6),
                         "rest_s": round(qph["rest_s"], 6),
                         "stats_tb_s": tbs(nd * 4, qph["stats_s"]), "encode_tb_s": tbs(nd * 5, qph["encode_s"]),
                         "equals_host_codec": same},
        "host_codec_and_register": {"s": round(hs, 4), "s_all": [round(r[0], 4) for r in hruns],
                                    **{k: round(v, 4) for k, v in hph.items()}},
        "torch_encoder": {"s": round(med(truns), 6), "s_all": [round(t, 6) for t in sorted(truns)]},
        "medoid": {"s": round(med(mruns), 6), "s_all": [round(t, 6) for t in sorted(mruns)],
                   "tb_s_two_passes": tbs(nd * 8, med(mruns)), "row": int(row)},
        "host_medoid": {"s": round(min(hm), 4), "s_all": [round(t, 4) for t in sorted(hm)], "row": int(row_host)},
    }
    out["quantize_over_host"] = round(qs / hs, 5)
    out["slowest_quantize_over_host"] = round(qruns[-1][0] / hs, 5)
    out["quantize_over_torch_encoder"] = round(qs / med(truns), 4)
    out["slowest_quantize_over_torch_encoder"] = round(qruns[-1][0] / med(truns), 4)
    out["medoid_over_host"] = round(med(mruns) / min(hm), 5)
    return out


def write_report(out_dir, a, lines):
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "sq8_bench.jsonl").write_text("".join(json.dumps(o) + "\n" for o in lines))
    t = ["# SQ8 search copy and entry point on the device (`diskann_hip_quantize_sq8`, `diskann_hip_medoid`, DESIGN §6.4)",
         "",
         "Written by `tools/diskann_sq8_bench.py " + " ".join(f"--shape {o['shape']}" for o in lines) +
         f"` on one GPU, one process. Rows are N(0, 1); the adjacency is random ids of degree {a.R}. Times are host "
         f"clocks around the synchronous calls, the Python wrapper included; device calls: median of {a.repeat} after a "
         f"warm-up call, host sides: the fastest of {a.host_repeat}; every repetition is in `sq8_bench.jsonl`. The phases "
         "are the call's own host clocks around its stream synchronisations: [0] column statistics (two kernels and the "
         "read-back of 2·d floats), [1] encode, [2] the rest (allocations, finite check — one more read of the rows —, "
         "decode tables, device-to-device copy of the graph). Bandwidths count n·d·4 bytes for the statistics, n·d·5 for "
         f"the encode and n·d·4 for each of the medoid's two passes, against {HBM_PEAK_TBS:g} TB/s (data sheet) and "
         f"≈{HBM_STREAM_TBS:g} TB/s (what a streaming copy kernel reaches on this part). A shape whose rows fit the "
         "256 MiB Infinity Cache (100000x128 is 51 MB) can read above the HBM rate on a repeated call: its figures say "
         "nothing about HBM.", "",
         "| shape | quantize_sq8 s (fastest – slowest) | statistics s (TB/s) | encode s (TB/s) | rest s | host codec + register + graph s "
         "(train / encode / register) | quantize / host: median (slowest) | torch encoder s (codec only) | quantize / torch: "
         "median (slowest) | equals host codec |", "|---|---|---|---|---|---|---|---|---|---|"]
    for o in lines:
        q, h, te = o["quantize_sq8"], o["host_codec_and_register"], o["torch_encoder"]
        t.append(f"| {o['shape']} | {q['s']} ({q['s_all'][0]} – {q['s_all'][-1]}) | {q['stats_s']} ({q['stats_tb_s']}) | {q['encode_s']} ({q['encode_tb_s']}) | "
                 f"{q['rest_s']} | {h['s']} ({h['train_s']} / {h['encode_s']} / {h['register_s']}) | "
                 f"{o['quantize_over_host']} ({o['slowest_quantize_over_host']}) | {te['s']} | "
                 f"{o['quantize_over_torch_encoder']} ({o['slowest_quantize_over_torch_encoder']}) | "
                 f"{q['equals_host_codec']} |")
    t += ["", "| shape | medoid s | TB/s over two passes | hipann.medoid (host) s | device / host | same row |",
          "|---|---|---|---|---|---|"]
    for o in lines:
        m, h = o["medoid"], o["host_medoid"]
        t.append(f"| {o['shape']} | {m['s']} | {m['tb_s_two_passes']} | {h['s']} | {o['medoid_over_host']} | "
                 f"{m['row'] == h['row']} |")
    t += ["", "The statistics and encode phases are the same work in every repetition; where the repetitions of "
          "`quantize_sq8` spread, the spread is in the rest phase (`s_all` and the phases of the median call are in "
          "`sq8_bench.jsonl`; `NOTES.md` has that phase's steps timed one by one)."]
    t += ["", f"The host codec ran on {lines[0]['host_threads']} threads (`oracle.sq8_encode`; `oracle.sq8_train` is one "
          "thread, as in the reference)."]
    for what, key in (("`quantize_sq8`, slowest repetition included,", "slowest_quantize_over_host"),
                      ("`medoid`", "medoid_over_host")):
        lost = [o["shape"] for o in lines if o[key] >= 1.0]
        t += ["", (f"{what} was faster than the host path it replaces at every shape above." if not lost else
                   f"{what} was NOT faster than the host path it replaces at: " + ", ".join(lost) + ".")]
    for what, key in (("at its median", "quantize_over_torch_encoder"),
                      ("in its slowest repetition", "slowest_quantize_over_torch_encoder")):
        lost = [o["shape"] for o in lines if o[key] >= 1.0]
        t += ["", (f"`quantize_sq8` (codec, finite check, handle and graph copy) {what} took less time than the torch "
                   "encoder's codec alone at every shape above." if not lost else
                   f"`quantize_sq8` (codec, finite check, handle and graph copy) {what} took MORE time than the torch "
                   "encoder's codec alone at: " + ", ".join(lost) + ".")]
    (out_dir / "README.md").write_text("\n".join(t) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="NxD, repeatable (default 100000x128 and 1000000x1536)")
    ap.add_argument("--R", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=15, help="timed repetitions of each device call (median reported)")
    ap.add_argument("--host-repeat", type=int, default=2, help="repetitions of each host side")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds each GPU step may take")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out-dir", default=None, help="write sq8_bench.jsonl and README.md here")
    a = ap.parse_args()
    lines = []
    for shape in a.shape or ["100000x128", "1000000x1536"]:
        out = run_shape(a, shape)
        lines.append(out)
        print(json.dumps(out), flush=True)
    if a.out_dir:
        write_report(Path(a.out_dir), a, lines)


def report_from_jsonl(path, out_dir):
    """Rewrite README.md from a kept sq8_bench.jsonl (no GPU needed)."""
    lines = [json.loads(ln) for ln in Path(path).read_text().splitlines() if ln.strip()]
    a = argparse.Namespace(R=lines[0]["R"], repeat=lines[0]["repeat"], host_repeat=lines[0]["host_repeat"])
    write_report(Path(out_dir), a, lines)


if __name__ == "__main__":
    main()
