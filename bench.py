#!/usr/bin/env python3
"""bench.py — MI355X search backend benchmark (driver contract: one JSON line on rank 0).

Metric (BASELINE.json): queries/s at recall@10 >= 0.95 on synthetic 10M x 768 fp32, batch = 1024
queries, at 1/2/4/8 GPUs.  A "step" = one search of the 1024-query batch against the whole
database (inputs already resident in HBM when the timed region starts; the PCIe-inclusive rate of
the host-pointer API is reported beside it as ``with_h2d_d2h``, never as ``value``).

Workloads (--workload):
  ivf   (default) FAISS IVFFlat nlist=1024 nprobe=32 over 10M x 768 (BASELINE configs[2], C3): the
        fastest configuration meeting recall@10 >= 0.95.  N GPUs: whole lists dealt to ranks by size
        (strong scaling), every rank scans the probed lists it owns, one packed all-gather of the
        per-rank top-k over RCCL + merge.
  flat  FAISS Flat L2 over 10M x 768 (exact: recall 1.0), rows sharded contiguously over the ranks.
  diskann  DiskProvider batch path, 1M x 1536 SQ8, L_search=128 (C4); replicas (weak scaling).

A plain run (no --full) does what the headline figure needs and nothing else: set up the index, warm up, time
--steps searches, write the last timed step's results when --dump-outputs DIR is given (DIR/distances.npy fp32,
DIR/labels.npy fp64: the (nq, k) arrays the caller of the timed search receives; the inputs are seeded, so two
builds run with the same arguments can be compared array for array), print the line.  Recall against exact
search, the kernel-timer roofline, the PCIe-inclusive rate, the other distance forms, the CPU baselines and
parity, and the sub-configurations below all take runs of their own and sit behind --full.

With --full, at N = 1 the default line also carries, from the same run, every other BASELINE configuration as a
sub-object of ``configs`` (each with its own roofline and CPU baseline): C1 (Flat 10k x 128, the CPU
path), C2 (Flat L2 1M x 768), Flat L2 10M x 768, C4 (DiskANN), the extension's real call shape
(nq = 1 / 4 latency, Flat and IVF), the reference's published batch-distance microbenchmark shapes
(README.md:140-147) with the MIN_GPU_WORK break-even, and the IVF recall/nprobe sweep at intrinsic
ranks 16/24/32.  --no-suite skips them.  At every N the IVF line also carries C5 (Flat IP, 12.5M rows
per GPU, sharded: exactly C5's 100M x 768 at N = 8); --no-c5 skips it.

Launch: python bench.py [--gpus N --steps K --warmup W] [--full] [--dump-outputs DIR].  N > 1 runs one process per GPU over RCCL: under
torch.distributed.run (the driver's launch) the ranks read RANK / WORLD_SIZE; started directly, bench.py
starts the N ranks itself (a torch.distributed.run child process — the parent never touches the GPU and never
re-execs) and exits with their status.  ``--workload selftest`` checks that launcher on the CPU (gloo): N
ranks rendezvous, all-gather their ranks and run the timed-region barrier / max-over-ranks protocol.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "duckdb-annsearch_amd"))
sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
FP32_MFMA_PEAK_TF = 157.3  # MI355X_MICROARCH.md: fp32 MFMA = fp32 vector peak
BF16_MFMA_PEAK_TF = 16 * FP32_MFMA_PEAK_TF  # dense bf16 MFMA = 16x the fp32 matrix rate (~2.5 PF)
I8_MFMA_PEAK_TOPS = 2 * BF16_MFMA_PEAK_TF  # dense int8 MFMA: the bf16 cycles at twice the K (MI355X_MICROARCH.md)
METRIC = "queries/sec @ recall@10>=0.95, 10Mx768 fp32, batch=1024"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# ------------------------------------------------------------------------------------------------
# the stdout line: headline fields + a compact per-config dict; everything else goes to a side file
# (the driver parses one bounded stdout line — r03's 23.4 KB line came back unparsed)
# ------------------------------------------------------------------------------------------------
DETAIL_PATH = Path(os.environ.get("HIPANN_BENCH_DETAIL", str(ROOT / "gpurun_out" / "bench_detail.json")))
LINE_BUDGET = 6000  # bytes of the printed line; tests/test_benchline.py holds the line under it
ROOF_KEYS = ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms", "merge_ms",
             "frac_vs_survey_bytes", "algorithmic_per_launch_gb")


def _rnd(v, nd=4):
    if isinstance(v, float):
        return round(v, nd) if abs(v) < 1e4 else round(v, 1)
    return v


def compact_roofline(r):
    out = {k: _rnd(r[k]) for k in ROOF_KEYS if k in r}
    if "kernel_ms" not in out and "kernel_ms_per_batch" in r:
        out["kernel_ms"] = _rnd(r["kernel_ms_per_batch"])
    return out


def compact_cpu(c, sample_chars=110):
    if not isinstance(c, dict):
        return c
    out = {k: _rnd(c[k]) for k in ("value", "unit", "cores", "kind") if k in c}
    if c.get("sample"):
        out["sample"] = c["sample"][:sample_chars]
    if c.get("error"):
        out["error"] = str(c["error"])[:120]
    return out


def compact_config(name, c):
    """value / ms_per_step / recall / roofline.frac / roofline.kernel_ms / cpu_baseline.value of one sub-config,
    plus the one or two numbers that sub-config exists for."""
    if not isinstance(c, dict):
        return c
    out = {}
    for k in ("value", "ms_per_step", "recall_at_10", "k", "request_k"):
        if c.get(k) is not None:
            out[k] = _rnd(c[k])
    roof = c.get("roofline")
    if isinstance(roof, dict):
        out["frac"] = _rnd(roof.get("frac"))
        out["kernel"] = roof.get("kernel")
        km = roof.get("kernel_ms", roof.get("kernel_ms_per_batch"))
        if km is not None:
            out["kernel_ms"] = _rnd(km)
        if roof.get("traffic") is not None:
            out["traffic_gb"] = _rnd(roof["traffic"])
    cpu = c.get("cpu_baseline")
    if isinstance(cpu, dict):
        out["cpu_qps"] = _rnd(cpu.get("value"))
    if c.get("rerank_fallbacks_total"):
        out["rerank_fallbacks"] = c["rerank_fallbacks_total"]
    if isinstance(c.get("ids_equal_to_oracle"), dict) and "fraction" in c["ids_equal_to_oracle"]:
        out["ids_eq_oracle"] = c["ids_equal_to_oracle"]["fraction"]
    par = c.get("parity_vs_cpu_path")
    if isinstance(par, dict):
        out["ids_eq_cpu_path"] = par.get("ids_eq_cpu_path")
        out["parity_ok"] = par.get("parity_ok")
        out["parity_queries"] = par.get("queries")
    if c.get("ids_equal_to_oracle_bfs") is not None:
        out["ids_eq_oracle_bfs"] = c["ids_equal_to_oracle_bfs"]
    for kk in ("nprobe", "sigma", "list_size_max_over_mean", "flagged_per_batch"):  # C3 on SURVEY's mixture
        if c.get(kk) is not None and "sweep" in c:
            out[kk] = c[kk]
    if c.get("vs_k10") is not None:
        out["vs_k10"] = c["vs_k10"]
    if isinstance(c.get("form_qps"), dict):  # the other forms: [QPS, fraction of ids equal to the reported form's]
        out["form_qps"] = c["form_qps"]
    if c.get("form") is not None and isinstance(c.get("roofline"), dict):
        out["form"] = c["form"]
    if isinstance(c.get("path"), dict):
        p = c["path"]
        out["path"] = f"form{p.get('form')} kf{p.get('filter_k')}" + (f" sub{p['sublists']}" if p.get("sublists") else "")
    if isinstance(c.get("latency"), dict):
        out["nq1_ms"] = _rnd((c["latency"].get("nq1") or {}).get("ms_per_call"))
    if "gpu_ids_equal_to_cpu_path" in c:  # C1
        out["gpu_ids_equal_to_cpu_path"] = c["gpu_ids_equal_to_cpu_path"]
        out["cpu_qps"] = (c.get("cpu_path") or {}).get("batch1000_queries_per_s")
        out["gpu_qps_host_ptrs"] = (c.get("gpu_path_host_pointers") or {}).get("batch1000_queries_per_s")
    if "break_even_n_times_d" in c:  # README batch-distance shapes
        out["break_even_n_times_d"] = c["break_even_n_times_d"]
        out["break_even_n_times_d_simd_cpu"] = c.get("break_even_n_times_d_simd_cpu")
        out["speedup_at_readme_shapes"] = [s.get("speedup") for s in c.get("shapes", [])]
    if "d128" in c and "d768" in c:  # flat AUTO gate
        out["break_even_ntotal"] = {k: c[k].get("break_even_ntotal") for k in ("d128", "d768")}
    for k, v in c.items():  # ivf recall-vs-nprobe sweep: [nprobe, QPS, recall] at the smallest nprobe >= 0.95
        if k.startswith("intrinsic_dim_") and isinstance(v, dict):
            b = v.get("smallest_nprobe_at_recall_0.95") or {}
            out[k] = [b.get("nprobe"), b.get("queries_per_s"), b.get("recall_at_10")]
    if c.get("error"):
        out["error"] = str(c["error"])[:160]
    return {k: v for k, v in out.items() if v is not None}


def compact_line(full):
    """The driver's stdout line from the full record: the contract's headline fields, roofline{bound, achieved,
    peak, frac, traffic, kernel_ms, frac_vs_survey_bytes}, cpu_baseline{value, unit, cores, kind}, recall and a
    compact `configs`; the rest stays in the detail file named by `detail`."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "recall_at_10")
    line = {k: _rnd(full[k]) for k in keep if k in full}
    if isinstance(full.get("roofline"), dict):
        line["roofline"] = compact_roofline(full["roofline"])
    if "cpu_baseline" in full:
        line["cpu_baseline"] = compact_cpu(full["cpu_baseline"])
    par = full.get("parity_vs_cpu_path")
    if isinstance(par, dict):
        line["ids_eq_cpu_path"] = par.get("ids_eq_cpu_path")
        line["parity_ok"] = par.get("parity_ok")
        line["parity_queries"] = par.get("queries")
    if isinstance(full.get("with_h2d_d2h"), dict):
        line["with_h2d_d2h_qps"] = full["with_h2d_d2h"].get("queries_per_s")
    if isinstance(full.get("latency"), dict):
        line["nq1_ms"] = (full["latency"].get("nq1") or {}).get("ms_per_call")
    if isinstance(full.get("append"), dict):
        a = full["append"]
        line["append2048"] = {k: a.get(k) for k in ("append_ms", "append_plus_search_ms", "vs_search_step",
                                                     "vs_search_from_idle")}
    fb = (full.get("ivf") or {}).get("rerank_fallbacks_total", full.get("rerank_fallbacks_total"))
    if fb is not None:
        line["rerank_fallbacks"] = fb
    if isinstance(full.get("configs"), dict):
        line["configs"] = {name: compact_config(name, c) for name, c in full["configs"].items()}
    for k in ("world_check", "build"):
        if k in full:
            line[k] = full[k]
    line["detail"] = str(DETAIL_PATH.relative_to(ROOT)) if DETAIL_PATH.is_relative_to(ROOT) else str(DETAIL_PATH)
    s = json.dumps(line)
    if len(s) > LINE_BUDGET:  # never lose the headline: drop the per-config extras first
        for name, c in line.get("configs", {}).items():
            line["configs"][name] = {k: c[k] for k in ("value", "ms_per_step", "recall_at_10", "frac", "kernel_ms",
                                                       "cpu_qps", "ids_eq_cpu_path", "parity_ok", "error") if k in c}
        line.get("cpu_baseline", {}).pop("sample", None)
    return line


def emit(full, rank, detail=True):
    """Rank 0: the full record to DETAIL_PATH, the compact line to stdout.  detail=False (a plain run: the record
    holds nothing the line does not) prints the line alone."""
    if rank != 0:
        return
    if not detail:
        line = compact_line(full)
        line.pop("detail", None)
        print(json.dumps(line), flush=True)
        return
    try:
        DETAIL_PATH.parent.mkdir(parents=True, exist_ok=True)
        DETAIL_PATH.write_text(json.dumps(full, indent=1))
    except OSError as e:
        log(f"[bench] could not write {DETAIL_PATH}: {e!r}")
    print(json.dumps(compact_line(full)), flush=True)


def build_provenance():
    """Which libhipann.so this process loaded (sha256 prefix, mtime) and what __graft_entry__.build() recorded
    about producing it (make outcome), so a line can be tied to the binary it measured."""
    import hashlib

    import hipann

    out = {}
    try:
        data = hipann.LIB_PATH.read_bytes()
        out["so_sha16"] = hashlib.sha256(data).hexdigest()[:16]
        out["so_mtime"] = time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime(hipann.LIB_PATH.stat().st_mtime))
    except OSError as e:
        out["error"] = repr(e)
    info = hipann.HERE / "build_info.json"
    if info.exists():
        try:
            bi = json.loads(info.read_text())
            out["make"] = bi.get("make")
            out["built_at"] = bi.get("built_at")
            out["recorded_sha16"] = bi.get("so_sha16")
            out["so_is_recorded_build"] = out.get("so_sha16") == bi.get("so_sha16")
            import __graft_entry__ as ge
            out["built_from_these_sources"] = bi.get("src_sha16") == ge.sources_sha16()
        except (ValueError, OSError):
            pass
    return out


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--workload", choices=["flat", "ivf", "diskann", "selftest"],
                   default=os.environ.get("HIPANN_BENCH_WORKLOAD", "ivf"))
    p.add_argument("--n", type=int, default=None, help="rows (10M; 1M for diskann)")
    p.add_argument("--d", type=int, default=None, help="dimension (768; 1536 for diskann)")
    p.add_argument("--l-search", type=int, default=128, help="diskann L_search")
    p.add_argument("--degree", type=int, default=64, help="diskann graph degree R")
    p.add_argument("--diskann-host-bfs", action="store_true",
                   help="diskann: the reference-shaped host BFS (one id-gather launch per step) instead of the "
                        "GPU-resident traversal")
    p.add_argument("--nq", type=int, default=1024)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--nlist", type=int, default=1024)
    p.add_argument("--nprobe", type=int, default=32)
    p.add_argument("--metric", choices=["l2", "ip"], default="l2")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-alt-forms", action="store_true", help="ivf/flat: skip timing the other distance forms")
    p.add_argument("--suite", dest="suite", action="store_true", default=None,
                   help="N=1: add the other BASELINE configurations as sub-objects (default for --workload ivf)")
    p.add_argument("--no-suite", dest="suite", action="store_false")
    p.add_argument("--no-c5", action="store_true", help="skip the C5 sub-line (Flat IP, 12.5M rows per GPU)")
    p.add_argument("--only", default=None, help="with the suite: run only these comma-separated configurations "
                   "(profiling runs; e.g. C3_ivf_survey_mixture)")
    p.add_argument("--cpu-seconds", type=float, default=10.0, help="target CPU sample duration (main line)")
    p.add_argument("--full", action="store_true",
                   help="beside the timed steps: recall, kernel-timer roofline, PCIe-inclusive rate, the other forms, "
                        "CPU baselines + parity, the suite and C5 (the --suite / --no-* options choose among these)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the last timed step's results to DIR/distances.npy (fp32) and "
                        "DIR/labels.npy (fp64)")
    a = p.parse_args()
    if not a.full:  # a plain run: set up, warm up, time the steps, print the line
        a.suite, a.no_c5, a.no_cpu_baseline, a.no_alt_forms = False, True, True, True
    if a.n is None:
        a.n = 1_000_000 if a.workload == "diskann" else 10_000_000
    if a.d is None:
        a.d = 1536 if a.workload == "diskann" else 768
    if a.suite is None:
        a.suite = a.workload == "ivf"
    return a


# ------------------------------------------------------------------------------------------------
# synthetic data (generated on the device, chunk-seeded so every sharding sees the same matrix)
# ------------------------------------------------------------------------------------------------
CHUNK = 125_000  # generation granularity (divides 10M / {1,2,4,8})


def _chunks(n, row0):
    r = 0
    while r < n:
        g_row = row0 + r
        chunk = g_row // CHUNK
        off = g_row - chunk * CHUNK
        take = min(CHUNK - off, n - r)
        yield r, chunk, off, take
        r += take


def gen_uniform_rows(torch, out, row0, seed):
    """Fill `out` (rows [row0, row0+len)) with U(-1,1) fp32."""
    for r, chunk, off, take in _chunks(out.shape[0], row0):
        gen = torch.Generator(device=out.device)
        gen.manual_seed(seed * 1_000_003 + chunk)
        blk = torch.rand((CHUNK, out.shape[1]), generator=gen, device=out.device, dtype=torch.float32)
        out[r:r + take].copy_(blk[off:off + take]).mul_(2.0).sub_(1.0)
    return out


def gen_clustered_rows(torch, out, row0, centres, sigma, seed):
    """Rows = centre[assign] + N(0, sigma^2)."""
    nc = centres.shape[0]
    for r, chunk, off, take in _chunks(out.shape[0], row0):
        gen = torch.Generator(device=out.device)
        gen.manual_seed(seed * 1_000_003 + chunk)
        a = torch.randint(0, nc, (CHUNK,), generator=gen, device=out.device)
        noise = torch.randn((CHUNK, out.shape[1]), generator=gen, device=out.device, dtype=torch.float32)
        blk = centres[a].add_(noise.mul_(sigma))
        out[r:r + take].copy_(blk[off:off + take])
    return out


def lowrank_basis(torch, r_dim, d, gen):
    """Random r×d matrix with orthonormal rows (QR of a gaussian), scaled so rows of z·B have O(1) entries."""
    g = torch.randn((d, r_dim), generator=gen, device=gen.device)
    q, _ = torch.linalg.qr(g)
    return (q.T.contiguous() * (d / r_dim) ** 0.5 / 3.0).contiguous()


def gen_lowrank_rows(torch, out, row0, basis, eta, seed):
    """Rows = z·B + eta·N(0, I_d), z ~ N(0, I_r): a low-intrinsic-dimension gaussian."""
    r_dim, d = basis.shape
    for r, chunk, off, take in _chunks(out.shape[0], row0):
        gen = torch.Generator(device=out.device)
        gen.manual_seed(seed * 1_000_003 + chunk)
        z = torch.randn((CHUNK, r_dim), generator=gen, device=out.device, dtype=torch.float32)
        noise = torch.randn((CHUNK, d), generator=gen, device=out.device, dtype=torch.float32)
        blk = torch.addmm(noise.mul_(eta), z, basis)
        out[r:r + take].copy_(blk[off:off + take])
    return out


def uniform_queries(torch, nq, d, dev):
    gq = torch.Generator(device=dev)
    gq.manual_seed(4242)
    return (torch.rand((nq, d), generator=gq, device=dev, dtype=torch.float32) * 2 - 1).contiguous()


# ------------------------------------------------------------------------------------------------
# timing helpers
# ------------------------------------------------------------------------------------------------
def timed_steps(torch, dist, world, fn, steps, gpu=True):
    """Barrier + sync, `steps` calls, sync + barrier; max over ranks.  Returns (seconds, what the last call
    returned).  gpu=False: the CPU self-test (gloo, no device synchronisation)."""
    sync = torch.cuda.synchronize if gpu else (lambda: None)
    last = None
    if world > 1:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        last = fn()
    sync()
    if world > 1:
        dist.barrier()
    el = time.perf_counter() - t0
    if world > 1:
        dev = torch.device("cuda", torch.cuda.current_device()) if gpu else torch.device("cpu")
        t = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    return el, last


def dump_outputs(args, rank, D, I):
    """--dump-outputs DIR: the (nq, k) distances and labels the last timed step returned (device tensors or host
    arrays), as DIR/distances.npy (fp32) and DIR/labels.npy (fp64: exact for every label below 2^53)."""
    if not args.dump_outputs or rank != 0:
        return
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)  # noqa: E731
    out = Path(args.dump_outputs)
    out.mkdir(parents=True, exist_ok=True)
    np.save(out / "distances.npy", host(D).astype(np.float32))
    np.save(out / "labels.npy", host(I).astype(np.float64))


def host_pointer_rate(torch, search_dev, xq, nq, k, steps):
    """The same search with the queries starting in host memory and the results returned to host memory
    (pinned buffers, H2D + search + D2H per step): the PCIe-inclusive rate of the host-pointer API."""
    q_h = xq.cpu().pin_memory()
    q_d = torch.empty_like(xq)
    D_h = torch.empty((nq, k), dtype=torch.float32).pin_memory()
    I_h = torch.empty((nq, k), dtype=torch.int64).pin_memory()

    def step():
        q_d.copy_(q_h, non_blocking=True)
        D, I = search_dev(q_d)
        D_h.copy_(D, non_blocking=True)
        I_h.copy_(I, non_blocking=True)

    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return {"queries_per_s": round(nq * steps / el, 1), "ms_per_step": round(el * 1e3 / steps, 3),
            "includes": "pinned H2D of the queries + search + D2H of D/I per step"}


PARITY_RULE = ("tests/_data.check_topk_parity (oracle/parity.py): ids and order identical except at fp64 near-ties "
               "within tau*scale (tau 1e-6), label sets equal below the CPU k-th key - window, distances within 1e-5 "
               "(relative) + 8e-6*scale of fp64")


def max_sqnorm_dev(x, chunk=1 << 20):
    """max_i ‖x_i‖² of a device tensor, in row chunks (no full-size temporary)."""
    m = 0.0
    for r0 in range(0, x.shape[0], chunk):
        c = x[r0:r0 + chunk]
        m = max(m, float((c * c).sum(1).max().item()))
    return m


def recall_at(got, gt, k):
    return float(np.mean([len(set(got[i][:k]) & set(gt[i][:k])) / k for i in range(len(gt))]))


def request_k_line(torch, index, xq, k_user, n_deleted, base_ms, steps=5):
    """The extension's request_k = min(k + |tombstones|, ntotal) (src/faiss_index.cpp:713-715) on the same index and
    batch: k = 10 with 20 deleted rows asks the GPU for 30.  Times `steps` device searches at request_k and reports
    the step against the k = 10 step (within 1.3x), and the path that ran (hipann_last_search_path)."""
    rk = k_user + n_deleted
    nq = xq.shape[0]
    stream = torch.cuda.current_stream().cuda_stream
    D = torch.empty((nq, rk), device=xq.device, dtype=torch.float32)
    I = torch.empty((nq, rk), device=xq.device, dtype=torch.int64)
    call = lambda: index.search_device(nq, xq.data_ptr(), rk, D.data_ptr(), I.data_ptr(), stream)  # noqa: E731
    call()
    torch.cuda.synchronize()
    index.set_kernel_timing(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    kms = index.kernel_ms(0)
    index.set_kernel_timing(False)
    ms = el * 1e3 / steps
    return {"workload": f"request_k = {k_user} + {n_deleted} tombstones = {rk} (faiss_index.cpp:713-715)", "k": k_user,
            "request_k": rk, "value": round(nq / (ms * 1e-3), 1), "ms_per_step": round(ms, 3),
            "roofline": {"kernel_ms": round(kms, 3)}, "vs_k10": round(ms / base_ms, 3) if base_ms > 0 else None,
            "path": index.last_search_path()}


def pmc_traffic(key: str, kernel: str):
    """HBM bytes per launch of `kernel` for workload `key` (e.g. "ivf_10000000x768") from the newest
    committed FETCH_SIZE pass (profiles/rNN/pmc_<key>.json, written by tools/pmc_traffic.py from a
    separate `rocprofv3 --pmc FETCH_SIZE` run of the same workload), or (None, None)."""
    for f in sorted((ROOT / "profiles").glob(f"r*/pmc_{key}.json"), reverse=True):
        try:
            js = json.loads(f.read_text())
        except Exception:
            continue
        if js.get("kernel") == kernel:
            return js.get("hbm_bytes_per_launch"), str(f.relative_to(ROOT))
    return None, None


def attach_traffic(roof, key, algorithmic_bytes):
    tb, tsrc = pmc_traffic(key, roof["kernel"])
    roof["traffic_key"] = key
    if tb is not None:
        roof["traffic"] = round(tb / 1e9, 3)
        roof["traffic_unit"] = "GB per launch (PMC FETCH_SIZE x1024 x2, gfx950 correction)"
        roof["traffic_source"] = tsrc
    roof["algorithmic_per_launch_gb"] = round(algorithmic_bytes / 1e9, 3)
    if tb is not None and algorithmic_bytes > 0:
        roof["traffic_over_algorithmic"] = round(tb / algorithmic_bytes, 3)


# ------------------------------------------------------------------------------------------------
# Flat
# ------------------------------------------------------------------------------------------------
FLAT_DEFAULT_FORM = 5
FLAT_FORMS = {5: ("flat_bf16_k64<I8>", 1, I8_MFMA_PEAK_TOPS,
                  "int8 MFMA (v_mfma_i32_16x16x64_i8, exact int32 sums), one int8 product per fp32 product over a "
                  "tiled int8 image with per-row scales; the bounded passes and exact fp32 rerank of form 4 with a "
                  "64-deep filter (the bound from the measured int8 residuals)"),
              4: ("flat_bf16_k64", 1, BF16_MFMA_PEAK_TF,
                  "bf16 MFMA (v_mfma_f32_16x16x32_bf16), one bf16 product per fp32 product over a tiled bf16 image of "
                  "the rows; kernel_ms = the keys-mode seed pass + the planned bounded passes (rows with scan key <= a per-query "
                  "bound to candidate buffers) + the bound / select kernels; merge_ms = exact fp32 direct-form rerank "
                  "of the 32 best + bound check (Cauchy-Schwarz bound of the bf16 residuals)"),
              0: ("flat_gemm_topk2", 1, FP32_MFMA_PEAK_TF, "fp32 MFMA (v_mfma_f32_32x32x2_f32)"),
              1: ("flat_gemm_topk_bf", 6, BF16_MFMA_PEAK_TF,
                  "bf16 MFMA (v_mfma_f32_32x32x16_bf16) over a 3-term split: 6 bf16 products per fp32 product"),
              2: ("flat_gemm_topk_bf", 3, BF16_MFMA_PEAK_TF,
                  "bf16 MFMA (v_mfma_f32_32x32x16_bf16) over a 2-term split: 3 bf16 products per fp32 product"),
              3: ("flat_gemm_topk_bf", 3, BF16_MFMA_PEAK_TF,
                  "bf16 MFMA (v_mfma_f32_32x32x16_bf16) over a 2-term split: 3 bf16 products per fp32 product; "
                  "the scan keeps 16 (IP: 32) per (split, query) as a filter, merge_ms = exact direct-form rerank "
                  "+ bound check")}


def flat_config(args, torch, dist, hipann, rank, world, dev, n, d, nq, k, metric, steps, warmup, alt_forms=True,
                cpu_seconds=0.0, oracle_queries=0, latency=False, host_rate=True, request_k=False, full=True,
                dump=False):
    """full=False (the headline of a plain run): only the set-up, the warm-up and the timed steps.  dump: this is the
    run's headline configuration, whose last timed step --dump-outputs writes."""
    from sharded import ShardedSearch, merge_packed_device_torch, shard_bounds

    lo, hi = shard_bounds(n, rank, world)
    n_local = hi - lo
    stream = torch.cuda.current_stream().cuda_stream
    t_setup = time.perf_counter()
    xb = torch.empty((n_local, d), device=dev, dtype=torch.float32)
    gen_uniform_rows(torch, xb, lo, 42)
    xq = uniform_queries(torch, nq, d, dev)
    index = hipann.HipIndexFlatDevice(d, metric, xb.data_ptr(), n_local, dev.index, copy=False, label_offset=lo)
    if os.environ.get("HIPANN_FLAT_FORM"):  # A/B; the library default is form 5 (int8 filter + exact rerank)
        index.form = int(os.environ["HIPANN_FLAT_FORM"])
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t_setup

    def local(q, D, I):
        index.search_device(q.shape[0], q.data_ptr(), k, D.data_ptr(), I.data_ptr(), stream)

    sharded = ShardedSearch(local, merge_packed_device_torch(hipann, metric), nq, k, dev)
    step = lambda: sharded.search(xq)  # noqa: E731
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    el, (Dl, Il) = timed_steps(torch, dist, world, step, steps)
    if dump:
        dump_outputs(args, rank, Dl, Il)
    del Dl, Il
    if not full:
        return {"workload": f"FAISS Flat {'L2' if metric == 0 else 'IP'}, {n}x{d} fp32, batch={nq}, k={k}",
                "value": round(nq * steps / el, 1), "unit": "queries/s", "ms_per_step": round(el * 1e3 / steps, 3),
                "steps": steps, "setup_s": round(setup_s, 1), "form": index.last_search_path()["form"]}, index, xb
    kern_ms, merge_ms = kernel_timing_steps(torch, index, step, steps)
    Dr, Ir = step()
    torch.cuda.synchronize()
    Ir = Ir.cpu().numpy().copy()
    Dr = Dr.cpu().numpy().copy()  # (the alternative forms below reuse the output buffers)
    form = index.last_search_path()["form"]  # the form the scan ran (the default falls back to 4 on small shapes)
    kname, terms, peak, fdesc = FLAT_FORMS[form]
    flops = 2.0 * nq * n_local * d
    achieved = terms * flops / (kern_ms * 1e-3) / 1e12 if kern_ms > 0 else 0.0
    roof = {"bound": "mfma", "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4), "traffic": None, "kernel": kname, "kernel_ms": round(kern_ms, 3),
            "merge_ms": round(merge_ms, 3),
            "algorithmic": f"{terms} x 2*nq*N_local*d = {terms * flops:.4g} MFMA FLOP per launch ({fdesc})",
            "fp32_equivalent_tflops": round(flops / (kern_ms * 1e-3) / 1e12, 2) if kern_ms > 0 else None}
    if kern_ms > 0:
        # SURVEY §8d prices Flat against the fp32 matrix-core peak (2·nq·N·d fp32 products); the default form
        # computes each product once in bf16 as a certified filter (exact fp32 rerank), so it can pass that peak
        roof["frac_vs_fp32_peak"] = round(flops / (kern_ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TF, 4)
        roof["fp32_peak"] = FP32_MFMA_PEAK_TF
    if form == 5 and kern_ms > 0:
        roof["unit"] = "TOPS"
        roof["frac_vs_bf16_peak"] = round(flops / (kern_ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TF, 4)
    if form in (4, 5) and kern_ms > 0:
        # operand delivery of the bf16 scan (256 x 256 tiles): per 64-dim K-step the database tile (32 KB, LDS-DMA)
        # and the 256 queries' fragments (32 KB, straight into registers) through the vector-memory return path —
        # the unit the PMC pass finds busiest (profiles/r03/pmc_flat_k64.json)
        qm = 256 if nq >= 256 else 128 if nq >= 128 else 64
        dpc = 64 if form == 5 else 32  # dims per 64-B chunk row of the image
        fill = -(-nq // qm) * -(-n_local // 256) * -(-d // dpc) * (qm + 256) * 64.0
        roof["operand_delivery"] = {"bytes_per_launch_gb": round(fill / 1e9, 2),
                                    "achieved_tbps": round(fill / (kern_ms * 1e-3) / 1e12, 2),
                                    "flop_per_byte": round(2.0 * nq * n_local * d / fill, 1),
                                    "note": "L2 -> CU bytes of A + B per launch; TD busy 0.78 at 10M x 768 (PMC)"}
    if world == 1:
        # the bytes the scan must stream once per search: form 5 the tiled int8 image (64 B per 64-dim chunk, chunk
        # count rounded up to even) + ‖x‖² (L2) + the row scale, plus the keys-mode seed pass over its first 16K rows;
        # form 4 the bf16 image the same way; the fp32 forms the fp32 rows
        if form in (4, 5):
            nk = -(-d // 64) if form == 5 else -(-d // 32)
            nk += nk % 2
            rowb = 64.0 * nk + (4.0 if metric == 0 else 0.0) + (4.0 if form == 5 else 0.0)
            alg_b = rowb * (n_local + min(n_local, 16384))
        else:
            alg_b = 4.0 * n_local * d
        attach_traffic(roof, f"flat_{n}x{d}{'' if metric == 0 else '_ip'}", alg_b)
    out = {"workload": f"FAISS Flat {'L2' if metric == 0 else 'IP'}, {n}x{d} fp32, batch={nq}, k={k}",
           "value": round(nq * steps / el, 1), "unit": "queries/s", "ms_per_step": round(el * 1e3 / steps, 3),
           "steps": steps, "recall_at_10": None, "roofline": roof, "setup_s": round(setup_s, 1),
           "rerank_fallbacks_total": index.rerank_fallbacks(), "form": form}
    if form in (3, 4, 5):
        out["precision"] = ("returned distances are fp32 " + ("direct-form Σ(q−x)²" if metric == 0 else "dot products")
                            + ", recomputed exactly for the kept candidates; FAISS CPU's BLAS path (nq >= 20) returns "
                            "max(0, ‖q‖²+‖x‖²−2q·x) from sgemm: the same ids (parity tests), distances equal up to the "
                            "fp32 rounding of the two forms. The bf16 / int8 scan is a certified filter, not the result.")
    if world > 1:
        return out, index, xb
    if request_k:
        out["request_k30"] = request_k_line(torch, index, xq, k, 20, el * 1e3 / steps)
    if host_rate:
        out["with_h2d_d2h"] = host_pointer_rate(torch, lambda q: sharded.search(q), xq, nq, k, max(3, steps // 2))
    # exactness: ids against the fp32 form (exact fp32 products, pinned by the C2 parity tests) on the whole
    # batch, and against the CPU oracle (FAISS BLAS-path restatement) on a query subset
    if alt_forms:
        alt = {}
        for f in (0, 1, 3, 4, 5):
            if f == form or (f == 3 and n_local > 2_000_000):  # the 2-term split at 10M+: ~60 ms a step, skip
                continue
            index.form = f
            step()
            torch.cuda.synchronize()
            if index.last_search_path()["form"] != f:  # this shape runs another form under that setting
                continue
            index.set_kernel_timing(True)
            ta = time.perf_counter()
            for _ in range(2):
                step()
            torch.cuda.synchronize()
            ea = time.perf_counter() - ta
            kms = index.kernel_ms(0)
            index.set_kernel_timing(False)
            _, Ia = step()
            torch.cuda.synchronize()
            Ia = Ia.cpu().numpy()
            alt[FLAT_FORMS[f][3]] = {"queries_per_s": round(nq * 2 / ea, 1), "kernel_ms": round(kms, 3),
                                     "ids_equal_to_reported_form": round(float((Ia == Ir).mean()), 6)}
            out.setdefault("form_qps", {})[f"form{f}"] = [round(nq * 2 / ea, 1), round(float((Ia == Ir).mean()), 5)]
            if f == 0:  # exact fp32 products: the reference for recall
                out["recall_at_10"] = round(recall_at(Ir, Ia, k), 6)
                out["recall_reference"] = "the fp32-MFMA form's top-k on the same batch (exact fp32 products)"
        index.form = FLAT_DEFAULT_FORM if not os.environ.get("HIPANN_FLAT_FORM") else int(os.environ["HIPANN_FLAT_FORM"])
        out["other_forms"] = alt
    if oracle_queries:
        # the extension's CPU path (FAISS IndexFlat::search, BLAS form at nq >= 20: oracle.c) on the first
        # oracle_queries of the batch, against the GPU's answers under the parity rule (oracle/parity.py)
        try:
            from oracle import oracle as O
            from oracle.parity import topk_parity
            xb_h = xb.cpu().numpy()
            xq_h = xq[:oracle_queries].cpu().numpy()
            t_o = time.perf_counter()
            Do, Io = O.flat_search(xb_h, xq_h, k, metric, label_offset=0)
            dt_o = time.perf_counter() - t_o
            Dg = Dr[:oracle_queries]
            par = topk_parity(lambda labs: xb_h[labs], xq_h, Dg, Ir[:oracle_queries], Do, Io, metric,
                              max_sqnorm_dev(xb))
            par["rule"] = PARITY_RULE
            par["cpu_path_s"] = round(dt_o, 1)
            out["ids_equal_to_oracle"] = {"fraction": float((Io == Ir[:oracle_queries]).mean()),
                                          "queries": oracle_queries,
                                          "oracle": "FAISS IndexFlat BLAS-path restatement (oracle.c)"}
            out["parity_vs_cpu_path"] = par
            del xb_h
        except Exception as e:  # report, never fail the line
            out["ids_equal_to_oracle"] = {"error": repr(e)}
    if latency:
        out["latency"] = flat_latency(torch, hipann, index, xb, xq, n_local, d, k, metric)
    if cpu_seconds > 0:
        out["cpu_baseline"] = flat_cpu_baseline(torch, xq, n, d, k, metric, cpu_seconds)
    return out, index, xb


def flat_latency(torch, hipann, index, xb, xq, n, d, k, metric):
    """The extension's call shape: FaissIndex::Search → search(1, …) (faiss_index.cpp:737), and a
    4-query batch; the direct-form scan (flat_scan_topk, nq < 20) streams the whole table per call."""
    stream = torch.cuda.current_stream().cuda_stream
    res = {}
    for nq in (1, 4):
        q = xq[:nq].contiguous()
        D = torch.empty((nq, k), device=xq.device)
        I = torch.empty((nq, k), device=xq.device, dtype=torch.int64)
        call = lambda: index.search_device(nq, q.data_ptr(), k, D.data_ptr(), I.data_ptr(), stream)  # noqa: E731
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        index.set_kernel_timing(True)
        it = 20
        t0 = time.perf_counter()
        for _ in range(it):
            call()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        kms = index.kernel_ms(0)
        index.set_kernel_timing(False)
        path = index.last_search_path()
        if path["form"] == 5:  # flat_i8_scan: the int8 image (64 dims per 64-B unit row, even chunk count) + scale, ‖x‖²
            nk = -(-d // 64)
            nk += nk & 1
            bytes_ = float(n) * (nk * 64 + 8)
            kname, alg = "flat_i8_scan", f"N*(int8 row + scale + norm) = {bytes_ / 1e9:.3f} GB per call (int8 filter)"
        else:
            bytes_ = 4.0 * n * d
            kname, alg = "flat_scan_topk", f"N*d*4 = {bytes_ / 1e9:.3f} GB per call"
        gbs = bytes_ / (kms * 1e-3) / 1e9 if kms > 0 else 0.0
        res[f"nq{nq}"] = {"ms_per_call": round(el * 1e3 / it, 4), "kernel": kname,
                          "kernel_ms": round(kms, 4), "path": path,
                          "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                       "frac": round(gbs / HBM_PEAK_GBS, 4), "algorithmic": alg}}
    return res


def flat_cpu_baseline(torch, xq, n, d, k, metric, cpu_seconds):
    from oracle import cpu_baseline as CB

    try:
        xq_h = xq.cpu().numpy()
        gen_rows = lambda rows: gen_uniform_rows(torch, torch.empty((rows, d), device=xq.device), 0,  # noqa: E731
                                                 42).cpu().numpy()
        probe = gen_rows(20_000)
        _, dt0, _ = CB.flat_blas_qps(probe, xq_h, k, n, metric)
        rows = int(min(n, 2_000_000, max(20_000, 20_000 * cpu_seconds / max(dt0, 1e-3))))
        qps, dt, nth = CB.flat_blas_qps(gen_rows(rows), xq_h, k, n, metric)
        return {"value": round(qps, 2), "unit": "queries/s", "cores": nth, "kind": "port",
                "sample": f"all {xq_h.shape[0]} queries x first {rows} of {n} rows ({dt:.1f} s), FAISS BLAS-path "
                          f"restatement (torch CPU sgemm 4096x1024 blocks + norms + top-k), extrapolated linearly to "
                          f"{n} rows"}
    except Exception as e:
        return {"value": None, "error": repr(e)}


# ------------------------------------------------------------------------------------------------
# IVFFlat
# ------------------------------------------------------------------------------------------------
IVF_FORMS = {0: ("ivf_scan_mfma", "decomposed, fp32 MFMA"), 1: ("ivf_scan_topk", "direct, VALU"),
             2: ("ivf_scan_dot", "decomposed, VALU"),
             3: ("ivf_scan_mfma_bf", "decomposed, bf16 MFMA over a 3-term split (6 products)"),
             4: ("ivf_scan_mfma_bf", "decomposed, bf16 MFMA over a 2-term split (3 products)"),
             5: ("ivf_scan_mfma_bf", "bf16 MFMA 2-term split scan as a filter (16 per list) + exact fp32 "
                                     "direct-form rerank, bound-checked (merge_ms includes the rerank)"),
             6: ("ivf_scan_mfma_h", "fp16 MFMA scan over a tiled fp16 image of the rows (2 B per element, "
                                    "2-term fp16 queries) as a filter (16 per list) + exact fp32 direct-form "
                                    "rerank, bound-checked with the measured fp16 residuals (merge_ms includes "
                                    "the rerank)"),
             7: ("ivf_scan_mfma_h", "int8 MFMA scan over a tiled int8 image of the rows (1 B per element + a "
                                    "per-row scale, int8 queries, exact int32 sums) as a filter (per-wave sub-lists, "
                                    "64 reranked) + exact fp32 direct-form rerank, bound-checked with the measured "
                                    "int8 residuals (merge_ms includes the rerank)")}


def ivf_row_bytes(form, d, metric):
    """HBM bytes one scanned row costs the form's list-scan kernel: the fp16 image (2d) + the row norm
    (L2) for form 6; the int8 image (d) + row scale + norm (L2) for form 7; SURVEY §8d's fp32 codes + label (4d + 8)
    for the fp32-row forms."""
    if form == 7:
        return d + 4 + (4 if metric == 0 else 0)
    return 2 * d + (4 if metric == 0 else 0) if form == 6 else 4 * d + 8


def ivf_row_bytes_desc(form):
    if form == 7:
        return "|l|*(d+8) (int8 image + row scale + L2 row norm)"
    return "|l|*(2d+4) (fp16 image + L2 row norm)" if form == 6 else "|l|*(4d+8)"


def build_ivf(args, torch, hipann, rank, world, dev, n, d, nlist, nprobe, metric, r_dim, eta):
    """Low-intrinsic-dimension data + the GPU IVF build.  N=1: one pass over the rows;
    N>1: list sharding (sharded.assign_lists) unless HIPANN_IVF_SHARD=rows."""
    from ivf_build import build_ivf_list_shard, build_ivf_shard
    from sharded import shard_bounds

    gc = torch.Generator(device=dev)
    gc.manual_seed(7)
    basis = lowrank_basis(torch, r_dim, d, gc)
    xq = torch.empty((args.nq, d), device=dev, dtype=torch.float32)
    gen_lowrank_rows(torch, xq, 0, basis, eta, 4242)
    mode = os.environ.get("HIPANN_IVF_SHARD", "lists")
    if world > 1 and mode == "lists":
        gen = lambda out, row0: gen_lowrank_rows(torch, out, row0, basis, eta, 42)  # noqa: E731
        index, info = build_ivf_list_shard(torch, hipann, gen, n, d, nlist, nprobe, metric, rank, world, dev)
    else:
        lo, hi = shard_bounds(n, rank, world)
        xb = torch.empty((hi - lo, d), device=dev, dtype=torch.float32)
        gen_lowrank_rows(torch, xb, lo, basis, eta, 42)
        index, info = build_ivf_shard(torch, hipann, xb, lo, n, nlist, nprobe, metric, rank, world,
                                      centres_seed=1234)
        del xb
    torch.cuda.empty_cache()
    return index, info, xq, f"low-rank gaussian, intrinsic dim {r_dim}, noise {eta}"


def ivf_scan_stats(index, probes, d, nlist, row_bytes=None):
    from ivf_build import half_scan_groups, i8_scan_groups, scan_bytes, scan_group_rows, scan_pairs

    cnt = np.bincount(probes[probes >= 0].ravel(), minlength=nlist)
    # the form's query groups: fp16 form (6) narrow / wide (HIPANN_IVF_WIDE=0 disables the wide items), else 32
    g, w, gm = (half_scan_groups(d, int(os.environ.get("HIPANN_IVF_WIDE", "2")), os.environ.get("HIPANN_IVF_GEMM", "0") != "0")
                if index.form == 6 else i8_scan_groups(d) if index.form == 7 else (32, 0, 0))
    return {"scan_bytes_per_batch_local": scan_bytes(index, probes, d, row_bytes),
            "fp32_rows_bytes_per_batch_local": scan_bytes(index, probes, d),
            "distinct_lists_probed": int(np.unique(probes[probes >= 0]).size),
            "scanned_pairs_per_batch_local": scan_pairs(index, probes),
            "group_rows_per_batch_local": scan_group_rows(index, probes, g, w, gm),
            "query_groups": [g, w, gm],
            "probes_per_list_p50_p90_max": [int(np.percentile(cnt, 50)), int(np.percentile(cnt, 90)), int(cnt.max())]}


def kernel_timing_steps(torch, index, step, steps):
    """(main kernel ms, merge ms) of the last of a few extra steps run with the library's event timers on.  The
    timed steps run with the timers off: the event records around the kernels are not part of the measured step."""
    index.set_kernel_timing(True)
    for _ in range(max(2, min(steps, 5))):
        step()
    torch.cuda.synchronize()
    out = index.kernel_ms(0), index.kernel_ms(1)
    index.set_kernel_timing(False)
    return out


def ivf_config(args, torch, dist, hipann, rank, world, dev, steps, warmup, suite_extras=False):
    from ivf_build import flat_ground_truth
    from sharded import ShardedSearch, merge_packed_device_torch

    n, d, nq, k, nlist, nprobe = args.n, args.d, args.nq, args.k, args.nlist, args.nprobe
    metric = 0 if args.metric == "l2" else 1
    stream = torch.cuda.current_stream().cuda_stream
    t_setup = time.perf_counter()
    r_dim = int(os.environ.get("HIPANN_IVF_RANK", "16"))
    eta = float(os.environ.get("HIPANN_IVF_NOISE", "0.02"))
    index, info, xq, data_desc = build_ivf(args, torch, hipann, rank, world, dev, n, d, nlist, nprobe, metric,
                                           r_dim, eta)
    index.form = int(os.environ.get("HIPANN_IVF_FORM", "6"))
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t_setup

    # list sharding at N > 1: the coarse step partitioned over the ranks (each computes its slice's probe lists, one
    # all-gather of the lists) instead of N identical coarse passes; HIPANN_IVF_COARSE=replicated for A/B
    from sharded import PartitionedProbes, coarse_partition_ok
    pp = None
    if world > 1 and os.environ.get("HIPANN_IVF_SHARD", "lists") == "lists" and \
            os.environ.get("HIPANN_IVF_COARSE", "partitioned") == "partitioned" and coarse_partition_ok(nq, world):
        pp = PartitionedProbes(lambda qs, out: index.coarse_device(qs.shape[0], qs.data_ptr(), out.data_ptr(), stream),
                               nq, min(nprobe, nlist), dev)

    def local(q, D, I):
        if pp is not None:
            P = pp.probes(q)
            index.search_probes_device(q.shape[0], q.data_ptr(), P.data_ptr(), k, D.data_ptr(), I.data_ptr(), stream)
        else:
            index.search_device(q.shape[0], q.data_ptr(), k, D.data_ptr(), I.data_ptr(), stream)

    sharded = ShardedSearch(local, merge_packed_device_torch(hipann, metric), nq, k, dev)
    step = lambda: sharded.search(xq)  # noqa: E731
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    info["coarse_step"] = "partitioned over ranks + one all-gather of the probe lists" if pp is not None else \
        "replicated on every rank" if world > 1 else "single GPU"
    if not args.full:  # a plain run: the timed steps and the line
        el, (Dl, Il) = timed_steps(torch, dist, world, step, steps)
        dump_outputs(args, rank, Dl, Il)
        return {"workload": f"FAISS IVFFlat nlist={nlist} nprobe={nprobe}, {n}x{d} fp32 ({data_desc}), batch={nq}, "
                            f"k={k}",
                "value": round(nq * steps / el, 1), "ms_per_step": round(el * 1e3 / steps, 3),
                "setup_s": round(setup_s, 1), "ivf": info}, index
    probes = index.last_probes(nq)
    info.update(ivf_scan_stats(index, probes, d, nlist, ivf_row_bytes(index.form, d, metric)))
    if world == 1:  # the list sizes and this batch's probe lists (tests/golden/c3_lists_*.npz: sharding balance tests)
        try:
            DETAIL_PATH.parent.mkdir(parents=True, exist_ok=True)
            np.savez_compressed(DETAIL_PATH.parent / f"ivf_lists_{n}x{d}.npz", sizes=np.diff(index._offsets),
                                probes=probes.astype(np.int16 if nlist < 32768 else np.int32))
        except OSError:
            pass
    el, (Dl, Il) = timed_steps(torch, dist, world, step, steps)
    dump_outputs(args, rank, Dl, Il)
    del Dl, Il
    kern_ms, merge_ms = kernel_timing_steps(torch, index, step, steps)
    Dr, Ir = step()
    torch.cuda.synchronize()
    Ir = Ir.cpu().numpy().copy()
    Dr = Dr.cpu().numpy().copy()
    gt = flat_ground_truth(torch, hipann, d, metric, xq, k, n, rank, world, ivf_info_tensor=index)
    recall = recall_at(Ir, gt, k) if rank == 0 and gt is not None else None
    b_alg = info["scan_bytes_per_batch_local"]
    if world > 1:  # per-rank scan bytes (list sharding balance)
        t = torch.tensor([b_alg, kern_ms], device=dev, dtype=torch.float64)
        allv = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(allv, t)
        per = [float(v[0].item()) for v in allv]
        info["per_rank_scan_gb"] = [round(x / 1e9, 3) for x in per]
        info["per_rank_scan_kernel_ms"] = [round(float(v[1].item()), 3) for v in allv]
        info["scan_balance_max_over_mean"] = round(max(per) / (sum(per) / world), 4)
    form = index.form
    kname, fname = IVF_FORMS[form]
    fpp = 3.0 if form == 1 else 2.0  # flop per (query, row, dim): sub + fma vs fma
    achieved = b_alg / (kern_ms * 1e-3) / 1e9 if kern_ms > 0 else 0.0
    roof = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None, "kernel": kname,
            "kernel_ms": round(kern_ms, 3), "merge_ms": round(merge_ms, 3),
            "algorithmic": f"sum over distinct probed lists {ivf_row_bytes_desc(form)} B per launch (this rank's lists)",
            "form": fname,
            "scan_tflops": round(fpp * d * info["scanned_pairs_per_batch_local"] / (kern_ms * 1e-3) / 1e12, 2)
            if kern_ms > 0 else None}
    if kern_ms > 0:
        # SURVEY §8d's B_alg = Σ|ℓ|·(4d + 8) (the fp32 rows + labels) over the same kernel time.  The default
        # form reads the fp16 image (2d + 4 B per row) and certifies with an exact fp32 rerank, so this fraction
        # can exceed 1: it is the speed-up over an fp32-row stream at the HBM roofline, not a bandwidth.
        b_survey = info["fp32_rows_bytes_per_batch_local"]
        roof["frac_vs_survey_bytes"] = round(b_survey / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        roof["survey_bytes_per_launch_gb"] = round(b_survey / 1e9, 3)
    if world == 1:
        attach_traffic(roof, f"ivf_{n}x{d}", b_alg)
    out = {"workload": f"FAISS IVFFlat nlist={nlist} nprobe={nprobe}, {n}x{d} fp32 ({data_desc}), batch={nq}, k={k}",
           "value": round(nq * steps / el, 1), "ms_per_step": round(el * 1e3 / steps, 3), "recall_at_10": recall,
           "roofline": roof, "setup_s": round(setup_s, 1),
           "ivf": {kk: v for kk, v in info.items() if kk != "scan_bytes_per_batch_local"}}
    if world > 1:
        return out, index
    out["with_h2d_d2h"] = host_pointer_rate(torch, lambda q: sharded.search(q), xq, nq, k, max(5, steps // 2))
    if suite_extras:
        out["request_k30"] = request_k_line(torch, index, xq, k, 20, el * 1e3 / steps)
    if not args.no_alt_forms:
        alt = {}
        for f in (5, 3, 0):
            if f == form:
                continue
            index.form = f
            step()
            torch.cuda.synchronize()
            index.set_kernel_timing(True)
            ta = time.perf_counter()
            for _ in range(5):
                step()
            torch.cuda.synchronize()
            ea = time.perf_counter() - ta
            kms = index.kernel_ms(0)
            index.set_kernel_timing(False)
            _, Ia = step()
            torch.cuda.synchronize()
            Ia = Ia.cpu().numpy()
            b_f = info["fp32_rows_bytes_per_batch_local"]
            alt[IVF_FORMS[f][1]] = {"form": f, "queries_per_s": round(nq * 5 / ea, 1), "scan_kernel_ms": round(kms, 3),
                                    "recall_at_10": recall_at(Ia, gt, k),
                                    "ids_equal_to_reported_form": round(float((Ia == Ir).mean()), 6),
                                    "roofline": {"bound": "hbm", "kernel": IVF_FORMS[f][0],
                                                 "achieved": round(b_f / (kms * 1e-3) / 1e9, 1) if kms > 0 else None,
                                                 "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                                 "frac": round(b_f / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                                                 if kms > 0 else None,
                                                 "algorithmic": "SURVEY §8d: Σ distinct probed lists |ℓ|·(4d+8) "
                                                                "(this form streams the fp32 rows)"}}
        index.form = form
        out["other_forms"] = alt
    out["ivf"]["rerank_fallbacks_total"] = index.rerank_fallbacks()
    if suite_extras:
        out["latency"] = ivf_latency(torch, index, xq, k, d, metric)
    if not args.no_cpu_baseline:
        out["cpu_baseline"] = ivf_cpu_baseline(index, xq, k, nprobe, metric, args.cpu_seconds, gpu_DI=(Dr, Ir))
        par = out["cpu_baseline"].pop("parity", None)
        if par is not None:
            out["parity_vs_cpu_path"] = par
    if suite_extras:  # last: it grows the index
        out["append"] = ivf_append_line(torch, index, xq, k, d, r_dim, eta, el * 1e3 / steps)
    return out, index


def ivf_append_line(torch, index, xq, k, d, r_dim, eta, base_ms, rows=2048, reps=10):
    """The extension's INSERT path on the GPU copy (faiss_index.cpp:469: Append per data chunk of <= 2048 rows):
    hipann_ivf_add of a 2048-row chunk (host rows: coarse assignment on the GPU, rows into their lists' slack, touched
    fp16-image passes re-tiled) followed by the next 1024-query search, timed together, against the plain search step
    (within 1.3x).  The first append moves the borrowed lists into owned storage with slack (timed apart)."""
    dev = xq.device
    gc = torch.Generator(device=dev)
    gc.manual_seed(7)
    basis = lowrank_basis(torch, r_dim, d, gc)
    new = torch.empty(((reps + 1) * rows, d), device=dev, dtype=torch.float32)
    gen_lowrank_rows(torch, new, 0, basis, eta, 777)
    new_h = new.cpu().numpy()
    del new
    nq = xq.shape[0]
    stream = torch.cuda.current_stream().cuda_stream
    D = torch.empty((nq, k), device=dev, dtype=torch.float32)
    I = torch.empty((nq, k), device=dev, dtype=torch.int64)
    search = lambda: index.search_device(nq, xq.data_ptr(), k, D.data_ptr(), I.data_ptr(), stream)  # noqa: E731
    n_before = index.ntotal
    torch.cuda.synchronize()
    t_idle = 0.0  # the same search from an idle GPU (its launch latency exposed, as after an append)
    for _ in range(reps):
        t0 = time.perf_counter()
        search()
        torch.cuda.synchronize()
        t_idle += time.perf_counter() - t0
    idle_ms = t_idle * 1e3 / reps
    t0 = time.perf_counter()
    index.add(new_h[:rows])
    first_ms = (time.perf_counter() - t0) * 1e3
    search()
    torch.cuda.synchronize()
    t_add = t_pair = 0.0
    for r in range(1, reps + 1):
        t0 = time.perf_counter()
        index.add(new_h[r * rows:(r + 1) * rows])
        t1 = time.perf_counter()
        search()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_add += t1 - t0
        t_pair += t2 - t0
    pair_ms = t_pair * 1e3 / reps
    return {"workload": f"hipann_ivf_add of {rows} host rows + the next {nq}-query search, {reps} times",
            "append_ms": round(t_add * 1e3 / reps, 3), "append_plus_search_ms": round(pair_ms, 3),
            "search_step_ms": round(base_ms, 3), "vs_search_step": round(pair_ms / base_ms, 3) if base_ms > 0 else None,
            "search_from_idle_ms": round(idle_ms, 3), "vs_search_from_idle": round(pair_ms / idle_ms, 3) if idle_ms > 0 else None,
            "first_append_ms": round(first_ms, 1),
            "first_append_note": "moves the borrowed CSR into owned lists with slack (once)",
            "ntotal": [n_before, index.ntotal], "rows_per_s": round(rows * reps / t_add, 1) if t_add > 0 else None}


def ivf_latency(torch, index, xq, k, d, metric=0):
    """nq = 1 / 4 through the IVF path (the extension's per-query call, faiss_index.cpp:737)."""
    stream = torch.cuda.current_stream().cuda_stream
    res = {}
    for nq in (1, 4):
        q = xq[:nq].contiguous()
        D = torch.empty((nq, k), device=xq.device)
        I = torch.empty((nq, k), device=xq.device, dtype=torch.int64)
        call = lambda: index.search_device(nq, q.data_ptr(), k, D.data_ptr(), I.data_ptr(), stream)  # noqa: E731
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        probes = index.last_probes(nq)
        from ivf_build import scan_bytes
        b = scan_bytes(index, probes, d, ivf_row_bytes(index.form, d, metric))
        index.set_kernel_timing(True)
        it = 20
        t0 = time.perf_counter()
        for _ in range(it):
            call()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        kms = index.kernel_ms(0)
        index.set_kernel_timing(False)
        gbs = b / (kms * 1e-3) / 1e9 if kms > 0 else 0.0
        res[f"nq{nq}"] = {"ms_per_call": round(el * 1e3 / it, 4), "scan_kernel_ms": round(kms, 4),
                          "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                       "frac": round(gbs / HBM_PEAK_GBS, 4),
                                       "algorithmic": f"probed lists {ivf_row_bytes_desc(index.form)} = {b / 1e9:.4f} GB per call"}}
    return res


def ivf_cpu_baseline(index, xq, k, nprobe, metric, cpu_seconds, gpu_DI=None):
    """The CPU path timed on the host cores, and (gpu_DI = the GPU's (D, I) for the same batch) its answers
    compared with the GPU's under the parity rule (oracle/parity.py): north_star's "returned ids match the
    extension's CPU FAISS path on identical inputs" at the headline size (faiss_index.cpp:729-737).  Every
    query of the batch runs whenever the oracle does it in ≤ 60 s (≈ 3.4 s for 1024 at 10M x 768)."""
    from oracle import cpu_baseline as CB

    try:
        cen, codes, ids = index._keep
        cen_h, codes_h, ids_h = cen.cpu().numpy(), codes.cpu().numpy(), ids.cpu().numpy()
        off = index._offsets
        xq_h = xq.cpu().numpy()
        nq = xq_h.shape[0]
        s0 = min(16, nq)
        _, dt0, _ = CB.ivf_qps(cen_h, off, ids_h, codes_h, xq_h[:s0], k, nprobe, metric)
        per_q = max(dt0, 1e-3) / s0
        s = nq if per_q * nq <= 60.0 else int(min(nq, max(s0, cpu_seconds / per_q)))
        qps, dt, nth, Do, Io = CB.ivf_search_timed(cen_h, off, ids_h, codes_h, xq_h[:s], k, nprobe, metric)
        res = {"value": round(qps, 2), "unit": "queries/s", "cores": nth, "kind": "port",
               "sample": f"first {s} of {nq} queries ({dt:.1f} s) through the C oracle's FAISS "
                         f"IndexIVFFlat::search restatement (coarse quantizer + direct SIMD distances + heaps, "
                         f"OpenMP over queries) on the same centroids and lists"}
        if gpu_DI is not None:
            from oracle.parity import topk_parity

            pos = np.empty(ids_h.shape[0], np.int64)
            pos[ids_h] = np.arange(ids_h.shape[0], dtype=np.int64)
            Dg, Ig = gpu_DI
            res["parity"] = topk_parity(lambda labs: codes_h[pos[labs]], xq_h[:s], Dg[:s], Ig[:s], Do, Io, metric,
                                        max_sqnorm_dev(codes), same_rtol=2e-6)
            res["parity"]["rule"] = PARITY_RULE + "; at equal ids, within 2e-6 of the CPU path's fp32 direct-form distance"
        return res
    except Exception as e:
        return {"value": None, "error": repr(e)}


C3_MIX_SIGMA = float(os.environ.get("HIPANN_C3_MIX_SIGMA", "0.8"))


def ivf_clustered_config(args, torch, dist, hipann, dev):
    """SURVEY §8(d)'s own C3 data model: 4096 centres U(-1,1)^768 (seed 7), rows = centre +
    N(0, σ²I) (seed 42), queries from the same mixture (seed 4242), σ calibrated so that recall@10 at nprobe 32 lies
    in [0.95, 0.99] (`tools/c3_clustered_sweep.py` on the MI355X: σ 0.7 → 0.991, 1.0 → 0.882; σ = 0.8 here).  The
    same GPU build as the headline (k-means++ and 25 Lloyd iterations with FAISS's split_clusters on a 256·nlist
    sample); Lloyd does not collapse into empty lists here, but the lists are skewed (max/mean reported).  Reports
    the smallest nprobe with recall@10 >= 0.95, its QPS and scan roofline, the nprobe = 32 point, the exact forms'
    flagged queries, and parity against the CPU path (IndexIVFFlat::search) on 256 queries."""
    from ivf_build import build_ivf_shard, flat_ground_truth

    n, d, nq, k, nlist = args.n, args.d, args.nq, args.k, args.nlist
    stream = torch.cuda.current_stream().cuda_stream
    gc = torch.Generator(device=dev)
    gc.manual_seed(7)
    centres = (torch.rand((4096, d), generator=gc, device=dev, dtype=torch.float32) * 2 - 1).contiguous()
    xb = torch.empty((n, d), device=dev, dtype=torch.float32)
    gen_clustered_rows(torch, xb, 0, centres, C3_MIX_SIGMA, 42)
    xq = torch.empty((nq, d), device=dev, dtype=torch.float32)
    gen_clustered_rows(torch, xq, 0, centres, C3_MIX_SIGMA, 4242)
    t0 = time.perf_counter()
    index, info = build_ivf_shard(torch, hipann, xb, 0, n, nlist, args.nprobe, 0, 0, 1, centres_seed=1234)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    del xb
    torch.cuda.empty_cache()
    gt = flat_ground_truth(torch, hipann, d, 0, xq, k, n, 0, 1, ivf_info_tensor=index)
    D = torch.empty((nq, k), device=dev)
    I = torch.empty((nq, k), device=dev, dtype=torch.int64)
    call = lambda: index.search_device(nq, xq.data_ptr(), k, D.data_ptr(), I.data_ptr(), stream)  # noqa: E731
    sweep, best = [], None
    for nprobe in (1, 2, 4, 8, 16, 32, 64):
        index.nprobe = nprobe
        call()
        torch.cuda.synchronize()
        f0 = index.rerank_fallbacks()
        t1 = time.perf_counter()
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        el = time.perf_counter() - t1
        rec = recall_at(I.cpu().numpy(), gt, k)
        sweep.append({"nprobe": nprobe, "queries_per_s": round(nq * 3 / el, 1), "recall_at_10": round(rec, 4),
                      "flagged_per_batch": (index.rerank_fallbacks() - f0) / 3})
        if rec >= 0.95 and best is None:
            best = nprobe
        if nprobe >= 32 and best is not None:
            break
    sizes = np.diff(index._offsets)
    out = {"workload": f"FAISS IVFFlat nlist={nlist}, {n}x{d} fp32 (SURVEY §8d mixture: 4096 centres U(-1,1), "
                       f"sigma {C3_MIX_SIGMA}), batch={nq}, k={k}, smallest nprobe with recall@10 >= 0.95",
           "sigma": C3_MIX_SIGMA, "build_s": round(build_s, 1),
           "list_size_max_over_mean": round(float(sizes.max() / sizes.mean()), 2),
           "list_size_p50_p90_p99_max": [int(np.percentile(sizes, p)) for p in (50, 90, 99)] + [int(sizes.max())],
           "lists_empty": int((sizes == 0).sum()), "sweep": sweep, "smallest_nprobe": best}
    if best is None:
        out["error"] = "recall@10 >= 0.95 not reached by nprobe 64"
        index.close()
        return out
    index.nprobe = best
    steps = 10
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    f0 = index.rerank_fallbacks()
    el, _ = timed_steps(torch, dist, 1, call, steps)
    flagged = (index.rerank_fallbacks() - f0) / steps
    kern_ms, merge_ms = kernel_timing_steps(torch, index, call, steps)
    call()
    torch.cuda.synchronize()
    Dr, Ir = D.cpu().numpy().copy(), I.cpu().numpy().copy()
    probes = index.last_probes(nq)
    st = ivf_scan_stats(index, probes, d, nlist, ivf_row_bytes(index.form, d, 0))
    b_alg = st["scan_bytes_per_batch_local"]
    grp = st["group_rows_per_batch_local"] * ivf_row_bytes(index.form, d, 0)
    out.update({"nprobe": best, "value": round(nq * steps / el, 1), "ms_per_step": round(el * 1e3 / steps, 3),
                "recall_at_10": round(recall_at(Ir, gt, k), 4), "rerank_fallbacks_total": flagged * steps,
                "flagged_per_batch": flagged,
                "roofline": {"bound": "hbm", "kernel": IVF_FORMS[index.form][0], "kernel_ms": round(kern_ms, 3),
                             "merge_ms": round(merge_ms, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "achieved": round(b_alg / (kern_ms * 1e-3) / 1e9, 1) if kern_ms > 0 else None,
                             "frac": round(b_alg / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if kern_ms > 0 else None,
                             "algorithmic": "sum over distinct probed lists |l|*(2d+4) B per launch",
                             "streamed_group_rows_gb": round(grp / 1e9, 3),
                             "frac_streamed_rows": round(grp / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                             if kern_ms > 0 else None},
                "ivf": {kk: v for kk, v in st.items() if kk != "scan_bytes_per_batch_local"}})
    if not args.no_cpu_baseline:
        xs = xq[:256].contiguous()
        cb = ivf_cpu_baseline(index, xs, k, best, 0, 30.0, gpu_DI=(Dr[:256], Ir[:256]))
        par = cb.pop("parity", None)
        out["cpu_baseline"] = cb
        if par is not None:
            out["parity_vs_cpu_path"] = par
    index.close()
    return out


def ivf_robustness(args, torch, dist, hipann, dev):
    """Recall@10 and QPS against nprobe at intrinsic ranks 16 / 24 / 32 (same 10M x 768 shape, same build):
    the smallest nprobe reaching recall@10 >= 0.95 and its QPS, per rank."""
    from ivf_build import flat_ground_truth

    k, nq, d, n = args.k, args.nq, args.d, args.n
    stream = torch.cuda.current_stream().cuda_stream
    res = {}
    for r_dim in (16, 24, 32):
        index, info, xq, _ = build_ivf(args, torch, hipann, 0, 1, dev, n, d, args.nlist, args.nprobe, 0, r_dim, 0.02)
        gt = flat_ground_truth(torch, hipann, d, 0, xq, k, n, 0, 1, ivf_info_tensor=index)
        D = torch.empty((nq, k), device=dev)
        I = torch.empty((nq, k), device=dev, dtype=torch.int64)
        sweep = []
        best = None
        for nprobe in (16, 32, 48, 64, 96, 128, 192, 256):
            index.nprobe = nprobe
            call = lambda: index.search_device(nq, xq.data_ptr(), k, D.data_ptr(), I.data_ptr(), stream)  # noqa
            call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            rec = recall_at(I.cpu().numpy(), gt, k)
            sweep.append({"nprobe": nprobe, "queries_per_s": round(nq * 3 / el, 1), "recall_at_10": round(rec, 4)})
            if rec >= 0.95 and best is None:
                best = sweep[-1]
            if rec >= 0.99:
                break
        res[f"intrinsic_dim_{r_dim}"] = {"smallest_nprobe_at_recall_0.95": best, "sweep": sweep,
                                         "list_size_min_max": [info["list_size_min"], info["list_size_max"]]}
        index.close()
        del index, call, xq
        torch.cuda.empty_cache()
    return res


# ------------------------------------------------------------------------------------------------
# DiskANN (C4)
# ------------------------------------------------------------------------------------------------
def diskann_config(args, torch, dist, hipann, rank, world, dev, n, d, nq, k, L, R, steps, warmup, cpu=True,
                   resident=True, full=True, dump=False):
    """C4: DiskProvider::search_batch over n x d SQ8, L_search, R, nq queries.  full=False (the
    headline of a plain run): the set-up, the warm-up and the timed steps only; dump: the run's headline
    configuration, whose last timed step --dump-outputs writes.

    Graph traversal does not shard, so N GPUs run N replicas (each holds the whole SQ8 DB and answers
    its own batch; weak scaling, no collective).  A step = one BFS batch of nq queries:
      * default: diskann_hip_search_batch_resident_device — the traversal on the GPU; roofline of that
        kernel, algorithmic bytes = distances x d (SQ8 code rows) + expansions x 4R (adjacency rows);
      * resident=False: diskann_hip_search_batch — the reference's structure (host lock-step BFS, one
        id-gather launch per step); roofline of the id-gather kernel, d + 12 B per distance."""
    import diskann_build as DB

    metric = 0 if args.metric == "l2" else 1
    t_setup = time.perf_counter()
    gc = torch.Generator(device=dev)
    gc.manual_seed(8)
    r_dim = int(os.environ.get("HIPANN_DISKANN_RANK", "16"))
    eta = float(os.environ.get("HIPANN_DISKANN_NOISE", "0.02"))
    basis = lowrank_basis(torch, r_dim, d, gc)
    xb = torch.empty((n, d), device=dev, dtype=torch.float32)
    gen_lowrank_rows(torch, xb, 0, basis, eta, 42)
    xq = torch.empty((nq, d), device=dev, dtype=torch.float32)
    gen_lowrank_rows(torch, xq, 0, basis, eta, 4242 + rank)
    codes, mins, scale = DB.sq8_encode(torch, xb)
    adj_t, medoid = DB.knn_graph(torch, xb, R=R, n_random=R // 4, seed=8)
    torch.cuda.synchronize()
    t_graph = time.perf_counter() - t_setup
    adj = DB.adjacency_u32(torch, adj_t)
    del adj_t
    codes_h = codes.cpu().numpy()
    db = hipann.DiskannDeviceDB(codes_h, hipann.DiskannDeviceDB.FMT_SQ8, mins.cpu().numpy(), scale.cpu().numpy())
    del codes
    torch.cuda.empty_cache()
    xq_h = xq.cpu().numpy()
    eps = np.array([medoid], np.uint32)
    stream = torch.cuda.current_stream().cuda_stream
    if resident:
        db.register_graph(adj)
        I_dev = torch.empty((nq, k), device=dev, dtype=torch.int64)
        D_dev = torch.empty((nq, k), device=dev, dtype=torch.float32)
    setup_s = time.perf_counter() - t_setup

    def step():
        if resident:
            st = db.search_batch_resident_device(eps, nq, xq.data_ptr(), k, L, I_dev.data_ptr(), D_dev.data_ptr(),
                                                 metric, stream)
            return None, None, st
        return db.search_batch(adj, eps, xq_h, k, L, metric)

    for _ in range(warmup):
        step()
    # the timed steps run with the library's event timers off (their markers are not part of the step); the kernel
    # time comes from a few extra steps with the timers on
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    evals = pops = requeries = 0
    bfs_steps = []
    for _ in range(steps):
        ids, dd, st = step()
        evals += st["evals"]
        pops += st.get("pops", 0)
        requeries += st.get("host_requeries", 0)
        bfs_steps.append(st["steps"])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    qps = world * nq * steps / elapsed
    if dump:
        dump_outputs(args, rank, D_dev if resident else dd, I_dev if resident else ids)
    data_desc = (f"low-rank gaussian rows, intrinsic dim {r_dim}, noise {eta}; SQ8-encoded; graph = {R - R // 4} "
                 f"exact cell-local nearest neighbours + {R // 4} random edges, medoid entry point")
    workload = f"DISKANN DiskProvider batch-distance, {n}x{d} sq8, L_search={L}, R={R}, batch={nq}, k={k}"
    if not full:
        db.close()
        return {"workload": workload, "value": round(qps, 1), "unit": "queries/s",
                "ms_per_step": round(elapsed * 1e3 / steps, 3), "steps": steps, "setup_s": round(setup_s, 1),
                "data": data_desc}
    tsteps = max(1, min(steps, 3))
    db.set_kernel_timing(True)
    evals_t = pops_t = 0
    for _ in range(tsteps):
        _, _, st_t = step()
        evals_t += st_t["evals"]
        pops_t += st_t.get("pops", 0)
    torch.cuda.synchronize()
    kern_total_ms, launches = db.kernel_stats()
    db.set_kernel_timing(False)
    if resident:
        ids = I_dev.cpu().numpy()
    gt = DB.exact_topk(torch, xb, xq, k, metric).cpu().numpy()
    recall = recall_at(ids, gt, k)
    if resident:
        b_alg = evals_t * d + pops_t * 4 * R
        kname = "diskann_bfs"
        alg = (f"distances x d B (SQ8 code rows) + expansions x 4R B (adjacency rows) = "
               f"{b_alg / tsteps / 1e9:.3f} GB per batch (one launch per batch)")
    else:
        b_alg = evals_t * (d + 12)
        kname = "dist_ids_sq8"
        alg = (f"distances x (d + 12) B = {d + 12} B per distance (SQ8 code row + id + query_map + out), summed "
               f"over the timed launches")
    achieved = b_alg / (kern_total_ms * 1e-3) / 1e9 if kern_total_ms > 0 else 0.0
    roof = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None, "kernel": kname,
            "kernel_ms_per_launch": round(kern_total_ms / max(launches, 1), 4),
            "kernel_ms_per_batch": round(kern_total_ms / tsteps, 3), "launches_per_batch": launches / tsteps,
            "distances_per_batch": evals // steps, "expansions_per_batch": pops // steps if resident else None,
            "algorithmic": alg}
    if world == 1:
        attach_traffic(roof, f"diskann_{n}x{d}", b_alg / max(launches, 1))
    out = {"workload": workload,
           "value": round(qps, 1), "unit": "queries/s", "ms_per_step": round(elapsed * 1e3 / steps, 3),
           "steps": steps, "recall_at_10": recall, "roofline": roof, "setup_s": round(setup_s, 1),
           "data": data_desc,
           "diskann": {"graph_build_s": round(t_graph, 1), "bfs_steps_per_batch": int(np.mean(bfs_steps)),
                       "traversal": "GPU-resident (one 2-wavefront workgroup per query)" if resident else
                                    f"host lock-step BFS ({os.environ.get('HIPANN_BFS_THREADS', '16')} threads) + "
                                    f"per-step id-gather launches",
                       "host_requeries": requeries}}
    if cpu and rank == 0 and world == 1:
        try:
            from oracle import oracle as O
            m_h, s_h = mins.cpu().numpy(), scale.cpu().numpy()
            s0 = 16
            t1 = time.perf_counter()
            O.diskann_search_batch(adj, eps, xq_h[:s0], k, L, metric, codes=codes_h, mins=m_h, scale=s_h)
            dt0 = time.perf_counter() - t1
            s1 = int(min(nq, max(s0, s0 * 5.0 / max(dt0, 1e-3))))
            t1 = time.perf_counter()
            oi, _, _ = O.diskann_search_batch(adj, eps, xq_h[:s1], k, L, metric, codes=codes_h, mins=m_h, scale=s_h)
            dt = time.perf_counter() - t1
            out["cpu_baseline"] = {
                "value": round(s1 / dt, 2), "unit": "queries/s", "cores": O.num_threads(), "kind": "port",
                "sample": f"first {s1} of {nq} queries ({dt:.1f} s) through the C oracle's DiskProvider::search_batch "
                          f"restatement (lock-step BFS on the host, SQ8 distances OpenMP over each step's candidates) "
                          f"on the same graph and codes"}
            out["ids_equal_to_oracle_bfs"] = round(float((oi == ids[:s1]).mean()), 5)
        except Exception as e:
            out["cpu_baseline"] = {"value": None, "error": repr(e)}
    db.close()
    del xb, xq
    torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------
# C1 and the reference's published microbenchmark
# ------------------------------------------------------------------------------------------------
def c1_config(torch, hipann, dev):
    """C1: FAISS Flat L2 10k x 128, k = 10, gpu=false — the CPU path (the oracle restates FAISS's CPU
    IndexFlatL2::search), timed at nq = 1000 (BLAS form) and per query (nq = 1, the extension's call),
    next to the GPU path through the host-pointer C ABI (hipann_flat_search, PCIe included), which
    EnsureGpuIndex's AUTO gates (ntotal >= 256, d >= 128, faiss_index.cpp:128-143) would select."""
    from oracle import oracle as O

    sys.path.insert(0, str(ROOT / "tests"))
    from _data import faiss_metal_case

    xb, xq = faiss_metal_case(10_000, 1000, 128)
    res = {"workload": "FAISS Flat L2, 10k x 128 fp32, k=10 (mt19937(42) U(-1,1), faiss-metal test inputs)"}
    t0 = time.perf_counter()
    Do, Io = O.flat_search(xb, xq, 10)
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i in range(200):
        O.flat_search(xb, xq[i:i + 1], 10)
    dt1 = time.perf_counter() - t0
    res["cpu_path"] = {"kind": "port", "cores": O.num_threads(), "batch1000_queries_per_s": round(1000 / dt, 1),
                       "nq1_ms_per_query": round(dt1 * 1e3 / 200, 4),
                       "note": "C oracle (FAISS IndexFlatL2::search restatement): BLAS form at nq >= 20 (OpenMP over "
                               "queries), direct fvec_L2sqr per query at nq = 1"}
    ix = hipann.HipIndexFlat(128, 0, xb)
    D, I = ix.search(xq, 10)
    res["gpu_ids_equal_to_cpu_path"] = float((I == Io).mean())
    for _ in range(3):
        ix.search(xq, 10)
    t0 = time.perf_counter()
    for _ in range(10):
        ix.search(xq, 10)
    dtg = time.perf_counter() - t0
    for i in range(5):
        ix.search(xq[i:i + 1], 10)
    t0 = time.perf_counter()
    for i in range(200):
        ix.search(xq[i:i + 1], 10)
    dtg1 = time.perf_counter() - t0
    res["gpu_path_host_pointers"] = {"batch1000_queries_per_s": round(10_000 / dtg, 1),
                                     "nq1_ms_per_query": round(dtg1 * 1e3 / 200, 4)}
    ix.close()
    return res


README_SHAPES = [(64, 128, 4, 448), (64, 768, 53, 453), (128, 1536, 210, 495), (256, 1536, 424, 415),
                 (512, 1536, 870, 380), (1024, 768, 784, 532)]  # (n, d, M1 Pro CPU us, Metal us), README.md:140-145


def batch_distance_microbench(hipann):
    """The reference's only published hot-path numbers (README.md:140-147): one query vs n candidates,
    L2, through the host-pointer bridge (diskann_hip_batch_distances: H2D of the candidates, kernel, D2H),
    next to the CPU (ComputeDistancesCPU restatement, one thread, as the Rust caller runs per query); and
    the break-even n·d that sets MIN_GPU_WORK (metal_ffi.rs:36-46)."""
    from oracle import oracle as O

    rng = np.random.default_rng(1)

    import ctypes

    lib = O.lib()
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731

    def time_pair(n, d, it):
        """Median per-call time of the three calls, sampled interleaved (GPU, scalar CPU, SIMD CPU, GPU, …) so
        that clock or load drift during the run hits all three alike."""
        q = rng.uniform(-1, 1, d).astype(np.float32)
        c = rng.uniform(-1, 1, (n, d)).astype(np.float32)
        out = np.empty(n, np.float32)
        ref = np.empty(n, np.float32)
        calls = (lambda: hipann.diskann_hip_batch_distances(q, c, n, d, 0, out),
                 lambda: lib.oracle_batch_distances(fp(q), fp(c), n, d, 0, fp(ref)),
                 lambda: lib.oracle_batch_distances_simd(fp(q), fp(c), n, d, 0, fp(ref)))
        for f in calls:
            for _ in range(5):
                f()
        ts = [[], [], []]
        for _ in range(it):
            for j, f in enumerate(calls):
                t0 = time.perf_counter()
                f()
                ts[j].append(time.perf_counter() - t0)
        g, cpu, simd = (float(np.median(t)) * 1e6 for t in ts)
        return g, cpu, simd

    rows = []
    for n, d, m1_cpu, metal in README_SHAPES:
        g, cpu, simd = time_pair(n, d, 200)
        rows.append({"n": n, "d": d, "gpu_us": round(g, 1), "cpu_us": round(cpu, 1), "speedup": round(cpu / g, 3),
                     "cpu_simd_us": round(simd, 1),
                     "reference_m1pro_cpu_us": m1_cpu, "reference_metal_us": metal,
                     "reference_speedup": round(m1_cpu / metal, 2)})
    sweep = []
    even = even_simd = None
    for nd_log in range(12, 23):
        nd = 1 << nd_log
        d = 768
        n = max(1, nd // d)
        g, cpu, simd = time_pair(n, d, 100)
        sweep.append({"n_times_d": n * d, "gpu_us": round(g, 1), "cpu_us": round(cpu, 1), "cpu_simd_us": round(simd, 1)})
        if even is None and g < cpu:
            even = n * d
        if even_simd is None and g < simd:
            even_simd = n * d
    return {"shapes": rows, "break_even_sweep_d768": sweep, "break_even_n_times_d": even,
            "break_even_n_times_d_simd_cpu": even_simd,
            "gates_this_run_supports": {"MIN_GPU_WORK": even_simd, "MIN_GPU_WORK_ONESHOT": even,
                                        "rule": "smallest swept n*d (powers of two, d = 768) whose median GPU call "
                                                "beats the median CPU call, samples interleaved"},
            "gates_from": "MIN_GPU_WORK_ONESHOT (ann_search.cpp:696-699, scalar ComputeDistancesCPU) <- break_even_n_times_d; "
                          "MIN_GPU_WORK (metal_ffi.rs:41, Rust SIMD distances) <- break_even_n_times_d_simd_cpu",
            "cpu": "oracle_batch_distances (ComputeDistancesCPU restatement, sequential fp32 sum, 1 thread); "
                   "cpu_simd: 16-accumulator AVX2 loop (timing model of diskann-vector's SIMD kernel, 1 thread)",
            "gpu": "diskann_hip_batch_distances (host pointers: candidates H2D + kernel + D2H, synchronous)",
            "current_gates": {"MIN_GPU_WORK": hipann.MIN_GPU_WORK, "MIN_GPU_WORK_ONESHOT": hipann.MIN_GPU_WORK_ONESHOT}}


def flat_auto_gate(hipann):
    """EnsureGpuIndex's AUTO gates (ntotal >= 256, d >= 128, faiss_index.cpp:128-143) are Metal numbers.  The
    extension searches one query per call (faiss_index.cpp:737), so the MI355X break-even is the table size
    from which the host-pointer nq = 1 call (hipann_flat_search: query in, scan, top-k out) beats the CPU
    path's per-query search (the oracle's FAISS IndexFlat direct-form restatement, one thread at nq = 1)."""
    from oracle import oracle as O

    rng = np.random.default_rng(3)
    out = {}
    for d, sizes in ((128, (1024, 4096, 16384, 65536, 262144, 1048576)), (768, (1024, 4096, 16384, 65536, 262144))):
        rows, even = [], None
        for n in sizes:
            xb = rng.random((n, d), dtype=np.float32)
            xq = rng.random((24, d), dtype=np.float32)
            ix = hipann.HipIndexFlat(d, 0, xb)
            for i in range(4):
                ix.search(xq[i:i + 1], 10)
            t0 = time.perf_counter()
            for i in range(4, 24):
                ix.search(xq[i:i + 1], 10)
            g = (time.perf_counter() - t0) / 20 * 1e6
            ix.close()
            O.flat_search(xb, xq[:1], 10)
            t0 = time.perf_counter()
            for i in range(4, 24):
                O.flat_search(xb, xq[i:i + 1], 10)
            c = (time.perf_counter() - t0) / 20 * 1e6
            rows.append({"ntotal": n, "gpu_us": round(g, 1), "cpu_us": round(c, 1)})
            if even is None and g < c:
                even = n
        out[f"d{d}"] = {"sweep": rows, "break_even_ntotal": even}
    out["reference_gate"] = "AUTO: ntotal >= 256 and d >= 128 (faiss_index.cpp:128-143)"
    out["cpu"] = "oracle flat_search, nq = 1 (direct fvec_L2sqr form, one thread)"
    out["gpu"] = "hipann_flat_search, nq = 1, host pointers (pinned staging, copy kernels, scan, top-k)"
    return out


def run_suite(args, torch, dist, hipann, dev):
    """Every other BASELINE configuration, N = 1, same run."""
    cfg = {}

    def guarded(name, fn):
        if args.only and name not in args.only.split(","):
            return
        t0 = time.perf_counter()
        try:
            cfg[name] = fn()
        except Exception as e:  # a sub-configuration never kills the headline line
            log(f"[bench] {name} failed: {e!r}")
            cfg[name] = {"error": repr(e)}
        cfg[name]["wall_s"] = round(time.perf_counter() - t0, 1)
        torch.cuda.empty_cache()

    def flat(n, metric=0, oracle_queries=0, latency=False, steps=10, request_k=False):
        out, index, xb = flat_config(args, torch, dist, hipann, 0, 1, dev, n, 768, 1024, args.k, metric, steps, 2,
                                     cpu_seconds=5.0, oracle_queries=oracle_queries, latency=latency,
                                     request_k=request_k)
        index.close()
        del index, xb
        return out

    guarded("C1_flat_10k_128_cpu_path", lambda: c1_config(torch, hipann, dev))
    guarded("C2_flat_l2_1m_768", lambda: flat(1_000_000, oracle_queries=1024))
    guarded("flat_l2_10m_768", lambda: flat(10_000_000, oracle_queries=1024, latency=True, steps=5, request_k=True))
    if "request_k30" in cfg.get("flat_l2_10m_768", {}):
        cfg["flat_l2_10m_768_request_k30"] = cfg["flat_l2_10m_768"].pop("request_k30")
    guarded("C4_diskann_1m_1536_sq8", lambda: diskann_config(args, torch, dist, hipann, 0, 1, dev, 1_000_000, 1536,
                                                             1024, args.k, 128, 64, 10, 2))
    # C4 through the path hip_ffi.rs's fallback takes when the graph is not registered: DiskProvider::search_batch's
    # own structure (host lock-step BFS, disk_provider.rs:539-638) with each step's distances from the id-gather
    # kernel (dist_ids_sq8: d + 12 B per distance) — the kernel SURVEY §8d's C4 row prices
    guarded("C4_diskann_1m_1536_sq8_host_bfs", lambda: diskann_config(args, torch, dist, hipann, 0, 1, dev, 1_000_000,
                                                                      1536, 1024, args.k, 128, 64, 3, 1,
                                                                      resident=False))
    guarded("reference_readme_batch_distances", lambda: batch_distance_microbench(hipann))
    guarded("flat_auto_gate_nq1", lambda: flat_auto_gate(hipann))
    guarded("ivf_recall_vs_nprobe", lambda: ivf_robustness(args, torch, dist, hipann, dev))
    guarded("C3_ivf_survey_mixture", lambda: ivf_clustered_config(args, torch, dist, hipann, dev))
    return cfg


C5_ROWS_PER_GPU = 12_500_000  # BASELINE configs[4]: 100M x 768 over 8 GPUs


def c5_config(args, torch, dist, hipann, rank, world, dev):
    """BASELINE configs[4]: Flat IP over 100M x 768 fp32 sharded across 8 GPUs — per-GPU
    partial top-k over a contiguous 12.5M-row shard (labels offset to global rows), one packed RCCL
    all-gather + merge on every rank.  Each rank holds 12.5M rows whatever N is, so N = 8 is exactly C5
    (100M rows) and N < 8 runs the same per-GPU shard over 12.5M·N rows (weak scaling)."""
    n = C5_ROWS_PER_GPU * world
    steps = max(3, min(args.steps, 10))
    out, index, xb = flat_config(args, torch, dist, hipann, rank, world, dev, n, 768, 1024, args.k, 1, steps, 2,
                                 alt_forms=world == 1 and not args.no_alt_forms, host_rate=False,
                                 oracle_queries=256 if world == 1 and not args.no_cpu_baseline else 0)
    index.close()
    del index, xb
    torch.cuda.empty_cache()
    out["scaling"] = "weak"
    out["rows_per_gpu"] = C5_ROWS_PER_GPU
    out["note"] = (f"{world} GPU(s) x 12.5M rows = {n / 1e6:g}M rows; at 8 GPUs this is C5's 100M x 768 "
                   "(per-GPU shard, one packed all-gather of nq x k (dist, label) per rank over RCCL, merge on "
                   "every rank)")
    if world == 1 and not args.no_cpu_baseline:
        xq = uniform_queries(torch, 1024, 768, dev)
        out["cpu_baseline"] = flat_cpu_baseline(torch, xq, 100_000_000, 768, args.k, 1, 5.0)
        out["cpu_baseline"]["note"] = "the whole 100M-row job on this host's cores (SURVEY §8d C5: a slice, extrapolated)"
    return out


# ------------------------------------------------------------------------------------------------
def spawn_ranks(args) -> int:
    """--gpus N > 1 started without a launcher: run the N ranks as torch.distributed.run's children (one process
    per GPU, rendezvous on 127.0.0.1) and return their exit status.  This parent process never initialises a GPU
    (only argument parsing happened) and is not replaced: the ranks are child processes; rank 0 prints the
    line to the inherited stdout."""
    import socket
    import subprocess

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", str(Path(__file__).resolve())] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on these hosts (RCCL)
    log(f"[bench] starting {args.gpus} ranks: {' '.join(cmd)}")
    return subprocess.call(cmd, env=env)


def selftest(args, torch, dist, world, rank):
    """CPU check of the launcher and the timing protocol (gloo): every rank joins, the ranks all-gather their
    RANK, and `steps` timed all-gathers run between the barriers with the max-over-ranks elapsed time."""
    if world > 1:
        dist.init_process_group("gloo")
    mine = torch.tensor([rank], dtype=torch.int64)
    seen = [torch.empty_like(mine) for _ in range(world)]
    step = (lambda: dist.all_gather(seen, mine)) if world > 1 else (lambda: seen[0].copy_(mine))  # noqa: E731
    for _ in range(args.warmup):
        step()
    el, _ = timed_steps(torch, dist, world, step, args.steps, gpu=False)
    ranks_seen = sorted(int(t.item()) for t in seen)
    if ranks_seen != list(range(world)):
        raise SystemExit(f"launcher self-test: ranks seen {ranks_seen} != 0..{world - 1}")
    line = {"metric": "launcher self-test (all-gathers/s)", "value": round(args.steps / el, 1), "unit": "all-gathers/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(el * 1e3 / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "int64", "data": "synthetic",
            "config": {"workload": "selftest", "parallelism": f"ranks{world}"},
            "world_check": {"backend": dist.get_backend() if world > 1 else None, "ranks_seen": ranks_seen}}
    if rank == 0 and args.dump_outputs:  # what the last timed all-gather left: the ranks it saw
        Path(args.dump_outputs).mkdir(parents=True, exist_ok=True)
        np.save(Path(args.dump_outputs) / "ranks_seen.npy", np.array([int(t.item()) for t in seen], np.float64))
    if rank == 0:
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


def world_check(torch, dist, world, rank, dev):
    """Every rank's RANK all-gathered over the data-path backend (RCCL at N > 1): the line states the ranks the
    collective saw, and the run stops if it is not 0..N-1."""
    if world == 1:
        return {"backend": None, "ranks_seen": [0]}
    mine = torch.tensor([rank], dtype=torch.int64, device=dev)
    allr = torch.empty(world, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(allr, mine)
    seen = sorted(allr.cpu().tolist())
    if seen != list(range(world)):
        raise SystemExit(f"RCCL saw ranks {seen}, expected 0..{world - 1}")
    return {"backend": dist.get_backend(), "ranks_seen": seen}


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log(f"[bench] note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE")
    if args.workload == "selftest":
        return selftest(args, torch, dist, world, rank)
    import hipann

    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
    if not hipann.is_available():
        raise SystemExit("libhipann.so / HIP device not available")
    wcheck = world_check(torch, dist, world, rank, dev)
    metric = 0 if args.metric == "l2" else 1

    if args.workload == "diskann":
        sub = diskann_config(args, torch, dist, hipann, rank, world, dev, args.n, args.d, args.nq, args.k,
                             args.l_search, args.degree, args.steps, args.warmup, cpu=not args.no_cpu_baseline,
                             resident=not args.diskann_host_bfs, full=args.full, dump=True)
        line = {"metric": "queries/sec @ recall@10>=0.95 (DiskANN DiskProvider batch path, 1Mx1536 sq8, L_search=128)",
                "value": sub.pop("value"), "unit": "queries/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": sub.pop("ms_per_step"), "higher_is_better": True,
                "scaling": "weak", "vs_baseline": None, "dtype": "u8 codes, f32 accumulate",
                "data": "synthetic (generated on device: " + sub.pop("data") + ")",
                "config": {"workload": sub.pop("workload"), "global_batch": args.nq * world, "n": args.n, "d": args.d,
                           "k": args.k, "parallelism": f"replicas{world}"}}
        line.update(sub)
    else:
        if args.workload == "flat":
            sub, index, xb_keep = flat_config(args, torch, dist, hipann, rank, world, dev, args.n, args.d, args.nq, args.k,
                                        metric, args.steps, args.warmup, alt_forms=not args.no_alt_forms,
                                        cpu_seconds=0.0 if args.no_cpu_baseline else args.cpu_seconds,
                                        full=args.full, dump=True)
            dtype = ("f32 results (int8-image certified filter, int32 sums + exact fp32 rerank)" if sub.get("form") == 5
                     else "f32 results (bf16-image certified filter + exact fp32 rerank)" if sub.get("form") == 4 else "f32")
            data = "U(-1,1) rows"
        else:
            sub, index = ivf_config(args, torch, dist, hipann, rank, world, dev, args.steps, args.warmup,
                                    suite_extras=args.suite and world == 1)
            dtype = ("f32 results (fp16-image certified filter + exact fp32 rerank)" if index.form == 6 else
                     "f32 results (int8-image certified filter, int32 sums + exact fp32 rerank)" if index.form == 7 else
                     "f32 results (bf16-split certified filter + exact fp32 rerank)" if index.form == 5 else "f32")
            data = "low-intrinsic-dimension gaussian rows (DESIGN.md §8)"
        line = {"metric": METRIC, "value": sub.pop("value"), "unit": "queries/s", "n_gpus": world,
                "steps": args.steps, "warmup": args.warmup, "ms_per_step": sub.pop("ms_per_step"),
                "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": dtype,
                "data": f"synthetic (generated on device: {data})",
                "config": {"workload": sub.pop("workload"), "global_batch": args.nq, "n": args.n, "d": args.d,
                           "k": args.k, "parallelism": f"shard{world}" + (
                               f" ({os.environ.get('HIPANN_IVF_SHARD', 'lists')})" if args.workload == "ivf" and
                               world > 1 else "")}}
        sub.pop("unit", None)
        line.update(sub)
        if args.workload == "ivf" and index.form == 6:
            line["precision"] = ("returned distances are fp32 direct-form Σ(q−x)² (FAISS CPU IVFFlatScanner "
                                 "arithmetic); the scan is a certified filter, not an fp32 stream: it reads an fp16 "
                                 "image of the rows (2d+4 B per row, half of SURVEY §8d's 4d+8) and only prunes, and a "
                                 "per-query bound (|scan key − exact| ≤ 2(|q|·max‖x−x̂‖ + ‖q−q̂‖·max‖x̂‖) + fp32 "
                                 "accumulation) proves no pruned row reaches the top-k (failures re-run on the device "
                                 "in the direct form).  roofline.frac counts the image bytes the kernel streams; "
                                 "roofline.frac_vs_survey_bytes counts SURVEY's fp32-row bytes; the fp32-row stream "
                                 "itself is other_forms' form 5 line with its own roofline")
        elif args.workload == "ivf" and index.form == 5:
            line["precision"] = ("returned distances are fp32 direct-form Σ(q−x)² (FAISS CPU IVFFlatScanner "
                                 "arithmetic); the bf16 2-term split scan only prunes, and a per-query bound "
                                 "(|scan key − exact| ≤ 2^-12·(|q|²+max|x|²)) proves no pruned row reaches the top-k "
                                 "(failures re-run on the device in the direct form)")
        if (args.suite and world == 1) or not args.no_c5:
            index.close()
            del index
            torch.cuda.empty_cache()
        rk_line = line.pop("request_k30", None)
        if args.suite and world == 1:
            line["configs"] = run_suite(args, torch, dist, hipann, dev)
        if rk_line is not None:
            line.setdefault("configs", {})["C3_ivf_request_k30"] = rk_line
        if not args.no_c5 and args.workload == "ivf":
            t0 = time.perf_counter()
            try:
                c5 = c5_config(args, torch, dist, hipann, rank, world, dev)
            except Exception as e:  # report, never lose the main line
                c5 = {"error": repr(e)}
            c5["wall_s"] = round(time.perf_counter() - t0, 1)
            line.setdefault("configs", {})["C5_flat_ip_100m_768_sharded"] = c5
    line["world_check"] = wcheck
    line["build"] = build_provenance()
    if os.environ.get("HIPANN_RR_PROF_DUMP"):  # tuning builds only (HIPANN_RR_PROF): the rerank's phase clocks
        import ctypes
        buf = (ctypes.c_ulonglong * 16)()
        if hipann.lib().hipann_debug_rr_prof(buf) == 0 and buf[7]:
            names = {0: "setup", 1: "loads", 5: "bound_count", 2: "select_sort", 3: "distances", 4: "order_ties", 8: "write"}
            log("rerank phase clocks per query (wave 0):", {v: round(buf[i] / buf[7]) for i, v in names.items()},
                "compaction-path", buf[6], "list-path", buf[9], "queries", buf[7])
    emit(line, rank, detail=args.full)
    if world > 1:
        dist.destroy_process_group()
    reap_children()


def reap_children():
    """VERDICT r05 item 10 (a process left behind after the bench, r04 and r05): every process this run started
    (psutil children, recursive) and every other process of its process group / session is named on stderr, and
    the children are terminated (then killed) before the bench returns."""
    try:
        import psutil
    except ImportError:
        return
    me = psutil.Process()
    kids = me.children(recursive=True)
    try:
        pgid, sid = os.getpgid(0), os.getsid(0)
        skip = {me.pid} | {q.pid for q in me.parents()} | {q.pid for q in kids}
        others = [p for p in psutil.process_iter(["pid", "name", "cmdline"])
                  if p.pid not in skip and p.ppid() not in skip - {me.pid} and _same_group(p, pgid, sid)]
    except Exception:
        others = []
    for p in kids + others:
        try:
            log(f"[bench] process at exit: pid {p.pid} ppid {p.ppid()} {' '.join(p.cmdline())[:160]!r}"
                f"{' (child)' if p in kids else ''}")
        except Exception:
            pass
    for p in kids:
        try:
            p.terminate()
        except Exception:
            pass
    _, alive = psutil.wait_procs(kids, timeout=3)
    for p in alive:
        try:
            p.kill()
        except Exception:
            pass


def _same_group(p, pgid, sid):
    try:
        return os.getpgid(p.pid) == pgid or os.getsid(p.pid) == sid
    except OSError:
        return False


if __name__ == "__main__":
    main()
