"""Flat range search against the top-k yardstick on one MI355X: 1M x 768 L2, nq = 1024 and nq = 1, one process,
the three workloads alternating:

  a  range search, radius = the median over the queries of their exact 10th-neighbour distance, plus 0.1 %
     (the entry point takes one radius per call), so about 10 rows per query qualify;
  b  hipann_flat_search_device, k = 10, form HIPANN_FLAT_FORM_BF16_EXACT, on the same handle: the same image;
  c  range search with the radius at the 1 % quantile of a sample of distances: the recheck and the fill when
     survivors are not rare.

Per workload: median and range of the repeats' wall time (device events around the call, which ends in the call's
own synchronisation for a / c), the scan passes' kernel time (hipann_last_kernel_ms(0), averaged over the repeats),
rows returned, and for a / c the filter survivors and the fraction of them the direct form rejected.
One JSON line per (nq, workload) on stdout (and in --out, when given).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "duckdb-annsearch_amd"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import torch

    import hipann

    n, d = args.n, args.d
    g = torch.Generator(device="cuda").manual_seed(1234)
    xb = torch.rand((n, d), generator=g, device="cuda") * 2 - 1
    xq_all = torch.rand((1024, d), generator=g, device="cuda") * 2 - 1
    ix = hipann.HipIndexFlatDevice(d, hipann.METRIC_L2, xb.data_ptr(), n)
    ix.form = 4  # HIPANN_FLAT_FORM_BF16_EXACT
    surv = hipann.lib().hipann_debug_flat_range_survivors
    surv.argtypes, surv.restype = [C.c_void_p], C.c_int64
    lines = []
    for nq in (1024, 1):
        xq = xq_all[:nq].contiguous()
        D10 = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
        I10 = torch.empty((nq, 10), dtype=torch.int64, device="cuda")
        ix.search_device(nq, xq.data_ptr(), 10, D10.data_ptr(), I10.data_ptr())
        torch.cuda.synchronize()
        r_a = float(D10[:, 9].median()) * 1.001
        sample = torch.cdist(xq[:64], xb[:20000]) ** 2
        r_c = float(torch.quantile(sample.flatten()[:1_000_000], 0.01))
        lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
        cap = int(nq * n * 0.03) + 1024
        Dr = torch.empty(cap, dtype=torch.float32, device="cuda")
        Ir = torch.empty(cap, dtype=torch.int64, device="cuda")

        def run(w):
            if w == "b":
                ix.search_device(nq, xq.data_ptr(), 10, D10.data_ptr(), I10.data_ptr())
                return nq * 10
            ok = ix.range_search_device(nq, xq.data_ptr(), r_a if w == "a" else r_c, lims.data_ptr(), Dr.data_ptr(),
                                        Ir.data_ptr(), cap)
            assert ok, "cap too small"
            return int(lims[nq])

        ms = {w: [] for w in "abc"}
        kms, rows, sv = {}, {}, {}
        for w in "abc":  # warm-up, then kernel time and survivors per workload on their own
            run(w)
            torch.cuda.synchronize()
            s0 = surv(ix.handle)
            ix.set_kernel_timing(True)
            for _ in range(3):
                rows[w] = run(w)
            torch.cuda.synchronize()
            kms[w] = ix.kernel_ms(0)
            ix.set_kernel_timing(False)
            sv[w] = (surv(ix.handle) - s0) // 3
        for _ in range(args.repeats):  # alternating, timing off
            for w in "abc":
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(w)
                e1.record()
                torch.cuda.synchronize()
                ms[w].append(e0.elapsed_time(e1))
        for w in "abc":
            rec = {"n": n, "d": d, "nq": nq, "workload": w, "radius": {"a": r_a, "b": None, "c": r_c}[w],
                   "ms_median": statistics.median(ms[w]), "ms_min": min(ms[w]), "ms_max": max(ms[w]), "ms": ms[w],
                   "scan_kernel_ms_per_pass": kms[w], "rows": rows[w]}
            if w != "b":
                rec["filter_survivors"] = sv[w]
                rec["rejected_fraction"] = (1 - rows[w] / sv[w]) if sv[w] else None
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
