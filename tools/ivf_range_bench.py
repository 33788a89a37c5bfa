"""IVF range search against the top-k yardstick on one MI355X: 2M x 768 L2, nlist 1024, nprobe 32 (the index the
remove timings use, built on the device), nq = 1024 and nq = 1, one process, the three workloads alternating:

  a  range search, radius = the median over the queries of their exact 35th-neighbour distance among the probed
     lists (the entry point takes one radius per call), so about 35 rows per query qualify;
  b  hipann_ivf_search_device, k = 10, on the same handle: the top-k path as it stands — the number to compare with;
  c  range search with the radius at the 1 % quantile of the distances between a sample of queries and the rows of
     their own probed lists: the recheck and the fill when survivors are not rare.

Per workload: median and range of the repeats' wall time (device events around the call, which for a / c includes
the call's one readback), rows returned, and for a / c the stages' device times (scan, offsets, fill: events around
each, a timed call of their own), the filter's survivors and the fraction of them the direct form rejected.
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
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch

    import hipann

    n, d, nlist, nprobe = args.n, args.d, args.nlist, args.nprobe
    g = torch.Generator(device="cuda").manual_seed(1234)
    xb = torch.rand((n, d), generator=g, device="cuda") * 2 - 1
    xq_all = torch.rand((1024, d), generator=g, device="cuda") * 2 - 1
    cen = xb[:: n // nlist][:nlist].contiguous()
    cq = hipann.HipIndexFlatDevice(d, hipann.METRIC_L2, cen.data_ptr(), nlist)
    assign = torch.empty((n, 1), dtype=torch.int64, device="cuda")
    a_d = torch.empty((65536, 1), dtype=torch.float32, device="cuda")
    for r0 in range(0, n, 65536):
        m = min(65536, n - r0)
        cq.search_device(m, xb[r0:r0 + m].data_ptr(), 1, a_d.data_ptr(), assign[r0:r0 + m].data_ptr())
    torch.cuda.synchronize()
    cq.close()
    order = torch.argsort(assign[:, 0], stable=True)
    off = np.zeros(nlist + 1, np.int64)
    off[1:] = np.cumsum(torch.bincount(assign[:, 0], minlength=nlist).cpu().numpy())
    codes = xb[order].contiguous()
    del xb
    ix = hipann.HipIndexIVFFlat.from_device(d, hipann.METRIC_L2, nlist, nprobe, cen.data_ptr(), off, order.data_ptr(),
                                            codes.data_ptr())
    info = hipann.lib().hipann_debug_ivf_info
    info.argtypes, info.restype = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)], C.c_int

    def stat(name):
        v = C.c_double()
        assert info(ix.handle, name.encode(), C.byref(v)) == 0, name
        return v.value

    lines = []
    for nq in (1024, 1):
        xq = xq_all[:nq].contiguous()
        Dk = torch.empty((nq, 35), dtype=torch.float32, device="cuda")
        Ik = torch.empty((nq, 35), dtype=torch.int64, device="cuda")
        ix.search_device(nq, xq.data_ptr(), 35, Dk.data_ptr(), Ik.data_ptr())
        torch.cuda.synchronize()
        r_a = float(Dk[:, 34].median()) * 1.0001
        probes = ix.last_probes(nq)[:8]
        sample = torch.cat([(torch.cdist(xq[i:i + 1], torch.cat([codes[off[l]:off[l + 1]] for l in pl])) ** 2).flatten()
                            for i, pl in enumerate(probes)])
        r_c = float(torch.quantile(sample[:: max(1, sample.numel() // 1_000_000)], 0.01))
        probed_rows = int(np.diff(off)[ix.last_probes(nq)].sum())
        D10 = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
        I10 = torch.empty((nq, 10), dtype=torch.int64, device="cuda")
        lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
        cap = int(probed_rows * 0.03) + 4096
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
        stage, rows, sv = {}, {}, {}
        for w in "abc":  # warm-up, then the stages and the survivors per workload in a timed call of their own
            rows[w] = run(w)
            torch.cuda.synchronize()
            if w == "b":
                continue
            s0 = stat("range_survivors")
            ix.set_kernel_timing(True)
            run(w)
            torch.cuda.synchronize()
            stage[w] = {k: stat("range_" + k + "_ms") for k in ("scan", "offsets", "fill")}
            ix.set_kernel_timing(False)
            sv[w] = int(stat("range_survivors") - s0)
        for _ in range(args.repeats):  # alternating, timing off
            for w in "abc":
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(w)
                e1.record()
                torch.cuda.synchronize()
                ms[w].append(e0.elapsed_time(e1))
        for w in "abc":
            rec = {"n": n, "d": d, "nlist": nlist, "nprobe": nprobe, "nq": nq, "workload": w,
                   "radius": {"a": r_a, "b": None, "c": r_c}[w], "ms_median": statistics.median(ms[w]),
                   "ms_min": min(ms[w]), "ms_max": max(ms[w]), "ms": ms[w], "rows": rows[w], "probed_rows": probed_rows}
            if w != "b":
                rec["stage_ms"] = stage[w]
                rec["filter_survivors"] = sv[w]
                rec["rejected_fraction"] = (1 - rows[w] / sv[w]) if sv[w] else None
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
