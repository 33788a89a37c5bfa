"""IVF SQ8 range search against the SQ8 top-k call on one MI355X: 2M x 768 L2, nlist 1024, nprobe 32, by_residual 1,
the data and quantizer of tools/ivf_sq8_bench.py.  nq = 1024 and nq = 1, one process, inputs resident, the two
workloads alternating on the same handle:

  range  hipann_ivfsq_range_search_device, radius = the median over (at most 128 of) the queries of their 35th-best
         distance among the probed lists (the entry point takes one radius per call), so about 35 rows per query qualify
  topk   hipann_ivfsq_search_device, k = 10: the number to compare with

Per workload: median and range of the repeats' device time (events around the call, which for range includes the call's
one readback); for range also the rows returned, the stages' device times (scan, offsets, fill: a timed call of their
own), the filter's survivors and the share of them the recheck rejected.  One JSON line per (nq, workload) on stdout
(and in --out, when given).
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
    ap.add_argument("--nq", type=int, nargs="*", default=[1024, 1])
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
    rows = xb[order].contiguous()
    del xb
    # the quantizer: per-dimension min / max of the residuals, FAISS's encode, in row chunks
    lists = torch.repeat_interleave(torch.arange(nlist, device="cuda"), torch.from_numpy(np.diff(off)).cuda())
    vmin = torch.full((d,), float("inf"), device="cuda")
    vmax = torch.full((d,), float("-inf"), device="cuda")
    for r0 in range(0, n, 262144):
        res = rows[r0:r0 + 262144] - cen[lists[r0:r0 + 262144]]
        vmin, vmax = torch.minimum(vmin, res.min(0).values), torch.maximum(vmax, res.max(0).values)
    vdiff = vmax - vmin
    codes = torch.empty((n, d), dtype=torch.uint8, device="cuda")
    for r0 in range(0, n, 262144):
        res = rows[r0:r0 + 262144] - cen[lists[r0:r0 + 262144]]
        codes[r0:r0 + 262144] = (((res - vmin) / vdiff).clamp(0, 1) * 255).to(torch.int32).to(torch.uint8)
    del res, rows
    sq = hipann.HipIndexIVFSQ8(cen.cpu().numpy(), vmin.cpu().numpy(), vdiff.cpu().numpy(), off, order.cpu().numpy(),
                               codes.cpu().numpy(), nprobe=nprobe, metric=hipann.METRIC_L2, by_residual=True)
    del codes
    info = hipann.lib().hipann_debug_ivfsq_info
    info.argtypes, info.restype = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)], C.c_int

    def stat(name):
        v = C.c_double()
        assert info(sq.handle, name.encode(), C.byref(v)) == 0, name
        return v.value

    lines = []
    for nq in args.nq:
        xq = xq_all[:nq].contiguous()
        ns = min(nq, 128)
        Dk = torch.empty((ns, 35), dtype=torch.float32, device="cuda")
        Ik = torch.empty((ns, 35), dtype=torch.int64, device="cuda")
        sq.search_device(ns, xq.data_ptr(), 35, Dk.data_ptr(), Ik.data_ptr())
        torch.cuda.synchronize()
        radius = float(Dk[:, 34].median()) * 1.0001
        D10 = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
        I10 = torch.empty((nq, 10), dtype=torch.int64, device="cuda")
        lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
        cap = 4096 * nq
        Dr = torch.empty(cap, dtype=torch.float32, device="cuda")
        Ir = torch.empty(cap, dtype=torch.int64, device="cuda")

        def run(w):
            if w == "topk":
                sq.search_device(nq, xq.data_ptr(), 10, D10.data_ptr(), I10.data_ptr())
                return nq * 10
            assert sq.range_search_device(nq, xq.data_ptr(), radius, lims.data_ptr(), Dr.data_ptr(), Ir.data_ptr(),
                                          cap), "cap too small"
            return int(lims[nq])

        found = {}
        for w in ("range", "topk"):  # warm-up
            found[w] = run(w)
        torch.cuda.synchronize()
        probed_rows = int(np.diff(off)[sq.last_probes(nq)].sum())
        s0, a0 = stat("range_survivors"), stat("range_admitted")
        sq.set_kernel_timing(True)  # the stages and the filter's counters in a timed call of their own
        run("range")
        torch.cuda.synchronize()
        stage = {k: stat("range_" + k + "_ms") for k in ("scan", "offsets", "fill")}
        scan_kernel_ms = sq.kernel_ms(0)
        sq.set_kernel_timing(False)
        surv, adm = int(stat("range_survivors") - s0), int(stat("range_admitted") - a0)
        ms = {"range": [], "topk": []}
        for _ in range(args.repeats):  # alternating, timing off
            for w in ("range", "topk"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(w)
                e1.record()
                torch.cuda.synchronize()
                ms[w].append(e0.elapsed_time(e1))
        for w in ("range", "topk"):
            rec = {"n": n, "d": d, "nlist": nlist, "nprobe": nprobe, "nq": nq, "workload": w,
                   "ms_median": statistics.median(ms[w]), "ms_min": min(ms[w]), "ms_max": max(ms[w]), "ms": ms[w],
                   "rows": found[w], "probed_rows": probed_rows}
            if w == "range":
                rec.update(radius=radius, stage_ms=stage, scan_kernel_ms=scan_kernel_ms, filter_survivors=surv,
                           admitted=adm, rejected_fraction=(1 - adm / surv) if surv else None)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
