"""IVF SQ8 against the IVFFlat yardstick on one MI355X: 2M x 768 L2, nlist 1024, nprobe 32, k 10 (--k: any list of k,
e.g. 10 30 64 for the deep scan path), by_residual 1, the
data of tools/ivf_range_bench.py, the quantizer trained by per-dimension min / max of the residuals, FAISS's encode.
nq = 1024 and nq = 1, one process, inputs resident, the two handles alternating:

  flat  hipann_ivf_search_device on an IVFFlat handle over the same rows, centroids and lists (form 6, defaults)
  sq8   hipann_ivfsq_search_device
  sq8_parent  (--parent-lib PATH) the same call on an SQ8 handle of another build of the library, e.g. the parent
        commit's, loaded beside this one: the comparator of a change to the SQ8 path

Per handle: median and range of the repeats' device time (events around the call); for sq8 also the code scan's and
the rerank's kernel times, the scan's filter depth (0: the direct kernel), the candidates the rerank recomputes per query, the u8 bytes the scan streams (the tiled
rows of every probed list once per query group) as a fraction of 8 TB/s, the flagged queries, both handles' HBM bytes and recall@10 against the fp32 rows' exact neighbours (a
property of the quantizer).  One JSON line per (nq, k, handle) on stdout (and in --out, when given).
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
    ap.add_argument("--k", type=int, nargs="*", default=[10])
    ap.add_argument("--parent-lib", default=None, help="another build of libhipann.so: adds the sq8_parent handle")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch

    import hipann

    n, d, nlist, nprobe, k = args.n, args.d, args.nlist, args.nprobe, 10  # (k = 10: the recall reference)
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
    # exact neighbours over the fp32 rows (for recall), in row chunks
    best_d = torch.full((1024, k), float("inf"), device="cuda")
    best_i = torch.full((1024, k), -1, dtype=torch.int64, device="cuda")
    qn = (xq_all * xq_all).sum(1, keepdim=True)
    for r0 in range(0, n, 262144):
        blk = rows[r0:r0 + 262144]
        dist = qn + (blk * blk).sum(1)[None, :] - 2.0 * xq_all @ blk.T
        dd, ii = torch.cat([best_d, dist], 1).topk(k, dim=1, largest=False)
        best_i = torch.gather(torch.cat([best_i, order[r0:r0 + 262144][None, :].expand(1024, -1)], 1), 1, ii)
        best_d = dd
    del dist
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
    del res
    ids_h = order.cpu().numpy()
    sq_args = (cen.cpu().numpy(), vmin.cpu().numpy(), vdiff.cpu().numpy(), off, ids_h, codes.cpu().numpy())
    sq = hipann.HipIndexIVFSQ8(*sq_args, nprobe=nprobe, metric=hipann.METRIC_L2, by_residual=True)
    handles = {"sq8": sq}
    if args.parent_lib:  # a second copy of the host module over the other library
        import importlib.util

        spec = importlib.util.spec_from_file_location("hipann_parent", Path(hipann.__file__))
        parent = importlib.util.module_from_spec(spec)
        sys.modules["hipann_parent"] = parent
        spec.loader.exec_module(parent)
        parent.LIB_PATH = Path(args.parent_lib).resolve()
        handles["sq8_parent"] = parent.HipIndexIVFSQ8(*sq_args, nprobe=nprobe, metric=hipann.METRIC_L2, by_residual=True)
    del codes, sq_args
    flat = hipann.HipIndexIVFFlat.from_device(d, hipann.METRIC_L2, nlist, nprobe, cen.data_ptr(), off, order.data_ptr(),
                                              rows.data_ptr())
    info = hipann.lib().hipann_debug_ivfsq_info
    info.argtypes, info.restype = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)], C.c_int

    def sq_info(name, default=None):
        v = C.c_double()
        if info(sq.handle, name, C.byref(v)) != 0:
            assert default is not None, name
            return default
        return v.value

    raw = -(-d // 32)
    nstep = -(-raw // (4 if raw <= 4 else 8)) * (4 if raw <= 4 else 8)
    handles = {"flat": flat, **handles}
    lines = []
    for nq, kk in ((nq, kk) for nq in args.nq for kk in args.k):
        xq = xq_all[:nq].contiguous()
        D = {w: torch.empty((nq, kk), dtype=torch.float32, device="cuda") for w in handles}
        I = {w: torch.empty((nq, kk), dtype=torch.int64, device="cuda") for w in handles}

        def run(w):
            handles[w].search_device(nq, xq.data_ptr(), kk, D[w].data_ptr(), I[w].data_ptr())

        fb0 = sq.rerank_fallbacks()
        for w in handles:  # warm-up (the IVFFlat handle builds its image here)
            run(w)
            run(w)
        torch.cuda.synchronize()
        flagged = sq.rerank_fallbacks() - fb0
        depth = int(sq_info(b"filter_depth"))
        kern, kern2 = {}, {}
        re0 = sq_info(b"rechecked")
        for w, h in handles.items():  # the scan (0) and rerank / merge (1) kernels' own time, a timed call each
            h.set_kernel_timing(True)
            run(w)
            torch.cuda.synchronize()
            kern[w], kern2[w] = h.kernel_ms(0), h.kernel_ms(1)
            h.set_kernel_timing(False)
        re_per_q = (sq_info(b"rechecked") - re0) / nq
        ms = {w: [] for w in handles}
        for _ in range(args.repeats):  # alternating, timing off
            for w in handles:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(w)
                e1.record()
                torch.cuda.synchronize()
                ms[w].append(e0.elapsed_time(e1))
        # queries per scan item at the call's depth (ivf_sq_group), for the bytes the scan streams
        group = 16 * max(qt for qt in range(0, 5) if 16 * qt * ((nstep * 16 + 8) * 4 + 16 + 64 * max(depth, 16)) <= 160 * 1024)
        cnt = np.bincount(sq.last_probes(nq).ravel(), minlength=nlist)
        passes = -(-np.diff(off) // 32)
        streamed = int((passes * -(-cnt // group)).sum()) * nstep * 1024
        for w, h in handles.items():
            hits = (I[w][:, :k, None] == best_i[:nq, None, :]).any(2).float().mean().item()
            rec = {"n": n, "d": d, "nlist": nlist, "nprobe": nprobe, "nq": nq, "k": kk, "handle": w,
                   "ms_median": statistics.median(ms[w]), "ms_min": min(ms[w]), "ms_max": max(ms[w]), "ms": ms[w],
                   "scan_kernel_ms": kern[w], "rerank_kernel_ms": kern2[w], "hbm_bytes": h.memory_bytes, "recall_at_10_vs_fp32_exact": hits}
            if w == "sq8":
                rec.update(flagged_queries_2_calls=flagged, rechecked_per_query=re_per_q, filter_depth=depth)
                if depth:
                    rec.update(group=group, u8_bytes_streamed=streamed,
                               fraction_of_8TBps=streamed / (kern[w] * 1e-3) / 8e12 if kern[w] else None)
            if w == "sq8_parent":
                rec.update(same_ids_as_sq8=bool((I[w] == I["sq8"]).all().item()),
                           same_distances_as_sq8=bool((D[w] == D["sq8"]).all().item()))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
