"""Building and growing an IVF SQ8 index on one MI355X: 2M x 768 L2, nlist 1024, by_residual 1, U(-1, 1) rows resident
in HBM, the centroids a stride sample of the rows (the data of tools/ivf_sq8_bench.py).  One process, wall time around
each call (train and add return after their last host wait):

  train   hipann_ivfsq_train_device over the whole table; beside it the ivf_sq_minmax kernel's byte count n·d·4 over
          8 TB/s (the call also runs the assignment, which the bound does not hold)
  add     hipann_ivfsq_add_device of the whole table into a handle created with zero rows; beside it the encode
          kernel's bytes (n·d·4 read + n·32·nstep written) over 8 TB/s (the call also runs the assignment, the
          statistics pass, one regroup and the readback of n assignments)
  chunk   hipann_ivfsq_add of a 2048-row host chunk, when it fits the lists' slack (chunks into the handle that took
          the whole table) and when it forces a regroup (the first chunk into a handle created dense from that
          handle's export, a fresh one per repeat; hipann_memory_bytes tells the two apart), against hipann_ivf_add
          of the same chunk into an IVFFlat handle over the same rows, centroids and lists — alternating

One JSON line per measurement on stdout (and in --out, when given): median, min and max of the repeats in ms.
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=40, help="2048-row chunks added to each handle")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import ctypes as C

    import numpy as np
    import torch

    import hipann

    n, d, nlist = args.n, args.d, args.nlist
    L = hipann.lib()
    g = torch.Generator(device="cuda").manual_seed(1234)
    xb = torch.rand((n, d), generator=g, device="cuda") * 2 - 1
    cen = xb[:: n // nlist][:nlist].contiguous()
    extra = (torch.rand((args.chunks * 2048, d), generator=g, device="cuda") * 2 - 1).cpu().numpy()
    lines = []

    def emit(name, ms, **kw):
        rec = dict(measure=name, n=n, d=d, nlist=nlist, repeats=len(ms), median_ms=statistics.median(ms), min_ms=min(ms),
                   max_ms=max(ms), **kw)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    vmin = torch.empty(d, device="cuda")
    vdiff = torch.empty(d, device="cuda")
    eb = C.create_string_buffer(1024)

    def train():
        rc = L.hipann_ivfsq_train_device(d, hipann.METRIC_L2, nlist, 1, C.c_void_p(cen.data_ptr()), n,
                                         C.c_void_p(xb.data_ptr()), 0, C.c_void_p(vmin.data_ptr()),
                                         C.c_void_p(vdiff.data_ptr()), None, eb, 1024)
        assert rc == 0, eb.value

    train()  # warm-up: scratch allocation, code load
    emit("train", [timed(train) for _ in range(args.repeats)], bound_ms=n * d * 4 / 8e12 * 1e3)
    cen_h, vmin_h, vdiff_h = cen.cpu().numpy(), vmin.cpu().numpy(), vdiff.cpu().numpy()
    nstep = (lambda raw: -(-raw // (4 if raw <= 4 else 8)) * (4 if raw <= 4 else 8))(-(-d // 32))

    def empty():
        return hipann.HipIndexIVFSQ8(cen_h, vmin_h, vdiff_h, np.zeros(nlist + 1, np.int64), np.zeros(0, np.int64),
                                     np.zeros((0, d), np.uint8), metric=hipann.METRIC_L2)

    ms = []
    sq = None
    for _ in range(args.repeats + 1):  # (the first is the warm-up)
        if sq is not None:
            sq.close()
        sq = empty()
        ms.append(timed(lambda: sq.add_device(n, xb.data_ptr())))
    emit("add_all", ms[1:], bound_ms=(n * d * 4 + n * 32 * nstep) / 8e12 * 1e3)
    # the IVFFlat handle over the same lists: the SQ8 handle's assignment, rows sorted by list
    ex_off = np.empty(nlist + 1, np.int64)
    assert L.hipann_ivfsq_export(sq.handle, None, None, None, ex_off.ctypes.data_as(C.POINTER(C.c_int64)), None, None, eb,
                                 1024) == 0
    ids = np.empty(n, np.int64)
    assert L.hipann_ivfsq_export(sq.handle, None, None, None, None, ids.ctypes.data_as(C.POINTER(C.c_int64)), None, eb,
                                 1024) == 0
    order = torch.from_numpy(ids).cuda()
    rows = xb[order].contiguous()
    del xb
    flat = hipann.HipIndexIVFFlat.from_device(d, hipann.METRIC_L2, nlist, 1, cen.data_ptr(), ex_off, order.data_ptr(),
                                              rows.data_ptr(), copy=True)
    fit, grow, fl = [], [], []
    for c in range(args.chunks):
        blk = extra[c * 2048:(c + 1) * 2048]
        mem = sq.memory_bytes
        t = timed(lambda: sq.add(blk))
        (grow if sq.memory_bytes != mem else fit).append(t)
        fl.append(timed(lambda: flat.add(blk)))
    if fit:
        emit("chunk_sq8_fit", fit)
    if grow:
        emit("chunk_sq8_regroup_in_run", grow)
    emit("chunk_ivfflat", fl[1:], note="the first chunk (it moves the borrowed rows into owned storage) left out")
    # the chunk that forces a regroup: the first add into a handle created dense from the export (capacity = length
    # in every list), a fresh handle per repeat, alternating with the IVFFlat handle
    ex = sq.export()
    sq.close()
    rg, fl2 = [], []
    for r in range(args.repeats):
        dense = hipann.HipIndexIVFSQ8(ex["centroids"], ex["vmin"], ex["vdiff"], ex["list_offsets"], ex["ids"],
                                      ex["codes"], metric=hipann.METRIC_L2)
        blk = extra[(r % args.chunks) * 2048:(r % args.chunks + 1) * 2048]
        mem = dense.memory_bytes
        rg.append(timed(lambda: dense.add(blk)))
        assert dense.memory_bytes > mem, "the dense handle's first chunk must regroup"
        fl2.append(timed(lambda: flat.add(blk)))
        dense.close()
    emit("chunk_sq8_regroup", rg, note="first 2048-row chunk into a dense handle: every list regrouped with slack")
    emit("chunk_ivfflat_beside_regroup", fl2)
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
