"""The host-driven lock-step BFS (csrc/diskann_host_bfs.cpp; DESIGN.md §6, "Host BFS stages").

Its two visited-set paths — the bits on the device (the default), the per-query hash sets on the host (every batch
whose bits would pass 1 GiB, or HIPANN_BFS_GPU_VISITED=0) — hand each query the same fresh (distance, id) pairs in
neighbour order, so ids, distances, evaluation count and step count are equal by construction.  One fresh child
process answers every case of tests/_host_bfs_cases.py on the host sets; this process answers them on the device sets.

And the resident search's fallback: a query the traversal kernel cannot take is re-run by the same host BFS, so on a
shape where every query is flagged the resident answer is search_batch's, bit for bit.
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _host_bfs_cases as H
from _bfs_cases import _ragged_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_sets(gpu, tmp_path_factory):
    """Every case's answer from a child process whose host BFS keeps the visited sets on the host."""
    out = tmp_path_factory.mktemp("host_bfs") / "host_sets.npz"
    env = dict(os.environ, HIPANN_BFS_GPU_VISITED="0")
    r = subprocess.run([sys.executable, str(Path(H.__file__).resolve()), str(out)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.parametrize("name", list(H.CASES))
def test_visited_set_paths_same_bits(gpu, host_sets, name):
    assert os.environ.get("HIPANN_BFS_GPU_VISITED") is None, "this process must run the default path"
    r = H.run_case(gpu, name)
    nq = H.CASES[name][3]
    assert r["ids"].shape == (nq, 10) and r["dists"].shape == (nq, 10)
    if name == "complete6_padding":  # six reachable rows, then the pads
        assert np.all(r["ids"][:, :6] >= 0) and np.all(r["ids"][:, 6:] == -1)
        assert np.all(r["dists"][:, 6:] == np.finfo(np.float32).max)
    if nq == 0:
        assert r["evals"] == 0 and r["steps"] == 0
    print(name, "evals", int(r["evals"]), "steps", int(r["steps"]), "host sets", int(host_sets[name + ".evals"]),
          int(host_sets[name + ".steps"]))
    assert np.array_equal(r["ids"], host_sets[name + ".ids"])
    assert np.array_equal(r["dists"].view(np.uint32), host_sets[name + ".dists"].view(np.uint32))
    assert r["evals"] == host_sets[name + ".evals"]
    assert r["steps"] == host_sets[name + ".steps"]


@pytest.mark.parametrize("R", [80, 32])
def test_flagged_resident_queries_equal_search_batch_sq8(gpu, oracle, R):
    """SQ8 with d = 36 (no multiple of 8: outside the traversal kernel at any R) at the shape of
    test_resident_bfs_host_fallback_shapes, and at R = 32, where d alone flags every query."""
    rng = np.random.default_rng(2)
    n, d = 1500, 36
    x = rng.standard_normal((n, d)).astype(np.float32)
    qs = x[:50] + 0.05
    adj = _ragged_graph(oracle, x, R, rng)
    mins, scale = oracle.sq8_train(x)
    db = gpu.DiskannDeviceDB(oracle.sq8_encode(x, mins, scale), 1, mins, scale)
    db.register_graph(adj)
    ids, dists, st = db.search_batch_resident([3], qs, 10, 32)
    assert st["pops"] == 0 and st["host_requeries"] == 50
    hi, hd, hst = db.search_batch(adj, [3], qs, 10, 32)
    assert np.array_equal(ids, hi)
    assert np.array_equal(dists.view(np.uint32), hd.view(np.uint32))
    assert st["evals"] == hst["evals"] and st["steps"] == hst["steps"]
