"""The seeded int8 scan's compact candidate runs (csrc/ivf_mfma.hip mf_finish_item: the second launch's waves append
only the rows they admitted, under one cursor per query; ivf_rerank_topk reads the seed list and cursor[q] entries;
DESIGN.md §5).  Every case runs the seeded path, answers the oracle's top-k under the parity rule, repeats bit for bit
three times, and equals — ids, distances and the certificate's flag count — the single-launch scan, which one fresh
child process gives for all cases with HIPANN_IVF_SEED=0.  The cases and their layouts are in
tests/_compact_run_cases.py.

Measured on an MI355X with HIPANN_IVF_RUN_STATS=1 (appended entries per query, mean / max): one_row_tail 7.6 / 36,
empty_run 0 / 0, full_run_near_copies 2240 / 7168 (20 of 64 runs past the rerank's 4096-entry block select, 16
queries flagged), two_groups_one_list 47.9 / 125, nprobe32 28.6 / 100, d100 41.1 / 119, d768_three_chunks_and_5
94.7 / 165, last_query_single_chunk 21.3 / 46.
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _compact_run_cases as R
from _data import check_topk_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def unseeded(gpu, tmp_path_factory):
    """Every case's answer from a child process that runs the single launch."""
    out = tmp_path_factory.mktemp("compact_run") / "unseeded.npz"
    env = dict(os.environ, HIPANN_IVF_SEED="0")
    r = subprocess.run([sys.executable, str(Path(R.__file__).resolve()), str(out)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.parametrize("name", list(R.CASES))
def test_compact_run(gpu, oracle, unseeded, name):
    assert os.environ.get("HIPANN_IVF_SEED", "1") != "0", "this process must run the default path"
    r = R.run_case(gpu, name)
    assert r["path"] == {"form": 7, "filter_k": 64, "sublists": 8, "seeded": 1}, r["path"]
    cen, off, ids, codes = r["lists"]
    Do, Io, Po = oracle.ivf_search(cen, off, ids, codes, r["xq"], r["k"], r["nprobe"], 0)
    assert (Io >= 0).all()  # the reference answer exists for every query
    assert np.array_equal(np.sort(r["probes"], axis=1), np.sort(Po, axis=1))
    check_topk_parity(codes, r["xq"], r["D"], r["I"], Do, Io, 0)
    for D2, I2 in r["repeats"]:  # the same batch again, twice: the appended order may differ, the answers may not
        assert np.array_equal(r["I"], I2) and np.array_equal(r["D"].view(np.uint32), D2.view(np.uint32))
    # the single launch: the same rows, the same bits, the same flag count
    assert np.array_equal(r["I"], unseeded[name + ".I"])
    assert np.array_equal(r["D"].view(np.uint32), unseeded[name + ".D"].view(np.uint32))
    single = int(unseeded[name + ".flagged"])
    print(name, "flagged", r["flagged"], "single launch", single)
    assert r["flagged"] == single
    if name == "full_run_near_copies":  # the flag-count comparison is not vacuous there
        assert 1 <= single < len(r["xq"]) // 2, single
