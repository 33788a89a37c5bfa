"""The seeded int8 list scan (csrc/ivf.cpp: the chunk-0 items, ivf_seed_bound, then the other items under the seed's
64th key): every case answers the oracle's top-k under the parity rule, repeats bit for bit, and equals —
ids, distances and the certificate's flag count — the answer of the single-launch scan, which one fresh child process
gives for all cases with HIPANN_IVF_SEED=0.  The cases and their layouts are in tests/_seed_cases.py.
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _seed_cases as S
from _data import check_topk_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def unseeded(gpu, tmp_path_factory):
    """Every case's answer from a child process that runs the single launch."""
    out = tmp_path_factory.mktemp("seed") / "unseeded.npz"
    env = dict(os.environ, HIPANN_IVF_SEED="0")
    r = subprocess.run([sys.executable, str(Path(S.__file__).resolve()), str(out)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.parametrize("name", list(S.CASES))
def test_seeded_scan(gpu, oracle, unseeded, name):
    assert os.environ.get("HIPANN_IVF_SEED", "1") != "0", "this process must run the default path"
    r = S.run_case(gpu, name)
    want_seeded = S.CASES[name][6]
    assert r["path"]["seeded"] == want_seeded, r["path"]
    if S.CASES[name][2] == 7 and r["metric"] == 0:
        assert r["path"] == {"form": 7, "filter_k": 64, "sublists": 8, "seeded": want_seeded}, r["path"]
    cen, off, ids, codes = r["lists"]
    Do, Io, Po = oracle.ivf_search(cen, off, ids, codes, r["xq"], r["k"], len(cen), r["metric"])
    assert np.array_equal(np.sort(r["probes"], axis=1), np.sort(Po, axis=1))
    check_topk_parity(r["rows"], r["xq"], r["D"], r["I"], Do, Io, r["metric"])
    assert np.array_equal(r["I"], r["I2"]) and np.array_equal(r["D"], r["D2"])  # the same batch again
    # the single launch: the same rows, the same bits, the same flag count
    assert np.array_equal(r["I"], unseeded[name + ".I"])
    assert np.array_equal(r["D"].view(np.uint32), unseeded[name + ".D"].view(np.uint32))
    print(name, "flagged", r["flagged"], "single launch", int(unseeded[name + ".flagged"]))
    assert r["flagged"] == int(unseeded[name + ".flagged"])
