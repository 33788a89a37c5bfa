"""CPU tests of the inner-product prune's numpy restatement (tests/_vamana_ip_ref.py): the crate's own
known answers through the update step, the properties of prune_ip, and the condition that keeps the GPU tests honest —
their inputs must exercise the rule's order dependence."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

import _vamana_ip_ref as V

GOLDEN = Path(__file__).resolve().parent / "golden" / "occluding_known_answers.json"


def test_known_answers():
    cases = json.loads(GOLDEN.read_text())["cases"]
    assert len(cases) == 4
    for d_ik, d_jk, f, t, want in cases:
        got = V.occlude_update(d_ik, d_jk, f, t)
        assert got.dtype == np.float32 and got == np.float32(want), (d_ik, d_jk, f, t, got)


def test_thresholds():
    assert V.thresholds(1.0) == [np.float32(1.0)]
    assert V.thresholds(1.2) == [np.float32(1.0), np.float32(1.2)]
    t2 = V.thresholds(2.0)
    assert len(t2) == 5 and t2[-1] == np.float32(2.0) and t2[-2] < np.float32(2.0)  # the last pass is capped


def test_canonical_zero_and_order():
    x = np.array([[1, 0], [0, 1], [-1, 0], [2, 0]], np.float32)
    # from row 0: d(0,1) = -0.0 -> +0.0, d(0,2) = 1, d(0,3) = -2: negatives come first
    dd = V.dist_ip(x, 0, [1, 2, 3])
    assert not np.signbit(dd[0]) and dd.tolist() == [0.0, 1.0, -2.0]
    sel, tr = V.prune_ip(x, 0, [1, 2, 3, 0, 9, 3], None, 1, 1.0)
    assert sel.tolist() == [3] and not tr


@pytest.mark.parametrize("kind", ["dup4", "ints"])
def test_prune_ip_properties(kind):
    x, targets, pools = V.prune_inputs(kind, 16)
    pair = V.pair_ip(x)
    n = x.shape[0]
    for t in range(targets.size):
        p = int(targets[t])
        ids = np.unique(pools[t][(pools[t] < n) & (pools[t] != p)]).astype(np.int64)
        for R in (1, 8, 64):
            for alpha in (1.0, 1.2, 2.0):
                sel, tr = V.prune_ip(x, p, pools[t], None, R, alpha, pair=pair)
                assert sel.size <= R and p not in sel and np.unique(sel).size == sel.size
                assert set(sel.tolist()) <= set(ids.tolist())
                assert tr == (ids.size > V.POOL_MAX)
                if ids.size:
                    dd = pair[p, ids]
                    first = int(ids[np.lexsort((ids, dd))[0]])
                    assert sel.size >= 1 and int(sel[0]) == first
                if alpha == 1.0:  # a single pass: nothing to remember
                    sl, _ = V.prune_ip(x, p, pools[t], None, R, alpha, pair=pair, stateless=True)
                    assert np.array_equal(sel, sl)
                # distances handed in (a search result's) give what computed ones give
                if ids.size:
                    s2, _ = V.prune_ip(x, p, ids, pair[p, ids], R, alpha)
                    assert np.array_equal(sel, s2)


@pytest.mark.parametrize("kind", ["dup4", "ints"])
def test_gpu_inputs_exercise_the_order_dependence(kind):
    """On each of test_prune_ip_exact's two inputs at alpha = 1.2 the stateless variant must select a different list
    than prune_ip for at least half of the targets (pools of 1 and 2 ids included, which cannot differ), and for some
    target at every d: a kernel that forgot the per-position counts could not pass there.  At d = 1536 the dots of
    rows of values 0..3 concentrate (3456 ± 105), only a row's copies occlude at t = 1.2, and fewer targets differ
    (15 of 40 against 30 and 32 of 40 at d = 16 and 100); the integer rows differ for 30 to 34 of 40 at every d."""
    differ, total = 0, 0
    for d in (16, 100, 1536):
        x, targets, pools = V.prune_inputs(kind, d)
        pair = V.pair_ip(x)
        here = 0
        for t in range(targets.size):
            a, _ = V.prune_ip(x, int(targets[t]), pools[t], None, 32, 1.2, pair=pair)
            b, _ = V.prune_ip(x, int(targets[t]), pools[t], None, 32, 1.2, pair=pair, stateless=True)
            here += int(not np.array_equal(a, b))
        print(kind, d, "targets whose stateless list differs:", here, "of", targets.size)
        assert here > 0
        differ += here
        total += targets.size
    assert 2 * differ >= total
