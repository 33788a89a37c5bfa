"""The seeded int8 scan's plan arithmetic (csrc/common.hpp ivf_phase_first / ivf_phase_list / ivf_phase_decode,
ivf_seed_run_slot / ivf_seed_pair_slots — the functions the plan, the scan and ivf_seed_bound use, run here on the host
through hipann_debug_ivf_seed_items / hipann_debug_ivf_seed_slots) against a numpy restatement:

  goff[l]     = Σ_{l' < l} ng(l'),  ng = ceil(cnt / group), the query groups of a list;
  launch 1    = the (list, chunk 0, group) items in list order, list l's at goff[l];
  launch 2    = the (list, chunk >= 1, group) items, list l's at item_off[l] − goff[l], chunk by chunk, groups fastest;
  a query's candidate slots start at slot_off[q·nprobe] + q: one that ends with its seed list, then nch − 1 per pair.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

CH, GROUP_WIDE = 2048, 96
LENS = [0, 1, 2048, 2049, 4096, 4097, 6000, 100, 0, 4097, 2048, 10_000]
CNTS = [0, 1, 96, 97, 192, 193, 250, 288, 0, 5, 289, 96]  # 0 for the empty lists; 1 - 3 groups (and 4 once)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _restate(lens, cnts):
    nch = -(-np.asarray(lens) // CH)
    ng = -(-np.asarray(cnts) // GROUP_WIDE)
    goff = np.concatenate([[0], np.cumsum(ng)])
    item_off = np.concatenate([[0], np.cumsum(ng * nch)])
    a = [(l, 0, g) for l in range(len(lens)) for g in range(ng[l])]
    b = [(l, c, g) for l in range(len(lens)) for c in range(1, nch[l]) for g in range(ng[l])]
    return goff, item_off, np.array(a, np.int32).reshape(-1, 3), np.array(b, np.int32).reshape(-1, 3)


def _device_side(hipann_mod, lens, cnts):
    L = hipann_mod.lib()
    nlist = len(lens)
    ll, cc = np.asarray(lens, np.int32), np.asarray(cnts, np.int32)
    item_off, goff = np.zeros(nlist + 1, np.int32), np.zeros(nlist + 1, np.int32)
    cap = 4096
    a, b = np.full((cap, 3), -1, np.int32), np.full((cap, 3), -1, np.int32)
    rc = L.hipann_debug_ivf_seed_items(_ip(ll), _ip(cc), nlist, GROUP_WIDE << 8, _ip(item_off), _ip(goff), cap, _ip(a),
                                       _ip(b))
    assert rc == 0
    return goff, item_off, a, b


def test_goff_and_item_decode(hipann_mod):
    for lens, cnts in ((LENS, CNTS), (LENS[::-1], CNTS[::-1]), ([0, 0, 5000], [0, 0, 7]), ([2048], [96]), ([1], [1])):
        goff, item_off, a, b = _device_side(hipann_mod, lens, cnts)
        g0, i0, a0, b0 = _restate(lens, cnts)
        assert np.array_equal(goff, g0) and np.array_equal(item_off, i0), (lens, goff, g0)
        assert np.array_equal(a[:len(a0)], a0) and (a[len(a0):] == -1).all(), lens
        assert np.array_equal(b[:len(b0)], b0) and (b[len(b0):] == -1).all(), lens
        # the two launches are the plan's items, each once
        assert len(a0) + len(b0) == i0[-1] and len(a0) == g0[-1]


def test_candidate_slots(hipann_mod):
    L = hipann_mod.lib()
    rng = np.random.default_rng(3)
    for nprobe, nq in ((4, 7), (32, 5), (1, 9)):
        nch = rng.choice([0, 0, 1, 1, 2, 3, 5], size=nq * nprobe)  # 0: an empty list, or one on another shard
        slot_off = np.concatenate([[0], np.cumsum(nch)]).astype(np.int32)
        cslot, bcnt = np.zeros(nq * nprobe, np.int64), np.zeros(nq, np.int32)
        L.hipann_debug_ivf_seed_slots(_ip(slot_off), nprobe, C.c_int64(nq), cslot.ctypes.data_as(C.POINTER(C.c_int64)),
                                      _ip(bcnt))
        used = set()
        for q in range(nq):
            first = int(slot_off[q * nprobe]) + q
            slots = np.maximum(nch[q * nprobe:(q + 1) * nprobe] - 1, 0)
            want = first + 1 + np.concatenate([[0], np.cumsum(slots)[:-1]])
            assert np.array_equal(cslot[q * nprobe:(q + 1) * nprobe], want), (q, cslot, want)
            assert bcnt[q] == slots.sum()
            mine = set(range(first, first + 1 + int(slots.sum())))
            assert not (mine & used)  # the queries' runs are disjoint
            used |= mine
        # every run lies inside the scan's buffer of Σ nch + nq slots
        assert max(used) < int(slot_off[-1]) + nq
