"""CPU tests of the removal entry points (hipann_flat_remove_ids / hipann_ivf_remove_ids).

The IVF kernel does not run FAISS's sequential loop (IndexIVF::remove_ids, DirectMap NoMap):

    j = 0; l = len
    while j < l:
        if member(id[j]): l -= 1; entry[j] = entry[l]
        else: j += 1

It uses the loop's closed form: with L live rows of which r are marked and L' = L − r, the marked positions below L'
(ascending) receive the unmarked positions at or above L' (descending).  ``sequential_remove`` restates the loop,
``closed_form_remove`` the plan the kernel derives; they are held equal here without a GPU, and the GPU tests
(tests/test_remove_ids_gpu.py) compare the device result with ``remove_from_csr`` built on the loop.
"""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]


def sequential_remove(marked: np.ndarray) -> np.ndarray:
    """FAISS's loop over one list; marked[j]: the id at position j is in the selector.  Returns, for every surviving
    position, the ORIGINAL position of the entry that ends up there."""
    src = list(range(len(marked)))
    j, l = 0, len(src)
    while j < l:
        if marked[src[j]]:
            l -= 1
            src[j] = src[l]
        else:
            j += 1
    return np.asarray(src[:l], np.int64)


def closed_form_remove(marked: np.ndarray) -> np.ndarray:
    """The kernel's plan (remove_kernels.hip ivf_remove_rows): holes ascending <- tail survivors descending."""
    marked = np.asarray(marked, bool)
    L = len(marked)
    lp = L - int(marked.sum())
    pos = np.arange(L, dtype=np.int64)
    holes = pos[:lp][marked[:lp]]
    tail = pos[lp:][~marked[lp:]][::-1]
    assert len(holes) == len(tail)
    src = pos.copy()
    src[holes] = tail
    return src[:lp]


def remove_from_csr(off, ids, codes, labels):
    """IndexIVF::remove_ids over ArrayInvertedLists in CSR form (the sequential loop, list by list).  Returns the new
    (offsets, ids, codes)."""
    sel = np.unique(np.asarray(labels, np.int64))
    nlist = len(off) - 1
    new_off = np.zeros(nlist + 1, np.int64)
    keep_rows = []
    for l in range(nlist):
        lo, hi = int(off[l]), int(off[l + 1])
        src = sequential_remove(np.isin(ids[lo:hi], sel))
        keep_rows.append(lo + src)
        new_off[l + 1] = new_off[l] + len(src)
    rows = np.concatenate(keep_rows) if keep_rows else np.zeros(0, np.int64)
    return new_off, np.ascontiguousarray(ids[rows]), np.ascontiguousarray(codes[rows])


def test_closed_form_equals_the_sequential_loop():
    rng = np.random.default_rng(7)
    masks = [np.zeros(0, bool), np.ones(1, bool), np.zeros(1, bool), np.ones(37, bool), np.zeros(37, bool)]
    tail = np.zeros(50, bool)
    tail[-9:] = True          # a marked tail: no move, only a shorter list
    masks.append(tail)
    head = np.zeros(50, bool)
    head[:9] = True
    masks.append(head)
    mixed = np.zeros(64, bool)
    mixed[[0, 5, 60, 62, 63]] = True  # marked rows on both sides of L'
    masks.append(mixed)
    while len(masks) < 200:
        L = int(rng.integers(1, 700))
        masks.append(rng.random(L) < rng.choice([0.02, 0.1, 0.5, 0.9, 0.99]))
    for m in masks:
        a, b = sequential_remove(m), closed_form_remove(m)
        assert np.array_equal(a, b), (m.nonzero()[0], a, b)
        assert len(a) == len(m) - int(m.sum()) and not m[a].any()


def test_remove_symbols_declared_and_exported(hipann_mod):
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hip_ann.h").read_text(), flags=re.S)
    lib = C.CDLL(str(hipann_mod.LIB_PATH))
    for name in ("hipann_flat_remove_ids", "hipann_ivf_remove_ids"):
        assert re.search(r"^int64_t\s+" + name + r"\s*\(void \*index, const int64_t \*labels, int64_t n, "
                         r"char \*err_buf, int err_len\);", hdr, flags=re.M), name
        assert hasattr(lib, name), name
        fn = getattr(hipann_mod.lib(), name)
        assert fn.restype is C.c_int64
    assert callable(hipann_mod.HipIndexFlat.remove_ids) and callable(hipann_mod.HipIndexIVFFlat.remove_ids)


def test_remove_bad_arguments_fail_before_any_device_call(hipann_mod):
    """A NULL handle, n < 0 and NULL labels return -1 with a message, with or without a device (the rule of
    tests/test_abi.py::test_argument_validation_precedes_device)."""
    L = hipann_mod.lib()
    lab = np.arange(4, dtype=np.int64)
    p = lab.ctypes.data_as(C.POINTER(C.c_int64))
    for fn in (L.hipann_flat_remove_ids, L.hipann_ivf_remove_ids):
        for args in ((None, p, 4), (None, p, -1), (None, None, 4), (None, None, 0)):
            eb = C.create_string_buffer(256)
            assert fn(*args, eb, 256) == -1
            assert eb.value, args
        assert fn(None, p, 4, None, 0) == -1  # no error buffer: still -1, no write
