"""What a real IVF search reports about its scan (hipann_last_search_path, hipann_ivf_last_seeded,
hipann_ivf_last_filter_image, hipann_debug_ivf_info) equals what the host-only resolver hook returns for the same
inputs (tests/test_ivf_scan_mode.py checks the hook against a hand-written table).  One tiny layout: d = 64, four lists
of 0 / 1 / 2048 / 2049 rows (two row chunks), fresh per case, so every image starts unbuilt and auto starts untested.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

from test_ivf_scan_mode import OUT

pytestmark = pytest.mark.gpu

D_, LENS = 64, [0, 1, 2048, 2049]
L2, IP = 0, 1


@pytest.fixture(scope="module")
def layout():
    rng = np.random.default_rng(11)
    cen = rng.standard_normal((len(LENS), D_)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    codes = np.concatenate([cen[l] + 0.3 * rng.standard_normal((n, D_)).astype(np.float32) for l, n in enumerate(LENS)])
    ids = np.arange(off[-1], dtype=np.int64)
    Q = (cen[rng.integers(0, len(LENS), 65)] + 0.3 * rng.standard_normal((65, D_))).astype(np.float32)
    return cen, off, ids, np.ascontiguousarray(codes, np.float32), Q


def _info(lib, ix, name):
    f = lib.hipann_debug_ivf_info
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
    v = C.c_double()
    assert f(ix.handle, name.encode(), C.byref(v)) == 0, name
    return int(v.value)


# form, metric, filter image, nq, kout, nprobe
CASES = [
    (6, L2, 0, 64, 10, 4),   # the fp16 image
    (6, L2, 1, 1, 10, 2),    # the fp16 form on the int8 image (seeded: two chunks)
    (6, L2, 2, 64, 12, 4),   # auto, untested: answered on the fp16 image, probation behind it
    (6, L2, 2, 63, 12, 4),   # auto below its batch threshold
    (6, L2, 1, 65, 13, 4),   # kout 13 never takes the filter image: fp16 sub-lists
    (6, IP, 1, 64, 10, 4),   # nor does IP
    (7, L2, 0, 65, 60, 4),   # int8, the last sub-list width, seeded
    (7, IP, 0, 63, 10, 2),   # int8, IP: no certificate, no seed
    (7, L2, 0, 64, 61, 4),   # beyond the sub-lists, k > 16: the VALU kernel
    (5, L2, 0, 64, 13, 4),   # 2-term scan with sub-lists
    (5, IP, 0, 1, 12, 2),
    (6, L2, 0, 1, 65, 4),    # k > 64
    (0, L2, 0, 63, 10, 2), (1, IP, 0, 64, 10, 4), (2, L2, 0, 65, 10, 4), (3, L2, 0, 63, 10, 2), (4, IP, 0, 1, 10, 4),
]


@pytest.mark.parametrize("form,metric,fimg,nq,kout,nprobe", CASES)
def test_reported_mode_is_the_resolved_mode(gpu, layout, form, metric, fimg, nq, kout, nprobe):
    cen, off, ids, codes, Q = layout
    lib = gpu.lib()
    ix = gpu.HipIndexIVFFlat(cen, off, ids, codes, nprobe, metric)
    ix.form, ix.filter_image = form, fimg
    env = lambda name, dflt: int(os.environ.get(name) or dflt)
    fmode = env("HIPANN_IVF_FILTER_IMAGE", -1)
    a = np.array([form, 0, metric, D_, kout, kout, min(nprobe, len(LENS)), _info(lib, ix, "max_nch"), 3,
                  env("HIPANN_IVF_HOST_FALLBACK", 0) != 0, env("HIPANN_IVF_SEED", 1) != 0, 3,
                  fmode if 0 <= fmode <= 2 else fimg, nq, _info(lib, ix, "n"), _info(lib, ix, "i8_state"), 0], np.int32)
    o = np.zeros(len(OUT), np.int32)
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.hipann_debug_ivf_scan_mode(ip(a), len(a), ip(o), len(o)) == 0
    m = dict(zip(OUT, (int(v) for v in o)))
    assert _info(lib, ix, "max_nch") == 2

    ix.search(Q[:nq], kout)
    path = ix.last_search_path(seeded=True)
    got = dict(form=path["form"], filter_k=path["filter_k"], sublists=path["sublists"], seeded=path["seeded"],
               filter_image=ix.last_filter_image(),
               **{s: _info(lib, ix, s) for s in ("kslot", "kfilt", "sub", "image", "group", "cand_off", "nq", "nprobe")},
               dbg_seeded=_info(lib, ix, "seeded"))
    want = dict(form=m["last_form"], filter_k=m["kfilt"] if m["exact"] else 0,
                sublists=m["kslot"] // m["kscan"] if m["sub"] else 0, seeded=m["seeded"],
                filter_image=int(m["exact"] and m["image"] == 2), kslot=m["kslot"],
                kfilt=m["kfilt"] if m["exact"] else 0, sub=m["sub"], image=m["image"],
                group=m["group"] if m["image"] else 0,  # (the info hook reports the image scans' group only)
                cand_off=int(a[6]) * nq * m["kslot"] if m["seeded"] else -1, nq=nq, nprobe=int(a[6]), dbg_seeded=m["seeded"])
    assert got == want, (got, want, m)
    # the images the resolver asked for are the images the search built, and no other
    assert (_info(lib, ix, "half_state") == 1) == bool(m["asked"] & 1)
    built_i8 = bool(m["asked"] & 2) or bool(m["probation"])  # probation builds the int8 image for its counting pass
    assert (_info(lib, ix, "i8_state") == 1) == built_i8
    ix.close()
