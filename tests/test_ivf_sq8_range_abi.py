"""IVF SQ8 range search C ABI without a device: the library exports both symbols with the header's argument counts,
and the Python methods exist."""
from __future__ import annotations

import re
from pathlib import Path

HEADER = Path(__file__).resolve().parents[1] / "include" / "hip_ann.h"


def test_ivfsq_range_symbols_match_header(hipann_mod):
    text = HEADER.read_text()
    L = hipann_mod.lib()
    for s in ("range_search", "range_search_device"):
        m = re.search(r"\bhipann_ivfsq_%s\(([^)]*)\)" % s, text)
        assert m, s
        fn = getattr(L, "hipann_ivfsq_" + s)
        assert len(fn.argtypes) == len(m.group(1).split(",")), s
    assert callable(hipann_mod.HipIndexIVFSQ8.range_search) and callable(hipann_mod.HipIndexIVFSQ8.range_search_device)
