"""IVF SQ8 C ABI without a device: the library exports the six hipann_ivfsq_* symbols with the header's argument
counts, and the Python class exists."""
from __future__ import annotations

import re
from pathlib import Path

HEADER = Path(__file__).resolve().parents[1] / "include" / "hip_ann.h"
SYMBOLS = ("create", "search", "search_device", "last_probes", "export", "rerank_fallbacks")


def test_ivfsq_symbols_match_header(hipann_mod):
    text = HEADER.read_text()
    L = hipann_mod.lib()
    for s in SYMBOLS:
        m = re.search(r"\bhipann_ivfsq_%s\(([^)]*)\)" % s, text)
        assert m, s
        fn = getattr(L, "hipann_ivfsq_" + s)
        assert len(fn.argtypes) == len(m.group(1).split(",")), s
    assert hasattr(hipann_mod, "HipIndexIVFSQ8")
