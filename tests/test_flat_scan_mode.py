"""The Flat scan mode (csrc/hip_ann.cpp flat_resolve_mode; DESIGN.md §5 "Flat scan modes") against a hand-written
table.  hipann_debug_flat_scan_mode runs the resolver on the host, with no device.

Where the expected values come from:

  * common.hpp: kRerankK 16 (the 2-term split's L2 filter), kFlatRerankKIP 32 (its IP filter and the bf16 image's),
    kRerankMaxK 12 (the last kout with the base filter; above it kf = min(64, max(base, 2 kout))).
  * hip_ann.cpp: BLAS threshold 20 queries, small table 16384 rows, fused lists k <= 64, seed bound and bounded passes
    from 8 * 65536 = 524288 rows, the small-batch int8 scan from 65536 rows for nq <= 16, d <= 1024, k <= 64.
  * the direct scan holds nq * roundup4(d) floats in 64 KiB of LDS: d = 1536 fits 10 queries (61440 B), not 11 (67584 B).
  * the bf16 list kernel's LDS (160 KiB): 3 stages of (QM + 256) * 64 B plus QM * k * 8 B of lists, QM = 32 queries per
    wave.  8 waves (nq >= 256): 98304 + 2048 k <= 163840, kmax 32.  4 waves (nq >= 128) and 2 waves: kmax 64.
  * the split GEMM lists' LDS: 2 * terms * 8192 B of stages plus 2048 k B of lists at 8 waves.  2 terms: 32768 +
    2048 k <= 163840 at k = 64, kmax 64.  3 terms: 49152 + 2048 k <= 163840, kmax 56.
  * the bounded passes need 8 waves and an even number of 32-dim chunks (d = 64: 2; d = 96: 3; d = 1025: 33; d = 1088: 34)
    and take any kf <= 64; the int8 form runs only as bounded passes with d <= 1024 and filters 64 deep.
  * exact: kout <= 12, or kout <= kf on the bounded passes, or kout + 4 <= kf on the list kernels; an exact form that
    is not exact at this kout runs the 3-term split, and a 3-term or 2-term list longer than its kmax the fp32 GEMM.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

FP32, S3, S2, S2X, B16X, I8X = range(6)
L2, IP = 0, 1
NONE, PADS, KEYS, SMALL_I8, DIRECT, LISTS, BOUNDED = range(7)
P_NONE, P_SMALL_I8, P_EXACT = range(3)
OUT = ("path", "form", "record", "last_form", "last_kfilt", "exact", "bounded", "seeded", "i8", "i8_prep", "kscan",
       "k_user", "pend_kind", "rerun_form", "need_qn", "prep_qn")
BIG = 8 * 65536


def resolve(hipann_mod, nq=256, n=BIG, d=64, metric=L2, k=10, kout=None, form=I8X, override=0, i8_small=1, seed=1,
            prep_fused=1, b16_k64=1):
    kout = k if kout is None else kout
    a = np.array([nq, n, d, metric, k, kout, form, override, i8_small, seed, prep_fused, b16_k64], np.int32)
    o = np.full(len(OUT), -7, np.int32)
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
    assert hipann_mod.lib().hipann_debug_flat_scan_mode(ip(a), len(a), ip(o), len(o)) == 0
    return dict(zip(OUT, (int(v) for v in o)))


def check(got, want, what):
    bad = {f: (got[f], v) for f, v in want.items() if got[f] != v}
    assert not bad, f"{what}: (got, want) {bad}"


def keys(k=10, need_qn=0):
    """The key-matrix path: nothing recorded, nothing pending."""
    return dict(path=KEYS, record=0, exact=0, bounded=0, seeded=0, i8=0, kscan=k, k_user=k, pend_kind=P_NONE,
                need_qn=need_qn, prep_qn=0)


def direct(k=10):
    return dict(path=DIRECT, record=1, last_form=FP32, last_kfilt=0, exact=0, bounded=0, seeded=0, i8=0, kscan=k,
                k_user=k, pend_kind=P_NONE, need_qn=0, prep_qn=0)


def small_i8(k=10, need_qn=1):
    return dict(path=SMALL_I8, form=I8X, record=1, last_form=I8X, last_kfilt=64, exact=1, bounded=0, i8=1, kscan=64,
                k_user=k, pend_kind=P_SMALL_I8, rerun_form=FP32, need_qn=need_qn, prep_qn=0)


def lists(form, k=10, kf=0, seeded=0, need_qn=1):
    """Per-split lists; kf > 0: an exact form's filter depth."""
    return dict(path=LISTS, form=form, record=1, last_form=form, last_kfilt=kf, exact=int(kf > 0), bounded=0,
                seeded=seeded, i8=0, i8_prep=0, kscan=kf or k, k_user=k, pend_kind=P_EXACT if kf else P_NONE,
                need_qn=need_qn, prep_qn=0, **(dict(rerun_form=S3) if kf else {}))


def bounded(form, kf, k=10, need_qn=1, prep=1):
    i8 = int(form == I8X)
    return dict(path=BOUNDED, form=form, record=1, last_form=form, last_kfilt=kf, exact=1, bounded=1, seeded=1, i8=i8,
                i8_prep=i8 & prep, kscan=kf, k_user=k, pend_kind=P_EXACT, rerun_form=S3, need_qn=need_qn,
                prep_qn=i8 & prep & need_qn)


# ---- every requested form at a BLAS shape: 256 queries, 524288 rows, d = 64, kout = 10 ----
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("form", range(6))
def test_every_form(hipann_mod, form, metric):
    l2 = int(metric == L2)
    want = {FP32: lists(FP32, need_qn=l2), S3: lists(S3, need_qn=l2), S2: lists(S2, need_qn=l2),
            S2X: lists(S2X, kf=16 if l2 else 32, need_qn=l2),  # the split scan's filter: L2 16, IP 32
            B16X: bounded(B16X, 32, need_qn=l2), I8X: bounded(I8X, 64, need_qn=l2)}[form]
    check(resolve(hipann_mod, form=form, metric=metric), want, (form, metric))


# ---- the key-matrix path ----
@pytest.mark.parametrize("kw,want", [
    (dict(k=64), bounded(I8X, 64, k=64)),
    (dict(k=65), keys(65, need_qn=1)),
    (dict(k=65, metric=IP), keys(65)),
    (dict(k=65, nq=4), keys(65)),            # below the BLAS threshold the keys come from the direct form: no ‖q‖²
    # a table of <= 1024 rows at nq < 20, of <= 16384 rows from 20 queries on
    (dict(nq=19, n=1024), keys()),
    (dict(nq=19, n=1025), direct()),
    (dict(nq=20, n=1024), keys(need_qn=1)),
    (dict(nq=20, n=1025), keys(need_qn=1)),
    (dict(nq=19, n=16384), direct()),
    (dict(nq=20, n=16384), keys(need_qn=1)),
    (dict(nq=19, n=16385), direct()),
    (dict(nq=20, n=16385), lists(B16X, kf=32)),  # 2 waves: no bounded passes, the list kernel holds 64
    # the per-row select writes kout <= 64
    (dict(nq=1, n=1024, k=10, kout=64), keys()),
    (dict(nq=1, n=1024, k=10, kout=65), direct()),
    # the direct-form keys hold their queries in 64 KiB of LDS
    (dict(nq=10, n=1024, d=1536), keys()),
    (dict(nq=11, n=1024, d=1536), direct()),
])
def test_keys_path_edges(hipann_mod, kw, want):
    check(resolve(hipann_mod, **kw), want, kw)


# ---- the small-batch int8 scan ----
@pytest.mark.parametrize("kw,want", [
    (dict(nq=16), small_i8()),
    (dict(nq=17), direct()),
    (dict(nq=1, metric=IP), small_i8(need_qn=0)),
    (dict(nq=16, n=65535), direct()),
    (dict(nq=16, d=1024), small_i8()),
    (dict(nq=16, d=1025), direct()),
    (dict(nq=16, form=B16X), direct()),
    (dict(nq=16, i8_small=0), direct()),
    (dict(nq=16, k=64), small_i8(k=64)),
    (dict(nq=16, k=65), keys(65)),
])
def test_small_int8_edges(hipann_mod, kw, want):
    kw = dict(dict(n=65536), **kw)
    check(resolve(hipann_mod, **kw), want, kw)


# ---- the bounded passes: 8 waves, >= 524288 rows, an even chunk count, the seed switch ----
@pytest.mark.parametrize("kw,want", [
    (dict(nq=255), lists(B16X, kf=32, seeded=1)),          # 4 waves: the bf16 list kernel, seeded
    (dict(nq=256), bounded(I8X, 64)),
    (dict(nq=255, form=B16X), lists(B16X, kf=32, seeded=1)),
    (dict(n=BIG - 1), lists(B16X, kf=32)),                 # no seed below 524288 rows
    (dict(n=BIG - 1, form=B16X), lists(B16X, kf=32)),
    (dict(d=1024), bounded(I8X, 64)),
    (dict(d=1025), lists(B16X, kf=32, seeded=1)),          # 33 chunks
    (dict(d=1088), bounded(B16X, 32)),                     # 34 chunks: bounded, but d > 1024 leaves the int8 image
    (dict(d=96), lists(B16X, kf=32, seeded=1)),            # 3 chunks
    (dict(d=96, form=B16X), lists(B16X, kf=32, seeded=1)),
    (dict(seed=0), lists(B16X, kf=32)),
    (dict(seed=0, form=B16X), lists(B16X, kf=32)),
    (dict(b16_k64=0), lists(B16X, kf=32, seeded=1)),
    (dict(prep_fused=0), bounded(I8X, 64, prep=0)),
    (dict(metric=IP), bounded(I8X, 64, need_qn=0)),
])
def test_bounded_edges(hipann_mod, kw, want):
    check(resolve(hipann_mod, **kw), want, kw)


# ---- the filter depth and what an exact form falls to ----
@pytest.mark.parametrize("kw,want", [
    # kRerankMaxK on the 2-term split (kmax 64 never caps it)
    (dict(form=S2X, k=12), lists(S2X, k=12, kf=16)),
    (dict(form=S2X, k=13), lists(S2X, k=13, kf=26)),
    (dict(form=S2X, k=13, metric=IP), lists(S2X, k=13, kf=32, need_qn=0)),
    (dict(form=S2X, k=30), lists(S2X, k=30, kf=60)),
    (dict(form=S2X, k=60), lists(S2X, k=60, kf=64)),       # 60 + 4 <= 64
    (dict(form=S2X, k=61), lists(FP32, k=61)),             # not exact: 3 terms, whose lists hold 56: fp32
    # the unbounded bf16 lists at 8 waves hold 32: kout + 4 <= 32
    (dict(form=B16X, n=BIG - 1, k=12), lists(B16X, k=12, kf=32)),
    (dict(form=B16X, n=BIG - 1, k=13), lists(B16X, k=13, kf=32)),
    (dict(form=B16X, n=BIG - 1, k=28), lists(B16X, k=28, kf=32)),
    (dict(form=B16X, n=BIG - 1, k=29), lists(S3, k=29)),
    (dict(form=I8X, n=BIG - 1, k=28), lists(B16X, k=28, kf=32)),
    (dict(form=I8X, n=BIG - 1, k=29), lists(S3, k=29)),
    (dict(form=B16X, n=BIG - 1, k=56), lists(S3, k=56)),
    (dict(form=B16X, n=BIG - 1, k=57), lists(FP32, k=57)),
    # at 4 waves they hold 64
    (dict(form=B16X, nq=255, k=29), lists(B16X, k=29, kf=58, seeded=1)),
    (dict(form=B16X, nq=255, k=60), lists(B16X, k=60, kf=64, seeded=1)),
    (dict(form=B16X, nq=255, k=61), lists(FP32, k=61)),
    # the bounded passes take any kout <= kf
    (dict(form=B16X, k=12), bounded(B16X, 32, k=12)),
    (dict(form=B16X, k=13), bounded(B16X, 32, k=13)),
    (dict(form=B16X, k=32), bounded(B16X, 64, k=32)),
    (dict(form=B16X, k=33), bounded(B16X, 64, k=33)),
    (dict(form=B16X, k=64), bounded(B16X, 64, k=64)),
    (dict(form=I8X, k=13), bounded(I8X, 64, k=13)),
    (dict(form=I8X, k=33), bounded(I8X, 64, k=33)),
    (dict(form=I8X, k=64), bounded(I8X, 64, k=64)),
    (dict(form=B16X, k=10, kout=65), lists(S3, k=10)),     # (kout > kf: only through the hook; a search has k > 64 then)
    # the plain split forms past their lists
    (dict(form=S3, k=56), lists(S3, k=56)),
    (dict(form=S3, k=57), lists(FP32, k=57)),
    (dict(form=S2, k=64), lists(S2, k=64)),
])
def test_filter_depth_edges(hipann_mod, kw, want):
    check(resolve(hipann_mod, **kw), want, kw)


def test_list_limits_relate_as_documented(hipann_mod):
    """The launchers' list limits only through what the resolver does with them: the 8-wave bf16 lists cap the filter
    at 32 <= the 4-wave lists' and the bounded passes' 64 = the 2-term lists' limit, above the 3-term lists' 56."""
    cap8 = resolve(hipann_mod, form=B16X, n=BIG - 1, k=20)["kscan"]   # min(40, kmax(8 waves))
    cap4 = resolve(hipann_mod, form=B16X, nq=255, k=40)["kscan"]      # min(64, kmax(4 waves))
    capb = resolve(hipann_mod, form=B16X, k=40)["kscan"]
    cap2 = resolve(hipann_mod, form=S2X, k=40)["kscan"]
    assert cap8 == 32 and cap8 <= cap4 == capb == cap2 == 64
    assert resolve(hipann_mod, form=S3, k=56)["form"] == S3 and resolve(hipann_mod, form=S3, k=57)["form"] == FP32


@pytest.mark.parametrize("kw", [dict(), dict(form=S2X), dict(form=S3), dict(nq=4, n=65536), dict(nq=4, n=2048)])
def test_override_call_does_not_record(hipann_mod, kw):
    a, b = resolve(hipann_mod, **kw), resolve(hipann_mod, override=1, **kw)
    assert a["record"] == 1 and b["record"] == 0
    assert {f: v for f, v in a.items() if f != "record"} == {f: v for f, v in b.items() if f != "record"}


def test_keys_path_never_records(hipann_mod):
    for kw in (dict(k=65), dict(nq=32, n=1024), dict(nq=1, n=1024)):
        assert resolve(hipann_mod, **kw)["record"] == 0 and resolve(hipann_mod, override=1, **kw)["record"] == 0


def test_empty_batch_and_empty_table(hipann_mod):
    check(resolve(hipann_mod, nq=0), dict(path=NONE, record=0, pend_kind=P_NONE, need_qn=0), "nq 0")
    check(resolve(hipann_mod, nq=0, n=0), dict(path=NONE, record=0), "nq 0, n 0")
    check(resolve(hipann_mod, n=0), dict(path=PADS, record=0, pend_kind=P_NONE, need_qn=0), "n 0")
    check(resolve(hipann_mod, n=0, k=65), dict(path=PADS, record=0), "n 0, k 65")


def test_every_exact_outcome_names_its_rerun(hipann_mod):
    """Pending kind and re-run form: the small-batch int8 scan re-runs on the fp32 direct scan (form 0 at nq < 20), the
    batched exact forms on the 3-term split; every other path leaves nothing pending."""
    seen = set()
    for form in range(6):
        for metric in (L2, IP):
            for nq, n in ((4, 65536), (4, 2048), (32, 20000), (64, 20000), (256, BIG), (256, BIG - 1), (32, 1024)):
                for k in (10, 13, 40, 64):
                    m = resolve(hipann_mod, nq=nq, n=n, k=k, form=form, metric=metric)
                    want = ((P_SMALL_I8, FP32) if m["path"] == SMALL_I8 else (P_EXACT, S3) if m["exact"] else
                            (P_NONE, m["rerun_form"]))
                    assert (m["pend_kind"], m["rerun_form"]) == want, (form, metric, nq, n, k, m)
                    assert m["exact"] == int(m["last_kfilt"] > 0) or m["path"] == KEYS
                    seen.add((m["path"], m["form"], m["exact"]))
    assert {(SMALL_I8, I8X, 1), (LISTS, S2X, 1), (LISTS, B16X, 1), (BOUNDED, B16X, 1), (BOUNDED, I8X, 1)} <= seen


def test_hook_rejects_bad_arguments(hipann_mod):
    L = hipann_mod.lib()
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
    good = np.array([256, BIG, 64, L2, 10, 10, I8X, 0, 1, 1, 1, 1], np.int32)
    o = np.zeros(len(OUT), np.int32)
    assert L.hipann_debug_flat_scan_mode(ip(good), 12, ip(o), 16) == 0
    assert L.hipann_debug_flat_scan_mode(ip(good), 11, ip(o), 16) == -1
    assert L.hipann_debug_flat_scan_mode(ip(good), 12, ip(o), 15) == -1
    for idx, v in ((0, -1), (1, -1), (2, 0), (3, 2), (4, 0), (5, 0), (6, -1), (6, 6)):
        bad = good.copy()
        bad[idx] = v
        assert L.hipann_debug_flat_scan_mode(ip(bad), 12, ip(o), 16) == -1, (idx, v)
