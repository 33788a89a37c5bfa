"""The IVF scan mode (csrc/ivf.cpp ivf_resolve_mode, ivf_filter_image_eligible, ivf_choose_filter_image; DESIGN.md §5
"Scan modes") against a hand-written table.  hipann_debug_ivf_scan_mode runs the resolver on the host, with no device:
its inputs say which tiled images "build", its outputs which were asked for.

The expected values are worked out from common.hpp (kRerankK 16, kRerankMaxK 12, kIvfSubMaxK 60, kSeedK 64), eight scan
waves (sub-list slots of 8 × 16 entries), and the group sizes of d = 64: 48 for the fp32 matrix-core scans, 64 for the
VALU kernel, 32 for the direct kernel, 96 wide (packed 96 << 8) for the fp16 and int8 images.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

DEC, DIRECT, VALU, S3, S2, S2X, HALFX, I8X = range(8)
L2, IP = 0, 1
WIDE = 96 << 8
OUT = ("form", "last_form", "exact", "image", "sub", "kscan", "kslot", "kfilt", "seeded", "tiled", "cert8", "group",
       "bigk", "asked", "eligible", "taken", "probation")


def resolve(hipann_mod, form, metric=L2, d=64, k=10, kout=None, np_=4, max_nch=2, align=3, override=0, host_fb=0,
            seed=1, build=3, fmode=0, nq=64, nrows=1000, i8_state=0, auto8=0):
    kout = k if kout is None else kout
    a = np.array([form, override, metric, d, k, kout, np_, max_nch, align, host_fb, seed, build, fmode, nq, nrows,
                  i8_state, auto8], np.int32)
    o = np.full(len(OUT), -7, np.int32)
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
    assert hipann_mod.lib().hipann_debug_ivf_scan_mode(ip(a), len(a), ip(o), len(o)) == 0
    return dict(zip(OUT, (int(v) for v in o)))


def mode(form, last_form, exact, image, sub, kscan, kslot, kfilt, tiled, group, seeded=0, cert8=0, bigk=0, asked=0):
    return dict(form=form, last_form=last_form, exact=exact, image=image, sub=sub, kscan=kscan, kslot=kslot, kfilt=kfilt,
                seeded=seeded, tiled=tiled, cert8=cert8, group=group, bigk=bigk, asked=asked)


def check(got, want, what):
    bad = {f: (got[f], v) for f, v in want.items() if got[f] != v}
    assert not bad, f"{what}: (got, want) {bad}"


# requested form -> mode at d = 64, k = kout = 10, nprobe 4, two chunks, both images building
PLAIN = {
    DEC: mode(DEC, DEC, 0, 0, 0, 10, 10, 10, 1, 48),
    DIRECT: mode(DIRECT, DIRECT, 0, 0, 0, 10, 10, 10, 0, 32),
    VALU: mode(VALU, VALU, 0, 0, 0, 10, 10, 10, 0, 64),
    S3: mode(S3, S3, 0, 0, 0, 10, 10, 10, 1, 48),
    S2: mode(S2, S2, 0, 0, 0, 10, 10, 10, 1, 48),
    S2X: mode(S2, S2X, 1, 0, 0, 16, 16, 16, 1, 48),
    HALFX: mode(S2, HALFX, 1, 1, 0, 16, 16, 16, 1, WIDE, asked=1),
}


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("form", range(8))
def test_every_form(hipann_mod, form, metric):
    if form == I8X:  # sub-lists always, the 64-deep filter; the per-row certificate and the seed are L2's
        l2 = int(metric == L2)
        want = mode(S2, I8X, 1, 2, 1, 16, 128, 64, 1, WIDE, seeded=l2, cert8=l2, asked=2)
    else:
        want = PLAIN[form]
    check(resolve(hipann_mod, form, metric), want, (form, metric))


@pytest.mark.parametrize("form,k,kout,want", [
    # kRerankMaxK: 12 keeps the 16-entry slots, 13 takes the sub-lists (filter depth max(kout + 4, 2 kout))
    (HALFX, 12, 12, mode(S2, HALFX, 1, 1, 0, 16, 16, 16, 1, WIDE, asked=1)),
    (HALFX, 13, 13, mode(S2, HALFX, 1, 1, 1, 16, 128, 26, 1, WIDE, asked=1)),
    (S2X, 12, 12, mode(S2, S2X, 1, 0, 0, 16, 16, 16, 1, 48)),
    (S2X, 13, 13, mode(S2, S2X, 1, 0, 1, 16, 128, 26, 1, 48)),
    (I8X, 13, 13, mode(S2, I8X, 1, 2, 1, 16, 128, 64, 1, WIDE, seeded=1, cert8=1, asked=2)),
    # kIvfSubMaxK: 60 is the last sub-list request; 61 asks for no image and takes the 3-term scan, whose 16-lane lists
    # hold k <= 16 (k = 61: the VALU kernel)
    (HALFX, 60, 60, mode(S2, HALFX, 1, 1, 1, 16, 128, 64, 1, WIDE, asked=1)),
    (HALFX, 61, 61, mode(VALU, VALU, 0, 0, 0, 61, 61, 61, 0, 64)),
    (HALFX, 10, 61, mode(S3, S3, 0, 0, 0, 10, 10, 10, 1, 48)),
    (I8X, 60, 60, mode(S2, I8X, 1, 2, 1, 16, 128, 64, 1, WIDE, seeded=1, cert8=1, asked=2)),
    (I8X, 61, 61, mode(VALU, VALU, 0, 0, 0, 61, 61, 61, 0, 64)),
    (S2X, 61, 61, mode(VALU, VALU, 0, 0, 0, 61, 61, 61, 0, 64)),
    # k > 64: the per-slot direct scan
    (HALFX, 64, 64, mode(VALU, VALU, 0, 0, 0, 64, 64, 64, 0, 64)),
    (HALFX, 65, 65, mode(DIRECT, DIRECT, 0, 0, 0, 65, 65, 65, 0, 32, bigk=1)),
    (I8X, 65, 65, mode(DIRECT, DIRECT, 0, 0, 0, 65, 65, 65, 0, 32, bigk=1)),
    (DEC, 65, 65, mode(DIRECT, DIRECT, 0, 0, 0, 65, 65, 65, 0, 32, bigk=1)),
    # the filter depth: min(64, max(kout + 4, 2 kout)) on fp16 sub-lists, 64 on int8, the scan's 16 without sub-lists
    (HALFX, 5, 10, mode(S2, HALFX, 1, 1, 0, 16, 16, 16, 1, WIDE, asked=1)),
    (HALFX, 5, 13, mode(S2, HALFX, 1, 1, 1, 16, 128, 26, 1, WIDE, asked=1)),
    (HALFX, 30, 30, mode(S2, HALFX, 1, 1, 1, 16, 128, 60, 1, WIDE, asked=1)),
    (I8X, 5, 10, mode(S2, I8X, 1, 2, 1, 16, 128, 64, 1, WIDE, seeded=1, cert8=1, asked=2)),
    (I8X, 30, 30, mode(S2, I8X, 1, 2, 1, 16, 128, 64, 1, WIDE, seeded=1, cert8=1, asked=2)),
])
def test_kout_edges_and_filter_depth(hipann_mod, form, k, kout, want):
    got = resolve(hipann_mod, form, k=k, kout=kout)
    check(got, want, (form, k, kout))
    if got["sub"]:
        assert got["kfilt"] == (64 if got["image"] == 2 else min(64, max(kout + 4, 2 * kout)))


def test_alignment_and_dimension(hipann_mod):
    # d = 6 (no float4 rows) and a query or code pointer off 16 bytes: the direct kernel (form 5 keeps its 16-deep scan)
    for kw in (dict(d=6), dict(align=2), dict(align=1), dict(align=0)):
        check(resolve(hipann_mod, S2X, **kw), mode(DIRECT, DIRECT, 0, 0, 0, 16, 16, 16, 0, 32), kw)
        for form in (DEC, VALU, S3, S2):
            check(resolve(hipann_mod, form, **kw), mode(DIRECT, DIRECT, 0, 0, 0, 10, 10, 10, 0, 32), (form, kw))
    # the images are zero-padded to whole super-steps and read their own aligned copies: any d, any pointer
    for kw in (dict(d=6), dict(d=67), dict(align=0)):
        got = resolve(hipann_mod, HALFX, **kw)
        check(got, dict(form=S2, last_form=HALFX, exact=1, image=1, asked=1, tiled=1), kw)
        got = resolve(hipann_mod, I8X, **kw)
        check(got, dict(form=S2, last_form=I8X, exact=1, image=2, asked=2, sub=1, kslot=128, kfilt=64, seeded=1), kw)


def test_seeding(hipann_mod):
    on = dict(image=2, sub=1, cert8=1, seeded=1)
    check(resolve(hipann_mod, I8X), on, "int8, L2, sub-lists, two chunks")
    check(resolve(hipann_mod, I8X, np_=32), on, "32 probes x 128 entries: the seed select's 4096")
    check(resolve(hipann_mod, I8X, np_=33), dict(on, seeded=0), "33 probes: too many chunk-0 entries")
    check(resolve(hipann_mod, I8X, max_nch=1), dict(on, seeded=0), "one chunk")
    check(resolve(hipann_mod, I8X, seed=0), dict(on, seeded=0), "the switch")
    check(resolve(hipann_mod, I8X, metric=IP), dict(on, cert8=0, seeded=0), "IP")
    check(resolve(hipann_mod, HALFX, k=13), dict(image=1, sub=1, cert8=0, seeded=0), "the fp16 image")
    check(resolve(hipann_mod, HALFX, fmode=1), dict(on, last_form=HALFX), "the fp16 form on the int8 image")


def test_failed_image_builds(hipann_mod):
    # a build that reports a non-finite row: kFormSplit2Exact's path, after exactly one request
    check(resolve(hipann_mod, HALFX, build=2), dict(PLAIN[S2X], asked=1), "fp16 image fails")
    check(resolve(hipann_mod, HALFX, build=0), dict(PLAIN[S2X], asked=1), "both would fail")
    # (form 7's sub-list request stands: the 2-term scan writes sub-lists, the filter depth is the fp16 rule's)
    check(resolve(hipann_mod, I8X, build=1), mode(S2, S2X, 1, 0, 1, 16, 128, 20, 1, 48, asked=2), "int8 image fails")
    # the fp16 form on a failing int8 filter image goes back to its own image
    check(resolve(hipann_mod, HALFX, fmode=1, build=1), dict(PLAIN[HALFX], asked=3, taken=0), "filter image fails")
    # an image is not asked for unless everything else holds
    for kw in (dict(k=61), dict(k=65)):
        assert resolve(hipann_mod, HALFX, **kw)["asked"] == 0 and resolve(hipann_mod, I8X, **kw)["asked"] == 0
    for form in (DEC, DIRECT, VALU, S3, S2, S2X):
        assert resolve(hipann_mod, form)["asked"] == 0


def test_filter_image(hipann_mod):
    int8 = mode(S2, HALFX, 1, 2, 1, 16, 128, 64, 1, WIDE, seeded=1, cert8=1, asked=2)
    fp16 = PLAIN[HALFX]
    r = lambda **kw: resolve(hipann_mod, HALFX, **kw)
    check(r(fmode=0), dict(fp16, eligible=1, taken=0, probation=0), "mode 0")
    check(r(fmode=1), dict(int8, eligible=1, taken=1, probation=0), "mode 1")
    check(r(fmode=1, nq=1), dict(int8, taken=1), "mode 1 has no batch threshold")
    check(r(fmode=2, auto8=0), dict(fp16, eligible=1, taken=0, probation=1), "auto, untested: probation")
    check(r(fmode=2, auto8=1), dict(int8, taken=1, probation=0), "auto, on")
    check(r(fmode=2, auto8=-1), dict(fp16, taken=0, probation=0), "auto, off")
    check(r(fmode=2, auto8=1, nq=63), dict(fp16, eligible=1, taken=0, probation=0), "auto below 64 queries")
    check(r(fmode=2, auto8=0, nq=63), dict(fp16, taken=0, probation=0), "no probation below 64 queries")
    never = dict(eligible=0, taken=0, probation=0, image=1, asked=1, last_form=HALFX)
    for fmode, auto8 in ((1, 0), (2, 0), (2, 1)):
        check(r(fmode=fmode, auto8=auto8, override=1), never, "an override")
        check(r(fmode=fmode, auto8=auto8, metric=IP), never, "IP")
        check(r(fmode=fmode, auto8=auto8, k=13), dict(never, sub=1, kfilt=26), "kout = 13")
        check(r(fmode=fmode, auto8=auto8, host_fb=1), never, "the host fallback")
        check(r(fmode=fmode, auto8=auto8, i8_state=-1), never, "an int8 image that cannot be built")
        check(r(fmode=fmode, auto8=auto8, nrows=0), never, "an empty shard")
        for form in (S2X, I8X):
            assert resolve(hipann_mod, form, fmode=fmode, auto8=auto8)["eligible"] == 0


def test_hook_rejects_bad_input(hipann_mod):
    L = hipann_mod.lib()
    a, o = np.zeros(17, np.int32), np.zeros(17, np.int32)
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
    assert L.hipann_debug_ivf_scan_mode(ip(a), 17, ip(o), 17) == -1  # d, k, kout, np, max_nch = 0
    a[:] = [HALFX, 0, L2, 64, 10, 10, 4, 2, 3, 0, 1, 3, 0, 64, 1000, 0, 0]
    assert L.hipann_debug_ivf_scan_mode(ip(a), 17, ip(o), 17) == 0
    assert L.hipann_debug_ivf_scan_mode(ip(a), 16, ip(o), 17) == -1
    assert L.hipann_debug_ivf_scan_mode(ip(a), 17, ip(o), 16) == -1
    a[0] = 8
    assert L.hipann_debug_ivf_scan_mode(ip(a), 17, ip(o), 17) == -1
