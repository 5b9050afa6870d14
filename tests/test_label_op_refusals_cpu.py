"""The refusals of the label operations, word for word: the return code and the exact edt_hip_last_error() text of every
refusal of the four device entry points (connected_components, fill_holes, dust, label_stats) and of the host forms, held
against tests/golden/label_op_refusals.json (recorded by tests/golden/make_golden_refusals.py from the library whose texts are
the contract).  The sibling CPU tiers match substrings; here the whole text and the order of the checks are pinned.  Every
case returns before the library looks for a device, so none is needed."""
import json
import os

import pytest

import test_components_cpu as cc
import test_dust_cpu as dust
import test_fill_holes_cpu as fh
import test_label_stats_cpu as ls

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_op_refusals.json")
BIG = dict(sx=2048, sy=1024, sz=1024)                                  # 2^31 voxels: one past the limit
SMALLER = dict(sx=1 << 20, sy=64, sz=1, ndim=2, connectivity=2)        # a call whose volume the workspace does not cover
# each line is reported although everything after it is broken too (test_refusal_order of the sibling tiers)
ORDER = [("dtype first", dict(dtype=9, connectivity=0, labels=None, **BIG)),
         ("connectivity before the size limit", dict(connectivity=0, labels=None, **BIG)),
         ("the size limit before pointers", dict(labels=None, n=None, **BIG)),
         ("the result pointer", dict(labels=None, n=None))]
DUST_ORDER = [("dtype first", dict(dtype=9, connectivity=0, lo=-1, labels=None, **BIG)),
              ("connectivity before the size limit", dict(connectivity=0, lo=-1, labels=None, **BIG)),
              ("the size limit before the bounds", dict(lo=-1, labels=None, counts=None, **BIG)),
              ("min_voxels before max_voxels", dict(lo=-1, hi=-2, labels=None, counts=None)),
              ("max_voxels before pointers", dict(lo=3, hi=2, labels=None, counts=None)),
              ("the result pointer", dict(labels=None, counts=None)),
              ("an empty range is allowed", dict(lo=4, hi=4, labels=None))]
VOXEL_SIZES = [(0.0, 1.0, 1.0), (-1.0, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, float("inf")), (1.0, 0.0, 1.0)]


def cases(lib):
    """[(id, call)]: every call is refused before any device work and leaves its reason in edt_hip_last_error()."""
    out = []

    def add(op, form, what, call, kw):
        out.append((f"{op} {form}: {what}", lambda: call(**kw)))

    for op, mod, bad, order in (("connected_components", cc, cc.SHARED_BAD, ORDER), ("fill_holes", fh, fh.SHARED_BAD, ORDER),
                                ("dust", dust, dust.BAD, DUST_ORDER), ("label_stats", ls, ls.SHARED_BAD, [])):
        a = mod._Args(lib)
        for what, kw in bad:
            add(op, "device", what, a.device, kw)
            add(op, "host", what, a.host, kw)
        for what, kw in order:
            add(op, "device", "order, " + what, a.device, dict(kw, ws=None))
            add(op, "host", "order, " + what, a.host, kw)
        add(op, "device", "null labels before the workspace", a.device, dict(labels=None, ws=None))
        add(op, "device", "no workspace", a.device, dict(ws=None))
        add(op, "device", "workspace one byte short", a.device, dict(ws_bytes=a.ws.size - 1))
        if op != "label_stats":
            add(op, "device", "workspace of a smaller call", a.device, SMALLER)
            add(op, "device", "2^31 voxels", a.device, BIG)
            add(op, "host", "2^31 voxels", a.host, BIG)
            add(op, "device", "2^90 voxels", a.device, dict(sx=1 << 30, sy=1 << 30, sz=1 << 30))
    a = fh._Args(lib)
    add("fill_holes", "device", "out is labels", a.device, dict(out=a.labels))
    add("fill_holes", "host", "out is labels", a.host, dict(out=a.labels))
    add("fill_holes", "device", "out is labels, before the workspace", a.device, dict(out=a.labels, ws=None))
    a = ls._Args(lib)
    add("label_stats", "device", "null dt", a.device, dict(dt=None))
    add("label_stats", "device", "workspace of a smaller call", a.device,
        dict(sx=1024, sy=1024, sz=1, ndim=2, max_labels=1 << 16))
    add("label_stats", "device", "max_labels beyond 2^38", a.device, dict(max_labels=(1 << 38) + 1))
    for w in VOXEL_SIZES:
        add("label_stats", "host", f"voxel sizes {w}", a.host, dict(dt=None, w=w))
    return out


def record(lib):
    """The table: one row per case, in the order of cases()."""
    rows = []
    for name, call in cases(lib):
        rc = call()
        rows.append({"id": name, "rc": rc, "error": lib.edt_hip_last_error().decode()})
    return rows


GOLDEN = []                                       # (empty only while the table is being recorded for the first time)
if os.path.exists(TABLE):
    with open(TABLE) as f:
        GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def lib():
    from edt import _lib
    return _lib.load()


def test_the_table_holds_every_case_and_only_refusals(lib):
    assert [row["id"] for row in GOLDEN] == [name for name, _ in cases(lib)]
    assert len({row["id"] for row in GOLDEN}) == len(GOLDEN) > 150
    assert all(row["rc"] in (-2, -4) and row["error"] for row in GOLDEN)      # BAD_ARG or UNSUPPORTED, with a reason


@pytest.fixture(scope="module")
def calls(lib):
    return dict(cases(lib))


@pytest.mark.parametrize("row", GOLDEN, ids=[row["id"] for row in GOLDEN])
def test_refusal_is_word_for_word(lib, calls, row):
    assert calls[row["id"]]() == row["rc"]
    assert lib.edt_hip_last_error().decode() == row["error"]
