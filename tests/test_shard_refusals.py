"""What the phase entry points of the Z-sharded path (csrc/edt_shard_api.hip) refuse, in which order and in which words, is part
of their behaviour: every one of them checks everything before its first launch and asks for no device on a refusal, so the
whole table runs without a GPU.  tests/golden/shard_refusals.json holds what the library answered before the phases got one
prologue and the record forms one body each; every answer must stay exactly that -- return code and edt_hip_last_error() text,
call for call.  (tests/golden/make_golden_shard_refusals.py wrote the table.)

The calls: one single-fault call per check of every entry point, double-fault calls for every pair of adjacent steps of its
prologue (which of the two answers IS the order), and the empty volume, which is EDT_OK whatever the pointers.  No call of the
table is well-formed: that one would launch.  Pointers are made-up addresses: a refusal never follows one."""
import ctypes
import json
import os

from conftest import ROOT

TABLE = os.path.join(ROOT, "tests", "golden", "shard_refusals.json")
ENV = ("EDT_HIP_FORCE_GENERIC",)

XY_HEAD = ["d_labels", "d_halo", "dtype", "sx", "sy", "sz", "wx", "wy"]
TAIL = ["d_workspace", "workspace_bytes", "stream"]
SPLITS = ["nparts", "y_splits", "d_blocks"]
PHASES = {  # the arguments of every phase entry point, in the order of include/edt_hip.h
    "edt_hip_shard_xy_device": XY_HEAD + ["flags", "d_partial", "d_zflags"] + TAIL,
    "edt_hip_shard_z_device": ["d_partial", "d_zflags", "sx", "sy", "sz", "wz", "flags"] + TAIL,
    "edt_hip_shard_z_device_ex": ["d_partial", "d_zflags", "sx", "sy", "sz", "wz", "field_floor", "flags"] + TAIL,
    "edt_hip_shard_xy_records_device": XY_HEAD + ["flags"] + SPLITS + TAIL,
    "edt_hip_shard_z_records_device": ["d_records", "sx", "sy", "sz", "wz", "flags"] + TAIL,
    "edt_hip_shard_z_records_device_ex": ["d_records", "sx", "sy", "sz", "wz", "field_floor", "flags"] + TAIL,
    "edt_hip_shard_z_records_device_w": ["d_records", "sx", "sy", "sz", "wx", "wy", "wz", "flags"] + TAIL,
    "edt_hip_shard_xy_records16_device": XY_HEAD + ["wz", "flags"] + SPLITS + ["d_refused"] + TAIL,
    "edt_hip_shard_z_records16_device": ["d_records", "d_out", "sx", "sy", "sz", "wx", "wy", "wz", "flags"] + TAIL,
}
BLOCKS = [0x20000000, 0x21000000]
WELL_FORMED = {  # (an XY phase: a slab of 4 slices cut into two destinations; a Z phase: 32 rows of 128 slices)
    "d_labels": 0x10000000, "d_halo": 0x11000000, "d_partial": 0x12000000, "d_zflags": 0x13000000, "d_records": 0x14000000,
    "d_out": 0x15000000, "d_refused": 0x16000000, "d_workspace": 0x40000000, "workspace_bytes": "need", "stream": None,
    "dtype": 2, "sx": 64, "wx": 1.0, "wy": 1.0, "wz": 1.0, "field_floor": 0.0, "flags": 0,
    "nparts": 2, "y_splits": [0, 64, 128], "d_blocks": BLOCKS,
}
EXTENTS = {True: {"sy": 128, "sz": 4}, False: {"sy": 32, "sz": 128}}  # (is an XY phase)
NO_QUANTUM = {"wx": 3.58, "wy": 3.58, "wz": 40.0}


def phase_steps(name):
    """The prologue of one entry point as [(step, [(what, overrides)])], in the order the entry point makes its checks: a
    single-fault call per entry, a double-fault call per pair of adjacent steps (the first fault of each)."""
    params = PHASES[name]
    xy, records, r16 = "_xy_" in name, "records" in name, "records16" in name
    pointers = [p for p in params if p.startswith("d_") and p not in ("d_halo", "d_workspace", "d_blocks")]
    shape = ([("bad dtype", {"dtype": 99})] if xy else []) + [(f"negative {e}", {e: -1}) for e in ("sx", "sy", "sz")] + [
        (f"{e} beyond 2^31-1", {e: 1 << 31}) for e in ("sx", "sy", "sz")]
    if xy:
        voxel = [(f"{w} = {v}", {w: v}) for w in ("wx", "wy") for v in (0.0, "nan", "inf")] + [("wx = -1", {"wx": -1.0})]
    else:
        voxel = [(f"wz = {v}", {"wz": v}) for v in (0.0, "nan", "inf")]
    null = [(f"null {p}", {p: None}) for p in pointers]
    if "nparts" in params:
        null += [("null y_splits", {"y_splits": None}), ("null d_blocks", {"d_blocks": None}), ("nparts = 0", {"nparts": 0})]
    support = [("sx = 2052", {"sx": 2052})] if records else []
    if r16:
        support += [("no quantum", NO_QUANTUM), ("rows of half granules", {"sx": 66}), ("wz = 0", {"wz": 0.0})]
        support += [("sy of two bands", {"sy": 64, "y_splits": [0, 32, 64]})] if xy else [("sz of two bands", {"sz": 64})]
    splits = [("y_splits from 32", {"y_splits": [32, 64, 128]}), ("y_splits to 96", {"y_splits": [0, 64, 96]}),
              ("y_splits not increasing", {"y_splits": [0, 128, 128]}), ("y_splits off 32", {"y_splits": [0, 48, 128]}),
              ("null block", {"d_blocks": [BLOCKS[0], None]})]
    if r16:
        splits.append(("block off 8 bytes", {"d_blocks": [BLOCKS[0], BLOCKS[1] + 4]}))
    workspace = [("null workspace", {"d_workspace": None}), ("workspace one byte short", {"workspace_bytes": "need-1"}),
                 ("workspace off 256 bytes", {"d_workspace": WELL_FORMED["d_workspace"] + 128})]
    steps = [("shape", shape), ("voxel sizes", voxel), ("null pointers", null)]
    if name == "edt_hip_shard_xy_records_device":
        steps += [("support", support), ("y_splits", splits), ("workspace", workspace),
                  ("blocks of whole granules", [("block off 16 bytes", {"d_blocks": [BLOCKS[0], BLOCKS[1] + 8]})])]
    elif name == "edt_hip_shard_xy_records16_device":
        steps += [("y_splits", splits), ("support", support), ("workspace", workspace)]
    elif name == "edt_hip_shard_z_records16_device":
        steps += [("support", support), ("records and output", [("d_records off 16 bytes", {"d_records": WELL_FORMED["d_records"] + 8}),
                                                                ("d_out off 16 bytes", {"d_out": WELL_FORMED["d_out"] + 8})]),
                  ("workspace", workspace)]
    else:
        steps += ([("support", support)] if records else []) + [("workspace", workspace)]
    return steps


def refusal_cases():
    """[entry point, what is wrong with the call, argument list] of every call of the table."""
    cases = []
    for name, params in PHASES.items():
        xy = "_xy_" in name
        steps = phase_steps(name)
        calls = [(f"{step}: {what}", over) for step, faults in steps for what, over in faults]
        # a negative size along y / z is taken as |w|: such a call gets as far as its workspace
        calls.append(("negative wy / wz, null workspace", {"wy": -1.0, "wz": -1.0, "d_workspace": None}))
        for (a, fa), (b, fb) in zip(steps, steps[1:]):
            calls.append((f"{a} and {b}: {fa[0][0]}, {fb[0][0]}", {**fb[0][1], **fa[0][1]}))
        if "nparts" in params:  # (the two XY record phases answer this one differently)
            calls.append(("unsupported extents and bad y_splits", {"sx": 2052, "y_splits": [32, 64, 128]}))
        # the empty volume: EDT_OK before any pointer is looked at -- but after the voxel sizes
        nothing = {p: None for p in params if p.startswith("d_") or p == "y_splits"}
        for e in ("sx", "sy", "sz"):
            calls.append((f"empty: {e} = 0", {e: 0}))
            calls.append((f"empty: {e} = 0, null pointers", {e: 0, **nothing}))
        calls.append(("voxel sizes and empty", {"sz": 0, **steps[1][1][0][1]}))
        for what, over in calls:
            v = {**WELL_FORMED, **EXTENTS[xy], **over}
            cases.append([name, what, [v[p] for p in params]])
    return cases


def _need(lib, name, args):
    """workspace_bytes of a call: what the size query of its form answers for its extents (a call whose extents have no
    answer: plenty)."""
    v = dict(zip(PHASES[name], args))
    query = lib.edt_hip_shard_records_workspace_bytes if "records" in name else lib.edt_hip_shard_workspace_bytes
    return int(query(v.get("dtype", 0), v["sx"], v["sy"], v["sz"])) or 1 << 30  # (a Z phase: EDT_U8)


def call(lib, name, args):
    """(return code, error text) of one call of the table; the text only of a refusal"""
    keep, c_args = [], []
    for p, a in zip(PHASES[name], args):
        if p == "y_splits" and a is not None:
            a = (ctypes.c_int64 * len(a))(*a)
        elif p == "d_blocks" and a is not None:
            a = (ctypes.c_void_p * len(a))(*a)
        elif p == "workspace_bytes":
            a = _need(lib, name, args) - (1 if a == "need-1" else 0)
        elif isinstance(a, str):
            a = float(a)
        keep.append(a)
        c_args.append(ctypes.c_void_p(a) if p.startswith("d_") and isinstance(a, int) else a)
    rc = int(getattr(lib, name)(*c_args))
    return rc, (lib.edt_hip_last_error().decode() if rc != 0 else None)


def answers(lib):
    return [[name, what, args, *call(lib, name, args)] for name, what, args in refusal_cases()]


def test_refusals_of_the_sharded_phases_are_those_of_the_recorded_table(monkeypatch):
    from edt import _lib
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    lib = _lib.load()
    mode = lib.edt_hip_get_debug_mode()
    lib.edt_hip_set_debug_mode(0)
    try:
        got = answers(lib)
    finally:
        lib.edt_hip_set_debug_mode(mode)
    with open(TABLE) as f:
        want = json.load(f)
    assert [c[:3] for c in want] == [c[:3] for c in got], "the table does not hold the calls of refusal_cases()"
    wrong = [(g, w[3:]) for g, w in zip(got, want) if g[3:] != w[3:]]
    assert not wrong, f"{len(wrong)} of {len(got)} answers differ, e.g. (call, got), recorded: {wrong[:5]}"
    assert {c[0] for c in want} == set(PHASES)
    # (all three return codes are there, and the two XY record phases answer "unsupported extents and bad y_splits" differently)
    assert {c[3] for c in want} == {0, -2, -4}
    both = [c[3] for c in want if c[1] == "unsupported extents and bad y_splits"]
    assert both == [-4, -2]
