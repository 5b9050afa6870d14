"""The route of a transform -- which kernels run and what lives where in the workspace -- is decided by one host function
(csrc/edt_api.hip: route_of) and exported as edt_hip_transform_route.  tests/golden/transform_routes.json holds what the
commit BEFORE that function existed decided, recorded from a probe in its dispatcher (tests/golden/README.md says how); every
field, every return code and every error text must stay exactly that.  Host arithmetic only: no GPU.
(tests/golden/make_golden_routes.py wrote the table.)

The table stores answers only, in the order of route_cases(), and a digest of the cases they belong to."""
import ctypes
import hashlib
import json
import os

import signed_cases as sc
from conftest import ROOT
from test_gpu_plain_rows import CASES as PLAIN_CASES
from test_workspace_layout import SHAPES_1D, SHAPES_2D, SHAPES_3D

TABLE = os.path.join(ROOT, "tests", "golden", "transform_routes.json")
ENV = ("EDT_HIP_FORCE_GENERIC", "EDT_HIP_WHOLE_INDEX_BYTES", "EDT_HIP_PLANE_PAD_BYTES")
ENV_VALUES = {"EDT_HIP_FORCE_GENERIC": "1", "EDT_HIP_WHOLE_INDEX_BYTES": "0", "EDT_HIP_PLANE_PAD_BYTES": "4096"}
SIZE_MAX = ctypes.c_size_t(-1).value
U8, U32, U64, F32 = 0, 2, 3, 4
BB, SQRT, GENERIC, BATCH, SMALL, BINARY, SIGNED = 1, 2, 4, 8, 16, 32, 64
OK, BAD_ARG, UNSUPPORTED = 0, -2, -4

FIELDS = ["x_kernel", "planes_from_labels", "index_form", "codes_whole", "y_pass", "z_pass", "plane16", "plane_inf_ok", "skip_nz",
          "row_flags", "zero_label", "sign", "binary_yz", "first_buffer", "second_volume", "index_fallback", "slab", "slabs",
          "code_pitch", "workspace_bytes"]
# every value a field can take (the sizes: whether they are zero, one, or more)
VALUES = {"x_kernel": {0, 1, 2, 3}, "y_pass": {0, 1, 2, 3, 4}, "z_pass": {0, 1, 2, 3, 4}, "zero_label": {0, 1, 2}, "sign": {0, 1, 2}}
# the refusals of a call before its first launch: (return code, how the error text begins)
REFUSALS = [(BAD_ARG, "unknown dtype"), (BAD_ARG, "ndim must be"), (BAD_ARG, "negative extent"), (BAD_ARG, "unused extents"),
            (UNSUPPORTED, "extent exceeds"), (BAD_ARG, "the voxel size along x"), (BAD_ARG, "voxel sizes (anisotropy)"),
            (BAD_ARG, "EDT_FLAG_BATCH_2D needs"), (UNSUPPORTED, "EDT_FLAG_SIGNED: shape not served"), (BAD_ARG, "workspace too small")]


class Route(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in FIELDS[:16]] + [(n, ctypes.c_int64) for n in FIELDS[16:19]] + [(FIELDS[19], ctypes.c_uint64)]


VOXEL_SIZES = [(1.0, 1.0, 1.0), (6.0, 6.0, 30.0), (1.0, 1.5, 0.5), (0.7, 1.3, 2.1), (0.5, 0.7, 1.3)]
FLAGS = [0, SQRT, GENERIC, BATCH, SMALL, BINARY, SIGNED, SIGNED | BINARY]
MODES = [0, 16, 32, 64, 0x400, 0x100000, 0x800000, 0x8000000, 0x10000000]
# the reduced list: every pass-X kernel, every kind of column pass, one and several slabs, two and one dimensions
FEW_3D = [(64, 100, 100), (64, 64, 64), (68, 100, 97), (600, 100, 97), (36, 100, 1000), (1100, 100, 97), (2200, 36, 10),
          (4100, 8, 5), (1024, 1024, 1024), (2048, 2048, 512)]
FEW = [(3, s) for s in FEW_3D] + [(2, (1024, 1024, 1)), (2, (5, 33000, 1)), (1, (5000, 1, 1))]


def ext3(shape):
    return (len(shape), tuple(shape) + (1,) * (3 - len(shape)))


def all_shapes():
    shapes = [(3, s) for s in SHAPES_3D] + [(2, s + (1,)) for s in SHAPES_2D] + [(1, (n, 1, 1)) for n in SHAPES_1D]
    shapes += [(3, (64, 100, 100)), (3, (8, 33, 257)), (3, (36, 500, 24)), (3, (2200, 36, 10)), (3, (4096, 64, 8)), (3, (17, 2049, 3))]
    shapes += [ext3(c.shape) for c in sc.CASES] + [ext3(s) for s, _ in sc.UNSUPPORTED] + [ext3(s) for s, _, _ in PLAIN_CASES]
    shapes += [(3, sc.BIG_SHAPE)]
    return sorted(set(shapes))


def case(dtype, ndim, ext, w, flags, ws="any", misalign=0, mode=0, env=None):
    return [dtype, ndim, *ext, *w, flags, ws, misalign, mode, env]


def route_cases():
    """[dtype, ndim, sx, sy, sz, wx, wy, wz, flags, workspace, out_misalignment, debug mode, environment hook] of every row.
    workspace: "any" (SIZE_MAX), or the bytes edt_hip_workspace_bytes_flags reports for the call's flags ("exact") or for its
    flags with EDT_FLAG_SMALL_WORKSPACE ("small"), or one byte less than either."""
    cases = []
    # the refusals of the shape and of the voxel sizes
    for bad in ([99, 3, 4, 4, 4], [U8, 0, 4, 4, 4], [U8, 4, 4, 4, 4], [U8, 3, -4, 4, 4], [U8, 2, 4, 4, 4], [U8, 1, 4, 4, 1],
                [U8, 3, 1 << 31, 1, 1]):
        cases.append(bad + [1.0, 1.0, 1.0, 0, "any", 0, 0, None])
    for w in ((0.0, 1.0, 1.0), (-1.0, 1.0, 1.0), (float("inf"), 1.0, 1.0), (1.0, 0.0, 1.0), (1.0, 1.0, float("nan")), (1.0, -2.0, -3.0)):
        cases.append(case(U8, 3, (64, 100, 100), w, 0))
    cases.append(case(U8, 2, (64, 100, 1), (1.0, 1.0, 0.0), 0))      # (the size of an axis the call does not have is not looked at)
    for ext in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):                     # (empty volumes: nothing to do, whatever else is asked)
        cases.append(case(U8, 3, ext, (1.0, 1.0, 1.0), SIGNED | BATCH, "small-1"))
    # the grid
    for ndim, ext in all_shapes():
        for dtype in (U8, U32, U64, F32):
            for w in VOXEL_SIZES:
                for bb in (0, BB):
                    for f in FLAGS:  # (BATCH_2D on the 2-D and 1-D shapes too: the refusal)
                        cases.append(case(dtype, ndim, ext, w, f | bb))
    # the reduced lists
    for ndim, ext in FEW:
        for w in (VOXEL_SIZES[0], VOXEL_SIZES[1], VOXEL_SIZES[3]):
            for bb in (0, BB):
                for f in (0, GENERIC, BINARY, SIGNED):
                    for mode in MODES[1:]:
                        cases.append(case(U8, ndim, ext, w, f | bb, mode=mode))
                for f in (0, SMALL, SIGNED):
                    for env in ENV:
                        cases.append(case(U8, ndim, ext, w, f | bb, env=env))
                for f in (0, GENERIC, SIGNED):
                    cases.append(case(U8, ndim, ext, w, f | bb, misalign=4))
                for f in (0, BATCH, SIGNED):
                    for ws in ("exact", "small", "exact-1", "small-1"):
                        cases.append(case(U8, ndim, ext, w, f | bb, ws=ws))
    cases.append(case(U8, 1, (5000, 1, 1), (1.0, 1.0, 1.0), 0, ws="none"))          # (a line without a workspace: a thread per row)
    cases.append(case(U8, 3, (64, 100, 100), (1.0, 1.0, 1.0), 0, ws="none"))
    return cases


def digest(cases):
    return hashlib.sha256(json.dumps(cases).encode()).hexdigest()


def answer(lib, c):
    """[return code, error text, the fields] of one case; sets the mode and the environment hook of the case"""
    dtype, ndim, sx, sy, sz, wx, wy, wz, flags, ws, misalign, mode, env = c
    for name in ENV:
        os.environ.pop(name, None)
    if env:
        os.environ[env] = ENV_VALUES[env]
    lib.edt_hip_set_debug_mode(mode)
    if ws == "any":
        nbytes = SIZE_MAX
    elif ws == "none":
        nbytes = 0
    else:
        f = flags | (SMALL if ws.startswith("small") else 0)
        nbytes = int(lib.edt_hip_workspace_bytes_flags(dtype, ndim, sx, sy, sz, f)) - (1 if ws.endswith("-1") else 0)
    r = Route()
    rc = lib.edt_hip_transform_route(dtype, ndim, sx, sy, sz, wx, wy, wz, flags, nbytes, misalign, ctypes.byref(r))
    err = lib.edt_hip_last_error().decode() if rc != OK else ""
    return [rc, err] + [int(getattr(r, n)) for n in FIELDS]


def answers(lib, cases):
    saved = {name: os.environ.get(name) for name in ENV}
    mode = lib.edt_hip_get_debug_mode()
    try:
        return [answer(lib, c) for c in cases]
    finally:
        lib.edt_hip_set_debug_mode(mode)
        for name, v in saved.items():
            os.environ.pop(name, None)
            if v is not None:
                os.environ[name] = v


def coverage_gaps(rows):
    """what the two conditions against an empty check miss: field values no accepted row takes, refusals no row is"""
    good = [r for r in rows if r[0] == OK]
    gaps = []
    for i, name in enumerate(FIELDS):
        seen = {r[2 + i] for r in good}
        if i < 16:
            missing = VALUES.get(name, {0, 1}) - seen
        else:
            missing = {k for k, hit in (("zero", 0 in seen), ("one", 1 in seen or i >= 18), ("more", any(v > 1 for v in seen))) if not hit}
        if missing:
            gaps.append((name, sorted(missing, key=str)))
    for rc, text in REFUSALS:
        if not any(r[0] == rc and r[1].startswith(text) for r in rows):
            gaps.append(("refusal", text))
    return gaps


def load_table():
    with open(TABLE) as f:
        t = json.load(f)
    return t, [t["answers"][i] for i in t["rows"]]


def test_routes_are_those_of_the_recorded_table():
    from edt import _lib
    lib = _lib.load()
    cases = route_cases()
    table, want = load_table()
    assert table["fields"] == FIELDS
    assert table["cases_sha256"] == digest(cases) and len(want) == len(cases), "the table does not hold the calls of route_cases()"
    got = answers(lib, cases)
    wrong = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(got)} routes differ, e.g. (case, got, recorded): {wrong[:3]}"


def test_the_table_is_no_empty_check():
    _, rows = load_table()
    assert coverage_gaps(rows) == []
    assert all(r[2:] == [0] * len(FIELDS) for r in rows if r[0] != OK)   # (a refusal leaves no route)


def test_forced_generic_in_the_environment_is_the_flag():
    """EDT_HIP_FORCE_GENERIC=1 and EDT_FLAG_FORCE_GENERIC give one route, one size and one refusal: the host-buffer entry
    points need not turn the one into the other before they call the dispatcher"""
    from edt import _lib
    lib = _lib.load()
    hooked = [c for c in route_cases() if c[12] == "EDT_HIP_FORCE_GENERIC"]
    flagged = [c[:8] + [c[8] | GENERIC] + c[9:12] + [None] for c in hooked]
    assert len(hooked) >= 100 and answers(lib, hooked) == answers(lib, flagged)


def test_plain_rows_run_on_the_integer_kernel_alone():
    """tests/test_gpu_plain_rows.py: the path it tests exists where both column passes are on the integer kernel alone"""
    from edt import _lib
    lib = _lib.load()
    for shape, an, bb in PLAIN_CASES:
        a = answers(lib, [case(U32, 3, shape, an, BB if bb else 0)])[0]
        r = dict(zip(FIELDS, a[2:]))
        assert a[0] == OK and r["y_pass"] == r["z_pass"] == 4 and r["row_flags"] == (1 if shape[0] <= 1024 else 0), (shape, an, bb, a)
