"""The sizes the library reports -- workspaces and slab records -- are part of its ABI: callers allocate by them and the plans
carve by the same arithmetic.  tests/golden/workspace_layout.json holds what the library answered before the column-pass
driver (csrc/edt_colpass.hip) and the shared workspace layouts replaced the hand-written copies; every answer must stay
exactly that.  Host arithmetic only: no GPU.  (tests/golden/make_golden_layout.py wrote the table.)"""
import json
import os

import pytest

from conftest import ROOT

TABLE = os.path.join(ROOT, "tests", "golden", "workspace_layout.json")
ENV = ("EDT_HIP_PLANE_PAD_BYTES", "EDT_HIP_WHOLE_INDEX_BYTES", "EDT_HIP_FORCE_GENERIC")

SHAPES_3D = [
    # tests/test_abi.py: test_argument_validation_needs_no_gpu, test_pitch_of_the_index_buffer_follows_the_slice_size
    (4, 4, 4), (64, 64, 64), (1024, 1024, 1024), (2048, 2048, 2048), (2048, 2048, 512), (63, 64, 64), (1024, 1024, 64),
    (2048, 512, 40), (2048, 2048, 8), (1024, 512, 64), (512, 1024, 64), (512, 512, 512), (1024, 1008, 64), (640, 512, 64),
    (160, 300, 140), (1024, 1024, 16),
    (40, 24, 33), (96, 280, 24), (36, 200, 1024), (2200, 36, 10), (16, 96, 1100), (4096, 64, 8), (64, 80, 72),
]
SHAPES_2D = [(1024, 1024), (260, 260)]
SHAPES_1D = [5000]


def layout_cases():
    """[function name, argument list] of every call of the table."""
    from edt import _lib
    flags = [0, _lib.FLAG_SMALL_WORKSPACE, _lib.FLAG_BATCH_2D, _lib.FLAG_FORCE_GENERIC]
    shapes = ([(3, s) for s in SHAPES_3D] + [(2, s + (1,)) for s in SHAPES_2D] + [(1, (n, 1, 1)) for n in SHAPES_1D] +
              [(4, (4, 4, 4)), (2, (4, 4, 4))])  # (bad ndim, unused extent != 1: 0 bytes)
    cases = [["edt_hip_workspace_bytes_flags", [99, 3, 4, 4, 4, 0]], ["edt_hip_shard_workspace_bytes", [99, 4, 4, 4]],
             ["edt_hip_shard_records_workspace_bytes", [99, 4, 4, 4]]]
    for ndim, (sx, sy, sz) in shapes:
        for dtype in (_lib.U8, _lib.U32, _lib.U64):
            for f in flags:
                cases.append(["edt_hip_workspace_bytes_flags", [dtype, ndim, sx, sy, sz, f]])
            cases.append(["edt_hip_shard_workspace_bytes", [dtype, sx, sy, sz]])
            cases.append(["edt_hip_shard_records_workspace_bytes", [dtype, sx, sy, sz]])
        cases.append(["edt_hip_voxel_graph_workspace_bytes", [ndim, sx, sy, sz]])
        for rows in sorted({sy, 32, max(32, sy // 2 // 32 * 32)}):
            cases.append(["edt_hip_shard_record_floats", [sx, rows]])
            cases.append(["edt_hip_shard_record16_words", [sx, rows]])
    return cases


def answers(lib):
    return [[name, args, int(getattr(lib, name)(*args))] for name, args in layout_cases()]


def test_reported_sizes_are_those_of_the_recorded_table(monkeypatch):
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
    assert [c[:2] for c in want] == [c[:2] for c in got], "the table does not hold the calls of layout_cases()"
    wrong = [(g, w[2]) for g, w in zip(got, want) if g[2] != w[2]]
    assert not wrong, f"{len(wrong)} of {len(got)} sizes differ, e.g. (call, args, got), recorded: {wrong[:5]}"
    assert any(c[2] > 1 << 32 for c in want) and any(c[2] == 0 for c in want)  # (64-bit answers and refusals are both there)
