"""CPU tier: the workspace contract of include/edt_hip.h ("Alignment") -- d_workspace of every *_device entry point must be
256-byte aligned, and any other pointer is refused with EDT_ERR_BAD_ARG before any device work.  The refusal happens while
the arguments are validated, so no device is needed: the buffers here are host stand-ins that are never dereferenced, the
workspace is `base + 4` with a correct size behind it, and the outputs keep their sentinel.  (The GPU tier repeats this on
device buffers: tests/test_gpu_offset_pointers.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from synth import aligned_host_bytes

BAD_ARG = -2
U8, U16, U32, U64, F32, F64, BOOL = range(7)
EXT = (64, 40, 33)
N = EXT[0] * EXT[1] * EXT[2]
FILL = -7


@pytest.fixture(scope="module")
def lib():
    from edt import _lib
    return _lib.load()


def p(a):
    return ctypes.c_void_p(a.ctypes.data)


class Stage:
    """valid arguments of every call over host stand-ins, and a workspace at base + `off`"""

    def __init__(self, off):
        self.off = off
        self.lab = np.ones(N, dtype=np.uint8)
        self.lab32 = np.ones(128 * 128 * 64, dtype=np.uint32)
        self.outs = []
        self.keep = []

    def out(self, dtype, count=N):
        a = np.full(count, FILL, dtype=dtype)
        self.outs.append(a)
        return a

    def ws(self, nbytes):
        assert nbytes > 0
        raw = aligned_host_bytes(nbytes + 256)
        self.keep.append(raw)
        return ctypes.c_void_p(raw.ctypes.data + self.off), int(nbytes)

    def untouched(self):
        return all(bool((a == FILL).all()) for a in self.outs)


def calls(lib, s):
    """(name, return code) of every *_device entry point that takes a workspace"""
    w = (6.0, 6.0, 30.0)
    f, i64, o32, o8 = s.out(np.float32), s.out(np.int64, 3), s.out(np.int32, 3 * N), s.out(np.int8)
    yield "edt_hip_edtsq_device", lib.edt_hip_edtsq_device(p(s.lab), U8, 3, *EXT, 1.0, 1.0, 1.0, 0, p(f), *s.ws(
        lib.edt_hip_workspace_bytes(U8, 3, *EXT)), None)
    yield "edt_hip_edtsq_device, a line", lib.edt_hip_edtsq_device(p(s.lab), U8, 1, N, 1, 1, 1.0, 1.0, 1.0, 0, p(f), *s.ws(
        lib.edt_hip_workspace_bytes(U8, 1, N, 1, 1)), None)
    yield "edt_hip_edtsq_voxel_graph_device", lib.edt_hip_edtsq_voxel_graph_device(
        p(s.lab), U8, p(s.lab), 3, *EXT, 1.0, 1.0, 1.0, 0, p(f), *s.ws(lib.edt_hip_voxel_graph_workspace_bytes(3, *EXT)), None)
    yield "edt_hip_extract_runs_device", lib.edt_hip_extract_runs_device(p(s.lab), U8, N, None, 0, p(i64), *s.ws(
        lib.edt_hip_runs_workspace_bytes(N)), None)
    yield "edt_hip_feature_transform_device", lib.edt_hip_feature_transform_device(
        p(s.lab), U8, 3, *EXT, 1.0, 1.0, 1.0, 0, p(o32), *s.ws(lib.edt_hip_feature_workspace_bytes(U8, 3, *EXT, 0)), None)
    yield "edt_hip_expand_labels_device", lib.edt_hip_expand_labels_device(
        p(s.lab), U8, 3, *EXT, 1.0, 1.0, 1.0, 1.0, p(o8), *s.ws(lib.edt_hip_expand_labels_workspace_bytes(U8, 3, *EXT)), None)
    tab = [s.out(np.int8, 16), s.out(np.int64, 16), s.out(np.float32, 16), s.out(np.int64, 16), s.out(np.int32, 96)]
    yield "edt_hip_label_stats_device", lib.edt_hip_label_stats_device(
        p(s.lab), U8, p(f), 3, *EXT, 16, *[p(t) for t in tab], p(i64), *s.ws(lib.edt_hip_label_stats_workspace_bytes(U8, N, 16)), None)
    yield "edt_hip_connected_components_device", lib.edt_hip_connected_components_device(
        p(s.lab), U8, 3, *EXT, 1, 0, p(o32), p(i64), *s.ws(lib.edt_hip_components_workspace_bytes(U8, 3, *EXT)), None)
    yield "edt_hip_fill_holes_device", lib.edt_hip_fill_holes_device(
        p(s.lab), U8, 3, *EXT, 1, 0, p(o8), p(i64), *s.ws(lib.edt_hip_fill_holes_workspace_bytes(U8, 3, *EXT)), None)
    yield "edt_hip_dust_device", lib.edt_hip_dust_device(
        p(s.lab), U8, 3, *EXT, 1, 0, 2, (1 << 63) - 1, 0, p(o8), p(i64), *s.ws(lib.edt_hip_dust_workspace_bytes(U8, 3, *EXT)), None)
    for op in range(4):
        yield "edt_hip_morphology_device", lib.edt_hip_morphology_device(
            p(s.lab), U8, 3, *EXT, 1.0, 1.0, 1.0, op, 2.0, 0, p(o8), *s.ws(lib.edt_hip_morphology_workspace_bytes(U8, 3, *EXT, op, 0)), None)
    radii, n_used = np.array([1.0, 2.0, 3.0]), s.out(np.int64, 1)
    yield "edt_hip_local_thickness_device", lib.edt_hip_local_thickness_device(
        p(s.lab), U8, 3, *EXT, 1.0, 1.0, 1.0, 0, p(radii), 3, 0.0, p(f), p(i64), p(n_used),
        *s.ws(lib.edt_hip_local_thickness_workspace_bytes(U8, 3, *EXT, 0)), None)
    yield "edt_hip_medial_axis_device", lib.edt_hip_medial_axis_device(
        p(s.lab), U8, 3, *EXT, 1.0, 1.0, 1.0, 0, 1.0, 0.0, p(o8), p(f), *s.ws(lib.edt_hip_medial_axis_workspace_bytes(U8, 3, *EXT, 0, 1)), None)
    z8 = s.out(np.int8)
    shard = s.ws(lib.edt_hip_shard_workspace_bytes(U8, *EXT))
    yield "edt_hip_shard_xy_device", lib.edt_hip_shard_xy_device(p(s.lab), None, U8, *EXT, 1.0, 1.0, 0, p(f), p(z8), *shard, None)
    yield "edt_hip_shard_z_device", lib.edt_hip_shard_z_device(p(f), p(z8), *EXT, 1.0, 0, *shard, None)
    yield "edt_hip_shard_z_device_ex", lib.edt_hip_shard_z_device_ex(p(f), p(z8), *EXT, 1.0, 0.0, 0, *shard, None)
    er = (64, 96, 8)
    block = aligned_host_bytes(4 * int(lib.edt_hip_shard_record_floats(er[0], er[1])) * er[2]).view(np.int32)
    block[:] = FILL
    s.outs.append(block)
    splits = (ctypes.c_int64 * 2)(0, er[1])
    ptrs = (ctypes.c_void_p * 1)(block.ctypes.data)
    rec = s.ws(max(lib.edt_hip_shard_records_workspace_bytes(U32, *er), lib.edt_hip_shard_records_workspace_bytes(U8, *er)))
    yield "edt_hip_shard_xy_records_device", lib.edt_hip_shard_xy_records_device(
        p(s.lab32), None, U32, *er, w[0], w[1], 1, 1, splits, ptrs, *rec, None)
    yield "edt_hip_shard_z_records_device", lib.edt_hip_shard_z_records_device(p(block), *er, w[2], 1, *rec, None)
    yield "edt_hip_shard_z_records_device_ex", lib.edt_hip_shard_z_records_device_ex(p(block), *er, w[2], 0.0, 1, *rec, None)
    yield "edt_hip_shard_z_records_device_w", lib.edt_hip_shard_z_records_device_w(p(block), *er, *w, 1, *rec, None)
    e16 = (64, 128, 128)
    assert lib.edt_hip_shard_records16_supported(U32, *e16, *w) == 1
    block16 = aligned_host_bytes(4 * int(lib.edt_hip_shard_record16_words(e16[0], e16[1])) * e16[2]).view(np.int32)
    block16[:] = FILL
    s.outs.append(block16)
    f16 = aligned_host_bytes(4 * e16[0] * e16[1] * e16[2]).view(np.int32)
    f16[:] = FILL
    s.outs.append(f16)
    splits16 = (ctypes.c_int64 * 2)(0, e16[1])
    ptrs16 = (ctypes.c_void_p * 1)(block16.ctypes.data)
    cnt = s.out(np.int32, 1)
    rec16 = s.ws(max(lib.edt_hip_shard_records_workspace_bytes(U32, *e16), lib.edt_hip_shard_records_workspace_bytes(U8, *e16)))
    yield "edt_hip_shard_xy_records16_device", lib.edt_hip_shard_xy_records16_device(
        p(s.lab32), None, U32, *e16, *w, 1, 1, splits16, ptrs16, p(cnt), *rec16, None)
    yield "edt_hip_shard_z_records16_device", lib.edt_hip_shard_z_records16_device(p(block16), p(f16), *e16, *w, 1, *rec16, None)


@pytest.mark.parametrize("off", [4, 1, 16, 128])
def test_every_device_entry_point_refuses_a_misaligned_workspace(lib, off):
    s = Stage(off)
    seen = []
    for name, rc in calls(lib, s):
        assert rc == BAD_ARG, (name, off, rc, lib.edt_hip_last_error())
        assert b"256-byte aligned" in lib.edt_hip_last_error(), (name, lib.edt_hip_last_error())
        assert s.untouched(), name
        seen.append(name.split(",")[0])
    # every *_device entry point of the header that takes a d_workspace was called
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "edt_hip.h")).read()
    declared = re.findall(r"\bint\s+(edt_hip_\w+)\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    takes_ws = {name for name, args in declared if "d_workspace" in args}
    assert takes_ws and takes_ws == set(seen), takes_ws ^ set(seen)


def test_header_states_the_contract():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "edt_hip.h")).read()
    assert "256-BYTE ALIGNED" in header and "alignment of their element type and nothing more" in header
