"""CPU tier: the case table of tests/test_gpu_signed.py (tests/signed_cases.py) against the library's host proof.

Whether the signed transform's sign is the epilogue of the last integer pass or a pass of its own is decided on the host
(csrc/edt_api.hip: route_of, the route's `sign`): rows of whole 16-byte granules, both column axes on the integer kernel, and the proof that
neither column pass can refuse a tile (edt_hip_q16_no_refusals: host arithmetic, no device).  The table states the route of
every row by hand; here every row is held against the proof before a GPU is involved, so that a row the GPU tier expects to be
fused can be, and the row that is there because its VALUES defeat the proof does."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import signed_cases as sc
import test_transform_routes_cpu as routes
from test_gpu_plain_rows import CASES as PLAIN_CASES


def _lib_loaded():
    from edt import _lib
    return _lib.load()


def library_proof(shape_xyz, w, bb):
    """edt_hip_q16_no_refusals: (the voxel sizes share a quantum, pass Y proven, pass Z proven)"""
    from edt import _lib
    lib = _lib.load()
    y, z = ctypes.c_int(-1), ctypes.c_int(-1)
    ndim = len(shape_xyz)
    ext = list(shape_xyz) + [1] * (3 - ndim)
    ws = [float(v) for v in w] + [1.0] * (3 - ndim)
    rc = lib.edt_hip_q16_no_refusals(*ext, *ws, ndim, int(bb), ctypes.addressof(y), ctypes.addressof(z))
    return rc, y.value, z.value


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_every_row_against_the_host_proof(case):
    proof = library_proof(case.shape, case.an, case.bb)
    if case.fused:
        assert len(case.shape) == 3 and case.shape[0] % 4 == 0 and min(case.shape[1:]) >= 97, case
        assert proof == (1, 1, 1), (case, proof)
    if "proof_fails" in case.cond:
        # the values row: everything else about it would allow the fused form
        assert case.shape[0] % 4 == 0 and min(case.shape[1:]) >= 97 and not case.fused
        assert proof[0] == 1 and proof[1:] != (1, 1), (case, proof)
        # ... and it is the values: the same extents at unit sizes are proven
        assert library_proof(case.shape, (1.0, 1.0, 1.0), case.bb) == (1, 1, 1)
    if not case.fused and "proof_fails" not in case.cond and case.family != "never":
        # a row of a fused family that the proof turned: it is the proof that says so
        assert proof != (1, 1, 1), (case, proof)
    assert (case.q is None) == (proof[0] == 0), (case, proof)
    # ... and the route of the call itself (edt_hip_transform_route): the sign is the epilogue of pass Z exactly where the table says
    ext = list(case.shape) + [1] * (3 - len(case.shape))
    ws = [float(v) for v in case.an] + [1.0] * (3 - len(case.an))
    code = {"uint8": 0, "uint16": 1, "uint32": 2, "uint64": 3, "float32": 4, "bool": 6}[np.dtype(case.dtype).name]
    a = routes.answers(_lib_loaded(), [routes.case(code, len(case.shape), ext, ws, routes.SIGNED | (routes.BB if case.bb else 0))])[0]
    assert a[0] == 0 and (a[2 + routes.FIELDS.index("sign")] == 1) == case.fused, (case, a)


def test_fused_rows_agree_with_the_table_of_plain_rows():
    """wherever tests/test_gpu_plain_rows.py lists a (shape, sizes, border), that file asserts the integer kernel alone: the row is fused here"""
    listed = {(s, a, b) for s, a, b in PLAIN_CASES}
    hits = [c for c in sc.CASES if (c.shape, c.an, c.bb) in listed and c.family != "never"]
    assert len(hits) >= 6
    assert all(c.fused for c in hits), [c for c in hits if not c.fused]


def test_quanta_of_the_table():
    """q is the largest number of which every squared voxel size is an integer multiple: the multiples are coprime"""
    for c in sc.CASES:
        if c.q is None:
            continue
        mult = [Fraction(a).limit_denominator(1 << 20) ** 2 / Fraction(c.q) for a in c.an]
        assert all(m.denominator == 1 for m in mult), (c, mult)
        assert math.gcd(*[int(m) for m in mult]) == 1, (c, mult)


def test_label_types_rotate_and_volumes_keep_their_names():
    assert {np.dtype(c.dtype) for c in sc.CASES} == {np.dtype(d) for d in sc.DTYPES}
    for fam in ("inf", "flat", "wide", "long"):
        assert len({np.dtype(c.dtype) for c in sc.CASES if c.family == fam}) >= 2, fam
    for c in sc.CASES:
        for name in c.volumes:
            assert name in sc.VOLUMES
    for name in sc.VOLUMES:
        lab = sc.make(name, (8, 40, 9), np.uint16)
        assert lab.flags.f_contiguous and lab.shape == (8, 40, 9)
        if name in sc.ONE_SIGN_BY_NAME:
            assert (lab == 0).all() or (lab != 0).all()
        elif not name.startswith("blocky"):   # (random blocks: the GPU tier asserts both signs at the rows' own shapes)
            assert (lab == 0).any() and (lab != 0).any(), name
        assert np.array_equal(sc.make(name, (8, 40, 9), bool), lab != 0)


def test_unsupported_shapes_are_refused_by_the_one_transform_form():
    from edt import _lib
    lib = _lib.load()
    for shape, _ in sc.UNSUPPORTED:
        if len(shape) == 1:
            continue  # (a line: the Python layer never asks -- edt.device._signed takes the two-transform branch)
        ext = list(shape) + [1] * (3 - len(shape))
        for code in (_lib.U8, _lib.U16, _lib.U32, _lib.U64, _lib.F32, _lib.BOOL):
            assert lib.edt_hip_signed_supported(code, len(shape), *ext, 0) == 0, (shape, code)
    for c in sc.CASES:
        ext = list(c.shape) + [1] * (3 - len(c.shape))
        assert lib.edt_hip_signed_supported(_lib.U8, len(c.shape), *ext, 0) == 1, c
    assert lib.edt_hip_signed_supported(_lib.U8, 3, *sc.BIG_SHAPE, 0) == 1


def test_the_big_volume_passes_one_trip_of_the_sign_kernel():
    n = int(np.prod(sc.BIG_SHAPE))
    assert sc.BIG_SHAPE[0] % 4 != 0          # rows of no whole granules: the sign is a pass of its own
    assert n > sc.TRIP_VOXELS + 8            # quads behind the first trip whatever the head, and a tail for some head
    assert {(n - h) % 4 for h in (1, 2, 3)} >= {1, 2}
