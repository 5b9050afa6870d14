"""CPU tier of watershed: the numpy + csgraph oracle (tests/watershed_oracle.py) against its naive pure-Python sibling, the
properties the contract states (include/edt_hip.h, "watershed"), the three shapes that motivated min_saliency on the field of the
tests' CPU transform, argument validation of the ABI functions (all of it happens before any device work, so no device is
needed), the Python argument handling, and the resources of the compiled kernels."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import watershed_oracle as oracle
from conftest import ROOT
from synth import aligned_host_bytes

BAD_ARG, UNSUPPORTED = -2, -4
U8, U16, U32, U64, F32, F64, BOOL = range(7)
NAMES = ("edt_hip_watershed_workspace_bytes", "edt_hip_watershed_device", "edt_hip_watershed")


@pytest.fixture(scope="module")
def lib():
    from edt import _lib
    return _lib.load()


def test_public_surface():
    import edt
    assert "watershed" in edt.__all__ and callable(edt.watershed)
    from edt import _lib, device
    assert callable(device.watershed)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    for doc in (edt.watershed.__doc__, device.watershed.__doc__):
        for word in ("STEEPEST-ASCENT", "drop of water", "hill climbing", "no markers", "flooding order", "greatest neighbour",
                     "single-linkage", "skimage", "SPLIT object"):
            assert word in " ".join(doc.split()), word


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def random_case(rng, nd, ties, max_extent=5):
    shape = tuple(int(v) for v in rng.integers(1, max_extent + 1, size=nd))
    lab = rng.integers(0, 3, size=shape).astype(rng.choice([np.uint8, np.int16, np.float32, np.uint64]))
    if ties:
        f = rng.integers(-1, 3, size=shape).astype(np.float32)
    else:
        f = rng.permutation(lab.size).reshape(shape).astype(np.float32) - np.float32(lab.size // 2)
    if rng.random() < 0.3:
        lab = np.asfortranarray(lab)
    return lab, f


@pytest.mark.parametrize("ties", [False, True], ids=["no_ties", "ties"])
@pytest.mark.parametrize("nd", [1, 2, 3])
def test_fast_oracle_against_naive_oracle(nd, ties):
    rng = np.random.default_rng(10 * nd + ties)
    split = 0
    for it in range(40):
        lab, f = random_case(rng, nd, ties)
        for c in range(1, nd + 1):
            for binary in (False, True):
                for h in (0.0, 0.5, 1.0, 2.5, 1e30):
                    got = oracle.watershed(lab, f, h, c, binary, return_N=True)
                    want = oracle.naive(lab, f, h, c, binary)
                    assert got[1] == want[1] and np.array_equal(got[0], want[0]), (it, lab.shape, c, binary, h)
                    assert got[0].dtype == np.uint32 and got[0].flags.f_contiguous == lab.flags.f_contiguous
                    split += got[1]
    assert split > 0


def test_oracle_special_values():
    nan = np.float32(np.nan)
    lab = np.array([1, 1, -0.0, nan, nan, 0, 2, 2, 2, 3], dtype=np.float32)
    f = np.array([1, 2, 9, 9, 9, 9, np.inf, np.inf, 1, -0.0], dtype=np.float32)
    out, n = oracle.watershed(lab, f, return_N=True)
    assert out.tolist() == [1, 1, 0, 2, 3, 0, 4, 4, 4, 5] and n == 5            # a NaN label is alone, -0.0 is background
    out, n = oracle.watershed(lab, f, binary=True, return_N=True)
    assert out.tolist() == [1, 1, 0, 2, 2, 0, 3, 3, 3, 3] and n == 3
    assert np.array_equal(oracle.naive(lab, f, binary=True)[0], out)
    z = np.array([0.0, -0.0, 0.0], dtype=np.float32)                              # +0.0 == -0.0: one plateau
    assert oracle.watershed(np.ones(3, np.uint8), z).tolist() == [1, 1, 1]
    assert oracle.watershed(np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.float32), return_N=True)[1] == 0
    assert oracle.watershed(np.array([1, 1, 0, 1], dtype=bool), np.array([3, 1, 5, 2], dtype=np.float32)).tolist() == [1, 1, 0, 2]


# ---- what the contract states ----------------------------------------------------------------------------------------------
def _objects(ndi, lab, c, binary):
    """scipy.ndimage.label per label value (of lab != 0 under binary), renumbered by first occurrence in C order"""
    st = ndi.generate_binary_structure(lab.ndim, c)
    comp = np.zeros(lab.shape, dtype=np.int64)
    n = 0
    for v in ([None] if binary else [v for v in np.unique(lab) if v != 0]):
        got, k = ndi.label(lab != 0 if v is None else lab == v, structure=st)
        comp[got > 0] = got[got > 0] + n
        n += k
    return oracle._number(comp, comp > 0, lab.shape)


def _refines(fine, coarse):
    """every set of `fine` lies in one set of `coarse` (0: background in both)"""
    if not np.array_equal(fine == 0, coarse == 0):
        return False
    pairs = np.unique(np.stack([fine.ravel(), coarse.ravel()]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1]


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_stated_properties(nd):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(nd)
    shape = {1: (60,), 2: (14, 17), 3: (7, 8, 9)}[nd]
    for it in range(6):
        ties = it % 2 == 1
        lab = ((rng.random(shape) < 0.8) * rng.integers(1, 3, size=shape)).astype(np.uint16)
        f = rng.integers(0, 4, size=shape).astype(np.float32) if ties else rng.permutation(lab.size).reshape(shape).astype(np.float32)
        for c in range(1, nd + 1):
            for binary in (False, True):
                objects, n_objects = _objects(ndi, lab, c, binary)
                st = ndi.generate_binary_structure(nd, c)
                prev = None
                for h in (0.0, 0.5, 1.0, 3.0, 1e30):
                    out, n = oracle.watershed(lab, f, h, c, binary, return_N=True)
                    assert n == out.max() and _refines(out, objects), (it, c, binary, h)     # every basin lies in one object
                    for b in range(1, n + 1):                                                 # ... and is connected at c
                        assert ndi.label(out == b, structure=st)[1] == 1, (it, c, binary, h, b)
                    if prev is not None:
                        assert _refines(prev, out), (it, c, binary, h)                        # unions of the basins at a smaller h
                    prev = out
                assert np.array_equal(out, objects) and n == n_objects                        # h = 1e30: connected_components
                flat, k = oracle.watershed(lab, np.full(shape, 2.5, np.float32), 0.0, c, binary, return_N=True)
                assert np.array_equal(flat, objects) and k == n_objects                       # a constant field: the same
                # h = 0: exactly one summit per basin (without ties there is no plateau that could drain two ways)
                base, n0 = oracle.watershed(lab, f, 0.0, c, binary, return_N=True)
                plateaus, is_max = oracle.regional_maxima(lab, f, c, binary)
                summits = np.unique(np.stack([base[is_max[plateaus]], plateaus[is_max[plateaus]]]), axis=1)
                per_basin = np.bincount(summits[0], minlength=n0 + 1)[1:]
                assert (per_basin >= 1).all()
                if not ties:
                    assert (per_basin == 1).all() and n0 == int(is_max.sum())
                # phase 2 at h = 0 changes nothing
                again = oracle.watershed(lab, f, 0.0, c, binary, return_N=True, always_phase2=True)
                assert again[1] == n0 and np.array_equal(again[0], base)


def test_a_draining_plateau_joins_the_basins_of_its_two_outlets():
    """3 | 1 1 1 | 3 in one row: the plateau of 1s is no maximum; its end voxels climb to the two summits and its middle voxel, a
    top voxel without a greater neighbour, is joined to both ends -- one basin, stated in the contract."""
    f = np.array([3, 1, 1, 1, 3], dtype=np.float32)
    lab = np.ones(5, dtype=np.uint8)
    out, n = oracle.watershed(lab, f, return_N=True)
    assert n == 1 and out.tolist() == [1] * 5 and oracle.naive(lab, f)[1] == 1
    plateaus, is_max = oracle.regional_maxima(lab, f)
    assert int(is_max.sum()) == 2                                # two summits in one basin
    # a plateau of two voxels has no such middle voxel: each end climbs to its own summit
    assert oracle.watershed(np.ones(4, np.uint8), np.array([3, 1, 1, 3], dtype=np.float32)).tolist() == [1, 1, 2, 2]
    # in 2-D, through the interior of a plateau
    f2 = np.array([[5, 1, 1, 1, 4], [0, 1, 1, 1, 0], [0, 1, 1, 1, 0]], dtype=np.float32)
    out2, n2 = oracle.watershed(np.ones_like(f2, dtype=np.uint8), f2, connectivity=1, return_N=True)
    assert n2 == 1


# ---- the three shapes behind min_saliency ------------------------------------------------------------------------------------
H_LADDER = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 1e30)
# basins at connectivity 1 and 3 along H_LADDER, as the oracle gives them on sqrt(oracle_port.edtsq) with a black border.  Tube and
# balls are the counts measured with scipy's transform when the operation was proposed; the blob mask is this file's own noise.
COUNTS = {
    "tube": ((19, 1, 1, 1, 1, 1, 1), (7, 1, 1, 1, 1, 1, 1)),
    "balls": ((2, 2, 2, 2, 2, 2, 1), (2, 2, 2, 2, 2, 2, 1)),
    "blobs": ((71, 12, 6, 6, 6, 6, 6), (24, 13, 9, 9, 8, 7, 6)),
}


@pytest.fixture(scope="module")
def shapes(oracle_port):
    made = {}
    for name, make in (("tube", oracle.diagonal_tube), ("balls", oracle.two_balls), ("blobs", oracle.blob_mask)):
        lab = make()
        made[name] = (lab, np.sqrt(oracle_port.edtsq(lab, (1.0, 1.0, 1.0), True)).astype(np.float32))
    return made


@pytest.mark.parametrize("name", ["tube", "balls", "blobs"])
def test_three_shapes(shapes, name):
    ndi = pytest.importorskip("scipy.ndimage")
    lab, f = shapes[name]
    got = tuple(tuple(oracle.watershed(lab, f, h, c, return_N=True)[1] for h in H_LADDER) for c in (1, 3))
    print(name, got)
    if name == "tube":
        for row in got:
            assert row[0] > 1 and row[1] == 1
    if name == "balls":
        for row in got:
            assert all(n == 2 for n in row[:6]) and row[6] == 1
    if name == "blobs":
        assert ndi.label(lab)[1] == got[0][6] == got[1][6] == 6
        for row in got:
            assert all(a >= b for a, b in zip(row, row[1:])) and row[0] > row[2]
    assert got == COUNTS[name]


# ---- ABI argument validation -------------------------------------------------------------------------------------------------
class _Args:
    """A valid argument set of both entry points over host stand-ins: every case below breaks exactly one item, and validation
    returns before anything is dereferenced."""

    def __init__(self, lib):
        self.lib = lib
        self.labels = np.ones(24, dtype=np.uint32)
        self.field = np.ones(24, dtype=np.float32)
        self.out = np.zeros(24, dtype=np.uint32)
        self.n = np.zeros(1, dtype=np.int64)
        self.ws = aligned_host_bytes(lib.edt_hip_watershed_workspace_bytes(U32, 3, 4, 3, 2))

    @staticmethod
    def p(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    def _args(self, kw):
        a = dict(labels=self.labels, dtype=U32, ndim=3, sx=4, sy=3, sz=2, field=self.field, connectivity=1, binary=0, h=0.5,
                 out=self.out, n=self.n, ws=self.ws, ws_bytes=None, w=(1.0, 1.0, 1.0), flags=0)
        a.update(kw)
        return a

    def device(self, **kw):
        a, p = self._args(kw), self.p
        raw = isinstance(a["ws"], int)                               # an address instead of an array: the size is self.ws's
        wb = (0 if a["ws"] is None else self.ws.size if raw else a["ws"].size) if a["ws_bytes"] is None else a["ws_bytes"]
        wp = ctypes.c_void_p(a["ws"]) if raw else p(a["ws"])
        return self.lib.edt_hip_watershed_device(p(a["labels"]), a["dtype"], a["ndim"], a["sx"], a["sy"], a["sz"], p(a["field"]),
                                                 a["connectivity"], a["binary"], a["h"], p(a["out"]), p(a["n"]), wp, wb, None)

    def host(self, **kw):
        a, p = self._args(kw), self.p
        return self.lib.edt_hip_watershed(p(a["labels"]), a["dtype"], a["ndim"], a["sx"], a["sy"], a["sz"], p(a["field"]), *a["w"],
                                          a["flags"], a["connectivity"], a["binary"], a["h"], p(a["out"]), p(a["n"]))


def _refused(lib, rc, what, code=BAD_ARG):
    assert rc == code, (what, rc)
    assert lib.edt_hip_last_error(), what


BAD = [
    ("unknown dtype", dict(dtype=7)), ("negative dtype", dict(dtype=-1)),
    ("ndim 0", dict(ndim=0)), ("ndim 4", dict(ndim=4)),
    ("unused sz", dict(ndim=2, connectivity=2)), ("unused sy", dict(ndim=1, sz=1, connectivity=1)),
    ("connectivity 0", dict(connectivity=0)), ("connectivity negative", dict(connectivity=-1)),
    ("connectivity 4", dict(connectivity=4)), ("connectivity 26", dict(connectivity=26)),
    ("connectivity 3 in 2-D", dict(ndim=2, sz=1, connectivity=3)), ("connectivity 2 in 1-D", dict(ndim=1, sy=1, sz=1, connectivity=2)),
    ("negative min_saliency", dict(h=-0.5)), ("NaN min_saliency", dict(h=float("nan"))), ("infinite min_saliency", dict(h=float("inf"))),
    ("min_saliency beyond float32", dict(h=1e39)), ("negative infinite min_saliency", dict(h=float("-inf"))),
    ("null labels", dict(labels=None)), ("null out", dict(out=None)), ("null n", dict(n=None)),
]


@pytest.mark.parametrize("what,kw", BAD, ids=[w for w, _ in BAD])
def test_abi_refuses_bad_arguments(lib, what, kw):
    a = _Args(lib)
    _refused(lib, a.device(**kw), "device: " + what)
    _refused(lib, a.host(**kw), "host: " + what)


def test_refusal_order(lib):
    """The order of connected_components -- shape (BAD_ARG), connectivity (BAD_ARG), the size limit (UNSUPPORTED) -- then
    min_saliency (BAD_ARG), then pointers, aliasing and the workspace (BAD_ARG): each is reported although everything after it is
    broken too."""
    a = _Args(lib)
    big = dict(sx=2048, sy=1024, sz=1024)
    for call, rest in ((a.device, dict(ws=None)), (a.host, {})):
        assert call(dtype=9, connectivity=0, h=-1.0, labels=None, **big, **rest) == BAD_ARG and b"dtype" in lib.edt_hip_last_error()
        assert call(connectivity=0, h=-1.0, labels=None, **big, **rest) == BAD_ARG and b"connectivity" in lib.edt_hip_last_error()
        assert call(h=-1.0, labels=None, n=None, **big, **rest) == UNSUPPORTED and b"2^31" in lib.edt_hip_last_error()
        assert call(h=-1.0, labels=None, n=None, **rest) == BAD_ARG and b"min_saliency" in lib.edt_hip_last_error()
        assert b"watershed" in lib.edt_hip_last_error()
        assert call(labels=None, n=None, **rest) == BAD_ARG and b"null" in lib.edt_hip_last_error()
        assert call(h=0.0, out=None, **rest) == BAD_ARG and b"null" in lib.edt_hip_last_error()
        assert call(h=1e30, labels=None, **rest) == BAD_ARG and b"null" in lib.edt_hip_last_error()
    # the device form: a field is required; NULL pointers, then aliasing, then the workspace
    assert a.device(field=None, ws=None) == BAD_ARG and b"null" in lib.edt_hip_last_error()
    assert a.device(out=a.labels, ws=None) == BAD_ARG and b"alias" in lib.edt_hip_last_error()
    assert a.device(out=a.field.view(np.uint32), ws=None) == BAD_ARG and b"alias" in lib.edt_hip_last_error()
    assert a.device(out=a.labels[4:], sz=1, ws=None) == BAD_ARG and b"alias" in lib.edt_hip_last_error()     # a partial overlap
    assert a.device(ws=None) == BAD_ARG and b"workspace" in lib.edt_hip_last_error()
    assert a.device(ws_bytes=a.ws.size - 1) == BAD_ARG and b"workspace" in lib.edt_hip_last_error()
    for off in (4, 1, 16, 128):                                  # (the offsets of tests/test_workspace_alignment_cpu.py)
        assert a.device(ws=a.ws.ctypes.data + off) == BAD_ARG and b"256-byte aligned" in lib.edt_hip_last_error(), off
    assert not a.out.any() and not a.n.any()                     # nothing was written
    # the host form: voxel sizes only where it computes the field itself, and no other flag than the border's
    assert a.host(field=None, w=(0.0, 1.0, 1.0), labels=None) == BAD_ARG and b"voxel size" in lib.edt_hip_last_error()
    assert a.host(field=None, w=(1.0, float("nan"), 1.0), labels=None) == BAD_ARG and b"voxel size" in lib.edt_hip_last_error()
    assert a.host(flags=2, w=(0.0, 1.0, 1.0), labels=None) == BAD_ARG and b"flags" in lib.edt_hip_last_error()
    assert a.host(h=-1.0, flags=2) == BAD_ARG and b"min_saliency" in lib.edt_hip_last_error()
    from edt import _lib
    if _lib.device_count() == 0:
        # an empty volume needs no pointer but n's; without a device the call then fails for want of one, not for an argument
        assert a.device(sx=0, labels=None, field=None, out=None, ws=None) == _lib.ERR_NO_DEVICE
        assert a.device() == _lib.ERR_NO_DEVICE and a.device(h=0.0) == _lib.ERR_NO_DEVICE
        assert a.host(w=(0.0, 0.0, 0.0)) == _lib.ERR_NO_DEVICE          # with a field the voxel sizes are not looked at
        assert a.host(field=None, flags=1) == _lib.ERR_NO_DEVICE
    n = np.full(1, -1, dtype=np.int64)
    assert a.host(sx=0, labels=None, field=None, out=None, n=n) == 0 and n[0] == 0      # (the host form only sets n)
    assert a.host(sx=0, labels=None, out=None, h=-1.0) == BAD_ARG
    assert a.host(sx=0, labels=None, out=None, n=None) == BAD_ARG


def test_workspace_query_and_size_limit(lib):
    q, fh = lib.edt_hip_watershed_workspace_bytes, lib.edt_hip_fill_holes_workspace_bytes
    assert q(7, 3, 8, 8, 8) == 0 and q(-1, 3, 8, 8, 8) == 0
    assert q(U32, 4, 8, 8, 8) == 0 and q(U32, 0, 8, 1, 1) == 0
    assert q(U32, 2, 8, 8, 8) == 0 and q(U32, 1, 8, 8, 1) == 0 and q(U32, 3, -1, 8, 8) == 0
    for code in (U8, U16, U32, U64, F32, F64, BOOL):
        for shape in ((64, 64, 1), (64, 64, 8), (70, 12, 9), (512, 512, 512), (1, 1, 1)):
            assert q(code, 3, *shape) == fh(code, 3, *shape) > 4 * shape[0] * shape[1] * shape[2]   # the peak plane and the chunk counts
            assert q(code, 3, *shape) % 256 == 0
    assert q(U32, 3, 2048, 1024, 1024) == 0
    assert q(U32, 3, 2047, 1024, 1024) > 4 * 2047 * 1024 * 1024
    assert q(U8, 1, (1 << 31) - 1, 1, 1) > 0
    assert q(U8, 3, 65536, 65536, 2) == 0 and q(U8, 3, 1 << 30, 1 << 30, 1 << 30) == 0
    a = _Args(lib)
    _refused(lib, a.device(sx=2048, sy=1024, sz=1024), "device: 2^31 voxels", UNSUPPORTED)
    _refused(lib, a.host(sx=2048, sy=1024, sz=1024), "host: 2^31 voxels", UNSUPPORTED)
    _refused(lib, a.device(sx=1 << 30, sy=1 << 30, sz=1 << 30), "device: 2^90 voxels", UNSUPPORTED)
    _refused(lib, a.host(sx=65536, sy=65536, sz=2), "host: 2^33 voxels", UNSUPPORTED)


# ---- the Python layer --------------------------------------------------------------------------------------------------------
def test_python_argument_handling(monkeypatch):
    import edt
    from edt import _lib
    seen = []

    def no_library():
        seen.append(1)
        raise AssertionError("the library was touched")

    img, vol, line = np.ones((4, 5), dtype=np.uint8), np.ones((3, 4, 5), dtype=np.uint16), np.ones(7, dtype=np.uint32)
    field = np.ones((3, 4, 5), dtype=np.float32)
    with monkeypatch.context() as m:
        m.setattr(_lib, "load", no_library)
        for data, bad in ((img, (0, 5, 26, 3, 6, 18, -1, 2.5, "8", True)), (vol, (0, 5, 4, 8, 27)), (line, (0, 2, 4, 6))):
            for c in bad:
                with pytest.raises(ValueError, match="watershed"):
                    edt.watershed(data, connectivity=c)
        for h in (-1.0, -1e-30, float("nan"), float("inf"), 1e39, "x", None, True, np.float32(-2)):
            with pytest.raises(ValueError, match="min_saliency"):
                edt.watershed(vol, field, min_saliency=h)
        for bad_field in (field[:2], field.astype(np.float64), field.reshape(3, 5, 4), np.ones(60, np.float32), field.astype(np.int32)):
            with pytest.raises(ValueError, match="field"):
                edt.watershed(vol, bad_field)
        nan_field = field.copy()
        nan_field[1, 2, 3] = np.nan
        with pytest.raises(ValueError, match="NaN"):
            edt.watershed(vol, nan_field)
        with pytest.raises(ValueError, match="NaN"):
            edt.watershed(np.asfortranarray(vol), np.asfortranarray(nan_field), min_saliency=1.0)
        with pytest.raises(ValueError, match="anisotropy"):
            edt.watershed(vol, anisotropy=(1.0, 0.0, 1.0))
        with pytest.raises(TypeError):
            edt.watershed(np.ones((2, 2, 2, 2), dtype=np.uint8))
        with pytest.raises(TypeError):
            edt.watershed(np.uint8(3))
        with pytest.raises(TypeError):
            edt.watershed(np.ones((4, 5), dtype=np.complex64))
        for shape in ((0,), (3, 0), (0, 2, 5)):
            for dtype in (np.float32, bool, np.int16):
                out, n = edt.watershed(np.zeros(shape, dtype=dtype), return_N=True)
                assert out.shape == shape and out.dtype == np.uint32 and n == 0
                assert edt.watershed(np.zeros(shape, dtype=dtype), np.zeros(shape, np.float32), 1.0).shape == shape
    assert not seen
    called = []
    with monkeypatch.context() as m:
        class Lib:
            @staticmethod
            def edt_hip_watershed(labels, code, nd, sx, sy, sz, f, wx, wy, wz, flags, c, binary, h, out, n):
                called.append((code, nd, sx, sy, sz, f is not None and f.value is not None, wx, wy, wz, flags, c, binary, h))
                ctypes.cast(n, ctypes.POINTER(ctypes.c_int64))[0] = 11
                return 0
        m.setattr(_lib, "load", lambda: Lib)
        nan_bg = field.copy()
        nan_bg[0, 0, 0] = np.nan
        holed = vol.copy()
        holed[0, 0, 0] = 0
        edt.watershed(holed, nan_bg)                                  # a NaN on the background is nobody's business
        edt.watershed(np.asfortranarray(vol), min_saliency=0.5, connectivity=18, anisotropy=(6, 6, 30), black_border=True, binary=True)
        edt.watershed(img.astype(np.int8), min_saliency=np.float32(1.5), connectivity=4, anisotropy=(2, 3))
        out, n = edt.watershed(line.astype(bool), np.arange(7, dtype=np.float32), 1e30, return_N=True)
    assert called == [(U16, 3, 5, 4, 3, True, 1.0, 1.0, 1.0, 0, 3, 0, 0.0), (U16, 3, 3, 4, 5, False, 6.0, 6.0, 30.0, 1, 2, 1, 0.5),
                      (U8, 2, 5, 4, 1, False, 3.0, 2.0, 1.0, 0, 1, 0, 1.5), (BOOL, 1, 7, 1, 1, True, 1.0, 1.0, 1.0, 0, 1, 0, float(np.float32(1e30)))]
    assert n == 11 and type(n) is int and out.dtype == np.uint32 and out.shape == (7,)
    if _lib.device_count() == 0:
        for data, c in ((img, 4), (img, None), (vol, 6), (vol, 26), (line, 1)):
            with pytest.raises(_lib.EdtHipError) as e:
                edt.watershed(data, connectivity=c)
            assert e.value.code == _lib.ERR_NO_DEVICE


# ---- the build ---------------------------------------------------------------------------------------------------------------
def test_watershed_kernels_have_no_scratch():
    """edt_watershed.hip compiled device-only for gfx950 with the flags of the other resource tests (tools/q16_resources.py): the
    code object's metadata gives no watershed kernel a private segment, and none spills a register."""
    if not os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import q16_resources
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "k.s")
        subprocess.run([hipcc, *q16_resources.FLAGS, "-S", "--cuda-device-only", "-o", asm, os.path.join(q16_resources.CSRC, "edt_watershed.hip")],
                       check=True, capture_output=True, cwd=d)
        text = open(asm).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                         r"\s+\.vgpr_spill_count:\s+(\d+)", meta)
    names = [k[0] for k in kernels]
    for stem, count in (("k_ws_init", 6), ("k_ws_ascend", 6), ("k_ws_merge", 6), ("k_ws_peaks", 1), ("k_ws_spread", 1)):
        assert sum(stem in n for n in names) == count, (stem, names)
    assert len(kernels) == 20
    for name, private, vgprs, spilled in kernels:
        print(name, "vgprs", vgprs)                                  # (recorded in DESIGN.md 20, not asserted)
        assert int(private) == 0 and int(spilled) == 0, (name, private, spilled)
