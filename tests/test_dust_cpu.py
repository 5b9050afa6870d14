"""CPU tier of dust: the numpy oracle (tests/dust_oracle.py) against scipy.ndimage.label + np.bincount, the sparse volumes of the
GPU tier, argument validation of the ABI functions (all of it happens before any device work, so no device is needed) and the
Python argument handling."""
import ctypes

import numpy as np
import pytest

import dust_oracle as oracle
from synth import aligned_host_bytes

BAD_ARG, UNSUPPORTED = -2, -4
U8, U16, U32, U64, F32, F64, BOOL = range(7)
INT64_MAX = (1 << 63) - 1
NAMES = ("edt_hip_dust_workspace_bytes", "edt_hip_dust_device", "edt_hip_dust")
SPARSE = ((0.45, False, 186, 37), (0.12, True, 80, 21))       # p, binary, removed at least, kept at least (threshold 4)


@pytest.fixture(scope="module")
def lib():
    from edt import _lib
    return _lib.load()


def test_public_surface():
    import edt
    assert "dust" in edt.__all__ and callable(edt.dust) and edt.DustCounts._fields == ("components", "kept", "removed_voxels")
    from edt import _lib, device
    assert callable(device.dust)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)


# ---- the oracle -----------------------------------------------------------------------------------------------------
def scipy_dust(ndi, data, lo, hi, c, binary, invert=False):
    """(out, components, kept, removed) from scipy.ndimage.label + np.bincount, label value by label value unless binary."""
    nd = data.ndim
    structure = ndi.generate_binary_structure(nd, c)
    out = data.copy()
    found = kept = removed = 0
    values = [None] if binary else [v for v in np.unique(data) if v != 0]
    for v in values:
        comp, n = ndi.label(data != 0 if v is None else data == v, structure=structure)
        size = np.bincount(comp.ravel(), minlength=n + 1)
        keep = (size >= lo) & (size < hi)
        if invert:
            keep = ~keep
        keep[0] = True
        gone = ~keep[comp]
        out[gone] = 0
        found += n
        kept += int(np.count_nonzero(keep[1:]))
        removed += int(np.count_nonzero(gone))
    return out, found, kept, removed


def test_sparse_volumes_have_something_to_remove_and_to_keep():
    """The volumes of the GPU tier on the CPU: at every seed and connectivity enough components are removed AND kept at
    threshold 4, and enough lie in [3, 9), for the comparison there to mean something."""
    for p, binary, removed, kept in SPARSE:
        for seed in range(5):
            lab = oracle.sparse_volume(seed, p)
            assert lab.flags.f_contiguous and lab.dtype == np.uint32 and lab.shape == (70, 12, 9)
            for c in (1, 2, 3):
                got = oracle.dust(lab, 4, c, binary=binary)
                assert got.removed_voxels >= removed and got.kept >= kept, (p, seed, c, got[1:])
                assert got.components - got.kept >= 20
                if not binary:
                    assert oracle.in_range(lab, 3, 9, c) >= 42, (seed, c)
                assert oracle.in_range(lab, 3, 9, c, binary) >= 20, (p, seed, c)


@pytest.mark.parametrize("seed", range(5))
def test_oracle_against_scipy_binary(seed):
    ndi = pytest.importorskip("scipy.ndimage")
    for p, _, _, _ in SPARSE:
        lab = oracle.sparse_volume(seed, p)
        for c in (1, 2, 3):
            for threshold, invert in ((4, False), ((3, 9), False), ((3, 9), True)):
                lo, hi = oracle.bounds(threshold)
                want = scipy_dust(ndi, lab, lo, hi, c, True, invert)
                for data in (lab, np.ascontiguousarray(lab)):
                    got = oracle.dust(data, threshold, c, binary=True, invert=invert)
                    assert np.array_equal(got.out, want[0]) and got[1:] == want[1:], (p, c, threshold, invert)
                    assert got.out.flags.f_contiguous == data.flags.f_contiguous


SCIPY_SHAPES = ((40,), (13, 11), (9, 8, 7), (70, 12, 9))


@pytest.mark.parametrize("shape", SCIPY_SHAPES, ids=[str(s) for s in SCIPY_SHAPES])
def test_oracle_against_scipy_multi_label(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(len(shape))
    nd = len(shape)
    removed = kept = 0
    for density in (0.4, 0.7):
        lab = ((rng.random(shape) < density) * rng.integers(1, 4, size=shape)).astype(np.int16)
        lab[lab == 3] = -3
        for c in range(1, nd + 1):
            for threshold, invert in ((3, False), ((2, 5), False), ((2, 5), True), (0, False), (lab.size + 1, False)):
                lo, hi = oracle.bounds(threshold)
                want = scipy_dust(ndi, lab, lo, hi, c, False, invert)
                got = oracle.dust(np.asfortranarray(lab), threshold, c, invert=invert)
                assert np.array_equal(got.out, want[0]) and got[1:] == want[1:], (shape, c, threshold, invert)
                removed += got.removed_voxels
                kept += got.kept
    assert removed > 0 and kept > 0


def test_oracle_special_values():
    nan = np.float32(np.nan)
    line = np.array([1, 1, -0.0, nan, nan, 0, 2, 2, 2, 0, np.inf], dtype=np.float32)
    got = oracle.dust(line, 2)
    assert got[1:] == (5, 2, 3)                                      # two NaN components and the inf go
    assert got.out[:2].tolist() == [1, 1] and np.signbit(got.out[2]) and got.out[3:6].tolist() == [0, 0, 0]
    assert not np.signbit(got.out[3]) and got.out[6:9].tolist() == [2, 2, 2] and got.out[10] == 0
    got = oracle.dust(line, 2, binary=True)
    assert got[1:] == (4, 3, 1) and np.isnan(got.out[3]) and np.isnan(got.out[4]) and got.out[10] == 0
    assert oracle.dust(np.zeros((0, 3), dtype=np.uint8), 4)[1:] == (0, 0, 0)
    b = np.array([1, 1, 0, 1], dtype=bool)
    assert oracle.dust(b, 2).out.tolist() == [True, True, False, False]


# ---- ABI argument validation -----------------------------------------------------------------------------------------
class _Args:
    """A valid argument set of both entry points over host stand-ins: every case below breaks exactly one item, and
    validation returns before anything is dereferenced."""

    def __init__(self, lib):
        self.lib = lib
        self.labels = np.ones(24, dtype=np.uint32)
        self.out = np.zeros(24, dtype=np.uint32)
        self.counts = np.zeros(3, dtype=np.int64)
        self.ws = aligned_host_bytes(lib.edt_hip_dust_workspace_bytes(U32, 3, 4, 3, 2))   # (256-byte aligned, as the ABI requires of d_workspace)

    @staticmethod
    def p(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    def _args(self, kw):
        a = dict(labels=self.labels, dtype=U32, ndim=3, sx=4, sy=3, sz=2, connectivity=1, binary=0, lo=2, hi=INT64_MAX, invert=0,
                 out=self.out, counts=self.counts, ws=self.ws, ws_bytes=None)
        a.update(kw)
        return a

    def device(self, **kw):
        a, p = self._args(kw), self.p
        wb = (0 if a["ws"] is None else a["ws"].size) if a["ws_bytes"] is None else a["ws_bytes"]
        return self.lib.edt_hip_dust_device(p(a["labels"]), a["dtype"], a["ndim"], a["sx"], a["sy"], a["sz"], a["connectivity"],
                                            a["binary"], a["lo"], a["hi"], a["invert"], p(a["out"]), p(a["counts"]), p(a["ws"]),
                                            wb, None)

    def host(self, **kw):
        a, p = self._args(kw), self.p
        return self.lib.edt_hip_dust(p(a["labels"]), a["dtype"], a["ndim"], a["sx"], a["sy"], a["sz"], a["connectivity"],
                                     a["binary"], a["lo"], a["hi"], a["invert"], p(a["out"]), p(a["counts"]))


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
    ("negative min_voxels", dict(lo=-1)), ("max_voxels below min_voxels", dict(lo=5, hi=4)),
    ("negative max_voxels", dict(lo=0, hi=-1)),
    ("null labels", dict(labels=None)), ("null out", dict(out=None)), ("null counts", dict(counts=None)),
]


@pytest.mark.parametrize("what,kw", BAD, ids=[w for w, _ in BAD])
def test_abi_refuses_bad_arguments(lib, what, kw):
    a = _Args(lib)
    _refused(lib, a.device(**kw), "device: " + what)
    _refused(lib, a.host(**kw), "host: " + what)


def test_refusal_order(lib):
    """The order of connected_components -- shape (BAD_ARG), connectivity (BAD_ARG), the size limit (UNSUPPORTED) -- then the two
    bounds (BAD_ARG), then pointers and the workspace (BAD_ARG): each is reported although everything after it is broken too."""
    a = _Args(lib)
    big = dict(sx=2048, sy=1024, sz=1024)
    for call, rest in ((a.device, dict(ws=None)), (a.host, {})):
        assert call(dtype=9, connectivity=0, lo=-1, labels=None, **big, **rest) == BAD_ARG and b"dtype" in lib.edt_hip_last_error()
        assert call(connectivity=0, lo=-1, labels=None, **big, **rest) == BAD_ARG and b"connectivity" in lib.edt_hip_last_error()
        assert call(lo=-1, labels=None, counts=None, **big, **rest) == UNSUPPORTED and b"2^31" in lib.edt_hip_last_error()
        assert call(lo=-1, hi=-2, labels=None, counts=None, **rest) == BAD_ARG and b"min_voxels must" in lib.edt_hip_last_error()
        assert call(lo=3, hi=2, labels=None, counts=None, **rest) == BAD_ARG and b"max_voxels must" in lib.edt_hip_last_error()
        assert call(labels=None, counts=None, **rest) == BAD_ARG and b"null" in lib.edt_hip_last_error()
        assert call(lo=4, hi=4, labels=None, **rest) == BAD_ARG and b"null" in lib.edt_hip_last_error()   # (an empty range is allowed)
    assert a.device(ws=None) == BAD_ARG and b"workspace" in lib.edt_hip_last_error()
    assert a.device(ws_bytes=a.ws.size - 1) == BAD_ARG and b"workspace" in lib.edt_hip_last_error()
    # an empty volume needs neither labels nor out; without a device the call then fails for want of one, not for an argument
    from edt import _lib
    if _lib.device_count() == 0:
        assert a.device(sx=0, labels=None, out=None, ws=None) == _lib.ERR_NO_DEVICE
        assert a.device() == _lib.ERR_NO_DEVICE and a.device(out=a.labels) == _lib.ERR_NO_DEVICE    # in place is no argument error
        assert a.host(out=a.labels) == _lib.ERR_NO_DEVICE
    counts = np.full(3, -1, dtype=np.int64)
    assert a.host(sx=0, labels=None, out=None, counts=counts) == 0 and counts.tolist() == [0, 0, 0]   # (the host form only zeroes the counts)
    assert a.host(sx=0, labels=None, out=None, lo=-1) == BAD_ARG


def test_workspace_query_and_size_limit(lib):
    q, fh = lib.edt_hip_dust_workspace_bytes, lib.edt_hip_fill_holes_workspace_bytes
    assert q(7, 3, 8, 8, 8) == 0 and q(-1, 3, 8, 8, 8) == 0
    assert q(U32, 4, 8, 8, 8) == 0 and q(U32, 0, 8, 1, 1) == 0
    assert q(U32, 2, 8, 8, 8) == 0 and q(U32, 1, 8, 8, 1) == 0 and q(U32, 3, -1, 8, 8) == 0
    for code in (U8, U16, U32, U64, F32, F64, BOOL):
        for shape in ((64, 64, 1), (64, 64, 8), (70, 12, 9), (512, 512, 512), (1, 1, 1)):
            assert q(code, 3, *shape) == fh(code, 3, *shape) > 0     # the parent plane and the per-chunk counts, and no more
    # sx * sy * sz <= 2^31 - 1: one voxel more is refused by the query and by both entry points, in 64-bit arithmetic
    assert q(U32, 3, 2048, 1024, 1024) == 0
    assert q(U32, 3, 2047, 1024, 1024) > 4 * 2047 * 1024 * 1024
    assert q(U8, 1, (1 << 31) - 1, 1, 1) > 0
    assert q(U8, 3, 65536, 65536, 2) == 0 and q(U8, 3, 1 << 30, 1 << 30, 1 << 30) == 0
    a = _Args(lib)
    _refused(lib, a.device(sx=2048, sy=1024, sz=1024), "device: 2^31 voxels", UNSUPPORTED)
    _refused(lib, a.host(sx=2048, sy=1024, sz=1024), "host: 2^31 voxels", UNSUPPORTED)
    _refused(lib, a.device(sx=1 << 30, sy=1 << 30, sz=1 << 30), "device: 2^90 voxels", UNSUPPORTED)
    _refused(lib, a.host(sx=65536, sy=65536, sz=2), "host: 2^33 voxels", UNSUPPORTED)


def test_header_exports_the_span_of_the_count_kernel():
    """The GPU tier lays a component across a boundary of the count kernel's span and reads the span from the header."""
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "edt_hip.h")).read()
    m = re.search(r"^#define EDT_HIP_DUST_COUNT_SPAN (\d+)$", text, flags=re.M)
    assert m and int(m.group(1)) % 256 == 0 and 1024 <= int(m.group(1)) <= 65536


# ---- the Python layer ------------------------------------------------------------------------------------------------
def test_python_argument_handling(monkeypatch):
    import edt
    from edt import _lib
    seen = []

    def no_library():
        seen.append(1)
        raise AssertionError("the library was touched")

    img, vol, line = np.ones((4, 5), dtype=np.uint8), np.ones((3, 4, 5), dtype=np.uint16), np.ones(7, dtype=np.uint32)
    with monkeypatch.context() as m:
        m.setattr(_lib, "load", no_library)
        for bad in (-1, 2.5, "4", None, True, (1,), (1, 2, 3), (3, 2), (-1, 4), (1, 2.0), 1 << 63, [5, 4], np.array([1, 2])):
            with pytest.raises(ValueError, match="dust"):
                edt.dust(vol, bad)
        for data, bad in ((img, (0, 5, 26, 3, 6, 18, -1, 2.5, "8", True)), (vol, (0, 5, 4, 8, 27)), (line, (0, 2, 4, 6))):
            for c in bad:
                with pytest.raises(ValueError, match="dust"):
                    edt.dust(data, 4, connectivity=c)
        with pytest.raises(TypeError):
            edt.dust(np.ones((2, 2, 2, 2), dtype=np.uint8), 4)
        with pytest.raises(TypeError):
            edt.dust(np.uint8(3), 4)
        with pytest.raises(TypeError):
            edt.dust(np.ones((4, 5), dtype=np.complex64), 4)
        # empty input: a copy, zero counts
        for shape in ((0,), (3, 0), (0, 2, 5)):
            for dtype in (np.float32, bool, np.int16):
                src = np.zeros(shape, dtype=dtype)
                out, counts = edt.dust(src, 4, return_counts=True)
                assert out.shape == shape and out.dtype == src.dtype and out is not src
                assert counts == edt.DustCounts(0, 0, 0) and counts.removed_voxels == 0
                assert edt.dust(src, (2, 9), invert=True).shape == shape
    assert not seen
    called = []
    with monkeypatch.context() as m:
        class Lib:
            @staticmethod
            def edt_hip_dust(labels, code, nd, sx, sy, sz, c, binary, lo, hi, invert, out, counts):
                called.append((code, nd, sx, sy, sz, c, binary, lo, hi, invert))
                ctypes.cast(counts, ctypes.POINTER(ctypes.c_int64))[2] = 11
                return 0
        m.setattr(_lib, "load", lambda: Lib)
        edt.dust(vol, 4)                                             # C order: x is the last axis; None is full connectivity
        edt.dust(np.asfortranarray(vol), (3, 9), connectivity=18, binary=True, invert=True)
        edt.dust(img.astype(np.int8), np.int64(0), connectivity=4)
        out, counts = edt.dust(line.astype(bool), [2, 2], return_counts=True)
    assert called == [(U16, 3, 5, 4, 3, 3, 0, 4, INT64_MAX, 0), (U16, 3, 3, 4, 5, 2, 1, 3, 9, 1),
                      (U8, 2, 5, 4, 1, 1, 0, 0, INT64_MAX, 0), (BOOL, 1, 7, 1, 1, 1, 0, 2, 2, 0)]
    assert counts == (0, 0, 11) and all(type(v) is int for v in counts) and out.dtype == np.bool_ and out.shape == (7,)
    if _lib.device_count() == 0:
        for data, c in ((img, 4), (img, None), (vol, 6), (vol, 26), (line, 1)):
            with pytest.raises(_lib.EdtHipError) as e:
                edt.dust(data, 4, connectivity=c)
            assert e.value.code == _lib.ERR_NO_DEVICE
