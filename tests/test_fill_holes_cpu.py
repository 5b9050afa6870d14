"""CPU tier of fill_holes: the public surface, argument validation of the ABI functions (all of it happens before any device
work, so no device is needed), the Python argument handling, and the numpy oracle against scipy.ndimage.binary_fill_holes
and against a brute-force flood fill from the boundary."""
import ctypes

import numpy as np
import pytest

import fill_holes_oracle as oracle

BAD_ARG, UNSUPPORTED = -2, -4
U8, U16, U32, U64, F32, F64, BOOL = range(7)
NAMES = ("edt_hip_fill_holes_workspace_bytes", "edt_hip_fill_holes_device", "edt_hip_fill_holes")


@pytest.fixture(scope="module")
def lib():
    from edt import _lib
    return _lib.load()


def test_public_surface():
    import edt
    assert "fill_holes" in edt.__all__ and callable(edt.fill_holes)
    from edt import _lib, device
    assert callable(device.fill_holes)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)


class _Args:
    """A valid argument set of both entry points over host stand-ins: every case below breaks exactly one item, and
    validation returns before anything is dereferenced."""

    def __init__(self, lib):
        self.lib = lib
        self.labels = np.ones(24, dtype=np.uint32)
        self.out = np.zeros(24, dtype=np.uint32)
        self.n = np.zeros(1, dtype=np.int64)
        self.ws = np.zeros(lib.edt_hip_fill_holes_workspace_bytes(U32, 3, 4, 3, 2), dtype=np.uint8)

    @staticmethod
    def p(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    def device(self, **kw):
        a = dict(labels=self.labels, dtype=U32, ndim=3, sx=4, sy=3, sz=2, connectivity=1, binary=0, out=self.out, n=self.n,
                 ws=self.ws, ws_bytes=None)
        a.update(kw)
        wb = (0 if a["ws"] is None else a["ws"].size) if a["ws_bytes"] is None else a["ws_bytes"]
        p = self.p
        return self.lib.edt_hip_fill_holes_device(p(a["labels"]), a["dtype"], a["ndim"], a["sx"], a["sy"], a["sz"],
                                                  a["connectivity"], a["binary"], p(a["out"]), p(a["n"]), p(a["ws"]), wb, None)

    def host(self, **kw):
        a = dict(labels=self.labels, dtype=U32, ndim=3, sx=4, sy=3, sz=2, connectivity=1, binary=0, out=self.out, n=self.n)
        a.update(kw)
        p = self.p
        return self.lib.edt_hip_fill_holes(p(a["labels"]), a["dtype"], a["ndim"], a["sx"], a["sy"], a["sz"], a["connectivity"],
                                           a["binary"], p(a["out"]), p(a["n"]))


def _refused(lib, rc, what, code=BAD_ARG):
    assert rc == code, (what, rc)
    assert lib.edt_hip_last_error(), what


SHARED_BAD = [
    ("unknown dtype", dict(dtype=7)), ("negative dtype", dict(dtype=-1)),
    ("ndim 0", dict(ndim=0)), ("ndim 4", dict(ndim=4)),
    ("unused sz", dict(ndim=2, connectivity=2)), ("unused sy", dict(ndim=1, sz=1, connectivity=1)),
    ("connectivity 0", dict(connectivity=0)), ("connectivity negative", dict(connectivity=-1)),
    ("connectivity 4", dict(connectivity=4)), ("connectivity 26", dict(connectivity=26)),
    ("connectivity 3 in 2-D", dict(ndim=2, sz=1, connectivity=3)), ("connectivity 2 in 1-D", dict(ndim=1, sy=1, sz=1, connectivity=2)),
    ("null labels", dict(labels=None)), ("null out", dict(out=None)), ("null n_filled", dict(n=None)),
]


@pytest.mark.parametrize("what,kw", SHARED_BAD, ids=[w for w, _ in SHARED_BAD])
def test_abi_refuses_bad_arguments(lib, what, kw):
    a = _Args(lib)
    _refused(lib, a.device(**kw), "device: " + what)
    _refused(lib, a.host(**kw), "host: " + what)


def test_output_may_not_alias_the_labels(lib):
    a = _Args(lib)
    _refused(lib, a.device(out=a.labels), "device: out is labels")
    _refused(lib, a.host(out=a.labels), "host: out is labels")


def test_refusal_order(lib):
    """As connected_components: shape (BAD_ARG), connectivity (BAD_ARG), the size limit (UNSUPPORTED), pointers and the
    workspace (BAD_ARG) -- each is reported although everything after it is broken too."""
    a = _Args(lib)
    big = dict(sx=2048, sy=1024, sz=1024)
    for call, rest in ((a.device, dict(ws=None)), (a.host, {})):
        assert call(dtype=9, connectivity=0, labels=None, **big, **rest) == BAD_ARG and b"dtype" in lib.edt_hip_last_error()
        assert call(connectivity=0, labels=None, **big, **rest) == BAD_ARG and b"connectivity" in lib.edt_hip_last_error()
        assert call(labels=None, n=None, **big, **rest) == UNSUPPORTED and b"2^31" in lib.edt_hip_last_error()
        assert call(labels=None, n=None, **rest) == BAD_ARG and b"null" in lib.edt_hip_last_error()
    assert a.device(labels=None, ws=None) == BAD_ARG and b"null" in lib.edt_hip_last_error()
    assert a.device(ws=None) == BAD_ARG and b"workspace" in lib.edt_hip_last_error()
    # an empty volume needs neither labels nor out; without a device the call then fails for want of one, not for an argument
    from edt import _lib
    if _lib.device_count() == 0:
        assert a.device(sx=0, labels=None, out=None, ws=None) == _lib.ERR_NO_DEVICE
    n = np.full(1, -1, dtype=np.int64)
    assert a.host(sx=0, labels=None, out=None, n=n) == 0 and n[0] == 0          # (the host form only sets the count)


def test_device_form_refuses_a_missing_or_small_workspace(lib):
    a = _Args(lib)
    _refused(lib, a.device(ws=None), "no workspace")
    _refused(lib, a.device(ws_bytes=a.ws.size - 1), "workspace one byte short")
    _refused(lib, a.device(sx=1 << 20, sy=64, sz=1, ndim=2, connectivity=2), "workspace of a smaller call")


def test_workspace_query(lib):
    q = lib.edt_hip_fill_holes_workspace_bytes
    assert q(7, 3, 8, 8, 8) == 0 and q(-1, 3, 8, 8, 8) == 0
    assert q(U32, 4, 8, 8, 8) == 0 and q(U32, 0, 8, 1, 1) == 0
    assert q(U32, 2, 8, 8, 8) == 0 and q(U32, 1, 8, 8, 1) == 0 and q(U32, 3, -1, 8, 8) == 0
    for code in (U8, U16, U32, U64, F32, F64, BOOL):
        sizes = [q(code, 3, 64, 64, s) for s in (1, 8, 64, 512)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (code, sizes)
    # the parent plane and the per-chunk counts: 4 bytes per voxel and a little, whatever the label width
    v = 512 ** 3
    assert 4 * v <= q(U64, 3, 512, 512, 512) == q(U8, 3, 512, 512, 512) < 4 * v + v // 64


def test_size_limit(lib):
    """sx * sy * sz <= 2^31 - 1 (parents are 32-bit and a root's top bit tags its state): one voxel more is refused, by the
    query and by both entry points, before any device work -- in 64-bit arithmetic."""
    q = lib.edt_hip_fill_holes_workspace_bytes
    assert q(U32, 3, 2048, 1024, 1024) == 0
    assert q(U32, 3, 2047, 1024, 1024) > 4 * 2047 * 1024 * 1024
    assert q(U8, 1, (1 << 31) - 1, 1, 1) > 0
    assert q(U8, 3, 65536, 65536, 2) == 0 and q(U8, 3, 1 << 30, 1 << 30, 1 << 30) == 0     # (products past 2^32, 2^64)
    a = _Args(lib)
    _refused(lib, a.device(sx=2048, sy=1024, sz=1024), "device: 2^31 voxels", UNSUPPORTED)
    _refused(lib, a.host(sx=2048, sy=1024, sz=1024), "host: 2^31 voxels", UNSUPPORTED)
    _refused(lib, a.device(sx=1 << 30, sy=1 << 30, sz=1 << 30), "device: 2^90 voxels", UNSUPPORTED)
    _refused(lib, a.host(sx=65536, sy=65536, sz=2), "host: 2^33 voxels", UNSUPPORTED)


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
        for data, bad in ((img, (0, 5, 26, 3, 6, 18, -1, 2.5, "8", True)), (vol, (0, 5, 4, 8, 27)), (line, (0, 2, 4, 6))):
            for c in bad:
                with pytest.raises(ValueError, match="fill_holes"):
                    edt.fill_holes(data, connectivity=c)
        with pytest.raises(TypeError):
            edt.fill_holes(np.ones((2, 2, 2, 2), dtype=np.uint8))
        with pytest.raises(TypeError):
            edt.fill_holes(np.ones((4, 5), dtype=np.complex64))
        # empty input: a copy, nothing filled
        for shape in ((0,), (3, 0), (0, 2, 5)):
            for dtype in (np.float32, bool, np.int16):
                src = np.zeros(shape, dtype=dtype)
                out, n = edt.fill_holes(src, return_fill_count=True)
                assert out.shape == shape and out.dtype == src.dtype and out is not src and n == 0
                assert edt.fill_holes(src).shape == shape
    assert not seen
    # None is connectivity 1 here -- not the full connectivity it means for connected_components -- and both spellings pass
    from edt import _connectivity

    def conn(c, nd):
        return _connectivity(c, nd, default=1, who="fill_holes")

    assert [conn(c, 2) for c in (None, 1, 2, 4, 8)] == [1, 1, 2, 1, 2]
    assert [conn(c, 3) for c in (None, 1, 2, 3, 6, 18, 26)] == [1, 1, 2, 3, 1, 2, 3]
    assert [conn(c, 1) for c in (None, 1)] == [1, 1]
    assert _connectivity(None, 3) == 3                           # connected_components keeps its default
    called = []
    with monkeypatch.context() as m:
        class Lib:
            @staticmethod
            def edt_hip_fill_holes(labels, code, nd, sx, sy, sz, c, binary, out, n):
                called.append((code, nd, sx, sy, sz, c, binary))
                return 0
        m.setattr(_lib, "load", lambda: Lib)
        edt.fill_holes(vol)                                      # C order: x is the last axis
        edt.fill_holes(np.asfortranarray(vol), connectivity=18, binary=True)
        edt.fill_holes(img.astype(np.int8), connectivity=8)
        edt.fill_holes(line.astype(bool))
    assert called == [(U16, 3, 5, 4, 3, 1, 0), (U16, 3, 3, 4, 5, 2, 1), (U8, 2, 5, 4, 1, 2, 0), (BOOL, 1, 7, 1, 1, 1, 0)]
    if _lib.device_count() == 0:
        for data, c in ((img, 4), (img, None), (vol, 6), (vol, 26), (line, 1)):
            with pytest.raises(_lib.EdtHipError) as e:
                edt.fill_holes(data, connectivity=c)
            assert e.value.code == _lib.ERR_NO_DEVICE


SCIPY_SHAPES = ((7, 6, 5), (9, 1, 8), (12, 11), (30,), (1, 9, 9), (8, 8, 8))


@pytest.mark.parametrize("shape", SCIPY_SHAPES, ids=[str(s) for s in SCIPY_SHAPES])
def test_oracle_against_scipy(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(sum(shape))
    nd = len(shape)
    filled_something = 0
    for density in (0.5, 0.7, 0.85):
        for trial in range(5):
            mask = rng.random(shape) < density
            lab = (mask * rng.integers(1, 4, size=shape)).astype(np.uint16)
            for c in range(1, nd + 1):
                want = ndi.binary_fill_holes(mask, structure=ndi.generate_binary_structure(nd, c))
                for data in (mask, np.asfortranarray(mask)):
                    got = oracle.fill_holes(data, c)
                    assert np.array_equal(got.out, want), (shape, density, c)
                    assert got.n_filled == int(want.sum() - mask.sum()) and got.mixed_cavities == 0
                    assert got.cavities == got.filled_cavities
                    filled_something += got.n_filled
                # multi-label under binary: the same voxels; without: a subset, and only 0 -> a wall label
                b = oracle.fill_holes(lab, c, binary=True)
                assert np.array_equal(b.out != 0, want) and np.array_equal(b.out[mask], lab[mask])
                m = oracle.fill_holes(lab, c)
                assert np.array_equal(m.out[mask], lab[mask]) and not np.any((m.out != 0) & ~want)
                assert m.cavities == b.cavities == m.filled_cavities + m.mixed_cavities
                changed = m.out != lab
                assert np.array_equal(m.out[changed], b.out[changed]) and int(changed.sum()) == m.n_filled
    if nd == 3 and 1 in shape:
        assert filled_something == 0                             # an axis of extent 1: every voxel is on the boundary
    else:
        assert filled_something > 0


def test_oracle_against_brute_force():
    rng = np.random.default_rng(7)
    vols = []
    for shape in ((10, 10, 10), (12, 9, 8), (31, 30), (40,), (9, 1, 9), (2, 9, 9)):
        for trial in range(3):
            vols.append((rng.integers(1, 3, size=shape) * (rng.random(shape) < 0.8)).astype(np.uint8))
    f = vols[0].astype(np.float32)
    f[f == 2] = np.nan
    z = np.argwhere(f == 0)
    f[tuple(z[::2].T)] = -0.0
    vols += [f, f.astype(np.float64), vols[1] != 0, vols[3].astype(np.uint64) << np.uint64(33),
             (vols[4].astype(np.uint64) << np.uint64(32)) + (vols[4] != 0), -vols[5].astype(np.int16)]
    mixed = filled = 0
    for lab in vols:
        for data in (lab, np.asfortranarray(lab)):
            for c in range(1, lab.ndim + 1):
                for binary in (False, True):
                    got = oracle.fill_holes(data, c, binary=binary)
                    want = oracle.brute_force(data, c, binary=binary)
                    assert got[1:] == want[1:], (lab.dtype, lab.shape, c, binary, got[1:], want[1:])
                    assert got.out.tobytes(order="A") == want.out.tobytes(order="A")      # (NaN and -0.0: bit for bit)
                    assert got.out.flags.f_contiguous == data.flags.f_contiguous
                    mixed += got.mixed_cavities
                    filled += got.filled_cavities
    assert mixed > 20 and filled > 20
    # the contract's special values
    nan = np.float32(np.nan)
    line = np.array([1, -0.0, 1, 0, 2, 2, 0, nan, nan, 0, nan, 0], dtype=np.float32)
    got = oracle.fill_holes(line)
    assert got.out[:7].tolist() == [1, 1, 1, 0, 2, 2, 0] and got.out[9] == 0 and (got.n_filled, got.mixed_cavities) == (1, 3)
    got = oracle.fill_holes(line, binary=True)
    assert got.out[:7].tolist() == [1, 1, 1, 1, 2, 2, 2] and np.isnan(got.out[9]) and got.out[11] == 0 and got.n_filled == 4
    assert oracle.fill_holes(np.zeros((5, 5)), 1).n_filled == 0 and oracle.fill_holes(np.ones((5, 5)), 2).cavities == 0


def test_blocky_volumes_have_cavities_of_both_kinds():
    """The random volumes of the GPU tier (tests/test_gpu_fill_holes.py) on the CPU: enough cavities, filled and mixed, at
    every connectivity for the comparison there to mean something."""
    for seed in range(5):
        lab = oracle.random_volume(seed)
        for c in (1, 2, 3):
            got = oracle.fill_holes(lab, c)
            assert got.cavities >= 20 and got.filled_cavities >= 5 and got.mixed_cavities >= 5, (seed, c, got[1:])
