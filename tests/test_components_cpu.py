"""CPU tier of connected_components: the public surface, argument validation of the ABI functions (all of it happens before
any device work, so no device is needed), the Python argument handling, and the numpy oracle against scipy.ndimage.label and
against a brute-force flood fill."""
import ctypes

import numpy as np
import pytest

import components_oracle as oracle
from synth import blocky_labels

BAD_ARG, UNSUPPORTED = -2, -4
U8, U16, U32, U64, F32, F64, BOOL = range(7)
NAMES = ("edt_hip_components_workspace_bytes", "edt_hip_connected_components_device", "edt_hip_connected_components")


@pytest.fixture(scope="module")
def lib():
    from edt import _lib
    return _lib.load()


def test_public_surface():
    import edt
    assert "connected_components" in edt.__all__ and callable(edt.connected_components)
    from edt import _lib
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
        self.ws = np.zeros(lib.edt_hip_components_workspace_bytes(U32, 3, 4, 3, 2), dtype=np.uint8)

    @staticmethod
    def p(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    def device(self, **kw):
        a = dict(labels=self.labels, dtype=U32, ndim=3, sx=4, sy=3, sz=2, connectivity=3, binary=0, out=self.out, n=self.n,
                 ws=self.ws, ws_bytes=None)
        a.update(kw)
        wb = (0 if a["ws"] is None else a["ws"].size) if a["ws_bytes"] is None else a["ws_bytes"]
        p = self.p
        return self.lib.edt_hip_connected_components_device(p(a["labels"]), a["dtype"], a["ndim"], a["sx"], a["sy"], a["sz"],
                                                            a["connectivity"], a["binary"], p(a["out"]), p(a["n"]), p(a["ws"]),
                                                            wb, None)

    def host(self, **kw):
        a = dict(labels=self.labels, dtype=U32, ndim=3, sx=4, sy=3, sz=2, connectivity=3, binary=0, out=self.out, n=self.n)
        a.update(kw)
        p = self.p
        return self.lib.edt_hip_connected_components(p(a["labels"]), a["dtype"], a["ndim"], a["sx"], a["sy"], a["sz"],
                                                     a["connectivity"], a["binary"], p(a["out"]), p(a["n"]))


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
    ("null labels", dict(labels=None)), ("null out", dict(out=None)), ("null n", dict(n=None)),
]


@pytest.mark.parametrize("what,kw", SHARED_BAD, ids=[w for w, _ in SHARED_BAD])
def test_abi_refuses_bad_arguments(lib, what, kw):
    a = _Args(lib)
    _refused(lib, a.device(**kw), "device: " + what)
    _refused(lib, a.host(**kw), "host: " + what)


def test_device_form_refuses_a_missing_or_small_workspace(lib):
    a = _Args(lib)
    _refused(lib, a.device(ws=None), "no workspace")
    _refused(lib, a.device(ws_bytes=a.ws.size - 1), "workspace one byte short")
    # the workspace must cover the volume of the CALL
    _refused(lib, a.device(sx=1 << 20, sy=64, sz=1, ndim=2, connectivity=2), "workspace of a smaller call")


def test_workspace_query(lib):
    q = lib.edt_hip_components_workspace_bytes
    assert q(7, 3, 8, 8, 8) == 0 and q(-1, 3, 8, 8, 8) == 0
    assert q(U32, 4, 8, 8, 8) == 0 and q(U32, 0, 8, 1, 1) == 0
    assert q(U32, 2, 8, 8, 8) == 0 and q(U32, 1, 8, 8, 1) == 0 and q(U32, 3, -1, 8, 8) == 0
    for code in (U8, U16, U32, U64, F32, F64, BOOL):
        sizes = [q(code, 3, 64, 64, s) for s in (1, 8, 64, 512)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (code, sizes)
    # nothing per voxel but the per-chunk counts of the numbering scan: far below one byte per voxel
    assert q(U32, 3, 512, 512, 512) < (512 ** 3) // 64


def test_size_limit(lib):
    """sx * sy * sz <= 2^31 - 1 (parents and numbers are 32-bit): one voxel more is refused, by the query and by both entry
    points, before any device work -- in 64-bit arithmetic (2048 * 1024 * 1024 = 2^31 wraps to a negative int32)."""
    q = lib.edt_hip_components_workspace_bytes
    assert q(U32, 3, 2048, 1024, 1024) == 0
    assert q(U32, 3, 2047, 1024, 1024) > 0
    assert q(U8, 1, (1 << 31) - 1, 1, 1) > 0
    assert q(U8, 3, 65536, 65536, 2) == 0 and q(U8, 3, 1 << 30, 1 << 30, 1 << 30) == 0     # (products past 2^32, 2^64)
    a = _Args(lib)
    _refused(lib, a.device(sx=2048, sy=1024, sz=1024), "device: 2^31 voxels", UNSUPPORTED)
    _refused(lib, a.host(sx=2048, sy=1024, sz=1024), "host: 2^31 voxels", UNSUPPORTED)
    _refused(lib, a.device(sx=1 << 30, sy=1 << 30, sz=1 << 30), "device: 2^90 voxels", UNSUPPORTED)


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
        for data, bad in ((img, (0, 5, 26, 3, 6, 18, -1, 2.5, "8")), (vol, (0, 5, 4, 8, 27)), (line, (0, 2, 4, 6))):
            for c in bad:
                with pytest.raises(ValueError):
                    edt.connected_components(data, connectivity=c)
        with pytest.raises(TypeError):
            edt.connected_components(np.ones((2, 2, 2, 2), dtype=np.uint8))
        with pytest.raises(TypeError):
            edt.connected_components(np.ones((4, 5), dtype=np.complex64))
        # empty input: an empty uint32 array, N = 0
        for shape in ((0,), (3, 0), (0, 2, 5)):
            out, n = edt.connected_components(np.zeros(shape, dtype=np.float32), return_N=True)
            assert out.shape == shape and out.dtype == np.uint32 and n == 0
            assert edt.connected_components(np.zeros(shape, dtype=bool)).shape == shape
    assert not seen
    # both spellings of connectivity are accepted: they pass the Python layer (without a device the library then refuses)
    from edt import connected_components as cc
    from edt import _connectivity
    assert [_connectivity(c, 2) for c in (None, 1, 2, 4, 8)] == [2, 1, 2, 1, 2]
    assert [_connectivity(c, 3) for c in (None, 1, 2, 3, 6, 18, 26)] == [3, 1, 2, 3, 1, 2, 3]
    assert [_connectivity(c, 1) for c in (None, 1)] == [1, 1]
    if _lib.device_count() == 0:
        for data, c in ((img, 4), (img, 8), (img, 1), (vol, 6), (vol, 18), (vol, 26), (vol, 2), (line, 1)):
            with pytest.raises(_lib.EdtHipError) as e:
                cc(data, connectivity=c)
            assert e.value.code == _lib.ERR_NO_DEVICE


def _first_index_renumbered(parts, order):
    """Per-label component images (disjoint supports, own numbering each) -> one image numbered by first memory index."""
    comp = np.zeros(parts[0][0].shape, dtype=np.int64, order=order)
    base = 0
    for part, n in parts:
        comp = np.where(part > 0, part + base, comp)
        base += n
    flat = comp.reshape(-1, order=order)
    ids, first = np.unique(flat, return_index=True)
    ids, first = ids[ids > 0], first[ids > 0]
    rank = np.zeros(base + 1, dtype=np.uint32)
    rank[ids[np.argsort(first)]] = np.arange(1, len(ids) + 1)
    return rank[comp].astype(np.uint32), len(ids)


@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_oracle_against_scipy(ndim):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(100 + ndim)
    for trial in range(12):
        shape = tuple(int(s) for s in rng.integers(1, (40, 14, 9)[ndim - 1] + 1, size=ndim))
        lab = blocky_labels(shape, nlabels=3, zero_frac=0.35, block=int(rng.integers(1, 4)), rng=rng).astype(np.uint16)
        for c in range(1, ndim + 1):
            st = ndi.generate_binary_structure(ndim, c)
            # binary, C order: scipy's own numbering
            want, n = ndi.label(lab != 0, structure=st)
            got, gn = oracle.connected_components(lab, c, binary=True, return_N=True)
            assert gn == n and np.array_equal(got, want), (shape, c)
            # multi-label: label() of every value, renumbered by first index
            parts = [ndi.label(lab == v, structure=st) for v in np.unique(lab[lab != 0])]
            if parts:
                want, n = _first_index_renumbered(parts, "C")
                got, gn = oracle.connected_components(lab, c, return_N=True)
                assert gn == n and np.array_equal(got, want), (shape, c)
            # F order: the same partition, numbered along the other memory order
            labf = np.asfortranarray(lab)
            gotf, gnf = oracle.connected_components(labf, c, binary=True, return_N=True)
            wantf, nf = ndi.label(np.ascontiguousarray((lab != 0).T), structure=st)
            assert gnf == nf and np.array_equal(gotf, wantf.T), (shape, c)


def test_oracle_against_flood_fill():
    rng = np.random.default_rng(7)
    vols = []
    for shape in ((6, 5, 4), (5, 6), (9,), (1, 4, 3), (6, 1, 1), (2, 2, 2)):
        for trial in range(4):
            vols.append(rng.integers(0, 3, size=shape).astype(np.uint8))
    f = rng.integers(0, 3, size=(5, 4, 3)).astype(np.float32)
    f[0, 0, 0] = f[0, 0, 1] = f[2, 2, 1] = np.nan
    f[1, 1, 1] = -0.0
    vols += [f, f.astype(np.float64), rng.integers(0, 2, size=(4, 5, 3)).astype(bool),
             (rng.integers(0, 3, size=(4, 3, 5)).astype(np.uint64) << np.uint64(33))]
    for lab in vols:
        for data in (lab, np.asfortranarray(lab)):
            for c in range(1, lab.ndim + 1):
                for binary in (False, True):
                    got, gn = oracle.connected_components(data, c, binary=binary, return_N=True)
                    want, n = oracle.flood_fill(data, c, binary=binary)
                    assert gn == n and np.array_equal(got, want), (lab.dtype, lab.shape, c, binary)
    # the contract's special values: -0.0 is background, a NaN voxel is a component of its own, under binary it joins
    out, n = oracle.connected_components(np.array([np.nan, np.nan, -0.0, 2.0, 2.0], dtype=np.float32), return_N=True)
    assert out.tolist() == [1, 2, 0, 3, 3] and n == 3
    assert oracle.connected_components(np.array([np.nan, np.nan, 1.0, -0.0, 2.0]), binary=True).tolist() == [1, 1, 1, 0, 2]
