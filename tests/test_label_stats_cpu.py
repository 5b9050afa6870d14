"""CPU tier of label_stats: the public surface, argument validation of the three ABI functions (all of it happens before
any device work, so no device is needed), and the numpy oracle against a brute-force loop over labels."""
import ctypes

import numpy as np
import pytest

import label_stats_oracle as oracle
from synth import blocky_labels

BAD_ARG = -2
U8, U16, U32, U64, F32, F64, BOOL = range(7)


@pytest.fixture(scope="module")
def lib():
    from edt import _lib
    return _lib.load()


def test_public_surface():
    import edt
    assert "label_stats" in edt.__all__ and callable(edt.label_stats)
    from edt import _lib
    for name in ("edt_hip_label_stats_workspace_bytes", "edt_hip_label_stats_device", "edt_hip_label_stats"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)


class _Args:
    """A valid argument set of both entry points over host stand-ins: every case below breaks exactly one item, and
    validation returns before anything is dereferenced."""

    def __init__(self, lib):
        self.lib = lib
        self.labels = np.ones(24, dtype=np.uint32)
        self.dt = np.ones(24, dtype=np.float32)
        self.keys = np.zeros(8, dtype=np.uint32)
        self.counts, self.arg = np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64)
        self.max, self.bbox = np.zeros(8, dtype=np.float32), np.zeros(48, dtype=np.int32)
        self.n = np.zeros(1, dtype=np.int64)
        self.ws = np.zeros(lib.edt_hip_label_stats_workspace_bytes(U32, 24, 8), dtype=np.uint8)

    @staticmethod
    def p(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    def device(self, **kw):
        a = dict(labels=self.labels, dtype=U32, dt=self.dt, ndim=3, sx=4, sy=3, sz=2, max_labels=8, keys=self.keys,
                 counts=self.counts, max=self.max, arg=self.arg, bbox=self.bbox, n=self.n, ws=self.ws, ws_bytes=None)
        a.update(kw)
        wb = (0 if a["ws"] is None else a["ws"].size) if a["ws_bytes"] is None else a["ws_bytes"]
        p = self.p
        return self.lib.edt_hip_label_stats_device(p(a["labels"]), a["dtype"], p(a["dt"]), a["ndim"], a["sx"], a["sy"], a["sz"],
                                                   a["max_labels"], p(a["keys"]), p(a["counts"]), p(a["max"]), p(a["arg"]),
                                                   p(a["bbox"]), p(a["n"]), p(a["ws"]), wb, None)

    def host(self, **kw):
        a = dict(labels=self.labels, dtype=U32, ndim=3, sx=4, sy=3, sz=2, w=(1.0, 1.0, 1.0), dt=self.dt, max_labels=8,
                 keys=self.keys, counts=self.counts, max=self.max, arg=self.arg, bbox=self.bbox, n=self.n)
        a.update(kw)
        p = self.p
        return self.lib.edt_hip_label_stats(p(a["labels"]), a["dtype"], a["ndim"], a["sx"], a["sy"], a["sz"], *a["w"], 0,
                                            p(a["dt"]), a["max_labels"], p(a["keys"]), p(a["counts"]), p(a["max"]),
                                            p(a["arg"]), p(a["bbox"]), p(a["n"]))


def _refused(lib, rc, what):
    assert rc == BAD_ARG, (what, rc)
    assert lib.edt_hip_last_error(), what


SHARED_BAD = [
    ("unknown dtype", dict(dtype=7)), ("negative dtype", dict(dtype=-1)),
    ("ndim 0", dict(ndim=0)), ("ndim 4", dict(ndim=4)),
    ("unused sz", dict(ndim=2)), ("unused sy", dict(ndim=1, sz=1)),
    ("max_labels 0", dict(max_labels=0)), ("max_labels negative", dict(max_labels=-3)),
    ("null labels", dict(labels=None)), ("null keys", dict(keys=None)), ("null counts", dict(counts=None)),
    ("null max", dict(max=None)), ("null argmax", dict(arg=None)), ("null bbox", dict(bbox=None)),
    ("null n_labels", dict(n=None)),
]


@pytest.mark.parametrize("what,kw", SHARED_BAD, ids=[w for w, _ in SHARED_BAD])
def test_abi_refuses_bad_arguments(lib, what, kw):
    a = _Args(lib)
    _refused(lib, a.device(**kw), "device: " + what)
    _refused(lib, a.host(**kw), "host: " + what)


def test_device_form_refuses_missing_field_and_workspace(lib):
    a = _Args(lib)
    _refused(lib, a.device(dt=None), "null dt")
    _refused(lib, a.device(ws=None), "no workspace")
    _refused(lib, a.device(ws_bytes=a.ws.size - 1), "workspace one byte short")
    # the workspace must cover the max_labels of the CALL
    small = np.zeros(lib.edt_hip_label_stats_workspace_bytes(U32, 1 << 20, 8), dtype=np.uint8)
    _refused(lib, a.device(sx=1024, sy=1024, sz=1, ndim=2, max_labels=1 << 16, ws=small), "workspace of a smaller call")


@pytest.mark.parametrize("w", [(0.0, 1.0, 1.0), (-1.0, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, float("inf")),
                               (1.0, 0.0, 1.0)])
def test_host_form_applies_the_voxel_size_rules_when_it_computes_the_field(lib, w):
    a = _Args(lib)
    _refused(lib, a.host(dt=None, w=w), w)


def test_workspace_query(lib):
    q = lib.edt_hip_label_stats_workspace_bytes
    assert q(7, 1000, 10) == 0 and q(-1, 1000, 10) == 0
    assert q(U32, 1000, 0) == 0 and q(U32, -1, 10) == 0
    for code in (U8, U16, U32, U64, F32, F64, BOOL):
        sizes = [q(code, 1 << 30, m) for m in (1, 2, 100, 1000, 65536, 1 << 20, 1 << 24)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (code, sizes)
    # hashed tables: at least 2 slots of 52 bytes per label and the 8-byte list entry
    for code in (U32, U64, F32, F64):
        for m in (65536, 1 << 20):
            assert q(code, 1 << 30, m) >= m * (2 * 52 + 8)
        assert q(code, 1 << 30, 1 << 20) > q(code, 1 << 30, 65536) > q(code, 1 << 30, 1000)
    # no more labels than voxels: room beyond that costs nothing
    assert q(U32, 5000, 1 << 30) == q(U32, 5000, 5000)


def test_python_argument_checks():
    import edt
    with pytest.raises(TypeError):
        edt.label_stats(np.ones((2, 2, 2, 2), dtype=np.uint8))
    lab = np.ones((4, 5), dtype=np.uint16)
    with pytest.raises(ValueError):
        edt.label_stats(lab, np.ones((5, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        edt.label_stats(lab, np.ones((4, 5), dtype=np.float64))
    with pytest.raises(ValueError):
        edt.label_stats(lab, np.ones((4, 5), dtype=np.float32), max_labels=0)
    with pytest.raises(ValueError):
        edt.label_stats(lab, max_labels=0)
    with pytest.raises(ValueError):
        edt.label_stats(lab, anisotropy=(1.0, 0.0))
    with pytest.raises(TypeError):
        edt.label_stats(np.ones((4, 5), dtype=np.complex64))


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.uint32, np.int64, np.float32, np.float64, bool])
@pytest.mark.parametrize("shape", [(0,), (3, 0), (0, 2, 5)])
def test_empty_input_gives_an_empty_table(dtype, shape):
    import edt
    nd = len(shape)
    for dt in (None, np.zeros(shape, dtype=np.float32)):
        got = edt.label_stats(np.zeros(shape, dtype=dtype), dt)
        assert got._fields == ("labels", "counts", "max", "argmax", "bbox_lo", "bbox_hi")
        assert got.labels.dtype == np.dtype(dtype) and got.labels.shape == (0,)
        assert got.counts.dtype == np.int64 and got.counts.shape == (0,)
        assert got.max.dtype == np.float32 and got.max.shape == (0,)
        assert got.argmax.dtype == np.int64 and got.argmax.shape == (0, nd)
        assert got.bbox_lo.dtype == np.int32 and got.bbox_lo.shape == (0, nd)
        assert got.bbox_hi.dtype == np.int32 and got.bbox_hi.shape == (0, nd)


def test_oracle_against_brute_force():
    rng = np.random.default_rng(11)
    vols = [blocky_labels((7, 5, 6), nlabels=4, zero_frac=0.3, block=2, rng=rng).astype(np.int16) - 2,
            blocky_labels((9, 8), nlabels=6, zero_frac=0.2, block=3, rng=rng).astype(np.uint64) << np.uint64(40),
            blocky_labels((5, 4, 3), nlabels=3, zero_frac=0.2, block=2, rng=rng).astype(np.float32) - 1.5]
    vols[2][0, 0, 0] = np.nan
    vols[2][1, 1, 1] = -0.0
    for lab in vols:
        dt = rng.integers(-2, 3, size=lab.shape).astype(np.float32)   # many ties
        dt[rng.random(lab.shape) < 0.1] = np.inf
        for data, field in ((lab, dt), (np.asfortranarray(lab), np.asfortranarray(dt))):
            got, want = oracle.label_stats(data, field), oracle.brute_force(data, field)
            assert len(want.labels) > 1
            oracle.assert_same(got, want, (lab.dtype, data.flags.f_contiguous))
    # ties follow MEMORY order: one label, one value everywhere -- the first voxel either way; a maximum at two places
    lab = np.ones((3, 4), dtype=np.uint8)
    dt = np.zeros((3, 4), dtype=np.float32)
    dt[0, 2] = dt[1, 0] = 5.0
    assert oracle.label_stats(lab, dt).argmax.tolist() == [[0, 2]]
    assert oracle.label_stats(np.asfortranarray(lab), np.asfortranarray(dt)).argmax.tolist() == [[1, 0]]
