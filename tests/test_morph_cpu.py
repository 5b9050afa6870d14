"""CPU tier of the morphology operations (include/edt_hip.h, "morphology"): the five symbols are exported and bound, every
refusal comes back with its code before any device work and with the outputs untouched (host stand-ins that are never
dereferenced serve as device pointers), the Python layers raise before the library is asked, and the numpy oracle
(tests/morph_oracle.py) is held against scipy's binary morphology with a ball."""
import ctypes

import numpy as np
import pytest

import morph_oracle as oracle
from synth import voronoi_labels

OK, NO_DEVICE, BAD_ARG, UNSUPPORTED = 0, -1, -2, -4
U8, U16, U32, U64, F32, F64, BOOL = range(7)
ERODE, DILATE, OPEN, CLOSE = range(4)
FARTHER, WITHIN = 0, 1
BLACK_BORDER, SQRT, MORPH_BINARY = 1, 2, 128
FILL = 0xA5
EXT = (9, 7, 5)
N = EXT[0] * EXT[1] * EXT[2]
BAD_RADII = [float("nan"), -1.0, -float("inf"), 1e200]          # NaN, negative, a square that overflows


@pytest.fixture(scope="module")
def lib():
    from edt import _lib
    return _lib.load()


def p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class Buffers:
    """valid arguments of all three calls over host arrays; the outputs hold a sentinel"""

    def __init__(self):
        self.labels = np.ones(N, dtype=np.uint32)
        self.guard = np.ones(N, dtype=np.uint32)
        self.field = np.ones(N, dtype=np.float32)
        self.out = np.full(N, FILL, dtype=np.uint32)
        self.mask = np.full(N, FILL, dtype=np.uint8)

    def untouched(self):
        return bool((self.out == FILL).all()) and bool((self.mask == FILL).all())


def select(lib, b, **kw):
    a = dict(values=b.labels, guard=None, dtype=U32, field=b.field, radius=2.0, rule=FARTHER, out=b.out, mask=b.mask, count=N)
    a.update(kw)
    return lib.edt_hip_morph_select_device(p(a["values"]), p(a["guard"]), a["dtype"], p(a["field"]), a["radius"], a["rule"],
                                           p(a["out"]), p(a["mask"]), a["count"], None)


def morphology(lib, b, **kw):
    a = dict(labels=b.labels, dtype=U32, ndim=3, ext=EXT, w=(1.0, 1.0, 1.0), op=ERODE, radius=2.0, flags=0, out=b.out)
    a.update(kw)
    out = a["out"] if isinstance(a["out"], (ctypes.c_void_p, type(None))) else p(a["out"])
    return lib.edt_hip_morphology(p(a["labels"]), a["dtype"], a["ndim"], *a["ext"], *a["w"], a["op"], a["radius"], a["flags"], out)


def test_symbols_are_exported_and_bound(lib):
    from edt import _lib
    import edt
    from edt import device
    for name in ("edt_hip_is_foreground_device", "edt_hip_morph_select_device", "edt_hip_morphology",
                 "edt_hip_morphology_workspace_bytes", "edt_hip_morphology_device"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert (_lib.MORPH_ERODE, _lib.MORPH_DILATE, _lib.MORPH_OPEN, _lib.MORPH_CLOSE) == (0, 1, 2, 3)
    assert (_lib.MORPH_FARTHER, _lib.MORPH_WITHIN, _lib.FLAG_MORPH_BINARY) == (0, 1, 128)
    for name in ("erode", "dilate", "opening", "closing"):
        assert name in edt.__all__ and callable(getattr(edt, name)) and callable(getattr(device, name))


def test_select_refusals(lib):
    b = Buffers()
    for what, kw in [("rule", dict(rule=2)), ("rule", dict(rule=-1)), ("dtype", dict(dtype=7)), ("count", dict(count=-1)),
                     ("neither out nor mask", dict(out=None, mask=None)),
                     ("null field", dict(field=None)), ("out without values", dict(values=None)),
                     ("out without values, mask given", dict(values=None, guard=b.guard)),
                     ("inf", dict(radius=float("inf")))] + [("radius", dict(radius=r)) for r in BAD_RADII]:
        assert select(lib, b, **kw) == BAD_ARG, (what, kw, lib.edt_hip_last_error())
        assert b"morph_select" in lib.edt_hip_last_error(), what
        assert b.untouched(), what
    # neither output: refused whatever else the call holds, also for an empty range
    assert select(lib, b, out=None, mask=None, count=0) == BAD_ARG
    assert select(lib, b, count=0) == OK and b.untouched()


def test_is_foreground_refusals(lib):
    b = Buffers()
    call = lambda labels, dtype, mask, count: lib.edt_hip_is_foreground_device(p(labels), dtype, p(mask), count, None)  # noqa: E731
    assert call(b.labels, 7, b.mask, N) == BAD_ARG
    assert call(b.labels, -1, b.mask, N) == BAD_ARG
    assert call(b.labels, U32, b.mask, -1) == BAD_ARG
    assert call(None, U32, b.mask, N) == BAD_ARG and b"null" in lib.edt_hip_last_error()
    assert call(b.labels, U32, None, N) == BAD_ARG
    assert call(None, U32, None, 0) == OK
    assert b.untouched()


def aligned_workspace(nbytes):
    """a host stand-in for a 256-byte aligned device workspace of nbytes (never dereferenced)"""
    raw = np.zeros(int(nbytes) + 256, dtype=np.uint8)
    return raw[(-raw.ctypes.data) % 256:][:int(nbytes)]


def morphology_device(lib, b, **kw):
    """edt_hip_morphology_device with a workspace of the size its query gives, unless ws / ws_bytes say otherwise"""
    a = dict(labels=b.labels, dtype=U32, ndim=3, ext=EXT, w=(1.0, 1.0, 1.0), op=ERODE, radius=2.0, flags=0, out=b.out)
    a.update({k: v for k, v in kw.items() if k not in ("ws", "ws_bytes")})
    need = lib.edt_hip_morphology_workspace_bytes(a["dtype"], a["ndim"], *a["ext"], a["op"], a["flags"])
    ws = kw["ws"] if "ws" in kw else aligned_workspace(max(need, 256))
    ws = ws if isinstance(ws, (ctypes.c_void_p, type(None))) else p(ws)
    out = a["out"] if isinstance(a["out"], (ctypes.c_void_p, type(None))) else p(a["out"])
    return lib.edt_hip_morphology_device(p(a["labels"]), a["dtype"], a["ndim"], *a["ext"], *a["w"], a["op"], a["radius"], a["flags"], out,
                                         ws, kw.get("ws_bytes", max(need, 256)), None)


def bad_arguments():
    bad = [("op", dict(op=4), BAD_ARG), ("op", dict(op=-1), BAD_ARG), ("dtype", dict(dtype=9), BAD_ARG),
           ("ndim", dict(ndim=4), BAD_ARG), ("unused extent", dict(ndim=2), BAD_ARG),
           ("null labels", dict(labels=None), BAD_ARG), ("null output", dict(out=None), BAD_ARG),
           ("voxel size", dict(w=(0.0, 1.0, 1.0)), BAD_ARG), ("voxel size", dict(w=(1.0, float("nan"), 1.0)), BAD_ARG)]
    for op in (ERODE, DILATE, OPEN, CLOSE):
        bad += [(f"radius, op {op}", dict(op=op, radius=r), BAD_ARG) for r in BAD_RADII]
    bad += [(f"inf, op {op}", dict(op=op, radius=float("inf")), BAD_ARG) for op in (ERODE, OPEN, CLOSE)]
    for op in (DILATE, CLOSE):
        bad += [(f"flag {f} on op {op}", dict(op=op, flags=f), UNSUPPORTED) for f in (BLACK_BORDER, MORPH_BINARY, BLACK_BORDER | MORPH_BINARY)]
    bad += [(f"flag {f} on op {op}", dict(op=op, flags=f), UNSUPPORTED) for op in (ERODE, OPEN) for f in (SQRT, 4, 64, 256, MORPH_BINARY | 16)]
    return bad


def test_morphology_refusals(lib):
    b = Buffers()
    for what, kw, code in bad_arguments():
        assert morphology(lib, b, **kw) == code, (what, kw, lib.edt_hip_last_error())
        assert b.untouched(), what
    # the op is looked at before the flags and the radius, the flags before the radius
    assert morphology(lib, b, op=7, flags=BLACK_BORDER, radius=-1.0) == BAD_ARG and b"op" in lib.edt_hip_last_error()
    assert morphology(lib, b, op=DILATE, flags=BLACK_BORDER, radius=-1.0) == UNSUPPORTED
    # an output that overlaps the labels: the same array, and a shifted view of one buffer
    big = np.ones(2 * N, dtype=np.uint32)
    for shift in (0, 1, N - 1):
        rc = morphology(lib, b, labels=big[:N], out=ctypes.c_void_p(big.ctypes.data + 4 * shift))
        assert rc == BAD_ARG and b"overlap" in lib.edt_hip_last_error(), shift
        rc = morphology(lib, b, labels=big[shift:shift + N], out=big[:N])
        assert rc == BAD_ARG and b"overlap" in lib.edt_hip_last_error(), shift
    assert bool((big == 1).all())
    # an empty volume: nothing touched, whatever the pointers
    assert morphology(lib, b, ext=(9, 0, 5), labels=None, out=None) == OK
    assert morphology(lib, b, ext=(0, 1, 1), ndim=1) == OK and b.untouched()


def test_device_entry_refuses_what_its_host_sibling_refuses(lib):
    """the same codes for the same bad arguments, before any device work (never EDT_ERR_NO_DEVICE) and with the output untouched"""
    b = Buffers()
    for what, kw, code in bad_arguments():
        assert morphology_device(lib, b, **kw) == code, (what, kw, lib.edt_hip_last_error())
        assert b.untouched(), what
    assert morphology_device(lib, b, op=7, flags=BLACK_BORDER, radius=-1.0) == BAD_ARG and b"op" in lib.edt_hip_last_error()
    assert morphology_device(lib, b, op=DILATE, flags=BLACK_BORDER, radius=-1.0) == UNSUPPORTED
    # the workspace: missing, too small, misaligned
    for op in (ERODE, DILATE, OPEN, CLOSE):
        need = lib.edt_hip_morphology_workspace_bytes(U32, 3, *EXT, op, 0)
        ws = aligned_workspace(need + 256)
        assert morphology_device(lib, b, op=op, ws=None) == BAD_ARG and b"workspace" in lib.edt_hip_last_error()
        assert morphology_device(lib, b, op=op, ws=ws, ws_bytes=need - 1) == BAD_ARG and b"workspace" in lib.edt_hip_last_error()
        assert morphology_device(lib, b, op=op, ws=ws[4:], ws_bytes=need) == BAD_ARG and b"256-byte aligned" in lib.edt_hip_last_error()
    # d_out == d_labels: refused where the last step still reads other voxels of the labels
    for op in (DILATE, CLOSE):
        assert morphology_device(lib, b, op=op, out=b.labels) == BAD_ARG and b"alias" in lib.edt_hip_last_error()
    assert bool((b.labels == 1).all()) and b.untouched()
    # an empty volume: nothing touched, whatever the pointers
    assert morphology_device(lib, b, ext=(9, 0, 5), labels=None, out=None, ws=None, ws_bytes=0) == OK
    assert morphology_device(lib, b, ext=(0, 1, 1), ndim=1) == OK and b.untouched()


def test_workspace_query(lib):
    query = lib.edt_hip_morphology_workspace_bytes
    for op in (ERODE, DILATE, OPEN, CLOSE):
        for dtype in (U8, U32, F64, BOOL):
            n = query(dtype, 3, *EXT, op, 0)
            assert n > 0 and n % 256 == 0, (op, dtype, n)
        assert query(9, 3, *EXT, op, 0) == 0 and query(U8, 4, *EXT, op, 0) == 0 and query(U8, 2, *EXT, op, 0) == 0
        assert query(U8, 3, 9, -1, 5, op, 0) == 0 and query(U8, 3, *EXT, op, SQRT) == 0
    assert query(U8, 3, *EXT, 4, 0) == 0 and query(U8, 3, *EXT, DILATE, BLACK_BORDER) == 0
    voxels = N
    # erode / opening / closing hold a field and a mask besides the transforms' scratch; dilate is expand_labels' scratch alone
    assert query(U32, 3, *EXT, DILATE, 0) == lib.edt_hip_expand_labels_workspace_bytes(U32, 3, *EXT)
    for op in (ERODE, OPEN, CLOSE):
        assert query(U32, 3, *EXT, op, 0) >= 5 * voxels + lib.edt_hip_workspace_bytes_flags(U8, 3, *EXT, 0)
    assert query(U32, 3, *EXT, ERODE, 0) >= 5 * voxels + lib.edt_hip_workspace_bytes_flags(U32, 3, *EXT, 0)


def test_without_a_device_the_host_entry_says_so(lib):
    from edt import _lib
    import edt
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present; the no-device path is exercised on the CPU runner")
    b = Buffers()
    for op, flags, radius in ((ERODE, BLACK_BORDER | MORPH_BINARY, 0.0), (DILATE, 0, float("inf")), (OPEN, 0, 2.0), (CLOSE, 0, 1.5)):
        assert morphology(lib, b, op=op, flags=flags, radius=radius) == NO_DEVICE
        assert morphology_device(lib, b, op=op, flags=flags, radius=radius) == NO_DEVICE
    # in place is not refused by the argument checks of erode and opening
    for op in (ERODE, OPEN):
        assert morphology_device(lib, b, op=op, out=b.labels) == NO_DEVICE
    assert b.untouched() and bool((b.labels == 1).all())
    with pytest.raises(_lib.EdtHipError) as e:
        edt.opening(np.ones((4, 4, 4), dtype=np.uint8), 1.0)
    assert e.value.code == _lib.ERR_NO_DEVICE


def test_python_layer_raises_before_the_library_is_asked(monkeypatch):
    import edt
    from edt import _lib

    def no_library():
        raise AssertionError("the library was asked")

    monkeypatch.setattr(_lib, "load", no_library)
    lab = np.ones((4, 5, 6), dtype=np.uint16)
    for fn in (edt.erode, edt.dilate, edt.opening, edt.closing):
        with pytest.raises(TypeError):
            fn(np.ones((2, 2, 2, 2), dtype=np.uint8))
        with pytest.raises(TypeError):
            fn(np.ones(()), 1.0)
        with pytest.raises(TypeError):
            fn(np.ones((4, 4), dtype=np.complex64))
        with pytest.raises(TypeError):
            fn(np.zeros((0, 4), dtype=np.complex64))
        for r in BAD_RADII + ([] if fn is edt.dilate else [float("inf")]):
            with pytest.raises(ValueError):
                fn(lab, r)
        with pytest.raises(ValueError):
            fn(lab, 1.0, anisotropy=(1.0, 1.0))
        with pytest.raises(ValueError):
            fn(lab, 1.0, anisotropy=(1.0, 0.0, 1.0))
        empty = np.zeros((3, 0, 2), dtype=np.int64)
        got = fn(empty, 2.0)
        assert got.shape == empty.shape and got.dtype == empty.dtype and got is not empty
    # the device module checks the radius with the same helper, before it looks at a tensor's contents
    assert edt._morph_radius(0, "erode") == 0.0 and edt._morph_radius(float("inf"), "dilate", inf_allowed=True) == float("inf")
    for r in BAD_RADII + [float("inf")]:
        with pytest.raises(ValueError):
            edt._morph_radius(r, "erode")


# ---- the oracle against scipy -------------------------------------------------------------------------------------------------
def volumes():
    """(3-D, 2-D) multi-label volumes with membranes, as the issue states them"""
    return [voronoi_labels((40, 33, 20), 10, seed, upsample=5, membrane=0.15) for seed in (1, 2)] + \
           [voronoi_labels((70, 45), 8, seed, upsample=6, membrane=0.15) for seed in (1, 2)]


@pytest.mark.parametrize("radius", [2, 3])
@pytest.mark.parametrize("black_border", [False, True])
def test_erode_and_opening_equal_the_per_label_scipy_composition(radius, black_border):
    ndimage = pytest.importorskip("scipy").ndimage
    for lab in volumes():
        ball = oracle.ball(radius, lab.ndim)
        eroded = oracle.erode(lab, radius, black_border=black_border)
        opened = oracle.opening(lab, radius, black_border=black_border)
        want_e, want_o = np.zeros_like(lab), np.zeros_like(lab)
        for l in np.unique(lab[lab != 0]):
            e = ndimage.binary_erosion(lab == l, ball, border_value=0 if black_border else 1)
            want_e[e] = l
            want_o[ndimage.binary_dilation(e, ball) & (lab == l)] = l
            # (the dilation of one label's erosion never leaves that label: the opening is anti-extensive)
            assert not (ndimage.binary_dilation(e, ball) & (lab != l)).any()
        assert np.array_equal(eroded, want_e) and np.array_equal(opened, want_o), (lab.shape, radius, black_border)
        assert 0 < np.count_nonzero(eroded) < np.count_nonzero(opened) < np.count_nonzero(lab)
        assert np.array_equal(oracle.opening(opened, radius, black_border=black_border), opened)      # idempotent
        # on the mask: scipy's binary erosion and opening
        m = (lab != 0).astype(np.uint8)
        me = ndimage.binary_erosion(m, ball, border_value=0 if black_border else 1)
        assert np.array_equal(oracle.erode(m, radius, black_border=black_border) != 0, me)
        assert np.array_equal(oracle.opening(m, radius, black_border=black_border) != 0, ndimage.binary_dilation(me, ball))
        assert np.array_equal(oracle.erode(lab, radius, black_border=black_border, binary=True), np.where(me, lab, 0))


@pytest.mark.parametrize("radius", [2, 3])
def test_closing_of_masks_equals_scipy_and_is_extensive_and_idempotent(radius):
    ndimage = pytest.importorskip("scipy").ndimage
    for m in [(voronoi_labels((40, 33, 20), 10, 1, upsample=5, membrane=0.3) != 0).astype(np.uint8),
              (voronoi_labels((70, 45), 8, 2, upsample=6, membrane=0.3) != 0).astype(np.uint8)]:
        ball = oracle.ball(radius, m.ndim)
        closed = oracle.closing(m, radius)
        want = ndimage.binary_erosion(ndimage.binary_dilation(m, ball), ball, border_value=1)
        assert np.array_equal(closed != 0, want), (m.shape, radius)
        assert closed[m != 0].all() and np.count_nonzero(closed) > np.count_nonzero(m)                # extensive
        assert np.array_equal(oracle.closing(closed, radius), closed)                                 # idempotent
        assert np.array_equal(oracle.dilate(m, radius) != 0, ndimage.binary_dilation(m, ball))
