"""CPU tier of the medial axis (include/edt_hip.h, "medial axis"): the numpy oracle (tests/medial_oracle.py) states the definition
twice -- the header's gather form and the paper's scatter loop -- and the two are held against each other and against the
pictures and properties the definition promises; the four symbols are exported and bound, every refusal comes back with its code
before any device work and with the outputs untouched (host stand-ins that are never dereferenced serve as device pointers), and
the Python layers raise before the library is asked."""
import ctypes
import math

import numpy as np
import pytest

import ft_oracle
import medial_oracle as oracle

OK, NO_DEVICE, BAD_ARG, UNSUPPORTED = 0, -1, -2, -4
U8, U16, U32, U64, F32, F64, BOOL = range(7)
BLACK_BORDER, SQRT, MORPH_BINARY = 1, 2, 128
FILL = 0xA5
EXT = (9, 7, 5)
N = EXT[0] * EXT[1] * EXT[2]
BAD_GAMMAS = [float("nan"), -1.0, float("inf"), -float("inf"), 1e200]        # ..., a square that overflows
BAD_RATIOS = [float("nan"), -1.0, float("inf"), -float("inf")]

# the 20 x 9 rectangle in a 24 x 11 frame (x along the line): the four diagonal branches into the corners and the central
# segment -- and the central segment alone once the features have to subtend 120 degrees
RECTANGLE = """
........................
..#..................#..
...#................#...
....#..............#....
.....#............#.....
......############......
.....#............#.....
....#..............#....
...#................#...
..#..................#..
........................
"""
RECTANGLE_120 = """
........................
........................
........................
........................
........................
......############......
........................
........................
........................
........................
........................
"""


def picture(text):
    return np.array([[c == "#" for c in line] for line in text.split()], dtype=bool)


def random_labels(rng, shape, nlabels, dtype=np.uint8):
    """a few blobs of 2-3 labels on background: coarse random blocks, so that objects are several voxels thick"""
    coarse = rng.integers(0, nlabels + 1, size=tuple((s + 2) // 3 for s in shape))
    lab = coarse
    for axis, s in enumerate(shape):
        lab = np.repeat(lab, 3, axis=axis).take(np.arange(s), axis=axis)
    return lab.astype(dtype)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------

def test_gather_equals_scatter_on_random_volumes():
    rng = np.random.default_rng(11)
    cases = 0
    for w, a in (((1.0, 1.0, 1.0), (1, 1, 1)), ((1.0, 1.0, 5.0), (1, 1, 25)), ((2.0, 1.0, 3.0), (4, 1, 9))):
        for bb in (False, True):
            for k in range(6):
                shape = tuple(int(v) for v in rng.integers(1, 13 if k else 17, size=3))
                lab = random_labels(rng, shape, 2 + k % 2)
                binary = k % 3 == 2
                of = (lab != 0).astype(np.uint8) if binary else lab
                feat, _ = ft_oracle.feature_transform(of, a, bb)
                for gamma, ratio in ((max(w), 0.0), (0.0, 0.0), (1.5 * max(w), oracle.ratio_of(60)), (min(w), oracle.ratio_of(120))):
                    g = oracle.gather(lab, feat, w, gamma, ratio, bb, binary)
                    s = oracle.scatter(lab, feat, w, gamma, ratio, bb, binary)
                    assert np.array_equal(g, s), (w, bb, shape, gamma, ratio)
                    with np.errstate(invalid="ignore"):
                        assert not g[lab == 0].any()
                cases += 1
    assert cases == 36


def test_gather_equals_scatter_in_fewer_dimensions():
    rng = np.random.default_rng(12)
    for nd, shape in ((1, (15, 1, 1)), (2, (12, 9, 1)), (2, (1, 7, 1))):
        for bb in (False, True):
            lab = random_labels(rng, shape, 3)
            feat, _ = ft_oracle.feature_transform(lab, (1, 4, 1), bb, ndim=nd)
            g = oracle.gather(lab, feat, (1.0, 2.0, 1.0), 1.0, 0.0, bb, False, nd)
            assert np.array_equal(g, oracle.scatter(lab, feat, (1.0, 2.0, 1.0), 1.0, 0.0, bb, False, nd))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 9, 10])
def test_runs_between_background_give_their_centre(n):
    """an odd run gives its centre voxel, an even run its two centre voxels; a single voxel has no neighbour of its label"""
    line = np.zeros(n + 5, dtype=np.uint16)
    line[2:2 + n] = 7
    want = np.zeros_like(line)
    if n >= 2:
        want[2 + (n - 1) // 2: 2 + n // 2 + 1] = 7
    assert np.array_equal(oracle.medial_axis(line), want)
    # the same run as a column of a 2-D array and along z of a 3-D one, between background; as wide as the array it is
    # a slab without an axis across x unless the border is black
    assert np.array_equal(oracle.medial_axis(line[:, None]), want[:, None])
    assert np.array_equal(oracle.medial_axis(line[:, None, None]), want[:, None, None])
    # gamma = 0 keeps every pair of different features: nothing changes for a run, whose centre is the only place where the
    # two features differ
    assert np.array_equal(oracle.medial_axis(line, gamma=0.0), want)


def test_one_label_everywhere():
    """without a border a label that fills the array has no feature and no axis; with the border it is the object in a frame
    of background (the feature transform's black_border) and has the axis of that object"""
    for shape in ((9,), (6, 7), (4, 5, 6)):
        full = np.full(shape, 3, dtype=np.uint32)
        assert not oracle.medial_axis(full).any()
        assert not oracle.medial_axis(full, binary=True).any()
        framed = np.pad(full, 1)
        inner = tuple(slice(1, -1) for _ in shape)
        assert np.array_equal(oracle.medial_axis(full, black_border=True), oracle.medial_axis(framed)[inner])
        assert oracle.medial_axis(full, black_border=True).any()


def test_rectangle_pictures():
    frame = np.zeros((11, 24), dtype=np.uint8)
    frame[1:10, 2:22] = 1
    plain, pruned = picture(RECTANGLE), picture(RECTANGLE_120)
    assert plain.sum() == 28 and pruned.sum() == 12
    for form in (oracle.gather, oracle.scatter):
        assert np.array_equal(oracle.on_axis(frame, form=form), plain)
        assert np.array_equal(oracle.on_axis(frame, min_angle=120, form=form), pruned)
    assert np.array_equal(oracle.on_axis(frame.astype(bool)), plain)
    assert np.array_equal(oracle.on_axis(frame * 9, binary=True), plain)


def test_axis_is_a_subset_of_the_foreground_and_keeps_the_labels():
    rng = np.random.default_rng(13)
    lab = random_labels(rng, (14, 12, 10), 3, np.int16) * np.int16(-5)
    for kw in (dict(), dict(black_border=True), dict(binary=True), dict(anisotropy=(1.0, 1.0, 2.0))):
        out = oracle.medial_axis(lab, **kw)
        assert out.dtype == lab.dtype and np.array_equal(out[out != 0], lab[out != 0]) and (out != 0).any()
        assert not (out != 0)[lab == 0].any()


def test_axis_shrinks_as_gamma_and_min_angle_grow():
    rng = np.random.default_rng(14)
    lab = random_labels(rng, (16, 15, 9), 2)
    for bb in (False, True):
        prev = None
        for gamma in (0.0, 1.0, 1.5, 2.0, 3.0, 5.0, 40.0):
            on = oracle.on_axis(lab, gamma=gamma, black_border=bb)
            assert prev is None or not (on & ~prev).any()
            prev = on
        assert not prev.any()
        prev = None
        for angle in (0, 30, 60, 90, 120, 150, 179):
            on = oracle.on_axis(lab, min_angle=angle, black_border=bb)
            assert prev is None or not (on & ~prev).any()
            prev = on


def test_ratio_helper_is_shared():
    import edt
    for a in (0, 1e-3, 30, 60, 90, 120, 179.5):
        assert edt._medial_ratio(a) == math.tan(math.radians(a) / 2.0) ** 2 == oracle.ratio_of(a)
    assert edt._medial_ratio(0) == 0.0 and abs(edt._medial_ratio(90) - 1.0) < 1e-15
    assert edt._medial_gamma(None, (6.0, -30.0, 6.0)) == 30.0 and edt._medial_gamma(2, (1.0,)) == 2.0


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from edt import _lib
    return _lib.load()


def p(a):
    return a if isinstance(a, (ctypes.c_void_p, type(None))) else ctypes.c_void_p(a.ctypes.data)


class Buffers:
    """valid arguments of both calls over host arrays; the outputs hold a sentinel"""

    def __init__(self):
        filled = lambda n, dtype: np.full(n * np.dtype(dtype).itemsize, FILL, dtype=np.uint8).view(dtype)  # noqa: E731
        self.labels = np.ones(N, dtype=np.uint32)
        self.features = np.zeros(3 * N, dtype=np.int32)
        self.field = np.ones(N, dtype=np.float32)
        self.out, self.radius = filled(N, np.uint32), filled(N, np.float32)

    def untouched(self):
        return all(bool((a.view(np.uint8) == FILL).all()) for a in (self.out, self.radius))


def step(lib, b, **kw):
    a = dict(labels=b.labels, dtype=U32, ndim=3, ext=EXT, w=(1.0, 1.0, 1.0), features=b.features, flags=0, gamma=1.0, ratio=0.0,
             out=b.out, field=b.field, radius=b.radius)
    a.update(kw)
    return lib.edt_hip_medial_axis_step_device(p(a["labels"]), a["dtype"], a["ndim"], *a["ext"], *a["w"], p(a["features"]), a["flags"],
                                               a["gamma"], a["ratio"], p(a["out"]), p(a["field"]), p(a["radius"]), None)


def host(lib, b, **kw):
    a = dict(labels=b.labels, dtype=U32, ndim=3, ext=EXT, w=(1.0, 1.0, 1.0), flags=0, gamma=1.0, ratio=0.0, out=b.out, radius=b.radius)
    a.update(kw)
    return lib.edt_hip_medial_axis(p(a["labels"]), a["dtype"], a["ndim"], *a["ext"], *a["w"], a["flags"], a["gamma"], a["ratio"],
                                   p(a["out"]), p(a["radius"]))


def aligned_workspace(nbytes):
    """a host stand-in for a 256-byte aligned device workspace of nbytes (never dereferenced)"""
    raw = np.zeros(int(nbytes) + 256, dtype=np.uint8)
    return raw[(-raw.ctypes.data) % 256:][:int(nbytes)]


def on_device(lib, b, **kw):
    """edt_hip_medial_axis_device with a workspace of the size its query gives, unless ws / ws_bytes say otherwise"""
    a = dict(labels=b.labels, dtype=U32, ndim=3, ext=EXT, w=(1.0, 1.0, 1.0), flags=0, gamma=1.0, ratio=0.0, out=b.out, radius=b.radius)
    a.update({k: v for k, v in kw.items() if k not in ("ws", "ws_bytes")})
    need = max(lib.edt_hip_medial_axis_workspace_bytes(a["dtype"], a["ndim"], *a["ext"], a["flags"], 0 if a["radius"] is None else 1), 256)
    ws = kw["ws"] if "ws" in kw else aligned_workspace(need)
    return lib.edt_hip_medial_axis_device(p(a["labels"]), a["dtype"], a["ndim"], *a["ext"], *a["w"], a["flags"], a["gamma"], a["ratio"],
                                          p(a["out"]), p(a["radius"]), p(ws), kw.get("ws_bytes", need), None)


def test_symbols_are_exported_and_bound(lib):
    from edt import _lib
    import edt
    from edt import device
    for name in ("edt_hip_medial_axis_step_device", "edt_hip_medial_axis", "edt_hip_medial_axis_workspace_bytes",
                 "edt_hip_medial_axis_device"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "medial_axis" in edt.__all__ and callable(edt.medial_axis) and callable(device.medial_axis)
    assert "d_workspace" not in " ".join(str(t) for t in _lib.SIGNATURES["edt_hip_medial_axis_step_device"][1])
    assert len(_lib.SIGNATURES["edt_hip_medial_axis_step_device"][1]) == 17 and len(_lib.SIGNATURES["edt_hip_medial_axis"][1]) == 14


COMMON_REFUSALS = ([("dtype", dict(dtype=9), BAD_ARG), ("dtype", dict(dtype=-1), BAD_ARG), ("ndim", dict(ndim=4), BAD_ARG),
                    ("ndim", dict(ndim=0), BAD_ARG), ("unused extent", dict(ndim=2), BAD_ARG), ("extent", dict(ext=(9, -1, 5)), BAD_ARG),
                    ("voxel size", dict(w=(0.0, 1.0, 1.0)), BAD_ARG), ("voxel size", dict(w=(1.0, float("nan"), 1.0)), BAD_ARG),
                    ("voxel size", dict(w=(-1.0, 1.0, 1.0)), BAD_ARG), ("voxel size", dict(w=(1.0, 1.0, float("inf"))), BAD_ARG),
                    ("null labels", dict(labels=None), BAD_ARG), ("null out", dict(out=None), BAD_ARG)]
                   + [(f"gamma {v}", dict(gamma=v), BAD_ARG) for v in BAD_GAMMAS]
                   + [(f"ratio {v}", dict(ratio=v), BAD_ARG) for v in BAD_RATIOS]
                   + [(f"flags {f}", dict(flags=f), UNSUPPORTED) for f in (SQRT, 4, 8, 16, 32, 64, 256, MORPH_BINARY | 16, BLACK_BORDER | SQRT)])


def test_step_refusals(lib):
    b = Buffers()
    bad = COMMON_REFUSALS + [("null features", dict(features=None), BAD_ARG), ("field without radius", dict(radius=None), BAD_ARG),
                             ("radius without field", dict(field=None), BAD_ARG), ("out is the labels", dict(out=b.labels), BAD_ARG)]
    for what, kw, code in bad:
        assert step(lib, b, **kw) == code, (what, lib.edt_hip_last_error())
        assert b.untouched() and bool((b.labels == 1).all()), what
    # refused for an empty volume too; a valid call over an empty volume is through, whatever the pointers
    assert step(lib, b, ext=(9, 0, 5), gamma=-1.0) == BAD_ARG and step(lib, b, ext=(9, 0, 5), radius=None) == BAD_ARG
    assert step(lib, b, ext=(9, 0, 5), flags=SQRT) == UNSUPPORTED
    assert step(lib, b, ext=(9, 0, 5), labels=None, features=None, out=None, field=None, radius=None) == OK
    assert step(lib, b, ext=(0, 1, 1), ndim=1) == OK and b.untouched()


def test_host_refusals(lib):
    b = Buffers()
    for what, kw, code in COMMON_REFUSALS:
        assert host(lib, b, **kw) == code, (what, lib.edt_hip_last_error())
        assert b.untouched(), what
    # buffers that overlap: out or radius over the labels, radius inside out
    big = np.ones(2 * N, dtype=np.uint32)
    for shift in (0, 1, N - 1):
        at = ctypes.c_void_p(big.ctypes.data + 4 * shift)
        assert host(lib, b, labels=big[:N], out=at) == BAD_ARG and b"overlap" in lib.edt_hip_last_error(), shift
        assert host(lib, b, labels=big[:N], radius=at) == BAD_ARG and b"overlap" in lib.edt_hip_last_error(), shift
        assert host(lib, b, labels=big[shift:shift + N], out=big[:N]) == BAD_ARG
        assert host(lib, b, out=big[:N], radius=at) == BAD_ARG and b"overlap" in lib.edt_hip_last_error(), shift
    assert bool((big == 1).all()) and b.untouched()
    # an empty volume: nothing touched, whatever the pointers -- but not whatever the pruning
    assert host(lib, b, ext=(9, 0, 5), labels=None, out=None, radius=None) == OK
    assert host(lib, b, ext=(0, 1, 1), ndim=1) == OK and b.untouched()
    assert host(lib, b, ext=(9, 0, 5), ratio=float("nan")) == BAD_ARG


def test_device_entry_refuses_what_its_host_sibling_refuses(lib):
    """the same codes for the same bad arguments, before any device work (never EDT_ERR_NO_DEVICE) and with the outputs untouched"""
    b = Buffers()
    for what, kw, code in COMMON_REFUSALS:
        assert on_device(lib, b, **kw) == code, (what, lib.edt_hip_last_error())
        assert b.untouched(), what
    # the workspace: missing, too small, misaligned
    for radius in (b.radius, None):
        need = lib.edt_hip_medial_axis_workspace_bytes(U32, 3, *EXT, 0, 0 if radius is None else 1)
        ws = aligned_workspace(need + 256)
        assert on_device(lib, b, radius=radius, ws=None) == BAD_ARG and b"workspace" in lib.edt_hip_last_error()
        assert on_device(lib, b, radius=radius, ws=ws, ws_bytes=need - 1) == BAD_ARG and b"workspace" in lib.edt_hip_last_error()
        assert on_device(lib, b, radius=radius, ws=ws[4:], ws_bytes=need) == BAD_ARG and b"256-byte aligned" in lib.edt_hip_last_error()
    # a workspace sized without the radius does not serve a call with it
    assert on_device(lib, b, ws=ws, ws_bytes=need) == BAD_ARG and b"workspace" in lib.edt_hip_last_error()
    # d_out == d_labels: the neighbours are still being read
    assert on_device(lib, b, out=b.labels) == BAD_ARG and b"alias" in lib.edt_hip_last_error()
    assert b.untouched() and bool((b.labels == 1).all())
    # an empty volume: nothing touched, whatever the pointers -- but not whatever the pruning
    assert on_device(lib, b, ext=(9, 0, 5), labels=None, out=None, radius=None, ws=None, ws_bytes=0) == OK
    assert on_device(lib, b, ext=(0, 1, 1), ndim=1) == OK and b.untouched()
    assert on_device(lib, b, ext=(9, 0, 5), ratio=float("nan")) == BAD_ARG


def test_workspace_query(lib):
    query = lib.edt_hip_medial_axis_workspace_bytes
    for dtype in (U8, U32, F64, BOOL):
        for flags in (0, BLACK_BORDER, MORPH_BINARY, BLACK_BORDER | MORPH_BINARY):
            binary = bool(flags & MORPH_BINARY) or dtype == BOOL
            of = U8 if binary else dtype
            for with_radius in (0, 1):
                n = query(dtype, 3, *EXT, flags, with_radius)
                assert n > 0 and n % 256 == 0, (dtype, flags, with_radius, n)
                # the planes, the mask under binary, the field with the radius, the scratch of the feature transform
                parts = 12 * N + N * binary + 4 * N * with_radius
                assert n >= parts + lib.edt_hip_feature_workspace_bytes(of, 3, *EXT, flags & BLACK_BORDER), (dtype, flags, with_radius)
            assert query(dtype, 3, *EXT, flags, 1) > query(dtype, 3, *EXT, flags, 0)
    assert query(U32, 3, *EXT, MORPH_BINARY, 1) == query(U8, 3, *EXT, MORPH_BINARY, 1) != query(U32, 3, *EXT, 0, 1)
    assert query(9, 3, *EXT, 0, 0) == 0 and query(U8, 4, *EXT, 0, 0) == 0 and query(U8, 2, *EXT, 0, 1) == 0
    assert query(U8, 3, 9, -1, 5, 0, 0) == 0 and query(U8, 3, *EXT, SQRT, 0) == 0 and query(U8, 3, *EXT, 256, 1) == 0


def test_a_valid_call_reaches_the_device_check(lib):
    """what is left of a call that passes every check above is the device: without one, EDT_ERR_NO_DEVICE and untouched outputs"""
    from edt import _lib
    import edt
    if _lib.device_count() > 0:
        return
    b = Buffers()
    assert step(lib, b) == NO_DEVICE and step(lib, b, field=None, radius=None, flags=BLACK_BORDER | MORPH_BINARY) == NO_DEVICE
    assert step(lib, b, gamma=0.0, ratio=3.0, w=(1.0, -2.0, -0.5)) == NO_DEVICE
    assert host(lib, b) == NO_DEVICE and host(lib, b, radius=None, flags=BLACK_BORDER | MORPH_BINARY, dtype=BOOL, labels=b.labels.view(np.uint8)) == NO_DEVICE
    assert on_device(lib, b) == NO_DEVICE and on_device(lib, b, radius=None, flags=BLACK_BORDER | MORPH_BINARY) == NO_DEVICE
    assert b.untouched()
    with pytest.raises(_lib.EdtHipError) as e:
        edt.medial_axis(np.ones((4, 4, 4), dtype=np.uint8), return_distance=True)
    assert e.value.code == _lib.ERR_NO_DEVICE


def test_python_layer_raises_before_the_library_is_asked(monkeypatch):
    import edt
    from edt import _lib

    def no_library():
        raise AssertionError("the library was asked")

    monkeypatch.setattr(_lib, "load", no_library)
    lab = np.ones((4, 5, 6), dtype=np.uint16)
    with pytest.raises(TypeError):
        edt.medial_axis(np.ones((2, 2, 2, 2), dtype=np.uint8))
    with pytest.raises(TypeError):
        edt.medial_axis(np.ones(()))
    with pytest.raises(TypeError):
        edt.medial_axis(np.ones((4, 4), dtype=np.complex64))
    for gamma in BAD_GAMMAS + ["abc", [None]]:
        with pytest.raises(ValueError):
            edt.medial_axis(lab, gamma=gamma)
        with pytest.raises(ValueError):
            edt.medial_axis(lab[:0], gamma=gamma)
    for angle in (float("nan"), -1.0, -1e-9, 180.0, 181, float("inf"), "abc", None):
        with pytest.raises(ValueError):
            edt.medial_axis(lab, min_angle=angle)
        with pytest.raises(ValueError):
            edt._medial_ratio(angle)
    with pytest.raises(ValueError):
        edt.medial_axis(lab, anisotropy=(1.0, 1.0))
    with pytest.raises(ValueError):
        edt.medial_axis(lab, anisotropy=(1.0, 0.0, 1.0))
    # an empty array: an empty result of the same dtype, and an empty float32 distance
    empty = np.zeros((3, 0, 2), dtype=np.int64)
    got = edt.medial_axis(empty, gamma=2.0, min_angle=30)
    assert got.shape == empty.shape and got.dtype == empty.dtype
    got, dist = edt.medial_axis(empty, return_distance=True, binary=True, black_border=True)
    assert got.shape == empty.shape and got.dtype == empty.dtype and dist.shape == empty.shape and dist.dtype == np.float32
