"""CPU tier of local thickness (include/edt_hip.h, "local thickness"): the four symbols are exported and bound, every refusal comes
back with its code before any device work and with the outputs untouched (host stand-ins that are never dereferenced serve as
device pointers), the Python layers raise before the library is asked, and the numpy oracle (tests/thickness_oracle.py) is held
against scipy's binary morphology with a ball, label by label, on a volume whose openings are not nested."""
import ctypes

import numpy as np
import pytest

import morph_oracle
import thickness_oracle as oracle
from synth import voronoi_labels

OK, NO_DEVICE, BAD_ARG, UNSUPPORTED = 0, -1, -2, -4
U8, U16, U32, U64, F32, F64, BOOL = range(7)
BLACK_BORDER, SQRT, MORPH_BINARY = 1, 2, 128
FILL = 0xA5
EXT = (9, 7, 5)
N = EXT[0] * EXT[1] * EXT[2]
BAD_RADII = [float("nan"), -1.0, 0.0, -0.0, float("inf"), -float("inf"), 1e200]        # ..., a square that overflows
NESTED_RADII = [1, 1.5, 2, 2.5, 3, 4, 5, 6, 7]


@pytest.fixture(scope="module")
def lib():
    from edt import _lib
    return _lib.load()


def p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class Buffers:
    """valid arguments of both calls over host arrays; the outputs hold a sentinel"""

    def __init__(self, k=3):
        filled = lambda n, dtype: np.full(n * np.dtype(dtype).itemsize, FILL, dtype=np.uint8).view(dtype)  # noqa: E731
        self.labels = np.ones(N, dtype=np.uint32)
        self.S = np.ones(N, dtype=np.float32)
        self.B = np.ones(N, dtype=np.float32)
        self.radii = np.arange(1, k + 1, dtype=np.float64)
        self.T, self.mask, self.sizes = filled(N, np.float32), filled(N, np.uint8), filled(k, np.int64)
        self.size, self.smax, self.n_used = filled(1, np.int64), filled(1, np.uint32), filled(1, np.int64)

    def untouched(self):
        return all(bool((a.view(np.uint8) == FILL).all()) for a in (self.T, self.mask, self.sizes, self.size, self.smax, self.n_used))


def step(lib, b, **kw):
    a = dict(S=b.S, B=b.B, radius=2.0, next_radius=3.0, T=b.T, mask=b.mask, size=b.size, smax=None, count=N)
    a.update(kw)
    return lib.edt_hip_thickness_step_device(p(a["S"]), p(a["B"]), a["radius"], a["next_radius"], p(a["T"]), p(a["mask"]),
                                             p(a["size"]), p(a["smax"]), a["count"], None)


def thickness(lib, b, **kw):
    a = dict(labels=b.labels, dtype=U32, ndim=3, ext=EXT, w=(1.0, 1.0, 1.0), flags=0, radii=b.radii, n_radii=None, step=1.0,
             T=b.T, sizes=b.sizes, n_used=b.n_used)
    a.update(kw)
    n_radii = (0 if a["radii"] is None else len(a["radii"])) if a["n_radii"] is None else a["n_radii"]
    ptr = lambda v: v if isinstance(v, (ctypes.c_void_p, type(None))) else p(v)  # noqa: E731
    return lib.edt_hip_local_thickness(ptr(a["labels"]), a["dtype"], a["ndim"], *a["ext"], *a["w"], a["flags"], ptr(a["radii"]), n_radii,
                                       a["step"], ptr(a["T"]), ptr(a["sizes"]), ptr(a["n_used"]))


def aligned_workspace(nbytes):
    """a host stand-in for a 256-byte aligned device workspace of nbytes (never dereferenced)"""
    raw = np.zeros(int(nbytes) + 256, dtype=np.uint8)
    return raw[(-raw.ctypes.data) % 256:][:int(nbytes)]


def thickness_device(lib, b, **kw):
    """edt_hip_local_thickness_device with a workspace of the size its query gives, unless ws / ws_bytes say otherwise"""
    a = dict(labels=b.labels, dtype=U32, ndim=3, ext=EXT, w=(1.0, 1.0, 1.0), flags=0, radii=b.radii, n_radii=None, step=1.0,
             T=b.T, sizes=b.sizes, n_used=b.n_used)
    a.update({k: v for k, v in kw.items() if k not in ("ws", "ws_bytes")})
    n_radii = (0 if a["radii"] is None else len(a["radii"])) if a["n_radii"] is None else a["n_radii"]
    ptr = lambda v: v if isinstance(v, (ctypes.c_void_p, type(None))) else p(v)  # noqa: E731
    need = max(lib.edt_hip_local_thickness_workspace_bytes(a["dtype"], a["ndim"], *a["ext"], a["flags"]), 256)
    ws = kw["ws"] if "ws" in kw else aligned_workspace(need)
    return lib.edt_hip_local_thickness_device(ptr(a["labels"]), a["dtype"], a["ndim"], *a["ext"], *a["w"], a["flags"], ptr(a["radii"]),
                                              n_radii, a["step"], ptr(a["T"]), ptr(a["sizes"]), ptr(a["n_used"]), ptr(ws),
                                              kw.get("ws_bytes", need), None)


def test_symbols_are_exported_and_bound(lib):
    from edt import _lib
    import edt
    from edt import device
    for name in ("edt_hip_thickness_step_device", "edt_hip_local_thickness", "edt_hip_local_thickness_workspace_bytes",
                 "edt_hip_local_thickness_device"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for name in ("local_thickness", "ThicknessSizes"):
        assert name in edt.__all__ and callable(getattr(edt, name))
    assert callable(device.local_thickness)
    assert edt.ThicknessSizes._fields == ("radii", "voxels")


def test_step_refusals(lib):
    b = Buffers()
    first = dict(B=None, size=None, smax=b.smax)            # a valid step 0
    bad = [("count", dict(count=-1)), ("null S", dict(S=None)), ("null T", dict(T=None)),
           ("null S, step 0", dict(first, S=None)), ("null T, step 0", dict(first, T=None)),
           ("mask without a next radius", dict(next_radius=-1.0)), ("a next radius without a mask", dict(mask=None)),
           ("mask without a next radius, step 0", dict(first, next_radius=-2.5)),
           ("size on step 0", dict(first, size=b.size)), ("smax on a radius step", dict(smax=b.smax))]
    bad += [(f"radius {r}", dict(radius=r)) for r in BAD_RADII]
    bad += [(f"next radius {r}", dict(next_radius=r)) for r in BAD_RADII if not r < 0] + [("next radius nan, no mask", dict(next_radius=float("nan"), mask=None))]
    for what, kw in bad:
        assert step(lib, b, **kw) == BAD_ARG, (what, lib.edt_hip_last_error())
        assert b"thickness_step" in lib.edt_hip_last_error(), what
        assert b.untouched(), what
    # refused for an empty range too; a valid call over an empty range is through
    assert step(lib, b, count=0, radius=-1.0) == BAD_ARG and step(lib, b, count=0, mask=None) == BAD_ARG
    assert step(lib, b, count=0) == OK and step(lib, b, count=0, **first) == OK
    assert step(lib, b, count=0, mask=None, next_radius=-1.0, size=None) == OK
    assert step(lib, b, count=0, radius=float("nan"), **first) == OK          # (step 0 ignores the radius)
    assert b.untouched()


def r(*v):
    return np.array(v, dtype=np.float64)


def bad_arguments():
    bad = [("dtype", dict(dtype=9), BAD_ARG), ("ndim", dict(ndim=4), BAD_ARG), ("ndim", dict(ndim=0), BAD_ARG),
           ("unused extent", dict(ndim=2), BAD_ARG),
           ("null labels", dict(labels=None), BAD_ARG), ("null thickness", dict(T=None), BAD_ARG),
           ("null sizes", dict(sizes=None), BAD_ARG), ("null n_used", dict(n_used=None), BAD_ARG),
           ("null sizes, default ladder", dict(radii=None, n_radii=4, sizes=None), BAD_ARG),
           ("voxel size", dict(w=(0.0, 1.0, 1.0)), BAD_ARG), ("voxel size", dict(w=(1.0, float("nan"), 1.0)), BAD_ARG),
           ("not ascending", dict(radii=r(1, 2, 2)), BAD_ARG), ("descending", dict(radii=r(3, 2, 1)), BAD_ARG),
           ("empty list", dict(n_radii=0), BAD_ARG), ("negative length", dict(n_radii=-1), BAD_ARG),
           ("negative room", dict(radii=None, n_radii=-1), BAD_ARG)]
    bad += [(f"radius {v} first", dict(radii=r(v, 8.0, 9.0)), BAD_ARG) for v in BAD_RADII]
    bad += [(f"radius {v} last", dict(radii=r(1, 2, v)), BAD_ARG) for v in BAD_RADII]
    bad += [(f"step {v}", dict(radii=None, n_radii=3, step=v), BAD_ARG) for v in BAD_RADII]
    bad += [(f"flags {f}", dict(flags=f), UNSUPPORTED) for f in (SQRT, 4, 8, 16, 32, 64, 256, MORPH_BINARY | 16, BLACK_BORDER | SQRT)]
    return bad


def test_local_thickness_refusals(lib):
    b = Buffers()
    for what, kw, code in bad_arguments():
        assert thickness(lib, b, **kw) == code, (what, lib.edt_hip_last_error())
        assert b.untouched(), what
    # the flags are looked at before the radii
    assert thickness(lib, b, flags=SQRT, radii=r(2, 1, 0)) == UNSUPPORTED
    # buffers that overlap: thickness or sizes over the labels, sizes inside thickness
    big = np.ones(2 * N, dtype=np.uint32)
    for shift in (0, 1, N - 1):
        assert thickness(lib, b, labels=big[:N], T=ctypes.c_void_p(big.ctypes.data + 4 * shift)) == BAD_ARG
        assert b"overlap" in lib.edt_hip_last_error(), shift
        assert thickness(lib, b, labels=big[shift:shift + N], T=big[:N].view(np.float32)) == BAD_ARG
    assert thickness(lib, b, labels=big[:N], sizes=ctypes.c_void_p(big.ctypes.data + 4 * (N - 1))) == BAD_ARG
    assert thickness(lib, b, T=big[:N].view(np.float32), sizes=ctypes.c_void_p(big.ctypes.data + 8)) == BAD_ARG
    assert b"overlap" in lib.edt_hip_last_error()
    assert bool((big == 1).all()) and b.untouched()
    # an empty volume: nothing touched, whatever the pointers
    assert thickness(lib, b, ext=(9, 0, 5), labels=None, T=None, sizes=None, n_used=None) == OK
    assert thickness(lib, b, ext=(0, 1, 1), ndim=1) == OK and b.untouched()
    # ... but not whatever the radii
    assert thickness(lib, b, ext=(9, 0, 5), radii=r(2, 1, 3)) == BAD_ARG


def test_device_entry_refuses_what_its_host_sibling_refuses(lib):
    """the same codes for the same bad arguments, before any device work (never EDT_ERR_NO_DEVICE) and with the outputs untouched"""
    b = Buffers()
    for what, kw, code in bad_arguments():
        assert thickness_device(lib, b, **kw) == code, (what, lib.edt_hip_last_error())
        assert b.untouched(), what
    assert thickness_device(lib, b, flags=SQRT, radii=r(2, 1, 0)) == UNSUPPORTED
    # the workspace: missing, too small, misaligned -- for an explicit list and for the default ladder
    need = lib.edt_hip_local_thickness_workspace_bytes(U32, 3, *EXT, 0)
    ws = aligned_workspace(need + 256)
    for kw in (dict(), dict(radii=None, n_radii=3)):
        assert thickness_device(lib, b, ws=None, **kw) == BAD_ARG and b"workspace" in lib.edt_hip_last_error()
        assert thickness_device(lib, b, ws=ws, ws_bytes=need - 1, **kw) == BAD_ARG and b"workspace" in lib.edt_hip_last_error()
        assert thickness_device(lib, b, ws=ws[4:], ws_bytes=need, **kw) == BAD_ARG and b"256-byte aligned" in lib.edt_hip_last_error()
    assert b.untouched()
    # an empty volume: nothing touched, whatever the pointers -- but not whatever the radii
    assert thickness_device(lib, b, ext=(9, 0, 5), labels=None, T=None, sizes=None, n_used=None, ws=None, ws_bytes=0) == OK
    assert thickness_device(lib, b, ext=(0, 1, 1), ndim=1) == OK and b.untouched()
    assert thickness_device(lib, b, ext=(9, 0, 5), radii=r(2, 1, 3)) == BAD_ARG


def test_workspace_query(lib):
    query = lib.edt_hip_local_thickness_workspace_bytes
    for dtype in (U8, U32, F64, BOOL):
        for flags in (0, BLACK_BORDER, MORPH_BINARY, BLACK_BORDER | MORPH_BINARY):
            n = query(dtype, 3, *EXT, flags)
            assert n > 0 and n % 256 == 0, (dtype, flags, n)
            # S, B and the mask, the word of Smax, the scratch of the binary transform
            assert n >= 9 * N + 4 + lib.edt_hip_workspace_bytes_flags(U8, 3, *EXT, 0)
    assert query(U32, 3, *EXT, 0) >= 9 * N + 4 + lib.edt_hip_workspace_bytes_flags(U32, 3, *EXT, 0)
    assert query(U32, 3, *EXT, MORPH_BINARY) == query(U8, 3, *EXT, 0) == query(BOOL, 3, *EXT, 0)
    assert query(9, 3, *EXT, 0) == 0 and query(U8, 4, *EXT, 0) == 0 and query(U8, 2, *EXT, 0) == 0 and query(U8, 3, 9, -1, 5, 0) == 0
    assert query(U8, 3, *EXT, SQRT) == 0 and query(U8, 3, *EXT, 256) == 0


def test_a_valid_call_reaches_the_device_check(lib):
    """what is left of a call that passes every check above is the device: without one, EDT_ERR_NO_DEVICE and untouched outputs"""
    from edt import _lib
    import edt
    if _lib.device_count() > 0:
        return
    b = Buffers()
    assert thickness(lib, b) == NO_DEVICE
    assert thickness(lib, b, flags=BLACK_BORDER | MORPH_BINARY, radii=None, n_radii=0, sizes=None, step=0.5) == NO_DEVICE
    assert step(lib, b) == NO_DEVICE and step(lib, b, B=None, size=None, smax=b.smax) == NO_DEVICE
    assert thickness_device(lib, b) == NO_DEVICE
    assert thickness_device(lib, b, flags=BLACK_BORDER | MORPH_BINARY, radii=None, n_radii=0, sizes=None, step=0.5) == NO_DEVICE
    assert b.untouched()
    with pytest.raises(_lib.EdtHipError) as e:
        edt.local_thickness(np.ones((4, 4, 4), dtype=np.uint8), [1.0, 2.0])
    assert e.value.code == _lib.ERR_NO_DEVICE
    with pytest.raises(_lib.EdtHipError) as e:
        edt.local_thickness(np.ones((4, 4, 4), dtype=np.uint8), black_border=True, return_sizes=True)
    assert e.value.code == _lib.ERR_NO_DEVICE


def test_python_layer_raises_before_the_library_is_asked(monkeypatch):
    import edt
    from edt import _lib

    def no_library():
        raise AssertionError("the library was asked")

    monkeypatch.setattr(_lib, "load", no_library)
    lab = np.ones((4, 5, 6), dtype=np.uint16)
    with pytest.raises(TypeError):
        edt.local_thickness(np.ones((2, 2, 2, 2), dtype=np.uint8))
    with pytest.raises(TypeError):
        edt.local_thickness(np.ones(()), [1.0])
    with pytest.raises(TypeError):
        edt.local_thickness(np.ones((4, 4), dtype=np.complex64), [1.0])
    for radii in [[]] + [[v] for v in BAD_RADII] + [[1.0, v] for v in BAD_RADII] + [[1, 1], [2, 1], [1, 2, 3, 3], "abc", [None]]:
        with pytest.raises(ValueError):
            edt.local_thickness(lab, radii)
        with pytest.raises(ValueError):
            edt._thickness_radii(radii)
    with pytest.raises(ValueError):
        edt.local_thickness(lab, [1.0], anisotropy=(1.0, 1.0))
    with pytest.raises(ValueError):
        edt.local_thickness(lab, anisotropy=(1.0, 0.0, 1.0))
    got = edt._thickness_radii([1, 1.5, np.float32(2)])
    assert got.dtype == np.float64 and got.tolist() == [1.0, 1.5, 2.0] and edt._thickness_radii(3).tolist() == [3.0]
    # an empty array: an empty result, the radii given back, no voxels
    empty = np.zeros((3, 0, 2), dtype=np.int64)
    got = edt.local_thickness(empty, [1, 2])
    assert got.shape == empty.shape and got.dtype == np.float32
    got, sizes = edt.local_thickness(empty, [1, 2], return_sizes=True)
    assert got.shape == empty.shape and sizes.radii.tolist() == [1.0, 2.0] and sizes.voxels.tolist() == [0, 0]
    assert sizes.radii.dtype == np.float64 and sizes.voxels.dtype == np.int64
    got, sizes = edt.local_thickness(empty, return_sizes=True)
    assert got.shape == empty.shape and sizes.radii.size == 0 and sizes.voxels.size == 0
    # the room Python gives the default ladder covers every S a volume can hold: S <= sum (w_i (n_i + 1))^2
    step, room = edt._ladder_room((30, 20, 10), (3.0, 3.0, 40.0))
    assert step == 3.0 and room >= np.sqrt((3 * 31) ** 2 + (3 * 21) ** 2 + (40 * 11) ** 2) / 3.0
    step, room = edt._ladder_room((5,), (0.5,))
    assert step == 0.5 and room >= 6


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nested():
    """the volume on which the openings by digital balls are not nested, C-ordered, with its oracle results"""
    lab = np.ascontiguousarray(voronoi_labels((70, 33, 20), 14, seed=3, upsample=8, membrane=0.12))
    T, radii, sizes = oracle.local_thickness(lab, NESTED_RADII)
    return lab, T, radii, sizes, oracle.openings(lab, NESTED_RADII)


def test_openings_are_not_nested_and_sizes_not_monotone(nested):
    lab, T, radii, sizes, O = nested
    assert sizes.tolist()[:4] == [41530, 42628, 39395, 41471]
    assert (np.diff(sizes) > 0).any() and (np.diff(sizes) < 0).any()
    skipped = sum(int(np.count_nonzero(O[j + 1] & ~O[j])) for j in range(len(O) - 1))
    assert skipped == 3390
    # the rule that stops at a voxel's first miss gives another answer, and a smaller one
    wrong = oracle.local_thickness(lab, NESTED_RADII, first_miss=True)[0]
    assert (wrong <= T).all() and np.count_nonzero(wrong != T) > 1000
    for j, r in enumerate(radii):
        assert np.count_nonzero(O[j]) == sizes[j] and not O[j][lab == 0].any()
    assert set(np.unique(T).tolist()) <= {0.0} | {float(np.float32(r)) for r in radii}
    assert not T[lab == 0].any() and np.count_nonzero(T[lab != 0] == 0) > 0            # thinner than the smallest ball


def test_oracle_equals_the_per_label_scipy_composition(nested):
    ndimage = pytest.importorskip("scipy").ndimage
    lab, T, radii, sizes, _ = nested
    want = np.zeros(lab.shape, dtype=np.float32)
    counts = np.zeros(len(radii), dtype=np.int64)
    for j, r in enumerate(radii):
        ball = morph_oracle.ball(r, lab.ndim)
        for l in np.unique(lab[lab != 0]):
            opened = ndimage.binary_dilation(ndimage.binary_erosion(lab == l, ball, border_value=1), ball) & (lab == l)
            want[opened] = np.float32(r)
            counts[j] += np.count_nonzero(opened)
    assert np.array_equal(T, want) and np.array_equal(sizes, counts)


def test_a_voxel_that_survives_an_erosion_is_at_least_that_thick(nested):
    lab, T, radii, _, _ = nested
    for bb, binary in ((False, False), (True, False), (False, True)):
        S = oracle.measured_field(lab, None, bb, binary).astype(np.float64)
        Tb = T if (bb, binary) == (False, False) else oracle.local_thickness(lab, NESTED_RADII, black_border=bb, binary=binary)[0]
        for r in radii:
            assert (Tb[S > r * r] >= np.float32(r)).all(), (bb, binary, r)
        assert not Tb[S == 0].any()


def test_default_ladder_ends_at_the_largest_finite_distance():
    lab = voronoi_labels((40, 33, 20), 10, seed=2, upsample=5, membrane=0.15)
    for an, bb, binary in ((None, False, False), ((1.0, 1.0, 2.0), True, False), ((0.5, 0.75, 0.5), False, True), ((3.58, 3.58, 40.0), True, True)):
        S = oracle.measured_field(lab, an, bb, binary).astype(np.float64)
        smax = S[np.isfinite(S)].max()
        radii = oracle.default_radii(lab, an, bb, binary)
        step = min(an) if an else 1.0
        assert radii.size >= 1 and np.array_equal(radii, np.arange(1, radii.size + 1) * np.float64(np.float32(step)))
        assert radii[-1] ** 2 < smax <= ((radii.size + 1) * np.float64(np.float32(step))) ** 2
        T, used, sizes = oracle.local_thickness(lab, None, an, bb, binary)
        assert np.array_equal(used, radii) and sizes[0] > 0
        # one more rung changes nothing: its ball fits nowhere
        more = np.append(radii, radii[-1] + np.float32(step))
        T2, _, sizes2 = oracle.local_thickness(lab, more, an, bb, binary)
        assert np.array_equal(T2, T) and sizes2[-1] == 0 and np.array_equal(sizes2[:-1], sizes)
    # one label, no border: no finite distance, an empty ladder, zero thickness; explicit radii: the last one everywhere
    one = np.full((12, 9, 5), 7, dtype=np.uint8)
    assert oracle.default_radii(one).size == 0 and not oracle.local_thickness(one)[0].any()
    T, _, sizes = oracle.local_thickness(one, [1.0, 2.5])
    assert (T == np.float32(2.5)).all() and sizes.tolist() == [one.size, one.size]
    assert oracle.default_radii(one, black_border=True).tolist() == [1.0, 2.0]            # S peaks at 3^2 in the middle
