"""GPU tier of the morphology operations (csrc/edt_morph.hip, edt_hip_morphology, edt.device): every comparison is exact
equality of the whole array, byte for byte, against the numpy restatement of the contract (tests/morph_oracle.py), through
edt.<op> on host arrays AND through edt.device.<op> on device tensors.  Shapes are the smallest at which the named thing can go
wrong: the streaming kernels take four voxels per thread where every pointer has the alignment of four of its elements (16 bytes
at the most) and one voxel otherwise (counts around a 16-byte piece of every type, around a wave and around a workgroup; every
element offset of every pointer within 16 bytes), the transforms are the
library's own and are covered by their tiers.  dilate and closing are compared where the voxel sizes share a quantum (the
feature-transform oracle is integer) on tiny volumes: that oracle is pure Python."""
import ctypes
import itertools

import numpy as np
import pytest

import morph_oracle as oracle
from synth import (bits_of, blocky_labels, offset_out, offset_view, outside_intact, palette, palette_labels, voronoi_labels)

pytestmark = pytest.mark.gpu

U8, U16, U32, U64, F32, F64, BOOL = range(7)
FARTHER, WITHIN = 0, 1
CODE = {"uint8": U8, "int8": U8, "uint16": U16, "int16": U16, "uint32": U32, "int32": U32, "uint64": U64, "int64": U64,
        "float32": F32, "float64": F64, "bool": BOOL}
MARK = {1: 0xA5, 2: 0xA5A5, 4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}
NAN = 0x7FC0BEEF
_SIGNED_VIEW = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
CARRIERS = [np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64, np.bool_]      # one dtype per ABI code
ALL_DTYPES = CARRIERS + [np.int8, np.int16, np.int32, np.int64]
COUNTS = [1, 15, 16, 17, 63, 64, 65, 255, 257, 4097]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    from edt import _lib
    _lib.load()
    if not torch.cuda.is_available() or _lib.device_count() == 0:
        pytest.fail("the GPU tier needs a HIP device")
    torch.cuda.set_device(0)


def lib():
    from edt import _lib
    return _lib.load()


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc):
    from edt import _lib
    _lib.check(rc)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes(order="A") == b.tobytes(order="A")


def ubits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}")


# ---- the two kernels, called directly -------------------------------------------------------------------------------------
def palette_line(dtype, n, rng):
    """n labels drawn from 0 and the dtype's palette (NaNs with payloads, -0.0, denormals, full-width integers)"""
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return rng.random(n) < 0.6
    pal = np.concatenate([np.zeros(1, dtype=dt), palette(dt)])
    return pal[rng.integers(0, len(pal), size=n)]


def select_want(values, guard, field, r2, rule):
    passes = field.astype(np.float64) > r2 if rule == FARTHER else field.astype(np.float64) <= r2
    if guard is not None:
        passes = passes | (guard != 0)
    out = np.zeros_like(values)
    out[passes] = values[passes]
    return out, (~passes).astype(np.uint8)


# (guard, out, mask, in place)
MODES = [(False, True, False, False), (False, False, True, False), (False, True, True, False), (True, True, False, False),
         (True, True, True, False), (False, True, False, True), (True, True, True, True), (True, False, True, False)]


def select_call(values, guard, field, r2, rule, mode, ks, what):
    """one edt_hip_morph_select_device call on offset views, checked against the oracle and for stores outside the views"""
    import torch
    with_guard, with_out, with_mask, in_place = mode
    k_val, k_field, k_out, k_mask = ks
    n, dt = values.size, values.dtype
    want_out, want_mask = select_want(values, guard if with_guard else None, field, r2, rule)
    vbuf, vview = offset_view(values, k_out if in_place else k_val)
    _, gview = offset_view(guard, k_val) if with_guard else (None, None)
    _, fview = offset_view(field, k_field, NAN)
    before = vbuf.clone()
    obuf = oview = mbuf = mview = None
    if with_out:
        obuf, oview = (vbuf, vview) if in_place else offset_out((n,), dt, k_out, MARK[dt.itemsize])
    if with_mask:
        mbuf, mview = offset_out((n,), np.uint8, k_mask, MARK[1])
    ok(lib().edt_hip_morph_select_device(vp(vview if with_out else None), vp(gview), CODE[dt.name], vp(fview), float(np.sqrt(r2)), rule,
                                         vp(oview), vp(mview), n, stream()))
    torch.cuda.synchronize()
    if with_out:
        assert np.array_equal(bits_of(oview), ubits(want_out)), (what, "out")
        if in_place:
            lo, hi = 16 + k_out, 16 + k_out + n
            assert torch.equal(vbuf[:lo], before[:lo]) and torch.equal(vbuf[hi:], before[hi:]), (what, "a store outside the view")
        else:
            assert outside_intact(obuf, k_out, n, MARK[dt.itemsize]), (what, "a store outside the output")
            assert torch.equal(vbuf, before), (what, "the values were written")
    if with_mask:
        assert np.array_equal(bits_of(mview), want_mask), (what, "mask")
        assert outside_intact(mbuf, k_mask, n, MARK[1]), (what, "a store outside the mask")


@pytest.mark.parametrize("dtype", CARRIERS)
def test_select_kernel_forms(dtype):
    """every count around the vector width, a wave and a workgroup; every element offset 0 .. 16 / itemsize - 1 of the values (and
    guard), the field, the output and the mask, each on its own with the others aligned, and all of them odd together; with and
    without guard, out only, mask only, both, and out == values.  The field ties with R2 on many voxels."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(dt.itemsize + (dt.kind == "f"))
    per16 = 16 // dt.itemsize
    offsets = [(0, 0, 0, 0)] + [(k, 0, 0, 0) for k in range(1, per16)] + [(0, k, 0, 0) for k in range(1, 4)] + \
              [(0, 0, k, 0) for k in range(1, per16)] + [(0, 0, 0, k) for k in range(1, 16)] + [(per16 - 1, 3, 1, 7), (1, 1, 1, 1)]
    r2 = np.float64(4.0)
    levels = np.array([0.0, 1.0, 2.0, 4.0, 4.0, np.nextafter(np.float32(4), np.float32(5)), 5.0, 9.0, np.inf], dtype=np.float32)
    turn = itertools.count()
    for n in COUNTS:
        values, guard = palette_line(dt, n, rng), palette_line(dt, n, rng)
        field = levels[rng.integers(0, len(levels), size=n)]
        if n > 64:
            assert (field == 4.0).any() and (field > 4.0).any() and (field < 4.0).any()
        for ks in offsets:
            t = next(turn)
            select_call(values, guard, field, r2, (FARTHER, WITHIN)[t % 2], MODES[t % len(MODES)], ks, (dt.name, n, ks))
        for mode, rule in itertools.product(MODES, (FARTHER, WITHIN)):       # every mode and rule, aligned and all-odd
            select_call(values, guard, field, r2, rule, mode, (0, 0, 0, 0), (dt.name, n, "aligned", mode, rule))
            select_call(values, guard, field, r2, rule, mode, (1, 1, 1, 1), (dt.name, n, "odd", mode, rule))


@pytest.mark.parametrize("dtype", CARRIERS)
def test_is_foreground_kernel_forms(dtype):
    import torch
    dt = np.dtype(dtype)
    rng = np.random.default_rng(100 + dt.itemsize)
    per16 = 16 // dt.itemsize
    for n in COUNTS:
        labels = palette_line(dt, n, rng)
        want = (labels != 0).astype(np.uint8)
        if n > 64 and dt.kind == "f":
            assert np.isnan(labels).any() and (ubits(labels) == 1 << (8 * dt.itemsize - 1)).any()        # NaN: 1; -0.0: 0
        for k_lab, k_mask in [(0, 0)] + [(k, 0) for k in range(1, per16)] + [(0, k) for k in range(1, 16)] + [(per16 - 1, 5)]:
            lbuf, lview = offset_view(labels, k_lab)
            before = lbuf.clone()
            mbuf, mview = offset_out((n,), np.uint8, k_mask, MARK[1])
            ok(lib().edt_hip_is_foreground_device(vp(lview), CODE[dt.name], vp(mview), n, stream()))
            torch.cuda.synchronize()
            assert np.array_equal(bits_of(mview), want), (dt.name, n, k_lab, k_mask)
            assert outside_intact(mbuf, k_mask, n, MARK[1]) and torch.equal(lbuf, before), (dt.name, n, k_lab, k_mask)


# ---- the operations: host arrays and device tensors against the oracle ------------------------------------------------------
def on_device(name, data, radius, anisotropy=None, **kw):
    """edt.device.<name> of the same memory (the C-ordered view of it; unsigned types wider than a byte as their signed views),
    returned as a numpy array laid out like ``data``"""
    import torch
    from edt import device
    fortran = data.flags.f_contiguous and not data.flags.c_contiguous
    a = data.T if fortran else data
    v = a.view(_SIGNED_VIEW[a.dtype]) if a.dtype in _SIGNED_VIEW else a
    t = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    an = anisotropy
    if an is not None and np.ndim(an) > 0 and fortran:
        an = tuple(an)[::-1]
    out = getattr(device, name)(t, radius, anisotropy=an, **kw)
    assert out.dtype == t.dtype and out.shape == t.shape and out.is_contiguous()
    assert (out is t) == bool(kw.get("in_place", False))
    got = out.cpu().numpy().view(a.dtype)
    return got.T if fortran else got


def check(name, data, radius, anisotropy=None, **kw):
    """host and device results equal the oracle's bytes; returns the oracle's array"""
    import edt
    want = getattr(oracle, name)(data, radius, anisotropy, **kw)
    got = getattr(edt, name)(data, radius, anisotropy=anisotropy, **kw)
    assert got.flags.f_contiguous == data.flags.f_contiguous and got.flags.c_contiguous == data.flags.c_contiguous
    assert same_bytes(got, want), (name, data.dtype, data.shape, radius, anisotropy, kw, int((ubits(got) != ubits(want)).sum()))
    dev = on_device(name, data, radius, anisotropy, **kw)
    assert same_bytes(np.asarray(dev, order="A"), want), (name, "device", data.dtype, data.shape, radius, anisotropy, kw)
    return want


def test_ties_decide_between_greater_and_greater_or_equal(oracle_port):
    lab = voronoi_labels((70, 33, 20), 14, seed=3, upsample=8, membrane=0.12)
    S = oracle_port.edtsq(lab, (1.0, 1.0, 1.0), False)
    ties = int((S == 4.0).sum())
    assert ties > 1000, ties
    fg = np.count_nonzero(lab)
    eroded = check("erode", lab, 2.0)
    opened = check("opening", lab, 2.0)
    assert np.count_nonzero(eroded) == int((S > 4.0).sum())                         # ">" : a tie is removed
    assert 0.05 * fg <= fg - np.count_nonzero(eroded) <= 0.95 * fg
    assert np.count_nonzero(eroded) < np.count_nonzero(opened) < fg
    assert not (opened[eroded != 0] != lab[eroded != 0]).any() and not (opened[opened != 0] != lab[opened != 0]).any()
    for bb, binary in ((True, False), (False, True), (True, True)):
        check("erode", lab, 2.0, black_border=bb, binary=binary)
        check("opening", lab, 2.0, black_border=bb, binary=binary)


def volume(shape, dtype, order, seed, block=6):
    lab = palette_labels(shape, dtype, rng=np.random.default_rng(seed), block=block, zero_frac=0.2, order=order)
    return lab


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_erode_and_opening_matrix(dtype):
    """every dtype with full-width palettes (NaN and -0.0 among them), 1-D / 2-D / 3-D, C and F order, both border modes, binary
    on and off, at unit and at anisotropic voxel sizes"""
    dt = np.dtype(dtype)
    changed = kept = 0
    for nd, order in itertools.product((1, 2, 3), "CF"):
        shape = ((150,), (41, 30), (29, 22, 14))[nd - 1]
        lab = volume(shape, dt, order, nd + (order == "F"))
        for an, r in ((None, 2.0), ((1.0, 1.0, 2.0)[-nd:], 2.0)):
            for bb, binary in itertools.product((False, True), (False, True)):
                e = check("erode", lab, r, an, black_border=bb, binary=binary)
                o = check("opening", lab, r, an, black_border=bb, binary=binary)
                changed += int(np.count_nonzero(ubits(o) != ubits(lab)))
                kept += int(np.count_nonzero(ubits(e)))
    assert changed > 0 and kept > 0
    # anisotropic sizes with and without a quantum: larger blocks, so that something is farther than r from every other label
    for nd, order in ((3, "F"), (3, "C"), (2, "F"), (2, "C")):
        shape = ((64, 50), (50, 42, 9))[nd - 2]
        lab = volume(shape, dt, order, 10 + nd, block=14)
        for an, r in (((6.0, 6.0, 30.0), 30.0), ((3.58, 3.58, 40.0), 8.0)):
            a = an[:nd] if order == "F" else an[:nd][::-1]
            for bb, binary in ((False, False), (True, True), (True, False)):
                e = check("erode", lab, r, a, black_border=bb, binary=binary)
                check("opening", lab, r, a, black_border=bb, binary=binary)
                if nd == 2:
                    assert np.count_nonzero(ubits(e)) > 0


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_dilate_and_closing_matrix(dtype):
    """byte-exact where the voxel sizes share a quantum; tiny volumes: the feature-transform oracle is pure Python"""
    dt = np.dtype(dtype)
    grown = closed_more = 0
    for nd, order in itertools.product((1, 2, 3), "CF"):
        shape = ((60,), (19, 14), (13, 11, 8))[nd - 1]
        lab = palette_labels(shape, dt, rng=np.random.default_rng(20 + nd), block=2, zero_frac=0.55, order=order)
        cases = ([(None, 1.5), (None, 2.0), ((1.0, 1.0, 2.0)[-nd:], 2.0), ((6.0, 6.0, 30.0)[:nd], 13.0)] if order == "F" else
                 [(None, 2.0), ((30.0, 6.0, 6.0)[-nd:], 13.0)])
        for an, r in cases:
            d = check("dilate", lab, r, an)
            c = check("closing", lab, r, an)
            grown += int(np.count_nonzero(d != 0) - np.count_nonzero(lab != 0))
            closed_more += int(np.count_nonzero(ubits(c) != ubits(d)))
    assert grown > 0 and closed_more > 0


def test_closing_without_a_quantum_keeps_the_input_and_stays_inside_the_dilation():
    import edt
    lab = np.asfortranarray(blocky_labels((40, 37, 9), nlabels=6, zero_frac=0.5, block=4, rng=np.random.default_rng(8)).astype(np.uint32))
    an, r = (3.58, 3.58, 40.0), 8.0
    closed = edt.closing(lab, r, anisotropy=an)
    dilated = edt.dilate(lab, r, anisotropy=an)
    assert same_bytes(dilated, edt.expand_labels(lab, r, anisotropy=an))
    assert np.array_equal(closed[lab != 0], lab[lab != 0])                          # extensive
    assert np.array_equal(closed[closed != 0], dilated[closed != 0])                # a subset of the dilation, under its labels
    assert np.count_nonzero(lab) < np.count_nonzero(closed) < np.count_nonzero(dilated)
    assert same_bytes(on_device("closing", lab, r, an), closed) and same_bytes(on_device("dilate", lab, r, an), dilated)


def test_degenerate_cases():
    import edt
    rng = np.random.default_rng(4)
    lab = np.asfortranarray(blocky_labels((33, 20, 9), nlabels=5, zero_frac=0.3, block=5, rng=rng).astype(np.uint16))
    flt = palette_labels((20, 9, 7), np.float32, rng=rng, block=3, order="F")
    for name in ("erode", "opening", "dilate", "closing"):                           # r = 0: the labels, -0.0 aside
        assert same_bytes(check(name, lab, 0.0), lab), name
        got = check(name, flt, 0.0)
        want = flt.copy(order="K")
        if name != "dilate":                                                         # (expand_labels copies the background as it is)
            want[flt == 0] = 0.0
        assert same_bytes(got, want), name
        zeros = np.zeros((17, 5, 3), dtype=np.int32, order="F")                      # all background
        assert same_bytes(check(name, zeros, 2.0), zeros), name
    assert (ubits(flt)[flt == 0] != 0).any()                                         # (there was a -0.0 to lose its sign)
    one = np.full((40, 9, 5), 7, dtype=np.uint8, order="F")                          # one label, no border: the field is +inf
    for name in ("erode", "opening", "closing", "dilate"):
        assert same_bytes(check(name, one, 3.0), one), name
    assert np.count_nonzero(check("erode", one, 1.0, black_border=True)) == 38 * 7 * 3
    assert 38 * 7 * 3 < np.count_nonzero(check("opening", one, 1.0, black_border=True)) < one.size     # (the box loses its corners)
    for bb in (False, True):                                                         # a radius that erodes everything
        assert not check("erode", lab, 40.0, black_border=bb).any()
        assert not check("opening", lab, 40.0, black_border=bb).any()
    assert not check("opening", one, 20.0, black_border=True).any()
    for shape in ((1,), (1, 1), (1, 1, 1), (30, 1), (1, 30), (1, 17, 1), (9, 1, 6), (1, 1, 25)):     # axis lengths 1
        thin = np.asfortranarray(blocky_labels(shape, nlabels=3, zero_frac=0.3, block=4, rng=rng).astype(np.uint32))
        thin.flat[0] = 2
        for name in ("erode", "opening", "dilate", "closing"):
            check(name, thin, 1.0)
            check(name, np.ascontiguousarray(thin), 2.0)
    rows = np.asfortranarray(blocky_labels((1025, 6, 3), nlabels=4, zero_frac=0.25, block=7, rng=rng).astype(np.uint8))   # x-rows of 1025
    for name in ("erode", "opening"):
        check(name, rows, 2.0)
        check(name, rows, 3.0, black_border=True, binary=True)
    line = blocky_labels((1025,), nlabels=3, zero_frac=0.4, block=3, rng=rng).astype(np.uint16)
    for name in ("erode", "opening", "dilate", "closing"):
        check(name, line, 2.0)
    empty = np.zeros((4, 0, 3), dtype=np.float64)
    for name in ("erode", "opening", "dilate", "closing"):
        assert getattr(edt, name)(empty, 1.0).shape == empty.shape and on_device(name, empty, 1.0).shape == empty.shape


def test_in_place_returns_the_same_tensor_with_the_same_result():
    import torch
    from edt import device
    lab = np.ascontiguousarray(voronoi_labels((48, 33, 20), 12, seed=5, upsample=6, membrane=0.1).T)
    for name, kw in (("erode", {}), ("opening", {}), ("erode", dict(black_border=True, binary=True)), ("opening", dict(binary=True))):
        want = getattr(oracle, name)(lab, 2.0, None, **kw)
        assert 0 < np.count_nonzero(want) < np.count_nonzero(lab)
        assert same_bytes(on_device(name, lab, 2.0, **kw), want)
        assert same_bytes(on_device(name, lab, 2.0, in_place=True, **kw), want)
    t = torch.from_numpy(lab.view(np.int32)).cuda()
    with pytest.raises(ValueError):
        device.opening(t.transpose(0, 2), 2.0, in_place=True)
    for r in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            device.erode(t, r)
    with pytest.raises(TypeError):
        device.closing(t.reshape(1, *t.shape), 1.0)
    assert np.array_equal(t.cpu().numpy(), lab.view(np.int32))


def test_opening_is_captured_on_a_side_stream_and_replays_on_changed_input():
    """one device.opening after a warm-up call on the same stream (plans and intermediates are cached per stream), captured
    into a graph; the replay reads whatever the input tensor holds by then"""
    import torch
    from edt import device
    labs = [np.ascontiguousarray(voronoi_labels((64, 40, 24), 10, seed=s, upsample=8, membrane=0.1).T) for s in (6, 7)]
    wants = [oracle.opening(lab, 2.0, (1.0, 1.0, 2.0), black_border=True) for lab in labs]
    assert not same_bytes(wants[0], wants[1])
    t = torch.from_numpy(labs[0].view(np.int32)).cuda()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        warm = device.opening(t, 2.0, anisotropy=(1.0, 1.0, 2.0), black_border=True)
        side.synchronize()
        assert same_bytes(warm.cpu().numpy().view(np.uint32), wants[0])
        with torch.cuda.graph(graph, stream=side):
            out = device.opening(t, 2.0, anisotropy=(1.0, 1.0, 2.0), black_border=True)
    for which in (1, 0, 1):
        t.copy_(torch.from_numpy(labs[which].view(np.int32)))
        out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bytes(out.cpu().numpy().view(np.uint32), wants[which]), which


def test_host_entry_runs_on_the_first_listed_device():
    import edt
    lab = voronoi_labels((40, 33, 20), 10, seed=2, upsample=5, membrane=0.15)
    want = oracle.erode(lab, 2.0, black_border=True)
    edt.set_devices([0, 0])
    try:
        assert same_bytes(edt.erode(lab, 2.0, black_border=True), want)
        assert same_bytes(edt.opening(lab, 2.0), oracle.opening(lab, 2.0))
    finally:
        edt.set_devices(None)
    assert same_bytes(edt.erode(lab, 2.0, black_border=True), want)
