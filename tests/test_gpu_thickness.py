"""GPU tier of local thickness (k_thickness_step in csrc/edt_morph.hip, edt_hip_local_thickness, edt.device.local_thickness): every
comparison is exact equality of the whole array, byte for byte, against the numpy restatement of the contract
(tests/thickness_oracle.py), through edt.local_thickness on host arrays AND through edt.device.local_thickness on device tensors.
Shapes are the smallest at which the named thing can go wrong: the step kernel takes four voxels per thread where S, B and T are
16-byte and the mask 4-byte aligned and one voxel otherwise (counts around four voxels, a wave, a workgroup, and one past a
single trip of the fixed grid in each form; every offset 0..3 of every pointer); the transforms are the library's own and are
covered by their tiers."""
import ctypes
import itertools

import numpy as np
import pytest

import thickness_oracle as oracle
from synth import (bits_of, blocky_labels, offset_out, offset_view, outside_intact, palette_labels, voronoi_labels)

pytestmark = pytest.mark.gpu

MARK = {1: 0xA5, 4: 0xA5A5A5A5}
_SIGNED_VIEW = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
ALL_DTYPES = [np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64, np.bool_, np.int8, np.int16, np.int32, np.int64]
COUNTS = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097]
GRID_THREADS = 2048 * 256                  # the fixed grid of the streaming kernels (csrc/edt_morph.hip)
NESTED_RADII = [1, 1.5, 2, 2.5, 3, 4, 5, 6, 7]
RADII = [1, 1.5, 2, 3]


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


# ---- the step kernel, called directly -------------------------------------------------------------------------------------
def levels(r, rn):
    """field values that tie with r^2 and with r'^2 -- equal, and one step of the format on either side --, 0, a positive
    denormal, values between and beyond, +inf"""
    f32 = np.float32
    out = [0.0, 1e-45, 0.25]
    for v in (f32(r * r), f32(rn * rn)):
        out += [np.nextafter(v, f32(0)), v, np.nextafter(v, f32(np.inf))]
    return np.array(out + [f32(rn * rn) * 3, np.inf], dtype=np.float32)


# (B, mask, size counter, max counter): a radius step takes the size counter, step 0 the max counter
MODES = [(True, True, True, False), (True, False, True, False), (True, True, False, False), (True, False, False, False),
         (False, True, False, True), (False, False, False, True), (False, True, False, False), (False, False, False, False)]


def step_call(S, B, prev, r, rn, mode, ks, what):
    """one edt_hip_thickness_step_device call on offset views, checked against numpy and for stores outside the views"""
    import torch
    with_B, with_mask, with_size, with_smax = mode
    k_S, k_B, k_T, k_mask = ks
    n = S.size
    r2, rn2 = np.float64(r) * np.float64(r), np.float64(rn) * np.float64(rn)
    Sbuf, Sview = offset_view(S, k_S, 0x7F000000)                     # (2^127 around the field: a read outside would raise the max)
    Bbuf, Bview = offset_view(B, k_B, 0) if with_B else (None, None)  # (0 around B: a read outside would count)
    Tbuf, Tview = offset_view(prev, k_T, MARK[4])
    Mbuf, Mview = offset_out((n,), np.uint8, k_mask, MARK[1]) if with_mask else (None, None)
    Sbefore, Bbefore = Sbuf.clone(), (Bbuf.clone() if with_B else None)
    size0, smax0 = 5, (0 if n % 2 else int(np.float32(0.3).view(np.uint32)))
    size = torch.full((1,), size0, dtype=torch.int64, device="cuda") if with_size else None
    smax = torch.full((1,), smax0, dtype=torch.int32, device="cuda") if with_smax else None
    ok(lib().edt_hip_thickness_step_device(vp(Sview), vp(Bview), float(r), float(rn) if with_mask else -1.0, vp(Tview), vp(Mview), vp(size),
                                           vp(smax), n, stream()))
    torch.cuda.synchronize()
    if with_B:
        inside = (S.astype(np.float64) > 0) & (B.astype(np.float64) <= r2)
        want = np.where(inside, np.float32(r).view(np.uint32), prev.view(np.uint32))
    else:
        want = np.zeros(n, dtype=np.uint32)
    assert np.array_equal(bits_of(Tview), want), (what, "T")
    assert outside_intact(Tbuf, k_T, n, MARK[4]), (what, "a store outside T")
    assert torch.equal(Sbuf, Sbefore) and (not with_B or torch.equal(Bbuf, Bbefore)), (what, "an input was written")
    if with_mask:
        assert np.array_equal(bits_of(Mview), (~(S.astype(np.float64) > rn2)).astype(np.uint8)), (what, "mask")
        assert outside_intact(Mbuf, k_mask, n, MARK[1]), (what, "a store outside the mask")
    if with_size:
        assert int(size.item()) == size0 + int(np.count_nonzero(inside)), (what, "size")
    if with_smax:
        finite = S[np.isfinite(S)]
        top = int(finite.max().view(np.uint32)) if finite.size else 0
        assert int(smax.item()) == max(smax0, top), (what, "max")


def fields(n, r, rn, rng):
    lv = levels(r, rn)
    S, B = lv[rng.integers(0, len(lv), size=n)], lv[rng.integers(0, len(lv), size=n)]
    prev = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)      # any bits, NaNs among them
    return S, B, prev


OFFSETS = [(0, 0, 0, 0)] + [tuple(k if j == which else 0 for j in range(4)) for which in range(4) for k in (1, 2, 3)] + \
          [(1, 1, 1, 1), (3, 1, 3, 1)]


@pytest.mark.parametrize("radii", [(2.0, 3.0), (1.5, 2.5)])
def test_step_kernel_forms(radii):
    """every count around the vector width, a wave and a workgroup; every offset 0..3 of S, B, T (floats) and the mask (bytes), each
    on its own with the others aligned, and all odd together; with and without B, the mask and the counters.  The fields tie with
    r^2 and r'^2 on many voxels and hold 0, a denormal and +inf; T keeps what it held where the voxel is not in."""
    r, rn = radii
    rng = np.random.default_rng(int(r * 10))
    turn = itertools.count()
    for n in COUNTS:
        S, B, prev = fields(n, r, rn, rng)
        if n > 64:
            for v in (np.float32(r * r), np.float32(rn * rn)):
                for f in (S, B):
                    assert (f == v).any() and (f == np.nextafter(v, np.float32(0))).any() and (f == np.nextafter(v, np.float32(np.inf))).any()
            assert (S == 0).any() and (S == np.float32(1e-45)).any() and np.isinf(S).any() and np.isinf(B).any()
        for ks in OFFSETS:
            step_call(S, B, prev, r, rn, MODES[next(turn) % len(MODES)], ks, (n, ks))
        for mode in MODES:                                                # every mode, aligned and all odd
            step_call(S, B, prev, r, rn, mode, (0, 0, 0, 0), (n, "aligned", mode))
            step_call(S, B, prev, r, rn, mode, (1, 3, 1, 3), (n, "odd", mode))


def test_step_kernel_past_one_trip_of_the_grid():
    """one count past a single trip of the fixed grid in each form: the stride loop's second trip and the tail behind the chunks"""
    rng = np.random.default_rng(7)
    r, rn = 2.0, 3.0
    for n, ks in ((GRID_THREADS * 4 + 5, (0, 0, 0, 0)), (GRID_THREADS + 3, (1, 0, 0, 0)), (GRID_THREADS + 3, (0, 0, 0, 2))):
        S, B, prev = fields(n, r, rn, rng)
        S[-1], S[-2] = np.float32(1e6), np.inf                            # the largest finite value sits in the tail
        step_call(S, B, prev, r, rn, MODES[0], ks, (n, ks, "radius step"))
        step_call(S, B, prev, r, rn, MODES[4], ks, (n, ks, "step 0"))


def test_step_with_no_finite_value_leaves_the_max_alone():
    S = np.full(300, np.inf, dtype=np.float32)
    B, prev = np.zeros(300, dtype=np.float32), np.ones(300, dtype=np.float32)
    step_call(S, B, prev, 2.0, 3.0, MODES[4], (0, 0, 0, 0), "all +inf")
    step_call(S, B, prev, 2.0, 3.0, MODES[0], (0, 0, 0, 0), "all +inf, all in")
    step_call(np.zeros(301, dtype=np.float32), B[:1].repeat(301), prev[:1].repeat(301), 2.0, 3.0, MODES[0], (0, 0, 0, 0), "all background")


# ---- the operation: host arrays and device tensors against the oracle ---------------------------------------------------------
def on_device(data, radii, anisotropy=None, **kw):
    """edt.device.local_thickness of the same memory (the C-ordered view of it; unsigned types wider than a byte as their signed
    views): ``(T laid out like data, radii, sizes)`` as numpy arrays"""
    import torch
    from edt import device
    fortran = data.flags.f_contiguous and not data.flags.c_contiguous
    a = data.T if fortran else data
    v = a.view(_SIGNED_VIEW[a.dtype]) if a.dtype in _SIGNED_VIEW else a
    t = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    an = anisotropy
    if an is not None and np.ndim(an) > 0 and fortran:
        an = tuple(an)[::-1]
    T, sizes = device.local_thickness(t, radii, anisotropy=an, return_sizes=True, **kw)
    assert T.dtype == torch.float32 and T.shape == t.shape and T.is_contiguous() and T.is_cuda
    assert sizes.voxels.is_cuda and sizes.voxels.dtype == torch.int64 and sizes.radii.dtype == np.float64
    got = T.cpu().numpy()
    return (got.T if fortran else got), sizes.radii, sizes.voxels.cpu().numpy()


def check(data, radii=None, anisotropy=None, **kw):
    """host and device results equal the oracle's bytes, radii and sizes; returns the oracle's (T, radii, sizes)"""
    import edt
    want, used, sizes = oracle.local_thickness(data, radii, anisotropy, **kw)
    what = (data.dtype, data.shape, "F" if data.flags.f_contiguous else "C", radii, anisotropy, kw)
    got, gs = edt.local_thickness(data, radii, anisotropy=anisotropy, return_sizes=True, **kw)
    assert got.flags.f_contiguous == data.flags.f_contiguous and got.flags.c_contiguous == data.flags.c_contiguous
    assert same_bytes(got, want), (what, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert gs.radii.dtype == np.float64 and gs.voxels.dtype == np.int64
    assert np.array_equal(gs.radii, used) and np.array_equal(gs.voxels, sizes), (what, gs, used, sizes)
    dev, dr, ds = on_device(data, radii, anisotropy, **kw)
    assert same_bytes(np.asarray(dev, order="A"), want), (what, "device")
    assert np.array_equal(dr, used) and np.array_equal(ds, sizes), (what, "device", dr, ds, used, sizes)
    return want, used, sizes


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_matrix(dtype):
    """every dtype with full-width palettes (NaN payloads and -0.0 among them), 1-D / 2-D / 3-D, C and F order, both border modes,
    binary on and off, explicit radii and the default ladder"""
    dt = np.dtype(dtype)
    thick = rungs = 0
    for nd, order in itertools.product((1, 2, 3), "CF"):
        shape = ((150,), (41, 30), (29, 22, 14))[nd - 1]
        lab = palette_labels(shape, dt, rng=np.random.default_rng(nd + (order == "F")), block=6, zero_frac=0.2, order=order)
        for bb, binary in itertools.product((False, True), (False, True)):
            T, _, sizes = check(lab, RADII, black_border=bb, binary=binary)
            assert not T[lab == 0].any() and sizes[0] <= np.count_nonzero(T) <= np.count_nonzero(lab != 0)
            thick += int(np.count_nonzero(T >= 2))
            rungs += check(lab, None, black_border=bb, binary=binary)[1].size
    assert thick > 0 and rungs > 0


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_anisotropic_volumes(dtype):
    """voxel sizes with a quantum (6, 6, 30) and without (3.58, 3.58, 40), larger blocks so that something is farther than r
    from every other label; the default ladder steps by the smallest voxel size"""
    dt = np.dtype(dtype)
    for nd, order in ((3, "F"), (3, "C"), (2, "F"), (2, "C")):
        shape = ((64, 50), (50, 42, 9))[nd - 2]
        lab = palette_labels(shape, dt, rng=np.random.default_rng(10 + nd), block=14, zero_frac=0.2, order=order)
        for an, radii in (((6.0, 6.0, 30.0), (6, 12, 18, 30)), ((3.58, 3.58, 40.0), (4, 8, 12))):
            a = an[:nd] if order == "F" else an[:nd][::-1]
            for bb, binary in ((False, False), (True, True), (True, False)):
                T, _, sizes = check(lab, radii, a, black_border=bb, binary=binary)
                if nd == 2:
                    assert (T >= radii[1]).any() and sizes[1] > 0
            used = check(lab, None, a, black_border=True)[1]
            assert used.size >= 1 and used[0] == np.float64(np.float32(min(a)))


@pytest.fixture(scope="module")
def nested():
    lab = voronoi_labels((70, 33, 20), 14, seed=3, upsample=8, membrane=0.12)
    return lab, oracle.local_thickness(lab, NESTED_RADII), oracle.local_thickness(lab, NESTED_RADII, first_miss=True)[0]


def test_openings_that_are_not_nested_take_the_largest_radius(nested):
    """the volume that tells "the largest j" from "stop at the first miss": thousands of voxels lie in a larger opening and not in the
    next smaller one, and the sizes go up and down"""
    import edt
    lab, (want, radii, sizes), first_miss = nested
    assert np.count_nonzero(first_miss != want) > 1000 and (np.diff(sizes) > 0).any() and (np.diff(sizes) < 0).any()
    got, gs = edt.local_thickness(lab, NESTED_RADII, return_sizes=True)
    assert same_bytes(got, want) and not same_bytes(got, first_miss)
    assert np.array_equal(gs.voxels, sizes) and np.array_equal(gs.radii, radii)
    dev, _, ds = on_device(lab, NESTED_RADII)
    assert same_bytes(np.asarray(dev, order="A"), want) and not same_bytes(np.asarray(dev, order="A"), first_miss) and np.array_equal(ds, sizes)
    for bb, binary in ((True, False), (False, True)):
        check(lab, [1, 2, 2.5, 4], black_border=bb, binary=binary)
    check(np.ascontiguousarray(lab), None)
    assert np.array_equal(edt.local_thickness(lab, NESTED_RADII), want)                # (without return_sizes: the array alone)


def test_degenerate_cases():
    import edt
    rng = np.random.default_rng(4)
    zeros = np.zeros((17, 5, 3), dtype=np.int32, order="F")                            # all background
    T, _, sizes = check(zeros, RADII)
    assert not T.any() and not sizes.any() and check(zeros, None)[1].size == 0
    one = np.full((40, 9, 5), 7, dtype=np.uint8, order="F")                            # one label, no border: S is +inf
    T, _, sizes = check(one, RADII)
    assert (T == np.float32(3)).all() and sizes.tolist() == [one.size] * 4
    T, used, sizes = check(one, None)
    assert not T.any() and used.size == 0 and sizes.size == 0
    T, used, sizes = check(one, None, black_border=True)                               # ... with a border: a box
    assert used.tolist() == [1.0, 2.0] and T.max() == 2 and 0 < sizes[1] < sizes[0] < one.size
    check(one, [1, 2, 3, 7], black_border=True)
    lab = np.asfortranarray(blocky_labels((33, 20, 9), nlabels=5, zero_frac=0.3, block=5, rng=rng).astype(np.uint16))
    S = oracle.measured_field(lab)
    smax = float(S[np.isfinite(S)].max())
    at = float(np.sqrt(smax))
    at = at if at * at >= smax else float(np.nextafter(at, np.inf))                    # the first radius whose square reaches Smax
    beyond = [1.0, 2.0, at, at + 1, 40.0]                                              # radii at and beyond sqrt(Smax): empty openings
    T, _, sizes = check(lab, beyond)
    assert sizes[2:].tolist() == [0, 0, 0] and sizes[1] > 0 and same_bytes(T, check(lab, beyond[:2])[0])
    for r in (1.0, 2.5, 40.0):                                                         # a single radius
        T, _, sizes = check(lab, [r], black_border=True)
        assert set(np.unique(T).tolist()) <= {0.0, r} and sizes[0] == np.count_nonzero(T)
    for shape in ((1,), (1, 1), (1, 1, 1), (30, 1), (1, 30), (1, 17, 1), (9, 1, 6), (1, 1, 25)):     # axis lengths 1
        thin = np.asfortranarray(blocky_labels(shape, nlabels=3, zero_frac=0.3, block=4, rng=rng).astype(np.uint32))
        thin.flat[0] = 2
        check(thin, [1, 2])
        check(np.ascontiguousarray(thin), None, black_border=True)
    rows = np.asfortranarray(blocky_labels((1025, 6, 3), nlabels=4, zero_frac=0.25, block=7, rng=rng).astype(np.uint8))   # x-rows of 1025
    check(rows, [1, 2, 3])
    check(rows, None, black_border=True, binary=True)
    line = blocky_labels((1025,), nlabels=3, zero_frac=0.4, block=9, rng=rng).astype(np.uint16)
    check(line, [1, 2, 4])
    check(line, None)
    empty = np.zeros((4, 0, 3), dtype=np.float64)
    for radii in (None, [1.0, 2.0]):
        got, gs = edt.local_thickness(empty, radii, return_sizes=True)
        dev, dr, ds = on_device(empty, radii)
        assert got.shape == dev.shape == empty.shape and got.dtype == np.float32
        assert gs.radii.tolist() == dr.tolist() == (radii or []) and gs.voxels.tolist() == ds.tolist() == [0] * len(radii or [])
    assert edt.local_thickness(empty).shape == empty.shape


def test_refusals_reach_python_as_errors():
    import torch
    import edt
    from edt import device
    lab = np.ones((6, 5, 4), dtype=np.int32)
    t = torch.from_numpy(lab).cuda()
    for radii in ([], [0.0], [2, 1], [1, 1], [float("nan")], [1, float("inf")], [1e200]):
        with pytest.raises(ValueError):
            device.local_thickness(t, radii)
        with pytest.raises(ValueError):
            edt.local_thickness(lab, radii)
    with pytest.raises(TypeError):
        device.local_thickness(t.reshape(1, *t.shape), [1.0])
    with pytest.raises(ValueError):
        device.local_thickness(t, [1.0], anisotropy=(1.0, 1.0))
    got = device.local_thickness(t, [1.0, 2.0])                                        # (without return_sizes: the tensor alone)
    assert isinstance(got, torch.Tensor) and bool((got == 2).all())


# ---- scratch and streams ------------------------------------------------------------------------------------------------------
def device_labels(lab):
    import torch
    return torch.from_numpy(np.ascontiguousarray(lab).view(np.int32)).cuda()


def test_two_calls_of_one_shape_share_the_scratch_and_nothing_else():
    """the cached S / B / mask hold the first call's data when the second begins; its result does not depend on them"""
    import torch
    from edt import device
    labs = [np.ascontiguousarray(voronoi_labels((48, 33, 20), 12, seed=s, upsample=6, membrane=0.1).T) for s in (5, 6)]
    calls = [(labs[0], [1, 2, 3], dict(black_border=True)), (labs[1], [1.5, 2.5], dict()), (labs[0], None, dict(binary=True)),
             (labs[1], [2.0], dict(black_border=True, binary=True))]
    wants = [oracle.local_thickness(lab, radii, None, **kw) for lab, radii, kw in calls]
    outs = [device.local_thickness(device_labels(lab), radii, return_sizes=True, **kw) for lab, radii, kw in calls]     # back to back
    torch.cuda.synchronize()
    for (T, sizes), (want, used, voxels) in zip(outs, wants):
        assert same_bytes(T.cpu().numpy(), want) and np.array_equal(sizes.radii, used) and np.array_equal(sizes.voxels.cpu().numpy(), voxels)
    assert len(device._workspaces["edt_hip_local_thickness_workspace_bytes"]) <= 9


def test_explicit_radii_are_captured_on_a_side_stream_and_replay_on_changed_input():
    """one call with explicit radii after a warm-up call on the same stream (plans and scratch are cached per stream), captured
    into a graph; every replay reads whatever the input tensor holds by then and counts from zero again"""
    import torch
    from edt import device
    labs = [np.ascontiguousarray(voronoi_labels((64, 40, 24), 10, seed=s, upsample=8, membrane=0.1).T) for s in (6, 7)]
    radii, an = [1, 2, 3.5], (1.0, 1.0, 2.0)
    wants = [oracle.local_thickness(lab, radii, an, black_border=True) for lab in labs]
    assert not same_bytes(wants[0][0], wants[1][0]) and not np.array_equal(wants[0][2], wants[1][2])
    t = device_labels(labs[0])
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        warm, ws = device.local_thickness(t, radii, anisotropy=an, black_border=True, return_sizes=True)
        side.synchronize()
        assert same_bytes(warm.cpu().numpy(), wants[0][0]) and np.array_equal(ws.voxels.cpu().numpy(), wants[0][2])
        with torch.cuda.graph(graph, stream=side):
            out, sizes = device.local_thickness(t, radii, anisotropy=an, black_border=True, return_sizes=True)
    for which in (1, 0, 1):
        t.copy_(device_labels(labs[which]))
        out.fill_(-1.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bytes(out.cpu().numpy(), wants[which][0]), which
        assert np.array_equal(sizes.voxels.cpu().numpy(), wants[which][2]), which


def test_the_default_ladder_is_refused_on_a_capturing_stream_and_the_capture_goes_on():
    """radii=None reads Smax back: on a stream that is being captured the library refuses before any device work (EdtHipError,
    not a failed synchronisation inside the capture), and the capture is still good for the explicit call that follows"""
    import torch
    from edt import _lib, device
    lab = np.ascontiguousarray(voronoi_labels((64, 40, 24), 10, seed=6, upsample=8, membrane=0.1).T)
    radii = [1, 2, 3.5]
    want = oracle.local_thickness(lab, radii, None, black_border=True)
    t = device_labels(lab)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        device.local_thickness(t, radii, black_border=True)                 # warm-up: scratch and code objects of this stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.EdtHipError, match="captured"):
                device.local_thickness(t, None, black_border=True)
            out, sizes = device.local_thickness(t, radii, black_border=True, return_sizes=True)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bytes(out.cpu().numpy(), want[0]) and np.array_equal(sizes.voxels.cpu().numpy(), want[2])


def test_host_entry_runs_on_the_first_listed_device():
    import edt
    lab = voronoi_labels((40, 33, 20), 10, seed=2, upsample=5, membrane=0.15)
    want, used, sizes = oracle.local_thickness(lab, None, None, black_border=True)
    edt.set_devices([0, 0])
    try:
        got, gs = edt.local_thickness(lab, black_border=True, return_sizes=True)
        assert same_bytes(got, want) and np.array_equal(gs.radii, used) and np.array_equal(gs.voxels, sizes)
        assert same_bytes(edt.local_thickness(lab, RADII), oracle.local_thickness(lab, RADII)[0])
    finally:
        edt.set_devices(None)
    got, gs = edt.local_thickness(lab, black_border=True, return_sizes=True)
    assert same_bytes(got, want) and np.array_equal(gs.voxels, sizes)
