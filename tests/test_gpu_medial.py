"""GPU tier of the medial axis (k_medial_axis in csrc/edt_medial.hip, edt_hip_medial_axis, edt.device.medial_axis): every comparison
is exact equality of the whole array, bit for bit, against the numpy restatement of the contract (tests/medial_oracle.py on
tests/ft_oracle.py), through edt.medial_axis on host arrays AND through edt.device.medial_axis on device tensors.
Shapes are the smallest at which the named thing can go wrong.  A wave of the kernel decides 62 voxels of x (the 64 lanes carry one
neighbour on either side), 4 rows of y and marches over 16 slices of z, four waves to a workgroup: extents around 62 and 64 lanes
and around two and four tiles of x, around 4 rows and 16 slices, and volumes of more than four tiles.  The grid is exact (one
wave per tile), so there is no second trip to cover.  The transforms are the library's own and are covered by their tiers."""
import ctypes
import itertools

import numpy as np
import pytest

import medial_oracle as oracle
from synth import bits_of, offset_out, offset_view, outside_intact, voronoi_labels
from test_gpu_thickness import ALL_DTYPES

pytestmark = pytest.mark.gpu

BLACK_BORDER, MORPH_BINARY = 1, 128
_SIGNED_VIEW = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
QUANTUM_SIZES = [(1.0, 1.0, 1.0), (6.0, 6.0, 30.0), (0.5, 0.5, 1.0)]            # (wx, wy, wz)
# array shapes, last axis x: x in {1, 2, 63, 64, 65, 129} and the kernel's 61 / 62 / 63 (one tile of x, +-1) and 124 / 125 (two);
# y, z in {1, 2, 3, 5, 17} and the kernel's 3 / 4 / 5 rows and 15 / 16 / 17 slices
SHAPES = [(1,), (2,), (63,), (64,), (65,), (129,), (250,),
          (1, 1), (2, 2), (3, 63), (5, 64), (17, 65), (4, 62), (5, 129), (9, 1), (3, 125), (8, 61),
          (1, 1, 1), (2, 3, 2), (5, 3, 63), (3, 5, 64), (17, 2, 65), (2, 5, 129), (15, 4, 5), (16, 5, 7), (17, 3, 6), (33, 4, 3),
          (3, 9, 62), (1, 5, 124), (5, 1, 61), (17, 17, 2), (5, 17, 1), (18, 9, 66)]


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
    """the same shape, dtype and bits, element by element, whatever the memory order of either"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes(order="C") == b.tobytes(order="C")


def to_device(a):
    """a numpy array as a device tensor of the same bits (unsigned 16/32/64-bit labels as the signed type of their width)"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED_VIEW[a.dtype]) if a.dtype in _SIGNED_VIEW else a).cuda()


def to_host(t, dtype):
    a = t.cpu().numpy()
    return a.view(dtype) if a.dtype != np.dtype(dtype) else a


def palette(dtype):
    """background and three labels: the extreme values of an integer type; for floats -0.0 (background), a NaN, a denormal"""
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return np.array([False, True, True, False])
    if dt.kind == "f":
        return np.array([0.0, 2.5, np.nan, -0.0, np.finfo(dt).smallest_subnormal, -np.inf], dtype=dt)
    info = np.iinfo(dt)
    return np.array([0, 1, info.max, info.min if info.min < 0 else info.max - 1], dtype=dt)


def labels_of(shape, dtype, seed):
    """blocks of 3 to 5 voxels of the palette's values: objects a few voxels thick, touching each other and the background"""
    rng = np.random.default_rng(seed)
    pal = palette(dtype)
    b = int(rng.integers(3, 6))
    lab = rng.integers(0, len(pal), size=tuple((s + b - 1) // b for s in shape))
    for axis, s in enumerate(shape):
        lab = np.repeat(lab, b, axis=axis).take(np.arange(s), axis=axis)
    return pal[lab]


def expected(data, on):
    out = data.copy(order="K")
    out[~on] = np.zeros((), dtype=data.dtype)
    return out


def cases():
    out = []
    for k, shape in enumerate(SHAPES + SHAPES):                   # every shape twice, seven steps apart in every cycle below
        k += 7 * (k // len(SHAPES))
        nd = len(shape)
        dtype = ALL_DTYPES[k % len(ALL_DTYPES)]
        w = QUANTUM_SIZES[k % 3][:nd]
        order = "F" if k % 2 else "C"
        an = w if order == "F" else w[::-1]                        # anisotropy in array axis order: x is axis 0 of an F array
        gamma, angle = [(None, 0.0), (None, 60.0), (0.0, 0.0), (1.5 * min(w), 0.0), (None, 120.0)][k % 5]
        out.append(pytest.param(shape, dtype, an, order, bool(k % 4 < 2), k % 3 == 2, gamma, angle,
                                id=f"{'x'.join(map(str, shape))}-{np.dtype(dtype).name}-{order}-{k}"))
    return out


@pytest.mark.parametrize("shape, dtype, an, order, bb, binary, gamma, angle", cases())
def test_end_to_end_against_the_oracle(shape, dtype, an, order, bb, binary, gamma, angle):
    """edt.medial_axis on the host array in its own memory order and edt.device.medial_axis on the same memory, with the radius"""
    import edt
    from edt import device
    # (SHAPES name x last: an F-ordered array has it first)
    data = labels_of(shape[::-1] if order == "F" else shape, dtype, seed=len(shape) * 100 + shape[-1])
    data = np.asfortranarray(data) if order == "F" else np.ascontiguousarray(data)
    fortran = data.flags.f_contiguous           # (also a C-ordered array with at most one axis longer than 1: edt._layout)
    kw = dict(gamma=gamma, min_angle=angle, anisotropy=an, black_border=bb, binary=binary)
    on = oracle.on_axis(data, **kw)
    want = expected(data, on)
    with np.errstate(invalid="ignore"):
        field = edt.edt((data != 0) if binary or data.dtype == bool else data, anisotropy=an, black_border=bb)
    want_radius = np.where(on, field, np.float32(0.0))
    got = edt.medial_axis(data, **kw)
    assert same_bytes(got, want) and got.flags.f_contiguous == data.flags.f_contiguous
    got, radius = edt.medial_axis(data, return_distance=True, **kw)
    assert same_bytes(got, want) and same_bytes(radius, want_radius)
    # the same memory as a device tensor: the transpose of an F-ordered array is C-ordered, its axes and voxel sizes reversed
    mem, an_mem = (data.T, an[::-1]) if fortran else (data, an)
    t = to_device(mem)
    got_t, radius_t = device.medial_axis(t, return_distance=True, **dict(kw, anisotropy=an_mem))
    assert same_bytes(to_host(got_t, dtype), np.ascontiguousarray(want.T if fortran else want))
    assert same_bytes(radius_t.cpu().numpy(), np.ascontiguousarray(want_radius.T if fortran else want_radius))
    assert same_bytes(to_host(device.medial_axis(t, **dict(kw, anisotropy=an_mem)), dtype), to_host(got_t, dtype))


def raw_step(t, planes, w, flags, gamma, ratio, out, field=None, radius=None):
    """edt_hip_medial_axis_step_device on tensors; w = (wx, wy, wz) of the tensor's reversed axes"""
    from edt import device
    nd = t.dim()
    ext = tuple(int(e) for e in t.shape[::-1]) + (1,) * (3 - nd)
    ww = tuple(float(np.float32(v)) for v in w) + (1.0,) * (3 - nd)
    ok(lib().edt_hip_medial_axis_step_device(vp(t), device.dtype_code(t.dtype), nd, *ext, *ww, vp(planes), flags, gamma, ratio, vp(out),
                                             vp(field), vp(radius), stream()))
    return out


@pytest.mark.parametrize("shape, an", [((6, 9, 70), (40.0, 3.58, 3.58)), ((5, 11, 64), (1.3, 0.7, 1.1)), ((17, 5, 9), (1.3, 0.7, 1.1)),
                                       ((13, 127), (0.7, 1.1)), ((300,), (3.58,))])
@pytest.mark.parametrize("bb", [False, True])
def test_step_alone_on_voxel_sizes_without_a_quantum(shape, an, bb):
    """the features are only bounded there, so the GPU's own feature transform feeds both the step and the oracle"""
    import torch
    from edt import device
    data = labels_of(shape, np.uint32, seed=7 + len(shape))
    t = to_device(data)
    planes = device.feature_transform(t, anisotropy=an, black_border=bb).flip(0).contiguous()       # x, y, z planes
    found = 0
    for gamma, angle in ((max(an), 0.0), (0.0, 45.0), (1.7 * min(an), 100.0)):
        on = oracle.on_axis(data, gamma=gamma, min_angle=angle, anisotropy=an, black_border=bb, features=planes.cpu().numpy())
        out = raw_step(t, planes, an[::-1], BLACK_BORDER if bb else 0, gamma, oracle.ratio_of(angle), torch.empty_like(t))
        assert same_bytes(to_host(out, np.uint32), expected(data, on)), (gamma, angle)
        found += int(on.sum())
    assert found > 0


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32, np.float64])
def test_offset_pointers_and_sentinels(dtype):
    """labels, features, field, out and radius each at an element offset of 1..3: the same bits, and nothing stored outside"""
    import torch
    from edt import device
    shape, an = (7, 6, 67), (1.0, 2.0, 1.0)
    data = labels_of(shape, dtype, seed=21)
    t = to_device(data)
    planes = device.feature_transform(t, anisotropy=an).flip(0).contiguous()
    field = device.edt(t, anisotropy=an)
    base_out, base_radius = torch.empty_like(t), torch.empty_like(field)
    raw_step(t, planes, an[::-1], 0, 1.0, 0.0, base_out, field, base_radius)
    assert bool((bits_of(base_out) != 0).any())
    size = np.dtype(dtype).itemsize
    mark = int.from_bytes(b"\xa5" * size, "little")
    for k in itertools.islice(itertools.product((0, 1, 2, 3), repeat=5), 1, None, 37):
        _, lab_v = offset_view(data, k[0])
        _, feat_v = offset_view(planes.cpu().numpy(), k[1])
        _, field_v = offset_view(field.cpu().numpy(), k[2])
        out_buf, out_v = offset_out(shape, dtype, k[3], mark)
        rad_buf, rad_v = offset_out(shape, np.float32, k[4], 0xA5A5A5A5)
        raw_step(lab_v, feat_v, an[::-1], 0, 1.0, 0.0, out_v, field_v, rad_v)
        assert np.array_equal(bits_of(out_v), bits_of(base_out)) and np.array_equal(bits_of(rad_v), bits_of(base_radius)), k
        assert outside_intact(out_buf, k[3], data.size, mark) and outside_intact(rad_buf, k[4], data.size, 0xA5A5A5A5), k
        # without a radius the field is not needed and the radius not written
        out_buf, out_v = offset_out(shape, dtype, k[3], mark)
        raw_step(lab_v, feat_v, an[::-1], 0, 1.0, 0.0, out_v)
        assert np.array_equal(bits_of(out_v), bits_of(base_out)) and outside_intact(out_buf, k[3], data.size, mark), k


@pytest.mark.parametrize("binary, bb", [(False, False), (True, True)])
def test_host_device_and_step_agree_on_a_volume_of_many_tiles(binary, bb):
    """40 x 50 x 130 voxels: 3 x 13 x 3 tiles, 30 workgroups -- the three layers give the same bits, the radius is the distance
    transform on the axis and +0.0 off it, and the axis is not trivial"""
    import torch
    import edt
    from edt import device
    data = np.ascontiguousarray(voronoi_labels((40, 50, 130), nseeds=12, seed=5, upsample=2, membrane=0.05).astype(np.uint16))
    an = (30.0, 6.0, 6.0)
    kw = dict(anisotropy=an, black_border=bb, binary=binary, min_angle=40.0)
    host, host_radius = edt.medial_axis(data, return_distance=True, **kw)
    t = to_device(data)
    dev, dev_radius = device.medial_axis(t, return_distance=True, **kw)
    assert same_bytes(to_host(dev, np.uint16), host) and same_bytes(dev_radius.cpu().numpy(), host_radius)
    of = (t != 0).to(torch.uint8) if binary else t
    planes = device.feature_transform(of, anisotropy=an, black_border=bb).flip(0).contiguous()
    out = raw_step(t, planes, an[::-1], (BLACK_BORDER if bb else 0) | (MORPH_BINARY if binary else 0), 30.0, oracle.ratio_of(40.0),
                   torch.empty_like(t))
    assert same_bytes(to_host(out, np.uint16), host)
    field = edt.edt((data != 0) if binary else data, anisotropy=an, black_border=bb)
    on = host != 0
    assert same_bytes(host_radius, np.where(on, field, np.float32(0.0)))
    assert 0 < on.sum() < (data != 0).sum() and np.array_equal(host[on], data[on])


def test_two_calls_of_one_shape_share_the_scratch_and_a_dirty_scratch_does_not_show():
    import torch
    from edt import device
    shape = (9, 11, 70)
    a, b = labels_of(shape, np.int32, seed=31), labels_of(shape, np.int32, seed=32)
    ta, tb = to_device(a), to_device(b)
    query = "edt_hip_medial_axis_workspace_bytes"
    cache = device._workspaces.setdefault(query, {})
    cache.clear()
    kw = dict(black_border=True, return_distance=True, binary=True)
    first, first_radius = device.medial_axis(ta, **kw)
    assert len(cache) == 1
    scratch = next(iter(cache.values()))
    ext = shape[::-1]
    assert scratch.numel() == getattr(lib(), query)(2, 3, *ext, BLACK_BORDER | MORPH_BINARY, 1) > 4 * 4 * ta.numel()
    where = scratch.data_ptr()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    other, _ = device.medial_axis(tb, **kw)
    again, again_radius = device.medial_axis(ta, **kw)
    torch.cuda.synchronize()
    # a second call of one shape allocates only what it returns: an axis and a radius each
    assert torch.cuda.memory_allocated() - before <= 4 * (ta.numel() * 4 + 2048)
    assert len(cache) == 1 and next(iter(cache.values())) is scratch and scratch.data_ptr() == where
    assert torch.equal(first, again) and torch.equal(first_radius, again_radius) and not torch.equal(first, other)
    # whatever the scratch holds
    scratch.fill_(0x7F)
    dirty, dirty_radius = device.medial_axis(ta, **kw)
    assert torch.equal(first, dirty) and torch.equal(first_radius, dirty_radius)
    assert same_bytes(to_host(first, np.int32), oracle.medial_axis(a, black_border=True, binary=True))
    # another dtype of the same shape under binary transforms the same mask: the same bytes, the same scratch
    device.medial_axis(to_device(a.astype(np.uint8)), **kw)
    assert len(cache) == 1
    device.medial_axis(ta, black_border=True)
    assert len(cache) == 2
