"""GPU tier of fill_holes (csrc/edt_fillholes.hip): every comparison is exact equality of the whole array, byte for byte, and of
the fill count against the numpy restatement of the contract (tests/fill_holes_oracle.py), through edt.fill_holes (host
buffers) and edt.device.fill_holes (device arrays).  Shapes are the smallest at which the named thing can go wrong: the forest
of the background works in 64-voxel groups, 256-voxel steps and 2048-voxel chunks, the sweeps of the fill in waves of 64."""
import ctypes
import itertools

import numpy as np
import pytest

import fill_holes_oracle as oracle
from synth import blob_mask

pytestmark = pytest.mark.gpu

U8, U16, U32, U64, F32, F64, BOOL = range(7)
_SIGNED_VIEW = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes(order="A") == b.tobytes(order="A")


def on_device(data, c, binary):
    """edt.device.fill_holes of the same memory: (out as a numpy array laid out like `data`, n_filled)."""
    import torch
    from edt import device
    a = data if data.flags.c_contiguous else data.T                # the C-ordered view of the same memory
    v = a.view(_SIGNED_VIEW[a.dtype]) if a.dtype in _SIGNED_VIEW else a
    t = torch.from_numpy(v).cuda()
    out, n = device.fill_holes(t, connectivity=c, binary=binary)
    assert out.dtype == t.dtype and out.shape == t.shape and out.data_ptr() != t.data_ptr()
    assert n.dtype == torch.int64 and n.dim() == 0 and n.is_cuda
    got = out.cpu().numpy().view(a.dtype)
    return (got if data.flags.c_contiguous else got.T), int(n)


def check(edt, data, c=None, binary=False, n=None):
    want = oracle.fill_holes(data, c, binary=binary)
    got, gn = edt.fill_holes(data, connectivity=c, binary=binary, return_fill_count=True)
    assert got.flags.f_contiguous == data.flags.f_contiguous and got.flags.c_contiguous == data.flags.c_contiguous
    assert gn == want.n_filled, (gn, want.n_filled)
    assert same_bytes(got, want.out)
    dev, dn = on_device(data, c, binary)
    assert dn == want.n_filled and same_bytes(np.asarray(dev, order="A"), want.out)
    if n is not None:
        assert gn == n, (gn, n)
    return got, want


def fvol(shape, dtype=np.uint8, fill=0):
    return np.full(shape, fill, dtype=dtype, order="F")          # axis 0 is x


def walled(lab, label=1):
    """`lab` with a wall of `label` along every face."""
    for axis in range(lab.ndim):
        sl = [slice(None)] * lab.ndim
        for k in (0, -1):
            sl[axis] = k
            lab[tuple(sl)] = label
    return lab


# ---- run and wave boundaries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sx", [1, 63, 64, 65, 130, 1025])
def test_run_and_wave_boundaries(edt_gpu, sx):
    rng = np.random.default_rng(sx)
    lab = fvol((sx, 5, 3))
    for z, y in itertools.product(range(3), range(5)):
        x = 0
        while x < sx:                                   # random runs of 0 / 0 / 1 / 2, 1 to 90 voxels long
            run = int(rng.integers(1, 91))
            lab[x:x + run, y, z] = max(0, int(rng.integers(-1, 3)))
            x += run
    walled(lab)
    total = 0
    for c in (1, 2, 3):
        _, want = check(edt_gpu, lab, c)
        check(edt_gpu, lab, c, binary=True)
        total += want.cavities
    assert total > 0 or sx == 1


def test_a_cavity_across_group_and_step_boundaries(edt_gpu):
    lab = fvol((130, 5, 3), np.uint16, fill=9)
    lab[1:129, 2, 1] = 0                                # idx 911 .. 1038 of the flattened volume: across 960 and 1024
    first, last = 1 + 130 * (2 + 5 * 1), 128 + 130 * (2 + 5 * 1)
    assert first < 960 < last and first < 1024 < last and 960 % 64 == 0 and 1024 % 256 == 0
    for c in (1, 2, 3):
        got, _ = check(edt_gpu, lab, c, n=128)
        assert np.all(got == 9)
    lab[128, 2, 1] = 9
    lab[129, 2, 1] = 0                                  # the same row ends in an open voxel: one cavity, one open component
    check(edt_gpu, lab, 1, n=127)
    lab = fvol((70, 3, 3), np.uint16, fill=9)
    lab[64, 1, 1] = 0                                   # a cavity of one voxel
    check(edt_gpu, lab, 3, n=1)


# ---- open versus closed --------------------------------------------------------------------------------------------
def test_open_versus_closed(edt_gpu):
    for axis, side in itertools.product(range(3), (0, -1)):
        lab = fvol((6, 7, 5), np.uint32, fill=5)
        p = [2, 3, 2]
        p[axis] = side
        lab[tuple(p)] = 0                               # on the face: open
        for c in (1, 2, 3):
            check(edt_gpu, lab, c, n=0)
        lab[tuple(p)] = 5
        p[axis] = 1 if side == 0 else lab.shape[axis] - 2
        lab[tuple(p)] = 0                               # one voxel inside it: closed
        for c in (1, 2, 3):
            got, _ = check(edt_gpu, lab, c, n=1)
            assert got[tuple(p)] == 5
    for thin in (1, 2):                                 # an axis of extent 1 or 2: every voxel lies on the boundary
        for axis in range(3):
            shape = [7, 7, 7]
            shape[axis] = thin
            lab = fvol(tuple(shape), np.uint8, fill=3)
            lab[tuple(s // 2 for s in shape)] = 0
            for c in (1, 2, 3):
                check(edt_gpu, lab, c, n=0)
                check(edt_gpu, np.ascontiguousarray(lab), c, n=0)
    # ... while the same plane as a 2-D array has a cavity
    img = fvol((7, 7), np.uint8, fill=3)
    img[3, 3] = 0
    check(edt_gpu, img, 1, n=1)
    check(edt_gpu, fvol((70, 9, 4), np.uint32), None, n=0)          # all background
    check(edt_gpu, fvol((70, 9, 4), np.uint32, fill=4), None, n=0)  # all foreground


# ---- connectivity really differs -----------------------------------------------------------------------------------
def test_connectivity_really_differs(edt_gpu):
    lab = fvol((5, 5, 5), fill=1)
    lab[1, 1, 2] = lab[0, 0, 2] = 0                     # reaches the outside through an edge-diagonal only
    for c, n in ((1, 1), (2, 0), (3, 0)):
        check(edt_gpu, lab, c, n=n)
    lab = fvol((5, 5, 5), fill=1)
    lab[1, 1, 1] = lab[0, 0, 0] = 0                     # ... through a corner-diagonal only
    for c, n in ((1, 1), (2, 1), (3, 0)):
        check(edt_gpu, lab, c, n=n)
    lab = fvol((5, 5, 5), fill=1)
    lab[3, 3, 3] = lab[4, 4, 4] = 0                     # the same at the far corner
    for c, n in ((1, 1), (2, 1), (3, 0)):
        check(edt_gpu, lab, c, n=n)
    img = fvol((5, 4), fill=1)
    img[1, 1] = img[0, 0] = 0                           # the 2-D analogue
    for c, n in ((1, 1), (2, 0), (4, 1), (8, 0)):
        got = edt_gpu.fill_holes(img, connectivity=c, return_fill_count=True)
        assert got[1] == n and same_bytes(got[0], oracle.fill_holes(img, 1 if c in (1, 4) else 2).out)
    lab = fvol((5, 5, 5), fill=1)
    lab[2, 2, 2] = 0
    lab[3, 3, 3] = 2                                    # a second label that touches the cavity at a corner only
    for c, n in ((1, 1), (2, 1), (3, 0)):
        _, want = check(edt_gpu, lab, c, n=n)
        assert want.mixed_cavities == (1 if c == 3 else 0)
    check(edt_gpu, lab, 3, binary=True, n=1)
    # None is 1
    lab = fvol((5, 5, 5), fill=1)
    lab[1, 1, 2] = lab[0, 0, 2] = 0
    assert edt_gpu.fill_holes(lab, return_fill_count=True)[1] == 1


# ---- representative and mixed --------------------------------------------------------------------------------------
def test_representative(edt_gpu):
    got, _ = check(edt_gpu, np.array([7, 0, 8], dtype=np.uint8), 1, binary=True, n=1)    # voxel 0 is the representative:
    assert got.tolist() == [7, 7, 8]                                                      # its state is 0 + 1, not "open"
    check(edt_gpu, np.array([7, 0, 8], dtype=np.uint8), 1, n=0)
    lab = fvol((3, 3, 3), np.uint16, fill=7)
    lab[1, 1, 1] = 0
    lab[0, 0, 0] = 9
    got, _ = check(edt_gpu, lab, 3, binary=True, n=1)   # voxel 0 is a wall voxel at c = 3 only
    assert got[1, 1, 1] == 9
    got, _ = check(edt_gpu, lab, 2, binary=True, n=1)
    assert got[1, 1, 1] == 7
    check(edt_gpu, lab, 3, n=0)
    got, _ = check(edt_gpu, lab, 2, n=1)
    assert got[1, 1, 1] == 7
    lab = fvol((5, 5, 5), np.uint32, fill=1)
    lab[2, 2, 2] = 0
    lab[2, 2, 3] = 2                                    # the differing wall voxel is the last one in memory order
    check(edt_gpu, lab, 1, n=0)
    got, _ = check(edt_gpu, lab, 1, binary=True, n=1)
    assert got[2, 2, 2] == 1


def test_label_values(edt_gpu):
    one = np.uint64(1)
    lab = fvol((5, 5, 5), np.uint64, fill=1)
    lab[2, 2, 2] = 0
    lab[3, 2, 2] = one + (one << np.uint64(32))         # differs in the high half only: mixed
    check(edt_gpu, lab, 1, n=0)
    lab[:] = one + (one << np.uint64(32))
    lab[2, 2, 2] = 0
    got, _ = check(edt_gpu, lab, 1, n=1)
    assert got[2, 2, 2] == one + (one << np.uint64(32))
    check(edt_gpu, lab.view(np.int64), 3, n=1)
    for dt in (np.float32, np.float64):
        lab = fvol((5, 5, 5), dt, fill=2.5)
        lab[2, 2, 2] = 0
        lab[2, 3, 2] = np.nan                           # one NaN in the wall: mixed; filled under binary
        check(edt_gpu, lab, 1, n=0)
        check(edt_gpu, lab, 1, binary=True, n=1)
        lab[2, 1, 2] = np.nan                           # ... also when the NaN is the representative
        lab[2, 2, 1] = 2.5
        lab[:, :, 0] = np.nan
        check(edt_gpu, lab, 1, n=0)
        got, _ = check(edt_gpu, lab, 1, binary=True, n=1)
        assert got[2, 2, 2] == 2.5 or np.isnan(got[2, 2, 2])
        lab = fvol((5, 5, 5), dt, fill=2.5)
        lab[2, 2, 2] = -0.0                             # -0.0 is background: filled, and counted
        lab[0, 0, 0] = -0.0                             # ... and an open one keeps its sign bit
        got, _ = check(edt_gpu, lab, 1, n=1)
        assert got[2, 2, 2] == 2.5 and np.signbit(got[0, 0, 0])


def test_nested(edt_gpu):
    lab = fvol((9, 9, 9), np.uint8, fill=1)
    lab[1:8, 1:8, 1:8] = 0
    lab[3:6, 3:6, 3:6] = 2
    lab[4, 4, 4] = 0                                    # A holds a cavity that holds an island B with a cavity of its own
    for c in (1, 2, 3):
        got, want = check(edt_gpu, lab, c, n=1)
        assert got[4, 4, 4] == 2 and got[1, 1, 1] == 0 and (want.filled_cavities, want.mixed_cavities) == (1, 1)
    got, _ = check(edt_gpu, lab, 1, binary=True, n=7 ** 3 - 3 ** 3 + 1)
    assert got[1, 1, 1] == 1 and got[4, 4, 4] == 2 and got[3, 3, 3] == 2


# ---- contention ----------------------------------------------------------------------------------------------------
def test_contention(edt_gpu):
    box = walled(fvol((66, 10, 6), np.uint32), 3)       # one cavity, 2048 voxels, every wall voxel on one word
    for c in (1, 2, 3):
        got, _ = check(edt_gpu, box, c, n=64 * 8 * 4)
        assert np.all(got == 3)
    box[65, 9, 5] = 4                                   # a corner of the box: a wall voxel at c = 3 only, and the last one
    check(edt_gpu, box, 2, n=2048)
    check(edt_gpu, box, 3, n=0)
    box[65, 8, 4] = 4                                   # the last wall voxel in memory order
    check(edt_gpu, box, 1, n=0)
    check(edt_gpu, box, 1, binary=True, n=2048)
    block = fvol((33, 17, 9), np.uint32, fill=1)        # a lattice of one-voxel cavities: many roots
    block[17:, :, :] = 2
    block[1:32:2, 1:16:2, 1:8:2] = 0
    for c in (1, 2, 3):
        _, want = check(edt_gpu, block, c)
        assert want.cavities == 16 * 8 * 4 and want.mixed_cavities == 8 * 4      # (those at x = 17, between the two labels)
        check(edt_gpu, block, c, binary=True, n=16 * 8 * 4)


# ---- every dtype, both orders, fewer dimensions --------------------------------------------------------------------
BASE = oracle.random_volume(11)


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64,
                                   np.float32, np.float64, bool])
def test_every_dtype(edt_gpu, dtype):
    dt = np.dtype(dtype)
    if dt == np.bool_:
        lab = BASE != 0
    else:
        lab = BASE.astype(dt)
        if dt.kind == "i":
            lab[BASE == 3] = -3
        if dt.kind == "f":
            lab[BASE == 3] = -2.5
            lab[BASE == 2] = np.inf
        if dt.itemsize == 8 and dt.kind == "u":
            lab[BASE == 2] = (1 << 63) + 2
    for data in (np.asfortranarray(lab), np.ascontiguousarray(lab)):
        _, want = check(edt_gpu, data, 1)
        assert want.filled_cavities >= 5 and (want.mixed_cavities >= 5 or dt == np.bool_)
        check(edt_gpu, data, 3)
        check(edt_gpu, data, 2, binary=True)
    img = lab[:, :, 5]
    for data in (np.asfortranarray(img), np.ascontiguousarray(img)):
        for c in (1, 2):
            check(edt_gpu, data, c)
    line = np.ascontiguousarray(lab[:, 7, 5])
    _, want = check(edt_gpu, line, 1)
    check(edt_gpu, line, None, binary=True)


def test_bool_bytes_through_the_abi(edt_gpu):
    from edt import _lib
    lib = _lib.load()
    lab = np.array([1, 0, 2, 0, 0, 255, 7, 0], dtype=np.uint8)

    def call(code, binary):
        out, n = np.full(8, 99, dtype=np.uint8), ctypes.c_int64(-1)
        _lib.check(lib.edt_hip_fill_holes(ctypes.c_void_p(lab.ctypes.data), code, 1, 8, 1, 1, 1, binary,
                                          ctypes.c_void_p(out.ctypes.data), ctypes.byref(n)))
        return out.tolist(), n.value

    for binary in (0, 1):                               # EDT_BOOL: any non-zero byte is foreground, always binary; the
        assert call(BOOL, binary) == ([1, 1, 2, 2, 2, 255, 7, 0], 3)     # representative's own byte is what fills
    assert call(U8, 1) == ([1, 1, 2, 2, 2, 255, 7, 0], 3)
    assert call(U8, 0) == (lab.tolist(), 0)             # the same bytes as uint8 labels: values decide, both cavities are mixed


# ---- random volumes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_random_volumes(edt_gpu, seed):
    lab = oracle.random_volume(seed)
    for c in (1, 2, 3):
        _, want = check(edt_gpu, lab, c)
        assert want.cavities >= 20 and want.filled_cavities >= 5 and want.mixed_cavities >= 5, (c, want[1:])
        check(edt_gpu, lab, c, binary=True)


# ---- entry points --------------------------------------------------------------------------------------------------
def test_determinism_and_dirty_scratch(edt_gpu):
    """The same call twice gives the same bytes -- also through the ABI on a reused workspace and output full of other bits, and
    the phases are named in the pass log."""
    import torch
    from edt import _lib, device
    lib = _lib.load()
    lab = oracle.random_volume(3)
    want = oracle.fill_holes(lab, 2)
    a, na = edt_gpu.fill_holes(lab, connectivity=2, return_fill_count=True)
    b, nb = edt_gpu.fill_holes(lab, connectivity=2, return_fill_count=True)
    assert na == nb == want.n_filled and same_bytes(a, b) and same_bytes(a, want.out)
    t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).cuda()
    ext = tuple(int(e) for e in t.shape[::-1])
    ws = torch.empty(lib.edt_hip_fill_holes_workspace_bytes(U32, 3, *ext), dtype=torch.uint8, device="cuda")
    vp = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    first = None
    for fill in (0xFF, 0x00, 0x5A, 0x80):
        ws.fill_(fill)
        out = torch.full(t.shape, -7, dtype=torch.int32, device="cuda")
        n = torch.full((), -1, dtype=torch.int64, device="cuda")
        for _ in range(2):
            _lib.check(lib.edt_hip_fill_holes_device(vp(t), U32, 3, *ext, 2, 0, vp(out), vp(n), vp(ws), ws.numel(),
                                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            assert int(n) == want.n_filled
            first = out.clone() if first is None else first
            assert torch.equal(out, first)
    assert same_bytes(first.cpu().numpy().view(np.uint32).T, want.out)
    device.set_profiling(True)
    try:
        device.fill_holes(t, connectivity=2)
        torch.cuda.synchronize()
        names = [name for name, _ in device.pass_times()]
        device.fill_holes(t, connectivity=2, binary=True)
        torch.cuda.synchronize()
        binary_names = [name for name, _ in device.pass_times()]
    finally:
        device.set_profiling(False)
    phases = ["mask", "rows", "merge", "flatten", "mark", "check", "fill"]
    assert names == ["fill_holes " + p for p in phases]
    assert binary_names == ["fill_holes " + p for p in phases if p != "check"]
    # empty input
    e, n = device.fill_holes(torch.zeros((0, 4), dtype=torch.int32, device="cuda"))
    assert e.shape == (0, 4) and int(n) == 0
    out, n = edt_gpu.fill_holes(np.zeros((3, 0, 2), dtype=np.float64), return_fill_count=True)
    assert out.shape == (3, 0, 2) and n == 0


# ---- composition ---------------------------------------------------------------------------------------------------
def test_composes_with_the_transform_on_the_device(edt_gpu):
    import torch
    from edt import device
    rng = np.random.default_rng(8)
    lab = blob_mask((48, 40, 36), rng=rng, p=0.6, block=6).astype(np.uint8)
    lab[rng.random(lab.shape) < 0.01] = 0               # pin-holes inside the blobs
    lab = np.ascontiguousarray(lab)
    want = oracle.fill_holes(lab, 1)
    assert want.n_filled > 50
    filled, n = device.fill_holes(torch.from_numpy(lab).cuda())
    dt = device.edt(filled)
    assert int(n) == want.n_filled
    ref = edt_gpu.edt(want.out)
    assert np.array_equal(dt.cpu().numpy(), ref)
    assert not np.array_equal(ref, edt_gpu.edt(lab))    # the holes did pin the field
