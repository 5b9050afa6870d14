"""GPU tier of dust (csrc/edt_dust.hip): every comparison is exact equality of the whole array, byte for byte, and of the three
counts against the numpy restatement of the contract (tests/dust_oracle.py), through edt.dust (host buffers) and
edt.device.dust (device arrays).  Shapes are the smallest at which the named thing can go wrong: the forest works in 64-voxel
groups, 256-voxel steps and 2048-voxel chunks, the count in 64-voxel groups, batches of four of them and spans of
EDT_HIP_DUST_COUNT_SPAN voxels per wave (read from the header), the filter in waves of 64."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import dust_oracle as oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu

U8, U16, U32, U64, F32, F64, BOOL = range(7)
INT64_MAX = (1 << 63) - 1
_SIGNED_VIEW = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
SPAN = int(re.search(r"^#define EDT_HIP_DUST_COUNT_SPAN (\d+)$", open(os.path.join(ROOT, "include", "edt_hip.h")).read(),
                     flags=re.M).group(1))


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes(order="A") == b.tobytes(order="A")


def to_device(data):
    """The C-ordered view of the same memory as a device tensor (unsigned types wider than a byte as their signed views)."""
    import torch
    a = data if data.flags.c_contiguous else data.T
    v = a.view(_SIGNED_VIEW[a.dtype]) if a.dtype in _SIGNED_VIEW else a
    return torch.from_numpy(np.ascontiguousarray(v)).cuda(), a


def on_device(data, threshold, c, binary, invert, in_place=False):
    """edt.device.dust of the same memory: (out as a numpy array laid out like `data`, the three counts)."""
    import torch
    from edt import device
    t, a = to_device(data)
    out, counts = device.dust(t, threshold, connectivity=c, binary=binary, invert=invert, in_place=in_place)
    assert out.dtype == t.dtype and out.shape == t.shape and (out.data_ptr() == t.data_ptr()) == in_place and (out is t) == in_place
    assert counts.dtype == torch.int64 and counts.shape == (3,) and counts.is_cuda
    got = out.cpu().numpy().view(a.dtype)
    return (got if data.flags.c_contiguous else got.T), tuple(int(v) for v in counts.cpu())


def check(edt, data, threshold, c=None, binary=False, invert=False, counts=None):
    want = oracle.dust(data, threshold, c, binary=binary, invert=invert)
    got, gc = edt.dust(data, threshold, connectivity=c, binary=binary, invert=invert, return_counts=True)
    assert got.flags.f_contiguous == data.flags.f_contiguous and got.flags.c_contiguous == data.flags.c_contiguous
    assert tuple(gc) == want[1:], (tuple(gc), want[1:])
    assert same_bytes(got, want.out)
    dev, dc = on_device(data, threshold, c, binary, invert)
    assert dc == want[1:] and same_bytes(np.asarray(dev, order="A"), want.out)
    if counts is not None:
        assert tuple(gc) == counts, (tuple(gc), counts)
    return got, want


def fvol(shape, dtype=np.uint8, fill=0):
    return np.full(shape, fill, dtype=dtype, order="F")          # axis 0 is x


# ---- group, step, chunk and span boundaries --------------------------------------------------------------------------
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
    removed = 0
    for c in (1, 2, 3):
        for threshold in (40, (20, 200)):
            _, want = check(edt_gpu, lab, threshold, c)
            check(edt_gpu, lab, threshold, c, binary=True)
            removed += want.removed_voxels
    assert removed > 0 or sx == 1


def test_one_run_across_group_and_step_boundaries(edt_gpu):
    lab = fvol((130, 5, 3), np.uint16)
    lab[1:129, 2, 1] = 9                                # idx 911 .. 1038 of the flattened volume: across 960 and 1024
    first, last = 1 + 130 * (2 + 5 * 1), 128 + 130 * (2 + 5 * 1)
    assert first < 960 < last and first < 1024 < last and 960 % 64 == 0 and 1024 % 256 == 0
    for c in (1, 2, 3):
        check(edt_gpu, lab, 128, c, counts=(1, 1, 0))   # its size is counted once: 128, not 129 and not two parts
        check(edt_gpu, lab, 129, c, counts=(1, 0, 128))
        check(edt_gpu, lab, (128, 129), c, counts=(1, 1, 0))
        check(edt_gpu, lab, (127, 128), c, counts=(1, 0, 128))


def test_a_component_across_a_span_boundary(edt_gpu):
    """A wave of the count kernel walks SPAN consecutive voxels and carries its open stretch across the 64-voxel groups; the
    next wave starts a stretch of its own at the boundary.  One x-run across flattened idx SPAN, one that ends exactly at it and
    one that starts exactly at it -- and a volume of several spans filled by one component."""
    sx = SPAN // 8 + 40
    lab = fvol((sx, 9, 2), np.uint32)
    assert lab.size > SPAN + sx
    y, x = divmod(SPAN, sx)                             # voxel (x, y, 0) is idx SPAN
    assert 20 < x < sx - 20 and y < 8
    lab[x - 17:x + 13, y, 0] = 5                        # across: 30 voxels
    lab[x - 9:x, y, 1] = 6                              # (other rows, for contrast: 9 and 11 voxels)
    lab[x:x + 11, y + 1, 1] = 7
    flat = lab.reshape(-1, order="F")
    assert flat[SPAN - 17] == 5 and flat[SPAN + 12] == 5 and flat[SPAN - 18] == 0 and flat[SPAN + 13] == 0
    check(edt_gpu, lab, 30, 1, counts=(3, 1, 20))
    check(edt_gpu, lab, 31, 1, counts=(3, 0, 50))
    check(edt_gpu, lab, (10, 30), 1, counts=(3, 1, 39))
    lab[:] = 0
    lab[x - 12:x, y, 0] = 5                             # ends at idx SPAN - 1
    lab[x:x + 7, y + 1, 0] = 5
    flat = lab.reshape(-1, order="F")
    assert flat[SPAN - 1] == 5 and flat[SPAN] == 0
    check(edt_gpu, lab, 12, 1, counts=(2, 1, 7))
    lab[:] = 0
    lab[x:x + 12, y, 0] = 5                             # starts at idx SPAN: its root is a span's first voxel
    assert lab.reshape(-1, order="F")[SPAN] == 5 and lab.reshape(-1, order="F")[SPAN - 1] == 0
    check(edt_gpu, lab, 12, 1, counts=(1, 1, 0))
    check(edt_gpu, lab, 13, 1, counts=(1, 0, 12))
    solid = fvol((sx, 9, 3), np.uint32, fill=4)         # more than three spans, one component
    assert solid.size > 3 * SPAN and solid.size % SPAN != 0
    check(edt_gpu, solid, solid.size, 1, counts=(1, 1, 0))
    check(edt_gpu, solid, solid.size + 1, 3, counts=(1, 0, solid.size))


# ---- threshold edges -------------------------------------------------------------------------------------------------
def test_threshold_edges(edt_gpu):
    k = 7
    lab = fvol((40, 6, 4), np.uint32)
    lab[2:2 + k - 1, 1, 1] = 3                          # sizes k - 1, k, k + 1
    lab[12:12 + k, 3, 1] = 3
    lab[22:22 + k + 1, 1, 3] = 3
    fg = 3 * k

    def present(out):
        return tuple(bool(out[p] != 0) for p in ((2, 1, 1), (12, 3, 1), (22, 1, 3)))

    got, _ = check(edt_gpu, lab, k, counts=(3, 2, k - 1))
    assert present(got) == (False, True, True)
    got, _ = check(edt_gpu, lab, (k, k + 1), counts=(3, 1, 2 * k))
    assert present(got) == (False, True, False)
    got, _ = check(edt_gpu, lab, k, invert=True, counts=(3, 1, 2 * k + 1))
    assert present(got) == (True, False, False)
    got, _ = check(edt_gpu, lab, (k, k + 1), invert=True, counts=(3, 2, k))
    assert present(got) == (True, False, True)
    for t in (0, 1):
        got, _ = check(edt_gpu, lab, t, counts=(3, 3, 0))
        assert same_bytes(got, lab)
    got, _ = check(edt_gpu, lab, lab.size + 1, counts=(3, 0, fg))
    assert not got.any()
    check(edt_gpu, lab, (k, k), counts=(3, 0, fg))      # an empty range keeps nothing
    check(edt_gpu, lab, (0, INT64_MAX), counts=(3, 3, 0))


def test_a_size_past_16_bits(edt_gpu):
    lab = fvol((70, 40, 30), np.uint8, fill=1)          # 84 000 voxels
    assert lab.size == 84000 > 65535
    check(edt_gpu, lab, 84000, counts=(1, 1, 0))
    check(edt_gpu, lab, 84001, counts=(1, 0, 84000))


# ---- many roots, contention ------------------------------------------------------------------------------------------
def test_many_roots(edt_gpu):
    x, y, z = np.meshgrid(np.arange(33), np.arange(17), np.arange(9), indexing="ij")
    board = np.asfortranarray(((x + y + z) % 2).astype(np.uint32))
    n = int(board.sum())
    got, _ = check(edt_gpu, board, 2, 1, counts=(n, 0, n))          # every foreground voxel its own component
    assert not got.any()
    check(edt_gpu, board, 1, 1, counts=(n, n, 0))
    check(edt_gpu, board, 2, 3, counts=(1, 1, 0))                   # ... and one component through the corners
    check(edt_gpu, board, n + 1, 3, counts=(1, 0, n))
    check(edt_gpu, board, n, 2, counts=(1, 1, 0))
    # stretches of one voxel that alternate between two roots, and between more roots than a wave of the count keeps sums for
    two = np.asfortranarray((1 + (x + y + z) % 2).astype(np.uint32))
    check(edt_gpu, two, n + 1, 2, counts=(2, 1, n))
    check(edt_gpu, two, 2, 1, counts=(two.size, 0, two.size))
    planes = np.asfortranarray((1 + x % 7).astype(np.uint32))       # 33 components of 17 * 9 voxels, seven labels in turn
    check(edt_gpu, planes, 17 * 9, 1, counts=(33, 33, 0))
    check(edt_gpu, planes, 17 * 9 + 1, 1, counts=(33, 0, planes.size))
    check(edt_gpu, planes, 17 * 9 + 1, 3, binary=True, counts=(1, 1, 0))


def test_contention(edt_gpu):
    box = fvol((66, 10, 6), np.uint32, fill=3)          # every stretch adds to one word
    for c in (1, 2, 3):
        check(edt_gpu, box, box.size, c, counts=(1, 1, 0))
        check(edt_gpu, box, box.size + 1, c, counts=(1, 0, box.size))
    box[33:, :, :] = 4                                  # two labels: two components, one under binary
    half = 33 * 10 * 6
    for c in (1, 3):
        check(edt_gpu, box, half, c, counts=(2, 2, 0))
        check(edt_gpu, box, half + 1, c, counts=(2, 0, 2 * half))
        check(edt_gpu, box, half + 1, c, binary=True, counts=(1, 1, 0))
        check(edt_gpu, box, 2 * half + 1, c, binary=True, counts=(1, 0, 2 * half))


# ---- sparse random volumes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("seed", range(5))
def test_sparse_volumes(edt_gpu, seed, binary):
    lab = oracle.sparse_volume(seed, 0.12 if binary else 0.45)
    for c in (1, 2, 3):
        _, want = check(edt_gpu, lab, 4, c, binary=binary)
        assert want.removed_voxels >= 20 and want.kept >= 20 and want.components - want.kept >= 20, (c, want[1:])
        _, want = check(edt_gpu, lab, (3, 9), c, binary=binary)
        assert want.kept >= 20 and want.kept == oracle.in_range(lab, 3, 9, c, binary), (c, want[1:])
        if seed == 2:
            check(edt_gpu, lab, 4, c, binary=binary, invert=True)
            check(edt_gpu, lab, (3, 9), c, binary=binary, invert=True)


# ---- every dtype, both orders, fewer dimensions ----------------------------------------------------------------------
BASE = oracle.sparse_volume(11, 0.45, shape=(18, 18, 12))


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
            lab[(BASE == 0) & (np.arange(18)[:, None, None] % 2 == 1)] = -0.0
        if dt.itemsize == 8 and dt.kind == "u":
            lab[BASE == 2] = (1 << 63) + 2
            lab[BASE == 3] = (1 << 32) + 1              # differs from label 1 in the high half only
    for data in (np.asfortranarray(lab), np.ascontiguousarray(lab)):
        _, want = check(edt_gpu, data, 4, 1)
        assert (want.kept >= 5 and want.components - want.kept >= 5) or dt == np.bool_
        check(edt_gpu, data, (2, 6), 3)
        check(edt_gpu, data, 5, 2, binary=True, invert=True)
    img = lab[:, :, 5]
    for data in (np.asfortranarray(img), np.ascontiguousarray(img)):
        for c in (1, 2):
            _, want = check(edt_gpu, data, 3, c)
            assert want.removed_voxels > 0 and want.kept > 0
    line = np.ascontiguousarray(lab[:, 7, 5])
    check(edt_gpu, line, 2, 1)
    check(edt_gpu, line, 2, None, binary=True)


def test_label_values(edt_gpu):
    one = np.uint64(1)
    high = one + (one << np.uint64(32))
    lab = fvol((6, 3, 1), np.uint64)
    lab[0:3, 1, 0] = 1
    lab[3:6, 1, 0] = high                               # differs in the high half only: two components of 3, not one of 6
    check(edt_gpu, lab, 4, counts=(2, 0, 6))
    got, _ = check(edt_gpu, lab, 3, counts=(2, 2, 0))
    assert got[5, 1, 0] == high
    check(edt_gpu, lab, 4, binary=True, counts=(1, 1, 0))
    check(edt_gpu, lab.view(np.int64), 4, counts=(2, 0, 6))
    neg = fvol((6, 3, 1), np.int32)
    neg[0:3, 1, 0] = -1
    neg[3:5, 1, 0] = -2
    got, _ = check(edt_gpu, neg, 3, counts=(2, 1, 2))
    assert got[:, 1, 0].tolist() == [-1, -1, -1, 0, 0, 0]
    for dt in (np.float32, np.float64):
        lab = fvol((12, 3, 1), dt)
        lab[0:2, 1, 0] = 2.5
        lab[2, 1, 0] = np.nan                           # a NaN voxel: a component of size 1 between two others
        lab[3:5, 1, 0] = 2.5
        lab[6:8, 1, 0] = np.inf
        lab[9, 1, 0] = -0.0                             # background: copied with its sign
        lab[10, 1, 0] = -2.5
        got, _ = check(edt_gpu, lab, 2, counts=(5, 3, 2))
        assert got[2, 1, 0] == 0 and not np.signbit(got[2, 1, 0]) and np.signbit(got[9, 1, 0]) and got[10, 1, 0] == 0
        assert np.isinf(got[6, 1, 0]) and got[0, 1, 0] == 2.5
        got, _ = check(edt_gpu, lab, 5, binary=True, counts=(3, 1, 3))     # under binary the NaN joins its neighbours: 5 voxels
        assert same_bytes(got[:5], lab[:5]) and np.isnan(got[2, 1, 0]) and np.signbit(got[9, 1, 0])
        payload = lab.copy()
        bits = payload.view(np.uint32 if dt == np.float32 else np.uint64)
        bits[2, 1, 0] |= 0x1234                         # a NaN's payload survives where it is kept
        got, _ = check(edt_gpu, payload, 1, counts=(5, 5, 0))
        assert same_bytes(got, payload)


def test_bool_bytes_through_the_abi(edt_gpu):
    from edt import _lib
    lib = _lib.load()
    lab = np.array([1, 2, 0, 255, 0, 7, 7, 9], dtype=np.uint8)

    def call(code, binary, t):
        out, counts = np.full(8, 99, dtype=np.uint8), np.full(3, -1, dtype=np.int64)
        _lib.check(lib.edt_hip_dust(ctypes.c_void_p(lab.ctypes.data), code, 1, 8, 1, 1, 1, binary, t, INT64_MAX, 0,
                                    ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(counts.ctypes.data)))
        return out.tolist(), counts.tolist()

    for binary in (0, 1):                               # EDT_BOOL: any non-zero byte is foreground, always binary; bytes are kept
        assert call(BOOL, binary, 2) == ([1, 2, 0, 0, 0, 7, 7, 9], [3, 2, 1])
    assert call(U8, 1, 2) == ([1, 2, 0, 0, 0, 7, 7, 9], [3, 2, 1])
    assert call(U8, 0, 2) == ([0, 0, 0, 0, 0, 7, 7, 0], [5, 1, 4])       # the same bytes as uint8 labels: values decide


# ---- entry points ----------------------------------------------------------------------------------------------------
def test_in_place(edt_gpu):
    import torch
    from edt import _lib
    lib = _lib.load()
    lab = oracle.sparse_volume(1, 0.45)
    for threshold, c, binary in ((4, 1, False), ((3, 9), 3, False), (4, 2, True)):
        want = oracle.dust(lab, threshold, c, binary=binary)
        a, ca = on_device(lab, threshold, c, binary, False)
        b, cb = on_device(lab, threshold, c, binary, False, in_place=True)
        assert ca == cb == want[1:] and same_bytes(np.asarray(a, order="A"), want.out) and same_bytes(np.asarray(b, order="A"), want.out)
    # the ABI with d_out == d_labels
    want = oracle.dust(lab, 4, 2)
    t, _ = to_device(lab)
    ext = tuple(int(e) for e in t.shape[::-1])
    ws = torch.empty(lib.edt_hip_dust_workspace_bytes(U32, 3, *ext), dtype=torch.uint8, device="cuda")
    counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    vp = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    _lib.check(lib.edt_hip_dust_device(vp(t), U32, 3, *ext, 2, 0, 4, INT64_MAX, 0, vp(t), vp(counts), vp(ws), ws.numel(),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert tuple(counts.tolist()) == want[1:] and same_bytes(t.cpu().numpy().view(np.uint32).T, want.out)
    # the host form in place
    buf = lab.copy(order="F")
    out = np.zeros(3, dtype=np.int64)
    p = ctypes.c_void_p(buf.ctypes.data)
    _lib.check(lib.edt_hip_dust(p, U32, 3, 70, 12, 9, 2, 0, 4, INT64_MAX, 0, p, ctypes.c_void_p(out.ctypes.data)))
    assert tuple(out.tolist()) == want[1:] and same_bytes(buf, want.out)
    with pytest.raises(ValueError):
        from edt import device
        device.dust(torch.zeros((4, 6), dtype=torch.int32, device="cuda").t(), 2, in_place=True)


def test_determinism_and_dirty_scratch(edt_gpu):
    """The same call twice gives the same bytes and counts -- also through the ABI on a reused workspace and output full of other
    bits -- the phases are named in the pass log, and the workspace is fill_holes' and no more."""
    import torch
    from edt import _lib, device
    lib = _lib.load()
    lab = oracle.sparse_volume(3, 0.45)
    want = oracle.dust(lab, (3, 9), 2)
    a, ca = edt_gpu.dust(lab, (3, 9), connectivity=2, return_counts=True)
    b, cb = edt_gpu.dust(lab, (3, 9), connectivity=2, return_counts=True)
    assert tuple(ca) == tuple(cb) == want[1:] and same_bytes(a, b) and same_bytes(a, want.out)
    t, _ = to_device(lab)
    ext = tuple(int(e) for e in t.shape[::-1])
    nbytes = lib.edt_hip_dust_workspace_bytes(U32, 3, *ext)
    assert nbytes == lib.edt_hip_fill_holes_workspace_bytes(U32, 3, *ext)
    for code, shape in ((U8, (512, 512, 512)), (F64, (70, 40, 30)), (U16, (1025, 5, 3))):
        assert lib.edt_hip_dust_workspace_bytes(code, 3, *shape) == lib.edt_hip_fill_holes_workspace_bytes(code, 3, *shape) > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    vp = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    first = None
    for fill in (0xFF, 0x00, 0x5A, 0x80):
        ws.fill_(fill)
        out = torch.full(t.shape, -7, dtype=torch.int32, device="cuda")
        counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        for _ in range(2):
            _lib.check(lib.edt_hip_dust_device(vp(t), U32, 3, *ext, 2, 0, 3, 9, 0, vp(out), vp(counts), vp(ws), ws.numel(),
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            assert tuple(counts.tolist()) == want[1:]
            first = out.clone() if first is None else first
            assert torch.equal(out, first)
    assert same_bytes(first.cpu().numpy().view(np.uint32).T, want.out)
    device.set_profiling(True)
    try:
        device.dust(t, 4, connectivity=2)
        torch.cuda.synchronize()
        names = [name for name, _ in device.pass_times()]
        device.dust(t, (3, 9), connectivity=1, binary=True, invert=True)
        torch.cuda.synchronize()
        binary_names = [name for name, _ in device.pass_times()]
    finally:
        device.set_profiling(False)
    assert names == binary_names == ["dust " + p for p in ("rows", "merge", "flatten", "count", "filter")]
    # empty input
    e, counts = device.dust(torch.zeros((0, 4), dtype=torch.int32, device="cuda"), 4)
    assert e.shape == (0, 4) and counts.tolist() == [0, 0, 0]
    counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    _lib.check(lib.edt_hip_dust_device(None, U32, 3, 4, 0, 2, 1, 0, 4, INT64_MAX, 0, None, vp(counts), None, 0, None))
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0, 0]
    out, counts = edt_gpu.dust(np.zeros((3, 0, 2), dtype=np.float64), 4, return_counts=True)
    assert out.shape == (3, 0, 2) and counts == (0, 0, 0)


# ---- composition -----------------------------------------------------------------------------------------------------
def test_composes_with_fill_holes_and_the_transform_on_the_device(edt_gpu):
    import torch
    import fill_holes_oracle
    from edt import device
    from synth import blob_mask
    rng = np.random.default_rng(8)
    lab = blob_mask((48, 40, 36), rng=rng, p=0.6, block=6).astype(np.uint8)
    lab[rng.random(lab.shape) < 0.01] = 0               # pin-holes inside the blobs
    lab[(lab == 0) & (rng.random(lab.shape) < 0.02)] = 2   # specks outside them
    lab = np.ascontiguousarray(lab)
    dusted = oracle.dust(lab, 4, 3)
    assert dusted.removed_voxels > 50 and dusted.kept >= 1
    want = fill_holes_oracle.fill_holes(dusted.out, 1)
    assert want.n_filled > 50
    x = torch.from_numpy(lab).cuda()
    d, counts = device.dust(x, 4)
    dt = device.edt(device.fill_holes(d)[0])
    assert tuple(counts.tolist()) == dusted[1:]
    ref = edt_gpu.edt(want.out)
    assert np.array_equal(dt.cpu().numpy(), ref)
    assert not np.array_equal(ref, edt_gpu.edt(lab))    # the specks and the holes did pin the field
    # the composition this call replaces: connected_components + bincount + a gather + a where
    comp, n = device.connected_components(x)
    size = torch.bincount(comp.reshape(-1).long(), minlength=int(n) + 1)
    composed = torch.where(size[comp.long()] >= 4, x, torch.zeros_like(x))
    assert torch.equal(composed, d) and int(n) == dusted.components
