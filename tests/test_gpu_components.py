"""GPU tier of connected_components (csrc/edt_components.hip): every comparison is exact equality of the whole array and of N
against the numpy restatement of the contract (tests/components_oracle.py).  Shapes are the smallest at which the named
thing can go wrong: the kernels take 64-voxel groups in 256-voxel steps, cut x-runs at every 256th voxel of the flattened
volume, number in chunks of 2048 voxels and scan 1024 chunks per round."""
import ctypes
import itertools

import numpy as np
import pytest

import components_oracle as oracle
from synth import blob_mask, blocky_labels, voronoi_labels

pytestmark = pytest.mark.gpu

U8, U16, U32, U64, F32, F64, BOOL = range(7)


def check(edt, data, c=None, binary=False, n=None):
    got, gn = edt.connected_components(data, connectivity=c, binary=binary, return_N=True)
    want, wn = oracle.connected_components(data, c, binary=binary, return_N=True)
    assert got.dtype == np.uint32 and got.shape == data.shape
    assert got.flags.f_contiguous == want.flags.f_contiguous and got.flags.c_contiguous == want.flags.c_contiguous
    assert gn == wn, (gn, wn)
    assert np.array_equal(got, want)
    if n is not None:
        assert gn == n, (gn, n)
    return got, gn


def fvol(shape, dtype=np.uint8):
    return np.zeros(shape, dtype=dtype, order="F")   # axis 0 is x


# ---- run and wave boundaries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sx", [1, 63, 64, 65, 130, 1025])
def test_run_and_wave_boundaries(edt_gpu, sx):
    rng = np.random.default_rng(sx)
    lab = fvol((sx, 5, 3))
    for z, y in itertools.product(range(3), range(5)):
        x = 0
        while x < sx:                                   # random runs of 0 / 1 / 2, 1 to 90 voxels long
            run = int(rng.integers(1, 91))
            lab[x:x + run, y, z] = rng.integers(0, 3)
            x += run
        for b in range(64, sx, 64):                     # ... and one that crosses every 64-voxel boundary of the row
            if rng.random() < 0.7:
                lab[max(0, b - int(rng.integers(1, 40))):b + int(rng.integers(1, 40)), y, z] = rng.integers(1, 3)
    for c in (1, 2, 3):
        check(edt_gpu, lab, c)
        check(edt_gpu, lab, c, binary=True)
    # the flattened volume's 64- and 256-voxel boundaries fall anywhere inside the rows: one label throughout
    lab[:] = 1
    check(edt_gpu, lab, 1, n=1)


# ---- connectivity really differs -----------------------------------------------------------------------------------
def test_checkerboard(edt_gpu):
    x, y, z = np.meshgrid(np.arange(9), np.arange(7), np.arange(5), indexing="ij")
    lab = np.asfortranarray(((x + y + z) % 2 == 0).astype(np.uint16) * 7)
    check(edt_gpu, lab, 1, n=int(np.count_nonzero(lab)))
    check(edt_gpu, lab, 2, n=1)
    check(edt_gpu, lab, 3, n=1)
    check(edt_gpu, np.ascontiguousarray(lab), 1, n=int(np.count_nonzero(lab)))


def _pair(shape, p, off, dtype=np.uint8):
    lab = fvol(shape, dtype)
    lab[p] = 3
    lab[tuple(a + b for a, b in zip(p, off))] = 3
    return lab


def test_corner_edge_and_face_pairs(edt_gpu):
    p = (2, 2, 2)
    for off in itertools.product((-1, 0, 1), repeat=3):
        axes = sum(map(abs, off))
        if axes == 0:
            continue
        lab = _pair((5, 5, 5), p, off)
        for c in (1, 2, 3):
            check(edt_gpu, lab, c, n=1 if axes <= c else 2)     # corner only: 2, 2, 1; edge only: 2, 1, 1; face: 1, 1, 1
    # at the volume's borders: y = 0, y = sy - 1, z = 0 and x = 0, x = sx - 1 of the rows that are read
    for p, off in (((0, 0, 0), (1, 1, 1)), ((3, 0, 1), (-1, 1, -1)), ((0, 2, 1), (1, -1, -1)), ((3, 2, 0), (-1, -1, 1)),
                   ((1, 2, 1), (0, -1, -1)), ((1, 1, 1), (0, 1, -1)), ((3, 1, 1), (-1, 1, -1)), ((0, 1, 1), (1, 1, -1))):
        lab = _pair((4, 3, 2), p, off)
        axes = sum(map(abs, off))
        for c in (1, 2, 3):
            check(edt_gpu, lab, c, n=1 if axes <= c else 2)


def test_the_plus_one_minus_one_row(edt_gpu):
    """(y + 1, z - 1): the one preceding row that lies AHEAD in y."""
    for dx in (-1, 0, 1):
        lab = _pair((70, 4, 3), (64, 1, 2), (dx, 1, -1))        # (x across a 64-voxel boundary)
        want = {0: (2, 1, 1), 1: (2, 2, 1), -1: (2, 2, 1)}[dx]
        for c in (1, 2, 3):
            check(edt_gpu, lab, c, n=want[c - 1])


def test_anti_diagonal_pair_2d(edt_gpu):
    for x in (0, 5, 63, 64):
        lab = fvol((66, 3))
        lab[x + 1, 0] = lab[x, 1] = 1                           # (x + 1, y - 1)
        check(edt_gpu, lab, 1, n=2)
        check(edt_gpu, lab, 2, n=1)
        lab = fvol((66, 3))
        lab[x, 0] = lab[x + 1, 1] = 1                           # (x - 1, y - 1)
        check(edt_gpu, lab, 1, n=2)
        check(edt_gpu, lab, 2, n=1)


# ---- labels decide -------------------------------------------------------------------------------------------------
def test_labels_decide(edt_gpu):
    lab = fvol((8, 4, 2), np.uint32)
    lab[0:4, :, :] = 5
    lab[4:8, :, :] = 6                                          # side by side: never merge
    for c in (1, 2, 3):
        got, _ = check(edt_gpu, lab, c, n=2)
        assert got[0, 0, 0] == 1 and got[4, 0, 0] == 2
        check(edt_gpu, lab, c, binary=True, n=1)
    lab = fvol((9, 3), np.uint32)
    lab[0:3, :] = 5
    lab[3:6, :] = 9
    lab[6:9, :] = 5                                             # the same value in two places: two numbers
    got, _ = check(edt_gpu, lab, 2, n=3)
    assert got[0, 0] == 1 and got[3, 0] == 2 and got[6, 0] == 3
    check(edt_gpu, lab, 2, binary=True, n=1)
    lab[3:6, :] = 0
    check(edt_gpu, lab, 2, n=2)
    check(edt_gpu, lab, 2, binary=True, n=2)


# ---- long chains ---------------------------------------------------------------------------------------------------
def serpentine(sx, sy):
    img = fvol((sx, sy))
    img[:, 0::2] = 4
    for k, y in enumerate(range(1, sy, 2)):
        img[sx - 1 if k % 2 == 0 else 0, y] = 4
    return img


def test_long_chains(edt_gpu):
    img = serpentine(65, 67)
    for c in (1, 2):
        check(edt_gpu, img, c, n=1)
    # a 3-D spiral: a serpentine in every other slice, one voxel between two slices where the serpentine below ends
    vol = fvol((33, 17, 9))
    s = serpentine(33, 17)
    ends = [(0, 0), (32 if (17 // 2) % 2 == 1 else 0, 16)]      # where the serpentine starts / ends (sy odd: last row is full)
    for k, z in enumerate(range(0, 9, 2)):
        vol[:, :, z] = s
        if z + 1 < 9:
            vol[ends[(k + 1) % 2] + (z + 1,)] = 4
    for c in (1, 2, 3):
        check(edt_gpu, vol, c, n=1)
    comb = fvol((131, 40))
    comb[0::2, :] = 2                                           # teeth along y ...
    comb[:, 39] = 2                                             # ... that join only in the last row
    for c in (1, 2):
        check(edt_gpu, comb, c, n=1)
    comb[:, 39] = 0
    check(edt_gpu, comb, 2, n=66)


# ---- many components -----------------------------------------------------------------------------------------------
def test_many_components(edt_gpu):
    """Every other voxel at connectivity 1: every set voxel is a root.  The numbering counts roots per chunk of 2048 voxels
    and scans 1024 chunks per round of its single-workgroup loop: 130 * 96 * 170 = 2 121 600 voxels are 1036 chunks, two
    rounds, the second one partial; and 130 is no multiple of anything."""
    shape = (130, 96, 170)
    assert 1024 < -(-np.prod(shape) // 2048) < 2048
    x, y, z = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij", sparse=True)
    lab = np.asfortranarray(((x + y + z) % 2 == 0).astype(np.uint8))
    got, n = edt_gpu.connected_components(lab, connectivity=1, return_N=True)
    flat = lab.reshape(-1, order="F").astype(np.int64)
    want = (np.cumsum(flat) * flat).astype(np.uint32).reshape(shape, order="F")
    assert n == int(flat.sum()) and np.array_equal(got, want)
    wo, wn = oracle.connected_components(lab, 1, return_N=True)
    assert wn == n and np.array_equal(wo, want)


# ---- every dtype ---------------------------------------------------------------------------------------------------
BLOCKY = np.asfortranarray(blocky_labels((70, 33, 20), nlabels=5, zero_frac=0.25, block=3, rng=np.random.default_rng(42)))


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64,
                                   np.float32, np.float64, bool])
def test_every_dtype(edt_gpu, dtype):
    dt = np.dtype(dtype)
    if dt == np.bool_:
        lab = BLOCKY != 0
    else:
        lab = BLOCKY.astype(dt)
        if dt.kind == "i":
            lab[BLOCKY == 3] = -3
        if dt.kind == "f":
            lab[BLOCKY == 3] = -2.5
            lab[BLOCKY == 4] = np.inf
    lab = np.asfortranarray(lab)
    for c in (1, 3):
        check(edt_gpu, lab, c)
    check(edt_gpu, lab, 2, binary=True)


def test_label_values(edt_gpu):
    one = np.uint64(1)
    lab = np.array([1, 1 + (one << np.uint64(32)), 1 + (one << np.uint64(32)), one << np.uint64(63), 0, 1], dtype=np.uint64)
    got, _ = check(edt_gpu, lab, 1, n=4)                         # differ only above bit 32: no merge
    assert got.tolist() == [1, 2, 2, 3, 0, 4]
    for dt in (np.float32, np.float64):
        nan = np.array(np.nan, dtype=dt)
        lab = np.asfortranarray(np.array([[1.0, -0.0, 1.0, nan, nan, 1.0], [-0.0, -0.0, 0.0, nan, 2.0, 2.0]], dtype=dt).T)
        got, _ = check(edt_gpu, lab, 2, n=7)                     # -0.0 is background, every NaN voxel a singleton
        assert got[1, 0] == 0 and got[0, 1] == 0 and len({int(got[3, 0]), int(got[4, 0]), int(got[3, 1])}) == 3
        got, _ = check(edt_gpu, lab, 2, binary=True, n=2)        # under binary NaN joins its neighbours
        assert got[3, 0] == got[5, 0] == got[4, 1]


def test_bool_bytes_join_through_the_abi(edt_gpu):
    from edt import _lib
    lib = _lib.load()
    lab = np.array([1, 2, 0, 2, 255, 1, 0, 7], dtype=np.uint8)
    for binary in (0, 1):
        out, n = np.zeros(8, dtype=np.uint32), ctypes.c_int64(-1)
        _lib.check(lib.edt_hip_connected_components(ctypes.c_void_p(lab.ctypes.data), BOOL, 1, 8, 1, 1, 1, binary,
                                                    ctypes.c_void_p(out.ctypes.data), ctypes.byref(n)))
        assert out.tolist() == [1, 1, 0, 2, 2, 2, 0, 3] and n.value == 3
    out, n = np.zeros(8, dtype=np.uint32), ctypes.c_int64(-1)     # the same bytes as uint8 labels: values decide
    _lib.check(lib.edt_hip_connected_components(ctypes.c_void_p(lab.ctypes.data), U8, 1, 8, 1, 1, 1, 0,
                                                ctypes.c_void_p(out.ctypes.data), ctypes.byref(n)))
    assert out.tolist() == [1, 2, 0, 3, 4, 5, 0, 6] and n.value == 6


# ---- order ---------------------------------------------------------------------------------------------------------
def test_memory_order_decides_the_numbering(edt_gpu):
    rng = np.random.default_rng(3)
    lab = blocky_labels((23, 14, 9), nlabels=3, zero_frac=0.4, block=2, rng=rng).astype(np.uint16)
    for c in (1, 2, 3):
        gc, nc = check(edt_gpu, np.ascontiguousarray(lab), c)
        gf, nf = check(edt_gpu, np.asfortranarray(lab), c)
        assert nc == nf and not np.array_equal(gc, gf)
        pairs = np.unique(np.stack([gc.ravel(), np.ascontiguousarray(gf).ravel()]), axis=1)
        assert pairs.shape[1] == nc + 1                          # the same partition (+ background)
    line = blocky_labels((300,), nlabels=3, zero_frac=0.3, block=5, rng=rng).astype(np.uint8)
    check(edt_gpu, line, 1)
    check(edt_gpu, line, None, binary=True)
    img = blocky_labels((37, 70), nlabels=3, zero_frac=0.3, block=3, rng=rng).astype(np.float32)
    for given, c in ((1, 1), (2, 2), (4, 1), (8, 2), (None, 2)):   # skimage's and cc3d's spelling
        for data in (img, np.asfortranarray(img)):
            got = edt_gpu.connected_components(data, connectivity=given)
            assert np.array_equal(got, oracle.connected_components(data, c))
    for shape in ((1, 40, 1), (40, 1, 1), (1, 1, 40), (1, 9)):    # both C- and F-contiguous
        unit = blocky_labels(shape, nlabels=2, zero_frac=0.3, block=3, rng=rng).astype(np.uint32)
        assert unit.flags.c_contiguous and unit.flags.f_contiguous
        for c in range(1, unit.ndim + 1):
            check(edt_gpu, unit, c)


# ---- degenerate ----------------------------------------------------------------------------------------------------
def test_degenerate(edt_gpu):
    got, _ = check(edt_gpu, fvol((70, 9, 4), np.uint32), None, n=0)
    assert not got.any()
    ones = np.ones((300, 200, 8), dtype=np.uint32, order="F")
    for c in (1, 3):
        got, n = edt_gpu.connected_components(ones, connectivity=c, return_N=True)
        assert n == 1 and got.dtype == np.uint32 and np.array_equal(got, ones)
    for shape in ((1,), (1, 1), (1, 1, 1)):
        check(edt_gpu, np.full(shape, 9, dtype=np.int64), None, n=1)
        check(edt_gpu, np.zeros(shape, dtype=np.int64), None, n=0)
    for shape in ((0,), (4, 0), (0, 3, 2)):
        out, n = edt_gpu.connected_components(np.zeros(shape, dtype=np.uint8), return_N=True)
        assert out.shape == shape and out.dtype == np.uint32 and n == 0


# ---- entry points --------------------------------------------------------------------------------------------------
def _raw_device_call(lib, t, c, binary, out, n, ws, stream=None):
    import torch
    from edt import _lib, device
    ext = tuple(int(e) for e in t.shape[::-1]) + (1,) * (3 - t.dim())
    vp = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    _lib.check(lib.edt_hip_connected_components_device(vp(t), device.dtype_code(t.dtype), t.dim(), *ext, c, binary, vp(out), vp(n),
                                                       vp(ws), ws.numel(), s))


def test_entry_points_agree(edt_gpu):
    import torch
    from edt import _lib, device
    lib = _lib.load()
    lab = voronoi_labels((72, 60, 44), nseeds=30, seed=4, upsample=4, membrane=0.04)   # 93 chunks of the numbering
    lab = np.asfortranarray(((1 + lab % 4) * (lab != 0)).astype(np.uint32))
    t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).cuda()      # z, y, x: the same memory
    nbytes = lib.edt_hip_components_workspace_bytes(U32, 3, *lab.shape)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for c, binary in ((1, False), (2, False), (3, False), (3, True)):
        want, wn = check(edt_gpu, lab, c, binary)
        out, n = device.connected_components(t, connectivity=c, binary=binary)
        assert out.dtype == torch.int32 and out.shape == t.shape and n.dtype == torch.int64 and n.dim() == 0 and n.is_cuda
        assert int(n) == wn and np.array_equal(out.cpu().numpy().view(np.uint32).T, want)
        for fill in (0xFF, 0x00, 0x5A):                          # a reused, dirty workspace and dirty outputs; repeated calls
            ws.fill_(fill)
            raw = torch.full(t.shape, -7, dtype=torch.int32, device="cuda")
            rn = torch.full((), -1, dtype=torch.int64, device="cuda")
            _raw_device_call(lib, t, c, int(binary), raw, rn, ws)
            assert int(rn) == wn and torch.equal(raw, out)
            _raw_device_call(lib, t, c, int(binary), raw, rn, ws)
            assert int(rn) == wn and torch.equal(raw, out)
    device.set_profiling(True)
    try:
        device.connected_components(t, connectivity=2)
        torch.cuda.synchronize()
        names = [name for name, _ in device.pass_times()]
    finally:
        device.set_profiling(False)
    assert names == ["components rows", "components merge", "components flatten", "components number", "components final"]


def test_device_form_is_graph_capturable(edt_gpu):
    """edt_hip_connected_components_device only enqueues kernels on the caller's stream (no allocation, no synchronisation):
    the whole labelling can be captured into a hipGraph and replayed."""
    import torch
    from edt import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    lab = voronoi_labels((96, 80, 72), nseeds=40, seed=4, upsample=4, membrane=0.04)
    lab = np.asfortranarray(((1 + lab % 3) * (lab != 0)).astype(np.uint32))
    t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).to(dev)
    out = torch.empty(t.shape, dtype=torch.int32, device=dev)
    n = torch.zeros((), dtype=torch.int64, device=dev)
    ws = torch.empty(lib.edt_hip_components_workspace_bytes(U32, 3, *lab.shape), dtype=torch.uint8, device=dev)
    _raw_device_call(lib, t, 3, 0, out, n, ws)                   # warm-up: lazy code-object loads
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _raw_device_call(lib, t, 3, 0, out, n, ws)
    want, wn = oracle.connected_components(lab, 3, return_N=True)
    for _ in range(3):
        out.zero_()
        n.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert int(n) == wn and np.array_equal(out.cpu().numpy().view(np.uint32).T, want)


# ---- composition ---------------------------------------------------------------------------------------------------
def test_composes_with_label_stats_on_the_device(edt_gpu):
    import torch
    from edt import device
    mask = blob_mask((96, 80, 72), rng=np.random.default_rng(8), p=0.45, block=6)
    t = torch.from_numpy(mask).cuda()
    comps, n = device.connected_components(t, connectivity=1)
    dt = device.edt(comps)
    stats = device.label_stats(comps, dt)
    n = int(n)
    assert n > 1 and len(stats.labels) == n and stats.labels.cpu().tolist() == list(range(1, n + 1))
    assert int(stats.counts.sum()) == int(np.count_nonzero(mask))
    assert bool(((stats.bbox_lo <= stats.argmax) & (stats.argmax <= stats.bbox_hi)).all())
    want, wn = oracle.connected_components(mask, 1, return_N=True)
    assert wn == n and np.array_equal(comps.cpu().numpy().view(np.uint32), want)
    assert sum(1 for _ in device.each(comps, dt)) == n


# ---- a mid-size property check -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def classes():
    lab = voronoi_labels((256, 256, 128), nseeds=300, seed=9, upsample=4, membrane=0.04)
    return np.asfortranarray(np.where(lab != 0, 1 + lab % 5, 0).astype(np.uint32))


@pytest.mark.parametrize("c", [1, 2, 3])
def test_mid_size_properties(edt_gpu, classes, c):
    ndi = pytest.importorskip("scipy.ndimage")                   # (tests/synth.py builds this volume with scipy already)
    lab = classes
    out, n = edt_gpu.connected_components(lab, connectivity=c, return_N=True)
    assert np.array_equal(out == 0, lab == 0)
    # every pair of neighbouring equal non-zero labels has equal numbers
    for off in oracle.offsets(3, c):
        a = tuple(slice(max(0, -o), s - max(0, o)) for o, s in zip(off, lab.shape))
        b = tuple(slice(max(0, o), s - max(0, -o)) for o, s in zip(off, lab.shape))
        conn = (lab[a] == lab[b]) & (lab[a] != 0)
        assert np.array_equal(out[a][conn], out[b][conn]), off
    # the numbers are 1..N in ascending order of first index (memory order), and every component holds one label value
    flat, lflat = out.reshape(-1, order="F"), lab.reshape(-1, order="F")
    ids, first = np.unique(flat, return_index=True)
    assert ids.tolist() == list(range(0 if (lab == 0).any() else 1, n + 1))
    fg = ids > 0
    assert np.all(np.diff(first[fg]) > 0)
    assert np.array_equal(lflat[first[fg]][flat[flat > 0] - 1], lflat[flat > 0])
    # N: scipy's count, label value by label value (with the equal-numbers property above, out is then exactly the partition)
    st = ndi.generate_binary_structure(3, c)
    assert n == sum(ndi.label(lab == v, structure=st)[1] for v in range(1, 6))
