"""GPU tier: labels across each dtype's full value range on every kernel path.

The rest of the suite only hands the kernels small whole numbers.  Here every volume holds values from
synth.palette_labels: neighbouring blocks are equal once narrowed (the low half of a wide integer, float64 -> float32,
a float32 denormal flushed to zero) and different at full width, NaNs compare unequal to themselves and -0.0 is
background.  Every case is compared bit for bit with the CPU oracle (tests/test_oracle.py pins it to the compiled
reference on these values, and checks that the palettes do tell a narrowed comparison from the right one)."""
import sys
import time

import numpy as np
import pytest

from synth import palette, palette_labels

pytestmark = pytest.mark.gpu

DTYPES = [np.uint64, np.int64, np.uint32, np.int32, np.uint16, np.int16, np.int8, np.float64, np.float32, bool]
WIDE = [np.uint64, np.int64, np.float64, np.float32, np.uint32, np.int16]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def explain(got, want):
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if len(bad) == 0:
        return "shape/dtype mismatch"
    i = tuple(bad[0])
    return f"{len(bad)} mismatches; first at {i}: got {got[i]!r} want {want[i]!r}"


def check(edt_gpu, oracle_port, lab, an, bb, what):
    want = oracle_port.edtsq(lab, an, bb)
    got = edt_gpu.edtsq(lab, anisotropy=an, black_border=bb)
    assert same(got, want), (what, lab.dtype, lab.shape, an, bb, explain(got, want))
    got = edt_gpu.edt(lab, anisotropy=an, black_border=bb)
    assert same(got, np.sqrt(want)), (what, "sqrt", lab.dtype, lab.shape, an, bb, explain(got, np.sqrt(want)))


@pytest.fixture
def debug_mode():
    from edt import _lib
    lib = _lib.load()
    try:
        yield lib.edt_hip_set_debug_mode
    finally:
        lib.edt_hip_set_debug_mode(0)


@pytest.fixture(scope="module", autouse=True)
def module_duration(request):
    """The module reports its own wall time: 16 s within the GPU tier and 27 s alone on an MI355X, the 2048 x 2048 x 33
    slab case and its oracle run included (the budget is about 60 s).  Written past pytest's output capture, so a plain
    run shows it."""
    t0 = time.perf_counter()
    yield
    line = f"\ntests/test_gpu_label_values.py: {time.perf_counter() - t0:.1f} s\n"
    capman = request.config.pluginmanager.getplugin("capturemanager")
    if capman is None:
        print(line)
        return
    with capman.global_and_fixture_disabled():
        sys.stdout.write(line)
        sys.stdout.flush()


# ---- pass X kernel families and the size-agnostic fallback --------------------------------------------------------
@pytest.mark.parametrize("mode,name", [(0, "default"), (64, "phased-column"), (32, "lds-row"),
                                        (96, "phased-both"), (0x100000, "fp32-pass-1")])
def test_kernel_families(edt_gpu, oracle_port, debug_mode, mode, name):
    rng = np.random.default_rng(1000 + mode)
    debug_mode(mode)
    for i, dt in enumerate(DTYPES):
        shape = [(72, 40, 36), (130, 33, 20), (40, 70, 9)][i % 3]
        lab = palette_labels(shape, dt, rng=rng, block=int(rng.integers(2, 7)), order="CF"[i % 2])
        for an, bb in (((1, 1, 1), False), ((6, 6, 30), True)):
            check(edt_gpu, oracle_port, lab, an, bb, name)
    img = palette_labels((300, 200), np.uint64, rng=rng, block=5)
    check(edt_gpu, oracle_port, img, (2, 3), False, name + " 2-D")


def test_generic_path(edt_gpu, oracle_port, monkeypatch):
    monkeypatch.setenv("EDT_HIP_FORCE_GENERIC", "1")
    rng = np.random.default_rng(1100)
    for i, dt in enumerate(DTYPES):
        for dims in (1, 2, 3):
            shape = tuple(int(rng.integers(5, 60)) for _ in range(dims))
            lab = palette_labels(shape, dt, rng=rng, block=int(rng.integers(1, 5)), order="CF"[(i + dims) % 2])
            an = ((1.0, 1.0, 1.0), (0.5, 0.7, 1.3))[(i + dims) % 2][:dims]
            check(edt_gpu, oracle_port, lab, an[0] if dims == 1 else an, bool(dims % 2), "generic")


# ---- the other shapes of pass X and of the column passes -----------------------------------------------------------
@pytest.mark.parametrize("shape", [(1025, 5, 3), (2049, 3, 3), (4096, 2, 2), (3000, 7),   # 2- and 4-wave rows
                                   (300, 200, 8), (90, 31, 33), (257, 17),                # axes of <= 32 rows
                                   (40, 36, 1100), (17, 2049, 3), (33, 5, 2100),          # beyond the wave kernels
                                   (1500,), (5000,)])                                     # 1-D lines
def test_other_shapes(edt_gpu, oracle_port, shape):
    rng = np.random.default_rng(sum(shape))
    for i, dt in enumerate(WIDE):
        lab = palette_labels(shape, dt, rng=rng, block=int(rng.integers(1, 6)), order="FC"[i % 2])
        for an, bb in (((1.0, 1.0, 1.0), False), ((6.0, 6.0, 30.0), True)):
            an = an[:len(shape)]
            check(edt_gpu, oracle_port, lab, an[0] if len(shape) == 1 else an, bb, "shape")


def test_stack_of_images(edt_gpu, oracle_port):
    rng = np.random.default_rng(1200)
    for dt in WIDE:
        stack = palette_labels((7, 45, 130), dt, rng=rng, block=3)
        for bb in (False, True):
            want = np.stack([oracle_port.edtsq(im, (2.0, 3.0), bb) for im in stack])
            got = edt_gpu.edtsq_stack(stack, anisotropy=(2.0, 3.0), black_border=bb)
            assert same(got, want), (dt, bb, explain(got, want))


# ---- the 16-bit integer column kernel: integer voxel sizes, its refused tiles and the fp32 hand-over ---------------------
Q16_MODES = [0, 0x10000000, 0x8000000, 0x40000000, 0x20000000]


def test_integer_column_path(edt_gpu, oracle_port, debug_mode):
    rng = np.random.default_rng(1300)
    for i, dt in enumerate(WIDE):
        # both column axes of at least four 32-row bands; large blocks leave rows without a boundary (refused tiles
        # under black_border=False)
        lab = palette_labels((64, 160, 136), dt, rng=rng, block=[5, 40][i % 2], zero_frac=0.05, order="F")
        for an, bb in (((1, 1, 1), False), ((2, 1, 3), True), ((6, 6, 30), False)):
            want = oracle_port.edtsq(lab, an, bb)
            for mode in Q16_MODES:
                debug_mode(mode)
                got = edt_gpu.edtsq(lab, anisotropy=an, black_border=bb)
                assert same(got, want), (dt, an, bb, hex(mode), explain(got, want))


# ---- the halo slice between the index slabs of a volume of more than 2^27 voxels --------------------------------------------
def test_slab_boundary_of_the_index_form(edt_gpu, oracle_port):
    """2048 x 2048 x 33 uint16: two index slabs (32 slices of 4 Mi voxels, then one).  0x0001 below the boundary and
    0x0101 above it in one quarter of the plane: only a full-width comparison of the halo slice sees the boundary there."""
    sx = sy = 2048
    lab = np.full((sx, sy, 33), 0x0001, dtype=np.uint16, order="F")
    lab[:sx // 2, :sy // 2, 32:] = 0x0101
    lab[sx // 2:, sy // 2:, 32:] = 0x0100
    lab[::97, ::89, 5] = 0
    want = oracle_port.edtsq(lab, (1.0, 1.0, 1.0), False)
    got = edt_gpu.edtsq(lab, anisotropy=(1.0, 1.0, 1.0), black_border=False)
    assert same(got, want), explain(got, want)
    assert want[0, 0, 32] == 1.0 and want[-1, -1, 32] == 1.0


# ---- virtual devices, the shard phases as virtual ranks, 16-bit records ---------------------------------------------------
def _pair_across_z(dt, shape, zcut, rng):
    lab = palette_labels(shape, dt, rng=rng, block=8, order="F")
    pal = palette(dt)   # pal[0] / pal[1]: 1 / 1+2^32, 1 / 0x101, 1.0 / 1+2^-52 ...: equal once narrowed
    lab[:, : shape[1] // 2, :zcut] = pal[0]
    lab[:, : shape[1] // 2, zcut:] = pal[1]
    return lab


def test_virtual_devices(edt_gpu, oracle_port):
    rng = np.random.default_rng(1400)
    for dt in (np.uint64, np.float64, np.float32, np.int16):
        lab = _pair_across_z(dt, (160, 144, 96), 32, rng)   # three ranks: z = 0..31, 32..63, 64..95
        want = oracle_port.edtsq(lab, (1.0, 1.0, 2.0), False)
        edt_gpu.set_devices([0, 0, 0])
        try:
            got = edt_gpu.edtsq(lab, anisotropy=(1.0, 1.0, 2.0))
        finally:
            edt_gpu.set_devices(None)
        assert same(got, want), (dt, explain(got, want))


def _as_tensor(lab, dev):
    import torch
    a = np.ascontiguousarray(lab.T)  # (sz, sy, sx), x fastest
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(dev)


def test_shard_phases_as_virtual_ranks(edt_gpu, oracle_port):
    import torch
    from edt import _lib
    from edt.distributed import HipOps, balanced_partition
    from virtual_ranks import flag_phases, record_phases
    dev = torch.device("cuda", 0)
    ops = HipOps()
    rng = np.random.default_rng(1500)
    world = 2
    for dt in (np.uint64, np.float64, np.float32):
        code = {np.uint64: _lib.U64, np.float64: _lib.F64, np.float32: _lib.F32}[dt]
        shape = (96, 80, 72)
        lab = _pair_across_z(dt, shape, 36, rng)
        t = _as_tensor(lab, dev)
        assert balanced_partition(shape[2], world)[1][0] == 36
        for an, bb in (((6.0, 6.0, 30.0), True), ((1.0, 1.5, 0.5), False)):
            got = flag_phases(ops, t, code, world, an, _lib.FLAG_BLACK_BORDER if bb else 0).cpu().numpy().T
            want = oracle_port.edtsq(lab, an, bb)
            assert same(got, want), (dt, an, bb, explain(got, want))

        # 16-bit slab records
        shape = (96, 280, 100)
        sx, sy, sz = shape
        lab = _pair_across_z(dt, shape, 50, rng)
        t = _as_tensor(lab, dev)
        assert balanced_partition(sz, world)[1][0] == 50
        for an, bb in (((1.0, 1.0, 1.0), True), ((2.0, 1.0, 3.0), True)):
            assert ops.records16_supported(code, sx, sy, sz, an)
            got, refused = record_phases(ops, t, code, world, 1, an, _lib.FLAG_BLACK_BORDER if bb else 0, rows16=True, fill=-1)
            assert refused == 0   # (the rows of a refused tile are unspecified: nothing to compare)
            got = got.cpu().numpy().T
            want = oracle_port.edtsq(lab, an, bb)
            assert same(got, want), (dt, "records16", an, bb, explain(got, want))


# ---- sdf / sdfsq: the fused sign epilogue and the sign as a pass of its own (debug bit 0x400) ------------------------------
@pytest.mark.parametrize("mode", [0, 0x400])
def test_sdf(edt_gpu, oracle_port, debug_mode, mode):
    import torch
    from edt import device
    debug_mode(mode)
    rng = np.random.default_rng(1600 + mode)
    for i, dt in enumerate(DTYPES):
        for shape in ((60, 45), (40, 52, 36), (64, 160, 136)) if i < 2 else ((40, 52, 36),):
            lab = palette_labels(shape, dt, rng=rng, block=int(rng.integers(2, 9)), zero_frac=0.3, order="CF"[i % 2])
            for an, bb in (((1.0, 1.0, 1.0), False), ((2.0, 1.0, 3.0), True), ((0.5, 0.7, 1.3), False)):
                an = an[:len(shape)]
                want = oracle_port.sdf(lab, an, bb)
                got = edt_gpu.sdf(lab, anisotropy=an, black_border=bb)
                assert same(got, want), (dt, shape, an, bb, explain(got, want))
                wantsq = oracle_port.sdfsq(lab, an, bb)
                got = edt_gpu.sdfsq(lab, anisotropy=an, black_border=bb)
                assert same(got, wantsq), (dt, shape, an, bb, "sq", explain(got, wantsq))
                c = np.ascontiguousarray(lab)
                t = _as_tensor(c.T, "cuda")   # (the C-ordered array as a tensor of the same shape)
                got = device.sdf(t, anisotropy=an, black_border=bb).cpu().numpy()
                assert same(got, oracle_port.sdf(c, an, bb)), (dt, shape, an, bb, "device")
    torch.cuda.synchronize()


# ---- the voxel graph: native and up-sampled (debug bit 0x20000) ------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 0x20000])
def test_voxel_graph(edt_gpu, oracle_port, debug_mode, mode):
    debug_mode(mode)
    rng = np.random.default_rng(1700 + mode)
    for i, dt in enumerate(DTYPES):
        shape = [(30, 26, 22), (41, 37)][i % 2]
        lab = palette_labels(shape, dt, rng=rng, block=int(rng.integers(2, 6)), order="CF"[i % 2])
        g = np.full(shape, 0b00111111, dtype=np.uint8)
        for bit in (0x01, 0x04, 0x10):
            g[rng.random(shape) < 0.08] &= np.uint8(~bit & 0xFF)
        g = np.asfortranarray(g) if lab.flags.f_contiguous else g
        for an, bb in (((2.0, 2.0, 3.0), False), ((1.0, 1.0, 1.0), True)):
            an = an[:len(shape)]
            want = oracle_port.edtsq(lab, an, bb, voxel_graph=g)
            got = edt_gpu.edtsq(lab, anisotropy=an, black_border=bb, voxel_graph=g)
            assert same(got, want), (dt, an, bb, hex(mode), explain(got, want))


# ---- the binary route for multi-valued labels ------------------------------------------------------------------------------
def test_binary_route(edt_gpu, oracle_port):
    rng = np.random.default_rng(1800)
    for i, dt in enumerate(DTYPES):
        shape = [(50, 44, 30), (70, 60)][i % 2]
        lab = palette_labels(shape, dt, rng=rng, block=int(rng.integers(2, 6)), order="FC"[i % 2])
        for an, bb in (((1.0, 1.0, 1.0), False), ((6.0, 6.0, 30.0), True)):
            an = an[:len(shape)]
            want = oracle_port.binary_edtsq(lab, an, bb)
            got = edt_gpu.binary_edtsq(lab, anisotropy=an, black_border=bb)
            assert same(got, want), (dt, an, bb, explain(got, want))


# ---- device entry points and helpers -------------------------------------------------------------------------------------
def test_device_entry_points(edt_gpu, oracle_port):
    """edt.device with torch tensors; uint64 / uint32 / uint16 labels through their same-width signed views."""
    import torch
    from edt import device
    rng = np.random.default_rng(1900)
    for dt in DTYPES:
        lab = palette_labels((36, 50, 70), dt, rng=rng, block=4)          # C order: (z, y, x)
        t = _as_tensor(lab.T, "cuda")
        for an, bb in (((1.0, 1.0, 1.0), False), ((3.0, 2.0, 1.0), True)):
            want = oracle_port.edtsq(lab, an, bb)
            assert same(device.edtsq(t, anisotropy=an, black_border=bb).cpu().numpy(), want), (dt, an, bb)
            assert same(device.edt(t, anisotropy=an, black_border=bb).cpu().numpy(), np.sqrt(want)), (dt, an, bb)
            assert same(device.sdf(t, anisotropy=an, black_border=bb).cpu().numpy(), oracle_port.sdf(lab, an, bb))
        g = np.full(lab.shape, 0b00111111, dtype=np.uint8)
        g[rng.random(lab.shape) < 0.1] &= np.uint8(0b11111011)
        got = device.edtsq_voxel_graph(t, torch.from_numpy(g).cuda(), anisotropy=(1.0, 2.0, 1.0), black_border=True)
        assert same(got.cpu().numpy(), oracle_port.edtsq(lab, (1.0, 2.0, 1.0), True, voxel_graph=g)), dt
        stack = palette_labels((5, 40, 66), dt, rng=rng, block=3)
        got = device.edtsq_stack(_as_tensor(stack.T, "cuda"), anisotropy=(2.0, 1.0), black_border=False).cpu().numpy()
        want = np.stack([oracle_port.edtsq(im, (2.0, 1.0), False) for im in stack])
        assert same(got, want), (dt, "stack", explain(got, want))


@pytest.mark.parametrize("dt", [np.uint64, np.int64, np.uint32, np.float64, np.float32, np.int8])
def test_select_label_each_and_runs(edt_gpu, dt):
    import torch
    from edt import device
    rng = np.random.default_rng(2000)
    lab = palette_labels((20, 33, 41), dt, rng=rng, block=3)
    t = _as_tensor(lab.T, "cuda")
    dt_host = edt_gpu.edt(lab, anisotropy=(1.0, 1.0, 1.0), black_border=True)
    dtt = torch.from_numpy(dt_host).cuda()
    keys = list(palette(dt)) + [0]
    if np.dtype(dt) == np.uint64:
        keys += [2**63 + 1, -1, -(2**63 - 1)]   # unsigned values and their bit patterns as int64
    if np.dtype(dt) == np.int64:
        keys += [-1, 2**64 - 1]
    if np.dtype(dt).kind in "iu":
        keys += [-1.0, 1.0]   # whole-number float keys of integer labels
    for key in keys:
        got = device.select_label(t, dtt, key).cpu().numpy()
        if np.dtype(dt).kind in "iu":   # the label with the key's bit pattern, signed or unsigned
            size = np.dtype(dt).itemsize
            k = np.array([int(key) % (1 << (8 * size))], dtype=f"u{size}").view(dt)[0]
        else:
            k = np.asarray(key).astype(dt)
        want = np.where(lab == k, dt_host, np.float32(0))
        assert same(got, want), (dt, key, explain(got, want))
    # each: one image per non-zero label (NaN labels excluded: the reference's std::map cannot order them)
    if np.dtype(dt).kind != "f":
        seen = {k: img.cpu().numpy() for k, img in device.each(t, dtt)}
        host = dict(edt_gpu.each(lab, dt_host))
        assert len(seen) == len(host) == len(np.unique(lab[lab != 0]))
        for k, img in seen.items():
            kk = np.array([k], dtype=np.int64 if np.dtype(dt).itemsize == 8 else np.int32).astype(dt)[0] \
                if np.dtype(dt).kind in "iu" else k
            assert same(img, host[kk]), (dt, k)
    # runs: the maximal constant runs of the flattened tensor (NaN never equals its neighbour, -0.0 equals 0.0)
    starts, ends, values = device.runs(t)
    flat = lab.reshape(-1)
    want = np.concatenate(([0], np.flatnonzero(flat[1:] != flat[:-1]) + 1))
    assert np.array_equal(starts.cpu().numpy(), want)
    assert np.array_equal(ends.cpu().numpy(), np.append(want[1:], flat.size))
    v = values.cpu().numpy()
    assert np.array_equal(v.view(f"u{v.itemsize}"), flat[want].view(f"u{v.itemsize}"))
    # ... and the host run utilities (edt.runs: {value: [(start, end), ...]}) find the same runs with the same values
    host = sorted((s, e, val) for val, rns in edt_gpu.runs(lab).items() for s, e in rns)
    assert [(s, e) for s, e, _ in host] == list(zip(starts.tolist(), ends.tolist()))
    hv = np.array([val for _, _, val in host], dtype=lab.dtype)
    if hv.dtype.kind == "f":   # (NaN payloads do not survive the host utilities' Python floats)
        assert np.array_equal(hv, v, equal_nan=True)
    else:
        assert np.array_equal(hv.view(f"u{v.itemsize}"), v.view(f"u{v.itemsize}"))
