"""GPU tier of label_stats (include/edt_hip.h): every field of the table, bit for bit, against the numpy oracle
(tests/label_stats_oracle.py) -- across run / wave / row boundaries, every label dtype and its extreme keys, one label under
contention, more labels than the workgroup table holds, adversarial hash keys, ties, repeated calls, every entry point, and a
volume past 2^32 voxels."""
import ctypes

import numpy as np
import pytest

import label_stats_oracle as oracle
from synth import blocky_labels, voronoi_labels

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64, np.float32, np.float64, bool]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    from edt import _lib
    _lib.load()
    if not torch.cuda.is_available() or _lib.device_count() == 0:
        pytest.fail("the GPU tier needs a HIP device")
    torch.cuda.set_device(0)


def random_field(shape, rng):
    """float32 independent of any labels: few distinct values (ties everywhere), negative ones and +inf"""
    dt = rng.integers(-3, 4, size=shape).astype(np.float32) * np.float32(0.75)
    dt[rng.random(shape) < 0.05] = np.inf
    return dt


def to_numpy(stats):
    return oracle.LabelStats(*[t.cpu().numpy() for t in stats])


def check(data, dt, what=""):
    """edt.label_stats(data, dt) equals the oracle, for the array as given and in the other memory order"""
    import edt
    for lab, field in ((data, dt), (np.asfortranarray(data), np.asfortranarray(dt))):
        want = oracle.label_stats(lab, field)
        oracle.assert_same(edt.label_stats(lab, field), want, (what, lab.dtype, lab.shape, oracle.memory_order(lab)))
    return want


def boundary_rows(sx, sy, sz):
    """rows whose runs end exactly at lanes 63 / 64 and at the 256-voxel step of a wave, shifted by one from row to row"""
    x = np.arange(sx)
    rows = []
    for r in range(sy * sz):
        cuts = np.array([63, 64, 65, 127, 128, 255, 256, 257, 320, 511, 512, 1023, 1024]) + (r % 3) - 1
        rows.append(1 + np.searchsorted(cuts, x, side="right") % 5)
    return np.array(rows, dtype=np.uint32).reshape(sz, sy, sx)


# ---- 1. run and wave boundaries -------------------------------------------------------------------------------------
@pytest.mark.parametrize("sx", [1, 63, 64, 65, 130, 1025])
def test_run_and_wave_boundaries(sx):
    import edt
    rng = np.random.default_rng(sx)
    shape = (2, 3, sx)   # C order: x is the last axis
    vols = [blocky_labels(shape, nlabels=6, zero_frac=0.25, block=3, rng=rng).astype(np.uint32),
            np.ascontiguousarray(voronoi_labels(shape[::-1], nseeds=9, seed=sx, upsample=2, membrane=0.1).T),
            boundary_rows(sx, 3, 2)]
    for i, lab in enumerate(vols):
        check(lab, random_field(shape, rng), ("3d", i))
        check(lab, edt.edt(lab), ("3d edt", i))
        check(lab[0], random_field(shape[1:], rng), ("2d", i))
        check(lab[1, 2], random_field(shape[2:], rng), ("1d", i))
    # the long axis slowest: rows of 3 and 2 voxels, many rows per wave step
    lab = np.ascontiguousarray(vols[0].T)
    check(lab, random_field(lab.shape, rng), "short rows")


# ---- 2. every dtype, extreme keys -----------------------------------------------------------------------------------
def extreme_keys(dtype):
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return np.array([True])
    if dt.kind in "iu":
        bits = 8 * dt.itemsize
        vals = [1, 2, (1 << bits) - 1, 1 << (bits - 1), (1 << (bits - 1)) + 1, (1 << (bits - 1)) - 1]
        if bits == 64:
            vals += [1 << 32, (1 << 32) + 1, 1 << 63 | 1 << 31]
        return np.array(vals, dtype=f"u{dt.itemsize}").view(dt)
    tiny = np.finfo(dt).smallest_subnormal
    return np.array([1.0, -1.0, tiny, -tiny, np.inf, -np.inf, 2.5, -2.5, np.finfo(dt).max, np.finfo(dt).min], dtype=dt)


@pytest.mark.parametrize("dtype", DTYPES, ids=[np.dtype(d).name for d in DTYPES])
def test_every_dtype_and_its_extreme_keys(dtype):
    rng = np.random.default_rng(3)
    shape = (9, 33, 40)
    pal = extreme_keys(dtype)
    ids = blocky_labels(shape, nlabels=len(pal), zero_frac=0.2, block=3, rng=rng)
    lab = np.concatenate([np.zeros(1, dtype=pal.dtype), pal])[ids]
    if np.dtype(dtype).kind == "f":   # -0.0 is background, NaN voxels belong to no label
        lab[rng.random(shape) < 0.03] = -0.0
        lab[rng.random(shape) < 0.03] = np.nan
        lab[0, 0, :5] = [np.nan, -0.0, 1.0, np.nan, np.nan]
    want = check(lab, random_field(shape, rng), "extreme keys")
    keys = want.labels
    assert len(keys) == len(pal)
    if np.dtype(dtype).kind == "i":   # signed ascending: the sign-bit value first, -1 before 1
        assert keys[0] == np.iinfo(dtype).min and np.all(np.diff(keys.astype(object)) > 0)
        assert keys[keys.tolist().index(1) - 1] == -1
    if np.dtype(dtype).kind == "f":
        assert keys[0] == -np.inf and keys[-1] == np.inf and not np.isnan(keys).any() and np.all(keys != 0)


# ---- 3. contention: one label everywhere ----------------------------------------------------------------------------
def test_one_label_everywhere():
    import edt
    rng = np.random.default_rng(4)
    shape = (64, 64, 128)
    lab = np.ones(shape, dtype=np.uint32)
    dt = random_field(shape, rng)
    dt[dt == np.inf] = 1.0
    dt[5, 6, 7] = dt[40, 1, 2] = 9.0
    got = edt.label_stats(lab, dt)
    oracle.assert_same(got, oracle.label_stats(lab, dt))
    assert got.counts.tolist() == [lab.size] and got.argmax.tolist() == [[5, 6, 7]]
    assert got.bbox_lo.tolist() == [[0, 0, 0]] and got.bbox_hi.tolist() == [[63, 63, 127]]
    got = edt.label_stats(lab, black_border=False)   # no boundary anywhere: the field is +inf
    assert got.labels.tolist() == [1] and got.counts.tolist() == [lab.size]
    assert got.max.tolist() == [np.inf] and got.argmax.tolist() == [[0, 0, 0]]
    assert got.bbox_lo.tolist() == [[0, 0, 0]] and got.bbox_hi.tolist() == [[63, 63, 127]]


# ---- 4. many labels: the workgroup table overflows ------------------------------------------------------------------
@pytest.fixture(scope="module")
def own_labels():
    rng = np.random.default_rng(5)
    shape = (9, 33, 40)
    lab = (rng.permutation(np.prod(shape)).astype(np.uint32) + 1).reshape(shape)
    dt = random_field(shape, rng)
    return lab, dt, oracle.label_stats(lab, dt)


def call_host_abi(lab, dt, cap):
    from edt import _lib
    lib = _lib.load()
    keys = np.zeros(cap, dtype=lab.dtype)
    counts, arg = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64)
    mx, bbox, n = np.zeros(cap, dtype=np.float32), np.zeros((cap, 6), dtype=np.int32), ctypes.c_int64(-1)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    sz, sy, sx = lab.shape
    rc = lib.edt_hip_label_stats(p(lab), _lib.U32, 3, sx, sy, sz, 1.0, 1.0, 1.0, 0, p(dt), cap, p(keys), p(counts), p(mx),
                                 p(arg), p(bbox), ctypes.byref(n))
    return rc, int(n.value), keys, counts, mx, arg, bbox


def test_every_voxel_its_own_label(own_labels):
    import edt
    lab, dt, want = own_labels
    assert len(want.labels) == lab.size
    oracle.assert_same(edt.label_stats(lab, dt), want)                       # (the default capacity covers it)
    oracle.assert_same(edt.label_stats(lab, dt, max_labels=lab.size), want)
    big = np.tile(lab, (8, 1, 1))                                            # 95040 labels: more than the first capacity
    big += (np.arange(8) * lab.size).astype(np.uint32).reshape(8, 1, 1).repeat(9, axis=0)
    bdt = np.tile(dt, (8, 1, 1))
    got = edt.label_stats(big, bdt)
    assert len(got.labels) == big.size > 65536
    oracle.assert_same(got, oracle.label_stats(big, bdt), "retry")


def test_too_small_a_table_is_not_an_error(own_labels):
    import edt
    lab, dt, want = own_labels
    rc, n, *_ = call_host_abi(lab, dt, 16)
    assert rc == 0 and n > 16
    rc, n, keys, counts, mx, arg, bbox = call_host_abi(lab, dt, lab.size)   # a following call with room: correct
    assert rc == 0 and n == lab.size
    assert np.array_equal(keys, want.labels) and np.array_equal(counts, want.counts) and np.array_equal(mx, want.max)
    assert np.array_equal(arg, np.ravel_multi_index(tuple(want.argmax.T), lab.shape))
    assert np.array_equal(bbox[:, 0::2][:, ::-1], want.bbox_lo) and np.array_equal(bbox[:, 1::2][:, ::-1], want.bbox_hi)
    with pytest.raises(ValueError, match="16"):
        edt.label_stats(lab, dt, max_labels=16)
    import torch
    from edt import device
    with pytest.raises(ValueError, match="16"):
        device.label_stats(torch.from_numpy(lab.view(np.int32)).cuda(), torch.from_numpy(dt).cuda(), max_labels=16)


# ---- 5. hash stress -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_labels", [None, 900])
def test_adversarial_hash_keys(max_labels):
    import edt
    rng = np.random.default_rng(6)
    cap = 65536 if max_labels is None else max_labels
    slots = 1024
    while slots < 2 * cap:
        slots *= 2
    k = np.arange(1, 301, dtype=np.uint64)
    pal = np.concatenate([k << np.uint64(32), k << np.uint64(20), k * np.uint64(slots)])
    pal = np.unique(pal)
    shape = (6, 30, 50)
    ids = rng.permutation(np.arange(int(np.prod(shape))) % (len(pal) + 1)).reshape(shape)   # every key occurs
    lab = np.concatenate([np.zeros(1, dtype=np.uint64), pal])[ids]
    dt = random_field(shape, rng)
    want = oracle.label_stats(lab, dt)
    assert len(want.labels) == len(pal) >= 800
    oracle.assert_same(edt.label_stats(lab, dt, max_labels=max_labels), want)
    oracle.assert_same(edt.label_stats(lab.view(np.int64), dt, max_labels=max_labels), oracle.label_stats(lab.view(np.int64), dt))
    oracle.assert_same(edt.label_stats(lab.view(np.float64), dt, max_labels=max_labels),
                       oracle.label_stats(lab.view(np.float64), dt))


# ---- 6. ties --------------------------------------------------------------------------------------------------------
def test_ties_follow_memory_order():
    import edt
    lab = np.zeros((12, 70, 9), dtype=np.uint16)
    lab[3:5, 10:, 2:8] = 7    # a slab two voxels thick: with a black border every voxel of it is at distance 1
    lab[9:11, :60, 1:] = 8
    for data in (lab, np.asfortranarray(lab)):
        got = edt.label_stats(data, black_border=True)
        want = oracle.label_stats(data, edt.edt(data, black_border=True))
        oracle.assert_same(got, want, oracle.memory_order(data))
        assert got.max.tolist() == [1.0, 1.0] and got.argmax.tolist() == [[3, 10, 2], [9, 0, 1]]
        assert got.bbox_lo.tolist() == [[3, 10, 2], [9, 0, 1]] and got.bbox_hi.tolist() == [[4, 69, 7], [10, 59, 8]]
    # a maximum shared by two voxels, one first in C order and the other first in F order
    dt = np.zeros(lab.shape, dtype=np.float32)
    dt[3, 60, 3] = dt[4, 11, 2] = 2.0
    assert edt.label_stats(lab, dt).argmax.tolist()[0] == [3, 60, 3]
    assert edt.label_stats(np.asfortranarray(lab), np.asfortranarray(dt)).argmax.tolist()[0] == [4, 11, 2]


# ---- 7. determinism -------------------------------------------------------------------------------------------------
def test_repeated_calls_give_the_same_bits(own_labels):
    import torch
    from edt import device
    rng = np.random.default_rng(7)
    big = np.ascontiguousarray(voronoi_labels((96, 96, 96), nseeds=2000, seed=2, upsample=2).T)
    cases = [(own_labels[0], own_labels[1]), (big, random_field(big.shape, rng))]
    for lab, dt in cases:
        tl, td = torch.from_numpy(lab.view(np.int32)).cuda(), torch.from_numpy(dt).cuda()
        first = to_numpy(device.label_stats(tl, td))
        assert len(first.labels) == len(np.unique(lab[lab != 0]))
        for _ in range(4):
            again = to_numpy(device.label_stats(tl, td))
            for a, b in zip(first, again):
                assert a.tobytes() == b.tobytes()
    oracle.assert_same(oracle.LabelStats(first.labels.view(np.uint32), *first[1:]), oracle.label_stats(*cases[1]))


# ---- 8. the entry points agree --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32, np.int64, np.float32, bool])
def test_entry_points_agree(dtype):
    import edt
    import torch
    from edt import device
    ids = blocky_labels((10, 21, 70), nlabels=9, zero_frac=0.2, block=4, rng=np.random.default_rng(8))
    lab = (ids != 0) if dtype is bool else (ids - 4).astype(dtype)   # (negative labels for the signed types)
    for an, bb in (((1.0, 1.0, 1.0), False), ((30.0, 6.0, 6.0), True), ((40.0, 3.58, 3.58), False), ((1.5, 0.7, 1.1), True)):
        dt = edt.edt(lab, anisotropy=an, black_border=bb)
        want = oracle.label_stats(lab, dt)
        oracle.assert_same(edt.label_stats(lab, dt), want, (an, bb, "dt given"))
        oracle.assert_same(edt.label_stats(lab, anisotropy=an, black_border=bb), want, (an, bb, "dt=None"))
        fl = np.asfortranarray(lab)
        oracle.assert_same(edt.label_stats(fl, anisotropy=an, black_border=bb),
                           oracle.label_stats(fl, edt.edt(fl, anisotropy=an, black_border=bb)), (an, bb, "dt=None, F"))
        got = device.label_stats(torch.from_numpy(lab).cuda(), torch.from_numpy(dt).cuda())
        assert all(t.is_cuda for t in got)
        oracle.assert_same(to_numpy(got), want, (an, bb, "device"))
    # 2-D and 1-D through the device API
    for sub in (lab[3], lab[3, 5]):
        dt = edt.edt(sub)
        oracle.assert_same(to_numpy(device.label_stats(torch.from_numpy(sub).cuda(), torch.from_numpy(dt).cuda())),
                           oracle.label_stats(sub, dt), sub.shape)


# ---- 9. past 2^32 voxels --------------------------------------------------------------------------------------------
def test_past_two_to_the_32_voxels():
    import torch
    from edt import device
    free, _ = torch.cuda.mem_get_info()
    if free < 24 << 30:
        pytest.skip(f"needs 24 GiB of free device memory (labels 4 GiB + field 16 GiB), {free >> 30} GiB are free")
    shape = (2, 32769, 65536)
    voxels = shape[0] * shape[1] * shape[2]
    assert voxels > 1 << 32
    lab = torch.ones(shape, dtype=torch.uint8, device="cuda")
    dt = torch.zeros(shape, dtype=torch.float32, device="cuda")
    flat_l, flat_d = lab.view(-1), dt.view(-1)
    # three other labels past 2^32 (label 9 also before it), distinct maxima past 2^32
    placed = {5: [(1 << 32) + 7, (1 << 32) + 65536 + 9], 200: [voxels - 1], 9: [123, (1 << 32) + 65536 + 100]}
    for key, offs in placed.items():
        for o in offs:
            flat_l[o] = key
    peaks = {1: ((1 << 32) + 12345, 3.0), 5: ((1 << 32) + 65536 + 9, 2.0), 9: ((1 << 32) + 65536 + 100, 7.0)}
    for key, (o, v) in peaks.items():
        flat_d[o] = v
    flat_d[(1 << 32) + 99999] = 3.0   # label 1's maximum again, later: the first one counts
    got = to_numpy(device.label_stats(lab, dt))
    del lab, dt, flat_l, flat_d
    torch.cuda.empty_cache()

    def coords(o):
        return [o // (shape[1] * shape[2]), (o // shape[2]) % shape[1], o % shape[2]]

    assert got.labels.tolist() == [1, 5, 9, 200]
    assert got.counts.tolist() == [voxels - 5, 2, 2, 1]
    assert got.max.tolist() == [3.0, 2.0, 7.0, 0.0]
    assert got.argmax.tolist() == [coords(peaks[1][0]), coords(peaks[5][0]), coords(peaks[9][0]), coords(voxels - 1)]
    boxes = {key: np.array([coords(o) for o in offs]) for key, offs in placed.items()}
    assert got.bbox_lo.tolist() == [[0, 0, 0]] + [boxes[k].min(0).tolist() for k in (5, 9, 200)]
    assert got.bbox_hi.tolist() == [[shape[0] - 1, shape[1] - 1, shape[2] - 1]] + [boxes[k].max(0).tolist() for k in (5, 9, 200)]
    assert boxes[5].tolist() == [[1, 32767, 7], [1, 32768, 9]] and boxes[9].tolist() == [[0, 0, 123], [1, 32768, 100]]
