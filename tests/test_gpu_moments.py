"""GPU tier of label_moments (include/edt_hip.h, "label_moments"): the raw ABI and both Python forms against the
Python-integer oracle (tests/moments_oracle.py) -- array_equal on keys, counts and sums and on the BITS of centroid and
covariance -- across run / wave / row / tile boundaries, the one-label short cut, every label dtype, more labels than the
workgroup table holds, adversarial hash keys, the capacity rule, sums past 2^53 and M_ab past 2^64, offset pointers, a dirty
reused workspace, capture and replay, repeated calls and the composition with connected_components."""
import ctypes

import numpy as np
import pytest

import moments_oracle as oracle
from synth import bits_of, blocky_labels, offset_out, offset_view, outside_intact

pytestmark = pytest.mark.gpu

U8, U16, U32, U64, F32, F64, BOOL = range(7)
CODE = {"uint8": U8, "int8": U8, "uint16": U16, "int16": U16, "uint32": U32, "int32": U32, "uint64": U64, "int64": U64,
        "float32": F32, "float64": F64, "bool": BOOL}
MARK = 0xA5A5A5A5A5A5A5A5


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


def ext3(a):
    return tuple(int(e) for e in a.shape[::-1]) + (1,) * (3 - a.ndim)


def upload(a):
    """a C-ordered numpy array as a device tensor (unsigned 16/32/64-bit types as the signed type of their width)"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u" and a.dtype.itemsize > 1:
        a = a.view(f"i{a.dtype.itemsize}")
    return torch.from_numpy(a.copy()).cuda()


class Abi:
    """One raw edt_hip_label_moments_device call on a C-ordered array: outputs of `cap` rows behind an element offset `k`,
    holding a sentinel; run(ws) enqueues it on the current stream, table() reads the first n rows back."""

    def __init__(self, lab, cap=None, code=None, k=0, k_lab=0):
        import torch
        self.lab, self.code, self.k = lab, CODE[lab.dtype.name] if code is None else code, k
        self.n_want = None
        self.cap = int(cap if cap is not None else max(1, len(np.unique(lab))))
        self.lbuf, self.labels = offset_view(lab, k_lab)
        kdt = lab.dtype if lab.dtype.kind == "f" else np.dtype(f"u{lab.dtype.itemsize}")
        self.kdt = kdt
        mark = MARK % (1 << (8 * kdt.itemsize))
        self.bufs = {}
        for name, shape, dt, m in (("keys", (self.cap,), kdt, mark), ("counts", (self.cap,), np.int64, MARK),
                                   ("sums", (self.cap, 9), np.int64, MARK), ("centroid", (self.cap, 3), np.float64, MARK),
                                   ("central", (self.cap, 6), np.float64, MARK), ("n", (1,), np.int64, MARK)):
            self.bufs[name] = offset_out(shape, dt, k, m) + (m,)
        self.nbytes = int(lib().edt_hip_label_moments_workspace_bytes(self.code, lab.size, self.cap))
        assert self.nbytes > 0
        self.torch = torch

    def workspace(self):
        return self.torch.empty(self.nbytes, dtype=self.torch.uint8, device="cuda")

    def run(self, ws=None):
        from edt import _lib
        ws = self.workspace() if ws is None else ws
        v = {name: b[1] for name, b in self.bufs.items()}
        rc = lib().edt_hip_label_moments_device(vp(self.labels), self.code, self.lab.ndim, *ext3(self.lab), self.cap, vp(v["keys"]),
                                                vp(v["counts"]), vp(v["sums"]), vp(v["centroid"]), vp(v["central"]), vp(v["n"]),
                                                vp(ws), ws.numel(), stream())
        _lib.check(rc)
        return self

    def n(self):
        self.torch.cuda.synchronize()
        return int(self.bufs["n"][1][0])

    def table(self):
        n = self.n()
        assert 0 <= n <= self.cap, (n, self.cap)
        for name, (buf, view, m) in self.bufs.items():
            assert outside_intact(buf, self.k, view.numel(), m), (name, "a store outside the output")
        v = {name: b[1] for name, b in self.bufs.items()}
        keys = bits_of(v["keys"][:n])
        if self.kdt.kind == "f":
            keys = keys.view(self.kdt)
        return (keys, v["counts"][:n].cpu().numpy(), v["sums"][:n].cpu().numpy(), bits_of(v["centroid"][:n]), bits_of(v["central"][:n]))


def same_table(got, want, what):
    keys, counts, sums, centroid, central = want
    want = (keys, counts, sums, np.ascontiguousarray(centroid).view(np.uint64), np.ascontiguousarray(central).view(np.uint64))
    for name, g, w in zip(("keys", "counts", "sums", "centroid", "central"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, g[:6], w[:6])


def to_numpy(m):
    return oracle.LabelMoments(*[t.cpu().numpy() for t in m])


def check(lab, what="", python=True, **abi_kw):
    """the raw ABI, edt.label_moments (the array as given and in the other memory order) and edt.device.label_moments equal the
    oracle"""
    import edt
    from edt import device
    want = oracle.label_moments(lab)
    same_table(Abi(lab, **abi_kw).run().table(), oracle.abi_table(lab, want), (what, "abi", lab.dtype, lab.shape))
    if python:
        oracle.assert_same(edt.label_moments(lab), want, (what, "host C", lab.shape))
        oracle.assert_same(edt.label_moments(np.asfortranarray(lab)), want, (what, "host F", lab.shape))
        got = device.label_moments(upload(lab))
        assert all(t.is_cuda for t in got)
        if lab.dtype.kind == "u" and lab.dtype.itemsize > 1:   # (torch holds them as signed: compare the bit patterns' tables)
            want = oracle.label_moments(lab.view(f"i{lab.dtype.itemsize}"))
        oracle.assert_same(to_numpy(got), want, (what, "device", lab.shape))
    return want


def run_labels(shape, rng, nlabels=5, longest=90):
    """labels from {0..nlabels} in runs of 1..longest voxels along the memory order: runs end inside rows, cross the 64-lane
    groups and the 256-voxel steps, and rows end inside runs"""
    size = int(np.prod(shape))
    lengths = rng.integers(1, longest + 1, size=size // 2 + 2)
    values = rng.integers(0, nlabels + 1, size=len(lengths))
    return np.repeat(values, lengths)[:size].reshape(shape).astype(np.uint32)


# ---- 1. run and row geometry --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sx", [1, 33, 64, 65, 100, 256, 300, 513])
def test_run_and_row_geometry(sx):
    rng = np.random.default_rng(sx)
    check(run_labels((3, 5, sx), rng), "runs of 1..90")
    assert len(check(run_labels((3, 5, sx), rng, longest=4), "runs of 1..4").labels) >= 3     # (what a volume of 15 voxels can hold)


@pytest.mark.parametrize("sx", [256, 300])
def test_one_label_throughout(sx):
    """sx = 256: every step is one label inside one row (the short cut); sx = 300: every step crosses a row (never taken)"""
    lab = np.full((3, 5, sx), 7, dtype=np.uint32)
    want = check(lab, "one label")
    assert want.counts.tolist() == [lab.size] and want.centroid.tolist() == [[1.0, 2.0, (sx - 1) / 2]]


def test_only_background():
    import edt
    lab = np.zeros((3, 5, 300), dtype=np.uint32)
    assert Abi(lab).run().n() == 0
    got = edt.label_moments(lab)
    assert got.labels.shape == (0,) and got.second.shape == (0, 3, 3)


@pytest.mark.parametrize("shape", [(257,), (7, 73), (3, 5, 17), (2, 769)])
def test_last_partial_tile(shape):
    assert int(np.prod(shape)) % 256 in (1, 2, 255)
    lab = run_labels(shape, np.random.default_rng(len(shape)), longest=40)
    lab.flat[-1] = 5                                       # the very last voxel counts
    check(lab, "partial tile")


def test_past_one_trip():
    """128^3 uint8: 8192 steps for the 7168 waves of the largest grid -- waves that take a second step"""
    rng = np.random.default_rng(6)
    lab = blocky_labels((128, 128, 128), nlabels=200, zero_frac=0.2, block=9, rng=rng).astype(np.uint8)
    want = check(lab, "second trip", python=False)
    assert len(want.labels) > 150


# ---- 2. every dtype -----------------------------------------------------------------------------------------------------
def top_keys(dtype):
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        bits = 8 * dt.itemsize
        return np.array([1, 2, (1 << bits) - 1, 1 << (bits - 1), (1 << (bits - 1)) - 1], dtype=f"u{dt.itemsize}").view(dt)
    tiny = np.finfo(dt).smallest_subnormal
    return np.array([1.0, -1.0, tiny, -tiny, np.inf, -np.inf, 2.5, np.finfo(dt).max], dtype=dt)


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64, np.float32,
                                   np.float64], ids=lambda d: np.dtype(d).name)
def test_every_dtype_and_the_top_of_its_range(dtype):
    rng = np.random.default_rng(3)
    shape = (5, 13, 70)
    pal = top_keys(dtype)
    ids = blocky_labels(shape, nlabels=len(pal), zero_frac=0.2, block=3, rng=rng)
    lab = np.concatenate([np.zeros(1, dtype=pal.dtype), pal])[ids]
    if np.dtype(dtype).kind == "f":   # -0.0 is background, NaN voxels belong to no label
        lab[rng.random(shape) < 0.03] = -0.0
        lab[rng.random(shape) < 0.03] = np.nan
        lab[0, 0, :5] = [np.nan, -0.0, 1.0, np.nan, np.nan]
    want = check(lab, "top keys")
    assert len(want.labels) == len(pal)
    if np.dtype(dtype).kind == "f":
        assert want.labels[0] == -np.inf and want.labels[-1] == np.inf and np.all(want.labels != 0)


def test_bool_bytes_one_and_two_are_one_label():
    import edt
    rng = np.random.default_rng(4)
    raw = rng.integers(0, 3, size=(4, 9, 130)).astype(np.uint8)          # bytes 0, 1 and 2
    want = oracle.label_moments(raw != 0)
    same_table(Abi(raw, code=BOOL, cap=1).run().table(), oracle.abi_table(raw != 0, want), "bool bytes")
    oracle.assert_same(edt.label_moments(raw != 0), want, "bool")
    assert want.labels.tolist() == [True]


# ---- 3. more labels than the workgroup's table, adversarial keys ---------------------------------------------------------
def test_every_voxel_its_own_label():
    lab = (np.arange(64 * 64 * 4, dtype=np.uint32) + 1).reshape(4, 64, 64)   # 1024 labels through every workgroup's range
    want = check(lab, "own labels")
    assert len(want.labels) == lab.size and np.all(want.covariance == 0.0)


@pytest.mark.parametrize("max_labels", [None, 900])
def test_adversarial_hash_keys(max_labels):
    import edt
    rng = np.random.default_rng(6)
    cap = 65536 if max_labels is None else max_labels
    slots = 1024
    while slots < 2 * cap:
        slots *= 2
    k = np.arange(1, 301, dtype=np.uint64)
    pal = np.unique(np.concatenate([k << np.uint64(32), k << np.uint64(20), k * np.uint64(slots)]))
    shape = (6, 30, 50)
    ids = rng.permutation(np.arange(int(np.prod(shape))) % (len(pal) + 1)).reshape(shape)   # every key occurs
    lab = np.concatenate([np.zeros(1, dtype=np.uint64), pal])[ids]
    want = oracle.label_moments(lab)
    assert len(want.labels) == len(pal) >= 800
    oracle.assert_same(edt.label_moments(lab, max_labels=max_labels), want)
    same_table(Abi(lab, cap=cap).run().table(), oracle.abi_table(lab, want), "adversarial keys")
    oracle.assert_same(edt.label_moments(lab.view(np.float64), max_labels=max_labels), oracle.label_moments(lab.view(np.float64)))


# ---- 4. capacity --------------------------------------------------------------------------------------------------------
def test_capacity_rule():
    import edt
    from edt import device
    lab = (np.arange(6 * 128 * 128, dtype=np.uint32) + 1).reshape(6, 128, 128)   # 98304 labels: more than the first capacity
    for short in (lab[0, :3], lab[:1]):
        nlab = short.size
        assert Abi(short, cap=nlab - 1).run().n() > nlab - 1                         # EDT_OK, and the caller retries
        assert Abi(short, cap=nlab).run().n() == nlab
    want = oracle.label_moments(lab)
    oracle.assert_same(edt.label_moments(lab), want, "retry, host")
    oracle.assert_same(to_numpy(device.label_moments(upload(lab))), oracle.label_moments(lab.view(np.int32)), "retry, device")
    with pytest.raises(ValueError, match="16"):
        edt.label_moments(lab, max_labels=16)
    with pytest.raises(ValueError, match="16"):
        device.label_moments(upload(lab), max_labels=16)


# ---- 5. exactness past 2^53 ---------------------------------------------------------------------------------------------
def test_exact_past_two_to_the_53():
    """float accumulation and a covariance built by subtracting rounded numbers both show here: M_xx of the lines and M_zz of
    the interleaved labels are past 2^64, S_xx of the longer line is past 2^53, and the far-corner object's covariance (1/4)
    is tiny against S^2 / n"""
    line = np.ones(300000, dtype=np.uint8)
    want = check(line, "line")
    assert int(want.counts[0]) * int(want.second[0, 0, 0]) - int(want.first[0, 0]) ** 2 > 1 << 64
    want = check(np.ones(400000, dtype=np.uint8), "longer line")
    assert int(want.second[0, 0, 0]) > 1 << 53
    two = np.empty((60000, 4, 3), dtype=np.uint16)
    two[0::2], two[1::2] = 1, 2
    want = check(two, "interleaved")
    assert int(want.counts[0]) * int(want.second[0, 0, 0]) - int(want.first[0, 0]) ** 2 > 1 << 64
    far = np.zeros((3000, 40, 40), dtype=np.uint32)
    far[-2:, -2:, -2:] = 9
    want = check(far, "far corner")
    assert want.covariance[0].tolist() == [[0.25, 0.0, 0.0], [0.0, 0.25, 0.0], [0.0, 0.0, 0.25]]
    assert want.centroid[0].tolist() == [2998.5, 38.5, 38.5]


# ---- 6. the contract of the device form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k_lab,k", [(np.uint8, 1, 1), (np.uint8, 3, 1), (np.uint16, 1, 3), (np.uint32, 1, 1), (np.uint64, 1, 1)])
def test_offset_pointers(dtype, k_lab, k):
    lab = run_labels((3, 7, 101), np.random.default_rng(k_lab), longest=30).astype(dtype)
    same_table(Abi(lab, k=k, k_lab=k_lab).run().table(), oracle.abi_table(lab), ("offsets", dtype, k_lab, k))


@pytest.fixture(scope="module")
def two_volumes():
    rng = np.random.default_rng(8)
    a = run_labels((5, 20, 77), rng, nlabels=40)
    b = (blocky_labels((5, 20, 77), nlabels=90, zero_frac=0.3, block=4, rng=rng).astype(np.uint32) * np.uint32(2654435761)) | np.uint32(1)
    b[blocky_labels((5, 20, 77), nlabels=1, zero_frac=0.5, block=6, rng=rng) == 0] = 0
    return [(v, oracle.abi_table(v)) for v in (a, b)]


def test_dirty_workspace_reused_across_volumes(two_volumes):
    calls = [Abi(v, cap=128) for v, _ in two_volumes]
    ws = calls[0].workspace()
    assert calls[0].nbytes == calls[1].nbytes
    for pattern in (0xFF, 0x5A):
        for nth in range(2):
            for call, (_, want) in zip(calls, two_volumes):
                if nth == 0:
                    ws.fill_(pattern)
                same_table(call.run(ws).table(), want, ("dirty workspace", hex(pattern), nth))


def test_capture_and_replay_on_dirty_scratch(two_volumes):
    import torch
    lab, want = two_volumes[0]
    call = Abi(lab, cap=128)
    ws = call.workspace()
    same_table(call.run(ws).table(), want, "warm-up")          # lazy code-object loads happen outside the capture
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call.run(ws)
    for pattern in (0xFF, 0x5A):
        ws.fill_(pattern)
        for _, view, _ in call.bufs.values():
            view.view(torch.int64 if view.element_size() == 8 else torch.int32).fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        same_table(call.table(), want, ("replay", hex(pattern)))


def test_two_calls_give_identical_bytes():
    from edt import device
    lab = np.ascontiguousarray(blocky_labels((48, 48, 96), nlabels=3000, zero_frac=0.2, block=3, rng=np.random.default_rng(9)).astype(np.int32))
    t = upload(lab)
    first = to_numpy(device.label_moments(t))
    assert len(first.labels) > 1000
    for _ in range(3):
        again = to_numpy(device.label_moments(t))
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes()
    oracle.assert_same(first, oracle.label_moments(lab), "many labels")


# ---- 7. composition, memory orders, dimensionalities --------------------------------------------------------------------
def test_composes_with_connected_components_on_the_device():
    import edt
    from edt import device
    mask = np.random.default_rng(10).random((40, 40, 40)) < 0.3
    comps, n = device.connected_components(upload(mask.astype(np.uint8)), connectivity=1)
    got = to_numpy(device.label_moments(comps))
    host = edt.connected_components(mask.astype(np.uint8), connectivity=1)
    want = oracle.label_moments(host.astype(np.int32))
    assert len(want.labels) == int(n) > 100
    oracle.assert_same(got, want, "components")
    assert want.labels.tolist() == list(range(1, int(n) + 1))


@pytest.mark.parametrize("shape", [(300,), (9, 70), (70, 9), (4, 6, 35)])
def test_both_python_forms_in_both_memory_orders(shape):
    import edt
    from edt import device
    lab = blocky_labels(shape, nlabels=6, zero_frac=0.25, block=3, rng=np.random.default_rng(len(shape))).astype(np.int16) - 3
    want = oracle.label_moments(lab)
    assert want.labels[0] < 0 < want.labels[-1]                          # signed order
    for data in (lab, np.asfortranarray(lab)):
        got = edt.label_moments(data)
        oracle.assert_same(got, want, (shape, data.flags.f_contiguous))
        assert got.first.shape == (len(want.labels), len(shape)) and got.second.shape == (len(want.labels),) + (len(shape),) * 2
    got = device.label_moments(upload(lab))
    oracle.assert_same(to_numpy(got), want, (shape, "device"))
    # principal axes: the same code on the host's and on the device's result
    for a, b in zip(edt.label_moments(lab).principal((2.0,) * len(shape)), got.principal((2.0,) * len(shape))):
        assert a.tobytes() == b.tobytes()
