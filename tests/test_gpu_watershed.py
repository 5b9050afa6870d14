"""GPU tier of watershed: bit-for-bit agreement with the numpy + csgraph oracle (tests/watershed_oracle.py), output and N, on
shapes chosen where the code can break -- runs cut at 256 voxels, chunks of 2048, 64-lane groups, unit axes --, over every
connectivity, `binary`, every label dtype and the fields the contract names; identity with connected_components where the
contract promises it; field=None on both surfaces; determinism under the densest ties; the workspace and stream contract of the
device ABI with the helpers of tests/test_gpu_workspace_contract.py; offset pointers; a seeded fuzz."""
import ctypes

import numpy as np
import pytest

import components_oracle
import watershed_oracle as oracle
from synth import blocky_labels
from test_gpu_workspace_contract import Case, capture_and_replay, device_out, fill, fresh_workspace, two_calls, upload

pytestmark = pytest.mark.gpu

BAD_ARG = -2
SHAPES = [(5000,), (3, 2049), (50, 257), (257, 3), (5, 7, 300), (3, 70, 65), (33, 31, 29), (29, 31, 1), (1, 1, 63)]
DTYPES = [np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64, np.bool_]
FIELDS = ["edt_black_border", "edt_open_border", "random", "small_integers", "constant", "signed_zeros", "infinite_patches"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    from edt import _lib
    _lib.load()
    if not torch.cuda.is_available() or _lib.device_count() == 0:
        pytest.fail("the GPU tier needs a HIP device")
    torch.cuda.set_device(0)


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_labels(shape, dtype, seed, zero_frac=0.15, block=6):
    """blocky multi-label volume; float dtypes carry a NaN and a -0.0, and labels that differ beyond 32 bits ride in uint64"""
    rng = np.random.default_rng(seed)
    ids = blocky_labels(shape, nlabels=3, zero_frac=zero_frac, block=block, rng=rng)
    if np.dtype(dtype) == np.bool_:
        return ids != 0
    lab = ids.astype(dtype)
    if np.dtype(dtype) == np.uint64:
        lab[lab == 2] = (1 << 40) + 2
        lab[lab == 3] = (1 << 41) + 2
    if np.dtype(dtype).kind == "f" and lab.size > 4:
        flat = lab.reshape(-1)
        flat[lab.size // 3] = np.nan
        flat[lab.size // 3 + 1] = np.nan
        flat[lab.size // 2] = -0.0
    return lab


def make_field(kind, lab, seed, anisotropy=None):
    """a float32 field of the labels' shape (numpy); the two transforms are the library's own, from the device"""
    from edt import device
    rng = np.random.default_rng(seed + 1000)
    shape = lab.shape
    if kind.startswith("edt"):
        src = lab.view(np.uint8) if lab.dtype == np.bool_ else np.nan_to_num(lab, nan=7.0) if lab.dtype.kind == "f" else lab
        f = device.edt(upload(src), anisotropy=anisotropy, black_border=(kind == "edt_black_border")).cpu().numpy()
        assert not np.isnan(f).any()
        return f
    if kind == "infinite_patches":                                          # what a transform without a border leaves, in places
        f = rng.integers(0, 4, size=shape).astype(np.float32)
        f[blocky_labels(shape, nlabels=1, zero_frac=0.6, block=3, rng=rng) != 0] = np.inf
        return f
    if kind == "random":
        return rng.permutation(lab.size).reshape(shape).astype(np.float32) * np.float32(0.37) - np.float32(7.0)
    if kind == "small_integers":
        return rng.integers(0, 3, size=shape).astype(np.float32)
    if kind == "constant":
        return np.full(shape, 1.25, dtype=np.float32)
    f = (rng.integers(-2, 3, size=shape) * 0.5).astype(np.float32)          # signed_zeros: negative values and both zeros
    f[(f == 0) & (rng.random(shape) < 0.5)] = -0.0
    return f


def run_device(lab, f, h, c, binary):
    """(out as uint32 numpy, N) of device.watershed"""
    from edt import device
    t = upload(lab.view(np.uint8) if lab.dtype == np.bool_ else lab)
    if lab.dtype == np.bool_:
        t = t.bool()
    out, n = device.watershed(t, upload(f), min_saliency=h, connectivity=c, binary=binary)
    assert out.dtype.is_signed and out.shape == t.shape and n.dim() == 0 and n.is_cuda
    return out.cpu().numpy().view(np.uint32), int(n.item())


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_parity_with_the_oracle(shape):
    nd = len(shape)
    k = SHAPES.index(shape)
    split = 0
    for c in range(1, nd + 1):
        for j, kind in enumerate(FIELDS):
            if int(np.prod(shape)) > 20000 and (j + c) % 2:        # the largest shape: every field, at alternating connectivities
                continue
            dtype = DTYPES[(k + j + 3 * c) % len(DTYPES)]
            binary = bool((k + j + c) % 2)
            aniso = ((1.0, 1.0, 1.0) if j % 2 == 0 else (6.0, 6.0, 30.0))[:nd]
            lab = make_labels(shape, dtype, seed=100 * k + 10 * c + j)
            f = make_field(kind, lab, seed=k, anisotropy=aniso)
            hs = (0.0, 0.5 * min(aniso), 1.0, 1e30)
            for h, (want, n_want) in zip(hs, oracle.ladder(lab, f, hs, c, binary)):
                got, n = run_device(lab, f, h, c, binary)
                assert n == n_want, (shape, c, kind, dtype.__name__, binary, h, n, n_want)
                assert np.array_equal(got, want), (shape, c, kind, dtype.__name__, binary, h, int((got != want).sum()))
                split += n
    assert split > 0


def test_every_dtype_meets_every_connectivity_and_binary():
    """the rotation of test_parity_with_the_oracle leaves combinations out: here every label dtype at every connectivity, with and
    without `binary`, on one small 3-D shape past one 256-voxel run and one 64-lane group"""
    shape = (5, 9, 67)
    for i, dtype in enumerate(DTYPES):
        lab = make_labels(shape, dtype, seed=i)
        f = make_field("small_integers" if i % 2 else "edt_black_border", lab, seed=i)
        for c in (1, 2, 3):
            for binary in (False, True):
                for h, (want, n_want) in zip((0.0, 1.0), oracle.ladder(lab, f, (0.0, 1.0), c, binary)):
                    got, n = run_device(lab, f, h, c, binary)
                    assert n == n_want and np.array_equal(got, want), (dtype.__name__, c, binary, h)


def test_bit_identity_with_connected_components():
    import torch
    from edt import device
    for shape, dtype in (((33, 31, 29), np.uint32), ((50, 257), np.float32), ((5000,), np.uint8), ((5, 7, 300), np.bool_)):
        lab = make_labels(shape, dtype, seed=7, zero_frac=0.3, block=4)
        t = upload(lab.view(np.uint8) if lab.dtype == np.bool_ else lab)
        t = t.bool() if lab.dtype == np.bool_ else t
        finite = upload(make_field("random", lab, seed=3))
        constant = upload(make_field("constant", lab, seed=3))
        for c in range(1, len(shape) + 1):
            for binary in (False, True):
                want, n_want = device.connected_components(t, connectivity=c, binary=binary)
                assert np.array_equal(want.cpu().numpy().view(np.uint32), components_oracle.connected_components(lab, c, binary))
                for f, h in ((constant, 0.0), (constant, 0.5), (finite, 1e30)):
                    got, n = device.watershed(t, f, min_saliency=h, connectivity=c, binary=binary)
                    assert int(n.item()) == int(n_want.item()) and bool((got == want).all()), (shape, c, binary, h)
    # one label everywhere under an open border: the library's own transform is +inf throughout -- a constant field
    ones = torch.ones((9, 20, 70), dtype=torch.int32, device="cuda")
    f = device.edt(ones, black_border=False)
    assert bool(torch.isinf(f).all())
    for h in (0.0, 0.5):
        got, n = device.watershed(ones, f, min_saliency=h)
        assert int(n.item()) == 1 and bool((got == 1).all())


def test_field_none_is_the_librarys_own_transform():
    import edt
    from edt import device
    signed = make_labels((9, 40, 33), np.int16, seed=5)
    signed[signed == 2] = -2                                  # a signed dtype, through the Python surfaces only
    for an, bb, binary, h in (((1.0, 1.0, 1.0), False, False, 0.5), ((6.0, 6.0, 30.0), True, True, 3.0), ((2.0, 1.0, 3.0), True, False, 0.0)):
        t = upload(signed)
        src = (t != 0) if binary else t
        f = device.edt(src, anisotropy=an, black_border=bb)
        want, n_want = device.watershed(t, f, min_saliency=h, binary=binary)
        got, n = device.watershed(t, None, min_saliency=h, anisotropy=an, black_border=bb, binary=binary)
        assert int(n.item()) == int(n_want.item()) and bool((got == want).all()), (an, bb, binary, "device")
        ref, n_ref = oracle.watershed(signed, f.cpu().numpy(), h, None, binary, return_N=True)
        assert n_ref == int(n.item()) and np.array_equal(got.cpu().numpy().view(np.uint32), ref)
        # host arrays: C order, and F order (the same memory read as the transposed volume)
        out, n_host = edt.watershed(signed, min_saliency=h, anisotropy=an, black_border=bb, binary=binary, return_N=True)
        assert out.flags.c_contiguous and n_host == n_ref and np.array_equal(out, ref), (an, bb, binary, "host C")
        out, n_host = edt.watershed(signed, f.cpu().numpy(), min_saliency=h, binary=binary, return_N=True)
        assert n_host == n_ref and np.array_equal(out, ref), (an, bb, binary, "host C, field given")
        fort = np.asfortranarray(signed)
        f_fort = edt.edt((fort != 0) if binary else fort, anisotropy=an, black_border=bb)
        ref_f, n_f = oracle.watershed(fort, f_fort, h, None, binary, return_N=True)
        out, n_host = edt.watershed(fort, min_saliency=h, anisotropy=an, black_border=bb, binary=binary, return_N=True)
        assert out.flags.f_contiguous and n_host == n_f and np.array_equal(out, ref_f), (an, bb, binary, "host F")
        out = edt.watershed(fort, np.asfortranarray(f_fort), min_saliency=h, binary=binary)
        assert out.flags.f_contiguous and np.array_equal(out, ref_f), (an, bb, binary, "host F, field given")


def test_the_result_does_not_depend_on_who_won_an_atomic():
    """the densest ties: a field of three small integers at full connectivity, with the saliency round -- five runs, one answer"""
    lab = make_labels((33, 31, 29), np.uint32, seed=11, zero_frac=0.05)
    f = make_field("small_integers", lab, seed=11)
    want, n_want = oracle.watershed(lab, f, 1.0, 3, True, return_N=True)
    runs = [run_device(lab, f, 1.0, 3, True) for _ in range(5)]
    for got, n in runs:
        assert n == n_want and got.tobytes() == runs[0][0].tobytes()
    assert np.array_equal(runs[0][0], want)


def test_a_nan_field_terminates_with_numbers_in_range():
    lab = make_labels((7, 20, 70), np.uint8, seed=2)
    f = make_field("random", lab, seed=2)
    f[np.random.default_rng(0).random(f.shape) < 0.2] = np.nan
    for h in (0.0, 1.0):
        got, n = run_device(lab, f, h, 3, False)
        assert np.array_equal(got == 0, lab == 0) and 1 <= n and got.max() == n and len(np.unique(got[got > 0])) == n


# ---- the device ABI: workspace, stream, pointers ---------------------------------------------------------------------------
EXT = (65, 40, 9)                          # (sx, sy, sz)


def abi_case(lab, f, h, c, binary, out=None, labels_t=None, field_t=None, want=None):
    """edt_hip_watershed_device as a Case of tests/test_gpu_workspace_contract.py; lab, f: C-ordered (z, y, x) numpy arrays"""
    import torch
    from edt import _lib, device
    lib = _lib.load()
    ext = tuple(int(e) for e in lab.shape[::-1])
    code = device.dtype_code(upload(lab[:1]).dtype)
    labels_t = upload(lab) if labels_t is None else labels_t
    field_t = upload(f) if field_t is None else field_t
    out = device_out(lab.shape, np.uint32) if out is None else out
    n = device_out((1,), np.int64)
    want, n_want = oracle.watershed(lab, f, h, c, binary, return_N=True) if want is None else want
    nbytes = lib.edt_hip_watershed_workspace_bytes(code, 3, *ext)

    def call(ws):
        _lib.check(lib.edt_hip_watershed_device(vp(labels_t), code, 3, *ext, vp(field_t), c, int(binary), h, vp(out), vp(n), vp(ws),
                                                ws.numel(), stream()))

    def check(what):
        assert int(n.cpu()[0]) == n_want, (what, int(n.cpu()[0]), n_want)
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want), (what, int((got != want).sum()))

    return Case(f"watershed h={h} c={c}", nbytes, call, check, outputs=(out, n))


@pytest.fixture(scope="module")
def abi_volumes():
    shape = EXT[::-1]
    a = make_labels(shape, np.uint32, seed=21)
    b = make_labels(shape, np.uint32, seed=22, zero_frac=0.4, block=3)
    return (a, make_field("edt_black_border", a, seed=21)), (b, make_field("small_integers", b, seed=22))


@pytest.mark.parametrize("h", [0.0, 1.0], ids=["ascent_only", "with_saliency"])
def test_workspace_contract(abi_volumes, h):
    import torch
    from edt import _lib
    lib = _lib.load()
    (a, fa), (b, fb) = abi_volumes
    first, second = abi_case(a, fa, h, 3, False), abi_case(b, fb, h, 2, True)
    ws = fresh_workspace(first.nbytes)
    two_calls(first, ws, "zero fill", "00")
    for pattern in ("ff", "5a", "80", "fltmax"):
        two_calls(first, ws, "pattern fill", pattern)
    # reused: after another operation's call on the same buffer, and after its own call on other labels
    t, out, cnt = upload(b), device_out(b.shape, np.uint32), device_out((3,), np.int64)
    _lib.check(lib.edt_hip_dust_device(vp(t), 2, 3, *EXT, 3, 0, 4, (1 << 63) - 1, 0, vp(out), vp(cnt), vp(ws), ws.numel(), stream()))
    two_calls(first, ws, "after dust")
    two_calls(second, ws, "after its own call on other labels")
    two_calls(first, ws, "and back")
    torch.cuda.synchronize()


@pytest.mark.parametrize("h", [0.0, 1.0], ids=["ascent_only", "with_saliency"])
def test_capture_and_replay(abi_volumes, h):
    (a, fa), _ = abi_volumes
    case = abi_case(a, fa, h, 3, False)
    capture_and_replay(case, fresh_workspace(case.nbytes))


def test_offset_pointers_and_a_misaligned_workspace(abi_volumes):
    """labels, field and out at the alignment of their element and nothing more, each in turn; the workspace at base + 4 refused"""
    import torch
    from edt import _lib
    lib = _lib.load()
    (a, fa), _ = abi_volumes
    voxels = a.size
    want = oracle.watershed(a, fa, 1.0, 3, False, return_N=True)          # (the same labels at every width)
    for which in ("labels", "field", "out", "all"):
        for dtype in (np.uint32, np.uint8, np.uint64):
            lab = a.astype(dtype)
            size = np.dtype(dtype).itemsize
            off = {k: (1 if which in (k, "all") else 0) for k in ("labels", "field", "out")}
            big_l = upload(np.concatenate([np.zeros(off["labels"], dtype), lab.reshape(-1)]))
            big_f = upload(np.concatenate([np.full(off["field"], np.nan, np.float32), fa.reshape(-1)]))
            big_o = device_out((voxels + off["out"] + 1,), np.uint32)
            lt, ft, ot = big_l[off["labels"]:], big_f[off["field"]:], big_o[off["out"]:off["out"] + voxels]
            assert lt.data_ptr() % size == 0 and ft.data_ptr() % 4 == 0 and ot.data_ptr() % 4 == 0
            case = abi_case(lab, fa, 1.0, 3, False, out=ot.view(a.shape), labels_t=lt, field_t=ft, want=want)
            ws = fresh_workspace(case.nbytes)
            fill(ws, "5a")
            before = big_o.cpu().numpy().copy()
            case.call(ws)
            case.check((which, dtype.__name__))
            after = big_o.cpu().numpy()
            assert np.array_equal(after[:off["out"]], before[:off["out"]]) and after[-1] == before[-1]   # nothing written around the view
    case = abi_case(a, fa, 1.0, 3, False, want=want)
    ws = fresh_workspace(case.nbytes + 256)
    n = device_out((1,), np.int64)
    rc = lib.edt_hip_watershed_device(vp(case.outputs[0]), 2, 3, *EXT, vp(upload(fa)), 3, 0, 1.0, vp(case.outputs[0]), vp(n),
                                      ctypes.c_void_p(ws.data_ptr() + 4), case.nbytes, stream())
    assert rc == BAD_ARG                                       # (out aliasing the labels: refused before the workspace is looked at)
    assert b"alias" in lib.edt_hip_last_error()
    lt = upload(a)
    rc = lib.edt_hip_watershed_device(vp(lt), 2, 3, *EXT, vp(upload(fa)), 3, 0, 1.0, vp(case.outputs[0]), vp(n),
                                      ctypes.c_void_p(ws.data_ptr() + 4), case.nbytes, stream())
    assert rc == BAD_ARG and b"256-byte aligned" in lib.edt_hip_last_error()
    torch.cuda.synchronize()


def test_pass_log_names_the_passes(abi_volumes):
    import torch
    from edt import device
    (a, fa), _ = abi_volumes
    t, f = upload(a), upload(fa)
    device.set_profiling(True)
    try:
        device.watershed(t, f, min_saliency=0.0)
        torch.cuda.synchronize()
        plain = [k for k, _ in device.pass_times()]
        device.watershed(t, f, min_saliency=1.0)
        torch.cuda.synchronize()
        merged = [k for k, _ in device.pass_times()]
    finally:
        device.set_profiling(False)
    assert plain == ["watershed ascend", "watershed flatten", "watershed number", "watershed final"]
    assert merged == ["watershed ascend", "watershed flatten", "watershed peaks", "watershed merge", "watershed flatten",
                      "watershed number", "watershed final"]


# ---- fuzz ---------------------------------------------------------------------------------------------------------------------
def test_seeded_fuzz():
    rng = np.random.default_rng(20240)
    for it in range(200):
        nd = int(rng.integers(1, 4))
        shape = tuple(int(v) for v in rng.integers(1, (400, 40, 14)[nd - 1], size=nd))
        dtype = DTYPES[int(rng.integers(len(DTYPES)))]
        kind = FIELDS[int(rng.integers(len(FIELDS)))]
        c = int(rng.integers(1, nd + 1))
        binary = bool(rng.integers(2))
        aniso = ((1.0, 1.0, 1.0), (6.0, 6.0, 30.0))[int(rng.integers(2))][:nd]
        h = (0.0, 0.5 * min(aniso), 1.0, 1e30, float(np.float32(rng.random() * 4)))[int(rng.integers(5))]
        seed = int(rng.integers(1 << 30))
        args = dict(it=it, shape=shape, dtype=dtype.__name__, field=kind, c=c, binary=binary, anisotropy=aniso, h=h, seed=seed)
        lab = make_labels(shape, dtype, seed, zero_frac=float(rng.random() * 0.6), block=int(rng.integers(1, 7)))
        f = make_field(kind, lab, seed, anisotropy=aniso)
        want, n_want = oracle.watershed(lab, f, h, c, binary, return_N=True)
        got, n = run_device(lab, f, h, c, binary)
        if n != n_want or not np.array_equal(got, want):
            print("watershed fuzz: failing case", args)
        assert n == n_want and np.array_equal(got, want), args
