"""label_stats, label_moments and label_topology held to each other through what they share (csrc/edt_labeltable.h: the keys,
the global table, the workgroup's LDS table and its spill, the finish and its order; edt/device.py: the capacity rule, the
retry and the signed order): on the same device tensor the three must give byte-identical ``labels`` and ``counts``, and at the
ABI a ``max_labels`` that is too small must end the same way in all three.

One shape, (3, 17, 130): with every voxel its own label that is 6630 labels -- more than any workgroup's LDS table holds (the
spill into the global table runs), more than 256 entries (the rank kernel runs more than one block and more than one trip of
its inner loop) -- and an x extent that is no multiple of 62 or 64 (partial tiles in the flat walk and in topology's tiles)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (3, 17, 130)
VOXELS = 3 * 17 * 130
U32 = 2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    from edt import _lib
    _lib.load()
    if not torch.cuda.is_available() or _lib.device_count() == 0:
        pytest.fail("the GPU tier needs a HIP device")
    torch.cuda.set_device(0)


def _own_labels():
    """every voxel its own label, 1..6630, shuffled (so the order of the table is not the order of the volume)"""
    return (np.random.default_rng(7).permutation(VOXELS) + 1).reshape(SHAPE)


def _cases():
    own = _own_labels()
    signed = own.astype(np.int32)
    signed.reshape(-1)[::2] *= -1
    f = (own * 0.25).astype(np.float32)
    f.reshape(-1)[5::7] = -0.0
    f.reshape(-1)[3::11] = np.nan
    return {
        "uint32 own labels": own.astype(np.uint32).view(np.int32),   # (a device tensor of 32-bit labels is int32: all positive)
        "int32 half negated": signed,
        "uint16 own labels": own.astype(np.uint16).view(np.int16),   # (below 2^15: the direct table, the one-workgroup scan)
        "float32 with -0.0 and NaN": f,
        "one label": np.full(SHAPE, 9, dtype=np.int32),
    }


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_labels_and_counts_agree(name):
    import torch
    from edt import device
    lab = CASES[name]
    t = torch.from_numpy(lab.copy()).cuda()
    dt = torch.ones(SHAPE, dtype=torch.float32, device="cuda")
    got = [device.label_stats(t, dt), device.label_moments(t), device.label_topology(t)]
    flat = lab.reshape(-1)
    flat = flat[(flat != 0) & (flat == flat)]                         # -0.0 and NaN are background
    keys, counts = np.unique(flat, return_counts=True)
    assert (len(keys) == 1) if name == "one label" else (5000 < len(keys) <= VOXELS)    # (the case is what its name says)
    want = (keys.astype(lab.dtype).tobytes(), counts.astype(np.int64).tobytes())
    for res in got:
        assert res.labels.dtype == t.dtype and res.counts.dtype == torch.int64
        assert (res.labels.cpu().numpy().tobytes(), res.counts.cpu().numpy().tobytes()) == want, (name, type(res).__name__)


def test_too_small_max_labels_ends_the_same_way():
    """6630 labels, room for 100: every one of the three returns EDT_OK and reports more labels than fit (include/edt_hip.h:
    "SOME value greater than max_labels"; how many keys got a slot before the overflow word was seen is not specified)"""
    import torch
    from edt import _lib
    lib = _lib.load()
    cap = 100
    t = torch.from_numpy(CASES["uint32 own labels"].copy()).cuda()
    dt = torch.ones(SHAPE, dtype=torch.float32, device="cuda")
    ext = SHAPE[::-1]
    vp = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device="cuda")  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ops = {
        "stats": ([new(torch.int32, cap), new(torch.int64, cap), new(torch.float32, cap), new(torch.int64, cap),
                   new(torch.int32, cap, 6)], (vp(t), U32, vp(dt), 3, *ext, cap)),
        "moments": ([new(torch.int32, cap), new(torch.int64, cap), new(torch.int64, cap, 9), new(torch.float64, cap, 3),
                     new(torch.float64, cap, 6)], (vp(t), U32, 3, *ext, cap)),
        "topology": ([new(torch.int32, cap), new(torch.int64, cap, 8), new(torch.int64, cap, 8)], (vp(t), U32, 3, *ext, cap)),
    }
    seen = {}
    for op, (cols, head) in ops.items():
        nbytes = int(getattr(lib, f"edt_hip_label_{op}_workspace_bytes")(U32, VOXELS, cap))
        assert nbytes > 0
        ws = new(torch.uint8, nbytes)
        n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        rc = getattr(lib, f"edt_hip_label_{op}_device")(*head, *map(vp, cols), vp(n), vp(ws), nbytes, stream)
        seen[op] = (rc, int(n.item()) > cap)
    assert seen == {op: (0, True) for op in ops}, seen
