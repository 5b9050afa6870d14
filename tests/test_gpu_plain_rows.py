"""GPU tier: rows without a run start stay out of the X-to-Y index volume (csrc/edt_rowwave.hip: rowflags; csrc/edt_colq16.hip:
q16_plain_quad, q16_indices).

Pass X neither measures nor stores a row in which no label changes -- its 16-bit indices follow from x, sx, the border rule
and whether the label is 0 -- and sets the row's bit in two words per (z, band of 32 rows); pass Y puts the indices back from
those while it fills its tile.  What the index buffer holds in such a row is whatever it held before, so a place of pass Y
that still read the buffer there would not fault: it would return the previous call's values.  Every result here is compared
bit for bit with the oracle and with the library's own output with every row stored (debug bit 0x800000) and on the fp32
kernels (0x8000000); every case first asks the library's host proof (edt_hip_q16_no_refusals) whether both column passes are
on the integer kernel alone, the condition under which the new path runs at all.

Shapes: the smallest that reach the integer kernel on both column axes (sy, sz >= 97, sx % 4 == 0): whole chunks and bands;
lanes past the row's end and a partial last band; 512 with a border (the marked middle column: `redo` reads plain rows); 600
with a border (more than 16 columns beyond 16 bits: the `full_wide` refill reads them)."""
import ctypes

import numpy as np
import pytest

from synth import voronoi_labels

pytestmark = pytest.mark.gpu

OFF, FP32 = 0x800000, 0x8000000
CASES = [((64, 128, 100), (1.0, 1.0, 1.0), False), ((64, 128, 100), (1.0, 1.0, 1.0), True), ((64, 128, 100), (6.0, 6.0, 30.0), True),
         ((68, 100, 97), (1.0, 1.0, 1.0), False), ((68, 100, 97), (1.0, 1.0, 1.0), True), ((68, 100, 97), (6.0, 6.0, 30.0), True),
         ((512, 100, 97), (1.0, 1.0, 1.0), True), ((512, 100, 97), (6.0, 6.0, 30.0), True),
         ((600, 100, 97), (1.0, 1.0, 1.0), True), ((600, 100, 97), (6.0, 6.0, 30.0), True)]


def plain_share(lab):
    """the fraction of rows (along x: axis 0) in which no label changes"""
    return float((lab == lab[:1]).all(axis=0).mean())


def alternating(shape):
    """plain and structured rows side by side inside every band: odd rows carry a second label and a stretch of background,
    even rows are one label from end to end (every fourth of them label 0) -- and so are row 0, row 31 and the last row, the
    rows whose stores leave one iteration late or behind the loop"""
    sx, sy, sz = shape
    lab = np.ones(shape, dtype=np.uint32, order="F")
    lab[:, 4::8, :] = 0
    odd = np.arange(sy) % 2 == 1
    odd[[0, 31, sy - 1]] = False
    lab[sx // 3: sx // 2, odd, :] = 2
    lab[sx - 5: sx - 2, odd, ::3] = 0
    lab[:, 31, :] = 3
    return lab


def striped(shape):
    """every row plain, the label changing from row to row and from slice to slice (label 0 among them): run starts along y
    and z everywhere, none along x"""
    sx, sy, sz = shape
    y, z = np.meshgrid(np.arange(sy), np.arange(sz), indexing="ij")
    return np.asfortranarray(np.broadcast_to(((y * 7 + z * 3) % 6).astype(np.uint32), shape))


def box(shape):
    sx, sy, sz = shape
    lab = np.zeros(shape, dtype=np.uint32, order="F")
    lab[sx // 4: 3 * sx // 4, sy // 4: 3 * sy // 4, sz // 4: 3 * sz // 4] = 1
    return lab


def voronoi_no_plain(shape):
    """a dense segmentation in which every row changes its label behind its first voxel"""
    lab = np.asfortranarray(voronoi_labels(shape, nseeds=40, seed=sum(shape), upsample=4, membrane=0.03))
    lab[0] = lab[1] + 1
    return lab


# name -> (maker, the share of plain rows: None = strictly between 0 and 1)
VOLUMES = {"ones": (lambda s: np.ones(s, dtype=np.uint32, order="F"), 1.0), "zeros": (lambda s: np.zeros(s, dtype=np.uint32, order="F"), 1.0),
           "alternating": (alternating, None), "striped": (striped, 1.0), "box": (box, None), "voronoi": (voronoi_no_plain, 0.0)}


def assert_on_integer_kernel(shape, an, bb):
    from edt import _lib
    lib = _lib.load()
    y, z = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.edt_hip_q16_no_refusals(*shape, *an, 3, int(bb), ctypes.addressof(y), ctypes.addressof(z))
    assert rc == 1 and y.value == 1 and z.value == 1, (shape, an, bb, rc, y.value, z.value)


def check(edt_gpu, oracle_port, lab, an, bb, what):
    from edt import _lib
    lib = _lib.load()
    want = oracle_port.edtsq(lab, an, bb)
    try:
        for mode in (0, OFF, FP32):
            lib.edt_hip_set_debug_mode(mode)
            got = edt_gpu.edtsq(lab, anisotropy=an, black_border=bb)
            assert np.array_equal(got, want), (what, lab.shape, an, bb, hex(mode), int((got != want).sum()))
    finally:
        lib.edt_hip_set_debug_mode(0)


@pytest.mark.parametrize("shape,an,bb", CASES)
def test_plain_rows_against_oracle_and_stored_rows(edt_gpu, oracle_port, shape, an, bb):
    assert_on_integer_kernel(shape, an, bb)
    for name, (make, share) in VOLUMES.items():
        lab = make(shape)
        s = plain_share(lab)
        if share is None:
            assert 0.0 < s < 1.0, (name, s)
        else:
            assert s == share, (name, s)
        check(edt_gpu, oracle_port, lab, an, bb, name)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint64])
def test_plain_rows_other_label_types(edt_gpu, oracle_port, dtype):
    shape = (68, 100, 97)
    for an, bb in (((1.0, 1.0, 1.0), False), ((6.0, 6.0, 30.0), True)):
        assert_on_integer_kernel(shape, an, bb)
        for make in (alternating, striped):
            lab = np.asfortranarray(make(shape).astype(dtype))
            check(edt_gpu, oracle_port, lab, an, bb, np.dtype(dtype).name)


@pytest.mark.parametrize("shape,an,bb", [((68, 100, 97), (1.0, 1.0, 1.0), False), ((512, 100, 97), (6.0, 6.0, 30.0), True),
                                         ((600, 100, 97), (1.0, 1.0, 1.0), True)])
def test_plain_rows_over_a_stale_workspace(edt_gpu, oracle_port, shape, an, bb):
    """One plan, one workspace: a segmentation without a plain row first -- it leaves its indices, and pass Y's results over
    them, in every row --, then volumes whose rows are plain where that one had structure.  A place of pass Y that read the
    index buffer in a plain row would give the first call's values."""
    import torch
    from edt import _lib, device
    assert_on_integer_kernel(shape, an, bb)
    plan = device.Plan(shape, _lib.U32)

    def run(lab):
        t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).cuda()  # z, y, x (x fastest)
        return plan.run(t, an, black_border=bb).cpu().numpy().T

    first = voronoi_no_plain(shape)
    assert plain_share(first) == 0.0
    assert np.array_equal(run(first), oracle_port.edtsq(first, an, bb)), "voronoi"
    for name in ("alternating", "ones", "box", "striped"):
        lab = VOLUMES[name][0](shape)
        assert np.array_equal(run(lab), oracle_port.edtsq(lab, an, bb)), name
