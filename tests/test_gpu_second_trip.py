"""GPU tier: the second trip of every capped grid.  The streaming kernels of the label operations run a fixed grid and a stride
loop: k_morph_select and k_is_foreground (csrc/edt_morph.hip) 2048 workgroups of 256 threads, four voxels per thread where every
pointer is aligned and one otherwise; k_is_background (csrc/edt_generic.hip), k_fh_mark / k_fh_check / k_fh_fill
(csrc/edt_fillholes.hip) and k_dust_filter (csrc/edt_dust.hip) 8192 workgroups of 256 threads, one voxel per thread.  The other
tiers never hand them more than one trip of that grid, so a wrong second trip -- the induction variable, the wave-uniform loops
whose last wave is partial, the per-thread counters reduced at the end, the tail behind the chunks -- would pass them all.  Every
test here uses the smallest size that gives a full first trip, a partial second trip and a ragged end, compares every bit with the
numpy oracle, and asserts on the oracle's result that the part behind the first trip is not trivial."""
import numpy as np
import pytest

import dust_oracle
import fill_holes_oracle
from synth import bits_of, blocky_labels, offset_out, offset_view, outside_intact
from test_gpu_dust import on_device as dust_on_device
from test_gpu_fill_holes import on_device as fill_on_device
from test_gpu_fill_holes import same_bytes
from test_gpu_morph import CODE, FARTHER, MARK, MODES, WITHIN, lib, ok, palette_line, select_call, select_want, stream, ubits, vp

pytestmark = pytest.mark.gpu

MORPH_TRIP = 2048 * 256                 # threads of the grid of csrc/edt_morph.hip
SWEEP_TRIP = 8192 * 256                 # ... of the sweeps of fill_holes and dust
# (count, element offset of every pointer, voxels of one trip): four voxels per thread and a tail of three behind 768 chunks of a
# second trip; one voxel per thread
FORMS = [(4 * MORPH_TRIP + 3 * 1024 + 3, 0, 4 * MORPH_TRIP), (MORPH_TRIP + 777, 1, MORPH_TRIP)]
CARRIERS = [np.uint8, np.float32, np.uint64]    # 1, 4 and 8 bytes; float32: the sign bit is not part of "!= 0"
GUARD_OUT_MASK, OUT_IS_VALUES = MODES[4], MODES[5]


@pytest.mark.parametrize("dtype", CARRIERS)
def test_select_kernel_past_one_trip_of_the_grid(edt_gpu, dtype):
    """k_morph_select's stride loop `c += step` (chunks of four voxels) and `i += step` (single voxels), and the tail behind the
    chunks: 2 097 152 + 3 * 1024 + 3 voxels on aligned pointers, 524 288 + 777 on odd ones.  Both rules, with guard, out and mask
    in one call and out == values in another; the field ties with R2 on many voxels; nothing is stored outside the outputs
    (select_call)."""
    assert GUARD_OUT_MASK == (True, True, True, False) and OUT_IS_VALUES == (False, True, False, True)
    dt = np.dtype(dtype)
    rng = np.random.default_rng(40 + dt.itemsize)
    r2 = np.float64(4.0)
    levels = np.array([0.0, 1.0, 2.0, 4.0, 4.0, np.nextafter(np.float32(4), np.float32(5)), 5.0, 9.0, np.inf], dtype=np.float32)
    for n, k, trip in FORMS:
        values, guard = palette_line(dt, n, rng), palette_line(dt, n, rng)
        field = levels[rng.integers(0, len(levels), size=n)]
        assert (field[trip:] == 4.0).any()
        for rule in (FARTHER, WITHIN):
            for with_guard in (True, False):
                out, mask = select_want(values, guard if with_guard else None, field, r2, rule)
                behind = ubits(out)[trip:]
                assert mask[trip:].any() and not mask[trip:].all()                         # failures and passes
                assert (behind != 0).any() and (behind[ubits(values)[trip:] != 0] == 0).any()   # labels kept and labels zeroed
            select_call(values, guard, field, r2, rule, GUARD_OUT_MASK, (k, k, k, k), (dt.name, n, k, rule, "guard, out, mask"))
            select_call(values, guard, field, r2, rule, OUT_IS_VALUES, (k, k, k, k), (dt.name, n, k, rule, "out == values"))


@pytest.mark.parametrize("dtype", CARRIERS)
def test_is_foreground_kernel_past_one_trip_of_the_grid(edt_gpu, dtype):
    """k_is_foreground's two loops, at the counts of the select"""
    import torch
    dt = np.dtype(dtype)
    rng = np.random.default_rng(140 + dt.itemsize)
    for n, k, trip in FORMS:
        labels = palette_line(dt, n, rng)
        want = (labels != 0).astype(np.uint8)
        assert want[trip:].any() and not want[trip:].all()
        if dt.kind == "f":
            assert np.isnan(labels[trip:]).any() and (ubits(labels)[trip:] == 1 << (8 * dt.itemsize - 1)).any()    # NaN: 1; -0.0: 0
        lbuf, lview = offset_view(labels, k)
        before = lbuf.clone()
        mbuf, mview = offset_out((n,), np.uint8, k, MARK[1])
        ok(lib().edt_hip_is_foreground_device(vp(lview), CODE[dt.name], vp(mview), n, stream()))
        torch.cuda.synchronize()
        assert np.array_equal(bits_of(mview), want), (dt.name, n, k)
        assert outside_intact(mbuf, k, n, MARK[1]) and torch.equal(lbuf, before), (dt.name, n, k)


# ---- fill_holes and dust --------------------------------------------------------------------------------------------------------
SHAPE = (161, 127, 129)         # C order, 129 voxels of x: 2 637 663 voxels = one trip of 2 097 152, 540 511 more, a last wave of 31
assert SWEEP_TRIP < int(np.prod(SHAPE)) < 2 * SWEEP_TRIP and int(np.prod(SHAPE)) % 64 == 31


def solid_volume():
    """twelve labels in blocks of 16 voxels, a tenth of the blocks background, 2 % of the voxels punched out: pin-holes inside a
    block (one label all around), between two blocks (mixed) and next to the background blocks, most of which reach the boundary"""
    rng = np.random.default_rng(2026)
    lab = blocky_labels(SHAPE, nlabels=12, zero_frac=0.1, block=16, rng=rng).astype(np.uint16)
    lab[rng.random(SHAPE) < 0.02] = 0
    return lab, rng


@pytest.fixture(scope="module")
def solid():
    return solid_volume()[0]


def open_background(bg, connectivity):
    """the background voxels connected to the array's boundary, by scipy.ndimage.label"""
    from scipy import ndimage as ndi
    comp, _ = ndi.label(bg, structure=ndi.generate_binary_structure(bg.ndim, connectivity))
    touching = np.unique(comp[fill_holes_oracle.boundary_mask(bg.shape) & bg])
    return np.isin(comp, touching) & bg


@pytest.mark.parametrize("connectivity, binary", [(1, False), (3, True)])
def test_fill_holes_past_one_trip_of_the_grid(edt_gpu, solid, connectivity, binary):
    """k_is_background, k_fh_mark, k_fh_check (multi-label only) and k_fh_fill on a volume of more than 8192 * 256 voxels whose
    count is no multiple of 64: the uint32 stride loops, the wave-uniform loops of mark and check with a partial last wave, and
    the fill counter that every thread carries over both trips.  Behind memory index 2 097 152 the oracle fills voxels, leaves
    background in mixed cavities (multi-label) and leaves open background."""
    want = fill_holes_oracle.fill_holes(solid, connectivity, binary=binary)
    bg = solid == 0
    still = (bg & (want.out == 0)).reshape(-1)[SWEEP_TRIP:]
    reaches = open_background(bg, connectivity).reshape(-1)[SWEEP_TRIP:]
    assert (bg & (want.out != 0)).reshape(-1)[SWEEP_TRIP:].sum() > 1000          # filled
    assert (still & reaches).sum() > 1000                                         # left 0: open
    if binary:
        assert not (still & ~reaches).any() and want.mixed_cavities == 0
    else:
        assert (still & ~reaches).sum() > 1000 and want.mixed_cavities > 1000    # left 0: a closed cavity between two labels
    got, n = fill_on_device(solid, connectivity, binary)
    assert n == want.n_filled and same_bytes(got, want.out)
    if not binary:
        got, n = edt_gpu.fill_holes(solid, connectivity=connectivity, binary=binary, return_fill_count=True)
        assert n == want.n_filled and same_bytes(got, want.out)


@pytest.mark.parametrize("connectivity, invert", [(1, False), (1, True)])      # (the filter does not see the connectivity)
def test_dust_past_one_trip_of_the_grid(edt_gpu, connectivity, invert):
    """k_dust_filter on the same volume with single-voxel specks in its background blocks: the uint32 stride loop and the three
    counters that every thread carries over both trips.  With (2, 5000) the specks (1 voxel) and the components of several
    blocks go, a block on its own (at most 4096 voxels) stays -- or the other way round under invert; behind memory index
    2 097 152 the oracle removes voxels and keeps voxels."""
    lab, rng = solid_volume()
    bg = lab == 0
    alone = bg.copy()
    for axis in range(3):
        alone &= np.roll(bg, 1, axis=axis) & np.roll(bg, -1, axis=axis)
    lab[alone & (rng.random(SHAPE) < 0.01)] = 7
    threshold = (2, 5000)
    want = dust_oracle.dust(lab, threshold, connectivity, invert=invert)
    fg = (lab != 0).reshape(-1)[SWEEP_TRIP:]
    stays = (want.out != 0).reshape(-1)[SWEEP_TRIP:]
    assert (fg & stays).sum() > 1000 and (fg & ~stays).sum() > 1000
    assert 100 < want.kept < want.components - 100 and want.removed_voxels > 1000
    got, counts = dust_on_device(lab, threshold, connectivity, False, invert)
    assert counts == want[1:] and same_bytes(got, want.out)
    if not invert:
        got, counts = edt_gpu.dust(lab, threshold, connectivity=connectivity, invert=invert, return_counts=True)
        assert tuple(counts) == want[1:] and same_bytes(got, want.out)
