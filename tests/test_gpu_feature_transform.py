"""GPU tier of the feature transform and expand_labels (include/edt_hip.h): bit-exact against the numpy oracle of the tie
rule (tests/ft_oracle.py) where the voxel sizes share a quantum, optimal within 2^-20 where they do not, consistent with
edtsq and scipy, and the same through every entry point."""
import ctypes

import numpy as np
import pytest

import ft_oracle
import noquantum_cases as nq
from synth import blocky_labels, palette_labels, voronoi_labels

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64, np.float32, np.float64, bool]
# ABI-order (x, y, z) voxel sizes with a quantum, and their squares in quanta
QUANTUM = {(1.0, 1.0, 1.0): (1, 1, 1), (6.0, 6.0, 30.0): (1, 1, 25), (4.0, 4.0, 40.0): (1, 1, 100),
           (0.5, 0.5, 1.0): (1, 1, 4)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    from edt import _lib
    _lib.load()
    if not torch.cuda.is_available() or _lib.device_count() == 0:
        pytest.fail("the GPU tier needs a HIP device")
    torch.cuda.set_device(0)


def as_dtype(ids, dtype):
    return (ids != 0) if dtype is bool else ids.astype(dtype)


def expected(data, bb, a):
    """scipy-layout features of ``data`` (oracle in ABI-order quanta ``a``), laid out as the library lays it out: x is
    axis 0 of an F-contiguous array -- also of one that is C-contiguous as well, as in every entry point --, the last
    axis otherwise."""
    nd = data.ndim
    if data.flags.f_contiguous:
        lab = data.reshape(data.shape + (1,) * (3 - nd))
        feats, _ = ft_oracle.feature_transform(lab, a, bb, ndim=nd)
        return np.stack([feats[k].reshape(data.shape) for k in range(nd)]).astype(np.int32)
    lab = ft_oracle.x_first(data)
    feats, _ = ft_oracle.feature_transform(lab, a, bb, ndim=nd)
    spatial = lab.shape[:nd]
    return np.stack([feats[nd - 1 - k].reshape(spatial).T for k in range(nd)]).astype(np.int32)


def check(data, w_xyz, bb, a, cache=None):
    """feature_transform(data) equals the oracle; ``w_xyz`` / ``a``: voxel sizes / quanta in ABI order (x first).
    ``cache``: expectations of earlier calls, by layout (volumes whose labels compare alike)."""
    import edt
    nd = data.ndim
    key = (data.shape, bool(data.flags.f_contiguous))
    want = cache.get(key) if cache is not None else None
    if want is None:
        want = expected(data, bb, a)
        if cache is not None:
            cache[key] = want
    an = tuple(w_xyz[:nd]) if data.flags.f_contiguous else tuple(w_xyz[:nd])[::-1]
    got = edt.feature_transform(data, anisotropy=an, black_border=bb)
    assert got.dtype == np.int32 and got.shape == (nd,) + data.shape
    assert np.array_equal(got, want), (data.dtype, data.shape, w_xyz, bb, "F" if data.flags.f_contiguous else "C")
    return want


def run_both_orders(data_c, w_xyz, bb, a, cache=None):
    """the C-ordered volume and the same volume with x as axis 0 (Fortran order)"""
    want = check(data_c, w_xyz, bb, a, cache)
    check(np.asfortranarray(data_c.T), w_xyz, bb, a, cache)
    return want


# ---- 1. bit-exact against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", ["blocky", "voronoi"])
@pytest.mark.parametrize("bb", [False, True])
def test_exact_against_oracle_every_dtype(gen, bb):
    if gen == "blocky":
        ids = blocky_labels((9, 11, 13), nlabels=5, zero_frac=0.2, block=3, rng=np.random.default_rng(5))
    else:
        ids = np.ascontiguousarray(voronoi_labels((13, 11, 9), nseeds=12, seed=3, upsample=2, membrane=0.1).T)
    for w, a in QUANTUM.items():
        cache, cache_bool = {}, {}
        for dt in DTYPES:
            run_both_orders(as_dtype(ids, dt), w, bb, a, cache_bool if dt is bool else cache)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32, np.uint64, np.int64, np.float32, np.float64, bool])
def test_exact_on_full_width_palettes(dtype, oracle_port):
    lab = palette_labels((10, 9, 8), dtype, rng=np.random.default_rng(2))
    for w, a in (((1.0, 1.0, 1.0), (1, 1, 1)), ((6.0, 6.0, 30.0), (1, 1, 25))):
        for bb in (False, True):
            want = run_both_orders(lab, w, bb, a)
            # fl32(D(p, f(p))) is edtsq wherever it is below 2^24
            an = w[::-1]
            ref = oracle_port.edtsq(lab, an, bb)
            grids = np.stack(np.meshgrid(*[np.arange(s) for s in lab.shape], indexing="ij"))
            w2 = np.array(an, dtype=np.float64) ** 2
            d = sum(w2[k] * (grids[k] - want[k]).astype(np.float64) ** 2 for k in range(3))
            has = ~np.all(want == -1, axis=0)
            d32 = np.where(has, d, np.inf).astype(np.float32)
            small = (ref < 2.0 ** 24) & (d32 < 2.0 ** 24)
            assert np.array_equal(d32[small], ref[small]), dtype


@pytest.mark.parametrize("length", [1, 2, 31, 32, 33, 63, 64, 65, 127, 1025])
def test_exact_axis_lengths_1d_2d_3d(length):
    rng = np.random.default_rng(length)
    # (C order: the last axis is x -- (4, 2, length) has rows of `length` voxels through the non-final pass X and y = 2,
    # (length, 3, 4) and (3, length, 2) put `length` on z and y)
    for shape in ((length,), (length, 5), (5, length), (length, 3, 4), (3, length, 2), (4, 2, length)):
        ids = blocky_labels(shape, nlabels=4, zero_frac=0.25, block=3, rng=rng).astype(np.uint32)
        for w, a in (((1.0, 1.0, 1.0), (1, 1, 1)), ((6.0, 6.0, 30.0), (1, 1, 25))):
            for bb in (False, True):
                run_both_orders(ids, w, bb, a)


def test_edge_cases():
    import edt
    # one label everywhere: no feature without a border; with one, every feature lies on the shell
    one = np.full((6, 7, 8), 3, dtype=np.uint16)
    assert np.all(edt.feature_transform(one) == -1)
    f = edt.feature_transform(one, black_border=True)
    run_both_orders(one, (1.0, 1.0, 1.0), True, (1, 1, 1))
    assert f.min() == -1
    # a single background voxel: everything points at it
    single = np.ones((5, 6, 7), dtype=np.uint8)
    single[2, 3, 4] = 0
    f = edt.feature_transform(single)
    assert np.all(f[0] == 2) and np.all(f[1] == 3) and np.all(f[2] == 4)
    # rows and columns without any boundary (stripes along every axis), and background-only volumes
    for ax in range(3):
        s = np.ones((6, 5, 4), dtype=np.uint32)
        idx = [slice(None)] * 3
        idx[ax] = slice(0, 1)
        s[tuple(idx)] = 2
        for bb in (False, True):
            run_both_orders(s, (1.0, 1.0, 1.0), bb, (1, 1, 1))
    zero = np.zeros((3, 4, 5), dtype=np.float32)
    zero[1, 1, 1] = -0.0
    f = edt.feature_transform(zero)
    grids = np.stack(np.meshgrid(*[np.arange(s) for s in zero.shape], indexing="ij"))
    assert np.array_equal(f, grids)


# ---- 2. no quantum ------------------------------------------------------------------------------------------------
def brute_d(lab_xyz, w, bb):
    lab = lab_xyz
    if bb:
        pad = np.zeros(tuple(s + 2 for s in lab.shape), dtype=lab.dtype)
        pad[1:-1, 1:-1, 1:-1] = lab
        off = 1
    else:
        pad, off = lab, 0
    coords = np.stack(np.meshgrid(*[np.arange(s) - off for s in pad.shape], indexing="ij"), -1).reshape(-1, 3)
    flat = pad.reshape(-1)
    w2 = np.array(w, dtype=np.float64) ** 2
    out = np.zeros(lab.shape)
    for idx in np.ndindex(lab.shape):
        if lab[idx] == 0:
            continue
        other = ~(flat == lab[idx]) & ~np.all(coords == np.array(idx), axis=1)
        out[idx] = (((coords[other] - np.array(idx)) ** 2) * w2).sum(1).min() if other.any() else np.inf
    return out


@pytest.mark.parametrize("w", [(3.58, 3.58, 40.0), (1.1, 0.7, 2.3)])
@pytest.mark.parametrize("bb", [False, True])
def test_no_quantum_optimal_and_deterministic(w, bb):
    import edt
    ids = blocky_labels((7, 8, 9), nlabels=4, zero_frac=0.2, block=2, rng=np.random.default_rng(7)).astype(np.uint32)
    data_f = np.asfortranarray(ids)  # x = axis 0: ABI order
    f1 = edt.feature_transform(data_f, anisotropy=w, black_border=bb)
    f2 = edt.feature_transform(data_f, anisotropy=w, black_border=bb)
    assert np.array_equal(f1, f2)
    w32 = np.array(w, dtype=np.float32).astype(np.float64)
    best = brute_d(ids, w32, bb)
    grids = np.stack(np.meshgrid(*[np.arange(s) for s in ids.shape], indexing="ij"))
    d = sum(w32[k] ** 2 * (grids[k] - f1[k]).astype(np.float64) ** 2 for k in range(3))
    fg = ids != 0
    assert np.all(d[fg] <= best[fg] * (1.0 + 2.0 ** -20))
    assert np.all(d[fg] >= best[fg] * (1.0 - 2.0 ** -20))
    assert np.array_equal(f1[:, ~fg], grids[:, ~fg])
    # a feature inside the volume carries another label; one outside lies on the border shell (one component off)
    inside = np.all((f1 >= 0) & (f1 < np.array(ids.shape).reshape(3, 1, 1, 1)), axis=0)
    pts = fg & inside
    assert not np.any(ids[tuple(f1[:, pts])] == ids[pts])
    if bb:
        off = ((f1 == -1) | (f1 == np.array(ids.shape).reshape(3, 1, 1, 1))).sum(0)
        assert np.all(off[fg & ~inside] == 1)
    else:
        assert np.all(inside[fg])


# ---- 3. scipy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", [(1, 1, 1), (30, 6, 6), (2, 3, 5)])
def test_binary_masks_against_scipy(sampling):
    import edt
    from scipy import ndimage
    rng = np.random.default_rng(11)
    mask = (rng.random((24, 31, 29)) < 0.97).astype(np.uint8)
    _, ind = ndimage.distance_transform_edt(mask, sampling=sampling, return_indices=True)
    ours = edt.feature_transform(mask, anisotropy=sampling)
    grids = np.stack(np.meshgrid(*[np.arange(s) for s in mask.shape], indexing="ij"))
    w2 = np.array(sampling, dtype=np.int64) ** 2
    d_ours = sum(w2[k] * (grids[k] - ours[k]).astype(np.int64) ** 2 for k in range(3))
    d_scipy = sum(w2[k] * (grids[k] - ind[k]).astype(np.int64) ** 2 for k in range(3))
    assert np.array_equal(d_ours, d_scipy)


# ---- 4. consistency with edtsq at 512^3 -----------------------------------------------------------------------------
def test_consistent_with_edtsq_at_512():
    import torch
    from edt import device
    lab = voronoi_labels((512, 512, 512), nseeds=2000, seed=0, upsample=4)  # (x, y, z), Fortran
    t = torch.from_numpy(np.ascontiguousarray(lab.T)).cuda()               # (z, y, x)
    an = (30.0, 6.0, 6.0)
    f = device.feature_transform(t, anisotropy=an)
    sq = device.edtsq(t, anisotropy=an)
    d = torch.zeros(t.shape, dtype=torch.float64, device=t.device)
    for k, n in enumerate(t.shape):
        shape = [1, 1, 1]
        shape[k] = n
        coord = torch.arange(n, device=t.device, dtype=torch.float64).view(shape)
        d += an[k] ** 2 * (coord - f[k].double()) ** 2
    del f
    d32 = d.float()
    both = (d32 < 2.0 ** 24) & (sq < 2.0 ** 24)
    assert bool(torch.equal(d32[both], sq[both]))
    rel = (d - sq.double()).abs() <= sq.double() * 2.0 ** -20
    assert bool(rel.all())


# ---- 5. generic vs the default kernel, long axes -------------------------------------------------------------------
def test_force_generic_and_long_axes():
    import torch
    from edt import device
    ids = blocky_labels((40, 70, 66), nlabels=5, zero_frac=0.2, block=3, rng=np.random.default_rng(1)).astype(np.int32)
    t = torch.from_numpy(ids).cuda()
    # (the flag is accepted and must not change the features; every axis length runs on the size-agnostic column kernel
    # today, so this pins the contract for a tiled form that serves the short axes)
    for bb in (False, True):
        assert torch.equal(device.feature_transform(t, (6.0, 6.0, 30.0), bb),
                           device.feature_transform(t, (6.0, 6.0, 30.0), bb, force_generic=True))
    for shape in ((32800, 3), (33000, 2, 2)):
        ids = blocky_labels(shape, nlabels=3, zero_frac=0.3, block=5, rng=np.random.default_rng(2)).astype(np.uint16)
        for bb in (False, True):
            run_both_orders(ids, (1.0, 1.0, 1.0), bb, (1, 1, 1))


# ---- 6. entry points agree ------------------------------------------------------------------------------------------
def test_host_device_and_return_distances_agree():
    import torch
    import edt
    from edt import device
    lab = voronoi_labels((60, 50, 40), nseeds=40, seed=4, upsample=2, membrane=0.05)
    data_c = np.ascontiguousarray(lab.T)
    for an, bb in (((30.0, 6.0, 6.0), False), ((40.0, 4.0, 4.0), True), ((2.3, 0.7, 1.1), False)):
        host, dist = edt.feature_transform(data_c, anisotropy=an, black_border=bb, return_distances=True)
        dev = device.feature_transform(torch.from_numpy(data_c).cuda(), anisotropy=an, black_border=bb).cpu().numpy()
        assert np.array_equal(host, dev)
        assert np.array_equal(dist, edt.edt(data_c, anisotropy=an, black_border=bb))


# ---- 7. expand_labels -------------------------------------------------------------------------------------------------
def expand_reference(labels, distance, an):
    """The definition (include/edt_hip.h) built from feature_transform(labels == 0)."""
    import edt
    f = edt.feature_transform((labels == 0).astype(np.uint8), anisotropy=an)
    nd = labels.ndim
    grids = np.stack(np.meshgrid(*[np.arange(s) for s in labels.shape], indexing="ij"))
    # D in fp64, terms added in ABI order x, y, z: array axes from the last one
    w2 = [np.float64(np.float32(a)) * np.float64(np.float32(a)) for a in an]
    D = np.zeros(labels.shape)
    for k in range(nd - 1, -1, -1):
        D = D + w2[k] * ((grids[k] - f[k]).astype(np.int64) ** 2).astype(np.float64)
    has = ~np.all(f == -1, axis=0)
    out = labels.copy()
    take = (labels == 0) & has & (D <= np.float64(distance) * np.float64(distance))
    src = tuple(np.where(take, f[k], 0) for k in range(nd))
    out[take] = labels[src][take]
    return out, f, D, take


@pytest.mark.parametrize("dtype", [np.uint8, np.uint32, np.int64, np.float32, np.float64])
@pytest.mark.parametrize("distance", [0.0, 1.0, 2.5, np.inf])
def test_expand_labels(dtype, distance):
    import torch
    import edt
    from edt import device
    from scipy import ndimage
    lab = voronoi_labels((30, 26, 22), nseeds=15, seed=2, upsample=2, membrane=0.3).T.astype(dtype)
    lab = np.ascontiguousarray(lab)
    for an in ((1.0, 1.0, 1.0), (3.0, 1.0, 2.0), (2.3, 0.7, 1.1)):
        want, f, D, take = expand_reference(lab, distance, an)
        got = edt.expand_labels(lab, distance=distance, anisotropy=an)
        assert got.dtype == lab.dtype and got.shape == lab.shape
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (an, distance)
        got_f = edt.expand_labels(np.asfortranarray(lab.T), distance=distance, anisotropy=an[::-1])
        assert got_f.flags.f_contiguous and np.array_equal(got_f.T.view(np.uint8), got.view(np.uint8))
        dev = device.expand_labels(torch.from_numpy(lab).cuda(), distance=distance, anisotropy=an).cpu().numpy()
        assert np.array_equal(dev.view(np.uint8), got.view(np.uint8))
        if an != (2.3, 0.7, 1.1):  # integer sizes: each filled voxel took a nearest foreground voxel's label
            dt = ndimage.distance_transform_edt(lab == 0, sampling=an)
            assert np.array_equal(D[take], (dt[take].astype(np.float64) ** 2).round())
        else:  # no quantum: the reference above rests on the library's own transform, so hold the result to scipy's minimum
            assert nq.undecided(lab.T, distance, an[::-1]) == 0       # (a condition on the data: x first)
            assert nq.check_expand(lab.T, got.T, distance, an[::-1]) == 0
    assert np.array_equal(edt.expand_labels(np.zeros_like(lab), distance=distance), np.zeros_like(lab))
    full = np.ones_like(lab)
    assert np.array_equal(edt.expand_labels(full, distance=distance), full)


def test_expand_labels_1d_2d():
    import edt
    lab = np.array([0, 0, 3, 0, 0, 0, 5, 0], dtype=np.uint16)
    assert edt.expand_labels(lab, 1).tolist() == [0, 3, 3, 3, 0, 5, 5, 5]
    assert edt.expand_labels(lab, 2).tolist() == [3, 3, 3, 3, 3, 5, 5, 5]
    img = np.ascontiguousarray(voronoi_labels((40, 33), nseeds=8, seed=1, upsample=2, membrane=0.3).T)
    for d in (1.0, 3.0):
        want, *_ = expand_reference(img, d, (2.0, 1.0))
        assert np.array_equal(edt.expand_labels(img, d, anisotropy=(2.0, 1.0)), want)


# ---- 8. past 2^31 voxels ----------------------------------------------------------------------------------------------
def test_past_2_31_voxels():
    import torch
    from edt import device
    torch.cuda.empty_cache()
    t = torch.ones((2049, 1024, 1024), dtype=torch.uint8, device="cuda")
    t[0] = 0
    f = device.feature_transform(t)  # tensor order: (z, y, x) -> expected (0, y, x)
    del t
    assert bool((f[0] == 0).all())
    assert bool((f[1] == torch.arange(1024, device="cuda", dtype=torch.int32).view(1, 1024, 1)).all())
    assert bool((f[2] == torch.arange(1024, device="cuda", dtype=torch.int32).view(1, 1, 1024)).all())
    del f
    torch.cuda.empty_cache()
