"""GPU tier of the fp64 instantiation of the feature transform (csrc/edt_feature.hip: k_ft_rows / k_ft_cols with V = double),
which serves the voxel sizes the library finds no quantum for, and of what is built on it there: expand_labels / dilate, closing
and medial_axis.

Two kinds of sizes (tests/noquantum_cases.py): on EXACT ones every value the kernels form is exact in fp64, so the output is held
bit for bit to the int64 tie rule of tests/ft_oracle.py with ft_oracle.exact_factors; on INEXACT ones the header's contract is
checked against scipy's per-label minimum (check_features, check_expand), and the 1-D transform, which decides by integer
compares alone, bit for bit.  The only tolerances are the header's 2^-20 and the 2^-48 derived for the checker's own fp64 sums.

Extents: x in 1, 2, 63, 64, 65, 129, 1030 (k_ft_rows takes 64-lane steps with carries between them), columns of 1, 2, 3, 64, 65,
300 and 1025 rows, and per column pass a volume with more than 256 columns, no multiple of 256 (a second, partial workgroup of
k_ft_cols).  Every volume that goes through the pure-Python oracle stays at or below 16 000 voxels.  A C-ordered array and the
F-ordered array of its transpose are the same memory and the same ABI call: the oracle runs once, on the x-first volume."""
import numpy as np
import pytest

import ft_oracle
import medial_oracle
import morph_oracle
import noquantum_cases as nq
from synth import blocky_labels, palette_labels, voronoi_labels
from test_gpu_feature_transform import DTYPES, as_dtype

pytestmark = pytest.mark.gpu

EXACT = list(nq.EXACT)
ORACLE_CAP = 16000
_SIGNED_VIEW = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    from edt import _lib
    _lib.load()
    if not torch.cuda.is_available() or _lib.device_count() == 0:
        pytest.fail("the GPU tier needs a HIP device")
    torch.cuda.set_device(0)


def to_device(a):
    """a numpy array as a device tensor of the same bits (unsigned 16/32/64-bit labels as the signed type of their width)"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED_VIEW[a.dtype]) if a.dtype in _SIGNED_VIEW else a).cuda()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes(order="C") == b.tobytes(order="C")


def layouts(xyz):
    """the x-first volume as an F-ordered array and, where that is a different array, as the C-ordered one of the same memory:
    (data, own) with ``own`` mapping an x-first result onto the array's axes.  (An array that is contiguous both ways -- 1-D, or
    unit extents -- is taken in F order by every entry point: its transpose is another problem, not another layout.)"""
    data_f = np.asfortranarray(xyz)
    yield data_f, (lambda v: v)
    data_c = np.ascontiguousarray(xyz.T)
    if not data_c.flags.f_contiguous:
        yield data_c, (lambda v: v.T)


def an_of(data, w_xyz):
    w = tuple(w_xyz[:data.ndim])
    return w if data.flags.f_contiguous else w[::-1]


def through_both(name, data, w_xyz, *args, **kw):
    """edt.<name> on the host array and edt.device.<name> on the same memory, both in the array's own axes; they must be equal
    bit for bit.  Returns the host module's result (a tuple stays a tuple)."""
    import edt
    from edt import device
    nd = data.ndim
    an = an_of(data, w_xyz)
    host = getattr(edt, name)(data, *args, anisotropy=an, **kw)
    fortran = data.flags.f_contiguous
    mem, an_mem = (data.T, an[::-1]) if fortran else (data, an)
    dev = getattr(device, name)(to_device(mem), *args, anisotropy=an_mem, **kw)

    def back(t, like):
        a = t.cpu().numpy()
        a = a.view(like.dtype) if a.dtype != like.dtype and a.dtype.itemsize == like.dtype.itemsize else a
        if name == "feature_transform":
            return np.stack([a[nd - 1 - k].T for k in range(nd)]) if fortran else a
        return a.T if fortran else a

    hs, ds = (host, dev) if isinstance(host, tuple) else ((host,), (dev,))
    assert len(hs) == len(ds)
    for h, d in zip(hs, ds):
        assert same_bits(h, back(d, h)), (name, data.shape, data.dtype, w_xyz, "host and device forms differ")
    return host


def oracle_features(xyz, w_xyz, bb):
    """(ndim, ...) int32 features of the x-first volume by the int64 tie rule on the sizes' exact factors"""
    nd = xyz.ndim
    assert xyz.size <= ORACLE_CAP
    a = ft_oracle.exact_factors(w_xyz[:nd]) + (1,) * (3 - nd)
    feats, _ = ft_oracle.feature_transform(xyz.reshape(xyz.shape + (1,) * (3 - nd)), a, bb, ndim=nd)
    return np.stack([feats[k].reshape(xyz.shape) for k in range(nd)]).astype(np.int32)


def own_features(want, data):
    """x-first features (ndim, ...) in the layout of the array ``data``: component k along array axis k"""
    nd = want.shape[0]
    return want if data.flags.f_contiguous else np.stack([want[nd - 1 - k].T for k in range(nd)])


def exact(xyz, w_xyz, bb, want=None):
    """feature_transform of the x-first volume in every layout and through both entry points equals the oracle, bit for bit"""
    if want is None:
        want = oracle_features(xyz, w_xyz, bb)
    for data, own in layouts(xyz):
        got = through_both("feature_transform", data, w_xyz, black_border=bb)
        assert got.dtype == np.int32 and got.shape == (data.ndim,) + data.shape
        bad = int(np.count_nonzero(got != own_features(want, data)))
        assert bad == 0, (bad, data.dtype, data.shape, w_xyz, bb, "F" if data.flags.f_contiguous else "C")
    return want


def cuts(vol):
    """the x-first volume and its 2-D and 1-D cuts"""
    return [vol, vol[:, :, 0], vol[:, 0, 0]]


# ---- 1. EXACT sizes: bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", ["blocky", "voronoi"])
@pytest.mark.parametrize("bb", [False, True])
def test_exact_every_dtype(gen, bb):
    if gen == "blocky":
        ids = blocky_labels((13, 11, 9), nlabels=5, zero_frac=0.2, block=3, rng=np.random.default_rng(5))
    else:
        ids = np.asarray(voronoi_labels((13, 11, 9), nseeds=12, seed=3, upsample=2, membrane=0.1))
    for w in EXACT:
        for vol in cuts(ids):
            want = want_bool = None
            for dt in DTYPES:
                if dt is bool:
                    want_bool = exact(as_dtype(vol, dt), w, bb, want_bool)
                else:
                    want = exact(as_dtype(vol, dt), w, bb, want)


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.uint32, np.int32, np.uint64, np.int64, np.float32, np.float64])
def test_exact_on_full_width_palettes(dtype):
    lab = np.ascontiguousarray(palette_labels((10, 9, 8), dtype, rng=np.random.default_rng(2)))
    for w in EXACT:
        for bb in (False, True):
            for vol in cuts(lab)[:2]:
                exact(vol, w, bb)


AXIS_LENGTHS = [1, 2, 3, 63, 64, 65, 129, 300, 1025, 1030]


@pytest.mark.parametrize("length", AXIS_LENGTHS)
def test_exact_axis_lengths_1d_2d_3d(length):
    """`length` on x, on y and on z, in 1-D, 2-D and 3-D; the sizes go round the table with the shape (two per shape, one per shape
    from 300 rows on: the oracle is the slow side)"""
    rng = np.random.default_rng(length)
    turn = AXIS_LENGTHS.index(length)
    # x first: (length, 2, 4) has rows of `length` voxels through the non-final pass X, (3, length, 2) columns of `length` rows
    # in the non-final pass Y, (5, length) in the final one, (4, 3, length) in pass Z
    for k, shape in enumerate(((length,), (length, 5), (5, length), (length, 2, 4), (3, length, 2), (4, 3, length))):
        ids = blocky_labels(shape, nlabels=4, zero_frac=0.25, block=3, rng=rng).astype(np.uint32)
        for j in range(1 if length >= 300 else 2):
            w = EXACT[(turn + 2 * k + 3 * j) % len(EXACT)]
            for bb in (False, True):
                exact(ids, w, bb)


@pytest.mark.parametrize("shape", [(129, 40, 3), (65, 5, 49), (300, 53), (2, 130, 61)])
@pytest.mark.parametrize("bb", [False, True])
def test_exact_past_one_workgroup_of_columns(shape, bb):
    """more than 256 columns and no multiple of 256: (129, 40, 3) has 387 columns in pass Y, (65, 5, 49) 325 in pass Z, (300, 53)
    300 in the final pass Y, (2, 130, 61) 260 in pass Z with two voxels of x: neighbouring lanes on different columns of y"""
    cols = [shape[0] * int(np.prod(shape[2:])), shape[0] * shape[1]][:len(shape) - 1]
    assert any(c > 256 and c % 256 for c in cols)
    k = len(shape) + shape[0]
    for j, gen in enumerate(("blocky", "voronoi")):
        if gen == "blocky":
            ids = blocky_labels(shape, nlabels=4, zero_frac=0.2, block=4, rng=np.random.default_rng(k)).astype(np.uint16)
        else:
            ids = np.asarray(voronoi_labels(shape, nseeds=9, seed=k, upsample=3, membrane=0.05)).astype(np.uint16)
        exact(ids, EXACT[(k + 3 * j + bb) % len(EXACT)], bb)


@pytest.mark.parametrize("w", EXACT)
def test_exact_structures_that_stress_the_hull(w):
    shape = (6, 7, 8)
    grids = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"))
    # one label throughout: border sites only; -1 without a border
    one = np.full(shape, 3, dtype=np.uint16)
    for vol in cuts(one):
        assert np.all(exact(vol, w, False) == -1)
        assert exact(vol, w, True).min() == -1
    # a single background voxel: everything points at it
    single = np.ones((5, 6, 7), dtype=np.uint8)
    single[2, 3, 4] = 0
    f = exact(single, w, False)
    assert np.all(f[0] == 2) and np.all(f[1] == 3) and np.all(f[2] == 4)
    exact(single, w, True)
    # stripes along each axis: rows and columns without any finite candidate
    for ax in range(3):
        s = np.ones((6, 5, 4), dtype=np.uint32)
        idx = [slice(None)] * 3
        idx[ax] = slice(0, 1)
        s[tuple(idx)] = 2
        for bb in (False, True):
            exact(s, w, bb)
            if ax < 2:
                exact(s[:, :, 0], w, bb)
    # background only (with a -0.0)
    zero = np.zeros((3, 4, 5), dtype=np.float32)
    zero[1, 1, 1] = -0.0
    for bb in (False, True):
        assert np.array_equal(exact(zero, w, bb), np.stack(np.meshgrid(*[np.arange(s) for s in zero.shape], indexing="ij")))
    # a checkerboard of two labels: every voxel is a run of its own
    board = (1 + grids.sum(0) % 2).astype(np.int64)
    for bb in (False, True):
        for vol in cuts(board):
            exact(vol, w, bb)


def near_tie(w_first, w_second, reach):
    """Two candidate offsets ``(d1, d2)`` -- d1 along the axis of the earlier pass, of size ``w_first``, d2 along the next one --
    whose exact squared distances are N1 < N2 and which an evaluation that rounds the earlier pass's product w^2 d^2 to fp32
    orders the other way round or cannot tell apart (a tie goes to the smaller row); None if there is no such pair within
    ``reach``.  Exact arithmetic separates them by a few quanta, 2^-24 of their size does not."""
    a = ft_oracle.exact_factors((w_first, w_second))
    d1, d2 = [v.ravel() for v in np.meshgrid(np.arange(reach[0] + 1), np.arange(reach[1] + 1), indexing="ij")]
    N = a[0] * d1 ** 2 + a[1] * d2 ** 2
    sq1, sq2 = nq.squares((w_first, w_second))
    rounded = (np.float32(sq1) * (d1 ** 2).astype(np.float32)).astype(np.float64) + sq2 * (d2 ** 2).astype(np.float64)
    assert np.float64(np.float32(sq1)) == sq1
    order = np.argsort(N, kind="stable")
    for gap in range(1, 9):
        i, j = order[:-gap], order[gap:]
        hit = np.nonzero((N[i] < N[j]) & (rounded[i] >= rounded[j]) & (d1[i] != d1[j]) & (d2[i] != d2[j]))[0]
        if len(hit):
            k = hit[0]
            return (int(d1[i[k]]), int(d2[i[k]])), (int(d1[j[k]]), int(d2[j[k]]))
    return None


# (the sizes of EXACT whose first or second square is no power of two times a small integer: 1 + 2^-7 and 1 + 2^-8.  The factor
# 16641 of 129 rounds too, but its near ties need a column of a thousand rows next to a row of a hundred voxels: past the cap.)
@pytest.mark.parametrize("w, form", [((1.0, 1.0078125, 1.0), "yz"), ((1.0078125, 1.0, 1.00390625), "xy"),
                                     ((0.75, 1.00390625, 1.0078125), "yz")])
def test_exact_near_ties_that_fp32_products_would_decide_otherwise(w, form):
    """One label with two background voxels A and B, B in the smaller row, and a voxel p that is nearer to A by a few quanta of
    some 10^7: pass values formed in fp32 (24 bits) would hand p to B.  "xy": a 2-D volume, pass X hands its values to the final pass Y; "yz": a volume
    of one voxel in x, the non-final pass Y hands its values to pass Z."""
    assert w in nq.EXACT
    reach = (64, 59)
    first, second = (w[0], w[1]) if form == "xy" else (w[1], w[2])
    found = near_tie(first, second, reach)
    assert found is not None
    (a1, a2), (b1, b2) = found
    vol = np.ones((2 * reach[0] + 2, 2 * reach[1] + 2), dtype=np.uint8)
    p = reach
    vol[p[0] + a1, p[1] + a2] = 0
    vol[p[0] - b1, p[1] - b2] = 0
    if form == "yz":
        vol = vol[None]
    want = exact(vol, w, False)
    at = (slice(None),) + ((0,) if form == "yz" else ()) + p
    assert tuple(want[at][-2:]) == (p[0] + a1, p[1] + a2)


# ---- 2. INEXACT sizes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 64, 65, 1030])
def test_inexact_1d_bit_for_bit(length):
    """pass X decides by integer compares alone: whatever the voxel size, the 1-D features are the tie rule's"""
    rng = np.random.default_rng(length)
    ids = blocky_labels((length,), nlabels=3, zero_frac=0.25, block=3, rng=rng)
    for w in nq.INEXACT:
        for dt in (np.uint32, np.float64, bool):
            vol = as_dtype(ids, dt)
            for bb in (False, True):
                feats, _ = ft_oracle.feature_transform(vol.reshape(length, 1, 1), (1, 1, 1), bb, ndim=1)
                want = feats[:1].reshape(1, length).astype(np.int32)
                got = through_both("feature_transform", vol, w, black_border=bb)
                assert np.array_equal(got, want), (w, dt, bb)
                nq.check_features(vol.reshape(length, 1, 1), got, w, bb, 1)


PROPERTY_SHAPES = [(130, 70, 40), (1030, 9, 7), (9, 300, 5), (5, 7, 1025), (130, 70), (1030, 9)]
PROPERTY_DTYPES = [np.uint8, np.uint32, np.float32, bool]


@pytest.mark.parametrize("gen", ["blocky", "voronoi"])
@pytest.mark.parametrize("shape", PROPERTY_SHAPES)
def test_inexact_properties(shape, gen):
    """the header's contract against scipy's per-label minimum; every size of INEXACT, the border and the dtype going round with
    the size, the shape and the generator (the reference is the slow side: the extents stay, the grid is cut)"""
    s, g = PROPERTY_SHAPES.index(shape), ("blocky", "voronoi").index(gen)
    nd = len(shape)
    if gen == "blocky":
        ids = blocky_labels(shape, nlabels=3 + (s + g) % 4, zero_frac=0.15, block=5 + s, rng=np.random.default_rng(s))
    else:
        ids = np.asarray(voronoi_labels(shape, nseeds=3 + (s + 2 * g) % 4, seed=s, upsample=4, membrane=0.04)).astype(np.int64)
    assert 3 <= len(np.unique(ids[ids != 0])) <= 6
    for i, w in enumerate(nq.INEXACT):
        bb = bool((i + s + g) % 2)
        vol = as_dtype(ids, PROPERTY_DTYPES[(i + s + 2 * g) % 4])
        first = None
        for data, own in layouts(vol):
            got = through_both("feature_transform", data, w, black_border=bb)
            again = through_both("feature_transform", data, w, black_border=bb)
            assert np.array_equal(got, again)
            lab, feat = nq.to_xyz(data, got)
            if first is None:
                first = feat
                nq.check_features(lab, feat, w[:nd], bb, nd)
            else:
                assert np.array_equal(feat, first)        # (the same memory: the same features)


# ---- 3. the compositions on EXACT sizes, bit for bit ------------------------------------------------------------------------
COMPOSITION_DTYPES = [np.uint8, np.uint32, np.int64, np.float32, np.float64, np.uint16, bool]


def composition_volumes(k):
    lab = np.asarray(voronoi_labels((24, 20, 18), nseeds=15, seed=2 + k, upsample=2, membrane=0.3))
    return [as_dtype(v, COMPOSITION_DTYPES[(k + j) % len(COMPOSITION_DTYPES)]) for j, v in enumerate(cuts(lab))]


@pytest.mark.parametrize("w", EXACT)
def test_expand_dilate_closing_on_exact_sizes(w):
    k = EXACT.index(w)
    for vol in composition_volumes(k):
        nd = vol.ndim
        step = min(w[:nd])
        data_f = np.asfortranarray(vol)
        for distance in (0.0, step, 2.5 * step, np.inf):
            grown = morph_oracle.expand_labels(data_f, distance, w[:nd])
            closed = None if distance == np.inf else morph_oracle.closing(data_f, distance, w[:nd])
            for data, own in layouts(vol):
                for name in ("expand_labels", "dilate"):
                    got = through_both(name, data, w, distance)
                    assert same_bits(got, own(grown)) and got.flags.f_contiguous == data.flags.f_contiguous, (name, w, distance)
                if closed is not None:
                    assert same_bits(through_both("closing", data, w, distance), own(closed)), (w, distance)
        if (vol == 0).any() and (vol != 0).any():       # (the last distance is +inf: every background voxel was filled)
            assert not (grown == 0).any()


@pytest.mark.parametrize("w", EXACT)
def test_medial_axis_on_exact_sizes(w):
    from test_gpu_medial import labels_of
    k = EXACT.index(w)
    combos = [(g, a) for g in (None, 0.0, 1.5) for a in (0.0, 60.0)]
    found = 0
    for j, shape in enumerate(((22, 18, 14), (40, 30), (130,))):
        nd = len(shape)
        dtype = COMPOSITION_DTYPES[(k + j + 1) % len(COMPOSITION_DTYPES)]
        vol = labels_of(shape, dtype, seed=10 * k + j)
        data_f = np.asfortranarray(vol)
        step = min(w[:nd])
        for bb in (False, True):
            binary = bool((k + j + bb) % 2)
            measured = morph_oracle.foreground(data_f) if (binary or data_f.dtype == np.bool_) else data_f
            field = np.sqrt(morph_oracle.edtsq(measured, w[:nd], bb))
            # the oracle's own features, once for the six parameter pairs: planes [c][z][y][x]
            feat, _ = ft_oracle.feature_transform(measured.reshape(shape + (1,) * (3 - nd)),
                                                  ft_oracle.exact_factors(w[:nd]) + (1,) * (3 - nd), bb, ndim=nd)
            planes = np.stack([feat[c].transpose(2, 1, 0) for c in range(nd)])
            for gamma, angle in combos:
                kw = dict(gamma=None if gamma is None else gamma * step, min_angle=angle, black_border=bb, binary=binary)
                on = medial_oracle.on_axis(data_f, anisotropy=w[:nd], features=planes, **kw)
                found += int(on.sum())
                axis = data_f.copy(order="K")
                axis[~on] = np.zeros((), dtype=data_f.dtype)
                radius = np.where(on, field, np.float32(0.0))
                for data, own in layouts(vol):
                    got, got_radius = through_both("medial_axis", data, w, return_distance=True, **kw)
                    assert same_bits(got, own(axis)), (w, shape, kw)
                    assert same_bits(got_radius, own(radius)), (w, shape, kw)
                    assert same_bits(through_both("medial_axis", data, w, **kw), own(axis))
    assert found > 0


# ---- 4. expand_labels on INEXACT sizes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", nq.INEXACT)
def test_expand_labels_on_inexact_sizes(w):
    k = nq.INEXACT.index(w)
    lab = np.asarray(voronoi_labels((30, 26, 22), nseeds=15, seed=2, upsample=2, membrane=0.3))
    for j, vol in enumerate(cuts(lab)):
        vol = as_dtype(vol, [np.uint8, np.uint32, np.float32, np.int64][(k + j) % 4])
        nd = vol.ndim
        step = min(w[:nd])
        # (whole multiples of a size tie with its own fp32 square: they are left to the exact sizes)
        for distance in (0.0, 1.25 * step, 2.5 * step, np.inf):
            assert nq.undecided(vol, distance, w[:nd]) == 0
            first = None
            for data, own in layouts(vol):
                got = through_both("expand_labels", data, w, distance)
                assert got.dtype == data.dtype and got.shape == data.shape
                out = got if data.flags.f_contiguous else got.T
                if first is None:
                    first = out
                    assert nq.check_expand(vol, out, distance, w[:nd]) == 0
                else:
                    assert same_bits(np.asarray(out), np.asarray(first))
