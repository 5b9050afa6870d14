"""Voxel sizes for which the library finds no quantum, and references for them -- TEST INFRASTRUCTURE ONLY (numpy and scipy).

The feature transform (csrc/edt_feature.hip) runs on exact int64 quanta where the voxel sizes share a quantum and on fp64
otherwise.  Two kinds of sizes take the fp64 kernels:

``EXACT``    every ``fl32(w_i)^2`` is exact in fp32 and the ratios are small rationals, but some ``a_i = w_i^2 / q`` exceeds the
             16384 the 16-bit column kernel's quantum allows, so the library refuses a quantum.  Every value the fp64 kernels
             form -- ``a d^2``, their sums, ``num``, ``den`` and ``t den`` of the hull -- is then an integer multiple of one
             power of two and stays below 2^53 times it (``4 sum a_i (s_i + 1)^2 < 2^53``: ``exact_bound``), so the arithmetic
             is exact, ``floor(num / den)`` too (the quotient's fraction is a multiple of ``1 / den``, far above its ulp), and
             the output must equal the int64 tie rule of ``ft_oracle.feature_transform`` with ``ft_oracle.exact_factors``,
             bit for bit.  The table maps the sizes (x, y, z) to those factors.
``INEXACT``  the squares are not exact in fp32: the header's contract holds, D(p, f(p)) <= (1 + 2^-20) min_q D(p, q), and the
             minimum comes from scipy, label by label (``best_sq``), independently of the library.

Volumes are indexed x first (``[x]``, ``[x, y]`` or ``[x, y, z]``: x the fastest axis of the ABI), voxel sizes likewise.
"""
from __future__ import annotations

import numpy as np

EXACT = {
    (1.0, 1.0078125, 1.0): (16384, 16641, 16384),
    (1.0078125, 1.0, 1.00390625): (66564, 65536, 66049),
    (0.75, 1.00390625, 1.0078125): (36864, 66049, 66564),
    (1.0, 129.0, 1.0): (1, 16641, 1),
    (129.0, 1.0, 3.0): (16641, 1, 9),
    (1.0, 0.00390625, 1.0): (65536, 1, 65536),
    (1.0, 181.0, 2.0): (1, 32761, 4),
}
INEXACT = ((3.58, 3.58, 40.0), (1.1, 0.7, 2.3), (0.1, 0.3, 0.2), (40.0, 3.58, 3.58))

UPPER = 1.0 + 2.0 ** -20     # include/edt_hip.h: D(p, f(p)) <= (1 + 2^-20) min_q D(p, q)
LOWER = 1.0 - 2.0 ** -48     # three products and two sums, each within 2^-53, on either side of the comparison


def exact_bound(a, extents):
    """4 sum a_i (s_i + 1)^2: above every value the kernels form at these extents, in quanta"""
    return 4 * sum(int(ai) * (int(s) + 1) ** 2 for ai, s in zip(a, extents))


def squares(w):
    """the fp64 squares of the voxel sizes rounded to fp32, as the ABI takes them"""
    return [np.float64(np.float32(v)) * np.float64(np.float32(v)) for v in w]


def _grids(shape):
    return np.meshgrid(*[np.arange(s, dtype=np.int64) for s in shape], indexing="ij") if len(shape) else []


def sq_from(shape, index, w):
    """D(p, index(p)) in fp64, the terms added in the order x, y, z"""
    w2 = squares(w)
    D = np.zeros(shape)
    for c, g in enumerate(_grids(shape)):
        D = D + w2[c] * ((g - index[c].astype(np.int64)) ** 2).astype(np.float64)
    return D


def _nearest_zero_sq(mask, w):
    """for every voxel of the boolean ``mask``: fp64 D to the nearest False voxel (0 on False voxels; +inf if there is none)"""
    from scipy import ndimage
    if mask.all():
        return np.full(mask.shape, np.inf)
    nd = mask.ndim
    sampling = [float(np.float32(v)) for v in w[:nd]]
    ind = ndimage.distance_transform_edt(mask, sampling=sampling, return_distances=False, return_indices=True)
    return sq_from(mask.shape, ind, w)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}")


def best_sq(lab_xyz, w, bb):
    """min over q of D(p, q), q a voxel whose label does not compare equal to p's, for every foreground voxel p of the x-first
    volume ``lab_xyz`` (1-D to 3-D; ``w``: its voxel sizes, x first): fp64 from scipy's indices, label by label; 0 on the
    background, +inf where nothing qualifies.  ``bb``: one shell of label 0 around the volume."""
    lab = np.asarray(lab_xyz)
    assert not (lab.dtype.kind == "f" and np.isnan(lab).any()), "a NaN voxel differs from itself: not served"
    nd = lab.ndim
    if bb:
        pad = np.zeros(tuple(s + 2 for s in lab.shape), dtype=lab.dtype)
        pad[(slice(1, -1),) * nd] = lab
    else:
        pad = lab
    out = np.zeros(pad.shape)
    for L in np.unique(pad):
        if L == 0:
            continue
        mine = pad == L
        out[mine] = _nearest_zero_sq(mine, w)[mine]
    return out[(slice(1, -1),) * nd] if bb else out


def to_xyz(data, feat):
    """``(lab, features)`` x first, both 3-D with unit extents behind the array's own: the scipy-layout features ``feat``
    (``(ndim,) + data.shape``, component k along array axis k) of a numpy array in the memory order the Python layer gives it
    (axis 0 is x for an F-contiguous array, the last axis otherwise).  Components past ndim are the voxel's own coordinate."""
    data, feat = np.asarray(data), np.asarray(feat)
    nd = data.ndim
    if data.flags.f_contiguous:
        lab, comps = data, [feat[k] for k in range(nd)]
    else:
        lab, comps = data.T, [feat[nd - 1 - k].T for k in range(nd)]
    shape3 = lab.shape + (1,) * (3 - nd)
    g3 = _grids(shape3)
    full = np.stack([comps[c].reshape(shape3).astype(np.int64) if c < nd else g3[c] for c in range(3)])
    return lab.reshape(shape3), full


def check_features(lab_xyz, feat, w, bb, ndim, best=None):
    """Asserts the header's contract for voxel sizes without a quantum (include/edt_hip.h, feature transform) on the x-first
    3-D volume ``lab_xyz`` (unit extents past ``ndim``) and its features ``(3 or ndim, sx, sy, sz)``; ``best``: best_sq of the
    volume's first ndim axes, if the caller has it already."""
    lab = np.asarray(lab_xyz)
    shape = lab.shape[:ndim]
    assert lab.shape[ndim:] == (1,) * (lab.ndim - ndim)
    lab = lab.reshape(shape)
    f = np.stack([np.asarray(feat[c]).reshape(shape).astype(np.int64) for c in range(ndim)])
    grids = np.stack(_grids(shape))
    ext = np.array(shape, dtype=np.int64).reshape((ndim,) + (1,) * ndim)
    with np.errstate(invalid="ignore"):
        fg = np.asarray(lab != 0)
    # a background voxel is its own feature
    assert np.array_equal(f[:, ~fg], grids[:, ~fg]), "a background voxel is not its own feature"
    if best is None:
        best = best_sq(lab, w, bb)
    none = np.all(f == -1, axis=0) & fg
    if not bb:
        # all components -1 iff nothing qualifies: no voxel of another label, no border
        nothing = fg & np.isinf(best)
        assert np.array_equal(none, nothing), "-1 in every component where a feature exists, or a feature where none does"
    else:
        assert not np.isinf(best[fg]).any()
        none = np.zeros(shape, dtype=bool)          # (in 1-D the border site -1 is all components -1: a feature)
    has = fg & ~none
    below, above = f < 0, f >= ext
    inside = has & ~np.any(below | above, axis=0)
    outside = has & ~inside
    # inside the volume: another label
    at = tuple(f[c][inside] for c in range(ndim))
    with np.errstate(invalid="ignore"):
        assert not np.any(lab[at] == lab[inside]), "a feature carries the voxel's own label"
    # outside: only under a border, one component off by one voxel, the others the voxel's own
    if not bb:
        assert not outside.any(), "a feature outside the volume without a border"
    else:
        off = (below | above).sum(0)
        assert np.all(off[outside] == 1), "a border feature off in more than one component"
        one_out = (f == -1) | (f == ext)
        assert np.all((one_out == (below | above))[:, outside]), "a border feature more than one voxel outside"
        own = (f == grids) | below | above
        assert np.all(own[:, outside]), "a border feature away from the voxel's own row"
    D = sq_from(shape, f, w)
    assert np.all(D[has] <= best[has] * UPPER), "a feature farther than (1 + 2^-20) times the nearest"
    assert np.all(D[has] >= best[has] * LOWER), "a feature nearer than the nearest: it cannot qualify"


def _nearest_foreground_sq(labels, w):
    with np.errstate(invalid="ignore"):
        bg = np.asarray(labels == 0)
    return bg, _nearest_zero_sq(bg, w)


def undecided(labels, distance, w):
    """how many background voxels of the x-first volume ``labels`` have their nearest foreground at a squared distance in
    (distance^2 / (1 + 2^-20), distance^2]: whether expand_labels fills them is up to the features' 2^-20"""
    bg, best = _nearest_foreground_sq(np.asarray(labels), w)
    d2 = np.float64(distance) * np.float64(distance)
    fin = bg & np.isfinite(best)
    return int(np.count_nonzero(fin & (best <= d2) & ~(best * UPPER <= d2)))


def check_expand(labels, out, distance, w):
    """Asserts expand_labels' definition (include/edt_hip.h) on the x-first volumes ``labels`` and ``out`` within the feature
    transform's contract; returns the number of undecided voxels (see ``undecided``), which are not judged."""
    labels, out = np.asarray(labels), np.asarray(out)
    assert out.shape == labels.shape and out.dtype == labels.dtype
    lb, ob = _bits(labels).reshape(labels.shape), _bits(out).reshape(labels.shape)
    bg, best = _nearest_foreground_sq(labels, w)
    d2 = np.float64(distance) * np.float64(distance)
    assert np.array_equal(ob[~bg], lb[~bg]), "a foreground voxel changed"
    with np.errstate(invalid="ignore"):
        filled = bg & np.asarray(out != 0)
    assert np.array_equal(ob[bg & ~filled], lb[bg & ~filled]), "an unfilled voxel changed"
    fin = bg & np.isfinite(best)
    must = fin & (best * UPPER <= d2)
    assert np.all(filled[must]), "a voxel within the distance was left empty"
    for L in np.unique(ob[filled]):
        mine = filled & (ob == L)
        DL = _nearest_zero_sq(lb != L, w)
        assert np.all(np.isfinite(DL[mine])), "a voxel took a label the volume does not hold"
        assert np.all(DL[mine] <= d2), "a voxel was filled beyond the distance"
        assert np.all(DL[mine] <= best[mine] * UPPER), "a voxel took a label that is not the nearest's"
    return int(np.count_nonzero(fin & (best <= d2) & ~must))
