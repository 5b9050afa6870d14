"""Numpy oracle of the integer medial axis (include/edt_hip.h, "medial axis") -- TEST INFRASTRUCTURE ONLY.

Two statements of the same definition, on features handed in (from ``ft_oracle.feature_transform`` or from anywhere else):

``gather``   the header's form, vectorised: every voxel looks at its 2 * ndim face neighbours and decides for itself, with the
             header's fp64 evaluation order (numpy's float64 products and sums are rounded once each, nothing is contracted);
``scatter``  the paper's loop (Hesselink & Roerdink 2008, procedure ``compare``): every PAIR (p, p + e_c) is visited once and
             marks p if crit >= 0 and its neighbour if crit <= 0 -- scalar Python floats, no code shared with ``gather``.

``lab`` is indexed ``[x, y, z]`` (x the fastest axis of the ABI; ``ft_oracle.x_first`` gets there from a numpy array),
``feat`` is ``(3, sx, sy, sz)`` integer features (component 0 = x; only the first ``ndim`` are read), ``w`` the three voxel
sizes (rounded to float32 like the ABI's).  Both return a boolean ``[x, y, z]`` volume: on the axis or not.
``on_axis`` / ``medial_axis`` are the whole operation on a numpy array in its own memory order, through ``ft_oracle``.
"""
from __future__ import annotations

import math

import numpy as np

import ft_oracle


def ratio_of(min_angle):
    """tan^2(theta / 2) of an angle in degrees: the ``ratio`` of the ABI"""
    return math.tan(math.radians(float(min_angle)) / 2.0) ** 2


def _squares(w):
    return [float(np.float64(np.float32(v)) * np.float64(np.float32(v))) for v in w]


def _has_feature(feat, ndim, black_border):
    if black_border:
        return np.ones(feat.shape[1:], dtype=bool)
    return ~np.all(feat[:ndim] == -1, axis=0)


def gather(lab, feat, w=(1.0, 1.0, 1.0), gamma=1.0, ratio=0.0, black_border=False, binary=False, ndim=3):
    lab = np.asarray(lab)
    feat = np.asarray(feat).astype(np.int64)
    assert lab.ndim == 3 and feat.shape == (3,) + lab.shape
    A = _squares(w)
    g2 = float(gamma) * float(gamma)
    has = _has_feature(feat, ndim, black_border)
    grids = np.meshgrid(*[np.arange(s, dtype=np.int64) for s in lab.shape], indexing="ij")
    on = np.zeros(lab.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        fg = lab != 0
    for axis in range(ndim):
        n = lab.shape[axis]
        if n < 2:
            continue
        for step in (-1, 1):
            # p runs over the voxels that have a neighbour q = p + step * e_axis inside the volume
            sp = [slice(None)] * 3
            sq = [slice(None)] * 3
            sp[axis] = slice(1, n) if step < 0 else slice(0, n - 1)
            sq[axis] = slice(0, n - 1) if step < 0 else slice(1, n)
            sp, sq = tuple(sp), tuple(sq)
            with np.errstate(invalid="ignore"):
                same = fg[sq] if binary else (lab[sq] == lab[sp])
            ok = fg[sp] & same & has[sp] & has[sq]
            sep = h = crit = None
            for c in range(ndim):
                d = (feat[c][sp] - feat[c][sq]).astype(np.float64)
                s = (feat[c][sp] + feat[c][sq] - grids[c][sp] - grids[c][sq]).astype(np.float64)
                t_sep, t_h, t_crit = A[c] * (d * d), A[c] * (s * s), A[c] * (d * s)
                sep = t_sep if sep is None else sep + t_sep
                h = t_h if h is None else h + t_h
                crit = t_crit if crit is None else crit + t_crit
            on[sp] |= ok & (sep > g2) & (sep >= ratio * h) & (crit >= 0.0)
    return on


def scatter(lab, feat, w=(1.0, 1.0, 1.0), gamma=1.0, ratio=0.0, black_border=False, binary=False, ndim=3):
    lab = np.asarray(lab)
    feat = np.asarray(feat)
    A = _squares(w)
    g2 = float(gamma) * float(gamma)
    skel = np.zeros(lab.shape, dtype=bool)

    def featured(p):
        return black_border or any(int(feat[c][p]) != -1 for c in range(ndim))

    def compare(p, q):
        lp, lq = lab[p], lab[q]
        if not (lp != 0) or not ((lq != 0) if binary else (lq == lp)) or not featured(p) or not featured(q):
            return
        sep = h = crit = 0.0
        for c in range(ndim):
            xf, yf = int(feat[c][p]), int(feat[c][q])
            d, s = float(xf - yf), float(xf + yf - p[c] - q[c])
            if c == 0:
                sep, h, crit = A[c] * (d * d), A[c] * (s * s), A[c] * (d * s)
            else:
                sep, h, crit = sep + A[c] * (d * d), h + A[c] * (s * s), crit + A[c] * (d * s)
        if sep > g2 and sep >= ratio * h:
            if crit >= 0.0:
                skel[p] = True
            if crit <= 0.0:
                skel[q] = True

    for p in np.ndindex(lab.shape):
        for c in range(ndim):
            if p[c] + 1 < lab.shape[c]:
                q = list(p)
                q[c] += 1
                compare(p, tuple(q))
    return skel


def quantum(w):
    """integers a_c with w_c^2 = a_c * q for voxel sizes whose squares are exact in fp32 (ft_oracle's ``a``)"""
    return ft_oracle.exact_factors(w)


def xyz_view(data, anisotropy=None):
    """``(lab [x, y, z], w (wx, wy, wz), ndim, back)`` of a numpy array in the memory order the Python layer gives it: axis 0
    is x for an F-contiguous array, the last axis otherwise; ``back`` maps an [x, y, z] volume onto ``data``'s axes."""
    data = np.asarray(data)
    nd = data.ndim
    an = (1.0,) * nd if anisotropy is None else tuple(np.ravel(anisotropy))
    fortran = data.flags.f_contiguous
    v = data if fortran else data.T
    w = tuple(an if fortran else an[::-1]) + (1.0,) * (3 - nd)
    shape = v.shape

    def back(vol):
        r = np.asarray(vol).reshape(shape)
        return r if fortran else r.T

    return v.reshape(shape + (1,) * (3 - nd)), w, nd, back


def on_axis(data, gamma=None, min_angle=0.0, anisotropy=None, black_border=False, binary=False, features=None, form=gather):
    """The boolean axis of a numpy array, in the array's own axes.  ``features``: ABI planes ``(ndim, ...)`` in x, y, z order
    over the [x, y, z] view flattened x fastest (what the device step reads); None: ``ft_oracle`` on voxel sizes whose squares
    are exact in fp32 (``ft_oracle.exact_factors``)."""
    lab, w, nd, back = xyz_view(data, anisotropy)
    if data.dtype == bool:
        binary = True
    if features is None:
        with np.errstate(invalid="ignore"):
            of = (lab != 0).astype(np.uint8) if binary else lab
        feat, _ = ft_oracle.feature_transform(of, quantum(w[:nd]) + (1,) * (3 - nd), black_border, ndim=nd)
    else:
        planes = np.asarray(features).reshape((nd,) + lab.shape[::-1])           # [c][z][y][x]
        feat = np.zeros((3,) + lab.shape, dtype=np.int64)
        for c in range(nd):
            feat[c] = planes[c].transpose(2, 1, 0)
    g = max(abs(float(np.float32(v))) for v in w[:nd]) if gamma is None else float(gamma)
    return back(form(lab, feat, w, g, ratio_of(min_angle), black_border, binary, nd))


def medial_axis(data, **kw):
    """What edt.medial_axis returns without ``return_distance``: the label on the axis, zero bits elsewhere"""
    data = np.asarray(data)
    on = on_axis(data, **kw)
    out = data.copy(order="K")
    out[~on] = np.zeros((), dtype=data.dtype)
    return out
