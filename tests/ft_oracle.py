"""Numpy oracle of the feature transform (include/edt_hip.h: edt_hip_feature_transform) -- TEST INFRASTRUCTURE ONLY.

The separable transform with the library's tie rule, in int64: pass X, then Y, then Z, each carrying the features of the
previous one.  ``lab`` is indexed ``[x, y, z]`` (x the fastest axis of the ABI; use ``x_first`` to get there from a numpy
array), ``a`` are the squared voxel sizes scaled to integers (``w_i^2 = a_i * q``).  Returns ``(features, values)``:
features int64 of shape ``(3,) + lab.shape`` (component 0 = x), values int64 in quanta (``INF`` where no feature exists).
Labels are compared with numpy ``==`` at full width, as the kernels compare them; label 0 (also -0.0) is background.
Tiny volumes only: pure Python loops over lines.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

INF = np.int64(1) << 62


def x_first(data):
    """A C-ordered array's x axis is its last one: the [x, y, z] view of ``data`` (1-D / 2-D padded with unit axes)."""
    v = np.asarray(data).T
    return v.reshape(v.shape + (1,) * (3 - v.ndim))


def exact_factors(w_xyz):
    """The integers ``a_i`` with ``fl32(w_i)^2 = a_i * q`` for one rational ``q``, reduced by their gcd -- the ``a`` of
    :func:`feature_transform` for any voxel sizes whose squares are exact in fp32, whether the library finds a quantum for
    them (then these are its ``a_i``: (6, 6, 30) -> (1, 1, 25)) or refuses one because some ``a_i`` exceeds its 16-bit
    windows ((1, 1.0078125, 1) -> (16384, 16641, 16384)).  AssertionError where a square is not exact in fp32: the fp64
    kernels round there, and no integer rule decides their ties."""
    w32 = [Fraction(float(np.float32(w))) for w in w_xyz]
    sq = [v * v for v in w32]
    assert all(v > 0 for v in sq), f"voxel sizes {tuple(w_xyz)} must be positive"
    exact = [Fraction(float(np.float32(float(v)))) == v for v in sq]
    assert all(exact), f"voxel sizes {tuple(w_xyz)}: a square is not exact in fp32, the integer oracle does not serve them"
    scale = math.lcm(*[v.denominator for v in sq])
    ints = [int(v * scale) for v in sq]
    g = math.gcd(*ints)
    return tuple(v // g for v in ints)


def _runs(line):
    n = len(line)
    s = 0
    for i in range(1, n + 1):
        if i == n or not (line[i] == line[i - 1]):
            yield s, i - 1
            s = i


def _is_bg(v):
    return bool(v == 0)


def _pass_x(lab, a, bb):
    sx, sy, sz = lab.shape
    val = np.zeros(lab.shape, dtype=np.int64)
    fx = np.zeros(lab.shape, dtype=np.int64)
    for y in range(sy):
        for z in range(sz):
            line = lab[:, y, z]
            for s, e in _runs(line):
                if _is_bg(line[s]):
                    fx[s:e + 1, y, z] = np.arange(s, e + 1)
                    continue
                left, right = bb or s > 0, bb or e < sx - 1
                for x in range(s, e + 1):
                    dl, dr = x - s + 1, e + 1 - x
                    if left and (not right or dl <= dr):
                        val[x, y, z], fx[x, y, z] = a * dl * dl, s - 1
                    elif right:
                        val[x, y, z], fx[x, y, z] = a * dr * dr, e + 1
                    else:
                        val[x, y, z], fx[x, y, z] = INF, -1
    return val, fx


def _pass_col(lab, val, carried, a, bb, axis):
    """One column pass along ``axis`` (1: y, 2: z) of ``lab`` ([x, y, z]); ``carried``: feature components < axis."""
    labm = np.moveaxis(lab, axis, 2)
    valm = np.moveaxis(val, axis, 2)
    carm = [np.moveaxis(c, axis, 2) for c in carried]
    n = labm.shape[2]
    out_val = np.zeros(labm.shape, dtype=np.int64)
    out_f = [np.zeros(labm.shape, dtype=np.int64) for _ in range(axis + 1)]
    for u in range(labm.shape[0]):
        for v in range(labm.shape[1]):
            line = labm[u, v]
            own = [u, v] if axis == 2 else [u, None, v]  # own coordinates along the non-scan axes
            for s, e in _runs(line):
                rows = np.arange(s, e + 1)
                if _is_bg(line[s]):
                    for c in range(axis + 1):
                        out_f[c][u, v, s:e + 1] = rows if c == axis else own[c]
                    continue
                f = valm[u, v, s:e + 1]
                fin = f < INF
                for i in rows:
                    best, src, row = INF, 0, -1
                    if fin.any():
                        cand = np.where(fin, f + a * (i - rows) ** 2, INF)
                        k = int(np.argmin(cand))          # first minimum: the smallest row
                        best, src, row = int(cand[k]), 1, s + k
                    if bb or s > 0:
                        bl = a * (i - s + 1) ** 2
                        if bl <= best:
                            best, src, row = bl, 2, s - 1
                    if bb or e < n - 1:
                        br = a * (e + 1 - i) ** 2
                        if br < best:
                            best, src, row = br, 3, e + 1
                    out_val[u, v, i] = best
                    for c in range(axis + 1):
                        if src == 0:
                            out_f[c][u, v, i] = -1
                        elif c == axis:
                            out_f[c][u, v, i] = row
                        elif src == 1:
                            out_f[c][u, v, i] = carm[c][u, v, row]
                        else:
                            out_f[c][u, v, i] = own[c]
    back = lambda arr: np.moveaxis(arr, 2, axis)  # noqa: E731
    return back(out_val), [back(c) for c in out_f]


def feature_transform(lab, a=(1, 1, 1), black_border=False, ndim=None):
    """Features (3, sx, sy, sz) and pass values of the [x, y, z] volume ``lab``; ``ndim`` passes (default: 3)."""
    lab = np.asarray(lab)
    assert lab.ndim == 3
    nd = 3 if ndim is None else ndim
    a = [int(v) for v in a]
    val, fx = _pass_x(lab, a[0], bool(black_border))
    feats = [fx]
    if nd >= 2:
        val, feats = _pass_col(lab, val, feats, a[1], bool(black_border), 1)
    if nd >= 3:
        val, feats = _pass_col(lab, val, feats, a[2], bool(black_border), 2)
    sx, sy, sz = lab.shape
    full = np.zeros((3,) + lab.shape, dtype=np.int64)
    grids = np.meshgrid(np.arange(sx), np.arange(sy), np.arange(sz), indexing="ij")
    for c in range(3):
        full[c] = feats[c] if c < nd else grids[c]
    if not black_border:  # (with a black border every voxel has a feature; -1 there is the border site)
        full[:, feats[0] < 0] = -1
    return full, val


def sqdist(features, a):
    """D(p, f(p)) in quanta for every voxel of an [x, y, z] feature volume (int64; -1 where there is no feature: every
    component -1)."""
    sx, sy, sz = features.shape[1:]
    grids = np.meshgrid(np.arange(sx), np.arange(sy), np.arange(sz), indexing="ij")
    d = sum(int(a[c]) * (grids[c] - features[c]) ** 2 for c in range(3))
    return np.where(np.all(features == -1, axis=0), -1, d)


def brute_min(lab, a, black_border=False):
    """O(N^2) global minimum of D(p, q) over q != p with NOT (label(q) == label(p)) for every foreground p (0 for
    background, INF where nothing qualifies); black_border adds a shell of label 0 around the volume."""
    lab = np.asarray(lab)
    a = [int(v) for v in a]
    if black_border:
        pad = np.zeros(tuple(s + 2 for s in lab.shape), dtype=lab.dtype)
        pad[1:-1, 1:-1, 1:-1] = lab
        off = 1
    else:
        pad, off = lab, 0
    coords = np.stack(np.meshgrid(*[np.arange(s) - off for s in pad.shape], indexing="ij"), -1).reshape(-1, 3)
    flat = pad.reshape(-1)
    out = np.zeros(lab.shape, dtype=np.int64)
    for idx in np.ndindex(lab.shape):
        L = lab[idx]
        if L == 0:
            continue
        other = ~(flat == L)
        p = np.array(idx)
        other &= ~np.all(coords == p, axis=1)
        if not other.any():
            out[idx] = INF
            continue
        d = ((coords[other] - p) ** 2 * np.array(a)).sum(1)
        out[idx] = d.min()
    return out
