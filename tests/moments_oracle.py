"""The label_moments contract (include/edt_hip.h, "label_moments") restated in Python integers, at the level of
``edt.label_moments``: one row per distinct non-zero label in ascending order, its voxel count, the exact raw first and second
moments per array axis, the centroid ``float(S_a) / float(n)`` and the population covariance
``float(n * S_ab - S_a * S_b) / float(n) / float(n)`` over Python integers -- ``float(int)`` is Python's correctly rounded
conversion, the ONE rounding of each exact integer.  The key rules (-0.0 is background, NaN voxels belong to no label, the memory order of an
array) are those of tests/label_stats_oracle.py."""
import collections

import numpy as np

from label_stats_oracle import memory_order

LabelMoments = collections.namedtuple("LabelMoments", ["labels", "counts", "first", "second", "centroid", "covariance"])


def derive(n, first, second):
    """(centroid, covariance) of one label from its exact sums: Python ints in, floats out"""
    nd = len(first)
    fn = float(n)
    centroid = [float(first[a]) / fn for a in range(nd)]
    cov = [[float(n * second[a][b] - first[a] * first[b]) / fn / fn for b in range(nd)] for a in range(nd)]
    return centroid, cov


def label_moments(data):
    data = np.asarray(data)
    nd = data.ndim
    flat = data.reshape(-1)
    with np.errstate(invalid="ignore"):
        fg = np.flatnonzero((flat != 0) & (flat == flat))   # (-0.0 != 0 is False; NaN == NaN is False)
    keys, inv = np.unique(flat[fg], return_inverse=True)
    inv = inv.reshape(-1)
    n = len(keys)
    coords = np.unravel_index(fg, data.shape)
    counts = np.bincount(inv, minlength=n).astype(np.int64)
    # inside the contract's range bound every sum fits int64, and an int64 sum that does not overflow is exact
    assert data.size * max(max(data.shape) - 1, 0) ** 2 < 1 << 63, "past the range bound of label_moments"
    first = np.zeros((n, nd), dtype=np.int64)
    second = np.zeros((n, nd, nd), dtype=np.int64)
    order = np.argsort(inv, kind="stable")
    starts = (np.cumsum(counts) - counts).astype(np.intp)
    c = [coords[a][order].astype(np.int64) for a in range(nd)]
    for a in range(nd if n else 0):
        first[:, a] = np.add.reduceat(c[a], starts)
        for b in range(a, nd):
            second[:, a, b] = second[:, b, a] = np.add.reduceat(c[a] * c[b], starts)
    centroid = np.zeros((n, nd), dtype=np.float64)
    cov = np.zeros((n, nd, nd), dtype=np.float64)
    for i in range(n):
        centroid[i], cov[i] = derive(int(counts[i]), first[i].tolist(), second[i].tolist())   # (tolist: Python ints)
    return LabelMoments(keys.astype(data.dtype), counts, first, second, centroid, cov)


def brute_force(data):
    """The same, label by label with np.nonzero -- what the oracle itself is held against on tiny volumes."""
    data = np.asarray(data)
    nd = data.ndim
    rows = []
    for key in sorted(set(v for v in data.reshape(-1).tolist() if v == v and v != 0)):
        pts = [[int(v) for v in axis] for axis in np.nonzero(data == key)]
        n = len(pts[0])
        first = [sum(pts[a]) for a in range(nd)]
        second = [[sum(p * q for p, q in zip(pts[a], pts[b])) for b in range(nd)] for a in range(nd)]
        rows.append((key, n, first, second) + derive(n, first, second))
    n = len(rows)
    return LabelMoments(np.array([r[0] for r in rows], dtype=data.dtype), np.array([r[1] for r in rows], dtype=np.int64),
                        np.array([r[2] for r in rows], dtype=np.int64).reshape(n, nd),
                        np.array([r[3] for r in rows], dtype=np.int64).reshape(n, nd, nd),
                        np.array([r[4] for r in rows], dtype=np.float64).reshape(n, nd),
                        np.array([r[5] for r in rows], dtype=np.float64).reshape(n, nd, nd))


def abi_table(data, want=None):
    """The table as the C ABI lays it out for the x-fastest buffer of `data` (x = the fastest axis of its memory order):
    (keys in the ABI's order -- integers as unsigned bit patterns --, counts, sums (n, 9), centroid (n, 3), central (n, 6)).
    want: label_moments(data), where the caller has it."""
    data = np.asarray(data)
    nd = data.ndim
    want = label_moments(data) if want is None else want
    axis = list(range(nd)) if memory_order(data) == "F" else list(range(nd))[::-1]   # x / y / z -> array axis
    n = len(want.labels)
    sums, centroid, central = np.zeros((n, 9), dtype=np.int64), np.zeros((n, 3), dtype=np.float64), np.zeros((n, 6), dtype=np.float64)
    pairs = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
    for k in range(nd):
        sums[:, k] = want.first[:, axis[k]]
        centroid[:, k] = want.centroid[:, axis[k]]
    for p, (a, b) in enumerate(pairs):
        if a < nd and b < nd:
            sums[:, 3 + p] = want.second[:, axis[a], axis[b]]
            central[:, p] = want.covariance[:, axis[a], axis[b]]
    keys = want.labels
    if keys.dtype.kind == "i":
        keys = keys.view(f"u{keys.dtype.itemsize}")
    elif keys.dtype.kind == "b":
        keys = keys.view(np.uint8)
    perm = np.argsort(keys, kind="stable") if keys.dtype.kind == "u" else np.arange(n)
    return keys[perm], want.counts[perm], sums[perm], centroid[perm], central[perm]


def assert_same(got, want, what=""):
    """array_equal on the integers and on the BITS of the floats"""
    for name, g, w in zip(LabelMoments._fields, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float64:
            g, w = np.ascontiguousarray(g).view(np.uint64), np.ascontiguousarray(w).view(np.uint64)
        assert np.array_equal(g, w), (what, name, g[:8], w[:8])
