"""numpy restatement of the label_stats contract (include/edt_hip.h), at the level of ``edt.label_stats``: one row per
distinct non-zero label in ascending order (``np.unique``: signed order for signed dtypes, numeric order for floats), its
voxel count, the largest ``dt`` over its voxels, the coordinates of the first voxel IN MEMORY ORDER that attains it and the
inclusive bounding box per array axis.  -0.0 is background; NaN voxels belong to no label.  Memory order is the library's:
Fortran for an F-contiguous array (also one that is C-contiguous as well), C otherwise."""
import collections

import numpy as np

LabelStats = collections.namedtuple("LabelStats", ["labels", "counts", "max", "argmax", "bbox_lo", "bbox_hi"])


def memory_order(data):
    return "F" if data.flags.f_contiguous else "C"


def label_stats(data, dt):
    data = np.asarray(data)
    if not data.flags.c_contiguous and not data.flags.f_contiguous:
        data = np.ascontiguousarray(data)
    dt = np.asarray(dt, dtype=np.float32)
    assert dt.shape == data.shape
    nd, order = data.ndim, memory_order(data)
    flat, fdt = data.reshape(-1, order=order), dt.reshape(-1, order=order)
    with np.errstate(invalid="ignore"):
        fg = np.flatnonzero((flat != 0) & (flat == flat))   # (-0.0 != 0 is False; NaN == NaN is False)
    keys, inv = np.unique(flat[fg], return_inverse=True)
    inv = inv.reshape(-1)
    n = len(keys)
    counts = np.bincount(inv, minlength=n).astype(np.int64)
    mx = np.full(n, -np.inf, dtype=np.float32)
    np.maximum.at(mx, inv, fdt[fg])
    hit = fdt[fg] == mx[inv]
    first = np.full(n, flat.size, dtype=np.int64)
    np.minimum.at(first, inv[hit], fg[hit])
    coords = np.stack(np.unravel_index(fg, data.shape, order=order), axis=1).astype(np.int32).reshape(len(fg), nd)
    lo = np.full((n, nd), np.iinfo(np.int32).max, dtype=np.int32)
    hi = np.full((n, nd), -1, dtype=np.int32)
    for k in range(nd):
        np.minimum.at(lo[:, k], inv, coords[:, k])
        np.maximum.at(hi[:, k], inv, coords[:, k])
    argmax = np.stack(np.unravel_index(first, data.shape, order=order), axis=1).astype(np.int64).reshape(n, nd)
    return LabelStats(keys.astype(data.dtype), counts, mx, argmax, lo, hi)


def brute_force(data, dt):
    """The same, label by label with masks -- what the oracle itself is held against on tiny volumes."""
    data, dt = np.asarray(data), np.asarray(dt, dtype=np.float32)
    nd, order = data.ndim, memory_order(data)
    flat, fdt = data.reshape(-1, order=order), dt.reshape(-1, order=order)
    rows = []
    for key in sorted(set(v for v in flat.tolist() if v == v and v != 0)):
        mask = flat == key
        idx = np.flatnonzero(mask)
        m = fdt[idx].max()
        first = int(idx[fdt[idx] == m][0])
        where = np.argwhere(data == key)
        rows.append((key, len(idx), m, np.unravel_index(first, data.shape, order=order), where.min(0), where.max(0)))
    n = len(rows)
    return LabelStats(np.array([r[0] for r in rows], dtype=data.dtype), np.array([r[1] for r in rows], dtype=np.int64),
                      np.array([r[2] for r in rows], dtype=np.float32),
                      np.array([r[3] for r in rows], dtype=np.int64).reshape(n, nd),
                      np.array([r[4] for r in rows], dtype=np.int32).reshape(n, nd),
                      np.array([r[5] for r in rows], dtype=np.int32).reshape(n, nd))


def assert_same(got, want, what=""):
    for name, g, w in zip(LabelStats._fields, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, g[:8], w[:8])
