"""The label_topology contract (include/edt_hip.h, "label_topology") restated in numpy, at the level of ``edt.label_topology``:
one row per distinct non-zero label in ascending order, its voxel count and the two cell-count tables per array axis.

``label_topology`` handles all labels at once: for every cell type, the incident voxels of every cell of that type are padded,
shifted copies of the label-index array; a cell is in ``closed[L]`` when L is among them and in ``interior[L]`` when they all
are L.  No ownership rule, no neighbourhood word: it shares nothing with csrc/edt_topology_math.h.  ``brute_force`` is the
second formulation, which shares nothing with the first: the set of every voxel's 3^nd cells in doubled integer coordinates,
grouped by type, in plain Python.  The key rules (-0.0 is background, NaN voxels belong to no label, the memory order of an
array) are those of tests/label_stats_oracle.py."""
import collections
import itertools

import numpy as np

from label_stats_oracle import memory_order

LabelTopology = collections.namedtuple("LabelTopology", ["labels", "counts", "closed", "interior"])


def label_index(data):
    """(keys ascending, an intp array of the data's shape: 0 for background, else 1 + the index of the voxel's key)"""
    data = np.asarray(data)
    flat = data.reshape(-1)
    with np.errstate(invalid="ignore"):
        fg = np.flatnonzero((flat != 0) & (flat == flat))   # (-0.0 != 0 is False; NaN == NaN is False)
    keys, inv = np.unique(flat[fg], return_inverse=True)
    idx = np.zeros(flat.shape, dtype=np.intp)
    idx[fg] = inv.reshape(-1) + 1
    return keys.astype(data.dtype), idx.reshape(data.shape)


def label_topology(data):
    data = np.asarray(data)
    nd = data.ndim
    keys, idx = label_index(data)
    n = len(keys)
    padded = np.pad(idx, 1)
    closed = np.zeros((n,) + (2,) * nd, dtype=np.int64)
    interior = np.zeros((n,) + (2,) * nd, dtype=np.int64)
    for kind in itertools.product((0, 1), repeat=nd):
        # along an axis the cell extends along it lies at a voxel; across it lies between two voxels (extent + 1 positions)
        choices = [[slice(1, data.shape[a] + 1)] if kind[a] else [slice(0, data.shape[a] + 1), slice(1, data.shape[a] + 2)]
                   for a in range(nd)]
        incident = np.sort(np.stack([padded[sl].reshape(-1) for sl in itertools.product(*choices)]), axis=0)
        distinct = incident != 0
        distinct[1:] &= incident[1:] != incident[:-1]
        closed[(slice(None),) + kind] = np.bincount(incident[distinct], minlength=n + 1)[1:]
        every = (incident[0] == incident[-1]) & (incident[0] != 0)
        interior[(slice(None),) + kind] = np.bincount(incident[0][every], minlength=n + 1)[1:]
    counts = np.bincount(idx.reshape(-1), minlength=n + 1)[1:].astype(np.int64)
    return LabelTopology(keys, counts, closed, interior)


def brute_force(data):
    """The same from sets of cells in doubled coordinates (voxel p is the cell 2p + 1; its cells are 2p + 1 + c), in plain
    Python: a cell's type is the parity of its coordinates, its incident voxels follow from them alone."""
    data = np.asarray(data)
    nd = data.ndim
    values = data.tolist() if nd else data
    def at(p):
        v = values
        for a in range(nd):
            if p[a] < 0 or p[a] >= data.shape[a]:
                return None
            v = v[p[a]]
        return v
    cells = collections.defaultdict(set)
    for p in itertools.product(*[range(s) for s in data.shape]):
        v = at(p)
        if v == v and v != 0:
            for c in itertools.product((-1, 0, 1), repeat=nd):
                cells[v].add(tuple(2 * p[a] + 1 + c[a] for a in range(nd)))
    keys = sorted(cells)
    n = len(keys)
    closed = np.zeros((n,) + (2,) * nd, dtype=np.int64)
    interior = np.zeros((n,) + (2,) * nd, dtype=np.int64)
    counts = np.zeros(n, dtype=np.int64)
    for i, key in enumerate(keys):
        for cell in cells[key]:
            kind = tuple(d % 2 for d in cell)
            closed[(i,) + kind] += 1
            incident = itertools.product(*[[d // 2] if d % 2 else [d // 2 - 1, d // 2] for d in cell])
            interior[(i,) + kind] += all(at(q) == key for q in incident)
        counts[i] = closed[(i,) + (1,) * nd]
    return LabelTopology(np.array(keys, dtype=data.dtype), counts, closed, interior)


def euler(table, full=True):
    """sum over types of (-1)^|S| closed[S] (full adjacency), or of (-1)^(nd - |S|) interior[S] (face adjacency), per label"""
    nd = table.closed.ndim - 1
    out = np.zeros(len(table.labels), dtype=np.int64)
    for kind in itertools.product((0, 1), repeat=nd):
        dim = sum(kind)
        out += ((-1) ** dim * table.closed if full else (-1) ** (nd - dim) * table.interior)[(slice(None),) + kind]
    return out


def abi_table(data, want=None, order=None):
    """The table as the C ABI lays it out for the x-fastest buffer of `data` (x = the fastest axis of its memory order): keys
    in the ABI's order -- integers as unsigned bit patterns --, closed (n, 8), interior (n, 8), a type's bit 0 = x.  A missing
    axis: the slab's closed cells transverse to it are two copies of the image's, its interior cells transverse to it are 0.
    want: label_topology(data), where the caller has it.  order: "C" or "F" where the caller says which axis is x (an array with
    unit axes is contiguous both ways); else the array's memory order."""
    data = np.asarray(data)
    nd = data.ndim
    want = label_topology(data) if want is None else want
    axis = list(range(nd)) if (order or memory_order(data)) == "F" else list(range(nd))[::-1]   # x / y / z -> array axis
    n = len(want.labels)
    closed, interior = np.zeros((n, 8), dtype=np.int64), np.zeros((n, 8), dtype=np.int64)
    for t in range(8):
        kind = [0] * nd
        for k in range(nd):
            kind[axis[k]] = (t >> k) & 1
        across_missing = sum(1 for k in range(nd, 3) if not (t >> k) & 1)
        closed[:, t] = want.closed[(slice(None),) + tuple(kind)] * 2 ** across_missing
        if not across_missing:
            interior[:, t] = want.interior[(slice(None),) + tuple(kind)]
    keys = want.labels
    if keys.dtype.kind == "i":
        keys = keys.view(f"u{keys.dtype.itemsize}")
    elif keys.dtype.kind == "b":
        keys = keys.view(np.uint8)
    perm = np.argsort(keys, kind="stable") if keys.dtype.kind == "u" else np.arange(n)
    return keys[perm], closed[perm], interior[perm]


def assert_same(got, want, what=""):
    for name, g, w in zip(LabelTopology._fields, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype.kind == "f":
            g, w = np.ascontiguousarray(g).view(f"u{g.dtype.itemsize}"), np.ascontiguousarray(w).view(f"u{w.dtype.itemsize}")
        assert np.array_equal(g, w), (what, name, g[:4], w[:4])
