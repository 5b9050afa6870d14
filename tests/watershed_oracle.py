"""The contract of watershed (include/edt_hip.h, "watershed") restated twice: in numpy + scipy.sparse.csgraph (the joins of both
phases as the edges of a graph, its components numbered by first occurrence in memory), and, for tiny volumes, as a deliberately
naive pure-Python loop over voxels with a union-find of its own, so that the fast oracle does not rest on itself."""
import itertools

import numpy as np


def _canonical(a):
    """`a` as a C-contiguous array whose flat index is the memory index (x the last axis), and whether it was transposed."""
    a = np.asarray(a)
    if not a.flags.c_contiguous and not a.flags.f_contiguous:
        a = np.ascontiguousarray(a)
    if a.flags.f_contiguous and not (a.flags.c_contiguous and a.ndim <= 1):
        return a.T, True                   # (both orders: F, as in every entry point of the module)
    return a, False


def _offsets(nd, c, half=False):
    """The neighbour offsets in ascending order of the memory index; half: the preceding ones only."""
    zero = (0,) * nd
    return [o for o in itertools.product((-1, 0, 1), repeat=nd) if 0 < sum(map(abs, o)) <= c and (not half or o < zero)]


def _pair(shape, off):
    """(a, b): for every voxel p of a, the voxel p + off is the one at the same place of b."""
    a = tuple(slice(max(0, -o), s - max(0, o)) for o, s in zip(off, shape))
    b = tuple(slice(max(0, o), s - max(0, -o)) for o, s in zip(off, shape))
    return a, b


def _number(comp, fg, shape):
    """0 for background, else 1..N by first occurrence of the component id in memory order."""
    flat = comp.reshape(-1)[fg.reshape(-1)]
    if flat.size == 0:
        return np.zeros(shape, dtype=np.uint32), 0
    ids, first = np.unique(flat, return_index=True)
    rank = np.empty(len(ids), dtype=np.int64)
    rank[np.argsort(first)] = np.arange(1, len(ids) + 1)
    out = np.zeros(int(np.prod(shape)), dtype=np.uint32)
    out[fg.reshape(-1)] = rank[np.searchsorted(ids, flat)]
    return out.reshape(shape), len(ids)


def _components(n, rows, cols):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    rows, cols = np.concatenate(rows) if rows else np.zeros(0, np.int64), np.concatenate(cols) if cols else np.zeros(0, np.int64)
    g = coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(n, n))
    return connected_components(g, directed=False)[1]


def _conn(lab, fg, a, b, binary):
    with np.errstate(invalid="ignore"):
        return fg[a] & fg[b] & (True if binary else lab[a] == lab[b])          # NaN equals nothing


def phase1(lab, f, c, binary):
    """(comp, top, fg) on canonical arrays: the phase-1 basin id of every voxel (background: its own), the top voxels."""
    shape, nd = lab.shape, lab.ndim
    with np.errstate(invalid="ignore"):
        fg = lab != 0
    idx = np.arange(lab.size, dtype=np.int64).reshape(shape)
    best = np.zeros(shape, dtype=np.float32)
    arg = np.full(shape, -1, dtype=np.int64)
    for off in _offsets(nd, c):
        a, b = _pair(shape, off)
        conn = _conn(lab, fg, a, b, binary)
        with np.errstate(invalid="ignore"):
            upd = conn & ((arg[a] < 0) | (f[b] > best[a]))                       # strictly greater: the smallest idx wins a tie
        best[a] = np.where(upd, f[b], best[a])
        arg[a] = np.where(upd, idx[b], arg[a])
    with np.errstate(invalid="ignore"):
        top = fg & ~((arg >= 0) & (best > f))
    climb = fg & ~top
    rows, cols = [idx[climb]], [arg[climb]]
    for off in _offsets(nd, c):
        a, b = _pair(shape, off)
        with np.errstate(invalid="ignore"):
            e = _conn(lab, fg, a, b, binary) & top[a] & (f[b] == f[a])
        rows.append(idx[a][e])
        cols.append(idx[b][e])
    return _components(lab.size, rows, cols).reshape(shape), top, fg


def phase2(lab, f, comp, fg, c, binary, h):
    """The phase-1 basins joined by one round of saliency merges: a new id per voxel."""
    shape, nd = lab.shape, lab.ndim
    n = int(comp.max()) + 1
    peak = np.full(n, -np.inf, dtype=np.float32)
    np.maximum.at(peak, comp[fg], f[fg])
    h = np.float32(h)
    rows, cols = [], []
    for off in _offsets(nd, c, half=True):
        a, b = _pair(shape, off)
        with np.errstate(invalid="ignore"):
            bar = (np.minimum(peak[comp[a]], peak[comp[b]]) - h).astype(np.float32)   # one float32 subtraction
            e = _conn(lab, fg, a, b, binary) & (np.minimum(f[a], f[b]) >= bar)
        rows.append(comp[a][e])
        cols.append(comp[b][e])
    return _components(n, rows, cols)[comp]


def _arguments(labels, field, connectivity, binary):
    lab, transposed = _canonical(labels)
    f = np.asarray(field)
    assert f.shape == np.shape(labels) and f.dtype == np.float32
    f = np.ascontiguousarray(f.T if transposed else f)
    c = lab.ndim if connectivity is None else connectivity
    return lab, f, transposed, c, bool(binary) or lab.dtype == np.bool_


def watershed(labels, field, min_saliency=0.0, connectivity=None, binary=False, return_N=False, always_phase2=False):
    """The contract.  always_phase2: run phase 2 at min_saliency == 0 too (where it must change nothing)."""
    lab, f, transposed, c, binary = _arguments(labels, field, connectivity, binary)
    if lab.size == 0:
        out = np.zeros(np.shape(labels), dtype=np.uint32)
        return (out, 0) if return_N else out
    comp, _, fg = phase1(lab, f, c, binary)
    if min_saliency > 0 or always_phase2:
        comp = phase2(lab, f, comp, fg, c, binary, min_saliency)
    out, n = _number(comp, fg, lab.shape)
    out = out.T if transposed else out
    return (out, n) if return_N else out


def ladder(labels, field, saliencies, connectivity=None, binary=False):
    """[(out, N) for every min_saliency of `saliencies`]: the contract again, phase 1 computed once."""
    lab, f, transposed, c, binary = _arguments(labels, field, connectivity, binary)
    comp, _, fg = phase1(lab, f, c, binary)
    made = []
    for h in saliencies:
        out, n = _number(phase2(lab, f, comp, fg, c, binary, h) if h > 0 else comp, fg, lab.shape)
        made.append((out.T if transposed else out, n))
    return made


def regional_maxima(labels, field, connectivity=None, binary=False):
    """(ids, is_max): the plateaus -- components of neighbouring voxels of one object with equal field values --, numbered from 1
    in memory order (0: background), and for every plateau whether no voxel of it has a greater neighbour of one object."""
    lab, f, transposed, c, binary = _arguments(labels, field, connectivity, binary)
    shape, nd = lab.shape, lab.ndim
    with np.errstate(invalid="ignore"):
        fg = lab != 0
    idx = np.arange(lab.size, dtype=np.int64).reshape(shape)
    rows, cols = [], []
    lower = np.zeros(shape, dtype=bool)
    for off in _offsets(nd, c):
        a, b = _pair(shape, off)
        conn = _conn(lab, fg, a, b, binary)
        e = conn & (f[a] == f[b])
        rows.append(idx[a][e])
        cols.append(idx[b][e])
        lower[a] |= conn & (f[b] > f[a])
    ids, n = _number(_components(lab.size, rows, cols).reshape(shape), fg, shape)
    is_max = np.ones(n + 1, dtype=bool)
    is_max[ids[lower]] = False
    is_max[0] = False
    return (ids.T if transposed else ids), is_max


def naive(labels, field, min_saliency=0.0, connectivity=None, binary=False, always_phase2=False):
    """(out, N) voxel by voxel in Python, with a union-find of its own: tiny volumes only."""
    lab, f, transposed, c, binary = _arguments(labels, field, connectivity, binary)
    shape, nd, n = lab.shape, lab.ndim, lab.size
    L, F = lab.reshape(-1), f.reshape(-1)
    offs = [o for o in itertools.product((-1, 0, 1), repeat=nd) if 0 < sum(abs(v) for v in o) <= c]

    def neighbours(i):
        p = np.unravel_index(i, shape)
        found = []
        for o in offs:
            q = tuple(int(a + b) for a, b in zip(p, o))
            if all(0 <= v < s for v, s in zip(q, shape)):
                j = int(np.ravel_multi_index(q, shape))
                if L[i] != 0 and L[j] != 0 and (binary or L[i] == L[j]):
                    found.append(j)
        return sorted(found)

    def make():
        return list(range(n))

    def find(par, i):
        while par[i] != i:
            i = par[i]
        return i

    def union(par, i, j):
        i, j = find(par, i), find(par, j)
        par[max(i, j)] = min(i, j)

    fg = [bool(L[i] != 0) for i in range(n)]
    nb = [neighbours(i) if fg[i] else [] for i in range(n)]
    par = make()
    for i in range(n):
        if not nb[i]:
            continue
        m = nb[i][0]
        for j in nb[i][1:]:
            if F[j] > F[m]:
                m = j
        if F[m] > F[i]:
            union(par, i, m)
        else:
            for j in nb[i]:
                if F[j] == F[i]:
                    union(par, i, j)
    if min_saliency > 0 or always_phase2:
        basin = [find(par, i) for i in range(n)]
        peak = {}
        for i in range(n):
            if fg[i] and (basin[i] not in peak or F[i] > peak[basin[i]]):
                peak[basin[i]] = F[i]
        joined = make()
        h = np.float32(min_saliency)
        for i in range(n):
            for j in nb[i]:
                if basin[i] != basin[j] and min(F[i], F[j]) >= np.float32(min(peak[basin[i]], peak[basin[j]]) - h):
                    union(joined, basin[i], basin[j])
        par = [find(joined, b) for b in basin]
    out, number = np.zeros(n, dtype=np.uint32), {}
    for i in range(n):
        if fg[i]:
            out[i] = number.setdefault(find(par, i), len(number) + 1)
    out = out.reshape(shape)
    return (out.T if transposed else out), len(number)


# ---- the shapes of the issue that motivated min_saliency ---------------------------------------------------------------------
def diagonal_tube():
    """40^3: a tube of radius 4.3 and half-length 16 along (1, 2, 3) / sqrt(14) through (20, 20, 20)."""
    g = np.stack(np.meshgrid(*[np.arange(40.0)] * 3, indexing="ij"), axis=-1) - 20.0
    d = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    t = g @ d
    r = np.sqrt(np.maximum((g * g).sum(-1) - t * t, 0.0))
    return ((np.abs(t) <= 16.0) & (r <= 4.3)).astype(np.uint8)


def two_balls():
    """(40, 40, 64): balls of radius 14 and 13.5 about (20, 20, 20) and (19.5, 21, 43); they overlap."""
    z, y, x = np.meshgrid(np.arange(40.0), np.arange(40.0), np.arange(64.0), indexing="ij")
    a = (z - 20) ** 2 + (y - 20) ** 2 + (x - 20) ** 2 <= 14.0 ** 2
    b = (z - 19.5) ** 2 + (y - 21) ** 2 + (x - 43) ** 2 <= 13.5 ** 2
    return (a | b).astype(np.uint8)


def blob_mask(seed=0):
    """48 x 56 x 72: Gaussian noise smoothed at sigma = 4, thresholded at 0.01."""
    from scipy.ndimage import gaussian_filter
    noise = np.random.default_rng(seed).standard_normal((48, 56, 72))
    return (gaussian_filter(noise, 4.0) > 0.01).astype(np.uint8)
