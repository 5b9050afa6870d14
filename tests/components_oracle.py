"""The contract of connected_components (include/edt_hip.h, "connected components") restated in numpy: min-propagation of the
memory index over the neighbour offsets with connected labels until nothing changes, then the surviving roots numbered in
ascending order.  Also a brute-force flood fill for tiny volumes, so that the oracle does not rest on scipy alone."""
import itertools

import numpy as np


def offsets(ndim, connectivity):
    """Half of the neighbour offsets (the lexicographically positive ones): at most `connectivity` non-zero entries."""
    return [o for o in itertools.product((-1, 0, 1), repeat=ndim) if 0 < sum(map(abs, o)) <= connectivity and o > (0,) * ndim]


def _order(data):
    return "F" if data.flags.f_contiguous else "C"   # (both: F, as in every entry point of the module)


def _pair(shape, off):
    a = tuple(slice(max(0, -o), s - max(0, o)) for o, s in zip(off, shape))
    b = tuple(slice(max(0, o), s - max(0, -o)) for o, s in zip(off, shape))
    return a, b


def connected_components(data, connectivity=None, binary=False, return_N=False):
    data = np.asarray(data)
    if not data.flags.c_contiguous and not data.flags.f_contiguous:
        data = np.ascontiguousarray(data)
    nd, order = data.ndim, _order(data)
    c = nd if connectivity is None else connectivity
    with np.errstate(invalid="ignore"):
        fg = data != 0                                     # -0.0 is background, NaN is foreground
    binary = binary or data.dtype == np.bool_
    big = data.size
    par = np.where(fg.reshape(-1, order=order), np.arange(data.size, dtype=np.int64), big)   # memory order
    pv = par.reshape(data.shape, order=order)              # a view
    links = []
    for off in offsets(nd, c):
        a, b = _pair(data.shape, off)
        with np.errstate(invalid="ignore"):
            conn = fg[a] & fg[b] & (True if binary else data[a] == data[b])    # NaN equals nothing
        links.append((a, b, conn))
    while True:
        before = par.copy()
        for a, b, conn in links:
            m = np.where(conn, np.minimum(pv[a], pv[b]), big)
            pv[a] = np.minimum(pv[a], m)                   # (the two views overlap: only ever lower a parent)
            pv[b] = np.minimum(pv[b], m)
        live = par < big
        par[live] = par[par[live]]                         # pointer jumping: long chains in O(log) rounds
        if np.array_equal(par, before):
            break
    roots = np.unique(par[par < big])
    out = np.where(par < big, np.searchsorted(roots, par) + 1, 0).astype(np.uint32).reshape(data.shape, order=order)
    return (out, len(roots)) if return_N else out


def flood_fill(data, connectivity=None, binary=False):
    """(out, N) by a stack-based flood fill from every unvisited foreground voxel in memory order: tiny volumes only."""
    data = np.asarray(data)
    nd, order = data.ndim, _order(data)
    c = nd if connectivity is None else connectivity
    binary = binary or data.dtype == np.bool_
    offs = [o for o in itertools.product((-1, 0, 1), repeat=nd) if 0 < sum(map(abs, o)) <= c]
    out = np.zeros(data.shape, dtype=np.uint32, order=order)
    n = 0
    for flat in range(data.size):
        p = np.unravel_index(flat, data.shape, order=order)
        if not data[p] != 0 or out[p]:
            continue
        n += 1
        out[p] = n
        stack = [p]
        while stack:
            q = stack.pop()
            for o in offs:
                r = tuple(int(i + j) for i, j in zip(q, o))
                if any(i < 0 or i >= s for i, s in zip(r, data.shape)) or out[r] or not data[r] != 0:
                    continue
                if binary or data[r] == data[q]:
                    out[r] = n
                    stack.append(r)
    return out, n
