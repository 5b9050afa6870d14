"""The contract of fill_holes (include/edt_hip.h, "fill holes") restated in numpy: the components of the background under the
connectivity (tests/components_oracle.py), those that touch the array's boundary struck out, the wall of every remaining one
gathered pair by pair over the neighbour offsets, its voxel of smallest memory index as the representative, and the fill where
every wall label equals the representative's (or always, under `binary`).  Also a brute-force flood fill from the boundary for
tiny volumes, so that the oracle does not rest on one method alone."""
import collections
import itertools

import numpy as np

import components_oracle

Filled = collections.namedtuple("Filled", ["out", "n_filled", "cavities", "filled_cavities", "mixed_cavities"])


def all_offsets(ndim, connectivity):
    return [o for o in itertools.product((-1, 0, 1), repeat=ndim) if 0 < sum(map(abs, o)) <= connectivity]


def _prepare(data, connectivity, binary):
    data = np.asarray(data)
    if not data.flags.c_contiguous and not data.flags.f_contiguous:
        data = np.ascontiguousarray(data)
    order = components_oracle._order(data)
    c = 1 if connectivity is None else connectivity
    with np.errstate(invalid="ignore"):
        bg = ~(data != 0)                                   # -0.0 is background, NaN is foreground
    return data, order, c, bg, bool(binary) or data.dtype == np.bool_


def boundary_mask(shape):
    edge = np.zeros(shape, dtype=bool)
    for axis, s in enumerate(shape):
        sl = [slice(None)] * len(shape)
        for k in (0, s - 1):
            sl[axis] = k
            edge[tuple(sl)] = True
    return edge


def fill_holes(data, connectivity=None, binary=False):
    """Filled(out, n_filled, cavities, filled_cavities, mixed_cavities); mixed cavities are those left 0 for their wall."""
    data, order, c, bg, binary = _prepare(data, connectivity, binary)
    out = data.copy(order=order)
    if data.size == 0:
        return Filled(out, 0, 0, 0, 0)
    comp, n = components_oracle.connected_components(np.array(bg, order=order), c, binary=True, return_N=True)
    comp = comp.astype(np.int64)
    closed = np.ones(n + 1, dtype=bool)
    closed[0] = False
    closed[comp[boundary_mask(data.shape) & bg]] = False
    idx = np.arange(data.size, dtype=np.int64).reshape(data.shape, order=order)     # memory order
    flat = data.reshape(-1, order=order)
    pairs = []
    rep = np.full(n + 1, data.size, dtype=np.int64)
    for off in all_offsets(data.ndim, c):
        a, b = components_oracle._pair(data.shape, off)      # b = a + off
        m = bg[a] & ~bg[b]
        k, q = comp[a][m], idx[b][m]
        np.minimum.at(rep, k, q)
        pairs.append((k, q))
    assert np.all(rep[1:][closed[1:]] < data.size)           # a cavity always has a wall
    mixed = np.zeros(n + 1, dtype=bool)
    if not binary:
        for k, q in pairs:
            live = closed[k]
            with np.errstate(invalid="ignore"):
                differs = flat[q[live]] != flat[rep[k[live]]]      # a NaN differs from everything, itself included
            mixed[k[live][differs]] = True
    fill = closed & ~mixed
    sel = fill[comp]
    out[sel] = flat[rep[comp[sel]]]
    return Filled(out, int(np.count_nonzero(sel)), int(np.count_nonzero(closed)), int(np.count_nonzero(fill)),
                  int(np.count_nonzero(closed & mixed)))


def brute_force(data, connectivity=None, binary=False):
    """The same by flooding the background from the array's boundary, then every remaining background voxel in turn: tiny
    volumes only."""
    data, order, c, bg, binary = _prepare(data, connectivity, binary)
    offs = all_offsets(data.ndim, c)
    shape = data.shape
    out = data.copy(order=order)
    seen = np.zeros(shape, dtype=bool)

    def inside(r):
        return all(0 <= i < s for i, s in zip(r, shape))

    def flood(start):
        seen[start] = True
        stack, members, wall = [start], [], set()
        while stack:
            p = stack.pop()
            members.append(p)
            for o in offs:
                r = tuple(int(i + j) for i, j in zip(p, o))
                if not inside(r):
                    continue
                if not bg[r]:
                    wall.add(r)
                elif not seen[r]:
                    seen[r] = True
                    stack.append(r)
        return members, wall

    for p in zip(*np.nonzero(boundary_mask(shape) & bg)):
        if not seen[p]:
            flood(tuple(int(v) for v in p))
    n_filled = cavities = filled = mixed = 0
    for p in zip(*np.nonzero(bg)):
        p = tuple(int(v) for v in p)
        if seen[p]:
            continue
        members, wall = flood(p)
        cavities += 1
        first = min(wall, key=lambda r: np.ravel_multi_index(r, shape, order=order))
        with np.errstate(invalid="ignore"):
            same = all(data[r] == data[first] for r in wall)
        if binary or same:
            filled += 1
            n_filled += len(members)
            for r in members:
                out[r] = data[first]
        else:
            mixed += 1
    return Filled(out, n_filled, cavities, filled, mixed)


def random_volume(seed):
    """The random multi-label volume of both tiers: 18 x 18 x 12 (x fastest), 3 labels in blocks of 6, 8 % of the voxels zeroed."""
    from synth import blocky_labels
    rng = np.random.default_rng(seed)
    lab = blocky_labels((18, 18, 12), nlabels=3, zero_frac=0.0, block=6, rng=rng).astype(np.uint32)
    lab[rng.random(lab.shape) < 0.08] = 0
    return np.asfortranarray(lab)
