"""The contract of dust (include/edt_hip.h, "dust") restated in numpy over the components of tests/components_oracle.py: the size
of every component by a bincount of its number, the test  min_voxels <= size < max_voxels  (the complement under `invert`), and
the voxels of the components that fail it set to all-zero bits.  Background is copied as it is, so -0.0 keeps its sign."""
import collections

import numpy as np

import components_oracle

Dusted = collections.namedtuple("Dusted", ["out", "components", "kept", "removed_voxels"])
NO_UPPER_BOUND = (1 << 63) - 1


def bounds(threshold):
    """(min_voxels, max_voxels): an integer t removes sizes below t, a pair (lo, hi) keeps lo <= size < hi."""
    if isinstance(threshold, (tuple, list)):
        return int(threshold[0]), int(threshold[1])
    return int(threshold), NO_UPPER_BOUND


def sizes(data, connectivity=None, binary=False):
    """(comp, sizes): the component numbers of the oracle and sizes[k] = voxels of component k (sizes[0] = 0)."""
    comp, n = components_oracle.connected_components(data, connectivity, binary=binary, return_N=True)
    size = np.bincount(comp.reshape(-1).astype(np.int64), minlength=n + 1)
    size[0] = 0
    return comp, size


def dust(data, threshold, connectivity=None, binary=False, invert=False):
    """Dusted(out, components, kept, removed_voxels)."""
    data = np.asarray(data)
    if not data.flags.c_contiguous and not data.flags.f_contiguous:
        data = np.ascontiguousarray(data)
    order = components_oracle._order(data)
    out = data.copy(order=order)
    if data.size == 0:
        return Dusted(out, 0, 0, 0)
    lo, hi = bounds(threshold)
    comp, size = sizes(data, connectivity, binary)
    keep = (size >= lo) & (size < hi)
    if invert:
        keep = ~keep
    keep[0] = True                                         # background is not a component: copied as it is
    gone = ~keep[comp]
    out[gone] = np.zeros((), dtype=data.dtype)             # all-zero bits: 0, +0.0, False
    return Dusted(out, len(size) - 1, int(np.count_nonzero(keep[1:])), int(np.count_nonzero(gone)))


def sparse_volume(seed, p, labels=3, shape=(70, 12, 9)):
    """The random volume of both tiers: F order (axis 0 is x), uint32, a voxel set with probability p, then its label drawn from
    1..labels."""
    rng = np.random.default_rng(seed)
    mask = rng.random(shape) < p
    lab = np.zeros(shape, dtype=np.uint32)
    lab[mask] = rng.integers(1, labels + 1, size=int(np.count_nonzero(mask)))
    return np.asfortranarray(lab)


def in_range(data, lo, hi, connectivity=None, binary=False):
    """The number of components with lo <= size < hi."""
    _, size = sizes(data, connectivity, binary)
    return int(np.count_nonzero((size[1:] >= lo) & (size[1:] < hi)))
