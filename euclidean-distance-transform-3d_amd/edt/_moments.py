"""What ``edt.label_moments`` and ``edt.device.label_moments`` share: the result type, the range bound of the ABI and the
mapping of its x / y / z columns to array axes (numpy arrays and torch tensors alike)."""
from __future__ import annotations

import collections

import numpy as np

# columns of the ABI's `sums` (after the three first moments) and `central`: the pair (a, b) of x / y / z axes
_PAIR = {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (1, 0): 3, (0, 2): 4, (2, 0): 4, (1, 2): 5, (2, 1): 5}


class LabelMoments(collections.namedtuple("LabelMoments", ["labels", "counts", "first", "second", "centroid", "covariance"])):
    """One row per distinct non-zero label, every field per ARRAY axis: the label values ascending, the voxel count (int64),
    the exact raw moments about the array's origin in voxel index units -- ``first[i, a]`` the sum of the coordinate along
    axis a, ``second[i, a, b]`` the sum of the products of the coordinates along a and b (int64, symmetric) -- the centroid
    ``(n, ndim)`` and the population covariance ``(n, ndim, ndim)`` in voxel units (float64; contract and rounding:
    include/edt_hip.h, "label_moments")."""
    __slots__ = ()

    def principal(self, anisotropy=None):
        """``(lengths2, axes)`` of every label from ``numpy.linalg.eigh`` of its covariance in physical units
        (``covariance[a][b] * w_a * w_b``, ``anisotropy`` = the voxel size per array axis, default 1): ``lengths2[i, k]`` the
        k-th LARGEST eigenvalue -- the variance along the k-th principal axis -- and ``axes[i, k]`` that axis as a unit vector
        over the array axes (its sign is arbitrary).  The table is small, so this step runs on the host: a device result
        (``edt.device.label_moments``) is brought to the host for it, and numpy arrays are returned either way."""
        cov = self.covariance
        cov = cov.cpu().numpy() if hasattr(cov, "cpu") else np.asarray(cov)
        nd = cov.shape[-1]
        w = np.ones(nd) if anisotropy is None else np.broadcast_to(np.asarray(anisotropy, dtype=np.float64), (nd,))
        if not np.all(np.isfinite(w)) or np.any(w == 0):
            raise ValueError(f"principal: voxel sizes must be non-zero and finite, got {anisotropy!r}")
        vals, vecs = np.linalg.eigh(cov * (w[:, None] * w[None, :]))
        return np.ascontiguousarray(vals[:, ::-1]), np.ascontiguousarray(np.swapaxes(vecs, 1, 2)[:, ::-1])


def check_range(shape):
    """The ABI's range bound, as a ValueError: below it every sum fits int64."""
    voxels, e = 1, 0
    for s in shape:
        voxels, e = voxels * int(s), max(e, int(s))
    if e > 1 and voxels * (e - 1) ** 2 >= 1 << 63:
        raise ValueError(f"label_moments: voxels * (largest extent - 1)^2 must stay below 2^63 for exact int64 moments, "
                         f"got shape {tuple(shape)}")


def assemble(keys, counts, sums, centroid, central, nd, x_is_last):
    """The ABI's table (x / y / z columns; rows already cut and ordered) as a LabelMoments per array axis.  x_is_last: the
    array's LAST axis runs fastest (C order, torch tensors); else its first."""
    axis = list(range(nd))[::-1] if x_is_last else list(range(nd))   # array axis -> x / y / z
    pairs = [_PAIR[(axis[a], axis[b])] for a in range(nd) for b in range(nd)]
    n = len(keys)
    first = sums[:, axis]
    second = sums[:, [3 + p for p in pairs]].reshape(n, nd, nd)
    return LabelMoments(keys, counts, first, second, centroid[:, axis], central[:, pairs].reshape(n, nd, nd))
