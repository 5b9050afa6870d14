"""What ``edt.label_topology`` and ``edt.device.label_topology`` share: the result type, the mapping of the ABI's 3-bit cell
types to array axes (numpy arrays and torch tensors alike) and the exact arithmetic of the derived quantities."""
from __future__ import annotations

import collections
import fractions
import itertools

import numpy as np


class LabelTopology(collections.namedtuple("LabelTopology", ["labels", "counts", "closed", "interior"])):
    """One row per distinct non-zero label: the label values ascending, the voxel count (int64) and the two cell-count tables
    (int64, shape ``(n,) + (2,) * ndim``, indexed per ARRAY axis: index 1 means the cell extends along that axis, so
    ``[..., 0, 0, 0]`` are vertices and ``[..., 1, 1, 1]`` the voxels themselves).  ``closed`` counts the cells with at least
    one incident voxel of the label (full adjacency), ``interior`` the cells whose incident voxels all carry it (face
    adjacency); positions outside the array hold no label (contract: include/edt_hip.h, "label_topology").  The table is small,
    so the methods run on the host: a device result is brought there, and numpy arrays are returned either way."""
    __slots__ = ()

    def _host(self, field):
        return field.cpu().numpy() if hasattr(field, "cpu") else np.asarray(field)

    def euler(self, connectivity=None):
        """The Euler number of every label, int64 ``(n,)``: components - tunnels + cavities in 3-D, components - holes in 2-D.
        ``connectivity`` in the spelling of ``connected_components`` (default: full, ``ndim``).  Only 1 (faces: 4 / 6
        neighbours, from ``interior``) and ``ndim`` (8 / 26 neighbours, from ``closed``) are defined."""
        from . import _connectivity
        closed = self._host(self.closed)
        nd = closed.ndim - 1
        c = _connectivity(connectivity, nd, who="euler")
        if c not in (1, nd):
            raise ValueError(f"euler: the cell counts define the Euler number for connectivity 1 and {nd} only, not for the "
                             f"adjacency between them, got {connectivity!r}")
        table = closed if c == nd else self._host(self.interior)
        out = np.zeros(len(table), dtype=np.int64)
        for idx in itertools.product((0, 1), repeat=nd):
            dim = sum(idx)
            sign = (-1) ** dim if c == nd else (-1) ** (nd - dim)
            out += sign * table[(slice(None),) + idx]
        return out

    def _volumes_exact(self, anisotropy):
        """``V[i][j]`` as exact Python integers or fractions (an object array ``(n, ndim + 1)``)"""
        closed = self._host(self.closed)
        nd = closed.ndim - 1
        w = [1] * nd if anisotropy is None else list(np.broadcast_to(np.asarray(anisotropy), (nd,)).tolist())
        if not all(isinstance(v, (int, float)) and not isinstance(v, bool) and np.isfinite(v) and v > 0 for v in w):
            raise ValueError(f"intrinsic_volumes: voxel sizes must be positive and finite, got {anisotropy!r}")
        w = [int(v) if float(v).is_integer() else fractions.Fraction(v) for v in w]   # (a float is an exact fraction)
        out = np.zeros((len(closed), nd + 1), dtype=object)
        for idx in itertools.product((0, 1), repeat=nd):
            axes = [a for a in range(nd) if idx[a]]
            column = closed[(slice(None),) + idx].astype(object)
            for j in range(len(axes) + 1):
                e_j = sum(_product(w[a] for a in pick) for pick in itertools.combinations(axes, j))
                out[:, j] += (-1) ** (len(axes) - j) * e_j * column
        return out

    def intrinsic_volumes(self, anisotropy=None):
        """The intrinsic volumes ``V_0 .. V_ndim`` of every label for the voxel sizes ``anisotropy`` (per array axis, default
        1), float64 ``(n, ndim + 1)``: ``V_ndim`` the volume, ``2 * V_(ndim-1)`` the area of the exposed voxel faces, ``V_1``
        the mean-breadth functional, ``V_0`` the Euler number (full adjacency).  Computed exactly -- in Python integers for
        integer voxel sizes, else in fractions -- and rounded once."""
        exact = self._volumes_exact(anisotropy)
        return np.array([[float(v) for v in row] for row in exact], dtype=np.float64).reshape(exact.shape)

    def surface_area(self, anisotropy=None):
        """``2 * V_(ndim-1)``, float64 ``(n,)``: the total area of the VOXEL FACES between the label and anything else, the
        array's edge included (the perimeter in 2-D).  It is exact and additive, and it is not an estimate of a smooth
        surface's area, to which it does not converge: for a ball it is about 1.5 times larger."""
        exact = self._volumes_exact(anisotropy)
        return np.array([float(2 * row[-2]) for row in exact], dtype=np.float64)


def _product(values):
    out = 1
    for v in values:
        out = out * v
    return out


def assemble(keys, closed, interior, nd, x_is_last):
    """The ABI's table (eight columns per table, bit 0 = x; rows already cut and ordered) as a LabelTopology per array axis.
    For a missing axis the slab's count with that axis' bit set is the image's.  x_is_last: the array's LAST axis runs fastest
    (C order, torch tensors); else its first."""
    xyz = list(range(nd))[::-1] if x_is_last else list(range(nd))   # array axis -> x / y / z
    missing = sum(1 << a for a in range(nd, 3))
    cols = [missing | sum(1 << xyz[a] for a in range(nd) if idx[a]) for idx in itertools.product((0, 1), repeat=nd)]
    shape = (len(keys),) + (2,) * nd
    return LabelTopology(keys, closed[:, 7], closed[:, cols].reshape(shape), interior[:, cols].reshape(shape))
