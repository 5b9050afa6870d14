"""Numpy oracle of the morphology operations (include/edt_hip.h, "morphology") -- TEST INFRASTRUCTURE ONLY.

A restatement of the contract, step by step.  The squared-distance fields come from the project's CPU transform
(oracle.harness.port(), bit-identical to the reference); every comparison is ``field.astype(float64) > R2`` or ``<= R2``
with ``R2 = float64(radius) * float64(radius)``.  expand_labels is restated from the header's definition over the
feature-transform oracle (tests/ft_oracle.py), so dilate and closing are served for voxel sizes whose squares are exact in
fp32 (w_i^2 = a_i q with integer a_i, ft_oracle.exact_factors: the sizes that share a quantum, and those the library refuses
one for because an a_i is too large for its 16-bit windows -- the fp64 kernels are exact there), and for tiny volumes only:
that oracle is pure Python loops over lines.

Arrays may be C or Fortran contiguous: the transforms and the tie rule of expand_labels follow the array's memory order, as the
library's do (x is the fastest axis of memory; an array that is both is taken as Fortran, as in edt/__init__.py).  Outputs have
the input's dtype, shape and memory order; voxels that do not pass are all-zero bits, the others are copied bit for bit."""
from __future__ import annotations

import numpy as np

import ft_oracle


def _port():
    from oracle import harness
    if not harness.have_port():
        harness.build("port")
    return harness.port()


def r2_of(radius):
    return np.float64(radius) * np.float64(radius)


def _anisotropy(data, anisotropy):
    if anisotropy is None:
        return (1.0,) * data.ndim
    return (float(anisotropy),) if np.ndim(anisotropy) == 0 else tuple(float(a) for a in anisotropy)


def edtsq(data, anisotropy=None, black_border=False):
    """the field edt_hip_edtsq_device writes for ``data`` (fp32), in the array's layout"""
    an = _anisotropy(data, anisotropy)
    return _port().edtsq(data, an[0] if data.ndim == 1 else an, black_border)


def foreground(data):
    """m[p] = (labels[p] != 0) as uint8, in the array's memory order: -0.0 is background, a NaN is foreground"""
    return (data != 0).astype(np.uint8, order="K")


def _select(values, passes):
    out = np.zeros_like(values)           # (memory order kept; all-zero bits)
    out[passes] = values[passes]          # (bit for bit: a NaN keeps its payload)
    return out


def _survives(labels, radius, anisotropy, black_border, binary):
    measured = foreground(labels) if (binary or labels.dtype == np.bool_) else labels
    return edtsq(measured, anisotropy, black_border).astype(np.float64) > r2_of(radius)


def erode(labels, radius=1.0, anisotropy=None, black_border=False, binary=False):
    labels = np.asarray(labels)
    if labels.size == 0:
        return labels.copy()
    return _select(labels, _survives(labels, radius, anisotropy, black_border, binary))


def opening(labels, radius=1.0, anisotropy=None, black_border=False, binary=False):
    labels = np.asarray(labels)
    if labels.size == 0:
        return labels.copy()
    z = (~_survives(labels, radius, anisotropy, black_border, binary)).astype(np.uint8, order="K")
    B = edtsq(z, anisotropy, False)
    return _select(labels, B.astype(np.float64) <= r2_of(radius))


def _quantum_factors(w_xyz):
    """integer a_i with w_i^2 = a_i q for the fp32 voxel sizes ``w_xyz`` (AssertionError if a square is not exact in fp32)"""
    return list(ft_oracle.exact_factors(w_xyz))


def expand_labels(labels, distance=1.0, anisotropy=None):
    """out = labels; a background voxel p takes labels[f] if its feature f in the feature transform of the mask labels == 0
    (no border) exists and D(p, f) <= distance^2, D = (fl64(wx^2 dx^2) + fl64(wy^2 dy^2)) + fl64(wz^2 dz^2)"""
    labels = np.asarray(labels)
    if labels.size == 0:
        return labels.copy()
    nd = labels.ndim
    an = _anisotropy(labels, anisotropy)
    fortran = labels.flags.f_contiguous
    xyz = labels if fortran else labels.T                     # x first
    w = tuple(an if fortran else an[::-1]) + (1.0,) * (3 - nd)
    lab3 = xyz.reshape(xyz.shape + (1,) * (3 - nd))
    f, _ = ft_oracle.feature_transform((lab3 == 0).astype(np.uint8), _quantum_factors(w), False, ndim=nd)
    grids = np.meshgrid(*[np.arange(s) for s in lab3.shape], indexing="ij")
    D = np.zeros(lab3.shape)
    for k in range(3):                                          # terms added in ABI order x, y, z
        w2 = np.float64(np.float32(w[k])) * np.float64(np.float32(w[k]))
        D = D + w2 * ((grids[k] - f[k]).astype(np.int64) ** 2).astype(np.float64)
    has = ~np.all(f == -1, axis=0)
    take = (lab3 == 0) & has & (D <= r2_of(distance))
    src = tuple(np.where(take, f[k], 0) for k in range(3))
    out3 = lab3.copy()
    out3[take] = lab3[src][take]
    out = np.zeros_like(labels)
    (out if fortran else out.T)[...] = out3.reshape(xyz.shape)
    return out


dilate = expand_labels


def closing(labels, radius=1.0, anisotropy=None):
    labels = np.asarray(labels)
    if labels.size == 0:
        return labels.copy()
    D = expand_labels(labels, radius, anisotropy)
    C = edtsq(foreground(D), anisotropy, False)
    return _select(D, (labels != 0) | (C.astype(np.float64) > r2_of(radius)))


def ball(radius, ndim):
    """the isotropic structuring element of scipy's binary morphology: the offsets with |d|^2 <= radius^2"""
    k = int(np.floor(radius))
    ax = np.arange(-k, k + 1)
    g = np.meshgrid(*[ax] * ndim, indexing="ij")
    return sum(v.astype(np.float64) ** 2 for v in g) <= r2_of(radius)
