"""Numpy oracle of local thickness (include/edt_hip.h, "local thickness") -- TEST INFRASTRUCTURE ONLY.

The contract over tests/morph_oracle.py, step by step: ``T = 0``; then for the radii in ascending order
``T[opening(labels, r, ...) != 0] = float32(r)``, with ``sizes[j]`` the voxel count of that opening.  The default ladder is
``j * step`` (fp64), ``step`` the smallest |voxel size| as fp32, over all ``j >= 1`` with ``(j * step) * (j * step) < Smax``,
``Smax`` the largest finite value of the field ``opening`` measures (morph_oracle.edtsq of the labels, or of their mask
under ``binary``), or 0.  Arrays may be C or Fortran contiguous; the result has the input's shape and memory order."""
from __future__ import annotations

import numpy as np

import morph_oracle


def measured_field(labels, anisotropy=None, black_border=False, binary=False):
    """S of the contract"""
    labels = np.asarray(labels)
    measured = morph_oracle.foreground(labels) if (binary or labels.dtype == np.bool_) else labels
    return morph_oracle.edtsq(measured, anisotropy, black_border)


def ladder_step(labels, anisotropy=None):
    an = (1.0,) * np.ndim(labels) if anisotropy is None else ((anisotropy,) if np.ndim(anisotropy) == 0 else tuple(anisotropy))
    return min(abs(float(np.float32(a))) for a in an)


def default_radii(labels, anisotropy=None, black_border=False, binary=False):
    S = measured_field(labels, anisotropy, black_border, binary)
    finite = S[np.isfinite(S)]
    smax = float(finite.max()) if finite.size else 0.0
    step = ladder_step(labels, anisotropy)
    radii, j = [], 1
    while (float(j) * step) * (float(j) * step) < smax:
        radii.append(float(j) * step)
        j += 1
    return np.array(radii, dtype=np.float64)


def openings(labels, radii, anisotropy=None, black_border=False, binary=False):
    """[O_j] as boolean arrays"""
    return [morph_oracle.opening(labels, float(r), anisotropy, black_border=black_border, binary=binary) != 0 for r in radii]


def local_thickness(labels, radii=None, anisotropy=None, black_border=False, binary=False, first_miss=False):
    """``(T, radii, sizes)``.  ``first_miss=True`` is the WRONG rule the contract rules out -- a voxel stops at the first opening
    that does not contain it --, kept to show that the test volumes tell the two apart."""
    labels = np.asarray(labels)
    radii = default_radii(labels, anisotropy, black_border, binary) if radii is None else np.asarray(radii, dtype=np.float64).reshape(-1)
    T = np.zeros(labels.shape, dtype=np.float32, order="F" if labels.flags.f_contiguous else "C")
    sizes = np.zeros(radii.size, dtype=np.int64)
    if labels.size == 0:
        return T, radii, sizes
    alive = np.ones(labels.shape, dtype=bool)
    for j, O in enumerate(openings(labels, radii, anisotropy, black_border, binary)):
        sizes[j] = np.count_nonzero(O)
        if first_miss:
            alive &= O
            O = alive
        T[O] = np.float32(radii[j])
    return T, radii, sizes
