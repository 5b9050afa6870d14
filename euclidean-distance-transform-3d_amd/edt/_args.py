"""The argument rules the two Python layers share: :mod:`edt` (numpy arrays) and :mod:`edt.device` (device tensors) refuse and
convert the arguments of one operation in one place.  numpy only: no torch, no library call."""
from __future__ import annotations

import collections
import math

import numpy as np

from . import _lib
from ._moments import LabelMoments
from ._topology import LabelTopology

LabelStats = collections.namedtuple("LabelStats", ["labels", "counts", "max", "argmax", "bbox_lo", "bbox_hi"])
DustCounts = collections.namedtuple("DustCounts", ["components", "kept", "removed_voxels"])
ThicknessSizes = collections.namedtuple("ThicknessSizes", ["radii", "voxels"])

# numpy's dtypes: the code of include/edt_hip.h a label dtype has, and the dtype under which the kernels read a code
# (signed -> unsigned, bool -> bytes); edt.device has torch's
_DTYPE_CODE = {
    np.dtype(np.uint8): _lib.U8, np.dtype(np.int8): _lib.U8,
    np.dtype(np.uint16): _lib.U16, np.dtype(np.int16): _lib.U16,
    np.dtype(np.uint32): _lib.U32, np.dtype(np.int32): _lib.U32,
    np.dtype(np.uint64): _lib.U64, np.dtype(np.int64): _lib.U64,
    np.dtype(np.float32): _lib.F32, np.dtype(np.float64): _lib.F64,
    np.dtype(bool): _lib.BOOL,
}
_NP_OF_CODE = {code: np.dtype(np.uint8) if code == _lib.BOOL else dtype for dtype, code in _DTYPE_CODE.items() if dtype.kind != "i"}


def _check_ndim(who, ndim, what="arrays"):
    if ndim < 1 or ndim > 3:
        raise TypeError(f"{who}: 1-D, 2-D or 3-D {what}, got {ndim}-D")


def _check_max_labels(who, max_labels):
    if max_labels is not None and int(max_labels) < 1:
        raise ValueError(f"{who}: max_labels must be at least 1, got {max_labels}")


def _xyz(shape, sizes, ndim, x_last=True):
    """The x-fastest extents and voxel sizes of the C ABI, both padded to three, from a shape in memory order and the voxel
    size of every axis (``None``: 1.0 each; rounded to float32, what the ABI takes; a ``ValueError`` unless there are ``ndim``).
    ``x_last``: x is the LAST axis (C order, device tensors) and both are reversed; otherwise it is the first (Fortran order)."""
    if sizes is None:
        sizes = (1.0,) * ndim
    elif len(sizes) != ndim:
        raise ValueError(f"anisotropy must have {ndim} entries, got {len(sizes)}")
    else:
        sizes = tuple(float(np.float32(a)) for a in sizes)
    extents = tuple(shape)
    if x_last:
        extents, sizes = extents[::-1], sizes[::-1]
    return extents + (1,) * (3 - ndim), sizes + (1.0,) * (3 - ndim)


def _label_table(who, code, voxels, max_labels, attempt):
    """What label_stats, label_moments and label_topology do around their library call: the capacity (``max_labels``, or the
    default rule) and the call -- retried with 8x the room while a default capacity proves too small, a ``ValueError`` if an
    explicit one does.  ``attempt(cap)`` allocates columns of ``cap`` rows, calls, and returns ``(labels found, columns)``.
    Returns the columns cut to the labels found."""
    cap = _lib.default_max_labels(code, voxels)[0] if max_labels is None else min(int(max_labels), voxels)
    while True:
        n, cols = attempt(cap)
        if n <= cap:
            return [c[:n] for c in cols]
        if max_labels is not None:
            raise ValueError(f"{who}: more than max_labels = {int(max_labels)} distinct non-zero labels")
        cap = min(voxels, 8 * cap)


# the columns of a table without rows: (dtype name, shape behind the row axis as a function of ndim); None: the labels' dtype
_EMPTY = {
    LabelStats: [(None, 0), ("int64", 0), ("float32", 0), ("int64", 1), ("int32", 1), ("int32", 1)],
    LabelMoments: [(None, 0), ("int64", 0), ("int64", 1), ("int64", 2), ("float64", 1), ("float64", 2)],
    LabelTopology: [(None, 0), ("int64", 0), ("int64", -1), ("int64", -1)],
}


def _empty_table(cls, ndim, zeros):
    """The table of a volume without voxels.  ``zeros(dtype name or None, shape)``: the layer's own allocation."""
    return cls(*[zeros(name, (0,) + ((2,) * ndim if k < 0 else (ndim,) * k)) for name, k in _EMPTY[cls]])


_NEIGHBOUR_COUNTS = {2: {4: 1, 8: 2}, 3: {6: 1, 18: 2, 26: 3}}   # cc3d's spelling of the connectivity


def _connectivity(connectivity, ndim, default=None, who="connected_components"):
    """The ABI's connectivity (1..ndim) of a call: None is `default` (itself None: full); 1..ndim as in skimage; cc3d's
    neighbour counts 4 / 8 (2-D) and 6 / 18 / 26 (3-D).  Anything else is a ValueError."""
    if connectivity is None:
        return ndim if default is None else default
    if isinstance(connectivity, (int, np.integer)) and not isinstance(connectivity, (bool, np.bool_)):
        c = int(connectivity)
        if 1 <= c <= ndim:
            return c
        if c in _NEIGHBOUR_COUNTS.get(ndim, {}):
            return _NEIGHBOUR_COUNTS[ndim][c]
    raise ValueError(f"{who}: connectivity of a {ndim}-D array is None, 1..{ndim}"
                     + (f" or one of {sorted(_NEIGHBOUR_COUNTS[ndim])}" if ndim in _NEIGHBOUR_COUNTS else "")
                     + f", got {connectivity!r}")


_NO_UPPER_BOUND = (1 << 63) - 1          # INT64_MAX: the ABI's "no upper bound"


def _dust_bounds(threshold):
    """(min_voxels, max_voxels) of the ABI from `threshold`: an integer t (sizes below t are removed) or a pair (lo, hi)
    (lo <= size < hi is kept).  Anything else, a negative value or hi < lo is a ValueError."""
    def integer(v):
        return (isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
                and 0 <= int(v) <= _NO_UPPER_BOUND)

    if integer(threshold):
        return int(threshold), _NO_UPPER_BOUND
    if (isinstance(threshold, (tuple, list)) and len(threshold) == 2 and integer(threshold[0]) and integer(threshold[1])
            and int(threshold[0]) <= int(threshold[1])):
        return int(threshold[0]), int(threshold[1])
    raise ValueError(f"dust: threshold is a non-negative integer or a pair (lo, hi) of them with lo <= hi, got {threshold!r}")


def _min_saliency(min_saliency):
    """min_saliency as the float32 the ABI takes: finite and >= 0, else ValueError."""
    try:
        with np.errstate(over="ignore"):
            h = float(np.float32(min_saliency))
    except (TypeError, ValueError):
        h = math.nan
    if isinstance(min_saliency, (bool, np.bool_)) or not (h >= 0.0 and math.isfinite(h)):
        raise ValueError(f"watershed: min_saliency must be finite (as float32) and >= 0, got {min_saliency!r}")
    return h


def _morph_radius(radius, who, inf_allowed=False):
    """The radius of a morphology call as a float: >= 0 with a finite square (``inf_allowed``: or +inf itself), else ValueError."""
    r = float(radius)
    if not r >= 0.0 or not (np.isfinite(r * r) or (inf_allowed and r == np.inf)):
        raise ValueError(f"{who}: radius must be >= 0 and its square finite" + (" (+inf allowed)" if inf_allowed else "")
                         + f", got {radius!r}")
    return r


def _morph_flags(black_border, binary):
    return (_lib.FLAG_BLACK_BORDER if black_border else 0) | (_lib.FLAG_MORPH_BINARY if binary else 0)


def _thickness_radii(radii, who="local_thickness"):
    """The radii of a local_thickness call as a float64 array: at least one, each > 0 with a finite square (``_morph_radius``),
    strictly ascending; anything else is a ValueError."""
    try:
        r = np.array([_morph_radius(v, who) for v in np.asarray(radii, dtype=np.float64).reshape(-1)], dtype=np.float64)
    except TypeError:
        raise ValueError(f"{who}: radii must be numbers, got {radii!r}") from None
    if r.size < 1 or not (r > 0.0).all() or not (np.diff(r) > 0.0).all():
        raise ValueError(f"{who}: radii must be at least one, > 0 and strictly ascending, got {radii!r}")
    return r


def _ladder_room(extents, w):
    """``(step, room)`` of the default ladder r_j = j * step: step is the smallest |voxel size|, and no ladder is longer than
    ``room``, because S <= sum_i (w_i (n_i + 1))^2 and the ladder ends where r_j^2 reaches the largest finite S."""
    step = min(abs(float(v)) for v in w)
    bound = sum((abs(float(v)) * (int(n) + 1)) ** 2 for v, n in zip(w, extents))
    return step, int(np.sqrt(bound) / step) + 2


def _medial_ratio(min_angle, who="medial_axis"):
    """The angle pruning of a medial_axis call, ``min_angle`` in degrees in [0, 180), as the ``ratio`` of the C ABI:
    ``tan(radians(a) / 2) ** 2`` (0 switches it off); anything else is a ValueError.  Both Python layers convert here."""
    try:
        a = float(min_angle)
    except TypeError:
        raise ValueError(f"{who}: min_angle must be a number, got {min_angle!r}") from None
    if not (0.0 <= a < 180.0):
        raise ValueError(f"{who}: min_angle must be in [0, 180) degrees, got {min_angle!r}")
    ratio = math.tan(math.radians(a) / 2.0) ** 2
    if not np.isfinite(ratio):
        raise ValueError(f"{who}: min_angle {min_angle!r} is too close to 180 degrees")
    return ratio


def _medial_gamma(gamma, w, who="medial_axis"):
    """The constant pruning of a medial_axis call as a float: ``None`` is the largest |voxel size| (the paper's "features more
    than one voxel apart"); otherwise finite, >= 0 and with a finite square, else ValueError."""
    if gamma is None:
        return max(abs(float(v)) for v in w)
    try:
        g = float(gamma)
    except TypeError:
        raise ValueError(f"{who}: gamma must be a number, got {gamma!r}") from None
    if not g >= 0.0 or not np.isfinite(g * g):
        raise ValueError(f"{who}: gamma must be finite and >= 0 with a finite square, got {gamma!r}")
    return g
