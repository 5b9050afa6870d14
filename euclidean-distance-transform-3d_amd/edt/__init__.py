"""Drop-in replacement for the reference's ``edt`` Python module, running on AMD MI355X.

Same public surface as the reference Cython binding (reference: src/edt.pyx:115-310,
:312-844): ``edt, edtsq, sdf, sdfsq, edt1d[sq], edt2d[sq], edt3d[sq]`` with the same
argument meaning, defaults and error behaviour.  The numerics run in hand-written HIP
kernels behind the C ABI of ``include/edt_hip.h``; this file is only the host-side
argument handling (shape / order / dtype dispatch), exactly as the reference keeps it in
Cython.  There is no CPU fallback: without the built library or without a GPU, calls raise.

Conventions kept from the reference:
  * arrays may be C or Fortran contiguous; C order is the same computation with extents
    and anisotropy reversed (src/edt.pyx:651-664);
  * signed integer labels are reinterpreted as unsigned (src/edt.pyx:670-705), booleans are
    one byte per voxel (:724-732);
  * ``parallel`` is accepted and ignored (the GPU grid replaces the thread pool);
  * empty input returns an empty float32 array (:281-282); >3 dims raises TypeError (:309-310).

Device-resident use (torch tensors on ``cuda``) goes through :mod:`edt.device`.
"""
from __future__ import annotations

import collections
import ctypes
import multiprocessing

import numpy as np

from . import _lib, _moments, _topology
from ._args import (  # noqa: F401  (the argument rules shared with edt.device; re-exported)
    _DTYPE_CODE, _NEIGHBOUR_COUNTS, _NP_OF_CODE, DustCounts, LabelMoments, LabelStats, LabelTopology, ThicknessSizes, _check_max_labels,
    _check_ndim, _connectivity, _dust_bounds, _empty_table, _label_table, _ladder_room, _medial_gamma, _medial_ratio, _min_saliency,
    _morph_flags, _morph_radius, _thickness_radii, _xyz)
from ._lib import EdtHipError  # noqa: F401  (re-export)

# a host that cannot run any transform fails HERE, with the reason (no built library; no GPU device node) -- _lib.probe_at_import
_lib.probe_at_import()

__all__ = [
    "edt", "edtsq", "sdf", "sdfsq",
    "edt1d", "edt1dsq", "edt2d", "edt2dsq", "edt3d", "edt3dsq",
    "each", "edt_stack", "edtsq_stack", "binary_edt", "binary_edtsq", "set_devices", "EdtHipError",
    "runs", "draw", "transfer", "erase", "reshape", "nvl", "feature_transform", "expand_labels",
    "label_stats", "label_moments", "LabelMoments", "label_topology", "LabelTopology",
    "connected_components", "fill_holes", "dust", "DustCounts",
    "erode", "dilate", "opening", "closing", "local_thickness", "ThicknessSizes",
    "medial_axis", "watershed",
]


def nvl(val, default_val):
    """`val`, or `default_val` when it is None (module-level helper of the reference, src/edt.pyx:115-118)."""
    return default_val if val is None else val


def reshape(arr, shape, order=None):
    """A view of a contiguous array under another shape, in the array's own memory order unless `order` ('C' / 'F') says
    otherwise -- no copy where the layout allows one (module-level helper of the reference, src/edt.pyx:851-877; an
    array that is contiguous in neither order is reshaped the numpy way)."""
    arr = np.asarray(arr)
    if order is None:
        order = "F" if arr.flags.f_contiguous else ("C" if arr.flags.c_contiguous else None)
    return arr.reshape(shape) if order is None else arr.reshape(shape, order=order)


def _label_code(data: np.ndarray) -> int:
    try:
        return _DTYPE_CODE[data.dtype]
    except KeyError:
        raise TypeError(
            f"Unsupported label dtype {data.dtype}; supported: (u)int8/16/32/64, float32, "
            "float64, bool.") from None


def _as_label_buffer(data: np.ndarray, code: int) -> np.ndarray:
    """Contiguous buffer the kernels can read: signed -> unsigned view, bool -> bytes."""
    want = _NP_OF_CODE[code]
    return data.view(want) if data.dtype != want else data


def _ptr(arr: np.ndarray) -> ctypes.c_void_p:
    return ctypes.c_void_p(arr.ctypes.data)


class _Call(collections.namedtuple("_Call", ["data", "order", "code", "buf", "nd", "e", "w"])):
    """One call as the C ABI sees it (:func:`_layout` makes it): the contiguous array and its memory order, the dtype code,
    the buffer the kernels read, the number of dimensions, and the x-fastest extents and voxel sizes, both padded to three."""
    __slots__ = ()

    @property
    def head(self):
        """how every entry point of the library begins: labels, dtype, ndim, extents"""
        return (_ptr(self.buf), self.code, self.nd, *self.e)

    def new(self, dtype=None):
        """an uninitialised result of the data's shape and memory order"""
        return np.empty(self.data.shape, dtype=self.data.dtype if dtype is None else dtype, order=self.order)


def _array(data, who, dtype=True):
    """Step one of a call, before its own arguments are looked at: an array of 1 to 3 dimensions and (``dtype``) of a label
    dtype.  Step two, :func:`_layout`, comes after them and after the empty case."""
    data = np.asarray(data)
    _check_ndim(who, data.ndim)
    if dtype:
        _label_code(data)
    return data, data.ndim


# ----------------------------------------------------------------------------------------
# public API
# ----------------------------------------------------------------------------------------
def sdf(data, anisotropy=None, black_border=False, parallel=1, voxel_graph=None, order=None):
    """Signed distance function: ``edt(data) - edt(data == 0)`` (reference: src/edt.pyx:121-158)."""
    data = np.asarray(data) if isinstance(data, list) else data
    if voxel_graph is None:
        # one round trip: both transforms and the subtraction run on the device (edt_hip_sdf)
        return _transform(data, anisotropy, black_border, parallel, None, take_sqrt=True, signed=True)

    def fn(labels):
        return edt(labels, anisotropy=anisotropy, black_border=black_border, parallel=parallel,
                   voxel_graph=voxel_graph)

    dt = fn(data)
    dt -= fn(data == 0)
    return dt


def sdfsq(data, anisotropy=None, black_border=False, parallel=1, voxel_graph=None):
    """Squared signed distance function (reference: src/edt.pyx:161-202)."""
    data = np.asarray(data) if isinstance(data, list) else data
    if voxel_graph is None:
        return _transform(data, anisotropy, black_border, parallel, None, take_sqrt=False, signed=True)

    def fn(labels):
        return edtsq(labels, anisotropy=anisotropy, black_border=black_border, parallel=parallel,
                     voxel_graph=voxel_graph)

    return fn(data) - fn(data == 0)


def edt(data, anisotropy=None, black_border=False, parallel=1, voxel_graph=None, order=None):
    """Anisotropic multi-label Euclidean distance transform of a 1-D/2-D/3-D array.

    Reference: src/edt.pyx:205-242.  The square root is fused into the last GPU pass
    (correctly rounded, hence identical to the reference's ``np.sqrt``).
    """
    return _transform(data, anisotropy, black_border, parallel, voxel_graph, take_sqrt=True)


def edtsq(data, anisotropy=None, black_border=False, parallel=1, voxel_graph=None, order=None):
    """Squared distance transform (reference: src/edt.pyx:245-310)."""
    return _transform(data, anisotropy, black_border, parallel, voxel_graph, take_sqrt=False)


def edt1d(data, anisotropy=1.0, black_border=False):
    return _run(np.asarray(data), (anisotropy,), black_border, None, True, ndim=1)


def edt1dsq(data, anisotropy=1.0, black_border=False):
    return _run(np.asarray(data), (anisotropy,), black_border, None, False, ndim=1)


def edt2d(data, anisotropy=(1.0, 1.0), black_border=False, parallel=1, voxel_graph=None):
    return _run(np.asarray(data), anisotropy, black_border, voxel_graph, True, ndim=2)


def edt2dsq(data, anisotropy=(1.0, 1.0), black_border=False, parallel=1, voxel_graph=None):
    return _run(np.asarray(data), anisotropy, black_border, voxel_graph, False, ndim=2)


def edt3d(data, anisotropy=(1.0, 1.0, 1.0), black_border=False, parallel=1, voxel_graph=None):
    return _run(np.asarray(data), anisotropy, black_border, voxel_graph, True, ndim=3)


def edt3dsq(data, anisotropy=(1.0, 1.0, 1.0), black_border=False, parallel=1, voxel_graph=None):
    return _run(np.asarray(data), anisotropy, black_border, voxel_graph, False, ndim=3)


def binary_edtsq(data, anisotropy=None, black_border=False, parallel=1):
    """The C++ facade's ``edt::binary_edtsq`` for 2-D / 3-D arrays of ANY label type (reference:
    src/edt.hpp:895-951 -> ``pyedt::_binary_edt{2,3}dsq<T>``, :487-576, :681-755): labels split runs along x only;
    along y and z every non-zero voxel is one foreground.  Equal to ``edtsq`` on 0/1 input.  (The reference's Python
    module reaches this route for ``bool`` arrays only; exposed here so the facade's semantics can be tested.)"""
    data = np.asarray(data)
    if data.ndim not in (2, 3):
        raise TypeError("binary_edtsq: 2-D or 3-D arrays")
    return _run(data, anisotropy, black_border, None, False, ndim=data.ndim, binary=True)


def binary_edt(data, anisotropy=None, black_border=False, parallel=1):
    data = np.asarray(data)
    if data.ndim not in (2, 3):
        raise TypeError("binary_edt: 2-D or 3-D arrays")
    return _run(data, anisotropy, black_border, None, True, ndim=data.ndim, binary=True)


def _planes_to_axes(planes, shape, order):
    """ABI feature planes (x, y, z of the x-fastest buffer) -> scipy's ``indices`` layout: component k is the coordinate
    along array axis k."""
    nd = len(shape)
    if order == "F":   # x is axis 0
        return planes.reshape((nd,) + tuple(shape[::-1])).transpose((0,) + tuple(range(nd, 0, -1)))
    return np.ascontiguousarray(planes.reshape((nd,) + tuple(shape))[::-1])


def feature_transform(data, anisotropy=None, black_border=False, parallel=1, return_distances=False):
    """Feature transform: for every voxel the index of a nearest voxel of another label (scipy's
    ``distance_transform_edt(..., return_indices=True)`` for multi-label volumes; contract and tie rule:
    include/edt_hip.h).  Returns int32 of shape ``(data.ndim,) + data.shape``; component k is the coordinate along
    array axis k.  Background voxels are their own feature.  With ``black_border`` one component may be -1 or the axis
    length (the border); a voxel without any feature (no border, one label everywhere) gets -1 in every component.
    ``return_distances=True`` also returns ``edt(data, anisotropy, black_border)``.  The tie rule runs its passes in
    the order of the array's memory axes, fastest first: axis 0 first for an F-contiguous array (also for one that is
    C-contiguous as well, e.g. with unit axes, as in every entry point of this module), the last axis first otherwise."""
    data, nd = _array(data, "feature_transform", dtype=False)
    if data.size == 0:
        feats = np.zeros((nd,) + data.shape, dtype=np.int32)
        return (feats, np.zeros(data.shape, dtype=np.float32)) if return_distances else feats
    c = _layout(data, anisotropy)
    planes = np.empty(nd * data.size, dtype=np.int32)
    _lib.check(_lib.load().edt_hip_feature_transform(*c.head, *c.w, 1 if black_border else 0, _ptr(planes)))
    feats = _planes_to_axes(planes, data.shape, c.order)
    if return_distances:
        return feats, edt(c.data, anisotropy=anisotropy, black_border=black_border, parallel=parallel)
    return feats


def expand_labels(data, distance=1.0, anisotropy=None, parallel=1):
    """Grow every label into the background by up to ``distance`` (physical units): each background voxel takes the
    label of its feature in the feature transform of ``data == 0`` if that voxel lies within ``distance``
    (skimage.segmentation.expand_labels with anisotropy; contract: include/edt_hip.h).  Same shape, dtype and memory
    order as ``data``."""
    data, nd = _array(data, "expand_labels", dtype=False)
    distance = float(distance)
    if not distance >= 0.0:
        raise ValueError(f"expand_labels: distance must be >= 0, got {distance}")
    if data.size == 0:
        return data.copy()
    c = _layout(data, anisotropy)
    out = c.new()
    _lib.check(_lib.load().edt_hip_expand_labels(*c.head, *c.w, distance, _ptr(out)))
    return out


def _table(who, c, max_labels, columns, call):
    """The numpy side of :func:`edt._args._label_table`: ``columns``, the (dtype, row shape) of every output column behind the
    keys, allocated per attempt; ``call(cap, column pointers, n)``, the entry point, ``n`` receiving the number of labels.
    Returns the columns cut to the labels found, the keys back under the data's own type and, for signed dtypes, all columns
    in signed order."""
    def attempt(cap):
        cols = [np.empty((cap,) + shape, dtype=dtype) for dtype, shape in [(c.buf.dtype, ())] + columns]
        count = ctypes.c_int64(0)
        _lib.check(call(cap, [_ptr(col) for col in cols], ctypes.byref(count)))
        return int(count.value), cols

    cols = _label_table(who, c.code, c.data.size, max_labels, attempt)
    cols[0] = cols[0].view(c.data.dtype)   # (signed dtypes: the bit patterns back under their own type)
    if c.data.dtype.kind == "i":           # the ABI orders bit patterns: negative keys come last there
        perm = np.argsort(cols[0], kind="stable")
        cols = [col[perm] for col in cols]
    return cols


def _no_rows(cls, data, nd):
    _label_code(data)
    return _empty_table(cls, nd, lambda name, shape: np.zeros(shape, dtype=data.dtype if name is None else name))


def label_stats(data, dt=None, anisotropy=None, black_border=False, parallel=1, max_labels=None):
    """One table row per distinct non-zero label of ``data`` (contract: include/edt_hip.h, "label_stats"), as the named
    tuple ``(labels, counts, max, argmax, bbox_lo, bbox_hi)`` of numpy arrays: the label values ascending (signed dtypes
    in signed order, as :func:`each` yields them), the voxel count (int64), the largest ``dt`` over the label's voxels
    (float32), the coordinates ``(n, ndim)`` per array axis of the voxel that attains it (int64) and the inclusive
    bounding box per array axis (int32, ``(n, ndim)`` each).

    ``dt``: any NaN-free float32 array of ``data``'s shape (``edt``, ``sdf`` ...).  ``dt=None`` computes
    ``edt(data, anisotropy, black_border)`` on the device inside the same call: the distance field never crosses to the
    host, only the table does.  ``-0.0`` is background and NaN voxels of float labels belong to no label.

    Ties: among the voxels that attain the maximum, ``argmax`` is the one with the smallest index in the array's MEMORY
    order.  For a C-contiguous array that is ``np.unravel_index(np.argmax(np.where(data == L, dt, -inf)), data.shape)``;
    for an F-contiguous one (also one that is C-contiguous as well, e.g. with unit axes, as in every entry point of this
    module) the first along ``order='F'``, i.e. the first axis runs fastest.

    ``max_labels=None``: exact for 8/16-bit labels, else room for 65536 labels, retried with 8x the room while it proves
    too small; an explicit ``max_labels`` that proves too small raises ``ValueError``."""
    data, nd = _array(data, "label_stats", dtype=False)
    if dt is not None:
        dt = np.asarray(dt)
        if dt.shape != data.shape or dt.dtype != np.float32:
            raise ValueError("dt must be a float32 array of the data's shape")
    _check_max_labels("label_stats", max_labels)
    if data.size == 0:
        return _no_rows(LabelStats, data, nd)
    c = _layout(data, anisotropy)
    if dt is not None:
        dt = np.asfortranarray(dt) if c.order == "F" else np.ascontiguousarray(dt)
    keys, counts, mx, arg, bbox = _table(
        "label_stats", c, max_labels, [(np.int64, ()), (np.float32, ()), (np.int64, ()), (np.int32, (6,))],
        lambda cap, cols, n: _lib.load().edt_hip_label_stats(*c.head, *c.w, 1 if black_border else 0,
                                                             None if dt is None else _ptr(dt), cap, *cols, n))
    n, order = len(keys), c.order
    lo, hi = bbox[:, 0:2 * nd:2], bbox[:, 1:2 * nd:2]
    argmax = np.stack(np.unravel_index(arg, c.data.shape, order=order), axis=1).astype(np.int64).reshape(n, nd)
    if order == "C":                       # x is the LAST array axis
        lo, hi = lo[:, ::-1], hi[:, ::-1]
    return LabelStats(np.ascontiguousarray(keys), counts, mx, argmax, np.ascontiguousarray(lo), np.ascontiguousarray(hi))


def label_moments(data, max_labels=None):
    """Centroid and second moments of every label: one table row per distinct non-zero label of ``data`` (1-D to 3-D; contract:
    include/edt_hip.h, "label_moments"), as the named tuple :class:`LabelMoments`
    ``(labels, counts, first, second, centroid, covariance)`` of numpy arrays, every field per array axis -- the label values
    ascending (signed dtypes in signed order), the voxel count, the EXACT raw first ``(n, ndim)`` and second ``(n, ndim, ndim)``
    moments about the array's origin (int64), the centroid and the population covariance in voxel units (float64, each value
    rounded once from exact integers; what ``cc3d.statistics`` and ``skimage.measure.regionprops`` call centroid and, up to the
    trace, inertia tensor).  ``result.principal(anisotropy)`` gives the principal axes.  The labels cross to the device once and
    one sweep reads them; only the table comes back.  ``-0.0`` is background and NaN voxels of float labels belong to no label.

    ``max_labels=None``: exact for 8/16-bit labels, else room for 65536 labels, retried with 8x the room while it proves too
    small; an explicit ``max_labels`` that proves too small raises ``ValueError``.  So does a volume with
    ``voxels * (largest extent - 1)**2 >= 2**63`` (lines of millions of voxels): its sums would leave int64."""
    data, nd = _array(data, "label_moments", dtype=False)
    _check_max_labels("label_moments", max_labels)
    if data.size == 0:
        return _no_rows(LabelMoments, data, nd)
    c = _layout(data)
    _moments.check_range(data.shape)
    keys, counts, sums, centroid, central = _table(
        "label_moments", c, max_labels, [(np.int64, ()), (np.int64, (9,)), (np.float64, (3,)), (np.float64, (6,))],
        lambda cap, cols, n: _lib.load().edt_hip_label_moments(*c.head, cap, *cols, n))
    got = _moments.assemble(np.ascontiguousarray(keys), counts, sums, centroid, central, nd, c.order == "C")
    return LabelMoments(*[np.ascontiguousarray(f) for f in got])


def label_topology(data, max_labels=None):
    """Euler numbers and surface of every label: one table row per distinct non-zero label of ``data`` (1-D to 3-D; contract:
    include/edt_hip.h, "label_topology"), as the named tuple :class:`LabelTopology` ``(labels, counts, closed, interior)`` of
    numpy arrays -- the label values ascending (signed dtypes in signed order), the voxel count, and two int64 tables of shape
    ``(n,) + (2,) * ndim`` indexed per array axis (index 1: the cell extends along that axis): ``closed`` counts the vertices,
    edges, faces and cubes with at least one incident voxel of the label (8- / 26-adjacency), ``interior`` those whose
    incident voxels all carry it (4- / 6-adjacency).  Positions outside the array hold no label.  ``result.euler(connectivity)``
    is components - tunnels + cavities (what ``skimage.measure.euler_number`` gives label by label),
    ``result.intrinsic_volumes(anisotropy)`` the four Minkowski functionals up to their constants and
    ``result.surface_area(anisotropy)`` the area of the exposed VOXEL FACES: exact and additive, and not an estimate of a smooth
    surface's area, to which it does not converge (about 1.5 times larger for a ball).  Every count is an exact integer, the
    same bits on every run.  The labels cross to the device once and one sweep reads them; only the table comes back.  ``-0.0``
    is background and NaN voxels of float labels belong to no label.

    ``max_labels=None``: exact for 8/16-bit labels, else room for 65536 labels, retried with 8x the room while it proves too
    small; an explicit ``max_labels`` that proves too small raises ``ValueError``."""
    data, nd = _array(data, "label_topology", dtype=False)
    _check_max_labels("label_topology", max_labels)
    if data.size == 0:
        return _no_rows(LabelTopology, data, nd)
    c = _layout(data)
    keys, closed, interior = _table("label_topology", c, max_labels, [(np.int64, (8,)), (np.int64, (8,))],
                                    lambda cap, cols, n: _lib.load().edt_hip_label_topology(*c.head, cap, *cols, n))
    got = _topology.assemble(np.ascontiguousarray(keys), closed, interior, nd, c.order == "C")
    return LabelTopology(*[np.ascontiguousarray(f) for f in got])


def connected_components(data, connectivity=None, binary=False, return_N=False):
    """Connected components of a 1-D to 3-D label array on the device (cc3d.connected_components /
    skimage.measure.label / scipy.ndimage.label; contract: include/edt_hip.h, "connected components").  Two neighbouring
    voxels belong to one component iff their labels are equal and non-zero; ``binary=True`` treats every non-zero voxel as
    one class (``scipy.ndimage.label(data != 0)``; a bool array is always binary).  ``-0.0`` is background; a NaN voxel
    is a component of its own, and joins its neighbours under ``binary``.

    ``connectivity``: ``None`` is full (``data.ndim``); ``1..ndim`` is the number of axes along which neighbours may
    differ (skimage); cc3d's neighbour counts ``4`` / ``8`` (2-D) and ``6`` / ``18`` / ``26`` (3-D) are accepted too.

    Returns a ``uint32`` array of ``data``'s shape and memory order: 0 for background, else the component's number in
    ``1..N``; with ``return_N=True`` the pair ``(out, N)``.  Components are numbered in the order in which a scan of the
    array's MEMORY meets them: for a C-contiguous array and ``binary`` that is scipy's numbering, for an F-contiguous one
    (also one that is C-contiguous as well, e.g. with unit axes, as in every entry point of this module) cc3d's.  At most
    2^31 - 1 voxels."""
    data, nd = _array(data, "connected_components")
    conn = _connectivity(connectivity, nd)
    if data.size == 0:
        out = np.zeros(data.shape, dtype=np.uint32)
        return (out, 0) if return_N else out
    c = _layout(data)
    out = c.new(np.uint32)
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().edt_hip_connected_components(*c.head, conn, 1 if binary else 0, _ptr(out), ctypes.byref(n)))
    return (out, int(n.value)) if return_N else out


def fill_holes(data, connectivity=None, binary=False, return_fill_count=False):
    """Fill the enclosed cavities of a 1-D to 3-D label array on the device (fill_voids.fill /
    scipy.ndimage.binary_fill_holes, for every label at once; contract: include/edt_hip.h, "fill holes").  A cavity is a
    connected component of zero voxels that does not touch the array's boundary; it takes the label of the voxels around
    it if they all carry one label, and stays 0 if they carry several (or a NaN).  ``binary=True`` fills every cavity
    with the label of its first wall voxel in memory order -- ``binary_fill_holes(data != 0)`` for a mask; a bool array
    is always binary.  ``-0.0`` is background.  Enclosed foreground is never touched.

    ``connectivity`` is the adjacency of the BACKGROUND: ``None`` means **1** (the background is 2 * ndim-connected:
    scipy's default structure and fill_voids' rule) -- NOT the full connectivity that ``None`` means for
    :func:`connected_components`.  ``1..ndim`` and cc3d's ``4`` / ``8``, ``6`` / ``18`` / ``26`` are accepted as there.

    Returns an array of ``data``'s dtype, shape and memory order; with ``return_fill_count=True`` the pair
    ``(out, n)``, ``n`` the number of voxels that were filled.  At most 2^31 - 1 voxels."""
    data, nd = _array(data, "fill_holes")
    conn = _connectivity(connectivity, nd, default=1, who="fill_holes")
    if data.size == 0:
        out = data.copy()
        return (out, 0) if return_fill_count else out
    c = _layout(data)
    out = c.new()
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().edt_hip_fill_holes(*c.head, conn, 1 if binary else 0, _ptr(out), ctypes.byref(n)))
    return (out, int(n.value)) if return_fill_count else out


def dust(data, threshold, connectivity=None, binary=False, invert=False, return_counts=False):
    """Remove the connected components of a 1-D to 3-D label array by their voxel count, on the device (cc3d.dust /
    skimage.morphology.remove_small_objects; contract: include/edt_hip.h, "dust").  Neither cc3d nor skimage is on the
    build machine: what is tested is the header's contract, not their behaviour.  A component is exactly a component of
    :func:`connected_components` with the same ``connectivity`` and ``binary``: ``-0.0`` is background, a NaN voxel is a
    component of its own (and joins its neighbours under ``binary``), a bool array is always binary.

    ``threshold``: an integer ``t`` removes the components of fewer than ``t`` voxels; a pair ``(lo, hi)`` keeps those
    with ``lo <= size < hi``.  ``invert=True`` removes what would be kept and keeps what would be removed.
    ``connectivity`` as in :func:`connected_components`: ``None`` is full, ``1..ndim``, or cc3d's ``4`` / ``8``,
    ``6`` / ``18`` / ``26``.

    Returns an array of ``data``'s dtype, shape and memory order: the voxels of kept components and the background bit for
    bit, the voxels of removed components zero.  With ``return_counts=True`` the pair
    ``(out, DustCounts(components, kept, removed_voxels))`` of Python ints.  At most 2^31 - 1 voxels."""
    data, nd = _array(data, "dust")
    lo, hi = _dust_bounds(threshold)
    conn = _connectivity(connectivity, nd, who="dust")
    if data.size == 0:
        out = data.copy()
        return (out, DustCounts(0, 0, 0)) if return_counts else out
    c = _layout(data)
    out = c.new()
    counts = np.zeros(3, dtype=np.int64)
    _lib.check(_lib.load().edt_hip_dust(*c.head, conn, 1 if binary else 0, lo, hi, 1 if invert else 0, _ptr(out), _ptr(counts)))
    return (out, DustCounts(*(int(v) for v in counts))) if return_counts else out


def watershed(data, field=None, min_saliency=0.0, connectivity=None, anisotropy=None, black_border=False, binary=False,
              return_N=False):
    """Split every label of a 1-D to 3-D label array into the basins of a float32 field, on the device (contract:
    include/edt_hip.h, "watershed").  This is the STEEPEST-ASCENT watershed -- "drop of water", hill climbing -- stated as the
    connected components of a graph: every voxel is joined to its greatest neighbour of the same object (ties: the first in
    memory order), a voxel without a greater one to its equal neighbours, and the basins are the components of these joins.
    It is NOT ``skimage.segmentation.watershed``: it takes no markers, its boundaries follow the ascent rule and not a flooding
    order, and ties go to the greatest neighbour, not the steepest slope, so anisotropy enters through the field only.  Neither
    skimage nor cc3d is on the build machine: what is tested is the header's contract.

    ``field``: a float32 array of ``data``'s shape without NaN on the foreground (``ValueError``); ``+inf`` is legal.
    ``field=None`` computes ``edt(data, anisotropy, black_border)`` -- of ``data != 0`` under ``binary`` -- on the device
    inside the same call; ``anisotropy`` and ``black_border`` are used for nothing else.
    ``min_saliency``: ``h >= 0`` in the field's units.  ``h > 0`` joins two neighbouring basins whose saddle voxels reach the
    lower of their two peaks minus ``h``, in ONE round of single-linkage merging over the basins of the ascent: it is not the
    h-maxima hierarchy, a chain of shallow saddles merges end to end.  Half a voxel removes the over-segmentation of the
    ascent along digital ridges; ``1e30`` gives :func:`connected_components` itself.
    ``connectivity`` and ``binary`` as in :func:`connected_components`: two voxels are of one object iff that function
    would connect them (``-0.0`` is background, a NaN label is alone, a bool array is always binary).

    Returns a ``uint32`` array of ``data``'s shape and memory order: 0 for background, else the basin's number in ``1..N``,
    in the order in which a scan of the array's MEMORY meets the basins; with ``return_N=True`` the pair ``(out, N)``.
    ``label_stats(watershed(x), dt)`` is then a table per SPLIT object.  At most 2^31 - 1 voxels."""
    data, nd = _array(data, "watershed")
    conn = _connectivity(connectivity, nd, who="watershed")
    h = _min_saliency(min_saliency)
    if field is not None:
        field = np.asarray(field)
        if field.shape != data.shape or field.dtype != np.float32:
            raise ValueError("watershed: field must be a float32 array of the data's shape")
    if data.size == 0:
        out = np.zeros(data.shape, dtype=np.uint32)
        return (out, 0) if return_N else out
    c = _layout(data, anisotropy)
    if field is not None:
        with np.errstate(invalid="ignore"):
            if np.isnan(field[c.data != 0]).any():
                raise ValueError("watershed: the field is NaN on a foreground voxel")
        field = np.asfortranarray(field) if c.order == "F" else np.ascontiguousarray(field)
    out = c.new(np.uint32)
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().edt_hip_watershed(*c.head, None if field is None else _ptr(field), *c.w, 1 if black_border else 0,
                                             conn, 1 if binary else 0, h, _ptr(out), ctypes.byref(n)))
    return (out, int(n.value)) if return_N else out


def _morphology(who, op, data, radius, anisotropy, flags):
    data, nd = _array(data, who)
    r = _morph_radius(radius, who, inf_allowed=op == _lib.MORPH_DILATE)
    if data.size == 0:
        return data.copy()
    c = _layout(data, anisotropy)
    out = c.new()
    _lib.check(_lib.load().edt_hip_morphology(*c.head, *c.w, op, r, flags, _ptr(out)))
    return out


def erode(data, radius=1.0, anisotropy=None, black_border=False, binary=False, parallel=1):
    """Erode every label of a 1-D to 3-D label array by the ball of physical radius ``radius`` (contract: include/edt_hip.h,
    "morphology"): a voxel keeps its label iff ``edtsq(data, anisotropy, black_border) > radius**2`` there, squared
    distances compared exactly, and becomes 0 otherwise -- per label, scipy's ``binary_erosion(data == l, ball,
    border_value=0 if black_border else 1)``.  Neighbouring labels erode each other; ``binary=True`` measures the mask
    ``data != 0`` instead, so only the background erodes (a bool array is always binary).  ``-0.0`` is background, NaN is
    foreground.  Same dtype, shape and memory order as ``data``; one trip over PCIe each way."""
    return _morphology("erode", _lib.MORPH_ERODE, data, radius, anisotropy, _morph_flags(black_border, binary))


def dilate(data, radius=1.0, anisotropy=None, parallel=1):
    """Grow every label into the background by up to ``radius``: exactly :func:`expand_labels` (``radius`` may be inf)."""
    return _morphology("dilate", _lib.MORPH_DILATE, data, radius, anisotropy, 0)


def opening(data, radius=1.0, anisotropy=None, black_border=False, binary=False, parallel=1):
    """Morphological opening of every label at once by the ball of radius ``radius``: the erosion of :func:`erode`, dilated
    again inside each voxel's own label -- a voxel keeps its label iff it lies within ``radius`` of a voxel that survives
    the erosion.  Removes spurs and bridges thinner than the ball without shrinking the bodies; idempotent.  Arguments and
    result as for :func:`erode`."""
    return _morphology("opening", _lib.MORPH_OPEN, data, radius, anisotropy, _morph_flags(black_border, binary))


def closing(data, radius=1.0, anisotropy=None, parallel=1):
    """Morphological closing by the ball of radius ``radius``: :func:`dilate`, then the new voxels are eroded again
    (the outside of the array does not erode).  Gaps and pits narrower than the ball take the label ``expand_labels`` gives
    them; every voxel of ``data`` keeps its label.  For a mask, scipy's ``binary_erosion(binary_dilation(m, ball), ball,
    border_value=1)``."""
    return _morphology("closing", _lib.MORPH_CLOSE, data, radius, anisotropy, 0)


def local_thickness(data, radii=None, anisotropy=None, black_border=False, binary=False, return_sizes=False, parallel=1):
    """Local thickness of every label of a 1-D to 3-D label array at once (porespy's ``local_thickness``, ImageJ's "Local
    Thickness", quantised to a ladder of radii; contract: include/edt_hip.h, "local thickness"): for every voxel the largest
    radius ``r`` of ``radii`` whose :func:`opening` -- same ``anisotropy``, ``black_border`` and ``binary`` -- still contains
    it, as float32; 0 for background and for voxels that lie in no opening.  "Largest" is meant literally: the openings by
    digital balls are not nested, and a voxel may lie in a larger one and not in the next smaller.

    ``radii``: strictly ascending, each > 0 with a finite square (a ValueError otherwise).  ``None`` is the ladder
    ``step, 2 step, 3 step, ...`` with ``step`` the smallest voxel size, as far as ``r**2`` stays below the largest finite value
    of ``edtsq(data, anisotropy, black_border)``: larger balls fit nowhere.  One label everywhere without a border has no
    finite distance: the default ladder is then empty and the result zero, while explicit radii give ``radii[-1]`` everywhere.

    Returns float32 of ``data``'s shape and memory order; with ``return_sizes=True`` the pair ``(thickness,
    ThicknessSizes(radii, voxels))``: the radii actually used (float64) and the voxel count of each radius' opening (int64),
    the granulometry curve.  One trip over PCIe each way; per radius one binary transform and one streaming kernel."""
    data, nd = _array(data, "local_thickness")
    r = None if radii is None else _thickness_radii(radii)
    if data.size == 0:
        out = np.zeros(data.shape, dtype=np.float32)
        used = np.zeros(0, dtype=np.float64) if r is None else r
        return (out, ThicknessSizes(used, np.zeros(used.size, dtype=np.int64))) if return_sizes else out
    c = _layout(data, anisotropy)
    step, room = (0.0, r.size) if r is not None else _ladder_room(c.e[:nd], c.w[:nd])
    out = c.new(np.float32)
    sizes = np.zeros(room, dtype=np.int64)
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().edt_hip_local_thickness(*c.head, *c.w, _morph_flags(black_border, binary), None if r is None else _ptr(r),
                                                   room, step, _ptr(out), _ptr(sizes), ctypes.byref(n)))
    if not return_sizes:
        return out
    k = int(n.value)
    used = r if r is not None else np.arange(1, k + 1, dtype=np.float64) * step
    return out, ThicknessSizes(used, sizes[:k].copy())


def medial_axis(data, gamma=None, min_angle=0.0, anisotropy=None, black_border=False, binary=False, return_distance=False,
                parallel=1):
    """The integer medial axis (Hesselink & Roerdink 2008) of every label of a 1-D to 3-D label array at once: the centre lines
    and centre surfaces of the objects, straight from the feature transform (contract: include/edt_hip.h, "medial axis").  A
    voxel is on the axis iff it has a face neighbour of its own label whose nearest voxel of another label (its feature) lies
    farther than ``gamma`` from the voxel's own feature, and the bisector of the two features passes on the voxel's side of
    the midpoint between the two voxels.

    ``gamma``: constant pruning, a physical distance; ``None`` is the largest voxel size (the paper's "more than one voxel
    apart").  ``min_angle``: angle pruning in degrees, in [0, 180): the two features must subtend at least this angle at the
    midpoint of the two voxels (0: off; larger angles keep only the centre of the object and drop the branches into its
    corners).  ``anisotropy``, ``black_border`` and ``binary`` as for :func:`erode`: with ``binary=True`` the axis is that of
    the mask ``data != 0`` (a bool array is always binary), otherwise neighbouring labels bound each other.  Without a black
    border an object that fills the array has no axis.

    Returns an array of ``data``'s shape, dtype and memory order: the label on the axis, 0 elsewhere.  With
    ``return_distance=True`` the pair ``(axis, distance)``: ``distance`` is float32, ``edt(data)`` (of the mask under binary) on
    the axis and 0 elsewhere -- the radius function.  One trip over PCIe each way."""
    data, nd = _array(data, "medial_axis")
    ratio = _medial_ratio(min_angle)
    if data.size == 0:
        _medial_gamma(gamma, (1.0,))
        return (data.copy(), np.zeros(data.shape, dtype=np.float32)) if return_distance else data.copy()
    c = _layout(data, anisotropy)
    g = _medial_gamma(gamma, c.w[:nd])
    out = c.new()
    dist = c.new(np.float32) if return_distance else None
    _lib.check(_lib.load().edt_hip_medial_axis(*c.head, *c.w, _morph_flags(black_border, binary), g, ratio, _ptr(out),
                                               None if dist is None else _ptr(dist)))
    return (out, dist) if return_distance else out


def set_devices(devices=None):
    """Z-shard every 3-D transform of host arrays over these GPUs of THIS process (``edt_hip_set_devices``: a host
    thread per device, one peer-to-peer exchange over xGMI, see ``csrc/edt_multi.hip``); ``None`` / ``[]`` = back to
    the current device alone.  ``EDT_HIP_DEVICES=0,1,...`` in the environment presets the list.  Results are
    bit-identical either way."""
    devs = [] if devices is None else [int(d) for d in devices]
    arr = (ctypes.c_int * max(1, len(devs)))(*devs)
    _lib.check(_lib.load().edt_hip_set_devices(ctypes.cast(arr, ctypes.c_void_p), len(devs)))


def _stack(images, anisotropy, black_border, take_sqrt):
    images = np.asarray(images)
    if images.ndim != 3:
        raise TypeError("a stack of 2-D images is a 3-D array (count, height, width)")
    if images.size == 0:
        return np.zeros(images.shape, dtype=np.float32)
    images = np.ascontiguousarray(images)      # C order: the last axis (width) is x
    code = _label_code(images)
    buf = _as_label_buffer(images, code)
    an = (1.0, 1.0) if anisotropy is None else tuple(float(np.float32(a)) for a in anisotropy)
    if len(an) != 2:
        raise ValueError("anisotropy of a 2-D image has 2 entries")
    count, sy, sx = images.shape
    out = np.empty(images.shape, dtype=np.float32)
    _lib.check(_lib.load().edt_hip_edt2dsq_batch(_ptr(buf), code, sx, sy, count, an[1], an[0],
                                                 1 if black_border else 0, 1 if take_sqrt else 0, _ptr(out)))
    return out


def edtsq_stack(images, anisotropy=None, black_border=False):
    """Squared EDT of every 2-D image of ``images[count, height, width]`` independently, in one call (an
    extension over the reference's API: the stack goes through the GPU as one batch, edt_hip_edt2dsq_batch).
    ``anisotropy`` = (height spacing, width spacing), as for a C-ordered 2-D array."""
    return _stack(images, anisotropy, black_border, take_sqrt=False)


def edt_stack(images, anisotropy=None, black_border=False):
    return _stack(images, anisotropy, black_border, take_sqrt=True)


# ----------------------------------------------------------------------------------------
# argument handling (mirrors src/edt.pyx:276-310) and dispatch into the C ABI
# ----------------------------------------------------------------------------------------
def _transform(data, anisotropy, black_border, parallel, voxel_graph, take_sqrt, signed=False):
    if isinstance(data, list):
        data = np.array(data)
    data = np.asarray(data)
    dims = data.ndim

    if data.size == 0:
        return np.zeros(shape=data.shape, dtype=np.float32)

    if parallel is not None and parallel <= 0:
        parallel = multiprocessing.cpu_count()  # accepted, unused

    if voxel_graph is not None and dims not in (2, 3):
        raise TypeError(
            "Voxel connectivity graph is only supported for 2D and 3D. Got {}.".format(dims))

    if dims < 1 or dims > 3:
        raise TypeError(
            "Multi-Label EDT library only supports up to 3 dimensions got {}.".format(dims))
    return _run(data, anisotropy, black_border, voxel_graph, take_sqrt, ndim=dims, signed=signed)


def _layout(data, anisotropy=None):
    """Step two of a call: the buffer the kernels read and how it maps onto the C ABI (x the fastest axis of memory), as a
    :class:`_Call`; validates the voxel sizes (``None``: 1.0 along every axis)."""
    ndim = data.ndim
    if not data.flags.c_contiguous and not data.flags.f_contiguous:
        data = np.ascontiguousarray(data)
    order = "F" if data.flags.f_contiguous else "C"
    code = _label_code(data)
    buf = _as_label_buffer(data, code)
    if anisotropy is None:
        return _Call(data, order, code, buf, ndim, *_xyz(data.shape, None, ndim, order == "C"))

    if np.ndim(anisotropy) == 0:
        anisotropy = (anisotropy,) * ndim if ndim == 1 else anisotropy
    weights = tuple(float(np.float32(a)) for a in np.asarray(anisotropy, dtype=np.float64).reshape(-1))
    if len(weights) != ndim:
        raise ValueError(f"anisotropy must have {ndim} entries, got {len(weights)}")
    # (stated deviation: the reference does not validate voxel sizes.  Along the fastest axis a size enters pass 1 as itself -- a
    # negative one makes the reference's backward sweep cross label boundaries, src/edt.hpp:107-109 --, along the other axes only
    # as its square, src/edt.hpp:181, :258: the sign is meaningless there and accepted, as the reference does; zero, NaN and
    # inf are refused everywhere, here and at the C ABI, include/edt_hip.h)
    fastest = 0 if order == "F" else ndim - 1
    if not all(np.isfinite(a) and a != 0.0 for a in weights) or weights[fastest] < 0.0:
        raise ValueError(f"anisotropy must be finite and non-zero (and positive along the fastest axis), got {weights}")
    return _Call(data, order, code, buf, ndim, *_xyz(data.shape, weights, ndim, order == "C"))   # x: the fastest axis of the buffer


def _run(data, anisotropy, black_border, voxel_graph, take_sqrt, ndim, signed=False, binary=False):
    if data.ndim != ndim:
        raise TypeError(f"expected a {ndim}-D array, got {data.ndim}-D")
    if data.size == 0:
        return np.zeros(shape=data.shape, dtype=np.float32)
    c = _layout(data, anisotropy)
    data, order, labels, e, w = c.data, c.order, _ptr(c.buf), c.e, c.w

    lib = _lib.load()
    out = np.empty(data.size, dtype=np.float32)
    bb = 1 if black_border else 0

    if voxel_graph is not None:
        if ndim not in (2, 3):
            raise TypeError(
                "Voxel connectivity graph is only supported for 2D and 3D. Got {}.".format(ndim))
        graph = np.asarray(voxel_graph)
        if graph.shape != data.shape:
            raise ValueError("voxel_graph must have the same shape as data")
        graph = np.ascontiguousarray(graph) if order == "C" else np.asfortranarray(graph)
        # only the low 6 bits are meaningful (src/edt.pyx:748-752)
        graph = graph.view(np.uint8) if graph.dtype.itemsize == 1 else graph.astype(np.uint8, order="K")
        fn = lib.edt_hip_edt2dsq_voxel_graph if ndim == 2 else lib.edt_hip_edt3dsq_voxel_graph
        _lib.check(fn(labels, c.code, _ptr(graph), *e[:ndim], *w[:ndim], bb, _ptr(out)))
        if take_sqrt:
            np.sqrt(out, out)
    elif signed:  # sdf / sdfsq: edt(x) - edt(x == 0), everything but the two copies on the device
        _lib.check(lib.edt_hip_sdf(*c.head, *w, bb, 0 if take_sqrt else 1, _ptr(out)))
    elif binary:
        _lib.check(lib.edt_hip_binary_edtsq(*c.head, *w, bb, 1 if take_sqrt else 0, _ptr(out)))
    elif ndim == 1:
        _lib.check(lib.edt_hip_squared_edt_1d_multi_seg(labels, c.code, _ptr(out), data.size, 1, w[0], bb))
        if take_sqrt:
            np.sqrt(out, out)
    else:
        fn = ((lib.edt_hip_edt2d if take_sqrt else lib.edt_hip_edt2dsq) if ndim == 2 else
              (lib.edt_hip_edt3d if take_sqrt else lib.edt_hip_edt3dsq))
        _lib.check(fn(labels, c.code, *e[:ndim], *w[:ndim], bb, 1, _ptr(out)))
    return out.reshape(data.shape, order=order)


# ----------------------------------------------------------------------------------------
# Run utilities and each(): per-label views of a distance transform (reference:
# src/edt.pyx:847-994, src/edt_voxel_graph.hpp:238-310).  Host-side conveniences on top of the DT
# with the reference's semantics (runs are half-open [start, end) ranges of the array's memory
# order); the device-resident counterpart of each() is edt.device.each / select_label.
# ----------------------------------------------------------------------------------------
def _flat(arr: np.ndarray) -> np.ndarray:
    """1-D view in memory order (src/edt.pyx:851-877: in-place reshape of a contiguous array)."""
    if arr.flags.f_contiguous and not arr.flags.c_contiguous:
        return arr.reshape(-1, order="F")
    return arr.reshape(-1)


def runs(labels):
    """``{label: [(start, end), ...]}`` -- where each label lies (src/edt_voxel_graph.hpp:238-268)."""
    flat = _flat(np.asarray(labels))
    out = {}
    if flat.size == 0:
        return out
    cuts = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    starts = np.concatenate(([0], cuts))
    ends = np.concatenate((cuts, [flat.size]))
    for s, e, v in zip(starts.tolist(), ends.tolist(), flat[starts].tolist()):
        out.setdefault(v, []).append((s, e))
    return dict(sorted(out.items()))  # std::map iterates in key order


def _check_runs(rns, voxels):
    for s, e in rns:
        if s < 0 or e > voxels or e < 0 or s >= e:
            raise RuntimeError("Invalid run.")  # src/edt_voxel_graph.hpp:277-283


def draw(label, runs, image):
    """Write ``label`` into ``image`` along ``runs`` (set_run_voxels, src/edt_voxel_graph.hpp:270-288).
    Like the reference (src/edt.pyx:895-913) it returns the FLAT view of the image it wrote through."""
    flat = _flat(image)
    _check_runs(runs, flat.size)
    for s, e in runs:
        flat[s:e] = label
    return flat


def transfer(runs, src, dest):
    """Copy ``src`` to ``dest`` along ``runs`` (transfer_run_voxels, src/edt_voxel_graph.hpp:290-310);
    returns the flat view of ``dest`` (src/edt.pyx:915-935)."""
    fs, fd = _flat(src), _flat(dest)
    assert fs.size == fd.size
    _check_runs(runs, fs.size)
    for s, e in runs:
        fd[s:e] = fs[s:e]
    return fd


def erase(runs, image):
    """Zero ``image`` along ``runs`` (src/edt.pyx:937-947)."""
    return draw(0, runs, image)


class _PerLabelImages:
    """Sized iterable behind :func:`each`: one ``(label, image)`` pair per non-zero label, in ascending
    label order, where ``image`` is ``dt`` on the label's voxels and 0 elsewhere.

    The label volume is scanned ONCE into a run table (start, end, value per run, sorted by value); every
    image is then painted run by run.  With ``reuse`` one canvas serves all labels: it is handed out
    read-only and wiped along the same runs before the next label is painted."""

    def __init__(self, labels, dt, reuse):
        self._shape = labels.shape
        self._order = "F" if labels.flags.f_contiguous else "C"
        self._dt = _flat(dt)
        self._reuse = reuse
        flat = _flat(labels)
        if flat.size == 0:
            cuts = np.zeros(0, dtype=np.int64)
            starts = ends = cuts
        else:
            cuts = np.flatnonzero(flat[1:] != flat[:-1]) + 1
            starts = np.concatenate(([0], cuts))
            ends = np.concatenate((cuts, [flat.size]))
        values = flat[starts]
        keep = values != 0
        starts, ends, values = starts[keep], ends[keep], values[keep]
        by_value = np.argsort(values, kind="stable")           # runs of one label stay in memory order
        self._starts, self._ends = starts[by_value], ends[by_value]
        self._labels, first = np.unique(values[by_value], return_index=True)
        self._bounds = np.append(first, values.size)            # runs of label i: [bounds[i], bounds[i+1])

    def __len__(self):
        return int(self._labels.size)

    def _paint(self, canvas, i, source):
        for s, e in zip(self._starts[self._bounds[i]:self._bounds[i + 1]].tolist(),
                        self._ends[self._bounds[i]:self._bounds[i + 1]].tolist()):
            canvas[s:e] = source[s:e] if source is not None else 0

    def __iter__(self):
        image = flat_image = None
        for i, label in enumerate(self._labels.tolist()):
            if image is None or not self._reuse:
                image = np.zeros(self._shape, dtype=np.float32, order=self._order)
                flat_image = _flat(image)
            self._paint(flat_image, i, self._dt)
            if not self._reuse:
                yield label, image
                continue
            image.flags.writeable = False
            yield label, image
            image.flags.writeable = True
            self._paint(flat_image, i, None)


def each(labels, dt, in_place=False):
    """Iterate ``(label, image)``: the distance transform ``dt`` restricted to each non-zero label of
    ``labels`` in turn (same contract as the reference's ``edt.each``, src/edt.pyx:950-994: ``len()`` is the
    number of labels, ``in_place=True`` reuses ONE read-only image instead of allocating one per label).
    For device-resident data see :func:`edt.device.each`."""
    return _PerLabelImages(np.asarray(labels), np.asarray(dt), bool(in_place))
