"""Device-resident entry points: torch tensors on an AMD GPU in, torch tensors out.

torch is used only as plumbing (device memory, streams); all arithmetic happens in the HIP
kernels behind ``edt_hip_edtsq_device`` (include/edt_hip.h).  Nothing is copied to the host
and nothing is allocated per call once a :class:`Plan` exists, so a call only enqueues
kernels on the current stream (graph-capturable, timeable with events).

Tensor layout: a contiguous tensor of shape ``(a, b, c)`` has its LAST dimension fastest, so
it is the same computation as a C-ordered numpy array: extents and anisotropy are reversed
before they reach the kernels (reference: src/edt.pyx:651-656).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, _moments, _topology
from ._args import (  # noqa: F401  (LabelStats: re-exported, the class of edt.label_stats)
    _NP_OF_CODE, LabelMoments, LabelStats, LabelTopology, ThicknessSizes, _check_max_labels, _check_ndim, _connectivity, _dust_bounds,
    _empty_table, _label_table, _ladder_room, _medial_gamma, _medial_ratio, _min_saliency, _morph_flags, _morph_radius, _thickness_radii,
    _xyz)

# torch's dtypes: the code of include/edt_hip.h a label dtype has (edt._args has numpy's)
_TORCH_CODE = {
    torch.uint8: _lib.U8, torch.int8: _lib.U8,
    torch.int16: _lib.U16, torch.int32: _lib.U32, torch.int64: _lib.U64,
    torch.float32: _lib.F32, torch.float64: _lib.F64, torch.bool: _lib.BOOL,
}
for _name, _code in (("uint16", _lib.U16), ("uint32", _lib.U32), ("uint64", _lib.U64)):
    if hasattr(torch, _name):
        _TORCH_CODE[getattr(torch, _name)] = _code


def dtype_code(dtype: torch.dtype) -> int:
    try:
        return _TORCH_CODE[dtype]
    except KeyError:
        raise TypeError(f"Unsupported label dtype {dtype}") from None


def as_device_tensor(obj) -> torch.Tensor:
    """A zero-copy torch view of any device array: a torch tensor itself, an object that speaks DLPack (``__dlpack__``:
    CuPy, JAX, recent Numba ...) or the CUDA array interface (``__cuda_array_interface__``: Numba device arrays, CuPy --
    also what those libraries expose on ROCm).  Every entry point of this module takes its array arguments through here
    (the boundary of src/edt.pyx:639-734, for callers whose data never was a numpy array); results are torch tensors,
    which speak both protocols in the other direction."""
    if isinstance(obj, torch.Tensor):
        t = obj
    elif hasattr(obj, "__dlpack__"):
        t = torch.from_dlpack(obj)
    elif hasattr(obj, "__cuda_array_interface__"):
        t = torch.as_tensor(obj, device=torch.device("cuda", torch.cuda.current_device()))
    else:
        raise TypeError(f"expected a device array (torch tensor, __dlpack__ or __cuda_array_interface__), got {type(obj).__name__}")
    if not t.is_cuda:
        raise TypeError("edt.device takes device-resident arrays; host arrays go through edt.edtsq / edt.edt / edt.sdf")
    return t


def _stream_ptr() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Plan:
    """Pre-sized scratch for volumes of one shape/dtype (x-fastest extents ``(sx, sy, sz)``)."""

    def __init__(self, extents_xyz, code: int, device=None, small_workspace=False):
        """small_workspace: scratch = the four bit planes only (EDT_FLAG_SMALL_WORKSPACE: passes X and Y exchange
        fp32 values instead of 16-bit distance indices -- no index slab of up to 256 MiB, a few per cent slower)"""
        self.lib = _lib.load()
        ext = tuple(int(e) for e in extents_xyz)
        self.ndim = len(ext)
        self.ext = ext + (1,) * (3 - self.ndim)
        self.code = code
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.base_flags = _lib.FLAG_SMALL_WORKSPACE if small_workspace else 0
        nbytes = self.lib.edt_hip_workspace_bytes_flags(code, self.ndim, *self.ext, self.base_flags)
        if nbytes == 0:
            _lib.check(-2)
        self.workspace = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        self._generic_ws = None  # the size-agnostic kernels need a second volume: allocated on first use
        self.voxels = int(np.prod(self.ext))

    def _workspace_for(self, flags):
        if not (flags & _lib.FLAG_FORCE_GENERIC):
            return self.workspace
        if self._generic_ws is None:
            nbytes = self.lib.edt_hip_workspace_bytes_flags(self.code, self.ndim, *self.ext, flags)
            self._generic_ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self._generic_ws

    def run(self, labels: torch.Tensor, weights_xyz, black_border=False, sqrt=False,
            out: torch.Tensor | None = None, force_generic=False, batch2d=False, binary=False,
            signed=False) -> torch.Tensor:
        """Enqueue the transform of ``labels`` (device, contiguous, ``voxels`` elements).  binary: the reference's
        binary route for multi-valued labels (EDT_FLAG_BINARY_YZ: labels split runs along x only).  signed: the signed
        transform (EDT_FLAG_SIGNED: sdf / sdfsq as ONE transform; :meth:`signed_supported` says whether the shape is served)."""
        if not labels.is_cuda or not labels.is_contiguous():
            raise ValueError("labels must be a contiguous device tensor")
        if labels.numel() != self.voxels:
            raise ValueError("labels size does not match the plan")
        # (same-width integer views are how uint32 / uint64 labels reach torch builds without those dtypes)
        if labels.element_size() != _lib.DTYPE_SIZE[self.code] or (
                labels.dtype.is_floating_point != (self.code in (_lib.F32, _lib.F64))):
            raise TypeError(f"labels dtype {labels.dtype} does not match the plan's dtype code {self.code}")
        if out is None:
            out = torch.empty(labels.shape, dtype=torch.float32, device=labels.device)
        w = tuple(float(np.float32(v)) for v in weights_xyz) + (1.0,) * (3 - self.ndim)
        flags = ((_lib.FLAG_BLACK_BORDER if black_border else 0) | (_lib.FLAG_SQRT if sqrt else 0)
                 | (_lib.FLAG_FORCE_GENERIC if force_generic else 0)
                 | (_lib.FLAG_BATCH_2D if batch2d else 0) | (_lib.FLAG_BINARY_YZ if binary else 0)
                 | (_lib.FLAG_SIGNED if signed else 0) | self.base_flags)
        ws = self._workspace_for(flags)
        rc = self.lib.edt_hip_edtsq_device(
            ctypes.c_void_p(labels.data_ptr()), self.code, self.ndim, *self.ext, w[0], w[1], w[2],
            flags, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream_ptr())
        _lib.check(rc)
        return out


    def signed_supported(self) -> bool:
        return bool(self.lib.edt_hip_signed_supported(self.code, self.ndim, *self.ext, self.base_flags))


_plans: dict = {}


def _plan_for(ext, code, device) -> Plan:
    # one plan (= one scratch buffer) per stream: transforms of one shape issued on different streams
    # must not share scratch, and a workspace is only ever used on the stream it was allocated on
    key = (tuple(ext), code, str(device), torch.cuda.current_stream(device).cuda_stream)
    if key not in _plans:
        if len(_plans) > 8:
            _plans.clear()
        _plans[key] = Plan(ext, code, device)
    return _plans[key]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _input(labels, anisotropy=None, who=None, code=True):
    """What every entry point asks of its input: ``(contiguous tensor, dtype code, nd, x-fastest extents, x-fastest voxel
    sizes)``, extents and sizes padded to three.  Refused, in this order: what is no device array; a tensor not of 1 to 3
    dimensions (``who``: the operation in the text; None: the reference's text); an ``anisotropy`` -- None, a number, or one size
    per tensor axis -- of another length than the tensor has axes; a dtype without a code (``code=False``: not looked at, the
    caller does after its own arguments and the empty case)."""
    labels = as_device_tensor(labels)
    nd = labels.dim()
    if who is not None:
        _check_ndim(who, nd, "tensors")
    elif nd < 1 or nd > 3:
        raise TypeError("Multi-Label EDT library only supports up to 3 dimensions got {}.".format(nd))
    if anisotropy is not None:
        anisotropy = (float(anisotropy),) if np.ndim(anisotropy) == 0 else tuple(float(a) for a in anisotropy)
    ext, w = _xyz(labels.shape, anisotropy, nd)
    return labels.contiguous(), dtype_code(labels.dtype) if code else None, nd, ext, w


def _transform(labels, anisotropy, black_border, sqrt, force_generic=False, binary=False, signed=False):
    """signed: the signed transform where the shape is served (one transform), None returned where it is not"""
    labels = as_device_tensor(labels)
    if labels.numel() == 0:
        return torch.zeros(labels.shape, dtype=torch.float32, device=labels.device)
    labels, code, nd, ext, w = _input(labels, anisotropy)
    plan = _plan_for(ext[:nd], code, labels.device)
    if signed and not plan.signed_supported():
        return None
    return plan.run(labels, w[:nd], black_border, sqrt, force_generic=force_generic, binary=binary, signed=signed)


def binary_edtsq(labels: torch.Tensor, anisotropy=None, black_border=False) -> torch.Tensor:
    """``edt::binary_edtsq`` on a 2-D / 3-D device tensor of ANY label type (reference: src/edt.hpp:487-576, :681-755):
    labels split runs along x only; along y and z every non-zero voxel is one foreground."""
    labels = as_device_tensor(labels)
    if labels.dim() not in (2, 3):
        raise TypeError("binary_edtsq: 2-D or 3-D tensors")
    return _transform(labels, anisotropy, black_border, sqrt=False, binary=True)


def edtsq(labels: torch.Tensor, anisotropy=None, black_border=False) -> torch.Tensor:
    """Squared EDT of a device tensor (same semantics as :func:`edt.edtsq` on a C-ordered array)."""
    return _transform(labels, anisotropy, black_border, sqrt=False)


def edt(labels: torch.Tensor, anisotropy=None, black_border=False) -> torch.Tensor:
    return _transform(labels, anisotropy, black_border, sqrt=True)


def feature_transform(labels: torch.Tensor, anisotropy=None, black_border=False, force_generic=False) -> torch.Tensor:
    """Feature transform of a device tensor (semantics: :func:`edt.feature_transform` on a C-ordered array; anisotropy
    in tensor axis order).  Returns int32 of shape ``(labels.dim(),) + labels.shape`` on the same device: component k is
    the coordinate along tensor axis k.  The kernels write the components in ABI order (x, y, z: tensor axes last to
    first) and the result is a reordered COPY of them: at its peak the call holds twice the output (4 bytes per voxel
    and component each) besides the workspace, which is freed before the copy."""
    labels, _, nd, ext, w = _input(labels, anisotropy, "feature_transform", code=False)
    if labels.numel() == 0:
        return torch.zeros((nd,) + tuple(labels.shape), dtype=torch.int32, device=labels.device)
    code = dtype_code(labels.dtype)
    flags = (_lib.FLAG_BLACK_BORDER if black_border else 0) | (_lib.FLAG_FORCE_GENERIC if force_generic else 0)
    ws = _workspace("edt_hip_feature_workspace_bytes", code, nd, *ext, flags, device=labels.device, keep=False)
    planes = torch.empty((nd,) + tuple(labels.shape), dtype=torch.int32, device=labels.device)  # x, y, z planes
    _lib.check(_lib.load().edt_hip_feature_transform_device(_vp(labels), code, nd, *ext, *w, flags, _vp(planes), _vp(ws), ws.numel(),
                                                            _stream_ptr()))
    del ws
    return planes.flip(0)  # tensor axis k = plane nd-1-k


def expand_labels(labels: torch.Tensor, distance=1.0, anisotropy=None) -> torch.Tensor:
    """:func:`edt.expand_labels` on a device tensor (anisotropy in tensor axis order); same shape and dtype."""
    labels, _, nd, ext, w = _input(labels, anisotropy, "expand_labels", code=False)
    distance = float(distance)
    if not distance >= 0.0:
        raise ValueError(f"expand_labels: distance must be >= 0, got {distance}")
    if labels.numel() == 0:
        return labels.clone()
    code = dtype_code(labels.dtype)
    ws = _workspace("edt_hip_expand_labels_workspace_bytes", code, nd, *ext, device=labels.device, keep=False)
    out = torch.empty_like(labels)
    _lib.check(_lib.load().edt_hip_expand_labels_device(_vp(labels), code, nd, *ext, *w, distance, _vp(out), _vp(ws), ws.numel(),
                                                        _stream_ptr()))
    return out


def _stack2d(images, anisotropy, black_border, sqrt):
    images = as_device_tensor(images)
    if images.dim() != 3:
        raise TypeError("a stack of 2-D images is a 3-D tensor (count, height, width)")
    if images.numel() == 0:
        return torch.zeros(images.shape, dtype=torch.float32, device=images.device)
    an = (1.0, 1.0) if anisotropy is None else tuple(float(a) for a in anisotropy)
    if len(an) != 2:
        raise ValueError("anisotropy of a 2-D image has 2 entries")
    images, code, _, ext, _ = _input(images)   # (width, height, count): x fastest
    return _plan_for(ext, code, images.device).run(images, (an[1], an[0], 1.0), black_border, sqrt, batch2d=True)


def edtsq_stack(images: torch.Tensor, anisotropy=None, black_border=False) -> torch.Tensor:
    """Squared EDT of every image of a stack ``(count, height, width)`` independently -- one launch per pass for
    the whole stack (EDT_FLAG_BATCH_2D), so that many small images fill the chip.  Same result as calling
    :func:`edtsq` on each image."""
    return _stack2d(images, anisotropy, black_border, sqrt=False)


def edt_stack(images: torch.Tensor, anisotropy=None, black_border=False) -> torch.Tensor:
    return _stack2d(images, anisotropy, black_border, sqrt=True)


def sdf(labels: torch.Tensor, anisotropy=None, black_border=False) -> torch.Tensor:
    """``edt(x) - edt(x == 0)`` without leaving the device (reference: src/edt.pyx:148-158) -- as ONE transform where the
    shape allows (EDT_FLAG_SIGNED: label 0 measured like every label, its voxels negated; bit-identical to the definition,
    whose two fields have disjoint supports), else as the two transforms and the subtraction."""
    return _signed(labels, anisotropy, black_border, sqrt=True)


def sdfsq(labels: torch.Tensor, anisotropy=None, black_border=False) -> torch.Tensor:
    """``edtsq(x) - edtsq(x == 0)`` without leaving the device (reference: src/edt.pyx:161-202)."""
    return _signed(labels, anisotropy, black_border, sqrt=False)


def _signed(labels, anisotropy, black_border, sqrt, one_transform=True):
    lib = _lib.load()
    labels = as_device_tensor(labels).contiguous()
    if labels.numel() == 0:
        return torch.zeros(labels.shape, dtype=torch.float32, device=labels.device)
    if one_transform and 2 <= labels.dim() <= 3:
        dt = _transform(labels, anisotropy, black_border, sqrt=sqrt, signed=True)
        if dt is not None:
            return dt
    dt = _transform(labels, anisotropy, black_border, sqrt=sqrt)
    mask = torch.empty(labels.shape, dtype=torch.bool, device=labels.device)
    _lib.check(lib.edt_hip_is_background_device(
        ctypes.c_void_p(labels.data_ptr()), dtype_code(labels.dtype),
        ctypes.c_void_p(mask.data_ptr()), labels.numel(), _stream_ptr()))
    bg = _transform(mask, anisotropy, black_border, sqrt=sqrt)
    _lib.check(lib.edt_hip_subtract_device(
        ctypes.c_void_p(dt.data_ptr()), ctypes.c_void_p(bg.data_ptr()),
        ctypes.c_void_p(dt.data_ptr()), dt.numel(), _stream_ptr()))
    return dt


def edtsq_voxel_graph(labels: torch.Tensor, voxel_graph: torch.Tensor, anisotropy=None,
                      black_border=False) -> torch.Tensor:
    """Squared EDT with a voxel connectivity graph (reference: edt.edtsq(..., voxel_graph=g),
    src/edt.pyx:736-845) on device tensors: a 2-D or 3-D labels tensor and a uint8 graph of the same shape
    (C order; bit layout of the reference).  Everything stays in HBM (edt_hip_edtsq_voxel_graph_device)."""
    labels, voxel_graph = as_device_tensor(labels), as_device_tensor(voxel_graph)
    if labels.dim() not in (2, 3) or voxel_graph.shape != labels.shape or voxel_graph.dtype != torch.uint8:
        raise TypeError("voxel_graph needs a 2-D or 3-D volume and a uint8 graph of the same shape")
    # a C-ordered tensor (z, y, x) is the x-fastest volume with extents and weights reversed
    labels, code, ndim, ext, w = _input(labels, anisotropy)
    voxel_graph = voxel_graph.contiguous()
    out = torch.empty(labels.shape, dtype=torch.float32, device=labels.device)
    ws = _workspace("edt_hip_voxel_graph_workspace_bytes", ndim, *ext, device=labels.device, keep=False)
    _lib.check(_lib.load().edt_hip_edtsq_voxel_graph_device(
        _vp(labels), code, _vp(voxel_graph), ndim, *ext, *w, _lib.FLAG_BLACK_BORDER if black_border else 0, _vp(out), _vp(ws),
        ws.numel(), _stream_ptr()))
    return out


def _key_buffer(code: int, key) -> np.ndarray:
    """The key of :func:`select_label` in the labels' own representation.  Signed labels are compared as their bit
    patterns, so an integer key may be given signed or unsigned (-1 and 2^64 - 1 both select the all-ones int64 / uint64
    label); a float key of integer labels is truncated towards zero, as numpy's cast does."""
    if code in (_lib.U8, _lib.U16, _lib.U32, _lib.U64):
        bits = 8 * _lib.DTYPE_SIZE[code]
        k = int(key)
        if not -(1 << (bits - 1)) <= k < (1 << bits):
            raise OverflowError(f"key {key!r} does not fit a {bits}-bit label")
        return np.array([k % (1 << bits)], dtype=_NP_OF_CODE[code])
    return np.array([key], dtype=_NP_OF_CODE[code])


def select_label(labels: torch.Tensor, dt: torch.Tensor, key, out: torch.Tensor = None) -> torch.Tensor:
    """``dt`` where ``labels == key``, 0 elsewhere -- the image :func:`edt.each` yields for one label,
    as one streaming kernel (edt_hip_select_label_device)."""
    labels, dt = as_device_tensor(labels), as_device_tensor(dt)
    if labels.shape != dt.shape or dt.dtype != torch.float32:
        raise ValueError("dt must be a float32 tensor of the labels' shape")
    labels, dt = labels.contiguous(), dt.contiguous()
    if out is None:
        out = torch.empty_like(dt)
    code = dtype_code(labels.dtype)
    host = _key_buffer(code, key)
    _lib.check(_lib.load().edt_hip_select_label_device(
        ctypes.c_void_p(labels.data_ptr()), code, ctypes.c_void_p(dt.data_ptr()),
        ctypes.c_void_p(host.ctypes.data), ctypes.c_void_p(out.data_ptr()), labels.numel(), _stream_ptr()))
    return out


def runs(labels: torch.Tensor):
    """Device-side ``extract_runs`` (reference: src/edt_voxel_graph.hpp:238-268): the maximal constant runs of
    the flattened (C-order) tensor as three device tensors ``(starts, ends, values)``, in memory order
    (run k covers ``[starts[k], ends[k])`` and holds ``values[k]``).  Two enqueue-only kernels sweeps
    (edt_hip_extract_runs_device); the only host synchronisation is reading the run count."""
    lib = _lib.load()
    labels = as_device_tensor(labels).contiguous()
    n = labels.numel()
    dev = labels.device
    if n == 0:
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        return z, z.clone(), labels.reshape(-1)
    code = dtype_code(labels.dtype)
    ws = _workspace("edt_hip_runs_workspace_bytes", n, device=dev, keep=False)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    lp, cp, wp = ctypes.c_void_p(labels.data_ptr()), ctypes.c_void_p(count.data_ptr()), ctypes.c_void_p(ws.data_ptr())
    _lib.check(lib.edt_hip_extract_runs_device(lp, code, n, None, 0, cp, wp, ws.numel(), _stream_ptr()))
    nruns = int(count.item())
    starts = torch.empty(nruns, dtype=torch.int64, device=dev)
    _lib.check(lib.edt_hip_extract_runs_device(lp, code, n, ctypes.c_void_p(starts.data_ptr()), nruns, cp, wp,
                                               ws.numel(), _stream_ptr()))
    ends = torch.empty_like(starts)
    ends[:-1] = starts[1:]
    ends[-1] = n
    return starts, ends, labels.reshape(-1)[starts]


class _DeviceLabelImages:
    """Sized iterable behind :func:`each`: the run table of the labels is extracted once on the device; every
    label's image is then produced by ONE streaming kernel over just the span of memory its runs cover
    (first run start .. last run end) instead of the whole volume."""

    def __init__(self, labels, dt, reuse):
        labels, dt = as_device_tensor(labels), as_device_tensor(dt)
        if labels.shape != dt.shape or dt.dtype != torch.float32:
            raise ValueError("dt must be a float32 tensor of the labels' shape")
        self.labels, self.dt, self.reuse = labels.contiguous(), dt.contiguous(), reuse
        starts, ends, values = runs(self.labels)
        keep = values != 0
        starts, ends, values = starts[keep], ends[keep], values[keep]
        self.keys, inverse = torch.unique(values, return_inverse=True)   # over RUNS, not voxels
        nk = self.keys.numel()
        big = self.labels.numel()
        lo = torch.full((nk,), big, dtype=torch.int64, device=labels.device).scatter_reduce(0, inverse, starts, "amin")
        hi = torch.zeros((nk,), dtype=torch.int64, device=labels.device).scatter_reduce(0, inverse, ends, "amax")
        self._keys, self._lo, self._hi = self.keys.tolist(), lo.tolist(), hi.tolist()

    def __len__(self):
        return len(self._keys)

    def _select(self, key, lo, hi, out):
        lab, dt, flat = self.labels.reshape(-1), self.dt.reshape(-1), out.reshape(-1)
        select_label(lab[lo:hi], dt[lo:hi], key, out=flat[lo:hi])

    def __iter__(self):
        shared = torch.zeros_like(self.dt) if self.reuse else None
        prev = None
        for key, lo, hi in zip(self._keys, self._lo, self._hi):
            if self.reuse:
                if prev is not None:
                    shared.reshape(-1)[prev[0]:prev[1]].zero_()   # wipe only what the previous label wrote
                out = shared
                prev = (lo, hi)
            else:
                out = torch.zeros_like(self.dt)
            self._select(key, lo, hi, out)
            yield key, out


def each(labels: torch.Tensor, dt: torch.Tensor, in_place: bool = False):
    """Device-resident :func:`edt.each` (reference: src/edt.pyx:950-994): an iterable of
    ``(label, image)`` with ``image = dt`` restricted to that label, zeros elsewhere; the label 0 is
    skipped.  ``in_place=True`` reuses ONE output tensor for every label (the reference's read-only
    in-place image).  The DT never leaves the device."""
    return _DeviceLabelImages(labels, dt, bool(in_place))


_SIGNED_TORCH = (torch.int8, torch.int16, torch.int32, torch.int64)


default_max_labels = _lib.default_max_labels


def _table(who, labels, code, max_labels, columns, query, call, keep):
    """The device side of :func:`edt._args._label_table`: ``columns``, the (dtype, row shape) of every output column behind the
    keys, allocated per attempt together with the int64 device word for the number of labels and the workspace of ``query``
    (``keep``: as :func:`_workspace`); ``call(cap, tail)``, the device entry point, ``tail`` being its arguments from the columns
    on.  Returns the columns cut to the labels found and, for signed dtypes, brought into signed order."""
    dev = labels.device

    def attempt(cap):
        cols = [torch.empty((cap,) + shape, dtype=dtype, device=dev) for dtype, shape in [(labels.dtype, ())] + columns]
        count = torch.empty(1, dtype=torch.int64, device=dev)
        ws = _workspace(query, code, labels.numel(), cap, device=dev, keep=keep)
        _lib.check(call(cap, [*map(_vp, cols), _vp(count), _vp(ws), ws.numel(), _stream_ptr()]))
        return int(count.item()), cols  # the only host synchronisation

    cols = _label_table(who, code, labels.numel(), max_labels, attempt)
    if labels.dtype in _SIGNED_TORCH:   # the ABI orders bit patterns: negative keys come last there
        perm = torch.argsort(cols[0], stable=True)
        cols = [c[perm] for c in cols]
    return cols


def _no_rows(cls, labels, nd):
    return _empty_table(cls, nd, lambda name, shape: torch.zeros(shape, dtype=labels.dtype if name is None else getattr(torch, name),
                                                                 device=labels.device))


def label_stats(labels: torch.Tensor, dt: torch.Tensor, max_labels=None) -> LabelStats:
    """One table row per distinct non-zero label, in one or two streaming sweeps over ``labels`` and ``dt`` (contract:
    include/edt_hip.h, "label_stats"): ``(labels, counts, max, argmax, bbox_lo, bbox_hi)`` as device tensors --
    the label values ascending (signed dtypes in signed order, as :func:`each` yields them), the voxel count (int64), the
    largest ``dt`` of the label (float32), the coordinates ``(n, ndim)`` along the tensor's axes of the first voxel, in
    memory order, that attains it (int64), and the inclusive bounding box per tensor axis (int32, ``(n, ndim)`` each).
    ``dt``: any NaN-free float32 tensor of the labels' shape (edt, sdf ...).  The only host synchronisation is reading
    the number of labels.  ``max_labels=None``: exact for 8/16-bit labels, else room for 65536 labels, retried with 8x
    the room while it proves too small; an explicit ``max_labels`` that proves too small raises ``ValueError``."""
    labels, dt = as_device_tensor(labels), as_device_tensor(dt)
    if labels.shape != dt.shape or dt.dtype != torch.float32:
        raise ValueError("dt must be a float32 tensor of the labels' shape")
    labels, code, nd, ext, _ = _input(labels, None, "label_stats")
    _check_max_labels("label_stats", max_labels)
    if labels.numel() == 0:
        return _no_rows(LabelStats, labels, nd)
    dt = dt.contiguous()
    keys, counts, mx, arg, bbox = _table(
        "label_stats", labels, code, max_labels, [(torch.int64, ()), (torch.float32, ()), (torch.int64, ()), (torch.int32, (6,))],
        "edt_hip_label_stats_workspace_bytes",
        lambda cap, tail: _lib.load().edt_hip_label_stats_device(_vp(labels), code, _vp(dt), nd, *ext, cap, *tail), keep=False)
    coords = []
    for extent in ext[:nd]:            # x, y, z of the flat index
        coords.append(arg % extent)
        arg = arg // extent
    argmax = torch.stack(coords[::-1], dim=1)
    lo = bbox[:, 0:2 * nd:2].flip(1).contiguous()
    hi = bbox[:, 1:2 * nd:2].flip(1).contiguous()
    return LabelStats(keys, counts, mx, argmax, lo, hi)


def label_moments(labels: torch.Tensor, max_labels=None) -> LabelMoments:
    """Device-resident :func:`edt.label_moments`: one table row per distinct non-zero label in ONE streaming sweep over
    ``labels``, nothing else is read (contract: include/edt_hip.h, "label_moments").  The named tuple
    ``(labels, counts, first, second, centroid, covariance)`` of device tensors, every field per tensor axis: the label values
    ascending (signed dtypes in signed order), the voxel count, the exact raw first ``(n, ndim)`` and second ``(n, ndim, ndim)``
    moments (int64), centroid and population covariance in voxel units (float64).  The table stays on the device; the only
    host synchronisation is reading the number of labels.  ``max_labels`` and the range bound: as :func:`edt.label_moments`."""
    labels, code, nd, ext, _ = _input(labels, None, "label_moments")
    _check_max_labels("label_moments", max_labels)
    if labels.numel() == 0:
        return _no_rows(LabelMoments, labels, nd)
    _moments.check_range(labels.shape)
    keys, counts, sums, centroid, central = _table(
        "label_moments", labels, code, max_labels, [(torch.int64, ()), (torch.int64, (9,)), (torch.float64, (3,)), (torch.float64, (6,))],
        "edt_hip_label_moments_workspace_bytes",
        lambda cap, tail: _lib.load().edt_hip_label_moments_device(_vp(labels), code, nd, *ext, cap, *tail), keep=False)
    return _moments.assemble(keys, counts, sums, centroid, central, nd, True)


_workspaces: dict = {}         # query name -> {(bytes, device, stream): scratch}


def _workspace(query, *query_args, device, keep) -> torch.Tensor:
    """The scratch of one library call: ``query(*query_args)`` bytes on ``device``; a query that answers 0 is a ``ValueError``.

    ``keep=True``: one buffer per query name, byte count, device and current stream (a workspace is only ever used on the stream
    it was allocated for; calls that need the same bytes share it, whatever their shape or dtype: every call initialises what it
    reads).  At most 9 are kept per query name, and the one cached longest ago makes room for a new one.
    ``keep=False``: allocated for this call and freed with it.

    Who keeps: connected_components, fill_holes, dust (on fill_holes' query), watershed, label_topology, erode / opening / closing,
    local_thickness and medial_axis.  Who does not: feature_transform (which frees it before it reorders its planes),
    expand_labels (and so dilate), edtsq_voxel_graph, runs, label_stats and label_moments.  The transforms have their scratch in
    a :class:`Plan`."""
    nbytes = int(getattr(_lib.load(), query)(*query_args))
    if nbytes == 0:
        raise ValueError(f"{query}{query_args} is 0: this dtype, shape (at most 2^31 - 1 voxels for the label operations) or "
                         "flags is not served")
    if not keep:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    cache = _workspaces.setdefault(query, {})
    key = (nbytes, str(device), torch.cuda.current_stream(device).cuda_stream)
    if key not in cache:
        if len(cache) > 8:
            del cache[next(iter(cache))]
        cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return cache[key]


def label_topology(labels: torch.Tensor, max_labels=None) -> LabelTopology:
    """Device-resident :func:`edt.label_topology`: one table row per distinct non-zero label in ONE sweep over ``labels``,
    nothing else is read (contract: include/edt_hip.h, "label_topology").  The named tuple ``(labels, counts, closed, interior)``
    of device tensors: the label values ascending (signed dtypes in signed order), the voxel count and the two int64 cell-count
    tables of shape ``(n,) + (2,) * ndim`` per tensor axis.  ``euler``, ``intrinsic_volumes`` and ``surface_area`` of the result
    bring the table to the host.  The table stays on the device; the only host synchronisation is reading the number of labels.
    The scratch is cached per size and stream.  ``max_labels``: as :func:`edt.label_topology`."""
    labels, code, nd, ext, _ = _input(labels, None, "label_topology")
    _check_max_labels("label_topology", max_labels)
    if labels.numel() == 0:
        return _no_rows(LabelTopology, labels, nd)
    keys, closed, interior = _table(
        "label_topology", labels, code, max_labels, [(torch.int64, (8,)), (torch.int64, (8,))], "edt_hip_label_topology_workspace_bytes",
        lambda cap, tail: _lib.load().edt_hip_label_topology_device(_vp(labels), code, nd, *ext, cap, *tail), keep=True)
    return _topology.assemble(keys, closed, interior, nd, True)


def connected_components(labels: torch.Tensor, connectivity=None, binary=False):
    """:func:`edt.connected_components` on a device array (semantics of a C-ordered array: the last tensor axis is
    fastest, and components are numbered in the tensor's memory order; contract: include/edt_hip.h, "connected
    components").  Returns ``(out, n)``: ``out`` an int32 tensor of the labels' shape -- 0 for background, else the
    component's number in ``1..N`` (at most 2^31 - 1 voxels, so the numbers fit) -- and ``n`` a 0-dim int64 DEVICE tensor
    holding ``N``: the call only enqueues kernels on the current stream, nothing is read back and nothing waits.  The
    scratch (one word per 2048 voxels) is cached per shape and stream.

    The result composes without leaving the device: ``label_stats(out, dt)`` is then a table per OBJECT,
    ``each(out, dt)`` yields one image per object, and ``edt(out)`` is the transform of the instances."""
    labels, code, nd, ext, _ = _input(labels, None, "connected_components")
    c = _connectivity(connectivity, nd)
    out = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
    if labels.numel() == 0:
        return out, torch.zeros((), dtype=torch.int64, device=labels.device)
    n = torch.empty((), dtype=torch.int64, device=labels.device)
    ws = _workspace("edt_hip_components_workspace_bytes", code, nd, *ext, device=labels.device, keep=True)
    _lib.check(_lib.load().edt_hip_connected_components_device(_vp(labels), code, nd, *ext, c, 1 if binary else 0, _vp(out),
                                                               _vp(n), _vp(ws), ws.numel(), _stream_ptr()))
    return out, n


def fill_holes(labels: torch.Tensor, connectivity=None, binary=False):
    """:func:`edt.fill_holes` on a device array (semantics of a C-ordered array: the last tensor axis is fastest;
    contract: include/edt_hip.h, "fill holes").  ``connectivity=None`` means 1, the adjacency of the background.
    Returns ``(out, n_filled)``: ``out`` a new tensor of the labels' dtype and shape, ``n_filled`` a 0-dim int64 DEVICE
    tensor: the call only enqueues kernels on the current stream, nothing is read back and nothing waits.  The scratch
    (4 bytes per voxel) is cached per shape and stream.

    ``edt(fill_holes(x)[0])`` is then the transform of the filled segmentation without a trip to the host."""
    labels, code, nd, ext, _ = _input(labels, None, "fill_holes")
    c = _connectivity(connectivity, nd, default=1, who="fill_holes")
    if labels.numel() == 0:
        return labels.clone(), torch.zeros((), dtype=torch.int64, device=labels.device)
    out = torch.empty(labels.shape, dtype=labels.dtype, device=labels.device)
    n = torch.empty((), dtype=torch.int64, device=labels.device)
    ws = _workspace("edt_hip_fill_holes_workspace_bytes", code, nd, *ext, device=labels.device, keep=True)
    _lib.check(_lib.load().edt_hip_fill_holes_device(_vp(labels), code, nd, *ext, c, 1 if binary else 0, _vp(out), _vp(n),
                                                     _vp(ws), ws.numel(), _stream_ptr()))
    return out, n


def dust(labels: torch.Tensor, threshold, connectivity=None, binary=False, invert=False, in_place=False):
    """:func:`edt.dust` on a device array (semantics of a C-ordered array: the last tensor axis is fastest; contract:
    include/edt_hip.h, "dust").  Neither cc3d nor skimage is on the build machine: what is tested is the header's contract,
    not their behaviour.  Returns ``(out, counts)``: ``out`` a new tensor of the labels' dtype and shape -- under
    ``in_place=True`` the (contiguous) input tensor itself, filtered where it lies -- and ``counts`` an int64[3] DEVICE
    tensor (components found, components kept, voxels removed): the call only enqueues kernels on the current stream,
    nothing is read back and nothing waits.  The scratch (4 bytes per voxel, the size of fill_holes') is cached per shape
    and stream, together with fill_holes'.

    ``edt(fill_holes(dust(x, t)[0])[0])`` is then the transform of the cleaned segmentation without a trip to the host."""
    raw = as_device_tensor(labels)
    labels, code, nd, ext, _ = _input(raw, None, "dust")
    lo, hi = _dust_bounds(threshold)
    c = _connectivity(connectivity, nd, who="dust")
    if in_place and not raw.is_contiguous():
        raise ValueError("dust: in_place needs a contiguous tensor")
    if labels.numel() == 0:
        return (labels if in_place else labels.clone()), torch.zeros(3, dtype=torch.int64, device=labels.device)
    out = labels if in_place else torch.empty(labels.shape, dtype=labels.dtype, device=labels.device)
    counts = torch.empty(3, dtype=torch.int64, device=labels.device)
    ws = _workspace("edt_hip_fill_holes_workspace_bytes", code, nd, *ext, device=labels.device, keep=True)
    _lib.check(_lib.load().edt_hip_dust_device(_vp(labels), code, nd, *ext, c, 1 if binary else 0, lo, hi, 1 if invert else 0,
                                               _vp(out), _vp(counts), _vp(ws), ws.numel(), _stream_ptr()))
    return out, counts


def watershed(labels: torch.Tensor, field: torch.Tensor = None, min_saliency=0.0, connectivity=None, anisotropy=None,
              black_border=False, binary=False):
    """:func:`edt.watershed` on a device array (semantics of a C-ordered array: the last tensor axis is fastest, and basins are
    numbered in the tensor's memory order; contract: include/edt_hip.h, "watershed"): the STEEPEST-ASCENT watershed ("drop of
    water", hill climbing) as the connected components of a graph.  It is not ``skimage.segmentation.watershed``: no markers,
    boundaries by the ascent rule and not a flooding order, ties to the greatest neighbour and not the steepest slope (so
    anisotropy enters through the field only); ``min_saliency`` is one round of single-linkage merging, not the h-maxima
    hierarchy.  Neither skimage nor cc3d is on the build machine: what is tested is the header's contract.

    ``field``: a float32 device tensor of the labels' shape; it is NOT looked at -- a NaN on a foreground voxel leaves the
    partition unspecified (the call still terminates, with numbers in ``0..N``).  ``field=None`` calls
    ``edt(labels, anisotropy, black_border)`` first, on ``labels != 0`` under ``binary``.
    Returns ``(out, n)``: ``out`` an int32 tensor of the labels' shape -- 0 for background, else the basin's number in ``1..N``
    -- and ``n`` a 0-dim int64 DEVICE tensor holding ``N``: the call only enqueues kernels on the current stream, nothing is read
    back and nothing waits.  The scratch (4 bytes per voxel, the size of fill_holes') is cached per shape and stream.

    ``label_stats(watershed(x)[0], dt)`` is then a table per SPLIT object, without leaving the device."""
    labels, code, nd, ext, _ = _input(labels, None, "watershed")
    c = _connectivity(connectivity, nd, who="watershed")
    h = _min_saliency(min_saliency)
    if field is not None:
        field = as_device_tensor(field)
        if field.shape != labels.shape or field.dtype != torch.float32 or field.device != labels.device:
            raise ValueError("watershed: field must be a float32 tensor of the labels' shape on their device")
    out = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
    if labels.numel() == 0:
        return out, torch.zeros((), dtype=torch.int64, device=labels.device)
    if field is None:
        field = edt(labels != 0 if binary and labels.dtype != torch.bool else labels, anisotropy, black_border)
    field = field.contiguous()
    n = torch.empty((), dtype=torch.int64, device=labels.device)
    ws = _workspace("edt_hip_watershed_workspace_bytes", code, nd, *ext, device=labels.device, keep=True)
    _lib.check(_lib.load().edt_hip_watershed_device(_vp(labels), code, nd, *ext, _vp(field), c, 1 if binary else 0, h, _vp(out),
                                                    _vp(n), _vp(ws), ws.numel(), _stream_ptr()))
    return out, n


def _morph_select(code, values, field, radius, rule, out=None, mask=None, guard=None):
    """edt_hip_morph_select_device over ``field.numel()`` voxels; ``code``: the dtype code of values / guard / out"""
    _lib.check(_lib.load().edt_hip_morph_select_device(
        None if values is None else _vp(values), None if guard is None else _vp(guard), code, _vp(field), radius, rule,
        None if out is None else _vp(out), None if mask is None else _vp(mask), field.numel(), _stream_ptr()))


def _morph_input(labels, radius, anisotropy, who, in_place=False, inf_allowed=False):
    raw = as_device_tensor(labels)
    r = _morph_radius(radius, who, inf_allowed)
    if in_place and not raw.is_contiguous():
        raise ValueError(f"{who}: in_place needs a contiguous tensor")
    return (*_input(raw, anisotropy, who), r)


def _morphology(who, op, labels, radius, anisotropy, flags=0, in_place=False):
    """One call of edt_hip_morphology_device on the current stream, on the cached workspace of its size."""
    labels, code, nd, ext, w, r = _morph_input(labels, radius, anisotropy, who, in_place)
    if labels.numel() == 0:
        return labels if in_place else labels.clone()
    ws = _workspace("edt_hip_morphology_workspace_bytes", code, nd, *ext, op, flags, device=labels.device, keep=True)
    out = labels if in_place else torch.empty_like(labels)
    _lib.check(_lib.load().edt_hip_morphology_device(_vp(labels), code, nd, *ext, *w, op, r, flags, _vp(out), _vp(ws), ws.numel(),
                                                     _stream_ptr()))
    return out


def erode(labels: torch.Tensor, radius=1.0, anisotropy=None, black_border=False, binary=False, in_place=False) -> torch.Tensor:
    """:func:`edt.erode` on a device array (semantics of a C-ordered array; anisotropy in tensor axis order; contract:
    include/edt_hip.h, "morphology"): one transform and one streaming select on the current stream, nothing read back.
    ``in_place=True`` writes the result into the (contiguous) input tensor and returns it."""
    return _morphology("erode", _lib.MORPH_ERODE, labels, radius, anisotropy, _morph_flags(black_border, binary), in_place)


def dilate(labels: torch.Tensor, radius=1.0, anisotropy=None) -> torch.Tensor:
    """:func:`edt.dilate` on a device array: exactly :func:`expand_labels`."""
    labels, *_, r = _morph_input(labels, radius, anisotropy, "dilate", inf_allowed=True)
    return expand_labels(labels, r, anisotropy)


def opening(labels: torch.Tensor, radius=1.0, anisotropy=None, black_border=False, binary=False, in_place=False) -> torch.Tensor:
    """:func:`edt.opening` on a device array: the transform of the labels, the mask of what the erosion removes, its
    binary transform, and the select of the voxels within ``radius`` of what survived -- two transforms and two streaming
    kernels on the current stream.  ``in_place=True`` writes the result into the (contiguous) input tensor and returns it."""
    return _morphology("opening", _lib.MORPH_OPEN, labels, radius, anisotropy, _morph_flags(black_border, binary), in_place)


def closing(labels: torch.Tensor, radius=1.0, anisotropy=None) -> torch.Tensor:
    """:func:`edt.closing` on a device array: :func:`expand_labels`, the binary transform of what it left empty, and the
    select that keeps the input's voxels and the new voxels farther than ``radius`` from the emptiness."""
    return _morphology("closing", _lib.MORPH_CLOSE, labels, radius, anisotropy)


def local_thickness(labels: torch.Tensor, radii=None, anisotropy=None, black_border=False, binary=False, return_sizes=False):
    """:func:`edt.local_thickness` on a device array (semantics of a C-ordered array; anisotropy in tensor axis order; contract:
    include/edt_hip.h, "local thickness"): one call of edt_hip_local_thickness_device on the cached workspace of its size -- the
    transform of the labels once, then per radius the binary transform of the mask the step before left and one streaming
    step.  Returns the float32 thickness, a new tensor; with ``return_sizes=True`` the pair ``(thickness, ThicknessSizes(radii,
    voxels))`` with ``radii`` a float64 numpy array (the radii used) and ``voxels`` an int64 DEVICE tensor.  With explicit
    ``radii`` the call only enqueues kernels on the current stream -- nothing is read back, and it can be captured into a graph.
    ``radii=None`` SYNCHRONISES once: the largest finite squared distance (4 bytes) is read back to build the ladder; on a
    stream that is being captured it is refused (``EdtHipError``)."""
    raw = as_device_tensor(labels)
    r = None if radii is None else _thickness_radii(radii)
    labels, code, nd, ext, w = _input(raw, anisotropy, "local_thickness")
    if labels.numel() == 0:
        T = torch.zeros(labels.shape, dtype=torch.float32, device=labels.device)
        used = np.zeros(0, dtype=np.float64) if r is None else r
        return (T, ThicknessSizes(used, torch.zeros(used.size, dtype=torch.int64, device=labels.device))) if return_sizes else T
    step, room = (0.0, r.size) if r is not None else _ladder_room(ext[:nd], w[:nd])
    flags = _morph_flags(black_border, binary)
    ws = _workspace("edt_hip_local_thickness_workspace_bytes", code, nd, *ext, flags, device=labels.device, keep=True)
    T = torch.empty(labels.shape, dtype=torch.float32, device=labels.device)
    sizes = torch.empty(room, dtype=torch.int64, device=labels.device)
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().edt_hip_local_thickness_device(
        _vp(labels), code, nd, *ext, *w, flags, None if r is None else ctypes.c_void_p(r.ctypes.data), room, step, _vp(T), _vp(sizes),
        ctypes.byref(n), _vp(ws), ws.numel(), _stream_ptr()))
    if not return_sizes:
        return T
    k = int(n.value)
    return T, ThicknessSizes(r if r is not None else np.arange(1, k + 1, dtype=np.float64) * step, sizes[:k])


def medial_axis(labels: torch.Tensor, gamma=None, min_angle=0.0, anisotropy=None, black_border=False, binary=False,
                return_distance=False):
    """:func:`edt.medial_axis` on a device array (semantics of a C-ordered array; anisotropy in tensor axis order; contract:
    include/edt_hip.h, "medial axis"): one call of edt_hip_medial_axis_device -- the mask under binary, the feature transform,
    the distance transform where the radius is wanted, and one streaming stencil, all enqueued on the current stream; nothing is
    read back.  The workspace is cached by its size and stream: a second call of one shape allocates only what it returns.
    Returns a new tensor of the labels' dtype and shape; with ``return_distance=True`` the pair ``(axis, distance)``, distance
    float32."""
    raw = as_device_tensor(labels)
    ratio = _medial_ratio(min_angle)
    labels, code, nd, ext, w = _input(raw, anisotropy, "medial_axis")
    g = _medial_gamma(gamma, w[:nd])
    if labels.numel() == 0:
        return (labels.clone(), torch.zeros(labels.shape, dtype=torch.float32, device=labels.device)) if return_distance else labels.clone()
    flags = _morph_flags(black_border, binary)
    ws = _workspace("edt_hip_medial_axis_workspace_bytes", code, nd, *ext, flags, 1 if return_distance else 0, device=labels.device,
                    keep=True)
    out = torch.empty_like(labels)
    radius = torch.empty(labels.shape, dtype=torch.float32, device=labels.device) if return_distance else None
    _lib.check(_lib.load().edt_hip_medial_axis_device(
        _vp(labels), code, nd, *ext, *w, flags, g, ratio, _vp(out), None if radius is None else _vp(radius), _vp(ws), ws.numel(),
        _stream_ptr()))
    return (out, radius) if return_distance else out


def pass_times():
    """Durations (ms) of the kernels of the last profiled call, as ``[(name, ms), ...]``."""
    lib = _lib.load()
    cap = 256  # (the sharded phases log several calls per step)
    buf = (ctypes.c_float * cap)()
    n = lib.edt_hip_get_pass_times(ctypes.cast(buf, ctypes.c_void_p), cap)
    return [(lib.edt_hip_get_pass_name(i).decode(), float(buf[i])) for i in range(min(n, cap))]


def set_profiling(enabled: bool) -> None:
    _lib.check(_lib.load().edt_hip_set_profiling(1 if enabled else 0))
