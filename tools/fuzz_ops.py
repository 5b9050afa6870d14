#!/usr/bin/env python3
"""Seeded randomised runs of the label operations against their numpy oracles, bit for bit, in the manner of tools/fuzz_gpu.py.
Three families, each round-robin over its operations:

  label      connected_components, fill_holes, dust, label_stats, feature_transform and expand_labels (OPS);
  field      erode, opening, dilate, closing, local_thickness and medial_axis (FIELD_OPS): the compositions of
             csrc/edt_fieldops.hip;
  noquantum  feature_transform, expand_labels, dilate, closing, medial_axis, erode, opening and local_thickness (NOQUANTUM_OPS)
             at voxel sizes the library finds no quantum for: the fp64 kernels of csrc/edt_feature.hip and the fp32 column
             kernels of the distance transform.

usage: python tools/fuzz_ops.py [ncases] [seed] [label|field|noquantum]

One MISMATCH line per failing case, one line of per-operation counts, a last line `N cases, M mismatches`; the exit status is
non-zero on any mismatch.  ``cases(seed, n, ops)`` is the generator on its own (numpy only): the CPU tier draws the same inputs
and holds the oracles against a second opinion (tests/test_fuzz_ops_cpu.py; label family: seeds 701..703, field family: seeds
711..713, noquantum family: seeds 721..723).

A case: 1 to 3 dimensions in C or F order; an x extent from the lengths where 64-voxel groups, 256-voxel cuts and row kernels
change (or 1..90), the other extents 1..40, the last ones clipped to the case's cap; blocks, noise near the percolation
threshold, a solid with pin-holes, per-voxel labels, a serpentine or a comb; each of the eleven label dtypes in turn, every
fifth case with the full-width palette (extreme keys, NaN, -0.0); a connectivity 1..ndim, binary or not.  The call goes through
edt.device.* on device buffers at a random element offset (tests/synth.py: offset_view; the buffers, surroundings included, must
come back unchanged), every fifth case through the host module edt.* as well, and the two must agree.

A field case is drawn the same way and adds voxel sizes that share a quantum (the QUANTUM table of
tests/test_gpu_feature_transform.py, cut to the dimensions), black_border and binary where the operation takes them, and a radius
of 0, 1, 1.5, 2 or 3 times the smallest voxel size (+inf too for dilate): the integer multiples have squares that the field
attains, so the `>` / `<=` ties of the selects are hit on purpose.  local_thickness takes the default ladder on every third case
and 1 to 4 ascending radii of the same multiples otherwise, always with its sizes; medial_axis a gamma of None, 0 or 1.5 times the
smallest voxel size, a min_angle of 0, 60 or 120 degrees, and the radius function on every second case.  erode, opening and
local_thickness are held against the compiled CPU transform (tests/morph_oracle.py, tests/thickness_oracle.py), dilate, closing and
medial_axis against the pure-Python feature transform (tests/ft_oracle.py, tests/medial_oracle.py), hence their smaller cap.

A noquantum case is drawn the same way again.  feature_transform, expand_labels, dilate, closing and medial_axis take their sizes
from the EXACT table of tests/noquantum_cases.py (squares exact in fp32, but factors beyond the 16-bit windows: the fp64 kernels
are exact there, so the same oracles hold bit for bit with ft_oracle.exact_factors), in 2-D and 3-D only -- a 1-D cut always has
a quantum; expand_labels' distance is 0, 1 or 2.5 times the smallest size or +inf, and D is formed from the fp64 squares of the
sizes, as the header has it.  erode, opening and local_thickness, whose oracle is exact for any size, take theirs from EXACT and
INEXACT in turn, in 1-D to 3-D."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "euclidean-distance-transform-3d_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from synth import blocky_labels, palette  # noqa: E402

OPS = ("connected_components", "fill_holes", "dust", "label_stats", "feature_transform", "expand_labels")
FIELD_OPS = ("erode", "opening", "dilate", "closing", "local_thickness", "medial_axis")
NOQUANTUM_OPS = ("feature_transform", "expand_labels", "dilate", "closing", "medial_axis", "erode", "opening", "local_thickness")
NOQUANTUM_EXACT_OPS = NOQUANTUM_OPS[:5]            # (held to tests/ft_oracle.py: sizes with exact factors only, 2-D and 3-D)
FAMILIES = {"label": OPS, "field": FIELD_OPS, "noquantum": NOQUANTUM_OPS}
COMPONENT_FAMILY = OPS[:3]
X_EXTENTS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1030)
STRUCTURES = ("blocky", "noise", "pinholes", "per_voxel", "chain")
CAP = {op: 60000 for op in OPS}
CAP["feature_transform"] = CAP["expand_labels"] = 16000     # (their oracle is the slow one)
CAP.update({op: 60000 for op in ("erode", "opening", "local_thickness")})       # (the compiled CPU transform)
CAP.update({op: 16000 for op in ("dilate", "closing", "medial_axis")})          # (tests/ft_oracle.py: pure Python)
RADIUS_MULTIPLES = (0.0, 1.0, 1.5, 2.0, 3.0)                # times the smallest voxel size
TAKES_FLAGS = ("erode", "opening", "local_thickness", "medial_axis")            # black_border and binary


def _tables():
    from test_gpu_feature_transform import DTYPES, QUANTUM
    return DTYPES, QUANTUM


def _shape(rng, op, nd, at_least, turn):
    """x-fastest extents: x first -- entry `turn` of X_EXTENTS, or (turn < 0) uniform in 1..90.  The extents behind x are
    clipped so that the case stays within its cap (never skipped); at_least > 0: grown -- the other extents first, up to 40,
    then x -- until the volume exceeds that many voxels."""
    cap = CAP[op]
    ext = [X_EXTENTS[turn % len(X_EXTENTS)] if turn >= 0 else int(rng.integers(1, 91))]
    ext += [int(rng.integers(1, 41)) for _ in range(nd - 1)]
    while at_least and int(np.prod(ext)) <= at_least:
        grow = [k for k in range(1, nd) if ext[k] < 40]
        if grow:
            ext[grow[0]] = min(40, ext[grow[0]] * 2 + 1)
        else:
            ext[0] = ext[0] * 2 + 1
    ext[0] = min(ext[0], cap)
    for k in range(1, nd):
        ext[k] = max(1, min(ext[k], cap // int(np.prod(ext[:k]))))
    return tuple(ext)


def _chain(ext, rng):
    """a serpentine or a comb along x and y (tests/test_gpu_components.py), repeated in every other slice: one long component"""
    nd = len(ext)
    sx, sy = ext[0], ext[1] if nd > 1 else 1
    img = np.zeros((sx, sy), dtype=np.int64)
    if rng.random() < 0.5:
        img[:, 0::2] = 4
        for k, y in enumerate(range(1, sy, 2)):
            img[sx - 1 if k % 2 == 0 else 0, y] = 4
    else:
        img[0::2, :] = 2
        img[:, sy - 1] = 2
    if nd == 1:
        return img[:, 0]
    if nd == 2:
        return img
    vol = np.zeros(ext, dtype=np.int64)
    vol[:, :, 0::2] = img[:, :, None]
    return vol


def _ids(rng, ext, structure):
    """small non-negative integers of shape `ext` (x first); 0 is background"""
    if structure == "blocky":
        return blocky_labels(ext, nlabels=int(rng.integers(1, 6)), zero_frac=float(rng.random() * 0.4), block=int(rng.integers(1, 7)),
                             rng=rng)
    if structure == "noise":      # near the percolation thresholds: few large, winding components
        return (rng.random(ext) < rng.choice([0.3, 0.5, 0.7])) * int(rng.choice([1, 2]))
    if structure == "pinholes":
        ids = np.full(ext, int(rng.integers(1, 4)), dtype=np.int64)
        ids[rng.random(ext) < 0.05] = 0
        return ids
    if structure == "per_voxel":
        return rng.integers(0, 3, size=ext)
    return _chain(ext, rng)


def _typed(ids, dtype, full_width):
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return ids != 0
    if not full_width:
        return ids.astype(dt)
    pal = palette(dt)                                   # extreme keys, NaN payloads, -0.0 (which is background)
    table = np.concatenate([np.zeros(1, dtype=pal.dtype), pal])
    stride = next(s for s in (3, 5, 7) if len(pal) % s)       # (the few small ids spread over the whole palette)
    return table[np.where(ids == 0, 0, 1 + (ids - 1) * stride % len(pal))]


def cases(seed, n, ops=OPS):
    """The `n` cases of `seed` over the family `ops`, as dicts: op, data (numpy, C or F order; axis 0 is x in F order, the last
    axis in C order), connectivity, binary, k (element offset of the device buffers), host (also through the host module), and
    the operation's own parameters: per-axis ones x first (w_xyz, a_xyz)."""
    DTYPES, QUANTUM = _tables()
    noquantum = tuple(ops) == NOQUANTUM_OPS
    rng = np.random.default_rng(seed)
    for i in range(n):
        op = ops[i % len(ops)]
        j = i // len(ops)                               # the operation's own case number
        # Stratified, so that a few short slices cover what a long run would: the dimensions and the connectivity go round with
        # the operation's case number, every second case takes the next entry of X_EXTENTS (consecutive seeds continue where
        # the last one stopped), and among the others every second one of the component family is grown past 2048 or 4096
        # voxels, so that chunk and span boundaries fall inside the volume.
        nd = 1 + (j + seed) % 3
        if noquantum and op in NOQUANTUM_EXACT_OPS:
            nd = 2 + (j + seed) % 2
        connectivity = 1 + (j // 3 + seed) % nd
        turn = (j // 2 + 5 * seed + 3 * ops.index(op)) if j % 2 == 0 else -1
        at_least = 0
        if op in COMPONENT_FAMILY and j % 4 == 1:
            at_least = 4096 if j % 8 == 1 else 2048
        ext = _shape(rng, op, nd, at_least, turn)
        order = "F" if rng.random() < 0.5 or ext[0] == 1 else "C"        # (a C-ordered array whose last extent is 1 is F-ordered too)
        structure = STRUCTURES[(j + i % len(ops)) % len(STRUCTURES)]
        dtype = DTYPES[i % len(DTYPES)]
        xyz = _typed(np.asarray(_ids(rng, ext, structure)), dtype, full_width=i % 5 == 4)     # indexed [x, y, z]
        data = np.asfortranarray(xyz) if order == "F" else np.ascontiguousarray(xyz.T)
        # (an array that is contiguous both ways -- 1-D, extents of 1 -- is taken in F order by every entry point and oracle)
        order = "F" if data.flags.f_contiguous else "C"
        case = dict(index=i, op=op, data=data, order=order, structure=structure, connectivity=connectivity,
                    binary=bool(rng.integers(0, 2)), k=int(rng.integers(0, 4)), host=i % 5 == 2)
        if noquantum:
            _noquantum_parameters(case, rng, j, nd, 4 * (seed % 3) + ops.index(op))
        elif op == "dust":
            lo = int(rng.integers(1, 12))
            case["threshold"] = lo if rng.random() < 0.5 else (lo, lo + int(rng.integers(1, 40)))
            case["invert"] = bool(rng.integers(0, 2))
        elif op == "label_stats":
            field = rng.standard_normal(data.shape).astype(np.float32) * np.float32(3)
            ties = rng.random(data.shape) < 0.1
            field[ties] = np.round(field[ties] * 4) / 4                 # (two fractional bits: ties)
            case["dt"] = np.asfortranarray(field) if order == "F" else field
        elif op == "feature_transform":
            w = list(QUANTUM)[int(rng.integers(0, len(QUANTUM)))]
            case["w_xyz"], case["a_xyz"] = w[:nd], QUANTUM[w][:nd]
            case["black_border"] = bool(rng.integers(0, 2))
        elif op == "expand_labels":
            case["distance"] = float(rng.choice([0.0, 1.0, 2.5, np.inf]))
            case["w_xyz"] = tuple(float(v) for v in rng.integers(1, 4, size=nd))
        elif op in FIELD_OPS:
            w = list(QUANTUM)[int(rng.integers(0, len(QUANTUM)))]
            case["w_xyz"], case["a_xyz"] = w[:nd], QUANTUM[w][:nd]
            _field_parameters(case, rng, j)
        yield case


def _noquantum_parameters(case, rng, j, nd, turn):
    """what a noquantum case draws on top of the common part: sizes without a quantum, going round their tables with the
    operation's case number -- two consecutive cases, one of each dimension or kind, share an entry, and three consecutive seeds
    start 4 entries apart, so that they cover the seven entries in every dimension (a_xyz: the sizes' exact factors, None for
    sizes whose squares are not exact in fp32)"""
    import ft_oracle
    from noquantum_cases import EXACT, INEXACT
    op = case["op"]
    if op in NOQUANTUM_EXACT_OPS:
        w = list(EXACT)[(j // 2 + turn) % len(EXACT)]
    else:
        w = list(EXACT)[(j // 2 + turn) % len(EXACT)] if j % 2 == 0 else INEXACT[(j // 2 + case["index"]) % len(INEXACT)]
    case["w_xyz"] = w[:nd]
    case["a_xyz"] = ft_oracle.exact_factors(w[:nd]) if w in EXACT else None
    if op == "feature_transform":
        case["black_border"] = bool(rng.integers(0, 2))
    elif op == "expand_labels":
        case["multiple"] = float((0.0, 1.0, 2.5, np.inf)[int(rng.integers(0, 4))])
        case["distance"] = case["multiple"] * min(case["w_xyz"]) if case["multiple"] else 0.0
    else:
        _field_parameters(case, rng, j, mild_ladder=True)


def _field_parameters(case, rng, j, mild_ladder=False):
    """what a field case draws on top of the common part and its voxel sizes; mild_ladder: local_thickness takes the default
    ladder only where the largest size is at most 4 times the smallest (its steps are the smallest size: at (1, 2^-8, 1) a
    ladder would have as many rungs as 256 times the extent)"""
    op = case["op"]
    step = min(case["w_xyz"])
    if op in TAKES_FLAGS:
        case["black_border"] = bool(rng.integers(0, 2))
    else:
        case["binary"] = False                          # (dilate and closing take neither)
    if op in ("erode", "opening", "dilate", "closing"):
        multiples = RADIUS_MULTIPLES + ((np.inf,) if op == "dilate" else ())
        case["multiple"] = float(multiples[int(rng.integers(0, len(multiples)))])
        case["radius"] = case["multiple"] * step
    elif op == "local_thickness":
        case["multiples"] = None
        if j % 3 or (mild_ladder and max(case["w_xyz"]) > 4 * step):
            picked = rng.permutation(len(RADIUS_MULTIPLES) - 1)[:int(rng.integers(1, 5))]
            case["multiples"] = tuple(RADIUS_MULTIPLES[1 + int(t)] for t in sorted(picked))
        case["radii"] = None if case["multiples"] is None else tuple(m * step for m in case["multiples"])
    else:
        case["gamma"] = (None, 0.0, 1.5 * step)[int(rng.integers(0, 3))]
        case["min_angle"] = (0.0, 60.0, 120.0)[int(rng.integers(0, 3))]
        case["return_distance"] = j % 2 == 0


def describe(case):
    d = case["data"]
    shown = ("threshold", "invert", "w_xyz", "black_border", "distance", "radius", "radii", "gamma", "min_angle", "return_distance")
    extra = {k: v for k, v in case.items() if k in shown}
    return (f"#{case['index']} {case['op']} {d.shape} {case['order']} {d.dtype.name} {case['structure']} c={case['connectivity']} "
            f"binary={case['binary']} k={case['k']} host={case['host']} {extra}")


# ---- expectations -----------------------------------------------------------------------------------------------------------
def axis_order(case, xyz):
    """a per-axis tuple given in ABI order (x first) in the order of the array's axes"""
    return tuple(xyz) if case["order"] == "F" else tuple(xyz)[::-1]


def expand_want(data, distance, a_xyz, w_xyz=None):
    """expand_reference of tests/test_gpu_feature_transform.py (the definition of include/edt_hip.h) with the inner feature
    transform from the numpy oracle, not from the library; a_xyz: the squared voxel sizes in quanta (integers), x first, which
    are the squared sizes themselves unless w_xyz gives the sizes: then D is formed from their fp64 squares, as the header does"""
    from test_gpu_feature_transform import expected
    nd = data.ndim
    order = "F" if data.flags.f_contiguous else "C"
    with np.errstate(invalid="ignore"):
        mask = np.array(data == 0, order=order).astype(np.uint8, order=order)
    f = expected(mask, False, a_xyz)                                    # component k: the coordinate along array axis k
    grids = np.stack(np.meshgrid(*[np.arange(s) for s in data.shape], indexing="ij")) if nd > 1 else np.arange(data.shape[0])[None]
    w2_xyz = a_xyz if w_xyz is None else [np.float64(np.float32(w)) * np.float64(np.float32(w)) for w in w_xyz]
    a_axis = tuple(w2_xyz) if order == "F" else tuple(w2_xyz)[::-1]
    D = np.zeros(data.shape)
    for k in (range(nd) if order == "F" else range(nd - 1, -1, -1)):    # terms added in ABI order x, y, z
        D = D + np.float64(a_axis[k]) * ((grids[k] - f[k]).astype(np.int64) ** 2).astype(np.float64)
    has = ~np.all(f == -1, axis=0)
    out = data.copy(order=order)
    with np.errstate(invalid="ignore"):
        take = np.asarray(data == 0) & has & (D <= np.float64(distance) * np.float64(distance))
    src = tuple(np.where(take, f[k], 0) for k in range(nd))
    out[take] = data[src][take]
    return out


def field_kwargs(case, anisotropy):
    """the keyword arguments of a field case for edt.<op>, edt.device.<op> and the oracles alike"""
    op = case["op"]
    kw = dict(anisotropy=tuple(anisotropy))
    if op in TAKES_FLAGS:
        kw.update(black_border=case["black_border"], binary=case["binary"])
    if op == "medial_axis":
        kw.update(gamma=case["gamma"], min_angle=case["min_angle"])
    return kw


def field_want(case):
    """erode / opening / dilate / closing: the array; local_thickness: (T, radii, sizes); medial_axis: (axis,) or (axis, radius)"""
    import medial_oracle
    import morph_oracle
    import thickness_oracle
    op, data = case["op"], case["data"]
    kw = field_kwargs(case, axis_order(case, case["w_xyz"]))
    if op in ("erode", "opening", "dilate", "closing"):
        return getattr(morph_oracle, op)(data, case["radius"], **kw)
    if op == "local_thickness":
        return thickness_oracle.local_thickness(data, case["radii"], **kw)
    on = medial_oracle.on_axis(data, **kw)
    axis = data.copy(order="K")
    axis[~on] = np.zeros((), dtype=data.dtype)
    if not case["return_distance"]:
        return (axis,)
    # the radius function: the CPU transform of what the axis is the axis of, on the axis, and +0.0 off it
    measured = morph_oracle.foreground(data) if (case["binary"] or data.dtype == np.bool_) else data
    field = np.sqrt(morph_oracle.edtsq(measured, kw["anisotropy"], case["black_border"]))
    return axis, np.where(on, field, np.float32(0.0))


def want_of(case):
    if case["op"] in FIELD_OPS:
        return field_want(case)
    import components_oracle
    import dust_oracle
    import fill_holes_oracle
    import label_stats_oracle
    from test_gpu_feature_transform import expected
    op, data, c, binary = case["op"], case["data"], case["connectivity"], case["binary"]
    if op == "connected_components":
        return components_oracle.connected_components(data, c, binary=binary, return_N=True)
    if op == "fill_holes":
        w = fill_holes_oracle.fill_holes(data, c, binary=binary)
        return w.out, w.n_filled
    if op == "dust":
        w = dust_oracle.dust(data, case["threshold"], c, binary=binary, invert=case["invert"])
        return w.out, (w.components, w.kept, w.removed_voxels)
    if op == "label_stats":
        return label_stats_oracle.label_stats(data, case["dt"])
    if op == "feature_transform":
        return expected(data, case["black_border"], case["a_xyz"])
    if "a_xyz" in case:
        return expand_want(data, case["distance"], case["a_xyz"], case["w_xyz"])
    return expand_want(data, case["distance"], tuple(int(v * v) for v in case["w_xyz"]))


# ---- the library ------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(
        np.ascontiguousarray(a).view(f"u{a.dtype.itemsize}"), np.ascontiguousarray(b).view(f"u{b.dtype.itemsize}"))


def _back(case, t):
    """a device result of the tensor's shape as a numpy array of the data's shape and dtype"""
    from synth import bits_of
    a = bits_of(t).view(case["data"].dtype if t.element_size() == case["data"].dtype.itemsize else f"u{t.element_size()}")
    return a.T if case["order"] == "F" else a


def _field_results(case, fn, x, kw, as_labels, as_floats):
    """a field case through `fn` (edt.<op> or edt.device.<op>) on `x`, in the form of field_want"""
    op = case["op"]
    if op in ("erode", "opening", "dilate", "closing"):
        return as_labels(fn(x, case["radius"], **kw))
    if op == "local_thickness":
        T, sizes = fn(x, case["radii"], return_sizes=True, **kw)
        return as_floats(T), np.asarray(sizes.radii), as_floats(sizes.voxels)
    if case["return_distance"]:
        axis, radius = fn(x, return_distance=True, **kw)
        return as_labels(axis), as_floats(radius)
    return (as_labels(fn(x, **kw)),)


def run_device(case):
    """the case through edt.device.* on buffers at element offset k; what want_of returns, plus whether the input buffers came
    back unchanged"""
    import torch
    import label_stats_oracle
    from edt import device
    from synth import offset_view
    op, data, c, binary, k = case["op"], case["data"], case["connectivity"], case["binary"], case["k"]
    tdata = data.T if case["order"] == "F" else data                     # C-contiguous: the same memory
    buf, t = offset_view(tdata, k)
    held = [(buf, buf.clone())]
    nd = data.ndim
    if op in FIELD_OPS:
        got = _field_results(case, getattr(device, op), t, field_kwargs(case, tuple(case["w_xyz"])[::-1]),
                             lambda x: _back(case, x), lambda x: x.cpu().numpy().T if case["order"] == "F" else x.cpu().numpy())
    elif op == "connected_components":
        out, n = device.connected_components(t, connectivity=c, binary=binary)
        got = (_back(case, out).view(np.uint32), int(n))
    elif op == "fill_holes":
        out, n = device.fill_holes(t, connectivity=c, binary=binary)
        got = (_back(case, out), int(n))
    elif op == "dust":
        out, counts = device.dust(t, case["threshold"], connectivity=c, binary=binary, invert=case["invert"])
        got = (_back(case, out), tuple(counts.tolist()))
    elif op == "label_stats":
        field = case["dt"].T if case["order"] == "F" else case["dt"]
        fbuf, ft = offset_view(field, k, 0x7FC0BEEF)
        held.append((fbuf, fbuf.clone()))
        s = [x.cpu().numpy() for x in device.label_stats(t, ft)]
        keys = s[0].view(data.dtype) if s[0].dtype.itemsize == data.dtype.itemsize else s[0]
        rows = np.argsort(keys, kind="stable") if data.dtype.kind == "u" else np.arange(len(keys))   # (unsigned labels travel as signed tensors)
        flip = (lambda a: a[:, ::-1]) if case["order"] == "F" else (lambda a: a)
        got = label_stats_oracle.LabelStats(keys[rows], s[1][rows], s[2][rows], np.ascontiguousarray(flip(s[3][rows])),
                                            np.ascontiguousarray(flip(s[4][rows])), np.ascontiguousarray(flip(s[5][rows])))
    elif op == "feature_transform":
        f = device.feature_transform(t, anisotropy=tuple(case["w_xyz"])[::-1], black_border=case["black_border"]).cpu().numpy()
        got = np.stack([f[nd - 1 - j].T for j in range(nd)]) if case["order"] == "F" else f
    else:
        out = device.expand_labels(t, distance=case["distance"], anisotropy=tuple(case["w_xyz"])[::-1])
        got = _back(case, out)
    torch.cuda.synchronize()
    return got, all(torch.equal(b, before) for b, before in held)


def run_host(case):
    """the case through the host module edt.*"""
    import edt
    import label_stats_oracle
    op, data, c, binary = case["op"], case["data"], case["connectivity"], case["binary"]
    if op in FIELD_OPS:
        return _field_results(case, getattr(edt, op), data, field_kwargs(case, axis_order(case, case["w_xyz"])), np.asarray, np.asarray)
    if op == "connected_components":
        return edt.connected_components(data, connectivity=c, binary=binary, return_N=True)
    if op == "fill_holes":
        return edt.fill_holes(data, connectivity=c, binary=binary, return_fill_count=True)
    if op == "dust":
        out, counts = edt.dust(data, case["threshold"], connectivity=c, binary=binary, invert=case["invert"], return_counts=True)
        return out, tuple(counts)
    if op == "label_stats":
        return label_stats_oracle.LabelStats(*edt.label_stats(data, case["dt"]))
    if op == "feature_transform":
        return edt.feature_transform(data, anisotropy=axis_order(case, case["w_xyz"]), black_border=case["black_border"])
    return edt.expand_labels(data, distance=case["distance"], anisotropy=axis_order(case, case["w_xyz"]))


def agrees(case, got, want):
    """'' if `got` equals `want` bit for bit, else what differs"""
    import label_stats_oracle
    op = case["op"]
    if op in FIELD_OPS:
        got, want = (got if isinstance(got, tuple) else (got,)), (want if isinstance(want, tuple) else (want,))
        names = {"local_thickness": ("the thickness", "the radii", "the sizes"), "medial_axis": ("the axis", "the radius")}
        names = names.get(op, ("the volume",))
        if len(got) != len(want):
            return f"{len(got)} results, not {len(want)}"
        for name, g, w in zip(names, got, want):
            g, w = np.asarray(g), np.asarray(w)
            if g.dtype != w.dtype or not same_bits(g, w):
                differ = int(np.count_nonzero(g != w)) if g.shape == w.shape else -1
                return f"{name} differs ({g.dtype.name}{g.shape} against {w.dtype.name}{w.shape}, {differ} elements)"
        return ""
    if op == "label_stats":
        try:
            label_stats_oracle.assert_same(got, want)
        except AssertionError as e:
            return f"table differs: {str(e)[:200]}"
        return ""
    if op in ("feature_transform", "expand_labels"):
        return "" if same_bits(got, want) else f"{int(np.count_nonzero(np.asarray(got) != np.asarray(want)))} elements differ"
    if not same_bits(got[0], want[0]):
        return "the volume differs"
    if tuple(np.atleast_1d(got[1]).tolist()) != tuple(np.atleast_1d(want[1]).tolist()):
        return f"counts {got[1]} != {want[1]}"
    return ""


def main(argv):
    ncases = int(argv[1]) if len(argv) > 1 else 60
    seed = int(argv[2]) if len(argv) > 2 else 1
    family = argv[3] if len(argv) > 3 else "label"
    if family not in FAMILIES:
        print(f"usage: {argv[0]} [ncases] [seed] [{'|'.join(FAMILIES)}]", file=sys.stderr)
        return 2
    ops = FAMILIES[family]
    bad, t0 = 0, time.time()
    ran = dict.fromkeys(ops, 0)
    for case in cases(seed, ncases, ops):
        want = want_of(case)
        got, inputs_intact = run_device(case)
        why = agrees(case, got, want)
        if not why and not inputs_intact:
            why = "the input buffers changed"
        if not why and case["host"]:
            why = agrees(case, run_host(case), want)
            why = why and "host module: " + why
        ran[case["op"]] += 1
        if why:
            bad += 1
            print("MISMATCH", describe(case), "--", why, flush=True)
    print("ops:", " ".join(f"{op}={ran[op]}" for op in ops))
    print(f"{ncases} cases, {bad} mismatches, {time.time() - t0:.1f} s")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
