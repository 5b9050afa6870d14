"""CPU tier of the randomised runs of the label operations (tools/fuzz_ops.py): the same cases the GPU tier draws
(tests/test_gpu_fuzz_ops.py: the same seeds), with the numpy oracles held against a second opinion -- scipy.ndimage and brute
force -- so that the GPU tier does not rest on one restatement; and the generator held to what it promises to cover.

Two families: the label operations (seeds 701..703; their draws are pinned by a digest, so that work on the generator cannot
move them unnoticed) and the field operations erode / opening / dilate / closing / local_thickness / medial_axis (seeds
711..713), whose second opinions are brute forces written from the definitions in exact integer arithmetic on the quanta of the
voxel sizes, independent of both the compiled CPU transform and tests/ft_oracle.py.  The field draws are pinned by a digest too.

A third family (seeds 721..723, 64 cases each) draws voxel sizes the library finds no quantum for (tests/noquantum_cases.py): the
same brute forces serve it on the sizes' exact factors (ft_oracle.exact_factors), a radius of m smallest sizes being
4 m^2 min(a) quanta."""
import hashlib
import itertools
import math
import os
import sys

import numpy as np
import pytest

import components_oracle
import dust_oracle
import fill_holes_oracle
import ft_oracle
import label_stats_oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_ops  # noqa: E402
from test_q16_logic import q16, quantum  # noqa: E402, F401  (the fixture builds the host shim of the library's quantum rule)

SEEDS = (701, 702, 703)        # (tests/test_gpu_fuzz_ops.py runs the same)
NCASES = 60
_drawn = {}


def drawn(seed):
    if seed not in _drawn:
        _drawn[seed] = list(fuzz_ops.cases(seed, NCASES))
    return _drawn[seed]


def scipy_components(ndi, data, c, binary):
    """the number of components from scipy.ndimage.label, label value by label value unless binary; NaN voxels, which equal
    nothing, are one component each"""
    structure = ndi.generate_binary_structure(data.ndim, c)
    with np.errstate(invalid="ignore"):
        fg = data != 0
    if binary or data.dtype == np.bool_:
        return ndi.label(fg, structure=structure)[1]
    nan = data != data
    values = np.unique(data[fg & ~nan])
    return sum(ndi.label(data == v, structure=structure)[1] for v in values) + int(np.count_nonzero(nan))


_checked = {}


def second_opinions(seed):
    """holds the oracles of every case of `seed` against scipy / brute force where one applies; how many cases of each
    operation were compared"""
    if seed not in _checked:
        _checked[seed] = _second_opinions(seed)
    return _checked[seed]


def _second_opinions(seed):
    from scipy import ndimage as ndi
    from test_dust_cpu import scipy_dust
    checked = dict.fromkeys(fuzz_ops.OPS, 0)
    for case in drawn(seed):
        op, data, c, binary = case["op"], case["data"], case["connectivity"], case["binary"]
        what = fuzz_ops.describe(case)
        floats_special = data.dtype.kind == "f" and not np.all(np.isfinite(data) & ((data != 0) | ~np.signbit(data)))
        if op == "connected_components":
            out, n = components_oracle.connected_components(data, c, binary=binary, return_N=True)
            assert n == scipy_components(ndi, data, c, binary), what
            assert n == (int(out.max()) if out.size else 0) and np.array_equal(out != 0, data != 0), what
            checked[op] += 1
        elif op == "dust" and not floats_special:
            lo, hi = dust_oracle.bounds(case["threshold"])
            w = dust_oracle.dust(data, case["threshold"], c, binary=binary, invert=case["invert"])
            out, found, kept, removed = scipy_dust(ndi, data, lo, hi, c, binary or data.dtype == np.bool_, case["invert"])
            assert np.array_equal(w.out, out) and (w.components, w.kept, w.removed_voxels) == (found, kept, removed), what
            checked[op] += 1
        elif op == "fill_holes" and (binary or data.dtype == np.bool_):
            w = fill_holes_oracle.fill_holes(data, c, binary=True)
            with np.errstate(invalid="ignore"):
                fg = data != 0
            filled = ndi.binary_fill_holes(fg, structure=ndi.generate_binary_structure(data.ndim, c))
            assert np.array_equal(w.out != 0, filled) and w.n_filled == int(np.count_nonzero(filled & ~fg)), what
            checked[op] += 1
        elif op == "label_stats":
            label_stats_oracle.assert_same(label_stats_oracle.label_stats(data, case["dt"]),
                                           label_stats_oracle.brute_force(data, case["dt"]), what)
            checked[op] += 1
        elif op == "feature_transform" and data.size <= 2000:
            nd, a, bb = data.ndim, case["a_xyz"], case["black_border"]
            lab = data.reshape(data.shape + (1,) * (3 - nd)) if case["order"] == "F" else ft_oracle.x_first(data)
            feats, _ = ft_oracle.feature_transform(lab, tuple(a) + (1,) * (3 - nd), bb, ndim=nd)
            d = ft_oracle.sqdist(feats, tuple(a) + (0,) * (3 - nd))
            best = ft_oracle.brute_min(lab, tuple(a) + (1,) * (3 - nd), bb) if nd == 3 else None
            if nd < 3:          # (the brute force pads every axis with the border shell: give the unused axes no neighbours)
                best = _brute_min_nd(lab, a, bb, nd)
            has = d >= 0
            assert np.array_equal(np.where(has, d, ft_oracle.INF), best), what
            checked[op] += 1
    return checked


@pytest.mark.parametrize("seed", SEEDS)
def test_oracles_against_a_second_opinion(seed):
    checked = second_opinions(seed)
    assert checked["connected_components"] == NCASES // 6 and checked["label_stats"] == NCASES // 6, checked


def _brute_min_nd(lab, a, bb, nd):
    """ft_oracle.brute_min on the first nd axes of an [x, y, z] volume whose other extents are 1"""
    sub = lab.reshape(lab.shape[:nd])
    pad = np.zeros(tuple(s + 2 for s in sub.shape), dtype=sub.dtype) if bb else sub
    if bb:
        pad[tuple(slice(1, -1) for _ in range(nd))] = sub
    off = 1 if bb else 0
    coords = np.stack(np.meshgrid(*[np.arange(s) - off for s in pad.shape], indexing="ij"), -1).reshape(-1, nd)
    flat = pad.reshape(-1)
    out = np.zeros(sub.shape, dtype=np.int64)
    for idx in np.ndindex(sub.shape):
        L = sub[idx]
        if L == 0:
            continue
        p = np.array(idx)
        other = ~(flat == L) & ~np.all(coords == p, axis=1)
        out[idx] = ((coords[other] - p) ** 2 * np.array(a[:nd])).sum(1).min() if other.any() else ft_oracle.INF
    return out.reshape(lab.shape)


def test_second_opinions_reach_every_operation_they_can():
    """over the three seeds dust, binary fill_holes and small feature transforms are each compared at least a few times"""
    total = dict.fromkeys(fuzz_ops.OPS, 0)
    for seed in SEEDS:
        for op, n in second_opinions(seed).items():
            total[op] += n
    assert total["dust"] >= 15 and total["fill_holes"] >= 8 and total["feature_transform"] >= 5, total


def test_generator_covers_what_it_promises():
    every = [c for seed in SEEDS for c in drawn(seed)]
    assert len(every) == 3 * NCASES
    for op in fuzz_ops.OPS:
        mine = [c for c in every if c["op"] == op]
        assert len(mine) == 3 * NCASES // 6, op
        assert {c["data"].ndim for c in mine} == {1, 2, 3}, op
        assert {c["order"] for c in mine} == {"C", "F"}, op
        assert {(c["data"].ndim, c["connectivity"]) for c in mine} >= {(1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (3, 3)}, op
        sx = [c["data"].shape[0] if c["order"] == "F" else c["data"].shape[-1] for c in mine]
        assert 1 in sx and 64 in sx and 65 in sx and max(sx) >= 257, (op, sorted(sx))
        assert all(c["data"].size <= fuzz_ops.CAP[op] for c in mine), op
        assert {c["k"] for c in mine} == {0, 1, 2, 3}, op
        assert any(c["host"] for c in mine), op
    for op in fuzz_ops.COMPONENT_FAMILY:
        sizes = [c["data"].size for c in every if c["op"] == op]
        assert sum(s > 2048 for s in sizes) * 4 >= len(sizes) and sum(s > 4096 for s in sizes) >= 3, (op, sorted(sizes))
    assert {c["structure"] for c in every} == set(fuzz_ops.STRUCTURES)
    assert len({c["data"].dtype for c in every}) == 11
    assert any(c["data"].dtype.kind == "f" and np.isnan(c["data"]).any() for c in every)
    # the same seed draws the same cases
    again = list(fuzz_ops.cases(SEEDS[0], NCASES))
    assert all(np.array_equal(a["data"], b["data"], equal_nan=a["data"].dtype.kind == "f") for a, b in zip(again, drawn(SEEDS[0])))


LABEL_DRAWS_SHA256 = "7c758e19b9538028084379d20e25eb2ed4c9918025ae03787c15a5f9145bf94e"


def test_the_label_family_draws_have_not_moved():
    """sha256 over describe(case) and the data bytes (memory order) of the 60 cases of seeds 701, 702 and 703, taken before the
    generator learnt the field family: what the GPU tier has run so far is what it still runs"""
    h = hashlib.sha256()
    for seed in SEEDS:
        for case in drawn(seed):
            h.update(fuzz_ops.describe(case).encode())
            h.update(case["data"].tobytes(order="A"))
    assert h.hexdigest() == LABEL_DRAWS_SHA256


# ---- the field family ---------------------------------------------------------------------------------------------------------
FIELD_SEEDS = (711, 712, 713)   # (tests/test_gpu_fuzz_ops.py runs the same)
FIELD_DRAWS_SHA256 = "46cac9a764190585d63cf3cd7d4bb48bcdb6d72294e90d6f729d02b7b2876ac9"
_drawn_field = {}


def drawn_field(seed):
    if seed not in _drawn_field:
        _drawn_field[seed] = list(fuzz_ops.cases(seed, NCASES, fuzz_ops.FIELD_OPS))
    return _drawn_field[seed]


def test_field_generator_covers_what_it_promises():
    from test_gpu_feature_transform import QUANTUM
    every = [c for seed in FIELD_SEEDS for c in drawn_field(seed)]
    assert len(every) == 3 * NCASES
    for op in fuzz_ops.FIELD_OPS:
        mine = [c for c in every if c["op"] == op]
        assert len(mine) == 3 * NCASES // 6, op
        assert {c["data"].ndim for c in mine} == {1, 2, 3}, op
        assert {c["order"] for c in mine} == {"C", "F"}, op
        sx = [c["data"].shape[0] if c["order"] == "F" else c["data"].shape[-1] for c in mine]
        assert 1 in sx and 64 in sx and 65 in sx and max(sx) >= 257, (op, sorted(sx))
        assert all(c["data"].size <= fuzz_ops.CAP[op] for c in mine), op
        assert {c["k"] for c in mine} == {0, 1, 2, 3}, op
        assert any(c["host"] for c in mine), op
        assert all(len(c["w_xyz"]) == len(c["a_xyz"]) == c["data"].ndim for c in mine), op
        if op in fuzz_ops.TAKES_FLAGS:
            assert {c["black_border"] for c in mine} == {False, True} and {c["binary"] for c in mine} == {False, True}, op
        else:
            assert not any("black_border" in c or c["binary"] for c in mine), op
    assert {c["structure"] for c in every} == set(fuzz_ops.STRUCTURES)
    assert len({c["data"].dtype for c in every}) == 11
    assert any(c["data"].dtype.kind == "f" and np.isnan(c["data"]).any() for c in every)
    assert {c["w_xyz"] for c in every if c["data"].ndim == 3} == set(QUANTUM) and len(QUANTUM) == 4 and (0.5, 0.5, 1.0) in QUANTUM
    assert all(tuple(ac * min(c["w_xyz"]) ** 2 for ac in c["a_xyz"]) == tuple(w * w for w in c["w_xyz"]) for c in every)
    for op in ("erode", "opening", "dilate", "closing"):
        mine = [c for c in every if c["op"] == op]
        assert any(c["radius"] == 0.0 for c in mine), op
        assert all(c["radius"] == c["multiple"] * min(c["w_xyz"]) for c in mine), op
        assert any(c["radius"] == np.inf for c in mine) == (op == "dilate"), op
    assert {c["multiple"] for c in every if "multiple" in c} == set(fuzz_ops.RADIUS_MULTIPLES) | {np.inf}
    ladders = [c["radii"] for c in every if c["op"] == "local_thickness"]
    assert sum(r is None for r in ladders) == 12 and {len(r) for r in ladders if r is not None} == {1, 2, 3, 4}
    assert all(r is None or all(x < y for x, y in zip(r, r[1:])) and r[0] > 0 for r in ladders)
    axes = [c for c in every if c["op"] == "medial_axis"]
    assert len({c["gamma"] is None for c in axes}) == 2 and any(c["gamma"] == 0.0 for c in axes)
    assert any(c["gamma"] == 1.5 * min(c["w_xyz"]) for c in axes)
    assert {c["min_angle"] for c in axes} == {0.0, 60.0, 120.0}
    assert sum(c["return_distance"] for c in axes) == len(axes) // 2
    again = list(fuzz_ops.cases(FIELD_SEEDS[0], NCASES, fuzz_ops.FIELD_OPS))
    assert [fuzz_ops.describe(c) for c in again] == [fuzz_ops.describe(c) for c in drawn_field(FIELD_SEEDS[0])]
    assert all(np.array_equal(a["data"], b["data"], equal_nan=a["data"].dtype.kind == "f") for a, b in zip(again, drawn_field(FIELD_SEEDS[0])))


def test_the_field_family_draws_have_not_moved():
    """the same digest over the 60 cases of seeds 711, 712 and 713, taken before the generator learnt the noquantum family"""
    h = hashlib.sha256()
    for seed in FIELD_SEEDS:
        for case in drawn_field(seed):
            h.update(fuzz_ops.describe(case).encode())
            h.update(case["data"].tobytes(order="A"))
    assert h.hexdigest() == FIELD_DRAWS_SHA256


# The brute forces.  A volume is indexed x first (`_xyz`), `a` are the squared voxel sizes in quanta q = min(w)^2 (integers),
# and a radius m * min(w) is the integer r4 = 4 m^2 (m is a multiple of 1/2; None: +inf): D(p, q) <= r^2 is
# 4 * sum_c a_c (p_c - q_c)^2 <= r4, in Python / int64 integers throughout.
BUDGET = 6 * 10**7      # voxels times offsets (erode, opening, local_thickness), or background times foreground voxels (dilate)


def _xyz(case):
    """the x-first view of the case's array, and the map of such a volume back onto the array's axes"""
    data = case["data"]
    return (data, lambda v: v) if case["order"] == "F" else (data.T, lambda v: v.T)


def _r4(multiple):
    return None if multiple == np.inf else int(round(4 * multiple * multiple))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}")


def _fg(lab):
    with np.errstate(invalid="ignore"):
        return np.asarray(lab != 0)


def ball_offsets(a, r4):
    """the integer offsets o (x first) of the ball: 4 * sum_c a_c o_c^2 <= r4"""
    reach = [math.isqrt(r4 // (4 * ac)) for ac in a]
    return [o for o in itertools.product(*[range(-k, k + 1) for k in reach]) if 4 * sum(ac * d * d for ac, d in zip(a, o)) <= r4]


def _pairs(shape, o):
    """the slices of the voxels p whose q = p + o lies inside the array, and those of the q; None where there is no such p"""
    if any(abs(d) >= s for s, d in zip(shape, o)):
        return None
    return (tuple(slice(max(0, -d), s - max(0, d)) for s, d in zip(shape, o)),
            tuple(slice(max(0, d), s - max(0, -d)) for s, d in zip(shape, o)))


def brute_erode(lab, a, r4, black_border, binary):
    """the survivors: foreground voxels with no voxel of another label (binary: no background) at D <= r^2, the voxels outside
    the array included under black_border"""
    fg = _fg(lab)
    alive = fg.copy()
    for o in ball_offsets(a, r4):
        if not any(o):
            continue
        ok = np.full(lab.shape, not black_border)                   # (what a p whose q lies outside gets)
        pair = _pairs(lab.shape, o)
        if pair:
            with np.errstate(invalid="ignore"):
                ok[pair[0]] = fg[pair[1]] if binary else (lab[pair[0]] == lab[pair[1]])
        alive &= ok
    return alive


def brute_opening(lab, a, r4, black_border, binary):
    """the union of the balls around the survivors, cut to the label"""
    fg = _fg(lab)
    alive = brute_erode(lab, a, r4, black_border, binary)
    held = alive.copy()
    for o in ball_offsets(a, r4):
        pair = _pairs(lab.shape, o)
        if any(o) and pair:
            with np.errstate(invalid="ignore"):
                mine = fg[pair[0]] if binary else (lab[pair[0]] == lab[pair[1]])
            held[pair[0]] |= alive[pair[1]] & mine
    return held


def _selected(data, passes):
    """the bits of `data` where `passes`, zero bits elsewhere"""
    return np.where(passes, _bits(data), 0).astype(_bits(data).dtype)


def brute_thickness(lab, a, r4s, step, black_border, binary, unit=1):
    """(T, radii, sizes) from brute-force openings; r4s None: the default ladder j = 1, 2, ... as long as some voxel's finite
    squared distance exceeds (j step)^2, i.e. as long as the erosion by j steps leaves a survivor in a volume whose distances
    are finite -- under a black border, or where not every voxel carries the one label.  None where the budget runs out.
    ``unit``: min(a), where the quantum is not the smallest size's square (r4 counts quarter squares of the smallest size)."""
    fg = _fg(lab)
    spent = 0
    T = np.zeros(lab.shape, dtype=np.float32)
    radii, sizes = [], []
    if r4s is None:
        with np.errstate(invalid="ignore"):
            uniform = lab.size == 1 or bool(fg.all() if binary else np.all(lab == lab.reshape(-1)[0]))
        ladder = itertools.count(1) if black_border or not uniform else iter(())
    else:
        ladder = iter(r4s)
    for t in ladder:
        r4 = 4 * t * t if r4s is None else t
        spent += 2 * len(ball_offsets(a, r4 * unit)) * lab.size
        if spent > BUDGET:
            return None
        if r4s is None and not brute_erode(lab, a, r4 * unit, black_border, binary).any():
            break
        held = brute_opening(lab, a, r4 * unit, black_border, binary) & fg
        radius = math.sqrt(r4 / 4.0) * step
        radii.append(radius)
        sizes.append(int(np.count_nonzero(held)))
        T[held] = np.float32(radius)
    return T, np.array(radii, dtype=np.float64), np.array(sizes, dtype=np.int64)


def dilate_properties(lab, out, a, r4, what):
    """every voxel `out` filled took the label of a foreground voxel at the brute-force minimum distance, and that distance is
    <= r^2; every voxel left empty has no foreground within r; the foreground is untouched"""
    fg = _fg(lab)
    ib, ob = _bits(lab).reshape(-1), _bits(out).reshape(-1)
    flat = fg.reshape(-1)
    assert np.array_equal(ob[flat], ib[flat]), what
    coords = np.stack(np.meshgrid(*[np.arange(s, dtype=np.int64) for s in lab.shape], indexing="ij"), -1).reshape(-1, lab.ndim)
    src, src_bits = coords[flat], ib[flat]
    weights = np.array(a, dtype=np.int64)
    empty = np.nonzero(~flat)[0]
    filled = _fg(out).reshape(-1)[empty]
    if not len(src):
        assert not filled.any() and np.array_equal(ob, ib), what
        return
    for lo in range(0, len(empty), 512):
        rows = empty[lo:lo + 512]
        D = (((coords[rows][:, None, :] - src[None, :, :]) ** 2) * weights).sum(-1)
        nearest = D.min(1)
        within = np.ones(len(rows), dtype=bool) if r4 is None else 4 * nearest <= r4
        assert np.array_equal(filled[lo:lo + 512], within), what
        took = ((D == nearest[:, None]) & (src_bits[None, :] == ob[rows][:, None])).any(1)
        assert took[within].all() and np.array_equal(ob[rows][~within], ib[rows][~within]), what


_checked_field = {}


def field_second_opinions(seed):
    if seed not in _checked_field:
        _checked_field[seed] = _field_second_opinions(seed)
    return _checked_field[seed]


def _field_second_opinions(seed):
    import medial_oracle
    import morph_oracle
    checked = dict.fromkeys(fuzz_ops.FIELD_OPS, 0)
    for case in drawn_field(seed):
        op, data = case["op"], case["data"]
        what = fuzz_ops.describe(case)
        lab, back = _xyz(case)
        a = case["a_xyz"]
        binary = case["binary"] or data.dtype == np.bool_
        if op in ("erode", "opening"):
            r4 = _r4(case["multiple"])
            if len(ball_offsets(a, r4)) * data.size > BUDGET:
                continue
            brute = (brute_erode if op == "erode" else brute_opening)(lab, a, r4, case["black_border"], binary)
            assert np.array_equal(_bits(fuzz_ops.want_of(case)), _selected(data, back(brute))), what
            checked[op] += 1
        elif op == "local_thickness":
            r4s = None if case["multiples"] is None else [_r4(m) for m in case["multiples"]]
            brute = brute_thickness(lab, a, r4s, min(case["w_xyz"]), case["black_border"], binary)
            if brute is None:
                continue
            T, radii, sizes = fuzz_ops.want_of(case)
            assert np.array_equal(radii, brute[1]) and np.array_equal(sizes, brute[2]), (what, radii, brute[1], sizes, brute[2])
            assert T.dtype == np.float32 and np.array_equal(_bits(T), _bits(back(brute[0]))), what
            checked[op] += 1
        elif op == "dilate":
            if int(np.count_nonzero(_fg(data))) * int(np.count_nonzero(~_fg(data))) > BUDGET:
                continue
            out = fuzz_ops.want_of(case)
            dilate_properties(lab, out if case["order"] == "F" else out.T, a, _r4(case["multiple"]), what)
            checked[op] += 1
        elif op == "closing":
            r4 = _r4(case["multiple"])
            if len(ball_offsets(a, r4)) * data.size > BUDGET:
                continue
            out = fuzz_ops.want_of(case)
            dilated = morph_oracle.dilate(data, case["radius"], fuzz_ops.axis_order(case, case["w_xyz"]))
            grown = dilated if case["order"] == "F" else dilated.T
            eroded = brute_erode(_fg(grown).astype(np.uint8), a, r4, False, True)
            keep = _fg(data) | back(eroded)
            assert np.array_equal(_fg(out), keep), what
            assert np.array_equal(_bits(out), _selected(dilated, keep)), what           # (under the dilation's labels)
            assert np.array_equal(_bits(out)[_fg(data)], _bits(data)[_fg(data)]), what  # no input voxel is lost
            checked[op] += 1
        elif data.size <= MEDIAL_SCATTER_VOXELS:
            kw = fuzz_ops.field_kwargs(case, fuzz_ops.axis_order(case, case["w_xyz"]))
            assert np.array_equal(medial_oracle.on_axis(data, form=medial_oracle.scatter, **kw),
                                  medial_oracle.on_axis(data, form=medial_oracle.gather, **kw)), what
            checked[op] += 1
    return checked


MEDIAL_SCATTER_VOXELS = 6000     # (the scatter form is a Python loop over the pairs of neighbours)


@pytest.mark.parametrize("seed", FIELD_SEEDS)
def test_field_oracles_against_a_second_opinion(seed):
    checked = field_second_opinions(seed)
    assert checked["erode"] == checked["opening"] == checked["closing"] == NCASES // 6, checked


def test_field_second_opinions_reach_every_operation():
    """over the three seeds, how many of the 30 cases of each operation the brute forces could afford to compare"""
    total = dict.fromkeys(fuzz_ops.FIELD_OPS, 0)
    for seed in FIELD_SEEDS:
        for op, n in field_second_opinions(seed).items():
            total[op] += n
    assert all(n >= 5 for n in total.values()), total
    assert total["erode"] == total["opening"] == total["closing"] == total["dilate"] == 30, total
    assert total["local_thickness"] >= 28 and total["medial_axis"] >= 23, total       # (what the budgets leave of the 30 each)


# ---- the noquantum family -----------------------------------------------------------------------------------------------------
NOQUANTUM_SEEDS = (721, 722, 723)   # (tests/test_gpu_fuzz_ops.py runs the same)
NOQUANTUM_NCASES = 64
_drawn_noquantum = {}


def drawn_noquantum(seed):
    if seed not in _drawn_noquantum:
        _drawn_noquantum[seed] = list(fuzz_ops.cases(seed, NOQUANTUM_NCASES, fuzz_ops.NOQUANTUM_OPS))
    return _drawn_noquantum[seed]


def test_noquantum_generator_covers_what_it_promises(q16):  # noqa: F811
    import noquantum_cases as nq
    ops = fuzz_ops.NOQUANTUM_OPS
    assert fuzz_ops.FAMILIES["noquantum"] == ops and len(ops) == 8
    every = [c for seed in NOQUANTUM_SEEDS for c in drawn_noquantum(seed)]
    assert len(every) == 3 * NOQUANTUM_NCASES
    for seed in NOQUANTUM_SEEDS:
        assert all(sum(c["op"] == op for c in drawn_noquantum(seed)) == 8 for op in ops)
    for op in ops:
        mine = [c for c in every if c["op"] == op]
        exact_only = op in fuzz_ops.NOQUANTUM_EXACT_OPS
        assert {c["data"].ndim for c in mine} == ({2, 3} if exact_only else {1, 2, 3}), op
        assert {c["order"] for c in mine} == {"C", "F"}, op
        assert all(c["data"].size <= fuzz_ops.CAP[op] for c in mine), op
        assert {c["k"] for c in mine} == {0, 1, 2, 3}, op
        assert any(c["host"] for c in mine), op
        assert all(len(c["w_xyz"]) == c["data"].ndim for c in mine), op
        full = {w for w in list(nq.EXACT) + list(nq.INEXACT)}
        of = {c["w_xyz"]: [w for w in full if w[:c["data"].ndim] == c["w_xyz"]] for c in mine}
        assert all(of.values()), op
        if exact_only:
            # every entry of EXACT, in 2-D and in 3-D; the library finds no quantum for any of the draws
            assert {c["w_xyz"] for c in mine if c["data"].ndim == 3} == set(nq.EXACT), op
            assert {c["w_xyz"] for c in mine if c["data"].ndim == 2} == {w[:2] for w in nq.EXACT}, op
            assert all(c["a_xyz"] == ft_oracle.exact_factors(c["w_xyz"]) for c in mine), op
            assert not any(quantum(q16, c["w_xyz"])[0] for c in mine), op
        else:
            exact = [c for c in mine if c["a_xyz"] is not None]
            assert len(exact) == len(mine) // 2 and all(c["a_xyz"] == ft_oracle.exact_factors(c["w_xyz"]) for c in exact), op
            assert {c["w_xyz"] for c in mine if c["a_xyz"] is None and c["data"].ndim == 3} == set(nq.INEXACT), op
            assert {c["black_border"] for c in mine} == {False, True} and {c["binary"] for c in mine} == {False, True}, op
    sx = {c["data"].shape[0] if c["order"] == "F" else c["data"].shape[-1] for c in every}
    assert sx >= {1, 2, 63, 64, 65, 129, 257, 1030}, sorted(sx)
    assert {c["structure"] for c in every} == set(fuzz_ops.STRUCTURES)
    assert len({c["data"].dtype for c in every}) == 11
    assert any(c["data"].dtype.kind == "f" and np.isnan(c["data"]).any() for c in every)
    grown = [c for c in every if c["op"] == "expand_labels"]
    assert {c["multiple"] for c in grown} == {0.0, 1.0, 2.5, np.inf}
    assert all(c["distance"] == (c["multiple"] * min(c["w_xyz"]) if c["multiple"] else 0.0) for c in grown)
    for op in ("erode", "opening", "dilate", "closing"):
        mine = [c for c in every if c["op"] == op]
        assert any(c["radius"] == 0.0 for c in mine) and all(c["radius"] == c["multiple"] * min(c["w_xyz"]) for c in mine), op
    ladders = [c for c in every if c["op"] == "local_thickness"]
    assert any(c["radii"] is None for c in ladders) and any(c["radii"] is not None for c in ladders)
    assert all(max(c["w_xyz"]) <= 4 * min(c["w_xyz"]) for c in ladders if c["radii"] is None)
    axes = [c for c in every if c["op"] == "medial_axis"]
    assert len({c["gamma"] is None for c in axes}) == 2 and {c["min_angle"] for c in axes} == {0.0, 60.0, 120.0}
    again = list(fuzz_ops.cases(NOQUANTUM_SEEDS[0], NOQUANTUM_NCASES, fuzz_ops.NOQUANTUM_OPS))
    assert [fuzz_ops.describe(c) for c in again] == [fuzz_ops.describe(c) for c in drawn_noquantum(NOQUANTUM_SEEDS[0])]
    assert all(np.array_equal(a["data"], b["data"], equal_nan=a["data"].dtype.kind == "f")
               for a, b in zip(again, drawn_noquantum(NOQUANTUM_SEEDS[0])))


def test_expand_want_forms_d_from_the_squared_sizes():
    """with the sizes given, D is w^2 d^2 in fp64, not a d^2 in quanta: at (1, 129) a voxel 1 row away lies at 16641, within 129"""
    lab = np.zeros((3, 3), dtype=np.uint8, order="F")
    lab[1, 0] = 7
    grown = fuzz_ops.expand_want(lab, 129.0, (1, 16641), (1.0, 129.0))
    assert grown[1, 1] == 7 and grown[0, 0] == 7 and grown[0, 1] == 0 and np.count_nonzero(grown) == 4
    assert np.count_nonzero(fuzz_ops.expand_want(lab, 1.0, (1, 16641), (1.0, 129.0))) == 3
    # (in quanta alone the same call would compare 16641 with 129^2 as well: the two agree where a is w^2 itself)
    assert np.array_equal(fuzz_ops.expand_want(lab, 129.0, (1, 16641)), grown)
    tiny = fuzz_ops.expand_want(lab, 2.0 ** -8, (65536, 1), (1.0, 2.0 ** -8))
    assert tiny[1, 1] == 7 and np.count_nonzero(tiny) == 2
    assert np.count_nonzero(fuzz_ops.expand_want(lab, 2.0 ** -8, (65536, 1))) == 1


_checked_noquantum = {}


def noquantum_second_opinions(seed):
    if seed not in _checked_noquantum:
        _checked_noquantum[seed] = _noquantum_second_opinions(seed)
    return _checked_noquantum[seed]


def _ft_attains_the_brute_minimum(case, what):
    data, nd, a, bb = case["data"], case["data"].ndim, case["a_xyz"], case["black_border"]
    lab = data.reshape(data.shape + (1,) * (3 - nd)) if case["order"] == "F" else ft_oracle.x_first(data)
    feats, _ = ft_oracle.feature_transform(lab, tuple(a) + (1,) * (3 - nd), bb, ndim=nd)
    d = ft_oracle.sqdist(feats, tuple(a) + (0,) * (3 - nd))
    best = ft_oracle.brute_min(lab, tuple(a), bb) if nd == 3 else _brute_min_nd(lab, a, bb, nd)
    assert np.array_equal(np.where(d >= 0, d, ft_oracle.INF), best), what


def _noquantum_second_opinions(seed):
    import medial_oracle
    import morph_oracle
    checked = dict.fromkeys(fuzz_ops.NOQUANTUM_OPS, 0)
    for case in drawn_noquantum(seed):
        op, data, a = case["op"], case["data"], case["a_xyz"]
        what = fuzz_ops.describe(case)
        if a is None:                   # (sizes without exact factors: the compiled CPU transform stands alone)
            continue
        lab, back = _xyz(case)
        unit = min(a)
        binary = case["binary"] or data.dtype == np.bool_
        r4 = None
        if "multiple" in case and case["multiple"] != np.inf:
            r4 = _r4(case["multiple"]) * unit
        if op == "feature_transform":
            if data.size <= 2000:
                _ft_attains_the_brute_minimum(case, what)
                checked[op] += 1
        elif op in ("erode", "opening"):
            if len(ball_offsets(a, r4)) * data.size > BUDGET:
                continue
            brute = (brute_erode if op == "erode" else brute_opening)(lab, a, r4, case["black_border"], binary)
            assert np.array_equal(_bits(fuzz_ops.want_of(case)), _selected(data, back(brute))), what
            checked[op] += 1
        elif op == "local_thickness":
            r4s = None if case["multiples"] is None else [_r4(m) for m in case["multiples"]]
            brute = brute_thickness(lab, a, r4s, min(case["w_xyz"]), case["black_border"], binary, unit=unit)
            if brute is None:
                continue
            T, radii, sizes = fuzz_ops.want_of(case)
            assert np.array_equal(radii, brute[1]) and np.array_equal(sizes, brute[2]), (what, radii, brute[1], sizes, brute[2])
            assert T.dtype == np.float32 and np.array_equal(_bits(T), _bits(back(brute[0]))), what
            checked[op] += 1
        elif op in ("dilate", "expand_labels"):
            if int(np.count_nonzero(_fg(data))) * int(np.count_nonzero(~_fg(data))) > BUDGET:
                continue
            out = fuzz_ops.want_of(case)
            dilate_properties(lab, out if case["order"] == "F" else out.T, a, r4, what)
            if op == "expand_labels":   # the two restatements of the definition agree
                grown = morph_oracle.expand_labels(data, case["distance"], fuzz_ops.axis_order(case, case["w_xyz"]))
                assert np.array_equal(_bits(out), _bits(grown)), what
            checked[op] += 1
        elif op == "closing":
            if len(ball_offsets(a, r4)) * data.size > BUDGET:
                continue
            out = fuzz_ops.want_of(case)
            dilated = morph_oracle.dilate(data, case["radius"], fuzz_ops.axis_order(case, case["w_xyz"]))
            grown = dilated if case["order"] == "F" else dilated.T
            eroded = brute_erode(_fg(grown).astype(np.uint8), a, r4, False, True)
            keep = _fg(data) | back(eroded)
            assert np.array_equal(_fg(out), keep), what
            assert np.array_equal(_bits(out), _selected(dilated, keep)), what
            checked[op] += 1
        elif data.size <= MEDIAL_SCATTER_VOXELS:
            kw = fuzz_ops.field_kwargs(case, fuzz_ops.axis_order(case, case["w_xyz"]))
            assert np.array_equal(medial_oracle.on_axis(data, form=medial_oracle.scatter, **kw),
                                  medial_oracle.on_axis(data, form=medial_oracle.gather, **kw)), what
            checked[op] += 1
    return checked


@pytest.mark.parametrize("seed", NOQUANTUM_SEEDS)
def test_noquantum_oracles_against_a_second_opinion(seed):
    checked = noquantum_second_opinions(seed)
    # (erode, opening and local_thickness: the four cases of the eight that have exact factors)
    assert checked["erode"] == checked["opening"] == 4 and checked["closing"] == 8, checked


def test_noquantum_second_opinions_reach_every_operation():
    total = dict.fromkeys(fuzz_ops.NOQUANTUM_OPS, 0)
    for seed in NOQUANTUM_SEEDS:
        for op, n in noquantum_second_opinions(seed).items():
            total[op] += n
    assert all(n >= 5 for n in total.values()), total
    # (what the budgets leave: of the 24 cases of each operation, 12 of erode, opening and local_thickness have exact factors)
    assert total["erode"] == total["opening"] == total["local_thickness"] == 12 and total["closing"] == total["dilate"] == 24, total
    assert total["expand_labels"] >= 20 and total["feature_transform"] >= 8 and total["medial_axis"] >= 15, total
