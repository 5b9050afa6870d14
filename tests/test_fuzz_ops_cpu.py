"""CPU tier of the randomised runs of the label operations (tools/fuzz_ops.py): the same cases the GPU tier draws
(tests/test_gpu_fuzz_ops.py: the same seeds), with the numpy oracles held against a second opinion -- scipy.ndimage and brute
force -- so that the GPU tier does not rest on one restatement; and the generator held to what it promises to cover."""
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
