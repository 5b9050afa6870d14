"""CPU tier of the voxel sizes without a quantum (tests/noquantum_cases.py): the table is what it claims to be -- the library's
own quantum rule (csrc/edt_colq16_lane.h, compiled for the host) refuses every entry, the EXACT ones have squares that are exact
in fp32 and stay below 2^53 at every extent the GPU tier uses --, the oracles serve them (ft_oracle with exact_factors attains
the brute-force minimum; best_sq equals the brute force), the sizes served so far get the factors they always got, and the
checkers of the GPU tier reject what they must."""
import numpy as np
import pytest

import ft_oracle
import medial_oracle
import morph_oracle
import noquantum_cases as nq
from synth import blocky_labels
from test_q16_logic import q16, quantum  # noqa: F401  (the fixture builds the host shim of the quantum rule)

MAX_EXTENT = 1100        # (no test of tests/test_gpu_feature_noquantum.py has a longer axis)


def cut(w, nd):
    return tuple(w[:nd])


def exact_in_fp32(w):
    sq = np.float64(np.float32(w)) * np.float64(np.float32(w))
    return np.float64(np.float32(sq)) == sq


# ---- the table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", list(nq.EXACT))
def test_exact_sizes_have_no_quantum_and_exact_squares(q16, w):  # noqa: F811
    a = nq.EXACT[w]
    assert len(nq.EXACT) == 7
    for nd in (3, 2):
        assert not quantum(q16, cut(w, nd))[0], (w, nd)
        assert all(exact_in_fp32(v) for v in cut(w, nd))
        fac = ft_oracle.exact_factors(cut(w, nd))
        # the table's factors, cut: the same ratios (a 2-D cut may reduce further)
        assert all(fac[i] * a[0] == fac[0] * a[i] for i in range(nd)), (w, nd, fac)
        assert nq.exact_bound(fac, (MAX_EXTENT,) * nd) < 2 ** 53
    assert ft_oracle.exact_factors(w) == a
    assert nq.exact_bound(a, (MAX_EXTENT,) * 3) < 2 ** 53
    # w_i^2 = a_i q with one q
    sq = nq.squares(w)
    assert sq[0] * a[1] == sq[1] * a[0] and sq[0] * a[2] == sq[2] * a[0]
    assert max(a) > 16384                            # (why the 16-bit windows refuse them)


def test_a_cut_that_has_a_quantum_is_left_out(q16):  # noqa: F811
    assert not quantum(q16, (1.5, 1.0078125, 2.0))[0]
    ok, _, a = quantum(q16, (1.5, 1.0078125))
    assert ok and a[:2] == [4096, 1849]
    assert (1.5, 1.0078125, 2.0) not in nq.EXACT


@pytest.mark.parametrize("w", nq.INEXACT)
def test_inexact_sizes_have_no_quantum_and_no_factors(q16, w):  # noqa: F811
    assert len(nq.INEXACT) == 4
    for nd in (3, 2):
        assert not quantum(q16, cut(w, nd))[0], (w, nd)
    with pytest.raises(AssertionError):
        ft_oracle.exact_factors(w)
    with pytest.raises(AssertionError):
        morph_oracle._quantum_factors(w)
    with pytest.raises(AssertionError):
        medial_oracle.quantum(w)


def _smallest_square_factors(w):
    """the rule morph_oracle and medial_oracle had before exact_factors: divide by the smallest square"""
    from fractions import Fraction
    w2 = [Fraction(float(np.float32(v))) ** 2 for v in w]
    a = [v / min(w2) for v in w2]
    assert all(f.denominator == 1 for f in a)
    return [int(f) for f in a]


def test_sizes_served_before_keep_their_factors():
    from test_gpu_feature_transform import QUANTUM
    assert len(QUANTUM) == 4
    for w, a in QUANTUM.items():
        for nd in (1, 2, 3):
            assert ft_oracle.exact_factors(cut(w, nd)) == tuple(a[:nd]) == tuple(_smallest_square_factors(cut(w, nd)))
            assert tuple(morph_oracle._quantum_factors(cut(w, nd))) == tuple(a[:nd]) == medial_oracle.quantum(cut(w, nd))
    # the integer sizes of tests/test_gpu_morph.py, test_gpu_medial.py, test_gpu_feature_transform.py, tools/fuzz_ops.py:
    # padded with unit axes as morph_oracle.expand_labels pads them
    served = [(1.0,), (2.0,), (3.0,), (2.0, 1.0), (1.0, 2.0), (1.0, 1.0, 1.0), (3.0, 1.0, 2.0), (2.0, 1.0, 3.0), (1.0, 2.0, 1.0),
              (2.0, 3.0, 1.0), (1.0, 3.0, 2.0), (30.0, 6.0, 6.0), (40.0, 4.0, 4.0), (1.0, 0.5, 0.5), (6.0, 6.0), (4.0, 4.0, 1.0),
              (0.5, 0.5, 1.0), (2.0, 2.0, 1.0), (3.0, 3.0, 3.0), (6.0, 1.0, 1.0), (0.5, 1.0, 1.0)]
    served += [(float(x), float(y), float(z)) for x in (1, 2, 3) for y in (1, 2, 3) for z in (1, 2, 3) if 1 in (x, y, z)]
    for w in served:
        old = _smallest_square_factors(w)
        assert list(ft_oracle.exact_factors(w)) == old == morph_oracle._quantum_factors(w), w
        assert medial_oracle.quantum(w) == tuple(old), w


# ---- the oracles on these sizes ---------------------------------------------------------------------------------------------
def brute_sq(lab, w, bb):
    """O(N^2) fp64 minimum of D(p, q) over the voxels q whose label does not compare equal to p's, 1-D to 3-D, x first"""
    nd = lab.ndim
    if bb:
        pad = np.zeros(tuple(s + 2 for s in lab.shape), dtype=lab.dtype)
        pad[(slice(1, -1),) * nd] = lab
    else:
        pad = lab
    off = 1 if bb else 0
    coords = np.stack(np.meshgrid(*[np.arange(s) - off for s in pad.shape], indexing="ij"), -1).reshape(-1, nd)
    flat = pad.reshape(-1)
    w2 = nq.squares(w)[:nd]
    out = np.zeros(lab.shape)
    for idx in np.ndindex(lab.shape):
        if lab[idx] == 0:
            continue
        other = ~(flat == lab[idx])
        if not other.any():
            out[idx] = np.inf
            continue
        d = np.zeros(int(other.sum()))
        for c in range(nd):
            d = d + w2[c] * ((coords[other, c] - idx[c]) ** 2).astype(np.float64)
        out[idx] = d.min()
    return out


SHAPES = ((11,), (9, 8), (9, 8, 7))


@pytest.mark.parametrize("w", list(nq.EXACT))
@pytest.mark.parametrize("bb", [False, True])
def test_ft_oracle_with_exact_factors_attains_the_brute_minimum(w, bb):
    from test_fuzz_ops_cpu import _brute_min_nd
    for nd, shape in ((2, (7, 6)), (3, (6, 5, 4))):
        a = ft_oracle.exact_factors(cut(w, nd))
        lab = blocky_labels(shape, nlabels=3, zero_frac=0.2, block=2, rng=np.random.default_rng(nd)).astype(np.uint8)
        lab3 = lab.reshape(shape + (1,) * (3 - nd))
        feats, _ = ft_oracle.feature_transform(lab3, a + (1,) * (3 - nd), bb, ndim=nd)
        d = ft_oracle.sqdist(feats, a + (0,) * (3 - nd))
        want = ft_oracle.brute_min(lab3, a, bb) if nd == 3 else _brute_min_nd(lab3, a, bb, nd)
        assert np.array_equal(np.where(d >= 0, d, ft_oracle.INF), want), (w, nd)
        nq.check_features(lab3, feats, cut(w, nd), bb, nd)


@pytest.mark.parametrize("w", list(nq.EXACT)[:2] + list(nq.INEXACT))
@pytest.mark.parametrize("bb", [False, True])
def test_best_sq_equals_the_brute_force(w, bb):
    from test_gpu_feature_transform import brute_d
    for shape in SHAPES:
        nd = len(shape)
        for dtype, nlabels in ((np.uint32, 4), (np.float32, 3), (bool, 1)):
            ids = blocky_labels(shape, nlabels=nlabels, zero_frac=0.2, block=2, rng=np.random.default_rng(nd + nlabels))
            lab = (ids != 0) if dtype is bool else ids.astype(dtype)
            got = nq.best_sq(lab, cut(w, nd), bb)
            assert np.array_equal(got, brute_sq(lab, cut(w, nd), bb)), (w, shape, dtype)
            if nd == 3:
                w32 = np.array(w, dtype=np.float32).astype(np.float64)
                assert np.array_equal(got, brute_d(lab, w32, bb)), (w, dtype)
    one = np.full((5, 4), 7, dtype=np.uint16)
    assert np.all(np.isinf(nq.best_sq(one, cut(w, 2), False)))
    assert np.all(np.isfinite(nq.best_sq(one, cut(w, 2), True)))


# ---- the checkers reject what they must -------------------------------------------------------------------------------------
W_VALID, A_VALID = (6.0, 6.0, 30.0), (1, 1, 25)


def _valid(bb, seed=3):
    lab = blocky_labels((9, 8, 7), nlabels=3, zero_frac=0.2, block=3, rng=np.random.default_rng(seed)).astype(np.uint8)
    feats, _ = ft_oracle.feature_transform(lab, A_VALID, bb)
    nq.check_features(lab, feats, W_VALID, bb, 3)
    return lab, feats


def _rejected(lab, feats, bb):
    with pytest.raises(AssertionError):
        nq.check_features(lab, feats, W_VALID, bb, 3)


def _inside(f, shape):
    return all(0 <= int(v) < s for v, s in zip(f, shape))


def test_check_features_rejects_a_feature_of_the_own_label():
    lab, feats = _valid(False)
    p = tuple(np.argwhere(lab != 0)[5])
    bad = feats.copy()
    bad[(slice(None),) + p] = p
    _rejected(lab, bad, False)


@pytest.mark.parametrize("bb", [False, True])
def test_check_features_rejects_a_feature_one_voxel_farther(bb):
    lab, feats = _valid(bb)
    found = 0
    for p in map(tuple, np.argwhere(lab != 0)):
        f = feats[(slice(None),) + p]
        for c in range(3):
            if f[c] == p[c]:
                continue
            g = f.copy()
            g[c] += 1 if f[c] > p[c] else -1
            if _inside(f, lab.shape) and _inside(g, lab.shape) and lab[tuple(g)] != lab[p]:
                bad = feats.copy()
                bad[(slice(None),) + p] = g
                _rejected(lab, bad, bb)
                found += 1
        if found >= 5:
            break
    assert found >= 5


def test_check_features_rejects_a_border_feature_off_in_two_components():
    lab, feats = _valid(True)
    ext = np.array(lab.shape).reshape(3, 1, 1, 1)
    outside = np.any((feats < 0) | (feats >= ext), axis=0) & (lab != 0)
    assert outside.any()
    for p in map(tuple, np.argwhere(outside)[:4]):
        f = feats[(slice(None),) + p]
        c = next(k for k in range(3) if 0 <= f[k] < lab.shape[k])
        for v in (-1, lab.shape[c]):
            bad = feats.copy()
            bad[(c,) + p] = v
            _rejected(lab, bad, True)
        # ... or two voxels outside, or on the shell away from the voxel's own row
        k = next(k for k in range(3) if not 0 <= f[k] < lab.shape[k])
        bad = feats.copy()
        bad[(k,) + p] = -2 if f[k] < 0 else lab.shape[k] + 1
        _rejected(lab, bad, True)
        bad = feats.copy()
        bad[(c,) + p] = (p[c] + 1) % lab.shape[c]
        _rejected(lab, bad, True)
    # and no feature lies outside without a border
    lab, feats = _valid(False)
    p = tuple(np.argwhere(lab != 0)[0])
    bad = feats.copy()
    bad[(0,) + p] = -1
    _rejected(lab, bad, False)


def test_check_features_rejects_a_missing_feature_and_a_moved_background():
    lab, feats = _valid(False)
    p = tuple(np.argwhere(lab != 0)[7])
    bad = feats.copy()
    bad[(slice(None),) + p] = -1
    _rejected(lab, bad, False)
    q = tuple(np.argwhere(lab == 0)[2])
    for c in range(3):
        bad = feats.copy()
        bad[(c,) + q] += 1 if q[c] + 1 < lab.shape[c] else -1
        _rejected(lab, bad, False)
    # one label throughout: -1 everywhere is right, a feature is not
    one = np.full((4, 3, 2), 5, dtype=np.uint8)
    feats, _ = ft_oracle.feature_transform(one, A_VALID, False)
    assert np.all(feats == -1)
    nq.check_features(one, feats, W_VALID, False, 3)
    bad = feats.copy()
    bad[:, 1, 1, 1] = (0, 0, 0)
    _rejected(one, bad, False)


def _expand_by_brute_force(lab, distance, w):
    """expand_labels from its definition with the nearest foreground voxel by brute force in fp64 (first minimum)"""
    nd = lab.ndim
    w2 = nq.squares(w)[:nd]
    src = np.argwhere(lab != 0)
    out = lab.copy()
    best = np.full(lab.shape, np.inf)
    for p in map(tuple, np.argwhere(lab == 0)):
        d = np.zeros(len(src))
        for c in range(nd):
            d = d + w2[c] * ((src[:, c] - p[c]) ** 2).astype(np.float64)
        k = int(np.argmin(d))
        best[p] = d[k]
        if d[k] <= np.float64(distance) ** 2:
            out[p] = lab[tuple(src[k])]
    return out, best


@pytest.mark.parametrize("w", [(1.1, 0.7, 2.3), (3.58, 3.58, 40.0)])
@pytest.mark.parametrize("shape", [(40,), (12, 11), (9, 8, 7)])
def test_check_expand_accepts_the_definition_and_rejects_what_it_must(w, shape):
    nd = len(shape)
    w = cut(w, nd)
    lab = blocky_labels(shape, nlabels=4, zero_frac=0.6, block=2, rng=np.random.default_rng(nd)).astype(np.float32)
    step = min(w)
    # (a distance of `step` itself would tie with the fp32 size's own square: whole multiples are left to the exact sizes)
    for distance in (0.0, 1.25 * step, 2.5 * step, np.inf):
        assert nq.undecided(lab, distance, w) == 0
        out, best = _expand_by_brute_force(lab, distance, w)
        assert nq.check_expand(lab, out, distance, w) == 0
    distance = 2.5 * step
    out, best = _expand_by_brute_force(lab, distance, w)
    d2 = np.float64(distance) ** 2
    filled = np.argwhere((lab == 0) & (out != 0))
    empty = np.argwhere((lab == 0) & (out == 0))
    assert len(filled) and len(empty)

    def rejected(bad):
        with pytest.raises(AssertionError):
            nq.check_expand(lab, bad, distance, w)

    # a wrong label taken: one the volume holds, but not the nearest's -- and one it does not hold
    p = tuple(filled[0])
    others = [v for v in np.unique(lab) if v != 0 and v != out[p]]
    tried = 0
    for v in others:
        bad = out.copy()
        bad[p] = v
        far = nq._nearest_zero_sq(lab != v, w)[p]
        if far > best[p] * nq.UPPER:
            rejected(bad)
            tried += 1
    assert tried
    bad = out.copy()
    bad[p] = 77.0
    rejected(bad)
    # a reachable voxel left empty
    bad = out.copy()
    bad[p] = 0
    rejected(bad)
    # a voxel filled beyond the distance
    q = tuple(empty[0])
    assert best[q] > d2
    bad = out.copy()
    bad[q] = lab[lab != 0][0]
    rejected(bad)
    # a foreground voxel changed
    r = tuple(np.argwhere(lab != 0)[0])
    bad = out.copy()
    bad[r] = 0
    rejected(bad)


def test_undecided_counts_the_band():
    lab = np.zeros((8,), dtype=np.uint8)
    lab[0] = 3
    w = (1.1,)
    d = float(np.sqrt(nq.squares(w)[0] * 9.0))                  # the voxel at x = 3 lies at exactly this distance, or just inside
    assert nq.undecided(lab, d * (1 + 2.0 ** -22), w) == 1
    assert nq.undecided(lab, d * (1 + 2.0 ** -19), w) == 0
    assert nq.undecided(lab, 1.0, w) == 0
