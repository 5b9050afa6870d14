"""CPU tier of the feature transform and expand_labels: the numpy oracle against brute force, the C ABI's argument
validation (no GPU needed: every refusal comes before device work), the Python surface, and the kernels' resources."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

import ft_oracle
from conftest import ROOT
from synth import blocky_labels, palette_labels

sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW_SYMBOLS = [
    "edt_hip_feature_workspace_bytes", "edt_hip_feature_transform_device", "edt_hip_feature_transform",
    "edt_hip_expand_labels_workspace_bytes", "edt_hip_expand_labels_device", "edt_hip_expand_labels",
]
BAD_ARG, UNSUPPORTED = -2, -4


@pytest.fixture(scope="module")
def lib():
    from edt import _lib
    return _lib.load()


# ---- oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 4, 3), (7, 1, 1), (6, 5, 1), (1, 6, 4), (3, 3, 7)])
@pytest.mark.parametrize("a", [(1, 1, 1), (1, 1, 25), (1, 1, 100), (1, 4, 2)])
@pytest.mark.parametrize("bb", [False, True])
def test_oracle_is_optimal_against_brute_force(shape, a, bb):
    rng = np.random.default_rng(hash((shape, a, bb)) & 0xFFFF)
    for trial in range(3):
        lab = blocky_labels(shape, nlabels=3, zero_frac=0.3, block=2, rng=rng).astype(np.uint16)
        feats, val = ft_oracle.feature_transform(lab, a, bb)
        want = ft_oracle.brute_min(lab, a, bb)
        got = ft_oracle.sqdist(feats, a)
        fg = lab != 0
        has = want < ft_oracle.INF
        assert np.array_equal(got[fg & has], want[fg & has])
        assert np.array_equal(val[fg & has], want[fg & has])
        assert np.all(feats[:, fg & ~has] == -1)
        # background voxels are their own feature, features of foreground voxels carry another label
        grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"))
        assert np.array_equal(feats[:, ~fg], grid[:, ~fg])
        for p in zip(*np.nonzero(fg & has)):
            f = feats[(slice(None),) + p]
            inside = all(0 <= f[c] < shape[c] for c in range(3))
            if inside:
                assert lab[tuple(f)] != lab[p]
            else:
                assert bb and sum(not (0 <= f[c] < shape[c]) for c in range(3)) == 1


def test_oracle_tie_rule_and_no_feature():
    # x-run [1,3] of label 1 in a row of 5: voxel 2 is 2 from both ends -> a-1 = 0
    lab = ft_oracle.x_first(np.array([0, 1, 1, 1, 0], dtype=np.uint8))
    feats, _ = ft_oracle.feature_transform(lab, (1, 1, 1), False, ndim=1)
    assert feats[0, :, 0, 0].tolist() == [0, 0, 0, 4, 4]
    one = np.ones((3, 4, 2), dtype=np.uint8)
    feats, _ = ft_oracle.feature_transform(one, (1, 1, 1), False)
    assert np.all(feats == -1)
    feats, _ = ft_oracle.feature_transform(one, (1, 1, 1), True)
    assert feats.min() == -1 and feats[0].max() == 3


# ---- ABI without a GPU -------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound(lib):
    from edt import _lib
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_workspace_sizes(lib):
    from edt import _lib
    v = 16 * 8 * 4
    assert lib.edt_hip_feature_workspace_bytes(_lib.U32, 3, 16, 8, 4, 0) >= 40 * v
    assert lib.edt_hip_feature_workspace_bytes(_lib.U32, 2, 16, 8, 1, 0) >= 24 * 16 * 8
    assert lib.edt_hip_feature_workspace_bytes(_lib.U32, 1, 16, 1, 1, 1) >= 4 * 16
    assert lib.edt_hip_feature_workspace_bytes(_lib.U32, 4, 16, 8, 4, 0) == 0
    assert lib.edt_hip_feature_workspace_bytes(_lib.U32, 2, 16, 8, 4, 0) == 0   # unused extent != 1
    assert lib.edt_hip_feature_workspace_bytes(_lib.U32, 3, 16, 8, 4, 8) == 0   # EDT_FLAG_BATCH_2D
    assert lib.edt_hip_expand_labels_workspace_bytes(_lib.U32, 3, 16, 8, 4) >= 41 * v
    assert lib.edt_hip_expand_labels_workspace_bytes(99, 3, 16, 8, 4) == 0


def test_validation_before_device_work(lib):
    from edt import _lib
    buf = np.ones(64, dtype=np.uint32)
    feats = np.zeros(3 * 64, dtype=np.int32)
    ws = np.zeros(1 << 16, dtype=np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    dev = lib.edt_hip_feature_transform_device
    # voxel sizes: zero, NaN, inf, negative along x
    for w in ((0.0, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, float("inf")), (-1.0, 1.0, 1.0)):
        assert dev(p(buf), _lib.U32, 3, 4, 4, 4, *w, 0, p(feats), p(ws), ws.nbytes, None) == BAD_ARG
        assert lib.edt_hip_feature_transform(p(buf), _lib.U32, 3, 4, 4, 4, *w, 0, p(feats)) == BAD_ARG
        assert lib.edt_hip_expand_labels(p(buf), _lib.U32, 3, 4, 4, 4, *w, 1.0, p(buf)) == BAD_ARG
    # ndim, unused extents, dtype
    assert dev(p(buf), _lib.U32, 0, 64, 1, 1, 1.0, 1.0, 1.0, 0, p(feats), p(ws), ws.nbytes, None) == BAD_ARG
    assert dev(p(buf), _lib.U32, 4, 4, 4, 4, 1.0, 1.0, 1.0, 0, p(feats), p(ws), ws.nbytes, None) == BAD_ARG
    assert dev(p(buf), _lib.U32, 1, 4, 4, 4, 1.0, 1.0, 1.0, 0, p(feats), p(ws), ws.nbytes, None) == BAD_ARG
    assert dev(p(buf), 99, 3, 4, 4, 4, 1.0, 1.0, 1.0, 0, p(feats), p(ws), ws.nbytes, None) == BAD_ARG
    # NULL pointers and a missing / too small workspace
    assert dev(None, _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, 0, p(feats), p(ws), ws.nbytes, None) == BAD_ARG
    assert dev(p(buf), _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, 0, None, p(ws), ws.nbytes, None) == BAD_ARG
    assert dev(p(buf), _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, 0, p(feats), None, ws.nbytes, None) == BAD_ARG
    assert dev(p(buf), _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, 0, p(feats), p(ws), 64, None) == BAD_ARG
    assert lib.edt_hip_feature_transform(None, _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, 0, p(feats)) == BAD_ARG
    assert lib.edt_hip_feature_transform(p(buf), _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, 0, None) == BAD_ARG
    # flags other than black border / force generic
    for fl in (2, 8, 16, 32, 64):
        assert dev(p(buf), _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, fl, p(feats), p(ws), ws.nbytes, None) == UNSUPPORTED
    # expand_labels: distance, NULL pointers, aliasing
    exd = lib.edt_hip_expand_labels_device
    out = np.zeros_like(buf)
    for d in (-1.0, float("nan")):
        assert exd(p(buf), _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, d, p(out), p(ws), ws.nbytes, None) == BAD_ARG
        assert lib.edt_hip_expand_labels(p(buf), _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, d, p(out)) == BAD_ARG
    assert exd(None, _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, 1.0, p(out), p(ws), ws.nbytes, None) == BAD_ARG
    assert exd(p(buf), _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, 1.0, None, p(ws), ws.nbytes, None) == BAD_ARG
    assert exd(p(buf), _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, 1.0, p(buf), p(ws), ws.nbytes, None) == BAD_ARG
    assert exd(p(buf), _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, 1.0, p(out), p(ws), 16, None) == BAD_ARG
    assert lib.edt_hip_expand_labels(None, _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, 1.0, p(out)) == BAD_ARG
    assert lib.edt_hip_expand_labels(p(buf), _lib.U32, 3, 4, 4, 4, 1.0, 1.0, 1.0, 1.0, None) == BAD_ARG
    # empty volumes are no work at all
    assert dev(p(buf), _lib.U32, 3, 4, 0, 4, 1.0, 1.0, 1.0, 0, p(feats), p(ws), ws.nbytes, None) == 0


# ---- Python surface without a GPU ---------------------------------------------------------------------------------------
def test_python_functions_exist():
    import edt
    assert "feature_transform" in edt.__all__ and "expand_labels" in edt.__all__
    assert callable(edt.feature_transform) and callable(edt.expand_labels)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.uint32, np.int64, np.float32, np.float64, bool])
@pytest.mark.parametrize("shape", [(0,), (3, 0), (0, 2, 5)])
def test_empty_inputs(dtype, shape):
    import edt
    data = np.zeros(shape, dtype=dtype)
    f = edt.feature_transform(data)
    assert f.shape == (len(shape),) + shape and f.dtype == np.int32
    f, d = edt.feature_transform(data, return_distances=True)
    assert f.shape == (len(shape),) + shape and d.shape == shape and d.dtype == np.float32
    e = edt.expand_labels(data, distance=2.0)
    assert e.shape == shape and e.dtype == data.dtype


def test_python_argument_checks():
    import edt
    with pytest.raises(TypeError):
        edt.feature_transform(np.zeros((2, 2, 2, 2), dtype=np.uint8))
    with pytest.raises(TypeError):
        edt.expand_labels(np.zeros((2, 2, 2, 2), dtype=np.uint8))
    with pytest.raises(ValueError):
        edt.feature_transform(np.zeros((2, 3), dtype=np.uint8), anisotropy=(1.0, 0.0))
    with pytest.raises(ValueError):
        edt.feature_transform(np.zeros((2, 3), dtype=np.uint8), anisotropy=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        edt.expand_labels(np.zeros((2, 3), dtype=np.uint8), distance=-1.0)
    with pytest.raises(TypeError):
        edt.feature_transform(np.zeros((2, 3), dtype=np.complex64))


def test_planes_to_axes_layout():
    import edt
    shape = (2, 3, 4)
    grids = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"))
    # C order: x is the last axis, plane 0 holds it
    planes_c = np.concatenate([grids[2].reshape(-1), grids[1].reshape(-1), grids[0].reshape(-1)])
    assert np.array_equal(edt._planes_to_axes(planes_c, shape, "C"), grids)
    # F order: x is the first axis
    planes_f = np.concatenate([grids[c].reshape(-1, order="F") for c in range(3)])
    assert np.array_equal(edt._planes_to_axes(planes_f, shape, "F"), grids)


# ---- resources -----------------------------------------------------------------------------------------------------------
def test_feature_kernels_have_no_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    import q16_resources
    funcs = q16_resources.scan(src="edt_feature.hip")
    kernels = [f for f in funcs if "k_ft_" in f["name"]]
    assert len(kernels) >= 40
    for f in kernels:
        assert f["scratch_ops"] == 0, f


def test_palette_oracle_separates_full_width_labels():
    # the oracle compares at full width: values equal once narrowed stay distinct labels
    lab = ft_oracle.x_first(palette_labels((6, 5, 4), np.float64))
    feats, _ = ft_oracle.feature_transform(lab, (1, 1, 1), False)
    fg = ~(lab == 0)
    for p in zip(*np.nonzero(fg)):
        f = feats[(slice(None),) + p]
        if f[0] >= 0:
            assert not (lab[tuple(f)] == lab[p])
