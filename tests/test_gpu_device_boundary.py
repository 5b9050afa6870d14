"""The device layer's argument boundary (edt/device.py: _input, _workspace): which entry point keeps its scratch in
``device._workspaces`` and which allocates it per call -- the policy _workspace's docstring lists, unchanged since before the
two were one function each --, that a second call of one shape on one stream allocates no scratch, and the refusal of an
``anisotropy`` of the wrong length by the transforms.  8 x 8 x 8 volumes: nothing here depends on the size."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# entry point -> (the query its scratch is cached under, or None where it is allocated per call; the call)
ENTRY_POINTS = {
    "connected_components": ("edt_hip_components_workspace_bytes", lambda d, t: d.connected_components(t)),
    "fill_holes": ("edt_hip_fill_holes_workspace_bytes", lambda d, t: d.fill_holes(t)),
    "dust": ("edt_hip_fill_holes_workspace_bytes", lambda d, t: d.dust(t, 3)),
    "watershed": ("edt_hip_watershed_workspace_bytes", lambda d, t: d.watershed(t)),
    "label_topology": ("edt_hip_label_topology_workspace_bytes", lambda d, t: d.label_topology(t)),
    "erode": ("edt_hip_morphology_workspace_bytes", lambda d, t: d.erode(t, 1.0)),
    "opening": ("edt_hip_morphology_workspace_bytes", lambda d, t: d.opening(t, 1.0)),
    "closing": ("edt_hip_morphology_workspace_bytes", lambda d, t: d.closing(t, 1.0)),
    "local_thickness": ("edt_hip_local_thickness_workspace_bytes", lambda d, t: d.local_thickness(t, radii=[1.0, 2.0])),
    "medial_axis": ("edt_hip_medial_axis_workspace_bytes", lambda d, t: d.medial_axis(t)),
    "feature_transform": (None, lambda d, t: d.feature_transform(t)),
    "expand_labels": (None, lambda d, t: d.expand_labels(t, 2.0)),
    "dilate": (None, lambda d, t: d.dilate(t, 2.0)),
    "label_stats": (None, lambda d, t: d.label_stats(t, d.edt(t))),
    "label_moments": (None, lambda d, t: d.label_moments(t)),
    "edtsq_voxel_graph": (None, lambda d, t: d.edtsq_voxel_graph(t, torch.full(t.shape, 63, dtype=torch.uint8, device=t.device))),
    "runs": (None, lambda d, t: d.runs(t)),
    "edt": (None, lambda d, t: d.edt(t)),                     # (the transforms: their scratch is a Plan's)
    "sdf": (None, lambda d, t: d.sdf(t)),
    "edtsq_stack": (None, lambda d, t: d.edtsq_stack(t)),
}


def volume(dtype):
    """three slabs of labels 1, 2, 0 with a hole in the first; uint32 goes to the device as the int32 of the same bits"""
    v = (np.arange(512).reshape(8, 8, 8) // 128 % 3 + 1) % 3
    v[1, 3:5, 3:5] = 0
    v = v.astype(dtype)
    return torch.from_numpy(v.view(np.int32) if dtype == np.uint32 else v).cuda()


@pytest.mark.parametrize("dtype", [np.uint32, np.uint8])
@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_who_keeps_its_scratch(edt_gpu, name, dtype):
    from edt import device
    query, call = ENTRY_POINTS[name]
    t = volume(dtype)
    device._workspaces.clear()
    call(device, t)
    held = {q: list(c.values()) for q, c in device._workspaces.items()}
    assert {q: len(b) for q, b in held.items()} == ({query: 1} if query else {}), held.keys()
    call(device, t)                                            # the same shape on the same stream: nothing is added
    again = {q: list(c.values()) for q, c in device._workspaces.items()}
    assert again.keys() == held.keys() and all(a is b for q in held for a, b in zip(again[q], held[q]))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["edt", "edtsq", "sdf", "sdfsq", "binary_edtsq"])
@pytest.mark.parametrize("anisotropy", [(1.0, 2.0), (1.0, 2.0, 3.0, 4.0), 2.0])
def test_transforms_refuse_an_anisotropy_of_the_wrong_length(edt_gpu, name, anisotropy):
    from edt import device
    with pytest.raises(ValueError, match="anisotropy must have 3 entries"):
        getattr(device, name)(volume(np.uint8), anisotropy=anisotropy)


def test_label_stats_is_one_class(edt_gpu):
    from edt import device
    assert device.LabelStats is edt_gpu.LabelStats
    assert type(device.label_stats(volume(np.uint8), device.edt(volume(np.uint8)))) is edt_gpu.LabelStats
