"""GPU tier: every device entry point on OFFSET pointers (include/edt_hip.h, "Alignment": label, field and output pointers need
the alignment of their element type and nothing more).

The torch allocator hands out buffers aligned to 512 bytes, so no other test reaches the fallback branch of an alignment
gate on a shape that otherwise takes the vector path.  Here every array under test is a view ``buf[16 + k : 16 + k + n]`` of
a larger device buffer (tests/synth.py: offset_view): element-aligned and, for k = 1, 2, 3, off every wider boundary.

  * inputs: the buffer around the labels holds the first / last voxel's own non-zero label -- a kernel that reads past
    either end and uses what it read lengthens a run or joins a component and fails the comparison;
  * outputs: the buffer, view included, is filled with a sentinel (a NaN payload for fp32) before the call; afterwards the
    view equals the oracle bit for bit and everything outside it still holds the sentinel's bits -- a vector store that runs
    past the head or the tail shows;
  * expectation: the CPU oracle (oracle_port for the transforms, the numpy oracles of tests/ for the rest), for the aligned
    call (k = 0) and for every offset, bit for bit -- no tolerances;
  * where the pass log tells the forms apart (the signed transform: its sign is the last integer pass's epilogue, or a pass
    of its own named "sign"), the aligned call took the fused form and the offset call did not.

The record forms of the sharded path document 8- and 16-byte requirements of their blocks: a block at a 4-byte offset is
refused before any launch.  A misaligned WORKSPACE is refused by every entry point that takes one (the last test; the entry
points that validate without a device are held to that in the CPU tier, tests/test_workspace_alignment_cpu.py)."""
import ctypes

import numpy as np
import pytest

import components_oracle
import dust_oracle
import fill_holes_oracle
import ft_oracle
import label_stats_oracle
import medial_oracle
import morph_oracle
import thickness_oracle
from synth import bits_of, blocky_labels, offset_out, offset_view, outside_intact

pytestmark = pytest.mark.gpu

U8, U16, U32, U64, F32, F64, BOOL = range(7)
BAD_ARG = -2
CODE = {"uint8": U8, "int8": U8, "uint16": U16, "int16": U16, "uint32": U32, "int32": U32, "uint64": U64, "int64": U64,
        "float32": F32, "float64": F64, "bool": BOOL}
WIDTHS = [np.uint8, np.uint16, np.uint32, np.uint64]          # one label type of every width
NAN = 0x7FC0BEEF                                              # sentinel of fp32 outputs: a NaN with a payload
MARK = {1: 0xA5, 2: 0xA5A5, 4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}   # sentinel of integer outputs, by width


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    from edt import _lib
    _lib.load()
    if not torch.cuda.is_available() or _lib.device_count() == 0:
        pytest.fail("the GPU tier needs a HIP device")
    torch.cuda.set_device(0)


def lib():
    from edt import _lib
    return _lib.load()


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    import torch
    torch.cuda.synchronize()


def workspace(nbytes):
    import torch
    assert nbytes > 0
    return torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")


def ok(rc):
    from edt import _lib
    _lib.check(rc)


def ext3(a):
    """x-fastest extents (sx, sy, sz) of a C-ordered array"""
    return tuple(int(e) for e in a.shape[::-1]) + (1,) * (3 - a.ndim)


def labels_c(ext_xyz, dtype=np.uint8, seed=0, zero_frac=0.2, block=5, nlabels=4):
    """C-ordered labels (x the last axis) in 0..nlabels whose first and last voxel, in memory order, are non-zero"""
    shape = tuple(ext_xyz[::-1])
    ids = blocky_labels(shape, nlabels=nlabels, zero_frac=zero_frac, block=block, rng=np.random.default_rng(seed))
    ids.flat[0] = ids.flat[-1] = 3
    return (ids != 0) if np.dtype(dtype) == np.bool_ else ids.astype(dtype)


def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def out_matches(obuf, oview, k, want_bits, what):
    """the view equals the expectation bit for bit and the buffer around it still holds the sentinel"""
    sync()
    size = oview.element_size()
    sentinel = NAN if oview.dtype.is_floating_point else MARK[size]
    got = bits_of(oview)
    assert got.shape == want_bits.shape, what
    assert np.array_equal(got, want_bits), (what, "mismatches", int((got != want_bits).sum()))
    assert outside_intact(obuf, k, oview.numel(), sentinel), (what, "a store outside the output")


def out_buffer(shape, dtype, k):
    dt = np.dtype(dtype)
    return offset_out(shape, dt, k, NAN if dt.kind == "f" else MARK[dt.itemsize])


# ---- 1-3. edt_hip_edtsq_device through device.Plan.run(out=...) ---------------------------------------------------------
_plans, _wants = {}, {}


def plan_for(ext, code):
    from edt import device
    key = (tuple(ext), code)
    if key not in _plans:
        _plans[key] = device.Plan(ext, code)
    return _plans[key]


def run_plan(lab, w_xyz, bb, sqrt, k_lab, k_out, want, what, **kw):
    """Plan.run on labels at offset k_lab into an output at offset k_out; the names of the passes it launched"""
    from edt import device
    ext = tuple(int(e) for e in lab.shape[::-1])
    plan = plan_for(ext, CODE[lab.dtype.name])
    _, lview = offset_view(lab, k_lab)
    obuf, oview = out_buffer(lab.shape, np.float32, k_out)
    device.set_profiling(True)
    try:
        got = plan.run(lview, w_xyz, black_border=bb, sqrt=sqrt, out=oview, **kw)
        sync()
        names = [n for n, _ in device.pass_times()]
    finally:
        device.set_profiling(False)
    assert got.data_ptr() == oview.data_ptr()
    out_matches(obuf, oview, k_out, f32_bits(want), (what, lab.dtype.name, ext, w_xyz, bb, sqrt, k_lab, k_out))
    return names


# (label dtype, offset of the labels, offset of the output); the first is the aligned call
PLAN_OFFSETS = [(np.uint32, 0, 0),
                (np.uint32, 0, 1), (np.uint32, 0, 2), (np.uint32, 0, 3),
                (np.uint8, 1, 0), (np.uint8, 2, 0), (np.uint8, 3, 0), (np.uint16, 1, 0), (np.uint16, 3, 0),
                (np.uint32, 1, 0), (np.uint64, 1, 0),
                (np.uint8, 3, 1), (np.uint16, 1, 3), (np.uint32, 1, 2)]
# (64, 40, 36) at sizes without a quantum: the fp32 wave kernel, rows of whole 16-byte granules -- only the pointer clears
# its aligned16; (64, 100, 100) at (6, 6, 30): both column axes on the 16-bit integer kernel when aligned
PLAN_CASES = [((64, 40, 36), (0.7, 1.3, 2.1)), ((64, 100, 100), (6.0, 6.0, 30.0))]


def transform_want(oracle_port, ext, w, bb, signed=False):
    key = (ext, w, bb, signed)
    if key not in _wants:
        lab = labels_c(ext, np.uint8, seed=sum(ext), zero_frac=0.45 if signed else 0.2)
        sq = oracle_port.sdfsq(lab, w[::-1], bb) if signed else oracle_port.edtsq(lab, w[::-1], bb)
        rt = oracle_port.sdf(lab, w[::-1], bb) if signed else np.sqrt(sq)
        _wants[key] = (lab, sq, rt)
    return _wants[key]


@pytest.mark.parametrize("bb", [True, False])
@pytest.mark.parametrize("ext,w", PLAN_CASES)
def test_transform_on_offset_labels_and_output(oracle_port, ext, w, bb):
    lab8, sq, rt = transform_want(oracle_port, ext, w, bb)
    for sqrt in (False, True):
        for dtype, k_lab, k_out in PLAN_OFFSETS:
            run_plan(lab8.astype(dtype), w, bb, sqrt, k_lab, k_out, rt if sqrt else sq, "edtsq_device")


@pytest.mark.parametrize("bb", [True, False])
def test_transform_rows_that_are_no_whole_granules(oracle_port, bb):
    """sx % 4 != 0 clears the gate whatever the pointer: the same through offset pointers"""
    lab8, sq, rt = transform_want(oracle_port, (65, 40, 36), (0.7, 1.3, 2.1), bb)
    for sqrt in (False, True):
        for dtype, k_lab, k_out in ((np.uint8, 0, 0), (np.uint8, 1, 1), (np.uint16, 1, 2)):
            run_plan(lab8.astype(dtype), (0.7, 1.3, 2.1), bb, sqrt, k_lab, k_out, rt if sqrt else sq, "edtsq_device, sx = 65")


@pytest.mark.parametrize("bb", [True, False])
@pytest.mark.parametrize("ext,w", [((64, 100, 100), (6.0, 6.0, 30.0)), ((64, 40, 36), (0.7, 1.3, 2.1))])
def test_signed_transform_into_an_offset_output(oracle_port, ext, w, bb):
    """EDT_FLAG_SIGNED = edt(x) - edt(x == 0), as tests/test_gpu_extras.py builds it.  Where both column passes provably stay on
    the integer kernel the aligned call negates in the last pass's epilogue; an output off the 16-byte grid leaves that form,
    and the sign is the streaming pass "sign", which serves any float-aligned output."""
    lab8, sq, rt = transform_want(oracle_port, ext, w, bb, signed=True)
    assert (sq < 0).any() and (sq > 0).any()
    assert plan_for(ext, U8).signed_supported()
    py, pz = ctypes.c_int(0), ctypes.c_int(0)
    quantum = lib().edt_hip_q16_no_refusals(*ext, *w, 3, int(bb), ctypes.byref(py), ctypes.byref(pz))
    fused_when_aligned = bool(quantum and py.value and pz.value)
    if w == (6.0, 6.0, 30.0) and bb:
        assert fused_when_aligned       # (the case that shows the gate; bb = False is decided by the library's own proof)
    for sqrt in (False, True):
        for k_out in (0, 1, 2, 3):
            names = run_plan(lab8, w, bb, sqrt, 0, k_out, rt if sqrt else sq, "signed", signed=True)
            assert ("sign" in names) == (not (fused_when_aligned and k_out == 0)), (ext, w, bb, k_out, names)


def test_stack_of_images_and_line_into_an_offset_output(oracle_port):
    rng = np.random.default_rng(9)
    stack = blocky_labels((9, 64, 64), nlabels=6, zero_frac=0.15, block=7, rng=rng).astype(np.uint32)
    stack.flat[0] = stack.flat[-1] = 3
    for an, bb in (((1.0, 1.0), False), ((3.0, 0.5), True)):
        want = np.stack([oracle_port.edtsq(img, an, bb) for img in stack])
        for sqrt in (False, True):
            for k_lab, k_out in ((0, 0), (0, 1), (1, 1)):
                run_plan(stack, (an[1], an[0], 1.0), bb, sqrt, k_lab, k_out, np.sqrt(want) if sqrt else want, "stack", batch2d=True)
    line = blocky_labels((1025,), nlabels=5, zero_frac=0.2, block=37, rng=rng).astype(np.uint16)
    line[0] = line[-1] = 3
    for w, bb in ((1.0, False), (0.7, True)):
        want = oracle_port.edtsq(line, w, bb)
        for sqrt in (False, True):
            for k_lab, k_out in ((0, 0), (0, 1), (3, 1)):
                run_plan(line, (w,), bb, sqrt, k_lab, k_out, np.sqrt(want) if sqrt else want, "line")


# ---- 4. edt_hip_edtsq_voxel_graph_device ---------------------------------------------------------------------------------
def voxel_graph_call(lab, graph, w_xyz, bb, k_lab, k_graph, k_out, want, what):
    L = lib()
    ext = ext3(lab)
    w = tuple(w_xyz) + (1.0,) * (3 - lab.ndim)
    _, lview = offset_view(lab, k_lab)
    _, gview = offset_view(graph, k_graph)
    obuf, oview = out_buffer(lab.shape, np.float32, k_out)
    ws = workspace(L.edt_hip_voxel_graph_workspace_bytes(lab.ndim, *ext))
    ok(L.edt_hip_edtsq_voxel_graph_device(vp(lview), CODE[lab.dtype.name], vp(gview), lab.ndim, *ext, *w, 1 if bb else 0,
                                          vp(oview), vp(ws), ws.numel(), stream()))
    out_matches(obuf, oview, k_out, f32_bits(want), (what, ext, w_xyz, bb, k_lab, k_graph, k_out))


@pytest.mark.parametrize("ext", [(32, 20, 12), (64, 33)])
def test_voxel_graph_on_offset_pointers(oracle_port, ext):
    """out % 8 switches the integer form off, out % 16 the 16-byte stores of the fp32 kernel's compact rows; under debug bit
    0x200000 (the separate gather pass) out % 16 chooses between its four-cell and its cell-by-cell form"""
    L = lib()
    rng = np.random.default_rng(sum(ext))
    lab = labels_c(ext, np.uint8, seed=3, zero_frac=0.25)
    graph = np.full(lab.shape, 0b00111111, dtype=np.uint8)
    for bit in (0x01, 0x04, 0x10):
        graph[rng.random(lab.shape) < 0.08] &= np.uint8(~bit & 0xFF)
    nd = len(ext)
    for w in ((1.0, 1.0, 1.0)[:nd], (0.7, 1.3, 2.1)[:nd]):
        for bb in (True, False):
            want = oracle_port.edtsq(lab, w[::-1], bb, voxel_graph=graph)
            for mode in (0, 0x200000):
                L.edt_hip_set_debug_mode(mode)
                try:
                    for k_lab, k_graph, k_out in ((0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3), (0, 1, 0), (1, 0, 0), (1, 1, 1)):
                        voxel_graph_call(lab, graph, w, bb, k_lab, k_graph, k_out, want, ("voxel graph", hex(mode)))
                    voxel_graph_call(lab.astype(np.uint16), graph, w, bb, 1, 1, 3, want, ("voxel graph, uint16", hex(mode)))
                finally:
                    L.edt_hip_set_debug_mode(0)


# ---- 5, 6. the streaming helpers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64, bool])
def test_select_label_with_dt_and_out_that_disagree_modulo_16(dtype):
    """k_select_label gates per quad on dt + i and out + i: dt at offset 1 and out at offset 2 never agree, 0 and 0 always do,
    1 and 1 agree from the third quad on"""
    L = lib()
    n = 1003
    rng = np.random.default_rng(5)
    lab = labels_c((n,), dtype, seed=8, block=3)
    dt = rng.random(n).astype(np.float32) + 1.0
    key = np.array([True if np.dtype(dtype) == np.bool_ else 3], dtype=dtype)
    want = np.where(lab == key[0], dt, np.float32(0)).astype(np.float32)
    for k_lab, k_dt, k_out in ((0, 0, 0), (0, 1, 2), (1, 1, 2), (1, 1, 1), (3, 2, 3), (0, 0, 1), (0, 3, 0)):
        _, lview = offset_view(lab, k_lab)
        _, dview = offset_view(dt, k_dt, NAN)
        obuf, oview = out_buffer((n,), np.float32, k_out)
        ok(L.edt_hip_select_label_device(vp(lview), CODE[np.dtype(dtype).name], vp(dview), ctypes.c_void_p(key.ctypes.data), vp(oview),
                                         n, stream()))
        out_matches(obuf, oview, k_out, f32_bits(want), ("select_label", dtype, k_lab, k_dt, k_out))


@pytest.mark.parametrize("n", [1003, 5])
def test_subtract_is_background_and_extract_runs(n):
    import torch
    L = lib()
    rng = np.random.default_rng(n)
    a, b = rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)
    for ka, kb, ko in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3)):
        _, av = offset_view(a, ka, NAN)
        _, bv = offset_view(b, kb, NAN)
        obuf, oview = out_buffer((n,), np.float32, ko)
        ok(L.edt_hip_subtract_device(vp(av), vp(bv), vp(oview), n, stream()))
        out_matches(obuf, oview, ko, f32_bits(a - b), ("subtract", n, ka, kb, ko))
    for dtype in WIDTHS + [np.float32, np.float64, bool]:
        lab = labels_c((n,), dtype, seed=n, block=2)
        for k_lab, k_mask in ((0, 0), (1, 0), (0, 1), (1, 1)):
            _, lview = offset_view(lab, k_lab)
            obuf, oview = out_buffer((n,), np.uint8, k_mask)
            ok(L.edt_hip_is_background_device(vp(lview), CODE[np.dtype(dtype).name], vp(oview), n, stream()))
            out_matches(obuf, oview, k_mask, (lab == 0).astype(np.uint8), ("is_background", dtype, n, k_lab, k_mask))
        starts_want = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]]).astype(np.int64)
        for k_lab in (0, 1, 3):
            _, lview = offset_view(lab, k_lab)
            ws = workspace(L.edt_hip_runs_workspace_bytes(n))
            count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            obuf, oview = out_buffer((len(starts_want),), np.int64, 1)
            ok(L.edt_hip_extract_runs_device(vp(lview), CODE[np.dtype(dtype).name], n, vp(oview), len(starts_want), vp(count), vp(ws),
                                             ws.numel(), stream()))
            sync()
            assert int(count) == len(starts_want), ("extract_runs", dtype, n, k_lab)
            out_matches(obuf, oview, 1, starts_want.view(np.uint64), ("extract_runs", dtype, n, k_lab))


# ---- 7. feature transform and expand_labels ------------------------------------------------------------------------------
def ft_want(lab, a, bb):
    """the oracle's features as the ABI lays them out: ndim planes (x, y, z) of the C-ordered volume"""
    nd = lab.ndim
    feats, _ = ft_oracle.feature_transform(ft_oracle.x_first(lab), a, bb, ndim=nd)
    return np.stack([np.ascontiguousarray(feats[k].reshape(lab.shape[::-1]).T) for k in range(nd)]).astype(np.int32)


@pytest.mark.parametrize("ext", [(33, 20, 12), (64, 20, 12)])
def test_feature_transform_and_expand_labels_on_offset_pointers(ext):
    L = lib()
    for w, a in (((1.0, 1.0, 1.0), (1, 1, 1)), ((6.0, 6.0, 30.0), (1, 1, 25))):
        lab8 = labels_c(ext, np.uint8, seed=ext[0], zero_frac=0.3, block=4)
        for bb in (False, True):
            want = ft_want(lab8, a, bb)
            for dtype, k_lab, k_out in ((np.uint8, 0, 0), (np.uint8, 0, 1), (np.uint8, 0, 2), (np.uint8, 0, 3), (np.uint8, 3, 0),
                                        (np.uint16, 1, 0), (np.uint32, 1, 1), (np.uint64, 1, 2), (np.float32, 1, 3)):
                lab = lab8.astype(dtype)
                code = CODE[np.dtype(dtype).name]
                flags = 1 if bb else 0
                _, lview = offset_view(lab, k_lab)
                obuf, oview = out_buffer((3,) + lab.shape, np.int32, k_out)
                ws = workspace(L.edt_hip_feature_workspace_bytes(code, 3, *ext, flags))
                ok(L.edt_hip_feature_transform_device(vp(lview), code, 3, *ext, *w, flags, vp(oview), vp(ws), ws.numel(), stream()))
                out_matches(obuf, oview, k_out, want.view(np.uint32), ("feature_transform", ext, w, bb, dtype, k_lab, k_out))
        # expand_labels: the definition of include/edt_hip.h from the oracle's features of the mask labels == 0 (no border)
        f = ft_want((lab8 == 0).astype(np.uint8), a, False)            # planes x, y, z
        grids = np.stack(np.meshgrid(*[np.arange(s) for s in lab8.shape], indexing="ij"))[::-1]   # coordinates x, y, z
        w2 = [np.float64(np.float32(v)) * np.float64(np.float32(v)) for v in w]
        D = np.zeros(lab8.shape)
        for k in range(3):                                            # terms added in ABI order x, y, z
            D = D + w2[k] * ((grids[k] - f[k]).astype(np.int64) ** 2).astype(np.float64)
        has = ~np.all(f == -1, axis=0)
        for distance in (1.0, 2.5 * w[0], np.inf):
            take = (lab8 == 0) & has & (D <= np.float64(distance) * np.float64(distance))
            src = tuple(np.where(take, f[k], 0) for k in (2, 1, 0))
            for dtype, k_lab, k_out in ((np.uint8, 0, 0), (np.uint8, 1, 0), (np.uint8, 0, 1), (np.uint8, 3, 2), (np.uint16, 1, 3),
                                        (np.uint32, 1, 1), (np.uint64, 1, 1), (np.float64, 1, 1)):
                lab = lab8.astype(dtype)
                want = lab.copy()
                want[take] = lab[src][take]
                code = CODE[np.dtype(dtype).name]
                _, lview = offset_view(lab, k_lab)
                obuf, oview = out_buffer(lab.shape, dtype, k_out)
                ws = workspace(L.edt_hip_expand_labels_workspace_bytes(code, 3, *ext))
                ok(L.edt_hip_expand_labels_device(vp(lview), code, 3, *ext, *w, float(distance), vp(oview), vp(ws), ws.numel(), stream()))
                out_matches(obuf, oview, k_out, want.view(f"u{want.dtype.itemsize}"),
                            ("expand_labels", ext, w, distance, dtype, k_lab, k_out))


# ---- 8. label_stats ----------------------------------------------------------------------------------------------------------
def test_label_stats_on_offset_labels_and_field():
    import torch
    L = lib()
    ext = (9, 33, 40)
    rng = np.random.default_rng(40)
    dt = (rng.integers(-3, 4, size=ext[::-1]).astype(np.float32) * np.float32(0.75))
    dt[rng.random(dt.shape) < 0.05] = np.inf
    for dtype in WIDTHS + [np.float32]:
        lab = labels_c(ext, dtype, seed=2, zero_frac=0.2, block=4, nlabels=9)
        want = label_stats_oracle.label_stats(lab, dt)
        n = len(want.labels)
        code = CODE[np.dtype(dtype).name]
        cap = 64
        for k_lab, k_dt in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (3 if lab.dtype.itemsize < 8 else 1, 2)):
            _, lview = offset_view(lab, k_lab)
            _, dview = offset_view(dt, k_dt, NAN)
            ws = workspace(L.edt_hip_label_stats_workspace_bytes(code, lab.size, cap))
            keys = torch.zeros(cap, dtype=lview.dtype, device="cuda")
            counts = torch.zeros(cap, dtype=torch.int64, device="cuda")
            mx = torch.zeros(cap, dtype=torch.float32, device="cuda")
            arg = torch.zeros(cap, dtype=torch.int64, device="cuda")
            bbox = torch.zeros((cap, 6), dtype=torch.int32, device="cuda")
            nl = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            ok(L.edt_hip_label_stats_device(vp(lview), code, vp(dview), 3, *ext, cap, vp(keys), vp(counts), vp(mx), vp(arg), vp(bbox),
                                            vp(nl), vp(ws), ws.numel(), stream()))
            sync()
            assert int(nl) == n, (dtype, k_lab, k_dt)
            arg_n = arg[:n].cpu().numpy()
            box = bbox[:n].cpu().numpy()
            got = label_stats_oracle.LabelStats(
                keys[:n].cpu().numpy().view(lab.dtype), counts[:n].cpu().numpy(), mx[:n].cpu().numpy(),
                np.stack(np.unravel_index(arg_n, lab.shape), axis=1).astype(np.int64).reshape(n, 3),
                np.ascontiguousarray(box[:, 0::2][:, ::-1]), np.ascontiguousarray(box[:, 1::2][:, ::-1]))
            label_stats_oracle.assert_same(got, want, (dtype, k_lab, k_dt))


# ---- 9. connected components, fill_holes, dust -----------------------------------------------------------------------------
def component_labels(ext, dtype):
    """independent noise near the percolation threshold: few large, winding components that reach both ends of the volume"""
    rng = np.random.default_rng(ext[0])
    shape = ext[::-1]
    ids = (rng.random(shape) < 0.55) * rng.integers(1, 3, size=shape)
    ids.flat[0] = ids.flat[-1] = 2
    ids.flat[1] = ids.flat[-2] = 2
    return ids.astype(dtype)


CC_OFFSETS = [(np.uint8, 0, 0), (np.uint8, 0, 1), (np.uint8, 0, 2), (np.uint8, 0, 3), (np.uint8, 1, 0), (np.uint8, 3, 1),
              (np.uint16, 1, 2), (np.uint32, 1, 3), (np.uint64, 1, 1)]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("ext", [(65, 12, 9), (64, 12, 9)])
def test_connected_components_on_offset_pointers(ext, c):
    import torch
    L = lib()
    lab8 = component_labels(ext, np.uint8)
    want, wn = components_oracle.connected_components(lab8, c, return_N=True)
    for dtype, k_lab, k_out in CC_OFFSETS:
        lab = lab8.astype(dtype)
        code = CODE[np.dtype(dtype).name]
        _, lview = offset_view(lab, k_lab)
        obuf, oview = out_buffer(lab.shape, np.uint32, k_out)
        n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        ws = workspace(L.edt_hip_components_workspace_bytes(code, 3, *ext))
        ok(L.edt_hip_connected_components_device(vp(lview), code, 3, *ext, c, 0, vp(oview), vp(n), vp(ws), ws.numel(), stream()))
        out_matches(obuf, oview, k_out, want, ("connected_components", ext, c, dtype, k_lab, k_out))
        assert int(n) == wn


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("ext", [(65, 12, 9), (64, 12, 9)])
def test_fill_holes_on_offset_pointers(ext, c):
    import torch
    L = lib()
    rng = np.random.default_rng(ext[0] + c)
    ids = blocky_labels(ext[::-1], nlabels=3, zero_frac=0.0, block=6, rng=rng)
    ids[rng.random(ids.shape) < 0.08] = 0                      # pin-holes: cavities of one wall label and of two
    ids.flat[0] = ids.flat[-1] = 2
    for binary in (0, 1):
        w8 = fill_holes_oracle.fill_holes(ids.astype(np.uint8), c, binary=bool(binary))
        assert w8.n_filled > 0
        for dtype, k_lab, k_out in CC_OFFSETS:
            lab = ids.astype(dtype)
            code = CODE[np.dtype(dtype).name]
            _, lview = offset_view(lab, k_lab)
            obuf, oview = out_buffer(lab.shape, dtype, k_out)
            n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            ws = workspace(L.edt_hip_fill_holes_workspace_bytes(code, 3, *ext))
            ok(L.edt_hip_fill_holes_device(vp(lview), code, 3, *ext, c, binary, vp(oview), vp(n), vp(ws), ws.numel(), stream()))
            out_matches(obuf, oview, k_out, w8.out.astype(dtype).view(f"u{lab.dtype.itemsize}"),
                        ("fill_holes", ext, c, binary, dtype, k_lab, k_out))
            assert int(n) == w8.n_filled


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("ext", [(65, 12, 9), (64, 12, 9)])
def test_dust_on_offset_pointers(ext, c):
    import torch
    from edt import device
    L = lib()
    lab8 = component_labels(ext, np.uint8)
    for threshold, invert in ((4, 0), ((3, 9), 0), ((3, 9), 1)):
        lo, hi = dust_oracle.bounds(threshold)
        w8 = dust_oracle.dust(lab8, threshold, c, invert=bool(invert))
        assert 0 < w8.kept < w8.components
        for dtype, k_lab, k_out in CC_OFFSETS:
            lab = lab8.astype(dtype)
            code = CODE[np.dtype(dtype).name]
            _, lview = offset_view(lab, k_lab)
            obuf, oview = out_buffer(lab.shape, dtype, k_out)
            counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
            ws = workspace(L.edt_hip_dust_workspace_bytes(code, 3, *ext))
            ok(L.edt_hip_dust_device(vp(lview), code, 3, *ext, c, 0, lo, hi, invert, vp(oview), vp(counts), vp(ws), ws.numel(), stream()))
            out_matches(obuf, oview, k_out, w8.out.astype(dtype).view(f"u{lab.dtype.itemsize}"),
                        ("dust", ext, c, threshold, invert, dtype, k_lab, k_out))
            assert counts.tolist() == [w8.components, w8.kept, w8.removed_voxels]
        # in place, on an offset tensor: its surroundings are what offset_view put there, the sentinel of an input
        for dtype, k in ((np.uint8, 1), (np.uint8, 3), (np.uint16, 1), (np.uint32, 1)):
            lab = lab8.astype(dtype)
            buf, view = offset_view(lab, k)
            before = buf.clone()
            out, counts = device.dust(view, threshold, connectivity=c, invert=bool(invert), in_place=True)
            sync()
            assert out.data_ptr() == view.data_ptr()
            assert np.array_equal(bits_of(view), w8.out.astype(dtype).view(f"u{lab.dtype.itemsize}")), ("dust in place", dtype, k)
            assert counts.tolist() == [w8.components, w8.kept, w8.removed_voxels]
            lo_, hi_ = 16 + k, 16 + k + lab.size
            assert torch.equal(buf[:lo_], before[:lo_]) and torch.equal(buf[hi_:], before[hi_:])


# ---- 9b. morphology, local thickness and the medial axis: the compositions ------------------------------------------------------
FIELD_OFFSETS = [(np.uint8, 0, 0), (np.uint8, 1, 0), (np.uint8, 0, 1), (np.uint8, 3, 1), (np.uint16, 1, 3), (np.uint32, 1, 1), (np.uint64, 1, 1)]


def test_field_operations_on_offset_labels_and_outputs(oracle_port):
    """The workspace keeps its alignment, so the fields and masks carved from it are 16-byte aligned while the labels, the
    output, T or the radius are not: the element form of the select and step kernels next to aligned fields.  sx = 33 is no
    multiple of 4.  (The sizes are int64 at offset 1: 8-byte aligned, as their type asks.)"""
    L = lib()
    ext, w = (33, 20, 12), (6.0, 6.0, 30.0)
    lab8 = labels_c(ext, np.uint8, seed=ext[0], zero_frac=0.3, block=4)
    an = w[::-1]
    r = 6.0
    opened, closed = morph_oracle.opening(lab8, r, an, black_border=True), morph_oracle.closing(lab8, r, an)
    assert 0 < np.count_nonzero(opened) < np.count_nonzero(lab8) < np.count_nonzero(closed) < lab8.size
    radii = np.array([6.0, 12.0, 21.0], dtype=np.float64)
    T_want, _, sizes_want = thickness_oracle.local_thickness(lab8, radii, an, black_border=True)
    assert 0 < sizes_want[-1] < sizes_want[0]
    on = medial_oracle.on_axis(lab8, anisotropy=an, black_border=True)
    assert 0 < np.count_nonzero(on) < np.count_nonzero(lab8)
    radius_want = np.where(on, np.sqrt(oracle_port.edtsq(lab8, an, True)), np.float32(0.0)).astype(np.float32)
    for dtype, k_lab, k_out in FIELD_OFFSETS:
        lab = lab8.astype(dtype)
        code = CODE[np.dtype(dtype).name]
        bits = f"u{lab.dtype.itemsize}"
        what = (dtype, k_lab, k_out)
        _, lview = offset_view(lab, k_lab)
        for op, flags, want in ((2, 1, opened), (3, 0, closed)):
            obuf, oview = out_buffer(lab.shape, dtype, k_out)
            ws = workspace(L.edt_hip_morphology_workspace_bytes(code, 3, *ext, op, flags))
            ok(L.edt_hip_morphology_device(vp(lview), code, 3, *ext, *w, op, r, flags, vp(oview), vp(ws), ws.numel(), stream()))
            out_matches(obuf, oview, k_out, want.astype(dtype).view(bits), ("morphology", op) + what)
        tbuf, tview = out_buffer(lab.shape, np.float32, k_out)
        sbuf, sview = out_buffer((radii.size,), np.int64, 1)
        n_used = ctypes.c_int64(-1)
        ws = workspace(L.edt_hip_local_thickness_workspace_bytes(code, 3, *ext, 1))
        ok(L.edt_hip_local_thickness_device(vp(lview), code, 3, *ext, *w, 1, ctypes.c_void_p(radii.ctypes.data), radii.size, 0.0, vp(tview),
                                            vp(sview), ctypes.byref(n_used), vp(ws), ws.numel(), stream()))
        out_matches(tbuf, tview, k_out, f32_bits(T_want), ("local_thickness",) + what)
        out_matches(sbuf, sview, 1, sizes_want.view(np.uint64), ("local_thickness sizes",) + what)
        assert n_used.value == radii.size
        obuf, oview = out_buffer(lab.shape, dtype, k_out)
        rbuf, rview = out_buffer(lab.shape, np.float32, (k_out + 1) % 4)
        ws = workspace(L.edt_hip_medial_axis_workspace_bytes(code, 3, *ext, 1, 1))
        ok(L.edt_hip_medial_axis_device(vp(lview), code, 3, *ext, *w, 1, float(max(w)), 0.0, vp(oview), vp(rview), vp(ws), ws.numel(),
                                        stream()))
        out_matches(obuf, oview, k_out, np.where(on, lab, np.zeros((), dtype)).astype(dtype).view(bits), ("medial_axis",) + what)
        out_matches(rbuf, rview, (k_out + 1) % 4, f32_bits(radius_want), ("medial_axis radius",) + what)


# ---- 10. the sharded phases ------------------------------------------------------------------------------------------------
def test_shard_phases_with_an_offset_partial_field(oracle_port):
    """edt_hip_shard_xy_device and edt_hip_shard_z_device as ONE virtual rank (tests/test_gpu_paths.py drives several): the fp32
    field between them, and the labels, at an element offset"""
    import torch
    L = lib()
    ext = (64, 40, 33)
    lab = labels_c(ext, np.uint32, seed=33, block=6)
    n = lab.size
    for w, bb in (((6.0, 6.0, 30.0), True), ((1.1, 0.7, 1.3), False)):
        want = oracle_port.edtsq(lab, w[::-1], bb)
        flags = 1 if bb else 0
        for k_lab, k_partial in ((0, 0), (0, 1), (1, 1), (0, 2), (0, 3)):
            _, lview = offset_view(lab, k_lab)
            pbuf, partial = out_buffer(lab.shape, np.float32, k_partial)
            zflags = torch.empty(lab.shape, dtype=torch.uint8, device="cuda")
            ws = workspace(max(L.edt_hip_shard_workspace_bytes(U32, *ext), L.edt_hip_shard_workspace_bytes(U8, *ext)))
            ok(L.edt_hip_shard_xy_device(vp(lview), None, U32, *ext, w[0], w[1], flags, vp(partial), vp(zflags), vp(ws), ws.numel(),
                                         stream()))
            sync()
            assert outside_intact(pbuf, k_partial, n, NAN), ("shard xy", w, k_lab, k_partial)
            ok(L.edt_hip_shard_z_device(vp(partial), vp(zflags), *ext, w[2], flags, vp(ws), ws.numel(), stream()))
            out_matches(pbuf, partial, k_partial, f32_bits(want), ("shard z", w, bb, k_lab, k_partial))


def test_record_forms_refuse_a_block_at_a_4_byte_offset():
    """include/edt_hip.h documents 8- and 16-byte requirements for the blocks of the slab records: refused with EDT_ERR_BAD_ARG
    before any launch (the blocks keep their sentinel)"""
    import torch
    L = lib()
    ext = (64, 96, 8)
    w = (6.0, 6.0, 30.0)
    lab = torch.ones(ext[::-1], dtype=torch.int32, device="cuda")
    splits = (ctypes.c_int64 * 2)(0, ext[1])
    ws = workspace(L.edt_hip_shard_records_workspace_bytes(U32, *ext))
    # fp32 records, rows of whole granules: 16 bytes
    words = int(L.edt_hip_shard_record_floats(ext[0], ext[1])) * ext[2]
    block = torch.full((words + 4,), -7, dtype=torch.int32, device="cuda")
    ptrs = (ctypes.c_void_p * 1)(block.data_ptr() + 4)
    rc = L.edt_hip_shard_xy_records_device(vp(lab), None, U32, *ext, w[0], w[1], 1, 1, splits, ptrs, vp(ws), ws.numel(), stream())
    sync()
    assert rc == BAD_ARG and b"16-byte" in L.edt_hip_last_error() and bool((block == -7).all())
    # records of 16-bit rows: 8 bytes for the blocks of the XY phase, 16 for the gathered records and the output of the Z phase
    assert L.edt_hip_shard_records16_supported(U32, 64, 128, 128, *w) == 1
    ext16 = (64, 128, 128)
    lab16 = torch.ones(ext16[::-1], dtype=torch.int32, device="cuda")
    splits16 = (ctypes.c_int64 * 2)(0, ext16[1])
    ws16 = workspace(max(L.edt_hip_shard_records_workspace_bytes(U32, *ext16), L.edt_hip_shard_records_workspace_bytes(U8, *ext16)))
    words16 = int(L.edt_hip_shard_record16_words(ext16[0], ext16[1])) * ext16[2]
    block16 = torch.full((words16 + 4,), -7, dtype=torch.int32, device="cuda")
    refused = torch.zeros(1, dtype=torch.int32, device="cuda")
    ptrs16 = (ctypes.c_void_p * 1)(block16.data_ptr() + 4)
    rc = L.edt_hip_shard_xy_records16_device(vp(lab16), None, U32, *ext16, *w, 1, 1, splits16, ptrs16, vp(refused), vp(ws16),
                                             ws16.numel(), stream())
    sync()
    assert rc == BAD_ARG and b"8-byte" in L.edt_hip_last_error() and bool((block16 == -7).all())
    out = torch.full((lab16.numel() + 4,), -7, dtype=torch.int32, device="cuda")
    for rec_off, out_off in ((4, 0), (0, 4)):
        rc = L.edt_hip_shard_z_records16_device(ctypes.c_void_p(block16.data_ptr() + rec_off), ctypes.c_void_p(out.data_ptr() + out_off),
                                                *ext16, *w, 1, vp(ws16), ws16.numel(), stream())
        sync()
        assert rc == BAD_ARG and b"16-byte" in L.edt_hip_last_error() and bool((out == -7).all()), (rec_off, out_off)


# ---- 11. the Python layer: z-slabs of a uint8 volume whose slices hold an odd number of voxels ---------------------------------
def test_python_layer_on_z_slabs_at_odd_addresses(oracle_port):
    import torch
    from edt import device
    from test_gpu_extras import _CudaArrayInterfaceOnly
    rng = np.random.default_rng(21)
    vol = blocky_labels((8, 15, 21), nlabels=4, zero_frac=0.2, block=3, rng=rng).astype(np.uint8)
    vol[2] = vol[3]                       # (the slice below the slab holds the slab's own first labels)
    field = (rng.integers(-3, 4, size=vol.shape).astype(np.float32) * np.float32(0.75))
    t, dt = torch.from_numpy(vol).cuda(), torch.from_numpy(field).cuda()
    slab, dslab = t[3:], dt[3:]
    assert slab.is_contiguous() and slab.data_ptr() % 2 == 1 and dslab.data_ptr() % 16 == 4
    sub = vol[3:]
    want = oracle_port.edtsq(sub, (1.0, 1.0, 1.0), False)
    assert np.array_equal(device.edtsq(slab).cpu().numpy(), want)
    wrapped = _CudaArrayInterfaceOnly(slab, "|u1")
    assert wrapped.__cuda_array_interface__["data"][0] == slab.data_ptr()
    assert np.array_equal(device.edtsq(wrapped).cpu().numpy(), want)
    for c in (1, 3):
        out, n = device.connected_components(slab, connectivity=c)
        wc, wn = components_oracle.connected_components(sub, c, return_N=True)
        assert int(n) == wn and np.array_equal(out.cpu().numpy().view(np.uint32), wc)
    got = label_stats_oracle.LabelStats(*[x.cpu().numpy() for x in device.label_stats(slab, dslab)])
    label_stats_oracle.assert_same(got, label_stats_oracle.label_stats(sub, field[3:]), "label_stats of a z-slab")
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), vol) and np.array_equal(dt.cpu().numpy().view(np.uint32), field.view(np.uint32))


# ---- the host-buffer ABI -------------------------------------------------------------------------------------------------------
def test_host_buffers_at_an_element_offset(oracle_port):
    L = lib()
    ext = (40, 24, 33)
    lab = labels_c(ext, np.uint8, seed=4)
    n = lab.size
    for dtype in (np.uint8, np.uint16):
        big = np.full(n + 8, 3, dtype=dtype)
        big[1:1 + n] = lab.reshape(-1)
        big[0], big[1 + n:] = lab.flat[0], lab.flat[-1]
        for w, bb in (((6.0, 6.0, 30.0), True), ((0.7, 1.3, 2.1), False)):
            want = oracle_port.edtsq(lab, w[::-1], bb)
            out = np.full(n + 8, NAN, dtype=np.uint32)
            labels_ptr = ctypes.c_void_p(big.ctypes.data + big.itemsize)
            out_ptr = ctypes.c_void_p(out.ctypes.data + 4)
            ok(L.edt_hip_edt3dsq(labels_ptr, CODE[np.dtype(dtype).name], *ext, *w, 1 if bb else 0, 1, out_ptr))
            assert np.array_equal(out[1:1 + n], want.reshape(-1).view(np.uint32)), (dtype, w, bb)
            assert out[0] == NAN and np.all(out[1 + n:] == NAN)


# ---- a misaligned workspace is refused before any launch -----------------------------------------------------------------------
def test_misaligned_workspace_is_refused_by_every_device_entry_point():
    """d_workspace = base + 4 with enough bytes behind it: EDT_ERR_BAD_ARG from every entry point that takes a workspace, the
    outputs untouched.  (No case lets a misaligned workspace reach a kernel: the refusal is what is tested.)"""
    import torch
    L = lib()
    ext = (64, 40, 33)
    n = ext[0] * ext[1] * ext[2]
    lab = torch.ones(ext[::-1], dtype=torch.uint8, device="cuda")
    lab32 = torch.ones(ext[::-1], dtype=torch.int32, device="cuda")
    fill = -7

    def out(dtype, count=n):
        return torch.full((count,), fill, dtype=dtype, device="cuda")

    def refused(rc, *outs):
        sync()
        assert rc == BAD_ARG and b"256-byte aligned" in L.edt_hip_last_error(), (rc, L.edt_hip_last_error())
        for o in outs:
            assert bool((o == fill).all())

    def ws_at_4(nbytes):
        ws = workspace(nbytes + 256)
        return ctypes.c_void_p(ws.data_ptr() + 4), int(nbytes), ws

    f, i64 = out(torch.float32), out(torch.int64, 3)
    p, nb, keep = ws_at_4(L.edt_hip_workspace_bytes(U8, 3, *ext))
    refused(L.edt_hip_edtsq_device(vp(lab), U8, 3, *ext, 1.0, 1.0, 1.0, 0, vp(f), p, nb, stream()), f)
    p, nb, keep = ws_at_4(L.edt_hip_workspace_bytes(U8, 1, n, 1, 1))
    refused(L.edt_hip_edtsq_device(vp(lab), U8, 1, n, 1, 1, 1.0, 1.0, 1.0, 0, vp(f), p, nb, stream()), f)
    p, nb, keep = ws_at_4(L.edt_hip_voxel_graph_workspace_bytes(3, *ext))
    refused(L.edt_hip_edtsq_voxel_graph_device(vp(lab), U8, vp(lab), 3, *ext, 1.0, 1.0, 1.0, 0, vp(f), p, nb, stream()), f)
    p, nb, keep = ws_at_4(L.edt_hip_runs_workspace_bytes(n))
    refused(L.edt_hip_extract_runs_device(vp(lab), U8, n, None, 0, vp(i64), p, nb, stream()), i64)
    o32 = out(torch.int32, 3 * n)
    p, nb, keep = ws_at_4(L.edt_hip_feature_workspace_bytes(U8, 3, *ext, 0))
    refused(L.edt_hip_feature_transform_device(vp(lab), U8, 3, *ext, 1.0, 1.0, 1.0, 0, vp(o32), p, nb, stream()), o32)
    o8 = out(torch.int8)
    p, nb, keep = ws_at_4(L.edt_hip_expand_labels_workspace_bytes(U8, 3, *ext))
    refused(L.edt_hip_expand_labels_device(vp(lab), U8, 3, *ext, 1.0, 1.0, 1.0, 1.0, vp(o8), p, nb, stream()), o8)
    p, nb, keep = ws_at_4(L.edt_hip_label_stats_workspace_bytes(U8, n, 16))
    tab = [out(torch.int8, 16), out(torch.int64, 16), out(torch.float32, 16), out(torch.int64, 16), out(torch.int32, 96)]
    refused(L.edt_hip_label_stats_device(vp(lab), U8, vp(f), 3, *ext, 16, *[vp(t) for t in tab], vp(i64), p, nb, stream()), i64, *tab)
    p, nb, keep = ws_at_4(L.edt_hip_components_workspace_bytes(U8, 3, *ext))
    refused(L.edt_hip_connected_components_device(vp(lab), U8, 3, *ext, 1, 0, vp(o32), vp(i64), p, nb, stream()), o32, i64)
    p, nb, keep = ws_at_4(L.edt_hip_fill_holes_workspace_bytes(U8, 3, *ext))
    refused(L.edt_hip_fill_holes_device(vp(lab), U8, 3, *ext, 1, 0, vp(o8), vp(i64), p, nb, stream()), o8, i64)
    p, nb, keep = ws_at_4(L.edt_hip_dust_workspace_bytes(U8, 3, *ext))
    refused(L.edt_hip_dust_device(vp(lab), U8, 3, *ext, 1, 0, 2, (1 << 63) - 1, 0, vp(o8), vp(i64), p, nb, stream()), o8, i64)
    # the compositions of the field operations
    for op in (0, 1, 2, 3):
        p, nb, keep = ws_at_4(L.edt_hip_morphology_workspace_bytes(U8, 3, *ext, op, 0))
        refused(L.edt_hip_morphology_device(vp(lab), U8, 3, *ext, 1.0, 1.0, 1.0, op, 2.0, 0, vp(o8), p, nb, stream()), o8)
    radii = np.array([1.0, 2.0], dtype=np.float64)
    n_used = ctypes.c_int64(fill)
    p, nb, keep = ws_at_4(L.edt_hip_local_thickness_workspace_bytes(U8, 3, *ext, 0))
    refused(L.edt_hip_local_thickness_device(vp(lab), U8, 3, *ext, 1.0, 1.0, 1.0, 0, ctypes.c_void_p(radii.ctypes.data), 2, 0.0, vp(f),
                                             vp(i64), ctypes.byref(n_used), p, nb, stream()), f, i64)
    assert n_used.value == fill
    p, nb, keep = ws_at_4(L.edt_hip_medial_axis_workspace_bytes(U8, 3, *ext, 0, 1))
    refused(L.edt_hip_medial_axis_device(vp(lab), U8, 3, *ext, 1.0, 1.0, 1.0, 0, 1.0, 0.0, vp(o8), vp(f), p, nb, stream()), o8, f)
    # the sharded phases
    z8 = out(torch.int8)
    p, nb, keep = ws_at_4(L.edt_hip_shard_workspace_bytes(U8, *ext))
    refused(L.edt_hip_shard_xy_device(vp(lab), None, U8, *ext, 1.0, 1.0, 0, vp(f), vp(z8), p, nb, stream()), f, z8)
    refused(L.edt_hip_shard_z_device(vp(f), vp(z8), *ext, 1.0, 0, p, nb, stream()), f)
    ext_r = (64, 96, 8)
    w = (6.0, 6.0, 30.0)
    labr = lab32[:ext_r[2], :ext_r[1], :].contiguous()
    words = int(L.edt_hip_shard_record_floats(ext_r[0], ext_r[1])) * ext_r[2]
    block = out(torch.int32, words)
    splits = (ctypes.c_int64 * 2)(0, ext_r[1])
    ptrs = (ctypes.c_void_p * 1)(block.data_ptr())
    p, nb, keep = ws_at_4(max(L.edt_hip_shard_records_workspace_bytes(U32, *ext_r), L.edt_hip_shard_records_workspace_bytes(U8, *ext_r)))
    refused(L.edt_hip_shard_xy_records_device(vp(labr), None, U32, *ext_r, w[0], w[1], 1, 1, splits, ptrs, p, nb, stream()), block)
    refused(L.edt_hip_shard_z_records_device(vp(block), *ext_r, w[2], 1, p, nb, stream()), block)
    refused(L.edt_hip_shard_z_records_device_ex(vp(block), *ext_r, w[2], 0.0, 1, p, nb, stream()), block)
    refused(L.edt_hip_shard_z_records_device_w(vp(block), *ext_r, *w, 1, p, nb, stream()), block)
    ext16 = (64, 128, 128)
    lab16 = torch.ones(ext16[::-1], dtype=torch.int32, device="cuda")
    block16 = out(torch.int32, int(L.edt_hip_shard_record16_words(ext16[0], ext16[1])) * ext16[2])
    splits16 = (ctypes.c_int64 * 2)(0, ext16[1])
    ptrs16 = (ctypes.c_void_p * 1)(block16.data_ptr())
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    f16 = out(torch.float32, lab16.numel())
    p, nb, keep = ws_at_4(max(L.edt_hip_shard_records_workspace_bytes(U32, *ext16), L.edt_hip_shard_records_workspace_bytes(U8, *ext16)))
    refused(L.edt_hip_shard_xy_records16_device(vp(lab16), None, U32, *ext16, *w, 1, 1, splits16, ptrs16, vp(cnt), p, nb, stream()), block16)
    refused(L.edt_hip_shard_z_records16_device(vp(block16), vp(f16), *ext16, *w, 1, p, nb, stream()), block16, f16)
    assert keep is not None
