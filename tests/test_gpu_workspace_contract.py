"""GPU tier: every device entry point that takes a WORKSPACE is held to the scratch and stream half of the device ABI
(include/edt_hip.h, "Workspace"): the call initialises whatever it reads of its scratch -- a reused, dirty buffer needs no
memset, and one buffer of the largest size serves calls of every flag set --, and it only enqueues work on the caller's stream
(no allocation, no synchronisation: capturable).  DESIGN.md section 13 has the region table this module tests: every carve,
who writes each region before anyone reads it, and which writes a call skips.

Raw ABI calls through edt._lib, as in tests/test_gpu_offset_pointers.py: outputs are prefilled with that file's sentinels (a NaN
with a payload, 0xA5..), expectations come from oracle_port and the numpy oracles of tests/ -- for the sharded phases the
intermediate records too, built here from the oracle's 2-D transforms -- and are compared bit for bit, no tolerances.

Four stages, named so that they can be selected (-k zero_fill / residue / pattern_fill / capture):
  zero_fill     the workspace zeroed before every call, two calls: the contract's easy half, and the stage that runs first;
  residue       the realistic dirt.  One buffer per extent, as large as the largest route needs, shared by all routes and never
                cleared; two label volumes per extent, so that what a call finds is always ANOTHER volume's planes, counters,
                map and index buffer.  Every ordered pair (route A, then route B) of the transform on (64, 100, 100); on
                (528, 130, 100), where tiles leave 16 bits, a refusing call before a shallow one and the reverse; long rows, a
                1-D line and an axis beyond the wave kernels after other routes; every other entry point after the first route
                and after its own call on other labels;
  pattern_fill  0xFF, 0x5A, 0x80 bytes and FLT_MAX words (the value the kernels take as +inf), two calls each;
  capture       warm-up, capture on a side stream, three replays with the workspace refilled differently and the outputs reset
                before each: a launch on the wrong stream, a hidden allocation or synchronisation, or an initialisation done by
                the host at call time would show.

The pass log tells the fused and the unfused signed route apart, the host's own proof the integer-only route, and the carve
sizes the routes whose regions shift: a route that collapsed onto another would test nothing.

What the capture stage found: a stream-side memset does not replay from a graph as the memset it was, so every
word a call sets on its stream is now set by a kernel of the call -- which is why fill_holes, dust and the calls on empty
volumes, whose counts are zeroed that way, run through the four stages here as well."""
import ctypes
import math

import numpy as np
import pytest

import dust_oracle
import fill_holes_oracle
import label_stats_oracle
import medial_oracle
import morph_oracle
import thickness_oracle
from synth import _signed_bits, bits_of, blocky_labels, box_edtsq_closed_form
from test_gpu_offset_pointers import MARK, NAN, U8, U16, U32, component_labels, f32_bits, ft_want, labels_c, lib, ok, stream, sync, vp
from test_gpu_q16 import slab_labels

pytestmark = pytest.mark.gpu

FLT_MAX_BITS = 0x7F7FFFFF
FLAG_BB, FLAG_SQRT, FLAG_GENERIC, FLAG_BATCH, FLAG_SMALL, FLAG_BINARY, FLAG_SIGNED = 1, 2, 4, 8, 16, 32, 64
FILLS = ["00", "ff", "5a", "80", "fltmax"]
DIRTY = FILLS[1:]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    from edt import _lib
    _lib.load()
    if not torch.cuda.is_available() or _lib.device_count() == 0:
        pytest.fail("the GPU tier needs a HIP device")
    torch.cuda.set_device(0)


# ---- buffers ---------------------------------------------------------------------------------------------------------------
def fill(ws, pattern):
    """every byte of the workspace 0x00 / 0xFF / 0x5A / 0x80, or every 32-bit word FLT_MAX"""
    import torch
    if pattern == "fltmax":
        ws.view(torch.int32).fill_(FLT_MAX_BITS)
    else:
        ws.fill_(int(pattern, 16))


def round256(nbytes):
    assert nbytes > 0
    return (int(nbytes) + 255) // 256 * 256


_shared = {}


def shared_workspace(key, nbytes):
    """THE buffer of an extent: allocated once at the largest size asked for, handed to every call, never cleared"""
    import torch
    have = _shared.get(key)
    if have is None or have.numel() < nbytes:
        assert have is None, (key, "sized before its first use", have.numel(), nbytes)
        have = _shared[key] = torch.empty(round256(nbytes), dtype=torch.uint8, device="cuda")
    return have


def fresh_workspace(nbytes):
    import torch
    return torch.empty(round256(nbytes), dtype=torch.uint8, device="cuda")


def sentinel_fill(t):
    import torch
    size = t.element_size()
    itype = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[size]
    t.view(itype).fill_(_signed_bits(NAN if t.dtype.is_floating_point else MARK[size], size))


def device_out(shape, dtype):
    """an output tensor of a numpy dtype (unsigned types as the signed type of their width), holding the sentinel"""
    import torch
    name = {"uint8": "uint8", "uint16": "int16", "uint32": "int32", "uint64": "int64", "int32": "int32", "int64": "int64",
            "float32": "float32"}[np.dtype(dtype).name]
    t = torch.empty(shape, dtype=getattr(torch, name), device="cuda")
    sentinel_fill(t)
    return t


def upload(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u" and a.dtype.itemsize > 1:
        a = a.view(f"i{a.dtype.itemsize}")
    return torch.from_numpy(a.copy()).cuda()


def equal_bits(t, want_bits, what):
    got = bits_of(t).reshape(-1)
    want_bits = np.ascontiguousarray(want_bits).reshape(-1)
    assert got.dtype == want_bits.dtype and got.shape == want_bits.shape, (what, got.dtype, want_bits.dtype, got.shape, want_bits.shape)
    assert np.array_equal(got, want_bits), (what, "mismatches", int((got != want_bits).sum()))


class Case:
    """One raw ABI call on device-resident inputs: reset() puts the sentinel into its outputs (and restores an input the call
    works on in place), call(ws) enqueues it on the current stream with `ws` as its workspace, check() compares with the oracle."""

    def __init__(self, name, nbytes, call, check, outputs=(), restore=None):
        self.name, self.nbytes, self.call, self._check, self.outputs, self.restore = name, int(nbytes), call, check, outputs, restore

    def reset(self):
        for t in self.outputs:
            sentinel_fill(t)
        if self.restore is not None:
            self.restore()

    def check(self, what):
        sync()
        self._check((self.name, what))


def two_calls(case, ws, what, pattern=None):
    """(the workspace filled,) the outputs reset, the call, the comparison -- twice"""
    for nth in (1, 2):
        if pattern is not None:
            fill(ws, pattern)
        case.reset()
        case.call(ws)
        case.check((what, pattern, "call", nth))


def capture_and_replay(case, ws, patterns=("ff", "fltmax", "5a")):
    import torch
    fill(ws, "00")
    case.reset()
    case.call(ws)                                   # warm-up: lazy code-object loads, function attributes
    case.check("warm-up")
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            case.call(ws)
    for pattern in patterns:
        fill(ws, pattern)
        case.reset()
        graph.replay()
        case.check(("replay", pattern))


# ---- the transform: routes on (64, 100, 100) -----------------------------------------------------------------------------------
EXT = (64, 100, 100)
W630, W111, WF = (6.0, 6.0, 30.0), (1.0, 1.0, 1.0), (0.7, 1.3, 2.1)
# (name, volumes, voxel sizes, black border, flags, debug mode, the oracle's function)
ROUTES = [
    ("integer only", "blocky", W630, 1, 0, 0, "edtsq"),                 # skip_nz, counters not zeroed, the 16-bit plane
    ("tiles of +inf", "slab", W111, 0, 0, 0, "edtsq"),                  # plane_inf_ok, the all-+inf shortcut, wide tiles
    ("no quantum", "blocky", WF, 0, 0, 0, "edtsq"),                     # the fp32 kernels: every plane written and read
    ("signed, fused", "blocky", W630, 1, FLAG_SIGNED, 0, "sdfsq"),      # true label bits in the foreground planes
    ("signed, sign pass", "blocky", W630, 1, FLAG_SIGNED, 0x400, "sdfsq"),
    ("binary yz", "blocky", W630, 1, FLAG_BINARY, 0, "binary"),
    ("stack of images", "blocky", W630, 1, FLAG_BATCH, 0, "stack"),     # another carve: no z planes
    ("forced generic", "blocky", W630, 1, FLAG_GENERIC, 0, "edtsq"),    # bufB / stack first: every region shifts
    ("small workspace", "blocky", W630, 1, FLAG_SMALL, 0, "edtsq"),     # no index buffer
    ("sqrt", "blocky", W630, 1, FLAG_SQRT, 0, "edt"),
    ("phased rows", "blocky", W630, 1, 0, 32, "edtsq"),
    ("phased columns", "slab", W111, 0, 0, 64, "edtsq"),
    ("fp32 pass X", "blocky", W630, 1, 0, 0x100000, "edtsq"),
    ("fp32 between Y and Z", "slab", W111, 0, 0, 0x10000000, "edtsq"),
    ("no integer kernel", "blocky", W630, 1, 0, 0x8000000, "edtsq"),
]
ROUTE_IDS = [r[0].replace(" ", "_").replace(",", "").replace("+", "") for r in ROUTES]
_volumes, _wants, _device = {}, {}, {}


def volume(kind, v, ext=EXT):
    """label volume v (0 / 1) of a kind, C-ordered uint8: different objects, v = 1 of "blocky" with ~45 % background"""
    key = (kind, v, ext)
    if key not in _volumes:
        if kind == "blocky":
            lab = labels_c(ext, np.uint8, seed=sum(ext) + 7 * v, zero_frac=0.45 if v else 0.2, block=5 + 2 * v)
        elif kind == "slab":
            lab = np.ascontiguousarray(slab_labels(ext, np.random.default_rng(sum(ext) + v)).T).astype(np.uint8)
            if v:                                             # (one more object in a corner: other planes, another map)
                corner = lab[:ext[2] // 3, :ext[1] // 3, :]
                corner[corner == 1] = 4
        else:
            raise KeyError(kind)
        _volumes[key] = lab
    return _volumes[key]


def device_labels(kind, v, ext=EXT):
    key = (kind, v, ext)
    if key not in _device:
        _device[key] = upload(volume(kind, v, ext))
    return _device[key]


def slices_after_xy(oracle_port, lab, wx, wy, bb):
    """the field after passes X and Y: the 2-D transform of every slice, with FLT_MAX (tofinite, src/edt.hpp:39-45) where a
    column pass that follows still has to find a boundary"""
    out = np.stack([oracle_port.edtsq(lab[z], (wy, wx), bool(bb)) for z in range(lab.shape[0])]).astype(np.float32)
    out[np.isinf(out)] = np.float32(np.finfo(np.float32).max)
    return out


def route_want(oracle_port, route, v):
    name, kind, w, bb, flags, mode, fn = route
    key = (kind, v, w, bb, fn)
    if key not in _wants:
        lab = volume(kind, v)
        if fn in ("edtsq", "edt"):
            sq = _wants.get((kind, v, w, bb, "edtsq"))
            if sq is None:
                sq = _wants[(kind, v, w, bb, "edtsq")] = oracle_port.edtsq(lab, w[::-1], bool(bb))
            _wants[key] = sq if fn == "edtsq" else np.sqrt(sq)
        elif fn == "sdfsq":
            _wants[key] = oracle_port.sdfsq(lab, w[::-1], bool(bb))
            assert (_wants[key] < 0).any() and (_wants[key] > 0).any()
        elif fn == "binary":
            _wants[key] = oracle_port.binary_edtsq(lab, w[::-1], bool(bb))
        elif fn == "stack":
            assert bb                                          # (a last pass: +inf would stay +inf)
            _wants[key] = slices_after_xy(oracle_port, lab, w[0], w[1], bb)
    return _wants[key]


def with_mode(mode, fn):
    L = lib()
    L.edt_hip_set_debug_mode(mode)
    try:
        return fn()
    finally:
        L.edt_hip_set_debug_mode(0)


def route_bytes(route, ext=EXT, ndim=3):
    """edt_hip_workspace_bytes_flags for the route's flags, asked under the route's debug mode"""
    nbytes = with_mode(route[5], lambda: lib().edt_hip_workspace_bytes_flags(U8, ndim, *ext, route[4] & ~FLAG_SQRT))
    assert nbytes > 0
    return int(nbytes)


def transform_buffer():
    return shared_workspace(EXT, max(route_bytes(r) for r in ROUTES))


_outs = {}


def transform_out(ext=EXT):
    if ext not in _outs:
        _outs[ext] = device_out(ext[::-1], np.float32)
    return _outs[ext]


def run_route(route, v, ws, out):
    """the route's call on its label volume v, enqueued: outputs reset first"""
    name, kind, w, bb, flags, mode, fn = route
    labels = device_labels(kind, v)
    sentinel_fill(out)
    with_mode(mode, lambda: ok(lib().edt_hip_edtsq_device(vp(labels), U8, 3, *EXT, *w, flags | (FLAG_BB if bb else 0), vp(out), vp(ws),
                                                          ws.numel(), stream())))


def route_case(oracle_port, route, v):
    name, kind, w, bb, flags, mode, fn = route
    want = f32_bits(route_want(oracle_port, route, v))
    labels, out = device_labels(kind, v), transform_out()

    def call(ws):
        with_mode(mode, lambda: ok(lib().edt_hip_edtsq_device(vp(labels), U8, 3, *EXT, *w, flags | (FLAG_BB if bb else 0), vp(out),
                                                              vp(ws), ws.numel(), stream())))
    return Case(("edtsq_device", name, v), route_bytes(route), call, lambda what: equal_bits(out, want, what), outputs=(out,))


def test_zero_fill_transform_routes(oracle_port):
    ws = transform_buffer()
    for route in ROUTES:
        for v in (0, 1):
            two_calls(route_case(oracle_port, route, v), ws, "zero fill", "00")


def test_residue_routes_differ():
    """a route that silently collapses onto another tests nothing: the integer-only route is the one the library's own proof
    names, the signed routes are told apart by the pass log (next test), and the routes whose regions shift ask for a
    different carve"""
    L = lib()
    py, pz = ctypes.c_int(0), ctypes.c_int(0)
    assert L.edt_hip_q16_no_refusals(*EXT, *W630, 3, 1, ctypes.byref(py), ctypes.byref(pz)) == 1 and py.value == 1 and pz.value == 1
    assert L.edt_hip_q16_no_refusals(*EXT, *WF, 3, 0, ctypes.byref(py), ctypes.byref(pz)) == 0       # no quantum: fp32 kernels
    assert L.edt_hip_signed_supported(U8, 3, *EXT, 0) == 1
    size = {r[0]: route_bytes(r) for r in ROUTES}
    base = size["integer only"]
    voxels = EXT[0] * EXT[1] * EXT[2]
    assert size["forced generic"] >= base - 2 * voxels + 8 * voxels - 65536       # bufB and the stacks, no index buffer
    assert size["small workspace"] <= base - 2 * voxels + 4096                    # no index buffer
    assert size["fp32 pass X"] <= base - 2 * voxels + 4096
    assert size["phased rows"] <= base - 2 * voxels + 4096
    assert size["stack of images"] < base                                          # no z planes
    assert size["signed, fused"] == size["signed, sign pass"] == size["no quantum"] == base
    assert transform_buffer().numel() >= max(size.values())


def test_residue_pass_log_tells_the_signed_routes_apart(oracle_port):
    from edt import device
    ws, out = transform_buffer(), transform_out()
    names = {}
    for route in ROUTES:
        if route[4] & FLAG_SIGNED or route[0] == "integer only":
            device.set_profiling(True)
            try:
                run_route(route, 1, ws, out)
                sync()
                names[route[0]] = [n for n, _ in device.pass_times()]
            finally:
                device.set_profiling(False)
            equal_bits(out, f32_bits(route_want(oracle_port, route, 1)), (route[0], "profiled"))
    assert "sign" not in names["signed, fused"] and "sign" in names["signed, sign pass"], names
    assert names["signed, fused"] == names["integer only"] == ["x_pass", "y_pass", "z_bits", "z_pass"], names


def names_of_the_route(route):
    """the pass log a call must leave, from the library's host query (edt_hip_transform_route) alone"""
    import test_transform_routes_cpu as table
    name, kind, w, bb, flags, mode, fn = route
    a = table.answers(lib(), [table.case(U8, 3, EXT, w, flags | (FLAG_BB if bb else 0), mode=mode)])[0]
    assert a[0] == 0, (name, a)
    r = dict(zip(table.FIELDS, a[2:]))
    assert r["slabs"] == 1, (name, r)                       # (several slabs would be one "xy_pass")
    names = ["x_pass"] + (["y_bits"] if r["planes_from_labels"] else []) + ["y_pass"]
    names += ["z_bits", "z_pass"] if r["z_pass"] else []
    return names + (["sign"] if r["sign"] == 2 else [])


@pytest.mark.parametrize("r", range(len(ROUTES)), ids=ROUTE_IDS)
def test_residue_pass_log_is_the_one_the_route_names(oracle_port, r):
    """what ran is what the host said would run -- and a column pass that left its route would have failed the call"""
    from edt import device
    route = ROUTES[r]
    ws, out = transform_buffer(), transform_out()
    want_names = names_of_the_route(route)
    device.set_profiling(True)
    try:
        run_route(route, 1, ws, out)
        sync()
        names = [n for n, _ in device.pass_times()]
    finally:
        device.set_profiling(False)
    assert names == want_names, (route[0], names, want_names)
    equal_bits(out, f32_bits(route_want(oracle_port, route, 1)), (route[0], "profiled against its route"))


@pytest.mark.parametrize("b", range(len(ROUTES)), ids=ROUTE_IDS)
def test_residue_every_route_after_every_route(oracle_port, b):
    """route A on volume 0, then route B on volume 1, on one buffer that nobody clears: B's result is the oracle's"""
    ws, out = transform_buffer(), transform_out()
    want = f32_bits(route_want(oracle_port, ROUTES[b], 1))
    for a, route_a in enumerate(ROUTES):
        run_route(route_a, 0, ws, out)
        run_route(ROUTES[b], 1, ws, out)
        sync()
        equal_bits(out, want, ("after", route_a[0], "route", ROUTES[b][0]))
    # ... and volume 0 after volume 1 (the same route: its own planes, counters and map of the other volume)
    run_route(ROUTES[b], 0, ws, out)
    sync()
    equal_bits(out, f32_bits(route_want(oracle_port, ROUTES[b], 0)), ("after itself", ROUTES[b][0]))


@pytest.mark.parametrize("r", range(len(ROUTES)), ids=ROUTE_IDS)
def test_pattern_fill_transform_routes(oracle_port, r):
    ws = transform_buffer()
    for pattern in DIRTY:
        two_calls(route_case(oracle_port, ROUTES[r], 1), ws, "pattern fill", pattern)


@pytest.mark.parametrize("r", [0, 2, 3], ids=[ROUTE_IDS[0], ROUTE_IDS[2], ROUTE_IDS[3]])
def test_capture_transform_routes(oracle_port, r):
    capture_and_replay(route_case(oracle_port, ROUTES[r], 0), transform_buffer())


# ---- the transform where tiles leave 16 bits: (528, 130, 100) --------------------------------------------------------------------
DEEP_EXT = (528, 130, 100)
DEEP_MODES = [0, 0x20000000, 0x40000000]          # default / no wide form: every list launched / whole tiles wide
_deep = {}


def deep_volumes(oracle_port):
    """(labels on the device, voxel sizes, black border, the expectation's bits) of: one label from edge to edge (x-distances of
    up to 264 voxels: 264^2 > 65535), a deep blocky volume, a shallow one"""
    if not _deep:
        shape = DEEP_EXT[::-1]
        box = np.ones(shape, dtype=np.uint8)
        _deep["box"] = (upload(box), W630, 1, f32_bits(np.ascontiguousarray(box_edtsq_closed_form(DEEP_EXT, W630).T)))
        rng = np.random.default_rng(sum(DEEP_EXT))
        deep = blocky_labels(shape, nlabels=3, zero_frac=0.0, block=300, rng=rng).astype(np.uint8)
        deep[rng.random(shape) < 0.0002] = 0
        _deep["deep"] = (upload(deep), W111, 0, f32_bits(oracle_port.edtsq(deep, W111[::-1], False)))
        shallow = labels_c(DEEP_EXT, np.uint8, seed=3, zero_frac=0.2, block=9)
        _deep["shallow"] = (upload(shallow), W630, 1, f32_bits(oracle_port.edtsq(shallow, W630[::-1], True)))
    return _deep


def deep_call(vol, ws, out, mode):
    labels, w, bb, _ = vol
    sentinel_fill(out)
    with_mode(mode, lambda: ok(lib().edt_hip_edtsq_device(vp(labels), U8, 3, *DEEP_EXT, *w, FLAG_BB if bb else 0, vp(out), vp(ws),
                                                          ws.numel(), stream())))


def deep_buffer():
    return shared_workspace(DEEP_EXT, max(with_mode(m, lambda: lib().edt_hip_workspace_bytes_flags(U8, 3, *DEEP_EXT, 0)) for m in DEEP_MODES))


def test_zero_fill_tiles_beyond_16_bits(oracle_port):
    ws, out, vols = deep_buffer(), transform_out(DEEP_EXT), deep_volumes(oracle_port)
    for name in ("box", "deep", "shallow"):
        for nth in (1, 2):
            fill(ws, "00")
            deep_call(vols[name], ws, out, 0)
            sync()
            equal_bits(out, vols[name][3], (name, "zero fill", nth))


@pytest.mark.parametrize("mode", DEEP_MODES, ids=[hex(m) for m in DEEP_MODES])
def test_residue_refusing_and_shallow_calls_in_both_orders(oracle_port, mode):
    """after a call whose tiles left 16 bits the map has cleared bits and (where the lists are launched) the counters are
    non-zero; after a shallow call the opposite holds: either state is the other call's residue"""
    ws, out, vols = deep_buffer(), transform_out(DEEP_EXT), deep_volumes(oracle_port)
    for first, second in (("box", "shallow"), ("shallow", "box"), ("deep", "shallow"), ("shallow", "deep"), ("deep", "box"), ("box", "deep")):
        deep_call(vols[first], ws, out, mode)
        deep_call(vols[second], ws, out, mode)
        sync()
        equal_bits(out, vols[second][3], (hex(mode), first, "then", second))


@pytest.mark.parametrize("pattern", DIRTY)
def test_pattern_fill_tiles_beyond_16_bits(oracle_port, pattern):
    ws, out, vols = deep_buffer(), transform_out(DEEP_EXT), deep_volumes(oracle_port)
    for name, mode in (("box", 0), ("deep", 0x20000000), ("shallow", 0), ("deep", 0)):
        fill(ws, pattern)
        deep_call(vols[name], ws, out, mode)
        sync()
        equal_bits(out, vols[name][3], (name, hex(mode), pattern))


# ---- long rows, a line, an axis beyond the wave kernels ------------------------------------------------------------------------
# (extents, ndim, voxel sizes, black border): rows of more than 4096 voxels (the line pipeline's scratch in the carve), a 1-D
# line of five blocks, a y axis of 2049 rows (tests/test_gpu_paths.py: test_axes_beyond_the_wave_kernels)
OTHER = [((4100, 7, 9), 3, WF, 0), ((5000, 1, 1), 1, (0.7, 1.0, 1.0), 1), ((17, 2049, 3), 3, W630, 1)]
OTHER_IDS = ["rows_of_4100", "line_of_5000", "axis_of_2049"]
_other = {}


def other_case(oracle_port, k, v):
    key = (k, v)
    if key not in _other:
        ext, ndim, w, bb = OTHER[k]
        dims = ext[:ndim]
        lab = labels_c(dims, np.uint16, seed=k + 5 * v, zero_frac=0.2, block=7 + 30 * v, nlabels=4)
        if ndim == 3:
            lab[0, 0, :] = 2                                    # a row without any boundary
        want = f32_bits(oracle_port.edtsq(lab, w[:ndim][::-1] if ndim > 1 else w[0], bool(bb)))
        labels, out = upload(lab), device_out(lab.shape, np.float32)
        nbytes = lib().edt_hip_workspace_bytes_flags(U16, ndim, *ext, 0)

        def call(ws, labels=labels, out=out):
            ok(lib().edt_hip_edtsq_device(vp(labels), U16, ndim, *ext, *w, FLAG_BB if bb else 0, vp(out), vp(ws), ws.numel(), stream()))
        _other[key] = Case(("edtsq_device", ext, v), nbytes, call, lambda what, out=out, want=want: equal_bits(out, want, what), outputs=(out,))
    return _other[key]


def buffer_after_a_route(nbytes, route):
    """the (64, 100, 100) buffer -- large enough for `nbytes` too, or a buffer of its own -- as `route` left it"""
    ws = transform_buffer()
    if ws.numel() < nbytes:
        ws = shared_workspace(("large", round256(nbytes)), nbytes)
    run_route(route, 0, ws, transform_out())
    return ws


@pytest.mark.parametrize("k", range(len(OTHER)), ids=OTHER_IDS)
def test_zero_fill_other_shapes(oracle_port, k):
    for v in (0, 1):
        case = other_case(oracle_port, k, v)
        two_calls(case, fresh_workspace(case.nbytes), "zero fill", "00")


@pytest.mark.parametrize("k", range(len(OTHER)), ids=OTHER_IDS)
def test_residue_other_shapes_after_a_route(oracle_port, k):
    c0, c1 = other_case(oracle_port, k, 0), other_case(oracle_port, k, 1)
    for route in (ROUTES[k], ROUTES[k + 5], ROUTES[k + 10]):   # (a different route for each shape)
        ws = buffer_after_a_route(max(c0.nbytes, c1.nbytes), route)
        two_calls(c0, ws, ("after route", route[0]))
        two_calls(c1, ws, "after the other labels")


@pytest.mark.parametrize("k", range(len(OTHER)), ids=OTHER_IDS)
def test_pattern_fill_other_shapes(oracle_port, k):
    case = other_case(oracle_port, k, 1)
    ws = fresh_workspace(case.nbytes)
    for pattern in DIRTY:
        two_calls(case, ws, "pattern fill", pattern)


# ---- the other entry points --------------------------------------------------------------------------------------------------
def case_voxel_graph(oracle_port, v, exact):
    """(64, 52, 50): both doubled axes on the integer kernel (104 and 100 rows) at (1, 1, 1) -- the index form, the hand-over
    counters; at (0.7, 1.3, 2.1) the table of sequential sums and the fp32 kernels"""
    ext = (64, 52, 50)
    rng = np.random.default_rng(17 + v)
    lab = labels_c(ext, np.uint8, seed=11 + v, zero_frac=0.25, block=6 + v)
    graph = np.full(lab.shape, 0b00111111, dtype=np.uint8)
    for bit in (0x01, 0x04, 0x10):
        graph[rng.random(lab.shape) < 0.08] &= np.uint8(~bit & 0xFF)
    w, bb = (W111, 0) if exact else (WF, 1)
    want = oracle_port.edtsq(lab, w[::-1], bool(bb), voxel_graph=graph)
    assert not np.isnan(want).any()
    want = f32_bits(want)
    labels, g, out = upload(lab), upload(graph), device_out(lab.shape, np.float32)

    def call(ws):
        ok(lib().edt_hip_edtsq_voxel_graph_device(vp(labels), U8, vp(g), 3, *ext, *w, bb, vp(out), vp(ws), ws.numel(), stream()))
    return Case(("edtsq_voxel_graph_device", w, v), lib().edt_hip_voxel_graph_workspace_bytes(3, *ext), call,
                lambda what: equal_bits(out, want, what), outputs=(out,))


FT_EXT, FT_W, FT_A = (33, 20, 12), W630, (1, 1, 25)


def ft_labels(v):
    return labels_c(FT_EXT, np.uint8, seed=FT_EXT[0] + v, zero_frac=0.3, block=4 + v)


def case_feature_transform(oracle_port, v):
    lab = ft_labels(v)
    want = ft_want(lab, FT_A, True).view(np.uint32)
    labels, out = upload(lab), device_out((3,) + lab.shape, np.int32)

    def call(ws):
        ok(lib().edt_hip_feature_transform_device(vp(labels), U8, 3, *FT_EXT, *FT_W, FLAG_BB, vp(out), vp(ws), ws.numel(), stream()))
    return Case(("feature_transform_device", v), lib().edt_hip_feature_workspace_bytes(U8, 3, *FT_EXT, FLAG_BB), call,
                lambda what: equal_bits(out, want, what), outputs=(out,))


def case_expand_labels(oracle_port, v):
    """the definition of include/edt_hip.h from the oracle's features of the mask labels == 0 (no border), as
    tests/test_gpu_offset_pointers.py states it"""
    lab8 = ft_labels(v)
    distance = 2.5 * FT_W[0]
    f = ft_want((lab8 == 0).astype(np.uint8), FT_A, False)            # planes x, y, z
    grids = np.stack(np.meshgrid(*[np.arange(s) for s in lab8.shape], indexing="ij"))[::-1]   # coordinates x, y, z
    w2 = [np.float64(np.float32(x)) * np.float64(np.float32(x)) for x in FT_W]
    D = np.zeros(lab8.shape)
    for k in range(3):                                                # terms added in ABI order x, y, z
        D = D + w2[k] * ((grids[k] - f[k]).astype(np.int64) ** 2).astype(np.float64)
    has = ~np.all(f == -1, axis=0)
    take = (lab8 == 0) & has & (D <= np.float64(distance) * np.float64(distance))
    src = tuple(np.where(take, f[k], 0) for k in (2, 1, 0))
    lab = lab8.astype(np.uint16)
    want = lab.copy()
    want[take] = lab[src][take]
    assert take.any() and not take[lab8 == 0].all()
    labels, out = upload(lab), device_out(lab.shape, np.uint16)

    def call(ws):
        ok(lib().edt_hip_expand_labels_device(vp(labels), U16, 3, *FT_EXT, *FT_W, float(distance), vp(out), vp(ws), ws.numel(), stream()))
    return Case(("expand_labels_device", v), lib().edt_hip_expand_labels_workspace_bytes(U16, 3, *FT_EXT), call,
                lambda what: equal_bits(out, want, what), outputs=(out,))


def case_label_stats(oracle_port, v):
    """32-bit labels: the open-addressing table, whose keys, counters and control words the call clears itself"""
    ext, cap = (9, 33, 40), 64
    rng = np.random.default_rng(40 + v)
    dt = (rng.integers(-3, 4, size=ext[::-1]).astype(np.float32) * np.float32(0.75))
    dt[rng.random(dt.shape) < 0.05] = np.inf
    lab = labels_c(ext, np.uint32, seed=2 + v, zero_frac=0.2, block=4, nlabels=9 + 20 * v)
    want = label_stats_oracle.label_stats(lab, dt)
    n = len(want.labels)
    assert 1 < n <= cap
    labels, field = upload(lab), upload(dt)
    keys, counts, mx = device_out((cap,), np.uint32), device_out((cap,), np.int64), device_out((cap,), np.float32)
    arg, bbox, nl = device_out((cap,), np.int64), device_out((cap, 6), np.int32), device_out((1,), np.int64)

    def call(ws):
        ok(lib().edt_hip_label_stats_device(vp(labels), U32, vp(field), 3, *ext, cap, vp(keys), vp(counts), vp(mx), vp(arg), vp(bbox),
                                            vp(nl), vp(ws), ws.numel(), stream()))

    def check(what):
        assert int(nl) == n, what
        box = bbox[:n].cpu().numpy()
        got = label_stats_oracle.LabelStats(
            keys[:n].cpu().numpy().view(lab.dtype), counts[:n].cpu().numpy(), mx[:n].cpu().numpy(),
            np.stack(np.unravel_index(arg[:n].cpu().numpy(), lab.shape), axis=1).astype(np.int64).reshape(n, 3),
            np.ascontiguousarray(box[:, 0::2][:, ::-1]), np.ascontiguousarray(box[:, 1::2][:, ::-1]))
        label_stats_oracle.assert_same(got, want, what)
        assert np.array_equal(got.max.view(np.uint32), want.max.view(np.uint32)), what
    return Case(("label_stats_device", v), lib().edt_hip_label_stats_workspace_bytes(U32, lab.size, cap), call, check,
                outputs=(keys, counts, mx, arg, bbox, nl))


def case_extract_runs(oracle_port, v):
    n = 5000
    lab = labels_c((n,), np.uint16, seed=n + v, block=2 + v)
    starts_want = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]]).astype(np.int64)
    assert len(starts_want) > 1024                          # (more runs than one block holds voxels: the scan's offsets are used)
    labels = upload(lab)
    starts, count = device_out((len(starts_want) + 8,), np.int64), device_out((1,), np.int64)

    def call(ws):
        ok(lib().edt_hip_extract_runs_device(vp(labels), U16, n, vp(starts), len(starts_want), vp(count), vp(ws), ws.numel(), stream()))

    def check(what):
        assert int(count) == len(starts_want), what
        equal_bits(starts[:len(starts_want)], starts_want.view(np.uint64), what)
        assert (bits_of(starts[len(starts_want):]) == MARK[8]).all(), what
    return Case(("extract_runs_device", v), lib().edt_hip_runs_workspace_bytes(n), call, check, outputs=(starts, count))


# -- the sharded phases: one virtual rank; the intermediate records are the oracle's too ----------------------------------------
def zflags_want(lab):
    """bit 0: foreground; bit 1: the label differs from the voxel below in z (slice 0 without a halo: always)"""
    starts = np.ones(lab.shape, dtype=bool)
    starts[1:] = lab[1:] != lab[:-1]
    return ((lab != 0).astype(np.uint8) | (starts.astype(np.uint8) << 1)).astype(np.uint8)


def pack_y(bits):
    """(sz, rows, sx) booleans -> (sz, ceil(rows / 32), sx) words: bit r of word b is row 32 b + r (rows beyond the end: 0)"""
    sz, rows, sx = bits.shape
    words = -(-rows // 32)
    padded = np.zeros((sz, words * 32, sx), dtype=np.uint64)
    padded[:, :rows, :] = bits
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64)).reshape(1, 1, 32, 1)
    return (padded.reshape(sz, words, 32, sx) * weights).sum(axis=2).astype(np.uint32)


def records_want(lab, field_words, ys, ye):
    """the slab records of destination rows ys..ye (include/edt_hip.h): per slice the rows' values -- `field_words`: (sz, sy,
    words per row) uint32 --, the foreground words, the "differs from the voxel below in z" words; (sz, record words) uint32"""
    sz = lab.shape[0]
    starts = np.ones(lab.shape, dtype=bool)
    starts[1:] = lab[1:] != lab[:-1]
    return np.concatenate([field_words[:, ys:ye, :].reshape(sz, -1), pack_y(lab[:, ys:ye, :] != 0).reshape(sz, -1),
                           pack_y(starts[:, ys:ye, :]).reshape(sz, -1)], axis=1).astype(np.uint32)


SH_EXT, SH_W = (64, 40, 33), (1.1, 0.7, 1.3)
_shard = {}


def shard_data(oracle_port, v):
    if ("flags", v) not in _shard:
        lab = labels_c(SH_EXT, np.uint32, seed=33 + v, block=6 + v)
        lab[5 + v, :, :] = 3                                  # a slice without any boundary: FLT_MAX between the phases
        partial = slices_after_xy(oracle_port, lab, SH_W[0], SH_W[1], 0)
        assert (partial == np.finfo(np.float32).max).any()
        _shard[("flags", v)] = (lab, partial, zflags_want(lab), oracle_port.edtsq(lab, SH_W[::-1], False))
    return _shard[("flags", v)]


def shard_bytes():
    L = lib()
    return max(L.edt_hip_shard_workspace_bytes(U32, *SH_EXT), L.edt_hip_shard_workspace_bytes(U8, *SH_EXT))


def case_shard_xy(oracle_port, v):
    lab, partial_want, flags_want, _ = shard_data(oracle_port, v)
    labels, partial, zflags = upload(lab), device_out(lab.shape, np.float32), device_out(lab.shape, np.uint8)

    def call(ws):
        ok(lib().edt_hip_shard_xy_device(vp(labels), None, U32, *SH_EXT, SH_W[0], SH_W[1], 0, vp(partial), vp(zflags), vp(ws), ws.numel(),
                                         stream()))

    def check(what):
        equal_bits(partial, f32_bits(partial_want), (what, "partial field"))
        equal_bits(zflags, flags_want, (what, "flags"))
    return Case(("shard_xy_device", v), shard_bytes(), call, check, outputs=(partial, zflags))


def case_shard_z(oracle_port, v, ex):
    lab, partial_want, flags_want, want = shard_data(oracle_port, v)
    pristine, partial, zflags = upload(partial_want), device_out(lab.shape, np.float32), upload(flags_want)
    floor = float(lib().edt_hip_field_floor(SH_W[0], SH_W[1]))
    assert floor > 0

    def call(ws):
        if ex:
            ok(lib().edt_hip_shard_z_device_ex(vp(partial), vp(zflags), *SH_EXT, SH_W[2], floor, 0, vp(ws), ws.numel(), stream()))
        else:
            ok(lib().edt_hip_shard_z_device(vp(partial), vp(zflags), *SH_EXT, SH_W[2], 0, vp(ws), ws.numel(), stream()))
    return Case(("shard_z_device_ex" if ex else "shard_z_device", v), shard_bytes(), call,
                lambda what: equal_bits(partial, f32_bits(want), what), restore=lambda: partial.copy_(pristine))


REC_SPLITS = (0, 64, 100)                                    # two destinations: 64 rows and 36 (a last word of four rows)


def record_data(oracle_port, v):
    """(64, 100, 100) at (6, 6, 30) with a black border: both scan axes on the integer kernel, no tile refused"""
    if ("records", v) not in _shard:
        lab = volume("blocky", v)
        field = slices_after_xy(oracle_port, lab, W630[0], W630[1], 1)
        q = float(math.gcd(math.gcd(int(W630[0]) ** 2, int(W630[1]) ** 2), int(W630[2]) ** 2))   # w_i^2 = a_i q
        quanta = field.astype(np.float64) / q
        assert np.array_equal(quanta, np.round(quanta)) and quanta.max() < 65535
        f16 = np.ascontiguousarray(quanta.astype(np.uint16)).view(np.uint32)          # packed pairs, x even in the low half
        parts = list(zip(REC_SPLITS[:-1], REC_SPLITS[1:]))
        _shard[("records", v)] = (lab, [records_want(lab, f32_bits(field), a, b) for a, b in parts],
                                  [records_want(lab, f16, a, b) for a, b in parts])
    return _shard[("records", v)]


def record_bytes(code=U8):
    L = lib()
    sx, sy, sz = EXT
    return max([L.edt_hip_shard_records_workspace_bytes(code, sx, sy, sz)] +
               [L.edt_hip_shard_records_workspace_bytes(U8, sx, b - a, sz) for a, b in zip(REC_SPLITS[:-1], REC_SPLITS[1:])])


def case_shard_xy_records(oracle_port, v, rows16):
    L = lib()
    lab, rec32, rec16 = record_data(oracle_port, v)
    wants = rec16 if rows16 else rec32
    sx, sy, sz = EXT
    for (a, b), w in zip(zip(REC_SPLITS[:-1], REC_SPLITS[1:]), wants):
        words = L.edt_hip_shard_record16_words(sx, b - a) if rows16 else L.edt_hip_shard_record_floats(sx, b - a)
        assert w.shape == (sz, words), (w.shape, words)
    assert L.edt_hip_shard_records_supported(U8, *EXT) == 1
    assert not rows16 or L.edt_hip_shard_records16_supported(U8, *EXT, *W630) == 1
    labels = device_labels("blocky", v)
    blocks = [device_out(w.shape, np.uint32) for w in wants]
    refused = device_out((1,), np.uint32)
    splits = (ctypes.c_int64 * len(REC_SPLITS))(*REC_SPLITS)
    ptrs = (ctypes.c_void_p * len(blocks))(*[b.data_ptr() for b in blocks])

    def call(ws):
        if rows16:
            ok(L.edt_hip_shard_xy_records16_device(vp(labels), None, U8, *EXT, *W630, FLAG_BB, len(blocks), splits, ptrs, vp(refused),
                                                   vp(ws), ws.numel(), stream()))
        else:
            ok(L.edt_hip_shard_xy_records_device(vp(labels), None, U8, *EXT, W630[0], W630[1], FLAG_BB, len(blocks), splits, ptrs, vp(ws),
                                                 ws.numel(), stream()))

    def check(what):
        assert not rows16 or int(refused) == 0, what
        for h, (block, w) in enumerate(zip(blocks, wants)):
            equal_bits(block, w, (what, "destination", h))
    # (the counter of refused tiles is the caller's: zeroed by the caller before every call)
    return Case(("shard_xy_records16_device" if rows16 else "shard_xy_records_device", v), record_bytes(), call, check, outputs=blocks,
                restore=lambda: refused.zero_())


def case_shard_z_records(oracle_port, v, form, h):
    """form: "" / "ex" (with the field's floor) / "w" (all three voxel sizes: the integer kernel) on the fp32 records of
    destination h, in place; "16": the 16-bit records into a dense array"""
    L = lib()
    lab, rec32, rec16 = record_data(oracle_port, v)
    sx, sy, sz = EXT
    ys, ye = REC_SPLITS[h], REC_SPLITS[h + 1]
    want = np.ascontiguousarray(route_want(oracle_port, ROUTES[0], v)[:, ys:ye, :])
    nbytes = record_bytes()
    if form == "16":
        records, out = upload(rec16[h]), device_out(want.shape, np.float32)

        def call(ws):
            ok(L.edt_hip_shard_z_records16_device(vp(records), vp(out), sx, ye - ys, sz, *W630, FLAG_BB, vp(ws), ws.numel(), stream()))

        def check(what):
            equal_bits(out, f32_bits(want), what)
            equal_bits(records, rec16[h], (what, "the records are only read"))
        return Case(("shard_z_records16_device", v, h), nbytes, call, check, outputs=(out,))
    pristine = upload(rec32[h])
    records = pristine.clone()
    nf = (ye - ys) * sx
    floor = float(L.edt_hip_field_floor(W630[0], W630[1]))

    def call(ws):
        if form == "w":
            ok(L.edt_hip_shard_z_records_device_w(vp(records), sx, ye - ys, sz, *W630, FLAG_BB, vp(ws), ws.numel(), stream()))
        elif form == "ex":
            ok(L.edt_hip_shard_z_records_device_ex(vp(records), sx, ye - ys, sz, W630[2], floor, FLAG_BB, vp(ws), ws.numel(), stream()))
        else:
            ok(L.edt_hip_shard_z_records_device(vp(records), sx, ye - ys, sz, W630[2], FLAG_BB, vp(ws), ws.numel(), stream()))

    def check(what):
        equal_bits(records[:, :nf], f32_bits(want), what)
        equal_bits(records[:, nf:], rec32[h][:, nf:], (what, "the records' bit planes"))
    return Case(("shard_z_records_device" + ("_" + form if form else ""), v, h), nbytes, call, check, restore=lambda: records.copy_(pristine))

# -- entry points whose stream-side initialisation this module's capture stage made a kernel's: fill_holes and
#    dust zero their counts ahead of their kernels, and every entry point with a count sets it for an empty volume -------------------
CC_EXT = (65, 12, 9)


def case_fill_holes(oracle_port, v):
    rng = np.random.default_rng(CC_EXT[0] + v)
    ids = blocky_labels(CC_EXT[::-1], nlabels=3, zero_frac=0.0, block=6 - v, rng=rng)
    ids[rng.random(ids.shape) < 0.08] = 0                      # pin-holes: cavities of one wall label and of two
    ids.flat[0] = ids.flat[-1] = 2
    lab = ids.astype(np.uint16)
    want = fill_holes_oracle.fill_holes(lab, 3, binary=False)
    assert want.n_filled > 0
    labels, out, n = upload(lab), device_out(lab.shape, np.uint16), device_out((1,), np.int64)

    def call(ws):
        ok(lib().edt_hip_fill_holes_device(vp(labels), U16, 3, *CC_EXT, 3, 0, vp(out), vp(n), vp(ws), ws.numel(), stream()))

    def check(what):
        assert int(n) == want.n_filled, what
        equal_bits(out, want.out.astype(np.uint16), what)
    return Case(("fill_holes_device", v), lib().edt_hip_fill_holes_workspace_bytes(U16, 3, *CC_EXT), call, check, outputs=(out, n))


def case_dust(oracle_port, v):
    lab = component_labels((CC_EXT[0] + v,) + CC_EXT[1:], np.uint8)
    ext = lab.shape[::-1]
    lo, hi = dust_oracle.bounds(4)
    want = dust_oracle.dust(lab, 4, 1, invert=False)
    assert 0 < want.kept < want.components
    labels, out, counts = upload(lab), device_out(lab.shape, np.uint8), device_out((3,), np.int64)

    def call(ws):
        ok(lib().edt_hip_dust_device(vp(labels), U8, 3, *ext, 1, 0, lo, hi, 0, vp(out), vp(counts), vp(ws), ws.numel(), stream()))

    def check(what):
        assert counts.tolist() == [want.components, want.kept, want.removed_voxels], what
        equal_bits(out, want.out.astype(np.uint8), what)
    return Case(("dust_device", v), lib().edt_hip_dust_workspace_bytes(U8, 3, *ext), call, check, outputs=(out, counts))


def case_empty_volumes(oracle_port, v):
    """a volume without voxels only sets the call's count(s), on the stream: no labels, no output, no workspace"""
    L = lib()
    e = ((0, 5, 4), (7, 0, 3))[v]
    n_cc, n_fh, n_ls, n_runs = (device_out((1,), np.int64) for _ in range(4))
    counts = device_out((3,), np.int64)

    def call(ws):
        ok(L.edt_hip_connected_components_device(None, U8, 3, *e, 1, 0, None, vp(n_cc), None, 0, stream()))
        ok(L.edt_hip_fill_holes_device(None, U8, 3, *e, 1, 0, None, vp(n_fh), None, 0, stream()))
        ok(L.edt_hip_dust_device(None, U8, 3, *e, 1, 0, 2, (1 << 63) - 1, 0, None, vp(counts), None, 0, stream()))
        ok(L.edt_hip_label_stats_device(None, U8, None, 3, *e, 16, None, None, None, None, None, vp(n_ls), None, 0, stream()))
        ok(L.edt_hip_extract_runs_device(None, U8, 0, None, 0, vp(n_runs), None, 0, stream()))

    def check(what):
        assert [int(n_cc), int(n_fh), int(n_ls), int(n_runs)] == [0, 0, 0, 0] and counts.tolist() == [0, 0, 0], what
    return Case(("empty volumes", e), 256, call, check, outputs=(n_cc, n_fh, n_ls, n_runs, counts))


# -- the compositions of the field operations: one workspace each, carved into fields, mask, planes and the transforms' scratch ---
MORPH_OPEN, MORPH_BINARY = 2, 128
FIELD_RADIUS = 6.0                                           # one voxel of x and y at FT_W: the outer voxel of every object erodes


def case_morphology(oracle_port, v):
    """opening of uint16 labels: both transforms, the select into the mask and the select into the output"""
    lab = ft_labels(v).astype(np.uint16)
    eroded = morph_oracle.erode(lab, FIELD_RADIUS, FT_W[::-1], black_border=True)
    assert 0 < np.count_nonzero(eroded) < np.count_nonzero(lab)
    want = morph_oracle.opening(lab, FIELD_RADIUS, FT_W[::-1], black_border=True)
    assert 0 < np.count_nonzero(want) < np.count_nonzero(lab)
    labels, out = upload(lab), device_out(lab.shape, np.uint16)

    def call(ws):
        ok(lib().edt_hip_morphology_device(vp(labels), U16, 3, *FT_EXT, *FT_W, MORPH_OPEN, FIELD_RADIUS, FLAG_BB, vp(out), vp(ws),
                                           ws.numel(), stream()))
    return Case(("morphology_device", v), lib().edt_hip_morphology_workspace_bytes(U16, 3, *FT_EXT, MORPH_OPEN, FLAG_BB), call,
                lambda what: equal_bits(out, want, what), outputs=(out,))


def case_local_thickness(oracle_port, v):
    """explicit radii: enqueue-only.  The sizes hold the sentinel before every call and replay: they are zeroed by a kernel"""
    lab = ft_labels(v)
    radii = np.array([1.0, 2.0, 3.5], dtype=np.float64) * min(FT_W)
    want, _, want_sizes = thickness_oracle.local_thickness(lab, radii, FT_W[::-1], black_border=True)
    assert 0 < want_sizes[-1] < want_sizes[0] < np.count_nonzero(lab)
    labels, T, sizes = upload(lab), device_out(lab.shape, np.float32), device_out((radii.size,), np.int64)
    n_used = ctypes.c_int64(-1)

    def call(ws):
        ok(lib().edt_hip_local_thickness_device(vp(labels), U8, 3, *FT_EXT, *FT_W, FLAG_BB, ctypes.c_void_p(radii.ctypes.data), radii.size,
                                                0.0, vp(T), vp(sizes), ctypes.byref(n_used), vp(ws), ws.numel(), stream()))

    def check(what):
        assert n_used.value == radii.size and sizes.tolist() == want_sizes.tolist(), (what, sizes.tolist(), want_sizes.tolist())
        equal_bits(T, f32_bits(want), what)
    return Case(("local_thickness_device", v), lib().edt_hip_local_thickness_workspace_bytes(U8, 3, *FT_EXT, FLAG_BB), call, check,
                outputs=(T, sizes))


MEDIAL_EXT = (65, 9, 17)                                     # more than one tile of 62 x 4 x 16 along every axis


def case_medial_axis(oracle_port, v):
    """with the radius, under binary: the planes, the mask and the field of the carve, and both transforms on one scratch"""
    lab = labels_c(MEDIAL_EXT, np.int32, seed=MEDIAL_EXT[0] + v, zero_frac=0.3, block=6 + v)
    kw = dict(anisotropy=FT_W[::-1], black_border=True, binary=True)
    on = medial_oracle.on_axis(lab, **kw)
    assert 0 < np.count_nonzero(on) < np.count_nonzero(lab)
    want = medial_oracle.medial_axis(lab, **kw)
    field = np.sqrt(oracle_port.edtsq((lab != 0).astype(np.uint8), FT_W[::-1], True))
    want_radius = np.where(on, field, np.float32(0.0)).astype(np.float32)
    labels, out, radius = upload(lab), device_out(lab.shape, np.int32), device_out(lab.shape, np.float32)
    gamma = float(max(FT_W))

    def call(ws):
        ok(lib().edt_hip_medial_axis_device(vp(labels), U32, 3, *MEDIAL_EXT, *FT_W, FLAG_BB | MORPH_BINARY, gamma, 0.0, vp(out), vp(radius),
                                            vp(ws), ws.numel(), stream()))

    def check(what):
        equal_bits(out, want.view(np.uint32), what)
        equal_bits(radius, f32_bits(want_radius), (what, "radius"))
    return Case(("medial_axis_device", v), lib().edt_hip_medial_axis_workspace_bytes(U32, 3, *MEDIAL_EXT, FLAG_BB | MORPH_BINARY, 1), call,
                check, outputs=(out, radius))


ENTRY = {
    "edtsq_voxel_graph_device": lambda o, v: case_voxel_graph(o, v, True),
    "edtsq_voxel_graph_device_fp32": lambda o, v: case_voxel_graph(o, v, False),
    "feature_transform_device": case_feature_transform,
    "expand_labels_device": case_expand_labels,
    "label_stats_device": case_label_stats,
    "extract_runs_device": case_extract_runs,
    "shard_xy_device": case_shard_xy,
    "shard_z_device": lambda o, v: case_shard_z(o, v, False),
    "shard_z_device_ex": lambda o, v: case_shard_z(o, v, True),
    "shard_xy_records_device": lambda o, v: case_shard_xy_records(o, v, False),
    "shard_z_records_device": lambda o, v: case_shard_z_records(o, v, "", 0),
    "shard_z_records_device_ex": lambda o, v: case_shard_z_records(o, v, "ex", 1),
    "shard_z_records_device_w": lambda o, v: case_shard_z_records(o, v, "w", 0),
    "shard_xy_records16_device": lambda o, v: case_shard_xy_records(o, v, True),
    "shard_z_records16_device": lambda o, v: case_shard_z_records(o, v, "16", 1 - v),
    "fill_holes_device": case_fill_holes,
    "dust_device": case_dust,
    "empty_volumes": case_empty_volumes,
    "morphology_device": case_morphology,
    "local_thickness_device": case_local_thickness,
    "medial_axis_device": case_medial_axis,
}
_cases = {}


def entry_case(oracle_port, name, v):
    if (name, v) not in _cases:
        _cases[(name, v)] = ENTRY[name](oracle_port, v)
    return _cases[(name, v)]


@pytest.mark.parametrize("name", list(ENTRY))
def test_zero_fill_entry_points(oracle_port, name):
    for v in (0, 1):
        case = entry_case(oracle_port, name, v)
        two_calls(case, fresh_workspace(case.nbytes), "zero fill", "00")


@pytest.mark.parametrize("name", list(ENTRY))
def test_residue_entry_points(oracle_port, name):
    """on the buffer the first transform route has just used: the call on labels 0, on labels 1 -- behind its own call on other
    labels --, and on labels 0 again"""
    c0, c1 = entry_case(oracle_port, name, 0), entry_case(oracle_port, name, 1)
    ws = buffer_after_a_route(max(c0.nbytes, c1.nbytes), ROUTES[0])
    two_calls(c0, ws, "after the first transform route")
    two_calls(c1, ws, "after its own call on other labels")
    two_calls(c0, ws, "and back")


@pytest.mark.parametrize("name", list(ENTRY))
def test_pattern_fill_entry_points(oracle_port, name):
    case = entry_case(oracle_port, name, 1)
    ws = fresh_workspace(case.nbytes)
    for pattern in DIRTY:
        two_calls(case, ws, "pattern fill", pattern)


@pytest.mark.parametrize("name", list(ENTRY))
def test_capture_entry_points(oracle_port, name):
    case = entry_case(oracle_port, name, 0)
    capture_and_replay(case, fresh_workspace(case.nbytes))
