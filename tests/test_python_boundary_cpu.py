"""The numpy layer of the package (edt/__init__.py) is argument handling only: which refusal comes first, which buffer, dtype
code, extents and voxel sizes reach the C ABI, and what comes back in which type, shape and memory order.
tests/golden/python_calls.json holds all of that for the calls of boundary_cases(), recorded from the commit BEFORE the two
Python layers were given one argument boundary (edt/_args.py); every row must stay exactly that.  No GPU and no kernel: a
recording stand-in takes the place of ``edt._lib.load`` and answers EDT_OK (tests/golden/README.md says what it writes down;
tests/golden/make_golden_python_calls.py wrote the table).

The table stores answers only, in the order of boundary_cases(), and a digest of the cases they belong to."""
import ctypes
import hashlib
import json
import os
import warnings

import numpy as np

from conftest import ROOT

TABLE = os.path.join(ROOT, "tests", "golden", "python_calls.json")
NAN, INF = float("nan"), float("inf")

# the names of edt.__all__ that never reach the library
NO_LIBRARY = {"each", "runs", "draw", "transfer", "erase", "reshape", "nvl", "EdtHipError", "LabelMoments", "LabelTopology",
              "DustCounts", "ThicknessSizes"}
CLASSES = ("TypeError", "ValueError", "EdtHipError")

NO_ANISOTROPY = ("label_moments", "label_topology", "connected_components", "fill_holes", "dust")
TABLES = ("label_stats", "label_moments", "label_topology")
BASE = {"dust": {"threshold": 2}}

SHAPES = [((5,), "C"), ((3, 4), "C"), ((2, 3, 4), "C"), ((1, 3, 1), "C"), ((3, 4), "F"), ((3, 4), "strided"), ((0, 3), "C"),
          ((2, 3, 4), "F"), ((2, 2, 2, 2), "C")]
DTYPES = ["uint8", "int8", "uint16", "int32", "uint64", "float32", "float64", "bool", "complex64"]
# (shape, layout, anisotropy): a scalar, tuples, a numpy array, values float32 rounds; a negative size off the fastest axis
# (accepted) and on it; zero, NaN, inf, a wrong length; an empty array with a bad anisotropy (an empty result)
ANISOTROPY = [
    ((5,), "C", 2.0), ((5,), "C", (0.1,)), ((5,), "C", ("np", [3.0])), ((5,), "C", -1.0), ((5,), "C", 0.0), ((5,), "C", NAN),
    ((5,), "C", INF), ((5,), "C", (1.0, 2.0)),
    ((3, 4), "C", (2.0, 0.1)), ((3, 4), "C", (-2.0, 1.0)), ((3, 4), "C", (1.0, -2.0)), ((3, 4), "C", (0.0, 1.0)),
    ((3, 4), "C", (NAN, 1.0)), ((3, 4), "C", (1.0, INF)), ((3, 4), "C", (1.0, 2.0, 3.0)), ((3, 4), "C", 2.0),
    ((3, 4), "F", (-2.0, 1.0)), ((3, 4), "F", (1.0, -2.0)), ((3, 4), "strided", (0.1, 3.0)),
    ((2, 3, 4), "C", (1.0, 2.0, 0.1)), ((2, 3, 4), "C", ("np", [4.0, 4.0, 40.0])), ((2, 3, 4), "C", (1.0, -1.0, 1.0)),
    ((2, 3, 4), "C", (1.0, 2.0)), ((2, 3, 4), "C", (0.1, 0.3)), ((2, 3, 4), "C", (1.0, 1.0, 1.0, 1.0)),
    ((2, 3, 4), "F", (0.1, 2.0, 3.0)), ((1, 3, 1), "C", (1.0, 2.0, -3.0)), ((0, 3), "C", (0.0, NAN)), ((0, 3), "C", (1.0,)),
]
RETRY = ("arr", (70000,), "uint32", "C")


def library_names(edt):
    return [n for n in edt.__all__ if n not in NO_LIBRARY]


def boundary_cases(names):
    """[name, input, keyword arguments, script of the stand-in] of every row.  An input or argument that is an array is spelled
    ("arr", shape, dtype, layout) -- build() makes it --, a numpy vector ("np", values).  The script: "counts", what the
    stand-in writes through the count pointer of successive calls ("cap+1": one more than the capacity it was given);
    "fail", [symbol, return code, error text] of a call it refuses."""
    cases = []

    def add(name, data, script=None, **kw):
        cases.append([name, data, dict(BASE.get(name, {}), **kw), script or {}])

    for name in names:
        if name == "set_devices":
            for devices in (None, [], [0], [1, 0, 3]):
                add(name, devices)
            continue
        for shape, layout in SHAPES:
            add(name, ("arr", shape, "uint32", layout))
        for dtype in DTYPES:
            add(name, ("arr", (3, 4), dtype, "C"))
            add(name, ("arr", (2, 3, 4), dtype, "F"))
        add(name, ("list", [[0, 1, 1], [2, 2, 0]]))
        add(name, ("arr", (2, 3, 4), "uint16", "C"), script={"fail": [None, -3, "scripted refusal"]})
        if name not in NO_ANISOTROPY:
            for shape, layout, an in ANISOTROPY:
                add(name, ("arr", shape, "uint8", layout), anisotropy=an)
            if name not in ("expand_labels", "dilate", "closing"):
                add(name, ("arr", (2, 3, 4), "int32", "C"), black_border=True)
    vol, img, line = ("arr", (2, 3, 4), "uint8", "C"), ("arr", (3, 4), "uint16", "F"), ("arr", (5,), "int32", "C")

    # the voxel graph of the transforms
    for name in ("edt", "edtsq", "sdf", "sdfsq", "edt2d", "edt2dsq", "edt3d", "edt3dsq"):
        for data in (vol, img, line, ("arr", (3, 4), "uint16", "strided")):
            add(name, data, voxel_graph=("arr", data[1], "uint8", "C"))
        add(name, vol, voxel_graph=("arr", (2, 3, 4), "uint32", "F"), anisotropy=(1.0, 2.0, 0.1), black_border=True)
        add(name, vol, voxel_graph=("arr", (2, 3, 5), "uint8", "C"))
        add(name, img, voxel_graph=("arr", (4, 3), "uint8", "C"))
    # connectivity
    for name, extra in (("connected_components", "return_N"), ("fill_holes", "return_fill_count"), ("dust", "return_counts"),
                        ("watershed", "return_N")):
        for data in (line, img, vol):
            for c in (0, True, 1, 2, 3, 4, 5, 6, 7, 8, 18, 26, 1.0):
                add(name, data, connectivity=c)
            add(name, data, binary=True, **{extra: True})
        add(name, ("arr", (0, 3), "uint8", "C"), connectivity=7, **{extra: True})
        add(name, ("arr", (0, 3), "uint8", "C"), **{extra: True})
    # dust
    for t in (-1, (3, 2), 2.5, 0, (2, 3), [2, 2], True, (1, 2, 3), 1 << 63):
        add("dust", vol, threshold=t)
    add("dust", img, threshold=(1, 5), invert=True, return_counts=True)
    # watershed
    for h in (NAN, -1, True, INF, 0.5, 1e39, "x", None):
        add("watershed", vol, min_saliency=h)
    for data in (vol, img, ("arr", (3, 4), "uint16", "strided")):
        add("watershed", data, field=("arr", data[1], "float32", "C"), return_N=True)
    add("watershed", vol, field=("arr", (2, 3, 4), "float32", "F"), anisotropy=(0.0, 1.0, 1.0))
    add("watershed", vol, field=("arr", (2, 3, 5), "float32", "C"))
    add("watershed", vol, field=("arr", (2, 3, 4), "float64", "C"))
    add("watershed", vol, field=("nan", (2, 3, 4)))
    add("watershed", ("arr", (0, 3), "uint8", "C"), field=("arr", (3, 0), "float32", "C"))
    add("watershed", vol, anisotropy=(2.0, 1.0, 0.1), black_border=True, binary=True, min_saliency=0.5)
    # label_stats' dt
    for data in (vol, img, ("arr", (3, 4), "uint16", "strided")):
        add("label_stats", data, dt=("arr", data[1], "float32", "C"))
    add("label_stats", vol, dt=("arr", (2, 3, 5), "float32", "C"))
    add("label_stats", vol, dt=("arr", (2, 3, 4), "float64", "C"))
    add("label_stats", vol, dt=("arr", (2, 3, 4), "float32", "F"), anisotropy=(1.0, NAN, 1.0), max_labels=5)
    # the label tables: max_labels, and the retry of a default capacity that proves too small
    for name in TABLES:
        for m in (0, -3, 1, 5, 100, 2.5):
            add(name, vol, max_labels=m)
        add(name, ("arr", (0, 3), "uint8", "C"), max_labels=0)
        add(name, ("arr", (3, 4), "int8", "F"), script={"counts": [0]})
        add(name, RETRY, script={"counts": ["cap+1", 0]})
        add(name, RETRY, script={"counts": ["cap+1", "cap+1", 0]})
        add(name, RETRY, script={"counts": ["cap+1"]}, max_labels=10)
        add(name, RETRY, max_labels=100000)
        add(name, ("arr", (300,), "uint8", "C"))
        add(name, ("arr", (300, 300), "uint16", "C"))
    # morphology
    for name in ("erode", "dilate", "opening", "closing"):
        for r in (-1, 1e200, INF, 0, 2.5, NAN, "x"):
            add(name, vol, radius=r)
        add(name, ("arr", (0, 3), "uint8", "C"), radius=-1)
        add(name, img, radius=2.0, anisotropy=(0.1, 3.0))
    for name in ("erode", "opening"):
        add(name, vol, black_border=True, binary=True)
        add(name, vol, binary=True)
    for d in (-1, NAN, 0, INF, 2.5):
        add("expand_labels", vol, distance=d)
    add("expand_labels", ("arr", (0, 3), "uint8", "C"), distance=-1)
    # local_thickness
    for radii in ([], [2, 1], [1, 1], [0, 1], [1.5], [1, 2.5, 4], ("np", [0.5, 1.0]), [-1], [1e200], "x", 2.0):
        for sizes in (False, True):
            add("local_thickness", vol, radii=radii, return_sizes=sizes)
    add("local_thickness", vol, script={"counts": [3]}, return_sizes=True)
    add("local_thickness", vol, script={"counts": [3]})
    add("local_thickness", img, script={"counts": [2]}, return_sizes=True, anisotropy=(-0.5, 3.0), black_border=True, binary=True)
    add("local_thickness", ("arr", (0, 3), "uint8", "C"), return_sizes=True)
    add("local_thickness", ("arr", (0, 3), "uint8", "C"), return_sizes=True, radii=[1, 2])
    add("local_thickness", ("arr", (0, 3), "uint8", "C"), radii=[2, 1])
    # medial_axis
    for a in (180, -1, 179.9999999999999, 0, 90.0, NAN, "x", None):
        add("medial_axis", vol, min_angle=a)
    for g in (-1, 0, 2.5, 1e200, NAN, INF, "x", None):
        add("medial_axis", vol, gamma=g, anisotropy=(1.0, -3.0, 2.0))
    add("medial_axis", vol, return_distance=True, black_border=True, binary=True)
    add("medial_axis", ("arr", (0, 3), "uint8", "C"), return_distance=True)
    add("medial_axis", ("arr", (0, 3), "uint8", "C"), gamma=-1)
    add("medial_axis", ("arr", (0, 3), "uint8", "C"), min_angle=180)
    # feature_transform
    for data in (line, img, vol, ("arr", (0, 3), "uint8", "C")):
        add("feature_transform", data, return_distances=True, black_border=True)
    # which refusal comes first: an unsupported dtype against the call's own arguments and the empty case
    odd, none = ("arr", (3, 4), "complex64", "C"), ("arr", (0, 3), "complex64", "C")
    for name in names:
        if name != "set_devices":
            add(name, none)
    for name in TABLES:
        add(name, odd, max_labels=0)
    add("label_stats", odd, dt=("arr", (3, 5), "float32", "C"))
    add("expand_labels", odd, distance=-1)
    add("dust", odd, threshold=-1)
    add("connected_components", odd, connectivity=0)
    add("watershed", odd, min_saliency=-1)
    add("erode", odd, radius=-1)
    add("local_thickness", odd, radii=[])
    add("medial_axis", odd, min_angle=180)
    add("feature_transform", odd, anisotropy=(1.0,))
    # the transforms' own
    for name in ("edt", "edtsq", "sdf", "sdfsq", "binary_edt", "binary_edtsq", "edt_stack", "edtsq_stack"):
        add(name, ("arr", (2, 3, 4), "float64", "strided"), black_border=True)
    return cases


def digest(cases):
    return hashlib.sha256(repr(cases).encode()).hexdigest()


def build(spec):
    """the argument a case spells: an array, a numpy vector, or the value itself"""
    if not (isinstance(spec, tuple) and spec and spec[0] in ("arr", "np", "list", "nan")):
        return spec
    if spec[0] == "np":
        return np.array(spec[1], dtype=np.float64)
    if spec[0] == "list":
        return [list(r) for r in spec[1]]
    if spec[0] == "nan":
        return np.full(spec[1], np.nan, dtype=np.float32)
    _, shape, dtype, layout = spec
    full = ((2 * shape[0],) + tuple(shape[1:])) if layout == "strided" else tuple(shape)
    v = (np.arange(int(np.prod(full)), dtype=np.int64) * 7 % 5 % 3).reshape(full)   # 0, 1, 2: background and two labels
    dt = np.dtype(dtype)
    if dt.kind == "i":
        v = np.where(v == 2, -1, v)
    a = (v * 1.5).astype(dt) if dt.kind in "fc" else (v != 0) if dt.kind == "b" else v.astype(dt)
    a = np.asfortranarray(a) if layout == "F" else np.ascontiguousarray(a)
    return a[::2] if layout == "strided" else a


# the pointers a call READS, by position, besides the labels at 0: (what it is, bytes per voxel) or ("count", argument that
# holds the count, bytes per entry)
READS = {
    "edt_hip_label_stats": {10: ("voxels", 4)}, "edt_hip_watershed": {6: ("voxels", 4)},
    "edt_hip_edt2dsq_voxel_graph": {2: ("voxels", 1)}, "edt_hip_edt3dsq_voxel_graph": {2: ("voxels", 1)},
    "edt_hip_local_thickness": {10: ("count", 11, 8)}, "edt_hip_set_devices": {0: ("count", 1, 4)},
}
# where a call takes its capacity and returns a count: symbol -> (capacity or None, count pointer)
COUNTS = {"edt_hip_label_stats": (11, 17), "edt_hip_label_moments": (6, 12), "edt_hip_label_topology": (6, 10),
          "edt_hip_connected_components": (None, 9), "edt_hip_fill_holes": (None, 9), "edt_hip_watershed": (None, 15),
          "edt_hip_local_thickness": (None, 15)}


class StandIn:
    """What takes the place of the loaded library: every edt_hip_* symbol is a function that writes its arguments down as
    the prototype of edt/_lib.py: SIGNATURES would convert them, and answers EDT_OK."""

    def __init__(self, lib_module, voxels, script):
        self._lib, self._voxels = lib_module, voxels
        self._counts = list(script.get("counts", []))
        self._fail = script.get("fail")
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("edt_hip_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, *args)

    @staticmethod
    def _address(arg):
        if arg is None:
            return 0
        if isinstance(arg, int):
            return arg
        if isinstance(arg, ctypes.c_void_p):
            return arg.value or 0
        return ctypes.addressof(arg._obj)        # ctypes.byref(...)

    def _call(self, name, *args):
        if name == "edt_hip_last_error":
            return self._fail[2].encode()
        restype, argtypes = self._lib.SIGNATURES[name]
        if len(args) != len(argtypes):
            raise TypeError(f"{name} takes {len(argtypes)} arguments ({len(args)} given)")
        row = [name]
        for i, (arg, kind) in enumerate(zip(args, argtypes)):
            if kind is ctypes.c_void_p:
                address = self._address(arg)
                nbytes = self._bytes_behind(name, i, args)
                row.append("0" if not address else "p" if nbytes is None else
                           "p:" + hashlib.sha256(ctypes.string_at(address, nbytes)).hexdigest()[:12])
            elif kind in (ctypes.c_float, ctypes.c_double):
                row.append(float(kind(arg).value).hex())
            else:
                row.append(int(kind(arg).value))
        self.calls.append(row)
        if self._fail and self._fail[0] in (None, name):
            return self._fail[1]
        if name in COUNTS and self._counts:
            cap, where = COUNTS[name]
            n = self._counts.pop(0)
            args[where]._obj.value = int(args[cap]) + 1 if n == "cap+1" else n
        return 0

    def _bytes_behind(self, name, i, args):
        if i == 0 and name != "edt_hip_set_devices":
            return self._voxels * self._lib.DTYPE_SIZE[int(args[1])]
        what = READS.get(name, {}).get(i)
        if what is None:
            return None
        return self._voxels * what[1] if what[0] == "voxels" else int(args[what[1]]) * what[2]


def describe(value):
    """type, dtype, shape and contiguity of what a call returned; scalars and the radii / sizes of ThicknessSizes as they are"""
    if isinstance(value, np.ndarray):
        flags = ("C" if value.flags.c_contiguous else "") + ("F" if value.flags.f_contiguous else "")
        return ["ndarray", str(value.dtype), list(value.shape), flags or "-"]
    if isinstance(value, tuple):
        if type(value).__name__ == "ThicknessSizes":
            return ["ThicknessSizes", [describe(v) + [[float(x).hex() for x in v.tolist()]] for v in value]]
        return [type(value).__name__, [describe(v) for v in value]]
    if isinstance(value, (bool, int, float, type(None))):
        return [type(value).__name__, repr(value)]
    return [type(value).__name__]


def answer(edt, case):
    """[exception (class, text) or None, the library calls made, what came back] of one case"""
    name, data, kwargs, script = case
    arg = build(data)
    voxels = 0 if arg is None or name == "set_devices" else int(np.asarray(arg).size)
    stand_in = StandIn(edt._lib, voxels, script)
    saved = edt._lib.load
    edt._lib.load = lambda: stand_in
    try:
        try:
            with warnings.catch_warnings():      # (the stand-in computes nothing: what a call returns is uninitialised memory)
                warnings.simplefilter("ignore")
                got = getattr(edt, name)(arg, **{k: build(v) for k, v in kwargs.items()})
        except Exception as e:  # noqa: BLE001  (the refusal is the answer)
            return [[type(e).__name__, str(e)], stand_in.calls, None]
        return [None, stand_in.calls, describe(got)]
    finally:
        edt._lib.load = saved


def coverage_gaps(cases, rows):
    """what would make the table an empty check: a library-calling name without a call, an exception class no row has"""
    import edt
    called = {c[0] for c, r in zip(cases, rows) if r[1]}
    gaps = [n for n in library_names(edt) if n not in called]
    return gaps + [k for k in CLASSES if not any(r[0] and r[0][0] == k for r in rows)]


def load_table():
    with open(TABLE) as f:
        t = json.load(f)
    return t, [t["answers"][i] for i in t["rows"]]


def test_calls_are_those_of_the_recorded_table():
    import edt
    cases = boundary_cases(library_names(edt))
    table, want = load_table()
    assert table["cases_sha256"] == digest(cases) and len(want) == len(cases), "the table does not hold the calls of boundary_cases()"
    got = [json.loads(json.dumps(answer(edt, c))) for c in cases]
    wrong = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]          # every row: none is left out
    assert not wrong, f"{len(wrong)} of {len(got)} calls differ, e.g. (case, got, recorded): {wrong[:3]}"


def test_the_table_is_no_empty_check():
    import edt
    cases = boundary_cases(library_names(edt))
    _, rows = load_table()
    assert coverage_gaps(cases, rows) == []
    retried = [r for c, r in zip(cases, rows) if c[1] == RETRY and c[3].get("counts") == ["cap+1", 0]]
    assert len(retried) == 3
    for r in retried:                                     # the capacities of the retry: 65536, then all 70000 voxels
        cap = COUNTS[r[1][0][0]][0]
        assert r[0] is None and [call[1 + cap] for call in r[1]] == [65536, 70000]
    explicit = [r for c, r in zip(cases, rows) if c[1] == RETRY and c[2].get("max_labels") == 10]
    assert len(explicit) == 3 and all(r[0] and r[0][0] == "ValueError" for r in explicit)


def test_label_stats_is_one_class():
    import edt
    import edt.device
    assert edt.LabelStats is edt.device.LabelStats
