"""CPU tier of label_moments (include/edt_hip.h, "label_moments"): the Python-integer oracle against a loop over labels and
against scipy, the closed form of a run's moments and the hand-rounded 128-bit arithmetic of csrc/edt_moments_math.h through a
host shim, every refusal of the three ABI functions (all of them happen before any device work, so no device is needed), the
Python surface, and the principal axes."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import moments_oracle as oracle
from synth import aligned_host_bytes, blocky_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
BAD_ARG, UNSUPPORTED = -2, -4
U8, U16, U32, U64, F32, F64, BOOL = range(7)
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def lib():
    from edt import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def shim():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, f"libmoments_{os.getpid()}.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                    "-I" + os.path.join(ROOT, "euclidean-distance-transform-3d_amd", "csrc"),
                    os.path.join(ROOT, "tests", "moments_shim.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    u64, i64, vp = ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p
    lib.moments_run.restype, lib.moments_run.argtypes = None, [u64, u64, u64, u64, vp]
    lib.moments_u128_to_double.restype, lib.moments_u128_to_double.argtypes = ctypes.c_double, [u64, u64]
    lib.moments_derive.restype, lib.moments_derive.argtypes = None, [vp, vp, vp]
    lib.moments_in_range.restype, lib.moments_in_range.argtypes = ctypes.c_int, [i64, i64, i64]
    yield lib
    try:
        os.remove(so)
    except OSError:
        pass


# ---- 1. the oracle ------------------------------------------------------------------------------------------------------
def test_oracle_against_a_loop_over_labels():
    rng = np.random.default_rng(21)
    vols = [blocky_labels((7, 5, 6), nlabels=4, zero_frac=0.3, block=2, rng=rng).astype(np.int16) - 2,
            blocky_labels((9, 8), nlabels=6, zero_frac=0.2, block=3, rng=rng).astype(np.uint64) << np.uint64(40),
            blocky_labels((5, 4, 3), nlabels=3, zero_frac=0.2, block=2, rng=rng).astype(np.float32) - 1.5,
            blocky_labels((23,), nlabels=3, zero_frac=0.2, block=2, rng=rng).astype(np.uint8)]
    vols[2][0, 0, 0] = np.nan
    vols[2][1, 1, 1] = -0.0
    for lab in vols:
        for data in (lab, np.asfortranarray(lab)):     # per array axis: the memory order changes nothing
            got, want = oracle.label_moments(data), oracle.brute_force(data)
            assert len(want.labels) > 1
            oracle.assert_same(got, want, (lab.dtype, data.flags.f_contiguous))
    # one voxel at (2, 3): every moment by hand
    lab = np.zeros((4, 5), dtype=np.uint8)
    lab[2, 3] = 9
    got = oracle.label_moments(lab)
    assert got.labels.tolist() == [9] and got.counts.tolist() == [1] and got.first.tolist() == [[2, 3]]
    assert got.second.tolist() == [[[4, 6], [6, 9]]] and got.centroid.tolist() == [[2.0, 3.0]]
    assert got.covariance.tolist() == [[[0.0, 0.0], [0.0, 0.0]]]


def test_oracle_centroid_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(22)
    lab = blocky_labels((12, 40, 33), nlabels=7, zero_frac=0.25, block=5, rng=rng).astype(np.uint16)
    got = oracle.label_moments(lab)
    want = np.array(ndimage.center_of_mass(np.ones(lab.shape), lab, got.labels.tolist()))
    # they round differently and both are a handful of fp64 operations: 4 ulp of the coordinate
    assert np.all(np.abs(got.centroid - want) <= 4 * np.spacing(np.abs(want)))


# ---- 2. the closed form and the hand-rounded arithmetic -----------------------------------------------------------------
def _run_sums(x0, n, y, z):
    xs = range(x0, x0 + n)
    return [n, sum(xs), n * y, n * z, sum(x * x for x in xs), n * y * y, n * z * z, y * sum(xs), z * sum(xs), n * y * z]


@pytest.mark.parametrize("x0", [0, 1, 63, 2 ** 16 - 1, 2 ** 31 - 257])
def test_closed_form_of_a_run_equals_python_integers(shim, x0):
    out = np.zeros(10, dtype=np.uint64)
    for y, z in ((0, 0), (1, 2), (2 ** 31 - 1, 2 ** 31 - 2), (12345, 2 ** 31 - 1)):
        for n in range(1, 257):
            shim.moments_run(x0, n, y, z, out.ctypes.data)
            want = [v % (1 << 64) for v in _run_sums(x0, n, y, z)]
            assert out.tolist() == want, (x0, n, y, z)


def _bits(x):
    return np.float64(x).view(np.uint64)


def test_128_bit_conversion_rounds_to_nearest_even(shim):
    rng = np.random.default_rng(23)
    vals = [0, 1, 2, 3, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 53 + 3, 2 ** 54 + 2, 2 ** 54 + 6, 2 ** 64 - 1, 2 ** 64,
            2 ** 64 + 2 ** 11, 2 ** 64 + 2 ** 11 + 1, 2 ** 64 + 3 * 2 ** 11, 2 ** 127, 2 ** 128 - 1, 2 ** 128 - 2 ** 74, 2 ** 128 - 2 ** 75,
            2 ** 100 + 2 ** 47, 2 ** 100 + 2 ** 47 + 1, 2 ** 100 + 2 ** 48 + 2 ** 47, (2 ** 53 - 1) << 70, ((2 ** 54 - 1) << 60) + 5]
    for bits in range(1, 129):                        # random values of every length, and their neighbours of a tie
        v = int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) * 16 % (1 << bits)
        vals += [v, v | 1, (v >> 1) << 1]
        if bits > 54:
            tie = ((v >> (bits - 54)) | 1) << (bits - 54)   # 54 significant bits, the last one set: exactly half way
            vals += [tie, tie + 1, tie - 1]
    for v in vals:
        if v >= 1 << 128:
            continue
        got = shim.moments_u128_to_double(v >> 64, v & (2 ** 64 - 1))
        assert _bits(got) == _bits(float(v)), (hex(v), got, float(v))


def test_derived_values_equal_python_integers(shim):
    """centroid and covariance as the finish kernel derives them, against the oracle's Python-integer form: sums past 2^53,
    M_ab past 2^64, a tiny covariance against large S^2 / n, negative off-diagonal terms"""
    cases = []
    cases.append([(x, 0, 0) for x in range(300000)])             # M_xx past 2^64, S_xx just below 2^53
    cases.append([(x, 0, 0) for x in range(400000)])             # S_xx past 2^53 too
    cases.append([(x, y, z) for z in range(0, 60000, 2) for y in range(4) for x in range(3)])
    cases.append([(38 + i, 38 + j, 2998 + k) for i in range(2) for j in range(2) for k in range(2)])
    cases.append([(i, 100 - i, 7 * i % 13) for i in range(50)])     # anti-correlated
    for pts in cases:
        p = np.array(pts, dtype=np.int64)
        n = len(pts)
        first = [int(p[:, a].sum()) for a in range(3)]
        second = [[int((p[:, a] * p[:, b]).sum()) for b in range(3)] for a in range(3)]
        sums = np.array([n] + first + [second[0][0], second[1][1], second[2][2], second[0][1], second[0][2], second[1][2]],
                        dtype=np.uint64)
        c, m = np.zeros(3), np.zeros(6)
        shim.moments_derive(sums.ctypes.data, c.ctypes.data, m.ctypes.data)
        wc, wm = oracle.derive(n, first, second)
        assert [_bits(v) for v in c] == [_bits(v) for v in wc]
        want = [wm[0][0], wm[1][1], wm[2][2], wm[0][1], wm[0][2], wm[1][2]]
        assert [_bits(v) for v in m] == [_bits(v) for v in want], (n, m, want)
        # and the definition is accurate: within 2 ulp of the exact rational covariance, however far the object is from the origin
        for k, (a, b) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
            exact = Fraction(n * second[a][b] - first[a] * first[b], n * n)
            assert abs(Fraction(float(m[k])) - exact) <= 2 * abs(exact) * Fraction(1, 2 ** 52), (k, m[k], float(exact))


def test_range_bound(shim):
    for ext in [(0, 0, 0), (1, 1, 1), (2 ** 31 - 1, 1, 1), (2 ** 22, 1, 1), (10 ** 6, 1, 1), (2048, 2048, 2048), (2097152, 1, 1),
                (2097153, 1, 1), (1, 5, 2 ** 21), (40, 40, 3000), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (65536, 65536, 1),
                (46341, 46341, 2)]:
        voxels, e = ext[0] * ext[1] * ext[2], max(ext)
        want = e <= 1 or voxels * (e - 1) ** 2 < 2 ** 63
        assert bool(shim.moments_in_range(*ext)) == want, ext


# unit -> (kernels: clear, 7 per sweep, finish_direct, compact, rank; {sweep: (LDS bytes, waves per SIMD its registers have to
# admit -- what it has had since it was written: a register more than that occupancy's budget costs a whole wave)}; sweeps
# whose LDS table has to admit 7 workgroups per compute unit; sweeps that have to fit 256 VGPRs)
_UNITS = {
    "edt_labelstats.hip": (18, {"k_ls_sweep1": (22528, 6), "k_ls_sweep2": (5120, 8)}, ("k_ls_sweep1",), ()),
    "edt_moments.hip": (11, {"k_mm_sweep": (22528, 7)}, ("k_mm_sweep",), ()),
    "edt_topology.hip": (11, {"k_tp_sweep": (18432, 2)}, (), ("k_tp_sweep",)),
}


@pytest.mark.parametrize("unit", sorted(_UNITS))
def test_kernels_of_the_unit_use_no_scratch(unit):
    """A unit of the per-label tables compiled for gfx950 (device code only): every kernel's scratch size is 0, every sweep
    keeps its LDS size -- for label_stats' first sweep and the moments sweep the table that gives 7 workgroups per compute
    unit --, no sweep of any label type loses a wave per SIMD, and the topology sweep, the tight one, stays within 256 VGPRs"""
    import re
    import shutil
    import tempfile
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if hipcc is None:
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "euclidean-distance-transform-3d_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                              "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-S",
                              "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(d, "unit.s"),
                              os.path.join(csrc, unit)], capture_output=True, text=True, check=True)
    kernels, lds_of, seven, tight = _UNITS[unit]
    names = re.findall(r"Function Name: (\S+)", res.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", res.stderr)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", res.stderr)]
    waves = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", res.stderr)]
    assert len(names) == len(scratch) == len(lds) == len(vgprs) == len(waves) == kernels, names
    assert scratch == [0] * kernels, dict(zip(names, scratch))
    for sweep, (want, occupancy) in lds_of.items():
        got = [b for n, b in zip(names, lds) if sweep in n]
        assert got == [want] * 7, (sweep, got)                      # one sweep per label type
        assert all(w >= occupancy for n, w in zip(names, waves) if sweep in n), (sweep, dict(zip(names, waves)))
        if sweep in seven:
            assert all(7 * b <= 160 * 1024 for b in got), (sweep, got)
        if sweep in tight:
            assert all(v <= 256 for n, v in zip(names, vgprs) if sweep in n), dict(zip(names, vgprs))


# ---- 3. the ABI's refusals ----------------------------------------------------------------------------------------------
def test_public_surface():
    import edt
    assert "label_moments" in edt.__all__ and callable(edt.label_moments)
    assert edt.LabelMoments._fields == ("labels", "counts", "first", "second", "centroid", "covariance")
    from edt import _lib
    for name in ("edt_hip_label_moments_workspace_bytes", "edt_hip_label_moments_device", "edt_hip_label_moments"):
        assert name in _lib.SIGNATURES and getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]


class _Args:
    """A valid argument set of both entry points over host stand-ins: every case below breaks exactly one item, and
    validation returns before anything is dereferenced.  Outputs and workspace hold a sentinel."""

    def __init__(self, lib):
        self.lib = lib
        self.labels = np.ones(24, dtype=np.uint32)
        self.keys = np.zeros(8, dtype=np.uint32)
        self.counts, self.sums = np.zeros(8, dtype=np.int64), np.zeros(72, dtype=np.int64)
        self.centroid, self.central = np.zeros(24, dtype=np.float64), np.zeros(48, dtype=np.float64)
        self.n = np.zeros(1, dtype=np.int64)
        self.ws = aligned_host_bytes(lib.edt_hip_label_moments_workspace_bytes(U32, 24, 8) + 256)
        self.outs = [self.keys, self.counts, self.sums, self.centroid, self.central, self.n, self.ws]
        for a in self.outs:
            a.view(np.uint8)[:] = SENTINEL

    def untouched(self):
        return all(np.all(a.view(np.uint8) == SENTINEL) for a in self.outs)

    @staticmethod
    def p(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    def device(self, **kw):
        a = dict(labels=self.labels, dtype=U32, ndim=3, sx=4, sy=3, sz=2, max_labels=8, keys=self.keys, counts=self.counts,
                 sums=self.sums, centroid=self.centroid, central=self.central, n=self.n, ws=self.ws[:-256], ws_bytes=None)
        a.update(kw)
        wb = (0 if a["ws"] is None else a["ws"].size) if a["ws_bytes"] is None else a["ws_bytes"]
        p = self.p
        return self.lib.edt_hip_label_moments_device(p(a["labels"]), a["dtype"], a["ndim"], a["sx"], a["sy"], a["sz"], a["max_labels"],
                                                     p(a["keys"]), p(a["counts"]), p(a["sums"]), p(a["centroid"]), p(a["central"]),
                                                     p(a["n"]), p(a["ws"]), wb, None)

    def host(self, **kw):
        a = dict(labels=self.labels, dtype=U32, ndim=3, sx=4, sy=3, sz=2, max_labels=8, keys=self.keys, counts=self.counts,
                 sums=self.sums, centroid=self.centroid, central=self.central, n=self.n)
        a.update(kw)
        p = self.p
        return self.lib.edt_hip_label_moments(p(a["labels"]), a["dtype"], a["ndim"], a["sx"], a["sy"], a["sz"], a["max_labels"],
                                              p(a["keys"]), p(a["counts"]), p(a["sums"]), p(a["centroid"]), p(a["central"]), p(a["n"]))


SHARED_BAD = [
    ("unknown dtype", dict(dtype=7), BAD_ARG), ("negative dtype", dict(dtype=-1), BAD_ARG),
    ("ndim 0", dict(ndim=0), BAD_ARG), ("ndim 4", dict(ndim=4), BAD_ARG),
    ("unused sz", dict(ndim=2), BAD_ARG), ("unused sy", dict(ndim=1, sz=1), BAD_ARG),
    ("negative extent", dict(sx=-4), BAD_ARG),
    ("max_labels 0", dict(max_labels=0), BAD_ARG), ("max_labels negative", dict(max_labels=-3), BAD_ARG),
    ("max_labels beyond 2^38", dict(max_labels=(1 << 38) + 1), BAD_ARG),
    ("null labels", dict(labels=None), BAD_ARG), ("null keys", dict(keys=None), BAD_ARG), ("null counts", dict(counts=None), BAD_ARG),
    ("null sums", dict(sums=None), BAD_ARG), ("null centroid", dict(centroid=None), BAD_ARG),
    ("null central", dict(central=None), BAD_ARG), ("null n_labels", dict(n=None), BAD_ARG),
    ("a line of 2^22 voxels", dict(ndim=1, sx=1 << 22, sy=1, sz=1), UNSUPPORTED),
    ("the range bound in 3-D", dict(sx=1 << 21, sy=2, sz=2), UNSUPPORTED),
]


@pytest.mark.parametrize("what,kw,code", SHARED_BAD, ids=[w for w, _, _ in SHARED_BAD])
def test_both_forms_refuse_bad_arguments_alike(lib, what, kw, code):
    a = _Args(lib)
    for form in (a.device, a.host):
        rc = form(**kw)
        assert rc == code, (what, form.__name__, rc, lib.edt_hip_last_error())
        assert lib.edt_hip_last_error(), what
        assert a.untouched(), (what, form.__name__)
    if code == UNSUPPORTED:
        assert b"2^63" in lib.edt_hip_last_error()


def test_zero_extents_need_no_data(lib):
    """an empty volume passes the argument check with every data pointer NULL: both forms then give the same answer, which
    without a device is that there is none, with nothing written"""
    from edt import _lib
    a = _Args(lib)
    none = dict(labels=None, keys=None, counts=None, sums=None, centroid=None, central=None)
    want = 0 if _lib.device_count() > 0 else _lib.ERR_NO_DEVICE
    for ext in (dict(sx=0), dict(sy=0), dict(sz=0)):
        assert a.device(ws=None, **ext, **none) == want and a.host(**ext, **none) == want, (ext, lib.edt_hip_last_error())
        assert want == 0 or a.untouched()
        assert a.device(n=None, **ext) == BAD_ARG and a.host(n=None, **ext) == BAD_ARG


def test_device_form_refuses_a_missing_short_or_misaligned_workspace(lib):
    a = _Args(lib)
    need = lib.edt_hip_label_moments_workspace_bytes(U32, 24, 8)
    for what, kw in (("no workspace", dict(ws=None)), ("one byte short", dict(ws_bytes=need - 1)),
                     ("workspace of a smaller call", dict(sx=1024, sy=1024, sz=1, ndim=2, max_labels=1 << 16)),
                     ("misaligned by 4", dict(ws=a.ws[4:4 + need])), ("misaligned by 128", dict(ws=a.ws[128:128 + need]))):
        rc = a.device(**kw)
        assert rc == BAD_ARG and lib.edt_hip_last_error(), (what, rc)
        assert (b"256-byte aligned" in lib.edt_hip_last_error()) == what.startswith("misaligned"), (what, lib.edt_hip_last_error())
        assert a.untouched(), what


def test_a_line_of_a_million_voxels_passes_the_argument_check(lib):
    """10^6 * (10^6 - 1)^2 < 2^63: whatever the call then answers (no device here, or success), it is not the range refusal"""
    from edt import _lib
    a = _Args(lib)
    labels = np.zeros(10 ** 6, dtype=np.uint8)
    ws = aligned_host_bytes(lib.edt_hip_label_moments_workspace_bytes(U8, 10 ** 6, 8))
    if _lib.device_count() > 0:
        rc = a.host(labels=labels, dtype=U8, ndim=1, sx=10 ** 6, sy=1, sz=1)
        assert rc == 0 and int(a.n[0]) == 0
    else:
        for rc in (a.device(labels=labels, dtype=U8, ndim=1, sx=10 ** 6, sy=1, sz=1, ws=ws),
                   a.host(labels=labels, dtype=U8, ndim=1, sx=10 ** 6, sy=1, sz=1)):
            assert rc == _lib.ERR_NO_DEVICE, (rc, lib.edt_hip_last_error())


def test_workspace_query(lib):
    q = lib.edt_hip_label_moments_workspace_bytes
    assert q(7, 1000, 10) == 0 and q(-1, 1000, 10) == 0
    assert q(U32, 1000, 0) == 0 and q(U32, 1000, -1) == 0 and q(U32, -1, 10) == 0
    for code in (U8, U16, U32, U64, F32, F64, BOOL):
        sizes = [q(code, 1 << 30, m) for m in (1, 2, 100, 1000, 65536, 1 << 20, 1 << 24)]
        assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes), (code, sizes)
    # direct tables: 88 bytes per slot; hashed tables: at least 2 slots of 88 bytes per label and the 8-byte list entry
    assert 256 * 88 <= q(U8, 1 << 30, 255) < 256 * 88 + 4096 and 65536 * 88 <= q(U16, 1 << 30, 65535) < 65536 * 88 + 4096
    for code in (U32, U64, F32, F64):
        for m in (65536, 1 << 20):
            assert m * (2 * 88 + 8) <= q(code, 1 << 30, m) < 2 * m * (2 * 88 + 8)
    # no more labels than voxels: room beyond that costs nothing
    assert q(U32, 5000, 1 << 30) == q(U32, 5000, 5000)
    # nothing per voxel
    assert q(U32, 1 << 40, 1000) == q(U32, 1 << 20, 1000)


# ---- 4. the Python surface ----------------------------------------------------------------------------------------------
def test_python_argument_checks():
    import edt
    with pytest.raises(TypeError):
        edt.label_moments(np.ones((2, 2, 2, 2), dtype=np.uint8))
    with pytest.raises(TypeError):
        edt.label_moments(np.uint8(3))
    with pytest.raises(TypeError):
        edt.label_moments(np.ones((4, 5), dtype=np.complex64))
    with pytest.raises(ValueError):
        edt.label_moments(np.ones((4, 5), dtype=np.uint16), max_labels=0)
    with pytest.raises(ValueError, match="2\\^63"):
        edt.label_moments(np.zeros(1 << 22, dtype=np.uint8))


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.uint32, np.int64, np.float32, np.float64, bool])
@pytest.mark.parametrize("shape", [(0,), (3, 0), (0, 2, 5)])
def test_empty_input_gives_an_empty_table(dtype, shape):
    import edt
    nd = len(shape)
    got = edt.label_moments(np.zeros(shape, dtype=dtype))
    assert isinstance(got, edt.LabelMoments)
    assert got.labels.dtype == np.dtype(dtype) and got.labels.shape == (0,)
    assert got.counts.dtype == np.int64 and got.counts.shape == (0,)
    assert got.first.dtype == np.int64 and got.first.shape == (0, nd)
    assert got.second.dtype == np.int64 and got.second.shape == (0, nd, nd)
    assert got.centroid.dtype == np.float64 and got.centroid.shape == (0, nd)
    assert got.covariance.dtype == np.float64 and got.covariance.shape == (0, nd, nd)
    lengths2, axes = got.principal()
    assert lengths2.shape == (0, nd) and axes.shape == (0, nd, nd)


def test_abi_columns_map_to_array_axes():
    """edt._moments.assemble: the ABI's x / y / z columns of a C and of an F array end at the array's own axes"""
    from edt import _moments
    lab = blocky_labels((4, 9, 6), nlabels=5, zero_frac=0.2, block=2, rng=np.random.default_rng(24)).astype(np.uint32)
    for data in (lab, np.asfortranarray(lab), lab[1], np.asfortranarray(lab[1]), lab[2, 3]):
        want = oracle.label_moments(data)
        keys, counts, sums, centroid, central = oracle.abi_table(data)
        got = _moments.assemble(keys, counts, sums, centroid, central, data.ndim, not data.flags.f_contiguous)
        oracle.assert_same([np.ascontiguousarray(f) for f in got], want, data.shape)


# ---- 5. principal axes --------------------------------------------------------------------------------------------------
def _table_of(lab):
    from edt import LabelMoments
    return LabelMoments(*oracle.label_moments(lab))


def test_principal_axes_of_an_axis_aligned_box():
    lab = np.zeros((6, 9, 14), dtype=np.uint8)
    lab[2:5, 1:6, 3:12] = 4                               # 3 x 5 x 9 voxels
    for w in (None, (2.0, 0.5, 1.5), (-30.0, 6.0, 6.0)):
        lengths2, axes = _table_of(lab).principal(w)
        ww = np.ones(3) if w is None else np.asarray(w)
        want = np.array([(n * n - 1) / 12 for n in (3, 5, 9)]) * ww ** 2
        order = np.argsort(-want, kind="stable")
        assert lengths2.shape == (1, 3) and axes.shape == (1, 3, 3)
        assert np.allclose(lengths2[0], want[order], rtol=1e-12, atol=0)
        assert np.allclose(np.abs(axes[0]), np.eye(3)[order], rtol=0, atol=1e-12)


def test_principal_axis_of_a_box_on_the_diagonal():
    lab = np.zeros((40, 40, 5), dtype=np.uint16)
    i, j, k = np.indices(lab.shape)
    lab[(np.abs(i - j) <= 2) & (i + j >= 10) & (i + j <= 68) & (k >= 1) & (k <= 3)] = 7   # long along (1, 1, 0)
    lengths2, axes = _table_of(lab).principal()
    assert lengths2[0, 0] > 10 * lengths2[0, 1]
    first = axes[0, 0] * np.sign(axes[0, 0, 0])
    assert np.allclose(first, np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0), rtol=0, atol=1e-12)
    assert np.allclose(np.linalg.norm(axes[0], axis=1), 1.0, rtol=1e-12)


@pytest.mark.parametrize("w", [(1.0, 0.0, 1.0), (1.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0), 0.0])
def test_principal_refuses_bad_voxel_sizes(w):
    lab = np.zeros((3, 4, 5), dtype=np.uint8)
    lab[1:, 1:, 1:] = 1
    with pytest.raises(ValueError):
        _table_of(lab).principal(w)
