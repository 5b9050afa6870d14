"""CPU tests that PIN the oracle (oracle/edt_oracle.c) before anything is compared to it:
against the golden vectors recorded from the reference, the reference's hand-derivable known
answers, the brute-force specification, and -- where available -- the compiled reference."""
import os

import numpy as np
import pytest

from conftest import load_golden
from oracle import spec
from synth import blocky_labels, box_edtsq_closed_form

INF = np.inf
ALL_TYPES = [np.uint8, np.uint16, np.uint32, np.uint64, np.float32, bool]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- golden vectors recorded from the real reference -----------------------------------
def test_golden_random(oracle_port):
    for c in load_golden("edt_random.npz"):
        lab = c["labels"]
        lab = np.asfortranarray(lab) if str(c["order"]) == "F" else np.ascontiguousarray(lab)
        an = tuple(c["anisotropy"])
        an = an[0] if lab.ndim == 1 else an
        bb = bool(c["black_border"])
        assert same(oracle_port.edtsq(lab, an, bb), c["edtsq"])
        assert same(oracle_port.edt(lab, an, bb), c["edt"])


def test_golden_configs(oracle_port):
    for c in load_golden("edt_configs.npz"):
        lab = np.asfortranarray(c["labels"])
        got = oracle_port.edtsq(lab, tuple(c["anisotropy"]), bool(c["black_border"]))
        assert same(got, c["edtsq"])


def test_golden_sdf_voxel_graph(oracle_port):
    for c in load_golden("edt_sdf_voxel_graph.npz"):
        lab, an, bb = c["labels"], tuple(c["anisotropy"]), bool(c["black_border"])
        if str(c["kind"]) == "sdf":
            got = oracle_port.sdf(lab, an, bb)
        else:
            got = oracle_port.edtsq(lab, an, bb, voxel_graph=c["graph"])
        assert same(got, c["out"])


def test_voxel_graph_reads_three_bits_and_no_other(oracle_port):
    """the oracle's field does not move when only the bits the reference ignores change -- everything but 0x01 / 0x04 / 0x10, and
    0x10 too in 2-D --, and does move when one of those it reads is cleared (tests/test_gpu_voxel_graph.py draws whole bytes)"""
    rng = np.random.default_rng(77)
    moved = 0
    for t, shape in enumerate([(9, 7), (1, 12), (14, 3), (6, 5, 7), (1, 8, 4), (11, 4, 5)]):
        read = 0x05 if len(shape) == 2 else 0x15
        lab = (rng.random(shape) < 0.9).astype([np.uint8, np.uint32, np.float32][t % 3])
        lab = np.asfortranarray(lab) if t % 2 else lab
        g = rng.integers(0, 256, size=shape, dtype=np.uint8)
        g = np.asfortranarray(g) if t % 2 else g
        an, bb = ((1.0, 1.0, 1.0), (2.0, 2.0, 3.0))[t % 2][:len(shape)], t % 4 < 2
        want = oracle_port.edtsq(lab, an, bb, voxel_graph=g)
        for other in (g & read, g | (0xFF & ~read), (g & read) | (rng.integers(0, 256, size=shape, dtype=np.uint8) & (0xFF & ~read))):
            other = np.asarray(other, dtype=np.uint8, order="F" if t % 2 else "C")
            assert same(oracle_port.edtsq(lab, an, bb, voxel_graph=other), want), (t, shape)
        if 1 in shape:      # (under a black border across a unit extent every distance is half a voxel already)
            continue
        for bit in (0x01, 0x04, 0x10)[:len(shape)]:
            moved += not same(oracle_port.edtsq(lab, an, bb, voxel_graph=np.asarray(g | read, dtype=np.uint8, order="F" if t % 2 else "C")),
                              oracle_port.edtsq(lab, an, bb, voxel_graph=np.asarray((g | read) & (0xFF & ~bit), dtype=np.uint8,
                                                                                    order="F" if t % 2 else "C")))
    assert moved == 2 + 2 + 3 + 3


# ---- known answers of the reference's own test-suite (automated_test.py) -----------------
@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_one_d_known_answers(oracle_port, dtype):
    # automated_test.py:62-146
    def check(labels, ans, bb, anisotropy=1.0):
        got = oracle_port.edtsq(np.array(labels, dtype=dtype), anisotropy, bb)
        assert same(got, np.array(ans, dtype=np.float32))

    check([1], [1], True)
    check([5 if dtype is not bool else 1], [1], True)
    check([0, 1, 1, 1, 0], [0, 1, 4, 1, 0], True)
    check([1, 1, 1, 1], [1, 4, 4, 1], True)
    check([1, 1, 1, 1], [4, 16, 16, 4], True, anisotropy=2.0)
    check([1], [INF], False)
    check([0, 1, 1, 1, 0], [0, 1, 4, 1, 0], False)
    check([1, 1, 1, 1], [INF, INF, INF, INF], False)
    check([0, 1, 1, 1], [0, 1, 4, 9], False)
    check([1, 1, 1, 0], [9, 4, 1, 0], False)
    if dtype is not bool:
        check([1, 1, 1, 1, 1, 0, 2, 2, 2, 2, 2, 1, 1, 1, 1, 3],
              [1, 4, 9, 4, 1, 0, 1, 4, 9, 4, 1, 1, 4, 4, 1, 1], True)
        check([1, 1, 1, 1, 1, 0, 2, 2, 2, 2, 2, 1, 1, 1, 1, 3],
              [25, 16, 9, 4, 1, 0, 1, 4, 9, 4, 1, 1, 4, 4, 1, 1], False)


def test_two_d_known_answers(oracle_port):
    # identity-like images, automated_test.py:188-230
    lab = np.ones((5, 5), dtype=np.uint32)
    got = oracle_port.edtsq(lab, (1, 1), True)
    want = np.array([[1, 1, 1, 1, 1], [1, 4, 4, 4, 1], [1, 4, 9, 4, 1], [1, 4, 4, 4, 1],
                     [1, 1, 1, 1, 1]], dtype=np.float32)
    assert same(got, want)
    assert np.all(np.isinf(oracle_port.edtsq(lab, (1, 1), False)))
    # label boundary through the middle: each half is its own object
    lab = np.array([[1, 1, 2, 2]] * 4, dtype=np.uint8)
    got = oracle_port.edtsq(lab, (1, 1), False)
    assert same(got, np.array([[4, 1, 1, 4]] * 4, dtype=np.float32))
    # a single background pixel in a field, anisotropy (5, 6) (C order: rows are y)
    lab = np.ones((3, 3), dtype=np.uint16)
    lab[1, 1] = 0
    got = oracle_port.edtsq(lab, (5, 6), False)
    want = np.array([[61, 25, 61], [36, 0, 36], [61, 25, 61]], dtype=np.float32)
    assert same(got, want)


def test_three_d_cube_known_answers(oracle_port):
    # automated_test.py:426-551 style: 3x3x3 cube, centre voxel distances
    lab = np.ones((3, 3, 3), dtype=np.uint32)
    got = oracle_port.edtsq(lab, (4, 4, 4), True)
    assert got[1, 1, 1] == 64 and got[0, 0, 0] == 16 and got[1, 1, 0] == 16
    got = oracle_port.edtsq(lab, (6, 6, 5), True)
    assert got[1, 1, 1] == 100.0  # 2 voxels * 5 along the cheapest axis
    assert same(got, np.ascontiguousarray(box_edtsq_closed_form((3, 3, 3), (6, 6, 5))))


def test_box_closed_form(oracle_port):
    for shape, an in (((17, 9, 23), (6, 6, 30)), ((8, 8, 8), (1, 1, 1)), ((5, 31, 2), (3, 1, 2))):
        lab = np.ones(shape, dtype=np.uint32, order="F")
        assert same(oracle_port.edtsq(lab, an, True), box_edtsq_closed_form(shape, an))


def test_scaling_identity(oracle_port):
    # automated_test.py:632-649: integer anisotropy scales the squared transform exactly
    rng = np.random.default_rng(3)
    lab = blocky_labels((20, 18, 16), nlabels=3, zero_frac=0.3, block=3, rng=rng).astype(np.uint8)
    base = oracle_port.edt(lab, (1, 1, 1), True)
    for w in (2, 7, 149):
        assert same(oracle_port.edt(lab, (w, w, w), True), (w * base).astype(np.float32))


def test_all_inf_and_empty(oracle_port):
    assert np.all(np.isinf(oracle_port.edt(np.ones((6, 5, 4), dtype=np.uint8), (1, 1, 1), False)))
    assert oracle_port.edtsq(np.zeros((0,), dtype=np.uint8)).shape == (0,)
    assert oracle_port.edtsq(np.zeros((3, 0, 2), dtype=np.uint8)).shape == (3, 0, 2)


def test_c_vs_f_order(oracle_port):
    rng = np.random.default_rng(4)
    lab = blocky_labels((13, 21, 8), nlabels=4, zero_frac=0.2, block=3, rng=rng).astype(np.uint32)
    a = oracle_port.edtsq(np.ascontiguousarray(lab), (2, 3, 5), False)
    b = oracle_port.edtsq(np.asfortranarray(lab), (2, 3, 5), False)
    assert same(a, b)


# ---- brute-force specification -------------------------------------------------------------
def test_against_bruteforce_spec(oracle_port):
    rng = np.random.default_rng(11)
    for t in range(40):
        dims = int(rng.integers(1, 4))
        shape = tuple(int(rng.integers(1, 13)) for _ in range(dims))
        lab = blocky_labels(shape, nlabels=3, zero_frac=0.3, block=int(rng.integers(1, 4)), rng=rng)
        lab = np.asfortranarray(lab.astype(np.uint16))
        an = [(1, 1, 1), (6, 6, 30), (0.5, 0.7, 1.3), (2, 1, 3)][t % 4][:dims]
        bb = bool(t % 2)
        want = spec.edtsq_xfast(lab, an, bb)
        got = oracle_port.edtsq(lab, an[0] if dims == 1 else an, bb)
        assert same(got, want), (t, shape, an, bb)


# ---- the compiled reference itself -----------------------------------------------------------
def test_against_compiled_reference(oracle_port, oracle_ref):
    rng = np.random.default_rng(12)
    dtypes = [np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64, bool, np.int16]
    for t in range(120):
        dims = int(rng.integers(1, 4))
        shape = tuple(int(rng.integers(1, 48)) for _ in range(dims))
        lab = blocky_labels(shape, nlabels=int(rng.integers(1, 9)), zero_frac=float(rng.random() * 0.5),
                            block=int(rng.integers(1, 7)), rng=rng).astype(dtypes[t % len(dtypes)])
        if t % 3 == 0:
            lab = np.asfortranarray(lab)
        an = [(1, 1, 1), (6, 6, 30), (0.5, 0.7, 1.3), (4, 4, 40), (1e-3, 2.5, 7)][t % 5][:dims]
        an = an[0] if dims == 1 else an
        bb = bool(rng.integers(0, 2))
        assert same(oracle_port.edtsq(lab, an, bb), oracle_ref.edtsq(lab, an, bb, parallel=1 + t % 2))


def _in_fresh_process(call):
    """Run ``test_oracle.<call>`` in a child interpreter.  For anything that loads the reference built with -ffast-math:
    that library turns on flush-to-zero / denormals-are-zero for the whole process it is loaded into, and every later
    computation on denormal labels -- the oracle's and the compiled reference's alike -- would read them as 0."""
    import subprocess
    import sys
    from conftest import ROOT
    code = f"import numpy as np, test_oracle; test_oracle.{call}; print('child ok')"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tests"), ROOT]))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert res.returncode == 0 and "child ok" in res.stdout, res.stdout + res.stderr


def denormals_are_honoured():
    """False once a -ffast-math library has put this process into denormals-are-zero mode."""
    return bool(np.array([1e-45], dtype=np.float32)[0] != 0) and bool(np.array([5e-324])[0] != 0)


def _fast_math_twin():
    from oracle import harness
    strict, fast = harness.ref(), harness.ref(fast=True)
    rng = np.random.default_rng(13)
    lab = np.asfortranarray(blocky_labels((40, 36, 28), 12, 0.1, 5, rng).astype(np.uint32))
    for an, bb in (((6, 6, 30), True), ((0.5, 0.7, 1.3), False)):
        assert same(strict.edtsq(lab, an, bb), fast.edtsq(lab, an, bb))


def test_reference_fast_math_twin_agrees(oracle_ref):
    # the setup.py-flag build and the strict build agree bit-for-bit (in a child process: see _in_fresh_process)
    _in_fresh_process("_fast_math_twin()")
    assert denormals_are_honoured()


def test_binary_route_against_compiled_reference(oracle_port, oracle_ref):
    # pyedt::_binary_edt{2,3}dsq<T> for multi-valued non-bool T (src/edt.hpp:487-576, :681-732): labels split runs in
    # pass 1 only; it differs from the multi-label transform as soon as two non-zero labels touch along y or z
    rng = np.random.default_rng(21)
    dtypes = [np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64, bool]
    differs = 0
    for t in range(84):
        dims = 2 + t % 2
        shape = tuple(int(rng.integers(1, 40)) for _ in range(dims))
        lab = blocky_labels(shape, nlabels=int(rng.integers(1, 6)), zero_frac=float(rng.random() * 0.5),
                            block=int(rng.integers(1, 7)), rng=rng).astype(dtypes[t % len(dtypes)])
        if t % 3 == 0:
            lab = np.asfortranarray(lab)
        an = [(1, 1, 1), (6, 6, 30), (0.5, 0.7, 1.3), (4, 4, 40)][t % 4][:dims]
        bb = bool(rng.integers(0, 2))
        want = oracle_ref.binary_edtsq(lab, an, bb, parallel=1 + t % 2)
        assert same(oracle_port.binary_edtsq(lab, an, bb), want), (t, shape, an, bb)
        differs += not same(want, oracle_ref.edtsq(lab, an, bb))
    assert differs > 10  # the case the facade used to get wrong is really exercised


# ---- labels across each dtype's full value range (synth.palette_labels) ---------------------------------------------------
PALETTE_DTYPES = [np.uint64, np.int64, np.uint32, np.int32, np.uint16, np.int16, np.uint8, np.int8, np.float64,
                  np.float32, bool]


@pytest.mark.parametrize("dtype", PALETTE_DTYPES)
def test_palette_labels_against_compiled_reference(oracle_port, oracle_ref, dtype):
    """The oracle port equals the compiled reference bit for bit on labels that differ only beyond a narrowing: every
    border rule, C / F order, 1-/2-/3-D, an integer and a non-integer voxel size; sdf and the binary route too."""
    from synth import palette_labels
    # (1e-45 / 5e-324 are labels here: they must not be read as 0 by both checkers at once)
    assert denormals_are_honoured(), "denormals-are-zero is on in the test process: a -ffast-math library was loaded"
    rng = np.random.default_rng(31 + PALETTE_DTYPES.index(dtype))
    for dims, shape in ((1, (157,)), (2, (37, 29)), (3, (23, 19, 17))):
        for order in "CF":
            lab = palette_labels(shape, dtype, rng=rng, block=int(rng.integers(1, 5)), order=order)
            for an in ((2.0, 1.0, 3.0), (0.5, 0.7, 1.3)):
                an = an[0] if dims == 1 else an[:dims]
                for bb in (False, True):
                    want = oracle_ref.edtsq(lab, an, bb)
                    assert same(oracle_port.edtsq(lab, an, bb), want), (dims, order, an, bb)
                    if dims > 1:
                        assert same(oracle_port.sdf(lab, an, bb), oracle_ref.sdf(lab, an, bb)), (dims, order, an, bb)
                        assert same(oracle_port.binary_edtsq(lab, an, bb), oracle_ref.binary_edtsq(lab, an, bb))


def _narrowing_guard(dtype):
    from oracle import harness
    from synth import narrowed, palette_labels
    ref = harness.ref()
    rng = np.random.default_rng(41)
    differs = 0
    for t in range(6):
        shape = ((40, 36, 28), (64, 48), (300,))[t % 3]
        lab = palette_labels(shape, dtype, rng=rng, block=3, order="CF"[t % 2])
        nar = narrowed(lab)
        assert nar.dtype == lab.dtype and nar.shape == lab.shape
        an = 1.0 if len(shape) == 1 else (1.0,) * len(shape)
        for bb in (False, True):
            differs += not same(ref.edtsq(lab, an, bb), ref.edtsq(nar, an, bb))
    assert differs == 12, differs
    if dtype == np.float32:  # the denormal alone (1e-45 flushed to 0) already changes the answer
        lab = palette_labels((40, 36, 28), dtype, rng=rng, block=3)
        den = np.where(lab.view(np.uint32) == 1, np.float32(0), lab)
        assert (lab.view(np.uint32) == 1).any() and not same(ref.edtsq(lab, (1, 1, 1), False),
                                                             ref.edtsq(den, (1, 1, 1), False))


@pytest.mark.parametrize("dtype", ["uint64", "int64", "uint32", "int32", "uint16", "int16", "float64", "float32"])
def test_palettes_tell_narrowed_labels_apart(oracle_ref, dtype):
    """Discrimination guard: on every palette volume the reference's answer changes when the labels are narrowed (low
    half of the bits, float64 -> float32, float32 denormals -> 0).  A GPU test on these volumes therefore fails for a
    kernel that compares narrowed labels; keep it so when a palette changes.  (In a fresh process, like every check
    whose answer depends on denormal labels: see _in_fresh_process.)"""
    _in_fresh_process(f"_narrowing_guard(np.{dtype})")


def _fixture_order(c):
    lab = c["labels"]
    return np.asfortranarray(lab) if str(c["order"]) == "F" else np.ascontiguousarray(lab)


def test_golden_label_values(oracle_port):
    """tests/golden/edt_label_values.npz (the reference's Python module on palette volumes of every dtype it takes)."""
    kinds = set()
    for n, c in enumerate(load_golden("edt_label_values.npz")):
        lab, kind, bb = _fixture_order(c), str(c["kind"]), bool(c["black_border"])
        an = tuple(c["anisotropy"])
        an = an[0] if lab.ndim == 1 else an
        kinds.add(kind)
        if kind == "edtsq":
            assert same(oracle_port.edtsq(lab, an, bb), c["edtsq"]), n
            assert same(oracle_port.edt(lab, an, bb), c["edt"]), n
        elif kind == "sdf":
            assert same(oracle_port.sdf(lab, an, bb), c["out"]), n
        elif kind == "voxel_graph":
            assert same(oracle_port.edtsq(lab, an, bb, voxel_graph=c["graph"]), c["out"]), n
    assert kinds == {"edtsq", "sdf", "voxel_graph", "each"}


def test_golden_label_values_each():
    """The host-side edt.each over palette labels against the reference's each() (no GPU: it only slices dt)."""
    import edt
    count = 0
    for c in load_golden("edt_label_values.npz"):
        if str(c["kind"]) != "each":
            continue
        lab = _fixture_order(c)
        got = list(edt.each(lab, c["dt"]))
        assert len(got) == len(c["keys"])
        for (k, img), want_k, want in zip(got, c["keys"].tolist(), c["images"]):
            assert k == want_k and same(img, want), (lab.dtype, k, want_k)
        count += 1
    assert count >= 8
