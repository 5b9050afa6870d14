"""The case table of the signed transform's structure families: tests/test_gpu_signed.py runs it on the GPU, tests/
test_signed_cases_cpu.py holds it against the library's host proof (edt_hip_q16_no_refusals) without one.

A row is (family, shape, sizes, black_border, expect_fused, quantum, volumes, modes, conditions).  All arrays are F-ordered
(sx, sy, sz): x is the fastest axis.  The label types uint8, uint16, uint32, uint64, float32, bool rotate over the rows.

expect_fused is WRITTEN HERE BY HAND: True where the sign must be the epilogue of the last integer pass (no pass named "sign"
in the pass log), False where it must be a pass of its own.  It is what the host's proof says for the row's (shape, sizes,
border) together with sx % 4 == 0 and sy, sz >= 97; a row whose route silently changes fails.  Where the proof disagreed with
what the rows were first written with, the proof won:

  * (36, 100, 1000) at (6, 6, 30) without a black border: pass Z is NOT proven (rows without a boundary carry +inf into a
    column of 1000 rows at a = 25) -- not fused;
  * (64, 128, 100) at (6, 6, 30) without a black border is not in the table of tests/test_gpu_plain_rows.py; the proof holds
    -- fused;
  * (1100, 100, 97) and (2052, 100, 97) with a black border: the proof holds at every size used here -- fused.

quantum is the largest q of which every squared voxel size is an integer multiple (the CPU tier checks that arithmetic); the
integer kernel counts in units of q, 16-bit lanes hold values up to 65535 of them."""
from collections import namedtuple

import numpy as np

from synth import blocky_labels
from test_gpu_plain_rows import alternating, box, striped

DTYPES = [np.uint8, np.uint16, np.uint32, np.uint64, np.float32, bool]

KEEP_PLANES, NO_SHORT_CUTS, FP32_PLANE, FP32_KERNELS = 0x400, 0x80, 0x10000000, 0x8000000
WIDE_ALL, NO_WIDE, FP32_ROWS = 0x40000000, 0x20000000, 0x100000
SIGN_AS_A_PASS = (KEEP_PLANES, FP32_KERNELS)   # the modes under which the pass log must show "sign" whatever the row says

Case = namedtuple("Case", "family shape an bb fused q volumes modes cond dtype")


def _fg(shape):
    return np.full(shape, 3, dtype=np.uint32, order="F")


def all_fg(shape):
    return _fg(shape)


def all_bg(shape):
    return np.zeros(shape, dtype=np.uint32, order="F")


def bg_one_fg_voxel(shape):
    lab = all_bg(shape)
    lab[tuple(s // 2 for s in shape)] = 3
    return lab


def fg_one_bg_voxel(shape):
    lab = _fg(shape)
    lab[tuple(s // 2 for s in shape)] = 0
    return lab


def bg_y_low(shape):
    """background for y < sy // 3: rows without a boundary along x everywhere, run starts along y alone"""
    lab = _fg(shape)
    lab[:, : shape[1] // 3] = 0
    return lab


def bg_z_high(shape):
    """background for z >= sz // 2: nothing but +inf behind passes X and Y, both labels resolved by pass Z alone"""
    lab = _fg(shape)
    lab[:, :, shape[2] // 2:] = 0
    return lab


def bg_corner(shape):
    lab = _fg(shape)
    lab[: shape[0] // 2, : shape[1] // 2, : shape[2] // 2] = 0
    return lab


def bg_x_slab(shape):
    """background for x >= sx - 5: finite along x, flat along y and z"""
    lab = _fg(shape)
    lab[shape[0] - 5:] = 0
    return lab


def fg_box(shape):
    """a box of label 1 strictly inside a background (tests/test_gpu_plain_rows.py: box)"""
    return box(shape)


def bg_box(shape):
    """its complement: a box of background strictly inside label 1"""
    return np.asfortranarray((box(shape) == 0).astype(np.uint32))


def blocky60(shape):
    return np.asfortranarray(blocky_labels(shape, nlabels=3, zero_frac=0.45, block=60, rng=np.random.default_rng(sum(shape))).astype(np.uint32))


def blocky12(shape):
    return np.asfortranarray(blocky_labels(shape, nlabels=3, zero_frac=0.45, block=12, rng=np.random.default_rng(sum(shape))).astype(np.uint32))


VOLUMES = {f.__name__: f for f in (all_fg, all_bg, bg_one_fg_voxel, fg_one_bg_voxel, bg_y_low, bg_z_high, bg_corner, bg_x_slab,
                                   fg_box, bg_box, striped, alternating, blocky60, blocky12)}
ONE_SIGN_BY_NAME = ("all_fg", "all_bg")   # the volumes that are "all foreground" / "all background" by name: one sign only


def make(name, shape, dtype):
    """the volume `name` of a row, in the row's label type (bool: label != 0), F-ordered"""
    lab = VOLUMES[name](tuple(shape))
    return np.asfortranarray(lab != 0 if np.dtype(dtype) == np.bool_ else lab.astype(dtype))


INF_VOLUMES = ("all_fg", "all_bg", "bg_one_fg_voxel", "fg_one_bg_voxel", "bg_y_low", "bg_z_high", "bg_corner", "bg_x_slab")
FLAT_VOLUMES = ("all_fg", "fg_box", "bg_box", "striped", "alternating")
ONE, ANISO, DEEP = (1.0, 1.0, 1.0), (6.0, 6.0, 30.0), (1.0, 12.0, 12.0)
INF_MODES = (KEEP_PLANES, NO_SHORT_CUTS, FP32_PLANE, FP32_KERNELS)
WIDE_MODES = (KEEP_PLANES, WIDE_ALL, NO_WIDE, FP32_ROWS, FP32_KERNELS)
LONG_MODES = (KEEP_PLANES, FP32_PLANE, FP32_KERNELS)
NEVER_MODES = (FP32_KERNELS, FP32_ROWS)

# (family, shape, sizes, black_border, expect_fused, quantum, volumes, modes, conditions)
_ROWS = [
    # a. volumes of +-inf: no border, fused; the second shape has partial tiles
    ("inf", (64, 128, 100), ONE, False, True, 1.0, INF_VOLUMES, INF_MODES, ("inf",)),
    ("inf", (68, 100, 97), ONE, False, True, 1.0, INF_VOLUMES, INF_MODES, ("inf",)),
    # b. tiles without structure, both border rules; 512 with a border has the marked middle column (`redo`)
    ("flat", (64, 128, 100), ONE, False, True, 1.0, FLAT_VOLUMES, INF_MODES, ()),
    ("flat", (64, 128, 100), ONE, True, True, 1.0, FLAT_VOLUMES, INF_MODES, ()),
    ("flat", (64, 128, 100), ANISO, False, True, 36.0, FLAT_VOLUMES, INF_MODES, ()),
    ("flat", (64, 128, 100), ANISO, True, True, 36.0, FLAT_VOLUMES, INF_MODES, ()),
    ("flat", (512, 100, 97), ANISO, True, True, 36.0, FLAT_VOLUMES, INF_MODES, ()),
    # c. wide lanes and rows of two and four waves, with a border.  "wide_x": pass X leaves more than 65535 quanta on BACKGROUND
    # rows (what the axes of 100 and 97 rows allow at (1, 1, 1) and (6, 6, 30): |sdfsq| <= (wy * sy / 2)^2 = 2500 / 90000 units
    # there, 2500 quanta either way, so no final value leaves 16 bits).  "wide_final": sizes (1, 12, 12) on the same shapes, at
    # which a NEGATIVE sdfsq value itself exceeds 65535 quanta -- pass Z's wide lanes then sign finite values.
    ("wide", (600, 100, 97), ONE, True, True, 1.0, ("fg_box", "bg_box"), WIDE_MODES, ("wide_x",)),
    ("wide", (600, 100, 97), ANISO, True, True, 36.0, ("fg_box", "bg_box"), WIDE_MODES, ("wide_x",)),
    ("wide", (1100, 100, 97), ONE, True, True, 1.0, ("fg_box", "bg_box"), WIDE_MODES, ("wide_x",)),
    ("wide", (1100, 100, 97), DEEP, True, True, 1.0, ("fg_box", "bg_box"), WIDE_MODES, ("wide_x", "wide_final")),
    ("wide", (2052, 100, 97), ONE, True, True, 1.0, ("fg_box", "bg_box"), WIDE_MODES, ("wide_x",)),
    ("wide", (2052, 100, 97), DEEP, True, True, 1.0, ("fg_box", "bg_box"), WIDE_MODES, ("wide_x", "wide_final")),
    # d. long column axes: 32 bands, workgroups of 512 threads, list tiles of 16 columns
    ("long", (36, 1000, 100), ONE, False, True, 1.0, ("blocky60", "bg_y_low"), LONG_MODES, ("long_y",)),
    ("long", (36, 1000, 100), ONE, True, True, 1.0, ("blocky60", "bg_y_low"), LONG_MODES, ("long_y",)),
    ("long", (36, 100, 1000), ANISO, False, False, 36.0, ("blocky60", "bg_y_low"), LONG_MODES, ("long_z",)),
    ("long", (36, 100, 1000), ANISO, True, True, 36.0, ("blocky60", "bg_y_low"), LONG_MODES, ("long_z",)),
    # e. supported, never fused: sx % 4 != 0; no quantum; two dimensions; and the proof failing on the VALUES (rows of 212 voxels
    # at a voxel size of 40 without a border: k^2 * 1600 beyond 2^24), shrunk along y and z to the integer kernel's smallest axes
    ("never", (66, 100, 97), ONE, False, False, 1.0, ("blocky12", "bg_y_low"), NEVER_MODES, ()),
    ("never", (66, 100, 97), ONE, True, False, 1.0, ("blocky12", "bg_y_low"), NEVER_MODES, ()),
    ("never", (64, 128, 100), (0.7, 1.3, 2.0), False, False, None, ("blocky12", "bg_y_low"), NEVER_MODES, ()),
    ("never", (64, 128, 100), (0.7, 1.3, 2.0), True, False, None, ("blocky12", "bg_y_low"), NEVER_MODES, ()),
    ("never", (128, 200), (1.0, 2.0), False, False, 1.0, ("blocky12", "bg_y_low"), NEVER_MODES, ()),
    ("never", (128, 200), (1.0, 2.0), True, False, 1.0, ("blocky12", "bg_y_low"), NEVER_MODES, ()),
    ("never", (600, 130), (1.0, 1.0), False, False, 1.0, ("blocky12", "bg_y_low"), NEVER_MODES, ()),
    ("never", (600, 130), (1.0, 1.0), True, False, 1.0, ("blocky12", "bg_y_low"), NEVER_MODES, ()),
    ("never", (212, 97, 97), (40.0, 2.0, 3.0), False, False, 1.0, ("blocky12", "bg_y_low"), NEVER_MODES, ("proof_fails",)),
]
CASES = [Case(*row, DTYPES[i % len(DTYPES)]) for i, row in enumerate(_ROWS)]

# h. the padded plane: these two volumes again with EDT_HIP_PLANE_PAD_BYTES = 8 and 4096
PADDED = [(CASES[0], "bg_z_high"), (CASES[2], "fg_box")]
PADS = (8, 4096)

# f. the sign as a pass of its own past one trip of its grid (csrc/edt_generic.hip: 16384 blocks x 256 threads x 4 voxels)
TRIP_VOXELS = 16384 * 256 * 4
BIG_SHAPE = (257, 257, 255)

# g. shapes the one-transform form does not serve: rows beyond the wave kernel, a 2-D axis beyond the in-place column kernels, a line
UNSUPPORTED = [((4100, 8, 5), (1.0, 1.0, 1.0)), ((5, 33000), (1.0, 2.0)), ((5000,), (1.0,))]


def case_id(c):
    return "{}-{}-{}-{}".format(c.family, "x".join(str(s) for s in c.shape), "x".join("%g" % a for a in c.an), "border" if c.bb else "open")
