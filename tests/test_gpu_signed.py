"""GPU tier: the signed transform (sdf / sdfsq as ONE transform, EDT_FLAG_SIGNED) on the structure families of the unsigned one.

The signed route has code of its own in pass X (csrc/edt_rowwave.hip: zero_label -- label 0 measured like a label, the
foreground plane all ones or the truth), in the transposer (the true label != 0 bits carried to the z axis), twice in the
integer column kernel's epilogue (csrc/edt_colq16.hip: the packed 16-bit lanes and the 32-bit lanes that carry values beyond
16 bits and +inf; both short cuts -- "tile without structure", "tile of nothing but +inf" -- are off under kEpiSign), and as a
pass of its own wherever the host cannot prove that both column passes stay on the integer kernel (csrc/edt_generic.hip:
k_negate_background).  The families (tests/signed_cases.py, held against the host proof by tests/test_signed_cases_cpu.py):

  a. volumes of +-inf without a border -- every tile behind pass X, or behind passes X and Y, is nothing but +inf and has to
     leave through the wide lanes, negated where the label is 0, with its short cut off;
  b. tiles without structure (boxes, stripes), both border rules, the marked middle column of rows of 512 (`redo`);
  c. values beyond 16 bits and rows of two and four waves;
  d. column axes of 1000 rows;
  e. shapes that are served but never fused (sx % 4 != 0, no quantum, 2-D, values that defeat the proof);
  f. the sign pass past one trip of its capped grid, into an output off the 16-byte grid;
  g. shapes the one-transform form refuses (the two-transform composition);
  h. a padded plane.

Every comparison is bit for bit (np.array_equal / torch.equal) with the oracle's edt(x) - edt(x == 0) and with this library's
two-transform composition, under the default form selection and under the form bits of the row.  Whether the sign was fused is
read from the pass log and compared with the route the table states by hand.  Every case first shows ON THE ORACLE'S RESULT
that it reaches what it is named for.

Two readings of the conditions, both forced by the transform itself:
  * a result holds +inf or -inf only if the whole volume is one label (a voxel is infinite only if its column, every row of
    that column's plane and so on span the volume), so "-inf on a tenth of the voxels and +inf too" is asserted over the
    volumes of a row of family a together (the all-background volume is one of eight), and every volume that is named for
    rows of +inf shows them on its labels: at least a tenth of its voxels lie in background rows without a boundary along x;
  * on axes of 100 and 97 rows no |sdfsq| exceeds (wy * sy / 2)^2 = 2500 quanta at (1, 1, 1) and (6, 6, 30), so at those sizes
    family c shows its values beyond 16 bits where they are: behind pass X, on a background row in one volume and on a
    foreground row in the other (the oracle's 1-D transform); the rows at (1, 12, 12) add the condition as stated -- a
    negative sdfsq value beyond 65535 quanta in the final result, so that pass Z's wide lanes sign finite values."""
import ctypes

import numpy as np
import pytest

import signed_cases as sc
from synth import blocky_labels, offset_out, outside_intact

pytestmark = pytest.mark.gpu

NAN = 0x7FC0BEEF


def lib():
    from edt import _lib
    return _lib.load()


def to_device(lab):
    """an F-ordered (sx, sy, sz) array as the C-ordered device tensor (z, y, x) of the same memory"""
    import torch
    a = np.ascontiguousarray(lab.T)
    if a.dtype.kind == "u" and a.dtype.itemsize > 1:
        a = a.view(f"i{a.dtype.itemsize}")
    return torch.from_numpy(a).cuda()


def host(t):
    return t.cpu().numpy().T


def pass_names(fn):
    import torch
    from edt import device
    device.set_profiling(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [n for n, _ in device.pass_times()]
    finally:
        device.set_profiling(False)
    return out, names


def oracle_pair(oracle_port, lab, an, bb):
    return oracle_port.sdfsq(lab, an, bb), oracle_port.sdf(lab, an, bb)


def signed_check(edt_gpu, oracle_port, lab, an, bb, expect_fused, modes, want=None, what=""):
    """sdfsq / sdf of `lab` (F-ordered) through the host module and on a device tensor, against the oracle and against the
    two-transform composition, under mode 0 and every mode of `modes`; the route from the pass log against `expect_fused`"""
    import torch
    from edt import device
    wantsq, wantrt = oracle_pair(oracle_port, lab, an, bb) if want is None else want
    t = to_device(lab)
    rev = tuple(an[::-1])
    L = lib()
    try:
        for mode in (0,) + tuple(modes):
            L.edt_hip_set_debug_mode(mode)
            tag = (what, lab.shape, lab.dtype.name, an, bb, hex(mode))
            got = edt_gpu.sdfsq(lab, anisotropy=an, black_border=bb)
            assert np.array_equal(got, wantsq), (tag, "sdfsq", int((got != wantsq).sum()))
            got = edt_gpu.sdf(lab, anisotropy=an, black_border=bb)
            assert np.array_equal(got, wantrt), (tag, "sdf", int((got != wantrt).sum()))
            if mode in (0,) + sc.SIGN_AS_A_PASS:
                dsq, names = pass_names(lambda: device.sdfsq(t, anisotropy=rev, black_border=bb))
                if mode == 0:
                    assert ("sign" not in names) == bool(expect_fused), (tag, names)
                    if expect_fused:
                        assert names == ["x_pass", "y_pass", "z_bits", "z_pass"], (tag, names)
                else:
                    assert "sign" in names, (tag, names)
            else:
                dsq = device.sdfsq(t, anisotropy=rev, black_border=bb)
            drt = device.sdf(t, anisotropy=rev, black_border=bb)
            assert np.array_equal(host(dsq), wantsq), (tag, "device.sdfsq", int((host(dsq) != wantsq).sum()))
            assert np.array_equal(host(drt), wantrt), (tag, "device.sdf", int((host(drt) != wantrt).sum()))
            assert torch.equal(dsq, device._signed(t, rev, bb, sqrt=False, one_transform=False)), (tag, "two transforms, sdfsq")
            assert torch.equal(drt, device._signed(t, rev, bb, sqrt=True, one_transform=False)), (tag, "two transforms, sdf")
    finally:
        L.edt_hip_set_debug_mode(0)


def rows_of_inf_share(lab):
    """the share of voxels in BACKGROUND rows (along x) without a boundary: +inf behind pass X without a border"""
    plain = (lab == lab[:1]).all(axis=0) & (lab[0] == 0)
    return float(plain.mean())


def conditions(oracle_port, case, name, lab, wantsq):
    """what the case is named for, on the oracle's result (and, for structure behind pass X, on the labels and the oracle's 1-D
    transform); called before the library is"""
    tag = (sc.case_id(case), name)
    if name not in sc.ONE_SIGN_BY_NAME:
        assert (wantsq < 0).any() and (wantsq > 0).any(), tag
    if "inf" in case.cond and name in ("all_bg", "bg_one_fg_voxel", "bg_y_low", "bg_z_high"):
        assert rows_of_inf_share(lab) >= 0.1, (tag, rows_of_inf_share(lab))
    if "inf" in case.cond and name == "bg_corner":
        # (the corner's own rows end at sx // 2: here the rows of +inf are the foreground's, next to finite background rows)
        assert float((lab == lab[:1]).all(axis=0).mean()) >= 0.5 and rows_of_inf_share(lab) == 0.0, tag
    if "wide_x" in case.cond:
        # the x-row through the volume's corner and the one through its middle, as the oracle's signed 1-D transform, in quanta
        rows = [lab[:, 0, 0], lab[:, lab.shape[1] // 2, lab.shape[2] // 2]]
        x = np.concatenate([oracle_port.sdfsq(np.ascontiguousarray(r), case.an[0], case.bb) for r in rows]) / case.q
        if name == "fg_box":
            assert x.min() < -65535, (tag, x.min())     # the background around the box: whole rows of label 0
        else:
            assert x.max() > 65535, (tag, x.max())      # the foreground around the box of background
    if "wide_final" in case.cond:
        if name == "bg_box":
            assert wantsq.min() / case.q < -65535, (tag, wantsq.min())
        else:
            assert wantsq.max() / case.q > 65535, (tag, wantsq.max())
    for cond, axis in (("long_y", 1), ("long_z", 2)):
        if cond in case.cond:
            assert lab.shape[axis] > 512
            far = np.take(wantsq, np.arange(512, lab.shape[axis]), axis=axis)
            # (the half space y < sy // 3 ends before row 512 of a long y axis: there its foreground is what lies beyond)
            if name == "bg_y_low" and axis == 1:
                assert (far > 0).any(), tag
            else:
                assert (far < 0).any() and (far > 0).any(), tag


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_signed_families(edt_gpu, oracle_port, case):
    neg_inf = pos_inf = total = 0
    todo = []
    for name in case.volumes:
        lab = sc.make(name, case.shape, case.dtype)
        want = oracle_pair(oracle_port, lab, case.an, case.bb)
        conditions(oracle_port, case, name, lab, want[0])
        neg_inf += int(np.isneginf(want[0]).sum())
        pos_inf += int(np.isposinf(want[0]).sum())
        total += lab.size
        todo.append((name, lab, want))
    if "inf" in case.cond:
        assert neg_inf * 10 >= total and pos_inf > 0, (sc.case_id(case), neg_inf, pos_inf, total)
    for name, lab, want in todo:
        signed_check(edt_gpu, oracle_port, lab, case.an, case.bb, case.fused, case.modes, want=want, what=name)


@pytest.mark.parametrize("pad", sc.PADS)
def test_signed_padded_plane(edt_gpu, oracle_port, pad, monkeypatch):
    """h. the index buffer / 16-bit plane with its slices further apart than sx * sy elements (EDT_HIP_PLANE_PAD_BYTES, read per
    plan): the volume that pass Z alone resolves, and the box, through the signed epilogue"""
    monkeypatch.setenv("EDT_HIP_PLANE_PAD_BYTES", str(pad))
    with_pad = lib().edt_hip_workspace_bytes_flags(0, 3, 64, 128, 100, 0)
    monkeypatch.setenv("EDT_HIP_PLANE_PAD_BYTES", "0")
    assert with_pad - lib().edt_hip_workspace_bytes_flags(0, 3, 64, 128, 100, 0) >= 100 * (pad & ~7) - 4096
    monkeypatch.setenv("EDT_HIP_PLANE_PAD_BYTES", str(pad))
    # (edt.device keeps one plan = one workspace per shape; one sized under another pad is too small for the index buffer, and the
    # call then runs without the index form -- correct, but not the route under test)
    from edt import device
    device._plans.clear()
    try:
        for case, name in sc.PADDED:
            lab = sc.make(name, case.shape, case.dtype)
            want = oracle_pair(oracle_port, lab, case.an, case.bb)
            conditions(oracle_port, case, name, lab, want[0])
            signed_check(edt_gpu, oracle_port, lab, case.an, case.bb, case.fused, case.modes, want=want, what=(name, "pad", pad))
    finally:
        device._plans.clear()


@pytest.mark.parametrize("shape,an", sc.UNSUPPORTED, ids=lambda v: "x".join(str(s) for s in v) if isinstance(v[0], int) else None)
def test_signed_two_transform_fallback(edt_gpu, oracle_port, shape, an):
    """g. shapes the one-transform form does not serve: both layers fall back to edt(x) - edt(x == 0)"""
    import torch
    from edt import _lib, device
    rng = np.random.default_rng(sum(shape))
    for i, dtype in enumerate((np.uint8, np.uint32, np.float32)):
        lab = np.asfortranarray(blocky_labels(shape, nlabels=4, zero_frac=0.45, block=7, rng=rng).astype(dtype))
        code = {np.uint8: _lib.U8, np.uint32: _lib.U32, np.float32: _lib.F32}[dtype]
        if len(shape) > 1:
            ext = tuple(shape) + (1,) * (3 - len(shape))
            assert lib().edt_hip_signed_supported(code, len(shape), *ext, 0) == 0, shape
        for bb in (True, False):
            a = an[0] if len(shape) == 1 else an
            wantsq, wantrt = oracle_pair(oracle_port, lab, a, bb)
            assert (wantsq < 0).any() and (wantsq > 0).any()
            assert np.array_equal(edt_gpu.sdfsq(lab, anisotropy=a, black_border=bb), wantsq), (shape, dtype, bb, "sdfsq")
            assert np.array_equal(edt_gpu.sdf(lab, anisotropy=a, black_border=bb), wantrt), (shape, dtype, bb, "sdf")
            t = to_device(lab)
            dsq, names = pass_names(lambda: device.sdfsq(t, anisotropy=tuple(an[::-1]), black_border=bb))
            assert "sign" not in names, (shape, names)   # (two transforms and a subtraction: no signed transform ran)
            assert np.array_equal(host(dsq), wantsq), (shape, dtype, bb, "device.sdfsq")
            assert np.array_equal(host(device.sdf(t, anisotropy=tuple(an[::-1]), black_border=bb)), wantrt), (shape, dtype, bb, "device.sdf")
            assert torch.equal(dsq, device._signed(t, tuple(an[::-1]), bb, sqrt=False, one_transform=False))


def test_signed_sign_pass_past_one_trip(edt_gpu, oracle_port):
    """f. k_negate_background (csrc/edt_generic.hip) on 257 x 257 x 255 = 16 842 495 voxels: its grid is capped at 16384 blocks of
    256 threads of 4 voxels, so the quads behind voxel 16 777 216 are the stride loop's second trip; the output lies 16 + 3
    floats behind a 256-byte boundary, so one voxel precedes the first 16-byte boundary (the head) and two are left behind
    the last whole quad (the tail).  Rows of 257 voxels are no whole granules: the sign is a pass of its own, which the pass log
    shows.  sdf and sdfsq, the buffer around the output intact.  (The oracle needs about 1.5 s for both here: the volume
    keeps its full size and the second-trip claim stands.)"""
    import torch
    from edt import _lib, device
    shape = sc.BIG_SHAPE
    sx, sy, sz = shape
    n = sx * sy * sz
    lab = np.asfortranarray(blocky_labels(shape, nlabels=3, zero_frac=0.45, block=40, rng=np.random.default_rng(5)).astype(np.uint8))
    wantsq, wantrt = oracle_pair(oracle_port, lab, (1.0, 1.0, 1.0), True)
    flat = wantsq.reshape(-1, order="F")
    assert (flat[sc.TRIP_VOXELS:] < 0).any() and (flat[sc.TRIP_VOXELS:] > 0).any()
    t = to_device(lab)
    plan = device.Plan(shape, _lib.U8)
    assert plan.signed_supported()
    k = 3
    for sqrt, want in ((False, wantsq), (True, wantrt)):
        obuf, oview = offset_out((sz, sy, sx), np.float32, k, NAN)
        # the kernel's own arithmetic, from the address: head, quads (more than one trip of the grid), tail
        head = (16 - oview.data_ptr() % 16) % 16 // 4
        quads = (n - head) // 4
        tail = n - head - 4 * quads
        assert head == 1 and tail == 2 and quads > 16384 * 256, (head, quads, tail)
        _, names = pass_names(lambda: plan.run(t, (1.0, 1.0, 1.0), black_border=True, sqrt=sqrt, out=oview, signed=True))
        assert "sign" in names, names
        got = oview.cpu().numpy().T
        assert np.array_equal(got, want), (sqrt, int((got != want).sum()))
        assert outside_intact(obuf, k, n, NAN), (sqrt, "a store outside the output")
        del obuf, oview
    torch.cuda.synchronize()
