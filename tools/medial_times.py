#!/usr/bin/env python3
"""Timing of medial_axis on device-resident volumes.

Volumes (512^3 unless --n says otherwise): the dense 2000-label segmentation cfg3 (uint32) at voxel sizes (1, 1, 1) and
synth.blob_mask (uint8) at (6, 6, 30), no black border, default pruning.  For every volume:
  `whole_ms`    edt.device.medial_axis (feature transform and step on the cached workspace; only the output is allocated);
  `ft_ms`       edt.device.feature_transform alone, as a user calls it (it allocates its workspace and reorders the planes);
  `ft_call_ms`  edt_hip_feature_transform_device alone on planes and scratch kept here: the part of `whole_ms` that is not the step;
  `step_ms`     edt_hip_medial_axis_step_device alone, and the same with a radius output;
  `torch_ms`    the same stencil composed from torch operations on the feature tensor (fp64, one operation per product and sum,
                so nothing is contracted).  Checked equal to the step's output, bit for bit, before anything is timed.
  `bare_ms`     a bare torch stream taken in the same run: torch.add of two fp32 volumes into a third (12 bytes per voxel).
All are means over --steps calls after --warmup, hipEvents around the loop, taken in turn --rounds times; the table shows the
median round and the spread (min .. max).  The step is shown as GB/s of the bytes it has to move: 4 * ndim of features and the
label read and written per voxel (+ 8 with the radius).
Prints one JSON line per row and a markdown table.  Run it under a time limit on an otherwise idle GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "euclidean-distance-transform-3d_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from edt import _lib, device  # noqa: E402
from morph_times import in_turn  # noqa: E402
from synth import blob_mask, config_volume  # noqa: E402


def torch_stencil(t, planes, w_xyz, gamma, ratio, black_border=False, binary=False):
    """include/edt_hip.h, "medial axis", on a 3-D tensor t[z][y][x] and its feature planes (x, y, z), in torch operations"""
    A = [float(np.float32(w)) ** 2 for w in w_xyz]
    g2 = float(gamma) * float(gamma)
    fg = t != 0
    has = torch.ones_like(fg) if black_border else ~((planes == -1).all(0))
    on = torch.zeros_like(fg)
    grid = [torch.arange(t.shape[2 - c], device=t.device, dtype=torch.int64).view([-1 if d == 2 - c else 1 for d in range(3)]) for c in range(3)]
    for axis in range(3):
        dim, n = 2 - axis, t.shape[2 - axis]
        if n < 2:
            continue
        for step in (-1, 1):
            p0, q0 = (1, 0) if step < 0 else (0, 1)
            P = lambda a: a.narrow(dim, p0, n - 1)  # noqa: E731
            Q = lambda a: a.narrow(dim, q0, n - 1)  # noqa: E731
            ok = P(fg) & (Q(fg) if binary else (Q(t) == P(t))) & P(has) & Q(has)
            sep = h = crit = None
            for c in range(3):
                fp, fq = P(planes[c]).long(), Q(planes[c]).long()
                two_p = 2 * grid[c] + step if c == axis else 2 * grid[c]
                if c == axis:
                    two_p = two_p.narrow(dim, p0, n - 1)
                d = (fp - fq).double()
                s = (fp + fq - two_p).double()
                t_sep, t_h, t_crit = A[c] * (d * d), A[c] * (s * s), A[c] * (d * s)
                sep = t_sep if sep is None else sep + t_sep
                h = t_h if h is None else h + t_h
                crit = t_crit if crit is None else crit + t_crit
            P(on).logical_or_(ok & (sep > g2) & (sep >= ratio * h) & (crit >= 0.0))
    return torch.where(on, t, torch.zeros((), dtype=t.dtype, device=t.device))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=10, help="calls per round of the torch composition (it is slow)")
    ap.add_argument("--volumes", default="cfg3,blobs")
    args = ap.parse_args()
    lib = _lib.load()
    torch.cuda.set_device(0)
    n = args.n
    rows = []
    for vol in args.volumes.split(","):
        if vol == "cfg3":
            lab = config_volume("cfg3", n)[0]                                # (x, y, z), Fortran, uint32
            t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).cuda()
            an = (1.0, 1.0, 1.0)
        else:
            t = torch.from_numpy(blob_mask((n,) * 3)).cuda()                 # uint8
            an = (30.0, 6.0, 6.0)                                            # tensor axis order: (wz, wy, wx)
        w = an[::-1]
        gamma, ratio = max(w), 0.0
        code = device.dtype_code(t.dtype)
        ext = (n, n, n)
        whole = lambda: device.medial_axis(t, anisotropy=an)  # noqa: E731
        ft = lambda: device.feature_transform(t, anisotropy=an)  # noqa: E731
        a = whole()
        # (on tensors of its own: the planes, the transform's scratch and the field, as the composition makes them)
        planes = torch.empty((3,) + tuple(t.shape), dtype=torch.int32, device=t.device)
        ws = torch.empty(int(lib.edt_hip_feature_workspace_bytes(code, 3, *ext, 0)), dtype=torch.uint8, device=t.device)
        field = device.Plan(ext, code).run(t, w, sqrt=True)
        out, radius = torch.empty_like(t), torch.empty_like(field)
        ft_call = lambda: _lib.check(lib.edt_hip_feature_transform_device(  # noqa: E731
            device._vp(t), code, 3, *ext, *w, 0, device._vp(planes), device._vp(ws), ws.numel(), device._stream_ptr()))

        def medial_step(field=None, radius=None):
            _lib.check(lib.edt_hip_medial_axis_step_device(
                device._vp(t), code, 3, *ext, *w, device._vp(planes), 0, gamma, ratio, device._vp(out),
                None if field is None else device._vp(field), None if radius is None else device._vp(radius), device._stream_ptr()))
        step = lambda: medial_step()  # noqa: E731
        step_radius = lambda: medial_step(field, radius)  # noqa: E731
        composed = lambda: torch_stencil(t, planes, w, gamma, ratio)  # noqa: E731
        ft_call()
        step()
        b = composed()
        torch.cuda.synchronize()
        equal = bool(torch.equal(a, out)) and bool(torch.equal(out, b))
        on_axis = int(torch.count_nonzero(out)) / max(1, int(torch.count_nonzero(t)))
        del a, b
        assert equal, f"{vol}: the torch composition, the step and device.medial_axis differ"
        x, y, z = torch.empty_like(field), torch.empty_like(field), torch.empty_like(field)
        bare = lambda: torch.add(x, y, out=z)  # noqa: E731
        (wm, wlo, whi), (fm, flo, fhi), (cm, clo, chi), (sm, slo, shi), (rm, rlo, rhi), (bm, blo, bhi) = in_turn(
            [whole, ft, ft_call, step, step_radius, bare], args.steps, args.warmup, args.rounds)
        (tm, tlo, thi), = in_turn([composed], args.torch_steps, 2, args.rounds)
        size = t.element_size()
        nominal, with_radius = t.numel() * (12 + 2 * size), t.numel() * (20 + 2 * size)
        r4 = lambda v: round(v, 4)  # noqa: E731
        row = {"volume": vol, "dtype": str(t.dtype), "n": n, "voxel_sizes": list(w), "on_axis_of_foreground": r4(on_axis),
               "whole_ms": r4(wm), "whole_range": [r4(wlo), r4(whi)], "ft_ms": r4(fm), "ft_range": [r4(flo), r4(fhi)],
               "ft_call_ms": r4(cm), "ft_call_range": [r4(clo), r4(chi)], "step_ms": r4(sm), "step_range": [r4(slo), r4(shi)],
               "step_bytes_per_voxel": 12 + 2 * size, "step_GBps": round(nominal / sm / 1e6, 1),
               "step_radius_ms": r4(rm), "step_radius_range": [r4(rlo), r4(rhi)], "step_radius_GBps": round(with_radius / rm / 1e6, 1),
               "torch_ms": r4(tm), "torch_range": [r4(tlo), r4(thi)], "step_over_torch": r4(sm / tm),
               "whole_minus_parts_ms": r4(wm - cm - sm),
               "bare": "torch.add of two fp32 volumes into a third", "bare_ms": r4(bm), "bare_range": [r4(blo), r4(bhi)],
               "bare_GBps": round(t.numel() * 12 / bm / 1e6, 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del t, planes, ws, field, out, radius, x, y, z
        device._workspaces.clear()
        torch.cuda.empty_cache()
    print()
    print("| volume | on axis / foreground | device.medial_axis ms | device.feature_transform ms | transform call ms | step ms (min .. max) | "
          "GB/s | step + radius ms | GB/s | torch composition ms | step / torch | bare stream ms | GB/s |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    for w in rows:
        print(f"| {w['volume']} {w['dtype'].replace('torch.', '')} {tuple(w['voxel_sizes'])} | {w['on_axis_of_foreground']:.3f} | {w['whole_ms']:.3f} | "
              f"{w['ft_ms']:.3f} | {w['ft_call_ms']:.3f} | {w['step_ms']:.3f} ({w['step_range'][0]:.3f} .. {w['step_range'][1]:.3f}) | "
              f"{w['step_GBps']:.0f} | {w['step_radius_ms']:.3f} | {w['step_radius_GBps']:.0f} | {w['torch_ms']:.2f} | {w['step_over_torch']:.4f} | "
              f"{w['bare_ms']:.3f} | {w['bare_GBps']:.0f} |")


if __name__ == "__main__":
    main()
