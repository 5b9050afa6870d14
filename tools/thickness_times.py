#!/usr/bin/env python3
"""Timing of local_thickness on device-resident volumes.

Volumes (512^3 unless --n says otherwise): the dense 2000-label segmentation cfg3 (uint32) and synth.blob_mask (uint8), at unit
voxel sizes, no black border, with the radii 1..8 and with the default ladder.  For every volume and ladder:
  (i)   `new_ms`: edt.device.local_thickness (with explicit radii it only enqueues; the default ladder reads 4 bytes back);
  (ii)  `hand_ms`: the same result composed by hand from what the library offered before -- for each radius
        T = torch.where(device.opening(x, r) != 0, r, T).  Checked equal to (i), bit for bit, before anything is timed.  For the
        default ladder the hand composition is given the radii (i) used: it pays no read-back.
Both are means over --steps calls after --warmup, hipEvents around the loop, taken in turn --rounds times (new, hand, new,
hand ...); the table shows the median round and the spread (min .. max).
The step kernel on its own (a radius step with the mask of the next radius and the size counter: S and B read, T and the mask
written where the voxel is in) is timed the same way and shown as GB/s of the bytes it has to move at most (13 per voxel) and of
those it moves if no voxel is in (9 per voxel), beside the same step without the counter, the last step of a ladder (neither
counter nor mask) and a bare torch stream taken in the same run: torch.add of two fp32 volumes
into a third (8 bytes read, 4 written per voxel).
--pass-times prints device.pass_times() after one profiled call per volume: the passes of its last binary transform (the log
holds the last transform).
Prints one JSON line per row and markdown tables.  Run it under a time limit on an otherwise idle GPU."""
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


def hand(t, radii):
    T = torch.zeros(t.shape, dtype=torch.float32, device=t.device)
    for r in radii:
        T = torch.where(device.opening(t, float(r)) != 0, float(r), T)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--volumes", default="cfg3,blobs")
    ap.add_argument("--ladders", default="1..8,default")
    ap.add_argument("--pass-times", action="store_true")
    args = ap.parse_args()
    lib = _lib.load()
    torch.cuda.set_device(0)
    n = args.n
    rows = []
    for vol in args.volumes.split(","):
        if vol == "cfg3":
            lab = config_volume("cfg3", n)[0]                                # (x, y, z), Fortran, uint32
            t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).cuda()
        else:
            t = torch.from_numpy(blob_mask((n,) * 3)).cuda()                 # uint8
        for ladder in [v for v in args.ladders.split(",") if v]:
            radii = None if ladder == "default" else [float(r) for r in range(1, 9)]
            new = lambda: device.local_thickness(t, radii)  # noqa: E731
            a, sizes = device.local_thickness(t, radii, return_sizes=True)
            used = [float(r) for r in sizes.radii]
            b = hand(t, used)
            torch.cuda.synchronize()
            equal = bool(torch.equal(a, b))
            thick = int(torch.count_nonzero(a)) / max(1, int(torch.count_nonzero(t)))
            del a, b
            assert equal, f"{ladder} on {vol}: the hand composition differs"
            (nm, nlo, nhi), (hm, hlo, hhi) = in_turn([new, lambda: hand(t, used)], args.steps, args.warmup, args.rounds)
            row = {"volume": vol, "dtype": str(t.dtype), "n": n, "ladder": ladder, "radii": len(used), "in_some_opening": round(thick, 4),
                   "new_ms": round(nm, 4), "new_range": [round(nlo, 4), round(nhi, 4)], "hand_ms": round(hm, 4),
                   "hand_range": [round(hlo, 4), round(hhi, 4)], "new_over_hand": round(nm / hm, 4)}
            print(json.dumps(row), flush=True)
            rows.append(row)
        if args.pass_times:
            lib.edt_hip_set_profiling(1)
            device.local_thickness(t, [1.0, 2.0])
            torch.cuda.synchronize()
            print(json.dumps({"volume": vol, "pass_times_of_the_last_binary_transform": device.pass_times()}), flush=True)
            lib.edt_hip_set_profiling(0)
        # the step kernel alone (radius 2, next radius 3), and a bare stream of 12 bytes per voxel
        # (on tensors of its own: S, the mask of radius 2 and its transform B, as the composition makes them)
        S, B = (torch.empty(t.shape, dtype=torch.float32, device=t.device) for _ in range(2))
        mask = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
        device.Plan((n, n, n), device.dtype_code(t.dtype)).run(t, (1.0, 1.0, 1.0), out=S)
        device._morph_select(_lib.U8, None, S, 2.0, _lib.MORPH_FARTHER, mask=mask)
        device.Plan((n, n, n), _lib.U8).run(mask, (1.0, 1.0, 1.0), out=B)
        T = torch.zeros(t.shape, dtype=torch.float32, device=t.device)
        size = torch.zeros(1, dtype=torch.int64, device=t.device)

        def thickness_step(next_radius, mask=None, size=None):
            _lib.check(lib.edt_hip_thickness_step_device(
                device._vp(S), device._vp(B), 2.0, -1.0 if next_radius is None else next_radius, device._vp(T),
                None if mask is None else device._vp(mask), None if size is None else device._vp(size), None, S.numel(),
                device._stream_ptr()))
        step = lambda: thickness_step(3.0, mask, size)  # noqa: E731
        uncounted = lambda: thickness_step(3.0, mask)  # noqa: E731
        last = lambda: thickness_step(None)  # noqa: E731
        step()
        torch.cuda.synchronize()
        inside = int(size.item()) / t.numel()
        x, y, z = torch.empty_like(S), torch.empty_like(S), torch.empty_like(S)
        bare = lambda: torch.add(x, y, out=z)  # noqa: E731
        (sm, slo, shi), (um, _, _), (lm, _, _), (bm, blo, bhi) = in_turn([step, uncounted, last, bare], args.steps, args.warmup, args.rounds)
        most, least = t.numel() * 13, t.numel() * 9
        row = {"volume": vol, "n": n, "op": "radius step (r = 2, next 3)", "voxels_in": round(inside, 4), "step_ms": round(sm, 4),
               "step_range": [round(slo, 4), round(shi, 4)], "GBps_at_13_bytes": round(most / sm / 1e6, 1),
               "GBps_at_9_bytes": round(least / sm / 1e6, 1), "without_count_ms": round(um, 4), "without_count_and_mask_ms": round(lm, 4),
               "bare": "torch.add of two fp32 volumes into a third", "bare_ms": round(bm, 4),
               "bare_range": [round(blo, 4), round(bhi, 4)], "bare_GBps": round(t.numel() * 12 / bm / 1e6, 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del t, S, B, mask, T, x, y, z
        device._workspaces.clear()
        torch.cuda.empty_cache()
    print()
    print("| volume | ladder | radii | voxels in some opening / foreground | new ms (min .. max) | hand composition ms (min .. max) | new / hand |")
    print("|---|---|---:|---:|---:|---:|---:|")
    for w in rows:
        if "new_ms" in w:
            print(f"| {w['volume']} {w['dtype'].replace('torch.', '')} | {w['ladder']} | {w['radii']} | {w['in_some_opening']:.3f} | {w['new_ms']:.3f} "
                  f"({w['new_range'][0]:.3f} .. {w['new_range'][1]:.3f}) | {w['hand_ms']:.3f} ({w['hand_range'][0]:.3f} .. {w['hand_range'][1]:.3f}) | "
                  f"{w['new_over_hand']:.3f} |")
    print()
    print("| volume | voxels in | step ms (min .. max) | GB/s at 13 B | GB/s at 9 B | without the count ms | without count and mask ms | bare stream | ms | GB/s |")
    print("|---|---:|---:|---:|---:|---:|---:|---|---:|---:|")
    for w in rows:
        if "step_ms" in w:
            print(f"| {w['volume']} | {w['voxels_in']:.3f} | {w['step_ms']:.3f} ({w['step_range'][0]:.3f} .. {w['step_range'][1]:.3f}) | "
                  f"{w['GBps_at_13_bytes']:.0f} | {w['GBps_at_9_bytes']:.0f} | {w['without_count_ms']:.3f} | {w['without_count_and_mask_ms']:.3f} | {w['bare']} | {w['bare_ms']:.3f} | {w['bare_GBps']:.0f} |")


if __name__ == "__main__":
    main()
