#!/usr/bin/env python3
"""Timing of erode / dilate / opening / closing on device-resident volumes.

Volumes (512^3 unless --n says otherwise): the dense 2000-label segmentation cfg3 (uint32) and synth.blob_mask (uint8).
Radius --radius (default 2), unit voxel sizes, no black border.  For every volume and operation:
  (i)   `new_ms`: the call of edt.device (erode, dilate, opening, closing);
  (ii)  `hand_ms`: the same result composed by hand from what the library offered before -- device.edtsq + torch.where for
        erode; that plus device.edtsq of a torch-built mask for opening; device.expand_labels for dilate; expand_labels, a
        torch-built mask, device.edtsq and torch.where for closing.  Checked equal to (i), bit for bit, before anything is timed.
Both are means over --steps calls after --warmup, hipEvents around the loop, taken in turn --rounds times (new, hand, new,
hand ...); the table shows the median round and the spread (min .. max).
The select kernel on its own (the erode form: values and field read, out written) is timed the same way and shown as GB/s of
the bytes it has to move, beside a bare stream of the same number of bytes: for 4-byte labels torch.add of two int32 volumes into
a third (the same mix: 8 bytes read, 4 written per voxel), otherwise a torch copy moving as many bytes in all.
Prints one JSON line per row and a markdown table.  Run it under a time limit on an otherwise idle GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "euclidean-distance-transform-3d_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from edt import _lib, device  # noqa: E402
from synth import blob_mask, config_volume  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def in_turn(fns, steps, warmup, rounds):
    """[(median, min, max)] of the per-call ms of every fn, timed in turn `rounds` times"""
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            ms[k].append(timed(fn, steps, warmup))
    return [(statistics.median(v), min(v), max(v)) for v in ms]


def hand(op, t, r):
    r2 = float(r) * float(r)
    zero = torch.zeros((), dtype=t.dtype, device=t.device)
    if op == "erode":
        return torch.where(device.edtsq(t) > r2, t, zero)
    if op == "opening":
        z = (~(device.edtsq(t) > r2)).to(torch.uint8)
        return torch.where(device.edtsq(z) <= r2, t, zero)
    if op == "dilate":
        return device.expand_labels(t, r)
    D = device.expand_labels(t, r)
    C = device.edtsq((D != 0).to(torch.uint8))
    return torch.where((t != 0) | (C > r2), D, zero)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ops", default="erode,opening,dilate,closing")
    ap.add_argument("--volumes", default="cfg3,blobs")
    args = ap.parse_args()
    _lib.load()
    torch.cuda.set_device(0)
    n, r = args.n, args.radius
    rows = []
    for vol in args.volumes.split(","):
        if vol == "cfg3":
            lab = config_volume("cfg3", n)[0]                                # (x, y, z), Fortran, uint32
            t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).cuda()
        else:
            t = torch.from_numpy(blob_mask((n,) * 3)).cuda()                 # uint8
        for op in [o for o in args.ops.split(",") if o]:
            new = lambda op=op: getattr(device, op)(t, r)  # noqa: E731
            a, b = new(), hand(op, t, r)
            torch.cuda.synchronize()
            equal = bool(torch.equal(a, b))
            kept = int(torch.count_nonzero(a)) / max(1, int(torch.count_nonzero(t)))
            del a, b
            assert equal, f"{op} on {vol}: the hand composition differs"
            (nm, nlo, nhi), (hm, hlo, hhi) = in_turn([new, lambda op=op: hand(op, t, r)], args.steps, args.warmup, args.rounds)
            row = {"volume": vol, "dtype": str(t.dtype), "n": n, "op": op, "radius": r, "kept": round(kept, 4), "new_ms": round(nm, 4),
                   "new_range": [round(nlo, 4), round(nhi, 4)], "hand_ms": round(hm, 4), "hand_range": [round(hlo, 4), round(hhi, 4)],
                   "new_over_hand": round(nm / hm, 4)}
            print(json.dumps(row), flush=True)
            rows.append(row)
        # the select kernel alone, and a bare stream of as many bytes
        field = device.edtsq(t)
        out = torch.empty_like(t)
        code = device.dtype_code(t.dtype)
        size = t.element_size()
        nbytes = t.numel() * (2 * size + 4)
        select = lambda: device._morph_select(code, t, field, r, _lib.MORPH_FARTHER, out=out)  # noqa: E731
        if size == 4:
            fi = field.view(torch.int32)
            bare, what = (lambda: torch.add(t, fi, out=out)), "torch.add of two int32 volumes into a third"
        else:
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            bare, what = (lambda: dst.copy_(src)), "torch copy of as many bytes in all"
        (sm, slo, shi), (bm, blo, bhi) = in_turn([select, bare], args.steps, args.warmup, args.rounds)
        row = {"volume": vol, "dtype": str(t.dtype), "n": n, "op": "select (erode form)", "bytes": nbytes, "select_ms": round(sm, 4),
               "select_range": [round(slo, 4), round(shi, 4)], "select_GBps": round(nbytes / sm / 1e6, 1), "bare": what,
               "bare_ms": round(bm, 4), "bare_range": [round(blo, 4), round(bhi, 4)], "bare_GBps": round(nbytes / bm / 1e6, 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del t, field, out
        torch.cuda.empty_cache()
    print()
    print("| volume | op | kept | new ms (min .. max) | hand composition ms (min .. max) | new / hand |")
    print("|---|---|---:|---:|---:|---:|")
    for w in rows:
        if "new_ms" in w:
            print(f"| {w['volume']} {w['dtype'].replace('torch.', '')} | {w['op']} | {w['kept']:.3f} | {w['new_ms']:.3f} ({w['new_range'][0]:.3f} .. "
                  f"{w['new_range'][1]:.3f}) | {w['hand_ms']:.3f} ({w['hand_range'][0]:.3f} .. {w['hand_range'][1]:.3f}) | {w['new_over_hand']:.3f} |")
    print()
    print("| volume | select ms | GB/s | bare stream | ms | GB/s |")
    print("|---|---:|---:|---|---:|---:|")
    for w in rows:
        if "select_ms" in w:
            print(f"| {w['volume']} {w['dtype'].replace('torch.', '')} | {w['select_ms']:.3f} | {w['select_GBps']:.0f} | {w['bare']} | {w['bare_ms']:.3f} | "
                  f"{w['bare_GBps']:.0f} |")


if __name__ == "__main__":
    main()
