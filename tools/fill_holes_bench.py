#!/usr/bin/env python3
"""Timing of fill_holes on device-resident uint32 volumes.

Cases (512^3 unless --n says otherwise): the dense segmentation cfg3 with 1 % of its voxels zeroed at random, the blob mask
(bench.py's cfg5 as uint32) with `binary`, one label everywhere with a lattice of one-voxel cavities, and all background
(nothing to fill: the floor).  Connectivity 1 throughout.  For every case:
  (i)   the mean over --steps calls after --warmup, hipEvents around the whole loop, of the C ABI call on pre-allocated
        buffers (`abi_ms`) and of edt.device.fill_holes (`python_ms`), plus the per-phase times of one profiled call;
  (ii)  the time to stream the bytes of the model of DESIGN.md 11 (25 bytes per voxel for 4-byte labels) as device copies:
        three copies of the label volume and a one-byte copy of half a volume (`stream_ms`);
  (iii) the same result composed from connected_components and torch: the components of labels == 0, scatter_reduce of
        boundary membership and of the smallest and largest wall label per component, and a gather (`composed`, below;
        checked equal to (i) before it is timed, which also warms it; mean of --composed-steps calls, `composed_ms`);
  (iv)  with --host, scipy.ndimage.binary_fill_holes on the host of the same box (`scipy_ms`, one call; context only).
Prints one JSON line per case and a markdown table.  Run it under a time limit on an otherwise idle GPU."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "euclidean-distance-transform-3d_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from edt import _lib, device  # noqa: E402
from synth import config_volume  # noqa: E402

CASES = ["cfg3_1pct", "blobs", "lattice", "background"]


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


def volume(name, n):
    """(labels as an (x, y, z) Fortran uint32 array, binary)"""
    if name == "cfg3_1pct":
        lab = config_volume("cfg3", n)[0].copy(order="F")
        lab[np.random.default_rng(1).random(lab.shape, dtype=np.float32) < 0.01] = 0
        return lab, False
    if name == "blobs":
        return np.asfortranarray(config_volume("cfg5", n)[0].astype(np.uint32)), True
    if name == "lattice":
        lab = np.ones((n, n, n), dtype=np.uint32, order="F")
        lab[1:-1:2, 1:-1:2, 1:-1:2] = 0
        return lab, False
    return np.zeros((n, n, n), dtype=np.uint32, order="F"), False


def composed(t, edge):
    """fill_holes(t, connectivity=1) of an int32 (z, y, x) tensor from what the library offered before it.  The fill value is
    the smallest wall label: the contract's for a cavity whose wall holds one label, and for any cavity of a one-label mask."""
    comp, n = device.connected_components(t == 0, connectivity=1)
    k = int(n) + 1                                               # (slot 0 takes everything that is not background)
    comp = comp.long()
    is_open = torch.zeros(k, dtype=torch.int32, device=t.device).scatter_reduce_(0, comp.reshape(-1), edge.reshape(-1), "amax")
    lo = torch.full((k,), 2 ** 31 - 1, dtype=torch.int32, device=t.device)
    hi = torch.zeros(k, dtype=torch.int32, device=t.device)
    for axis in range(3):
        for a, b in ((slice(0, -1), slice(1, None)), (slice(1, None), slice(0, -1))):
            sa, sb = [slice(None)] * 3, [slice(None)] * 3
            sa[axis], sb[axis] = a, b
            wall = t[tuple(sb)]
            idx = torch.where(wall != 0, comp[tuple(sa)], 0).reshape(-1)
            lo.scatter_reduce_(0, idx, wall.reshape(-1), "amin")
            hi.scatter_reduce_(0, idx, wall.reshape(-1), "amax")
    value = torch.where((is_open == 0) & (lo == hi), lo, 0)
    value[0] = 0
    return torch.where(comp > 0, value[comp], t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--composed-steps", type=int, default=3, help="(iii) takes seconds per call")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--host", action="store_true", help="also time scipy.ndimage.binary_fill_holes on the host (one call per case)")
    args = ap.parse_args()
    lib = _lib.load()
    torch.cuda.set_device(0)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    n3 = (args.n,) * 3
    edge = torch.zeros(n3, dtype=torch.int32, device="cuda")
    for axis in range(3):
        edge.select(axis, 0).fill_(1)
        edge.select(axis, args.n - 1).fill_(1)
    half = torch.empty(args.n ** 3 // 2, dtype=torch.uint8, device="cuda")
    half2 = torch.empty_like(half)
    rows = []
    for name in args.cases.split(","):
        lab, binary = volume(name, args.n)                   # (x, y, z), Fortran
        row = {"case": name, "shape_xyz": lab.shape, "binary": binary, "background_fraction": round(float((lab == 0).mean()), 4)}
        if args.host:
            from scipy import ndimage
            t0 = time.perf_counter()
            row["scipy_filled"] = int(ndimage.binary_fill_holes(lab.T != 0).sum() - np.count_nonzero(lab))
            row["scipy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).cuda()
        del lab
        ext = tuple(t.shape[::-1])
        code = device.dtype_code(t.dtype)
        ws = torch.empty(lib.edt_hip_fill_holes_workspace_bytes(code, 3, *ext), dtype=torch.uint8, device="cuda")
        out = torch.empty_like(t)
        n = torch.zeros((), dtype=torch.int64, device="cuda")

        def call():
            _lib.check(lib.edt_hip_fill_holes_device(vp(t), code, 3, *ext, 1, int(binary), vp(out), vp(n), vp(ws), ws.numel(),
                                                     stream()))

        call()
        other = composed(t, edge)
        row["composed_equal"] = bool(torch.equal(other, out))
        row["filled"] = int(n.item())
        assert row["composed_equal"], "the composed form differs from fill_holes"
        del other
        abi_ms = timed(call, args.steps, args.warmup)
        python_ms = timed(lambda: device.fill_holes(t, connectivity=1, binary=binary), args.steps, args.warmup)
        device.set_profiling(True)
        call()
        torch.cuda.synchronize()
        passes = device.pass_times()
        device.set_profiling(False)

        def stream_bytes():   # 25 bytes per voxel
            for _ in range(3):
                out.copy_(t)
            half2.copy_(half)

        stream_ms = timed(stream_bytes, args.steps, args.warmup)
        composed_ms = timed(lambda: composed(t, edge), args.composed_steps, 0)   # (warmed by the comparison above)
        row.update({"abi_ms": round(abi_ms, 4), "python_ms": round(python_ms, 4),
                    "passes": {k.replace("fill_holes ", ""): round(v, 4) for k, v in passes}, "stream_ms": round(stream_ms, 4),
                    "ratio_to_stream": round(abi_ms / stream_ms, 2), "composed_ms": round(composed_ms, 3),
                    "workspace_bytes": ws.numel(), "steps": args.steps})
        print(json.dumps(row), flush=True)
        rows.append(row)
        del ws, out, t
        torch.cuda.empty_cache()
    print()
    phases = ["mask", "rows", "merge", "flatten", "mark", "check", "fill"]
    print("| case | background | filled | " + " / ".join(phases) + " (ms) | (i) ABI call ms | (i) Python call ms | (ii) stream ms | (i)/(ii) | (iii) composed ms | (iv) scipy ms |")
    print("|---|---:|---:|---|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        p = " / ".join(f"{r['passes'][k]:.3f}" if k in r["passes"] else "-" for k in phases)
        print(f"| {r['case']}{' binary' if r['binary'] else ''} | {r['background_fraction']:.3f} | {r['filled']} | {p} | {r['abi_ms']:.3f} | "
              f"{r['python_ms']:.3f} | {r['stream_ms']:.3f} | {r['ratio_to_stream']:.2f} | {r['composed_ms']:.1f} | {r.get('scipy_ms', '')} |")


if __name__ == "__main__":
    main()
