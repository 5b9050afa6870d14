#!/usr/bin/env python3
"""Timing of the feature transform and expand_labels on device-resident 512^3 uint32 volumes.

For every case: the per-pass times of one profiled call (edt_hip_set_profiling hook), the mean time of a call over
--steps calls after --warmup (hipEvents around the whole loop), and the edtsq time of the same volume for comparison.
Cases: cfg2 (ones, (6,6,30), black border), cfg3 (Voronoi, 2000 labels), cfg3f (the same labels at (3.58, 3.58, 40):
fp64 values), sphere250 and diagF (tests/synth.py: SWEEP), and expand_labels on cfg3m (Voronoi with membranes).
Prints one JSON line per case and a markdown table.  Run it under a time limit on the GPU host."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "euclidean-distance-transform-3d_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from edt import _lib, device  # noqa: E402
from synth import config_volume  # noqa: E402

CASES = [("cfg2", "ft"), ("cfg3", "ft"), ("cfg3f", "ft"), ("sphere250", "ft"), ("diagF", "ft"), ("cfg3m", "expand")]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default=",".join(c for c, _ in CASES))
    args = ap.parse_args()
    lib = _lib.load()
    torch.cuda.set_device(0)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rows = []
    for name, kind in CASES:
        if name not in args.cases.split(","):
            continue
        lab, an, bb = config_volume(name, args.n)           # (x, y, z), Fortran
        t = torch.from_numpy(np.ascontiguousarray(lab.T)).cuda()
        del lab
        ext = tuple(t.shape[::-1])
        code = device.dtype_code(t.dtype)
        w = tuple(float(np.float32(a)) for a in an)
        if kind == "ft":
            flags = _lib.FLAG_BLACK_BORDER if bb else 0
            ws = torch.empty(lib.edt_hip_feature_workspace_bytes(code, 3, *ext, flags), dtype=torch.uint8, device="cuda")
            out = torch.empty((3,) + tuple(t.shape), dtype=torch.int32, device="cuda")

            def call():
                _lib.check(lib.edt_hip_feature_transform_device(vp(t), code, 3, *ext, *w, flags, vp(out), vp(ws),
                                                                ws.numel(), stream()))
        else:
            ws = torch.empty(lib.edt_hip_expand_labels_workspace_bytes(code, 3, *ext), dtype=torch.uint8, device="cuda")
            out = torch.empty_like(t)

            def call():
                _lib.check(lib.edt_hip_expand_labels_device(vp(t), code, 3, *ext, *w, 1.5 * max(w), vp(out), vp(ws),
                                                            ws.numel(), stream()))
        ms = timed(call, args.steps, args.warmup)
        device.set_profiling(True)
        call()
        torch.cuda.synchronize()
        passes = device.pass_times()
        device.set_profiling(False)
        del ws, out
        plan = device.Plan(ext, code)
        sq = torch.empty(t.shape, dtype=torch.float32, device="cuda")
        edtsq_ms = timed(lambda: plan.run(t, w, bb, out=sq), args.steps, args.warmup)
        del plan, sq, t
        torch.cuda.empty_cache()
        row = {"case": name, "op": kind, "anisotropy": an, "black_border": bb, "ms": round(ms, 3),
               "passes": {k: round(v, 3) for k, v in passes}, "edtsq_ms": round(edtsq_ms, 3), "steps": args.steps}
        print(json.dumps(row), flush=True)
        rows.append(row)
    print()
    print("| case | op | voxel sizes | black border | passes (ms) | mean ms | edtsq ms |")
    print("|---|---|---|---|---|---:|---:|")
    for r in rows:
        p = ", ".join(f"{k.split()[-1]} {v:.2f}" for k, v in r["passes"].items())
        print(f"| {r['case']} | {r['op']} | {tuple(r['anisotropy'])} | {r['black_border']} | {p} | {r['ms']:.2f} | "
              f"{r['edtsq_ms']:.3f} |")


if __name__ == "__main__":
    main()
