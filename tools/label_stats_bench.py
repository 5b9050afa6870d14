#!/usr/bin/env python3
"""Timing of label_stats on device-resident uint32 volumes.

Cases: cfg2 (512^3, one label), cfg3 (512^3, Voronoi, 2000 labels) and snemi (the README workload: 512 x 512 x 100, 334
full-resolution Voronoi labels, bench.py: snemi_like).  dt is edt() of the volume, resident.  For every case:
  (i)   label_stats on the resident dt: the mean over --steps calls after --warmup, hipEvents around the whole loop, of the
        C ABI call on pre-allocated buffers (`abi_ms`) and of edt.device.label_stats (`python_ms`: allocations and the read of
        n_labels included), plus the per-pass times of one profiled call;
  (ii)  a bare read of the same bytes, labels + dt, TWICE (the two-sweep form): torch amax over both tensors as fp32 (`read_ms`);
  (iii) snemi only: the same table from edt.device.each(..., in_place=True) with amax, argmax and count_nonzero per image
        (`each_ms`, one pass over all labels, host synchronisation at the end).
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
from synth import config_volume, voronoi_full  # noqa: E402

CASES = ["cfg2", "cfg3", "snemi"]


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
    if name == "snemi":
        return voronoi_full((512, 512, 100), 334, seed=7), (4.0, 4.0, 40.0), False
    return config_volume(name, n)


def each_table(t, dt):
    rows = []
    for key, img in device.each(t, dt, in_place=True):
        rows.append((key, img.amax(), img.argmax(), torch.count_nonzero(img)))
    torch.cuda.synchronize()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    lib = _lib.load()
    torch.cuda.set_device(0)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rows = []
    for name in args.cases.split(","):
        lab, an, bb = volume(name, args.n)                  # (x, y, z), Fortran
        t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).cuda()
        del lab
        dt = device.edt(t, anisotropy=an[::-1], black_border=bb)
        ext = tuple(t.shape[::-1])
        code = device.dtype_code(t.dtype)
        cap = device.default_max_labels(code, t.numel())[0]
        ws = torch.empty(lib.edt_hip_label_stats_workspace_bytes(code, t.numel(), cap), dtype=torch.uint8, device="cuda")
        keys = torch.empty(cap, dtype=t.dtype, device="cuda")
        counts, arg = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int64, device="cuda")
        mx = torch.empty(cap, dtype=torch.float32, device="cuda")
        bbox, nl = torch.empty((cap, 6), dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")

        def call():
            _lib.check(lib.edt_hip_label_stats_device(vp(t), code, vp(dt), 3, *ext, cap, vp(keys), vp(counts), vp(mx), vp(arg),
                                                      vp(bbox), vp(nl), vp(ws), ws.numel(), stream()))

        abi_ms = timed(call, args.steps, args.warmup)
        python_ms = timed(lambda: device.label_stats(t, dt), args.steps, args.warmup)
        device.set_profiling(True)
        call()
        torch.cuda.synchronize()
        passes = device.pass_times()
        device.set_profiling(False)

        tf = t.view(torch.float32)   # (the same bytes; float reductions are torch's fastest readers)

        def read_twice():
            for _ in range(2):
                tf.amax()
                dt.amax()

        read_ms = timed(read_twice, args.steps, args.warmup)
        row = {"case": name, "shape_xyz": ext, "labels": int(nl.item()), "abi_ms": round(abi_ms, 4),
               "python_ms": round(python_ms, 4), "passes": {k: round(v, 4) for k, v in passes},
               "read_ms": round(read_ms, 4), "ratio_to_read": round(abi_ms / read_ms, 2), "max_labels": cap,
               "workspace_bytes": ws.numel(), "steps": args.steps}
        if name == "snemi":
            each_table(t, dt)
            t0 = time.perf_counter()
            got = each_table(t, dt)
            row["each_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            row["each_over_label_stats"] = round(row["each_ms"] / python_ms, 1)
            assert len(got) == row["labels"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del ws, keys, counts, arg, mx, bbox, t, dt
        torch.cuda.empty_cache()
    print()
    print("| case | labels | sweep 1 / sweep 2 / finish (ms) | (i) ABI call ms | (i) Python call ms | (ii) read x2 ms | (i)/(ii) | (iii) each() ms |")
    print("|---|---:|---|---:|---:|---:|---:|---:|")
    for r in rows:
        p = " / ".join(f"{v:.3f}" for k, v in r["passes"].items() if "clear" not in k)
        print(f"| {r['case']} | {r['labels']} | {p} | {r['abi_ms']:.3f} | {r['python_ms']:.3f} | {r['read_ms']:.3f} | "
              f"{r['ratio_to_read']:.2f} | {r.get('each_ms', '')} |")


if __name__ == "__main__":
    main()
