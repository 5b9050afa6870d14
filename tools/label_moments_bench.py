#!/usr/bin/env python3
"""Timing of label_moments on device-resident uint32 volumes.

Cases: cfg2 (512^3, one label), cfg3 (512^3, Voronoi, 2000 labels) and snemi (the README workload: 512 x 512 x 100, 334
full-resolution Voronoi labels, bench.py: snemi_like).  For every case, in one session:
  (i)   label_moments: the mean over --steps calls after --warmup, hipEvents around the whole loop, of the C ABI call on
        pre-allocated buffers (`abi_ms`) and of edt.device.label_moments (`python_ms`: allocations and the read of n_labels
        included), plus the per-pass times of one profiled call;
  (a)   a bare read of the labels: torch amax over the same bytes as fp32 (`read_ms`) -- the floor;
  (b)   edt_hip_label_stats_device on the same volume and its resident edt (`stats_ms`), from the library --stats-lib names
        (a build of another commit) or else from this build;
  (c)   the same table composed from torch: unique with return_inverse, a coordinate grid and ten index_add_ in int64
        (`torch_ms`, the mean of --torch-steps calls) -- what a user writes without this call; its sums are also what (i) is
        checked against here, at full size.
Prints one JSON line per case and a markdown table.  Run it under a time limit on an otherwise idle GPU."""
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


def torch_table(t):
    """(keys, counts, sums (n, 9) in the ABI's order) of a (z, y, x) tensor, composed from torch"""
    keys, inv = torch.unique(t.reshape(-1), return_inverse=True)
    n = keys.numel()
    z, y, x = torch.meshgrid(*[torch.arange(s, dtype=torch.int64, device=t.device) for s in t.shape], indexing="ij")
    x, y, z = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    cols = [torch.ones_like(x), x, y, z, x * x, y * y, z * z, x * y, x * z, y * z]
    acc = torch.zeros((10, n), dtype=torch.int64, device=t.device)
    for k, c in enumerate(cols):
        acc[k].index_add_(0, inv, c)
    keep = keys != 0
    return keys[keep], acc[0][keep], acc[1:, keep].T.contiguous()


def stats_library(path):
    """label_stats of another build (the comparison of DESIGN.md 17): its library under its own path, bound like ours"""
    if not path:
        return _lib.load()
    lib = ctypes.CDLL(path)
    for name in ("edt_hip_label_stats_workspace_bytes", "edt_hip_label_stats_device"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--stats-lib", default="", help="libedt_hip.so of the build whose label_stats is comparison (b)")
    args = ap.parse_args()
    lib = _lib.load()
    slib = stats_library(args.stats_lib)
    torch.cuda.set_device(0)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rows = []
    for name in args.cases.split(","):
        lab, an, bb = volume(name, args.n)                  # (x, y, z), Fortran
        t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).cuda()
        del lab
        ext = tuple(t.shape[::-1])
        code = device.dtype_code(t.dtype)
        cap = device.default_max_labels(code, t.numel())[0]
        i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")  # noqa: E731
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")  # noqa: E731
        ws = torch.empty(lib.edt_hip_label_moments_workspace_bytes(code, t.numel(), cap), dtype=torch.uint8, device="cuda")
        keys, counts, sums, centroid, central, nl = torch.empty(cap, dtype=t.dtype, device="cuda"), i64(cap), i64(cap, 9), f64(cap, 3), f64(cap, 6), i64(1)

        def call():
            _lib.check(lib.edt_hip_label_moments_device(vp(t), code, 3, *ext, cap, vp(keys), vp(counts), vp(sums), vp(centroid),
                                                        vp(central), vp(nl), vp(ws), ws.numel(), stream()))

        abi_ms = timed(call, args.steps, args.warmup)
        python_ms = timed(lambda: device.label_moments(t), args.steps, args.warmup)
        device.set_profiling(True)
        call()
        torch.cuda.synchronize()
        passes = device.pass_times()
        device.set_profiling(False)
        n = int(nl.item())

        tf = t.view(torch.float32)   # (the same bytes; float reductions are torch's fastest readers)
        read_ms = timed(lambda: tf.amax(), args.steps, args.warmup)

        # (b) label_stats on the same volume
        dt = device.edt(t, anisotropy=an[::-1], black_border=bb)
        sws = torch.empty(slib.edt_hip_label_stats_workspace_bytes(code, t.numel(), cap), dtype=torch.uint8, device="cuda")
        skeys, scounts, sarg = torch.empty(cap, dtype=t.dtype, device="cuda"), i64(cap), i64(cap)
        smx, sbbox, snl = torch.empty(cap, dtype=torch.float32, device="cuda"), torch.empty((cap, 6), dtype=torch.int32, device="cuda"), i64(1)

        def stats_call():
            rc = slib.edt_hip_label_stats_device(vp(t), code, vp(dt), 3, *ext, cap, vp(skeys), vp(scounts), vp(smx), vp(sarg),
                                                 vp(sbbox), vp(snl), vp(sws), sws.numel(), stream())
            assert rc == 0, rc

        stats_ms = timed(stats_call, args.steps, args.warmup)
        assert int(snl.item()) == n and torch.equal(scounts[:n], counts[:n])
        del dt, sws

        # (c) composed from torch, and the check of (i) against it
        tkeys, tcounts, tsums = torch_table(t)
        ok = bool(torch.equal(tkeys, keys[:n]) and torch.equal(tcounts, counts[:n]) and torch.equal(tsums, sums[:n]))
        del tkeys, tcounts, tsums
        torch_ms = timed(lambda: torch_table(t), args.torch_steps, 1)

        row = {"case": name, "shape_xyz": ext, "labels": n, "abi_ms": round(abi_ms, 4), "python_ms": round(python_ms, 4),
               "passes": {k: round(v, 4) for k, v in passes}, "read_ms": round(read_ms, 4), "ratio_to_read": round(abi_ms / read_ms, 2),
               "stats_ms": round(stats_ms, 4), "stats_lib": args.stats_lib or "this build", "torch_ms": round(torch_ms, 3),
               "equals_torch": ok, "max_labels": cap, "workspace_bytes": ws.numel(), "steps": args.steps}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del ws, keys, counts, sums, centroid, central, t
        torch.cuda.empty_cache()
    print()
    print("| case | labels | clear / sweep / finish (ms) | (i) ABI call ms | (i) Python call ms | (a) read ms | (i)/(a) | (b) label_stats ms | (c) torch ms |")
    print("|---|---:|---|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        p = " / ".join(f"{v:.3f}" for v in r["passes"].values())
        print(f"| {r['case']} | {r['labels']} | {p} | {r['abi_ms']:.3f} | {r['python_ms']:.3f} | {r['read_ms']:.3f} | "
              f"{r['ratio_to_read']:.2f} | {r['stats_ms']:.3f} | {r['torch_ms']:.1f} |")
    assert all(r["equals_torch"] for r in rows), "label_moments differs from the table composed from torch"


if __name__ == "__main__":
    main()
