#!/usr/bin/env python3
"""Timing of dust on device-resident uint32 volumes.

Cases (512^3 unless --n says otherwise), threshold 4 throughout: one solid label (every stretch of the count adds to ONE word: the
worst case of its atomics), the dense segmentation cfg3 (2000 labels), cfg3 with 1 % of its voxels set to random other labels
(specks: what dust is for), the 3-D checkerboard at connectivity 1 (every foreground voxel a component of its own: the most
roots there can be) and at connectivity 3 (one component through the corners: the longest merge), and all background (the
floor).  Full connectivity unless the case says otherwise.  For every case:
  (i)   the mean over --steps calls after --warmup, hipEvents around the whole loop, of the C ABI call on pre-allocated
        buffers (`abi_ms`), plus the per-pass times of one profiled call;
  (ii)  the time to stream the bytes of the model of DESIGN.md 12 (24 bytes per voxel for 4-byte labels: labels read three
        times, parents written and read, output written) as three device copies of the volume (`stream_ms`);
  (iii) the same result composed from what the library offered before: connected_components, torch.bincount of its output, a
        gather and a where (`composed`, below; checked equal to (i) before it is timed, which also warms it; mean of
        --composed-steps calls, `composed_ms`);
  (iv)  connected_components itself on the same input (`cc_ms`: the ABI call on pre-allocated buffers).
Prints one JSON line per case and a markdown table, and says whether the two conditions of DESIGN.md 12 hold: `dust count` of the
solid label below the whole connected_components call on it, and (i) below (iii) on every case.  Run it under a time limit on an
otherwise idle GPU."""
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

CASES = ["solid", "cfg3", "cfg3_specks", "checker_c1", "checker_c3", "background"]
THRESHOLD = 4
INT64_MAX = (1 << 63) - 1


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
    """(labels as an int32 (z, y, x) device tensor, connectivity)"""
    if name == "solid":
        return torch.full((n, n, n), 7, dtype=torch.int32, device="cuda"), 3
    if name == "background":
        return torch.zeros((n, n, n), dtype=torch.int32, device="cuda"), 3
    if name.startswith("checker"):
        i = torch.arange(n, dtype=torch.int32, device="cuda")
        board = (i[:, None, None] + i[None, :, None] + i[None, None, :]) & 1
        return board.contiguous(), 1 if name == "checker_c1" else 3
    lab = config_volume("cfg3", n)[0]                                # (x, y, z), Fortran
    t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).cuda()
    if name == "cfg3_specks":
        gen = torch.Generator(device="cuda").manual_seed(1)
        speck = torch.rand(t.shape, device="cuda", generator=gen) < 0.01
        other = torch.randint(1, 2001, t.shape, dtype=torch.int32, device="cuda", generator=gen)
        t = torch.where(speck, other, t)
    return t, 3


def composed(t, c):
    """dust(t, THRESHOLD, connectivity=c) from connected_components, a bincount of the numbers, a gather and a where."""
    comp, n = device.connected_components(t, connectivity=c)
    comp = comp.long()
    size = torch.bincount(comp.reshape(-1), minlength=int(n) + 1)
    size[0] = THRESHOLD                                              # (background is kept as it is)
    return torch.where(size[comp] >= THRESHOLD, t, torch.zeros_like(t)), int(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--composed-steps", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    lib = _lib.load()
    torch.cuda.set_device(0)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rows = []
    for name in args.cases.split(","):
        t, c = volume(name, args.n)
        ext = tuple(t.shape[::-1])
        code = device.dtype_code(t.dtype)
        ws = torch.empty(lib.edt_hip_dust_workspace_bytes(code, 3, *ext), dtype=torch.uint8, device="cuda")
        cc_ws = torch.empty(lib.edt_hip_components_workspace_bytes(code, 3, *ext), dtype=torch.uint8, device="cuda")
        out = torch.empty_like(t)
        counts = torch.zeros(3, dtype=torch.int64, device="cuda")
        n_cc = torch.zeros((), dtype=torch.int64, device="cuda")

        def call():
            _lib.check(lib.edt_hip_dust_device(vp(t), code, 3, *ext, c, 0, THRESHOLD, INT64_MAX, 0, vp(out), vp(counts), vp(ws),
                                               ws.numel(), stream()))

        def cc_call():   # (its uint32 output goes where dust's went: both are 4 bytes per voxel)
            _lib.check(lib.edt_hip_connected_components_device(vp(t), code, 3, *ext, c, 0, vp(out), vp(n_cc), vp(cc_ws),
                                                               cc_ws.numel(), stream()))

        cc_ms = timed(cc_call, args.steps, args.warmup)
        call()
        other, n = composed(t, c)
        row = {"case": name, "shape_xyz": ext, "connectivity": c, "counts": counts.tolist(),
               "composed_equal": bool(torch.equal(other, out)) and n == int(counts[0])}
        assert row["composed_equal"], "the composed form differs from dust"
        del other
        abi_ms = timed(call, args.steps, args.warmup)
        device.set_profiling(True)
        call()
        torch.cuda.synchronize()
        passes = device.pass_times()
        device.set_profiling(False)

        def stream_bytes():   # 24 bytes per voxel
            for _ in range(3):
                out.copy_(t)

        stream_ms = timed(stream_bytes, args.steps, args.warmup)
        composed_ms = timed(lambda: composed(t, c), args.composed_steps, 0)   # (warmed by the comparison above)
        row.update({"abi_ms": round(abi_ms, 4), "passes": {k.replace("dust ", ""): round(v, 4) for k, v in passes},
                    "stream_ms": round(stream_ms, 4), "ratio_to_stream": round(abi_ms / stream_ms, 2),
                    "composed_ms": round(composed_ms, 3), "cc_ms": round(cc_ms, 4), "workspace_bytes": ws.numel(),
                    "steps": args.steps})
        print(json.dumps(row), flush=True)
        rows.append(row)
        del ws, cc_ws, out, t
        torch.cuda.empty_cache()
    print()
    phases = ["rows", "merge", "flatten", "count", "filter"]
    print("| case | components / kept / voxels removed | " + " / ".join(phases) + " (ms) | (i) ABI call ms | (ii) stream ms | (i)/(ii) | (iii) composed ms | (iv) connected_components ms |")
    print("|---|---|---|---:|---:|---:|---:|---:|")
    for r in rows:
        p = " / ".join(f"{r['passes'][k]:.3f}" if k in r["passes"] else "-" for k in phases)
        print(f"| {r['case']} (c = {r['connectivity']}) | {' / '.join(str(v) for v in r['counts'])} | {p} | {r['abi_ms']:.3f} | "
              f"{r['stream_ms']:.3f} | {r['ratio_to_stream']:.2f} | {r['composed_ms']:.1f} | {r['cc_ms']:.3f} |")
    print()
    for r in rows:
        if r["case"] == "solid":
            ok = r["passes"]["count"] < r["cc_ms"]
            print(f"condition 1 (dust count of the solid label {r['passes']['count']:.3f} ms < connected_components {r['cc_ms']:.3f} ms): "
                  + ("holds" if ok else "FAILS"))
    bad = [r["case"] for r in rows if not r["abi_ms"] < r["composed_ms"]]
    print("condition 2 (dust faster than the composed form on every case): " + ("holds" if not bad else f"FAILS on {bad}"))


if __name__ == "__main__":
    main()
