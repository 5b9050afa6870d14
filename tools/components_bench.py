#!/usr/bin/env python3
"""Timing of connected_components on device-resident uint32 volumes.

Cases (512^3 unless --n says otherwise): the blob mask with `binary` (bench.py's cfg5 as uint32), the dense segmentation
cfg3, the sweep volume sw256, one label everywhere, and a 3-D checkerboard at connectivity 1 (every set voxel its own
component) and at connectivity 3 (one component, through corners only).  For every case:
  (i)   the mean over --steps calls after --warmup, hipEvents around the whole loop, of the C ABI call on pre-allocated
        buffers (`abi_ms`) and of edt.device.connected_components (`python_ms`), plus the per-phase times of one profiled call;
  (ii)  the time to stream the same bytes: the byte model of DESIGN.md 10 (8 reads or writes of 4 bytes per voxel) as
        four torch copies of the label volume (one read + one write each, `stream_ms`);
  (iii) with --host, scipy.ndimage.label on the host of the same box (`scipy_ms`, one call; context only).
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

CASES = ["blobs", "cfg3", "sw256", "ones", "checker_c1", "checker_c3"]


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
    """(labels as an (x, y, z) Fortran uint32 array, connectivity, binary)"""
    if name == "blobs":
        return np.asfortranarray(config_volume("cfg5", n)[0].astype(np.uint32)), 3, True
    if name in ("cfg3", "sw256"):
        return config_volume(name, n)[0], 3, False
    if name == "ones":
        return np.ones((n, n, n), dtype=np.uint32, order="F"), 3, False
    x, y, z = np.meshgrid(*[np.arange(n)] * 3, indexing="ij", sparse=True)
    return np.asfortranarray(((x + y + z) % 2 == 0).astype(np.uint32)), (1 if name == "checker_c1" else 3), False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--host", action="store_true", help="also time scipy.ndimage.label on the host (one call per case)")
    args = ap.parse_args()
    lib = _lib.load()
    torch.cuda.set_device(0)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rows = []
    for name in args.cases.split(","):
        lab, c, binary = volume(name, args.n)                # (x, y, z), Fortran
        row = {"case": name, "shape_xyz": lab.shape, "connectivity": c, "binary": binary}
        if args.host:
            from scipy import ndimage
            st = ndimage.generate_binary_structure(3, c)
            t0 = time.perf_counter()
            if binary or name in ("ones", "checker_c1", "checker_c3"):
                row["scipy_components"] = int(ndimage.label(lab.T != 0, structure=st)[1])
            else:   # multi-label: scipy has no such call; the binary labelling of the same volume is the context figure
                row["scipy_components_binary"] = int(ndimage.label(lab.T != 0, structure=st)[1])
            row["scipy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).cuda()
        del lab
        ext = tuple(t.shape[::-1])
        code = device.dtype_code(t.dtype)
        ws = torch.empty(lib.edt_hip_components_workspace_bytes(code, 3, *ext), dtype=torch.uint8, device="cuda")
        out = torch.empty(t.shape, dtype=torch.int32, device="cuda")
        n = torch.zeros((), dtype=torch.int64, device="cuda")

        def call():
            _lib.check(lib.edt_hip_connected_components_device(vp(t), code, 3, *ext, c, int(binary), vp(out), vp(n), vp(ws),
                                                               ws.numel(), stream()))

        abi_ms = timed(call, args.steps, args.warmup)
        python_ms = timed(lambda: device.connected_components(t, connectivity=c, binary=binary), args.steps, args.warmup)
        device.set_profiling(True)
        call()
        torch.cuda.synchronize()
        passes = device.pass_times()
        device.set_profiling(False)

        def stream_bytes():   # 8 x 4 bytes per voxel: four copies
            for _ in range(4):
                out.copy_(t)

        stream_ms = timed(stream_bytes, args.steps, args.warmup)
        call()
        row.update({"components": int(n.item()), "abi_ms": round(abi_ms, 4), "python_ms": round(python_ms, 4),
                    "passes": {k: round(v, 4) for k, v in passes}, "stream_ms": round(stream_ms, 4),
                    "ratio_to_stream": round(abi_ms / stream_ms, 2), "workspace_bytes": ws.numel(), "steps": args.steps})
        print(json.dumps(row), flush=True)
        rows.append(row)
        del ws, out, t
        torch.cuda.empty_cache()
    print()
    print("| case | c | components | rows / merge / flatten / number / final (ms) | (i) ABI call ms | (i) Python call ms | (ii) stream ms | (i)/(ii) | (iii) scipy ms |")
    print("|---|---:|---:|---|---:|---:|---:|---:|---:|")
    for r in rows:
        p = " / ".join(f"{v:.3f}" for v in r["passes"].values())
        print(f"| {r['case']} | {r['connectivity']}{' binary' if r['binary'] else ''} | {r['components']} | {p} | {r['abi_ms']:.3f} | "
              f"{r['python_ms']:.3f} | {r['stream_ms']:.3f} | {r['ratio_to_stream']:.2f} | {r.get('scipy_ms', '')} |")


if __name__ == "__main__":
    main()
