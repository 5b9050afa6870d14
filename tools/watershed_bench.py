#!/usr/bin/env python3
"""Timing of edt.device.watershed on device-resident uint32 volumes.

Label sets (512^3 unless --n says otherwise): one label everywhere, the ~2000-label segmentation cfg3 and the blob mask cfg5 (with
`binary`).  For every label set, connectivity 1 and 3, min_saliency 0 and 1 voxel:
  (i)   the mean over --steps calls after --warmup, device events around the whole loop, of device.watershed with the field
        given (the library's own transform with a black border, computed once outside the loop) and with field=None (the
        transform inside every call), plus the per-pass times of one profiled call of each of the two -- repeated --repeats
        times, so that the spread shows;
  (ii)  the yardstick: device.connected_components on the same volume and connectivity, in the same session, timed the same way
        and alternating with (i).
Prints one JSON line per row and a markdown table.  A run without a device fails.  Run it under a time limit on an otherwise idle
GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "euclidean-distance-transform-3d_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from edt import _lib, device  # noqa: E402
from synth import config_volume  # noqa: E402

CASES = ["ones", "cfg3", "blobs"]


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


def profiled(fn):
    device.set_profiling(True)
    try:
        fn()
        torch.cuda.synchronize()
        return [(k, round(v, 4)) for k, v in device.pass_times()]
    finally:
        device.set_profiling(False)


def volume(name, n):
    """(labels as a (z, y, x) int32 device tensor, binary)"""
    if name == "ones":
        return torch.ones((n, n, n), dtype=torch.int32, device="cuda"), False
    lab = config_volume("cfg5" if name == "blobs" else name, n)[0]          # (x, y, z), Fortran
    return torch.from_numpy(np.ascontiguousarray(lab.T).astype(np.uint32).view(np.int32)).cuda(), name == "blobs"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    _lib.load()
    assert torch.cuda.is_available() and _lib.device_count() > 0, "watershed_bench needs a HIP device"
    torch.cuda.set_device(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "n": args.n, "steps": args.steps, "warmup": args.warmup}), flush=True)
    rows = []
    for name in args.cases.split(","):
        t, binary = volume(name, args.n)
        field = device.edt((t != 0) if binary else t, black_border=True)
        for c in (1, 3):
            cc = lambda: device.connected_components(t, connectivity=c, binary=binary)  # noqa: E731
            n_cc = int(cc()[1].item())
            for h in (0.0, 1.0):
                given = lambda: device.watershed(t, field, min_saliency=h, connectivity=c, binary=binary)  # noqa: E731
                inside = lambda: device.watershed(t, None, min_saliency=h, connectivity=c, black_border=True, binary=binary)  # noqa: E731
                basins = int(given()[1].item())
                assert int(inside()[1].item()) == basins
                cc_ms, given_ms, inside_ms = [], [], []
                for _ in range(args.repeats):                                 # alternating: the yardstick shares the session's noise
                    cc_ms.append(timed(cc, args.steps, args.warmup))
                    given_ms.append(timed(given, args.steps, args.warmup))
                    inside_ms.append(timed(inside, args.steps, args.warmup))
                med = lambda v: float(np.median(v))  # noqa: E731
                row = {"case": name, "connectivity": c, "binary": binary, "min_saliency": h, "components": n_cc, "basins": basins,
                       "components_ms": [round(v, 4) for v in cc_ms], "watershed_ms": [round(v, 4) for v in given_ms],
                       "watershed_field_none_ms": [round(v, 4) for v in inside_ms],
                       "ratio_to_components": round(med(given_ms) / med(cc_ms), 2),
                       "passes": profiled(given), "components_passes": profiled(cc)}
                print(json.dumps(row), flush=True)
                rows.append(row)
        del t, field
        torch.cuda.empty_cache()
    print()
    print("| labels | c | min_saliency | components | basins | connected_components ms | watershed ms (field given) | ratio | watershed ms (field=None) | "
          "ascend / flatten / peaks / merge / flatten / number / final (ms) |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---|")
    for r in rows:
        med = lambda v: float(np.median(v))  # noqa: E731
        p = " / ".join(f"{v:.3f}" for _, v in r["passes"])
        print(f"| {r['case']}{' binary' if r['binary'] else ''} | {r['connectivity']} | {r['min_saliency']:g} | {r['components']} | "
              f"{r['basins']} | {med(r['components_ms']):.3f} | {med(r['watershed_ms']):.3f} | {r['ratio_to_components']:.2f} | "
              f"{med(r['watershed_field_none_ms']):.3f} | {p} |")


if __name__ == "__main__":
    main()
