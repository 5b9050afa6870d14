#!/usr/bin/env python3
"""Timing of label_topology on device-resident uint32 volumes.

Cases: cfg2 (512^3, one label), cfg3 (512^3, Voronoi, 2000 labels) and snemi (the README workload: 512 x 512 x 100, 334
full-resolution Voronoi labels).  For every case, in one process:
  `topology_ms`   edt.device.label_topology (cached scratch; the outputs are allocated and n_labels is read per call);
  `abi_ms`        edt_hip_label_topology_device alone on buffers kept here, and the per-pass times of one profiled call;
  `moments_ms`    edt.device.label_moments on the same tensor: the yardstick -- the same table machinery, one read of the labels,
                  no stencil;
  `read_ms`       a bare read of the labels: torch amax over the same bytes as fp32.
All are means over --steps calls after --warmup, hipEvents around the loop, taken in turn --rounds times; the table shows the
median round and the spread (min .. max).
On snemi also `torch_ms`: what users do today -- per label, `labels == k`, the closed and interior cell counts by shifted `|` and
`&` of the mask, and sums (the mean of --torch-steps calls).  Its Euler numbers and face counts are checked equal to the
call's before anything is timed.
Prints one JSON line per case and a markdown table.  Run it under a time limit on an otherwise idle GPU."""
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
from synth import config_volume, voronoi_full  # noqa: E402

CASES = ["cfg2", "cfg3", "snemi"]


def volume(name, n):
    if name == "snemi":
        return voronoi_full((512, 512, 100), 334, seed=7)
    return config_volume(name, n)[0]


def torch_cells(mask):
    """(closed, interior) of one 0 / 1 uint8 (z, y, x) mask as two lists of eight 0-dim tensors, indexed by the ABI's type
    (bit 0 = x): across every axis a cell does not extend along, the mask padded by one and OR-ed with its shift (closed) or
    AND-ed with it (interior)"""
    closed, interior = [], []
    for t in range(8):
        c = i = mask
        for k in range(3):
            if (t >> k) & 1:
                continue
            dim = 2 - k
            p = torch.nn.functional.pad(c, [(1 if d == dim else 0) for d in (2, 2, 1, 1, 0, 0)])
            c = p.narrow(dim, 0, p.shape[dim] - 1) | p.narrow(dim, 1, p.shape[dim] - 1)
            i = i.narrow(dim, 0, i.shape[dim] - 1) & i.narrow(dim, 1, i.shape[dim] - 1)
        closed.append(c.sum())
        interior.append(i.sum())
    return closed, interior


def torch_table(t, keys):
    """(closed, interior), int64 (n, 8) each, label by label"""
    rows = [torch_cells((t == k).to(torch.uint8)) for k in keys.tolist()]
    return torch.stack([torch.stack(c) for c, _ in rows]), torch.stack([torch.stack(i) for _, i in rows])


def abi_columns(table):
    """a LabelTopology of a (z, y, x) tensor as the ABI's (n, 8) columns"""
    cols = [((t >> 2) & 1, (t >> 1) & 1, t & 1) for t in range(8)]
    pick = lambda a: torch.stack([a[(slice(None),) + c] for c in cols], dim=1)  # noqa: E731
    return pick(table.closed), pick(table.interior)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=1, help="calls per round of the per-label torch composition (it is slow)")
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    lib = _lib.load()
    torch.cuda.set_device(0)
    rows = []
    for case in args.cases.split(","):
        lab = volume(case, args.n)                                           # (x, y, z), Fortran, uint32
        t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).cuda()
        del lab
        code = device.dtype_code(t.dtype)
        ext = tuple(int(e) for e in t.shape[::-1])
        table = device.label_topology(t)
        n = len(table.labels)
        cap = device.default_max_labels(code, t.numel())[0]
        ws = torch.empty(int(lib.edt_hip_label_topology_workspace_bytes(code, t.numel(), cap)), dtype=torch.uint8, device=t.device)
        keys = torch.empty(cap, dtype=t.dtype, device=t.device)
        closed, interior = (torch.empty((cap, 8), dtype=torch.int64, device=t.device) for _ in range(2))
        count = torch.empty(1, dtype=torch.int64, device=t.device)
        abi = lambda: _lib.check(lib.edt_hip_label_topology_device(  # noqa: E731
            device._vp(t), code, 3, *ext, cap, device._vp(keys), device._vp(closed), device._vp(interior), device._vp(count),
            device._vp(ws), ws.numel(), device._stream_ptr()))
        abi()
        want_closed, want_interior = abi_columns(table)
        assert int(count) == n and torch.equal(closed[:n], want_closed) and torch.equal(interior[:n], want_interior)
        assert int(table.counts.sum()) == int(torch.count_nonzero(t))
        device.set_profiling(True)
        abi()
        torch.cuda.synchronize()
        passes = device.pass_times()
        device.set_profiling(False)
        as_float = t.view(torch.float32)
        whole = lambda: device.label_topology(t)  # noqa: E731
        moments = lambda: device.label_moments(t)  # noqa: E731
        read = lambda: torch.amax(as_float)  # noqa: E731
        (wm, wlo, whi), (am, alo, ahi), (mm, mlo, mhi), (rm, rlo, rhi) = in_turn([whole, abi, moments, read], args.steps, args.warmup,
                                                                                args.rounds)
        r4 = lambda v: round(v, 4)  # noqa: E731
        row = {"case": case, "shape_zyx": list(t.shape), "labels": n, "topology_ms": r4(wm), "topology_range": [r4(wlo), r4(whi)],
               "abi_ms": r4(am), "abi_range": [r4(alo), r4(ahi)], "passes_ms": passes, "moments_ms": r4(mm),
               "moments_range": [r4(mlo), r4(mhi)], "topology_over_moments": r4(wm / mm), "read_ms": r4(rm),
               "read_range": [r4(rlo), r4(rhi)], "abi_GBps_of_one_read": round(t.numel() * 4 / am / 1e6, 1),
               "read_GBps": round(t.numel() * 4 / rm / 1e6, 1)}
        if case == "snemi":
            euler_full, euler_face = table.euler(3), table.euler(1)
            tc, ti = torch_table(t, table.labels)
            sign = torch.tensor([(-1) ** bin(s).count("1") for s in range(8)], dtype=torch.int64, device=t.device)
            assert np.array_equal((tc * sign).sum(1).cpu().numpy(), euler_full), "torch composition: Euler numbers, full adjacency"
            assert np.array_equal((-(ti * sign)).sum(1).cpu().numpy(), euler_face), "torch composition: Euler numbers, face adjacency"
            assert torch.equal(tc, want_closed) and torch.equal(ti, want_interior), "torch composition: cell counts"
            (tm, tlo, thi), = in_turn([lambda: torch_table(t, table.labels)], args.torch_steps, 0, args.rounds)
            row.update({"torch_ms": r4(tm), "torch_range": [r4(tlo), r4(thi)], "torch_over_topology": r4(tm / wm)})
        print(json.dumps(row), flush=True)
        rows.append(row)
        del t, as_float, ws, keys, closed, interior, table
        device._workspaces.clear()
        torch.cuda.empty_cache()
    print()
    print("| case | labels | device.label_topology ms (min .. max) | ABI call ms | device.label_moments ms | topology / moments | "
          "bare read ms | GB/s of one read at the ABI call | torch per label ms |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|")
    for w in rows:
        print(f"| {w['case']} {tuple(w['shape_zyx'])} | {w['labels']} | {w['topology_ms']:.3f} ({w['topology_range'][0]:.3f} .. "
              f"{w['topology_range'][1]:.3f}) | {w['abi_ms']:.3f} | {w['moments_ms']:.3f} | {w['topology_over_moments']:.2f} | "
              f"{w['read_ms']:.3f} | {w['abi_GBps_of_one_read']:.0f} | {w.get('torch_ms', float('nan')):.1f} |")


if __name__ == "__main__":
    main()
