#!/usr/bin/env python3
"""bench.py -- headline benchmark: Mvox/s of the 3-D multi-label squared EDT (edt3dsq).

Contract (driver): `python bench.py --gpus N --steps K --warmup W` prints ONE JSON line.
For N > 1 it is launched under torch.distributed.run, one rank per GPU (RCCL).

  * N = 1 headline workload = BASELINE.json configs[1]: 512^3 uint32 single label, anisotropy
    (6,6,30), black_border=True, labels and output resident in HBM (no PCIe in the timed region).
    A plain run sets up, warms up, times EXACTLY K steps and prints the line (`value`, `ms_per_step` = the mean of the K
    timed steps, `timing`); nothing else.  `--dump-outputs DIR` writes the last timed step's output to DIR/edtsq.npy
    (a fixed seeded sample where it passes 32 MiB) before the line is printed.  Everything below -- per-kernel times and
    the roofline, the checks of the timed output, the numpy round trip, the secondaries, the CPU baseline -- runs with
    `--full` only.
    With `--full` the same line carries a `secondary` list: configs[2] (cfg3: 512^3, 2000 labels, black_border=False), its
    membrane / anisotropic twin (cfg3m), four large-cell segmentations (cfg3L / cfg3La / cfg3M / cfg3Ma: full-resolution
    Voronoi cells ~130 / ~65 voxels across), the 1024^3 segmentation of configs[3] on ONE GPU (cfg4), configs[4]
    (cfg5: voxel graph) and `snemi_like` (the reference README's 334-label extraction workload) -- each with
    ms_per_step, per-kernel times and the 32 B/voxel whole-job fraction, and EVERY ONE checked bit for bit against
    the compiled reference on this host (`output_verified`; EDT_BENCH_VERIFY=0 skips the checks).
  * N > 1 workload = ONE global multi-label volume with 512^3 voxels PER GPU (N=8 -> the 1024^3
    segmentation of BASELINE configs[3]), Z-sharded; the X and Y passes are slab-local, ONE all-to-all
    (RCCL send/recv group over xGMI) re-partitions Z-slabs into Y-slabs before the Z pass.  Weak scaling.
    This leg runs its self-test and its check of the gathered result whatever `--full` says; `--dump-outputs DIR`
    writes rank 0's share of the last step's output (DIR/edtsq_rank0.npy).
  * a "step" = one complete edtsq of the (local part of the) volume.
  * roofline (--full at N = 1): dominant kernel's ALGORITHMIC bytes (pass X reads labels + writes
    fp32, passes Y/Z read labels + read/write fp32 -> 8 / 12 / 12 B per uint32 voxel) divided
    by its duration measured with hipEvents inside the library on the launch stream; beside that
    model, `real_*`: the bytes the kernels really move (PMC of a committed profile, `traffic_source`)
    over this run's times, against the 8 TB/s spec and the ~6.3 TB/s a streaming kernel reaches.
  * cpu_baseline (--full): the real reference (oracle/_ref, compiled from the reference sources) on
    this host's cores: the headline volume and the cfg3 volume, 1 thread and all threads,
    1 warm-up + best of 3, CPU model stated.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "euclidean-distance-transform-3d_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (MI355X_MICROARCH.md)
PROFILE_TAG = "r06"    # profiles/<tag>_traffic.json holds the PMC-derived HBM bytes per launch
HBM_ACHIEVABLE_GBS = 6300.0  # what a streaming kernel reaches on this part (MI355X_MICROARCH.md)
VG_NATIVE_MODEL_BPV = 42  # bytes per voxel the native voxel-graph form has to move (voxel_graph_secondary)
WARM_MS = 60.0         # untimed steps run for at least this long before the `--warmup` ones (steady clocks)


def algorithmic_bytes_per_voxel(label_bytes, fused=False):
    """X reads labels + writes fp32, Y and Z read labels + read/write fp32.  On the fused
    path the bit kernel does pass X's label read and the first column kernel does the rest of X and Y."""
    if fused:
        return {"x_bits": label_bytes, "y_pass": 4 + label_bytes + 8, "z_pass": label_bytes + 8}
    return {"x_pass": label_bytes + 4, "y_pass": label_bytes + 8, "z_pass": label_bytes + 8}


def measured_traffic(kernel=None, config="cfg2"):
    """HBM bytes per launch from the PMC passes of a round (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate
    runs, corrected as MI355X_MICROARCH.md prescribes for gfx950); tools/profile_r03.sh collects them,
    profiles/<tag>_traffic.json holds the per-kernel result.  NOT measured in this run: the returned dict names the
    file it was read from (`source`).  kernel=None: every kernel of the configuration."""
    for tag in (PROFILE_TAG,):  # (older rounds profiled other kernels: their tables do not describe this build)
        rel = os.path.join("profiles", f"{tag}_traffic.json")
        try:
            with open(os.path.join(ROOT, rel)) as f:
                blob = json.load(f)
        except (OSError, ValueError):
            continue
        if isinstance(blob.get(config, None), dict):
            entry = blob[config]
        elif "x_pass" in blob and config == "cfg2":   # (round 1: one flat table, the headline configuration)
            entry = blob
        else:
            continue                                    # this file has nothing for this configuration
        if kernel is None:
            ks = {k: v for k, v in entry.items() if isinstance(v, dict) and "total" in v}
            if ks:
                return {"kernels": ks, "source": rel}
        elif kernel in entry:
            return dict(entry[kernel], source=rel)
    return None


def whole_step_traffic(config):
    """HBM bytes of ONE whole step (all its kernels; PMC of the committed profile, see measured_traffic), or None."""
    t = measured_traffic(None, config)
    if t is None:
        return None
    return {"total": int(sum(v["total"] for v in t["kernels"].values())),
            "read": int(sum(v.get("read", 0) for v in t["kernels"].values())),
            "write": int(sum(v.get("write", 0) for v in t["kernels"].values())), "source": t["source"]}


def real_traffic_fields(ms_per_step, kernel_ms, dom, config):
    """The honest companions of the 32 B/voxel model: bytes the kernels REALLY move (PMC, from a committed profile of
    the same configuration -- not re-measured in this run), over this run's times, against the 8 TB/s spec and the
    ~6.3 TB/s a streaming kernel reaches."""
    t = measured_traffic(None, config)
    if t is None:
        return {}
    ks = t["kernels"]
    out = {"traffic_source": t["source"] + " (PMC passes of a profiling run of this configuration; constant, not "
                                           "measured in this run)"}
    if dom in ks and dom in kernel_ms:
        gbs = ks[dom]["total"] / (kernel_ms[dom] * 1e-3) / 1e9
        out.update({"real_bytes": ks[dom]["total"], "real_GBs": round(gbs, 1),
                    "real_frac_of_spec": round(gbs / HBM_PEAK_GBS, 4),
                    "real_frac_of_achievable": round(gbs / HBM_ACHIEVABLE_GBS, 4)})
    total = sum(v["total"] for v in ks.values())
    gbs = total / (ms_per_step * 1e-3) / 1e9
    out.update({"whole_job_real_bytes": int(total), "whole_job_real_GBs": round(gbs, 1),
                "whole_job_real_frac_of_spec": round(gbs / HBM_PEAK_GBS, 4),
                "whole_job_real_frac_of_achievable": round(gbs / HBM_ACHIEVABLE_GBS, 4)})
    return out


# the arithmetic the column passes compute in: exact 16-bit integer multiples of the voxel sizes' common quantum
# (csrc/edt_colq16.hip) wherever a tile's values fit, the reference's fp64 envelope arithmetic elsewhere; fp32 storage
DTYPE = "u16 integer quanta (exact) with f64 envelope fallback / f32 storage / u32 labels"


DUMP_MAX_ELEMS = 8 << 20   # --dump-outputs: at most 32 MiB of float32 per array; larger outputs are sampled
DUMP_SEED = 0


def dump_outputs(directory, arrays):
    """--dump-outputs: every array as <directory>/<name>.npy in float32 (float64 stays float64).  An array of more than
    DUMP_MAX_ELEMS elements is written as a fixed sample: DUMP_MAX_ELEMS flat indices drawn with seed DUMP_SEED and sorted,
    the same for every run of the same shape, so that two builds can be compared output for output.  Returns what was
    written, for the result line."""
    os.makedirs(directory, exist_ok=True)
    written = {}
    for name, t in arrays.items():
        flat = t.detach().reshape(-1)
        if flat.dtype != torch.float64:
            flat = flat.to(torch.float32)
        n = flat.numel()
        if n > DUMP_MAX_ELEMS:
            g = torch.Generator().manual_seed(DUMP_SEED)
            idx = torch.sort(torch.randint(n, (DUMP_MAX_ELEMS,), generator=g)).values
            flat = flat[idx.to(flat.device)]
            how = f"sample of {DUMP_MAX_ELEMS} of {n} elements (flat indices drawn with seed {DUMP_SEED}, sorted)"
        else:
            how = f"all {n} elements"
        np.save(os.path.join(directory, name + ".npy"), flat.cpu().numpy())
        written[name] = {"shape": list(t.shape), "written": how}
    return written


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def physical_cores():
    """Physical cores of the host (unique (package, core) pairs of /proc/cpuinfo); os.cpu_count() counts hardware threads."""
    try:
        seen, phys, core = set(), None, None
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("physical id"):
                    phys = line.split(":", 1)[1].strip()
                elif line.startswith("core id"):
                    core = line.split(":", 1)[1].strip()
                elif not line.strip():
                    if phys is not None and core is not None:
                        seen.add((phys, core))
                    phys = core = None
        if phys is not None and core is not None:
            seen.add((phys, core))
        if seen:
            return len(seen)
    except OSError:
        pass
    return os.cpu_count() or 1


def reference_lib():
    """The CPU checker: the compiled reference (oracle/_ref) when it travelled with the tree, else our
    plain-C restatement.  Test / baseline infrastructure only."""
    from oracle import harness
    if harness.have_ref():
        return harness.ref(fast=True), "reference"
    if not harness.have_port():
        harness.build("port")
    return harness.port(), "port"


def time_reference(lib, kind, lab, anisotropy, bb, threads):
    """1 warm-up + best of 3 per thread count; returns ({threads: Mvox/s}, last output)."""
    code = 2 if lab.dtype.itemsize == 4 else 0
    sx, sy, sz = lab.shape
    res, out = {}, None
    for p in threads:
        best = float("inf")
        for it in range(4):
            t0 = time.perf_counter()
            out = (lib.raw3d(lab, code, sx, sy, sz, anisotropy, bb, parallel=p) if kind == "reference"
                   else lib.raw3d(lab, code, sx, sy, sz, anisotropy, bb))
            dt = time.perf_counter() - t0
            if it > 0:
                best = min(best, dt)
            if it == 1 and dt > 12.0:  # a slow single-thread pass: one timed run is enough
                break
        res[p] = lab.size / best / 1e6
    return res, out


def host_round_trip(lab, an, bb, reps=4):
    """edt.edtsq(numpy) -> numpy, wall clock per call: H2D of the labels, the kernels, D2H of the result into
    a fresh array (its pages first-touched by helper threads while the labels travel)."""
    import edt
    keep, times = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        keep.append(edt.edtsq(lab, anisotropy=an, black_border=bb))  # results kept alive: no unmap in the timing
        times.append(time.perf_counter() - t0)
    ms = min(times[1:]) * 1e3
    return {"numpy_to_numpy_ms": round(ms, 2), "mvox_per_s": round(lab.size / ms / 1e3, 1),
            "bytes_over_pcie": int(lab.nbytes + lab.size * 4),
            "note": "host-buffer entry point edt_hip_edt3dsq: pageable H2D + kernels + pageable D2H into a fresh "
                    "array; best of %d after one warm-up" % (reps - 1)}


class DeviceRun:
    """One configuration resident on the device: labels, output, plan."""

    def __init__(self, name, n, dev):
        from edt import device
        from synth import config_volume
        self.name, self.n, self.dev = name, n, dev
        if name == "cfg4" and n >= 768:
            # the 4 GiB label volume is built on the device from the coarse grid (no 4 GiB host array)
            from synth import voronoi_coarse
            c = n // 4
            coarse = voronoi_coarse((c, c, c), max(8, int(round(16000 * (n / 1024.0) ** 3))), seed=1)
            t = torch.from_numpy(np.ascontiguousarray(coarse.T).view(np.int32)).to(dev)
            for ax in range(3):
                t = t.repeat_interleave(4, dim=ax)
            self.labels, self.lab_np = t.contiguous(), None
            self.an, self.bb, self.label_bytes = (1.0, 1.0, 1.0), False, 4
            shape = (n, n, n)
            self.shape = shape
        else:
            lab_np, an, bb = config_volume(name, n)
            self.lab_np, self.an, self.bb = lab_np, an, bb
            self.label_bytes = lab_np.dtype.itemsize
            shape = lab_np.shape
            self.shape = shape
            # (sx,sy,sz) Fortran array == contiguous tensor of shape (sz,sy,sx): no copy of the bytes
            self.labels = torch.from_numpy(
                np.ascontiguousarray(lab_np.T).view(np.int32 if self.label_bytes == 4 else np.uint8)).to(dev)
        self.vox = shape[0] * shape[1] * shape[2]
        self.out = torch.empty(shape[::-1], dtype=torch.float32, device=dev)
        self.plan = device.Plan(shape, 2 if self.label_bytes == 4 else 0, dev)
        # EDT_BENCH_ALTERNATE=1 (a probe, not the headline): two copies of the labels and two outputs taken in turn, so that
        # nothing a step reads or writes was touched by the step before it -- what a cache-policy change is worth when the
        # same volume is NOT transformed again and again
        self.alt = None
        if os.environ.get("EDT_BENCH_ALTERNATE") == "1":
            self.alt = (self.labels.clone(), torch.empty_like(self.out))
        self.turn = 0

    def host_labels(self):
        """The labels as an (sx, sy, sz) Fortran array on the host (a view of the device tensor's bytes when the
        volume was built on the device)."""
        if self.lab_np is not None:
            return self.lab_np
        dt = np.uint32 if self.label_bytes == 4 else np.uint8
        return self.labels.cpu().numpy().view(dt).T

    def step(self, generic=False):
        if self.alt is not None:
            self.turn ^= 1
            if self.turn:
                self.plan.run(self.alt[0], self.an, black_border=self.bb, sqrt=False, out=self.alt[1], force_generic=generic)
                self.last_out = self.alt[1]
                return
        self.plan.run(self.labels, self.an, black_border=self.bb, sqrt=False, out=self.out, force_generic=generic)
        self.last_out = self.out

    def measure(self, steps, warmup, generic=False, per_kernel=True):
        """`steps` timed steps after the warm-up; per_kernel=False: the timing alone (no profiled steps after it, no
        per-kernel fields in the summary, and `self.last_out` still holds the output of the last TIMED step)."""
        # Warm-up by TIME, then by count: a handful of sub-millisecond steps does not bring the part to its steady clocks
        # (round 4: the driver's 20-step figure sat 4 % above the 1000-step one).  At least WARM_MS of untimed steps, then
        # the `warmup` steps of the contract.
        t0 = time.perf_counter()
        extra = 0
        while (time.perf_counter() - t0) * 1e3 < WARM_MS:
            for _ in range(8):
                self.step(generic)
            torch.cuda.synchronize()
            extra += 8
        for _ in range(warmup):
            self.step(generic)
        torch.cuda.synchronize()
        # EXACTLY `steps` timed steps, as at most five batches between synchronisations.  The figure (`ms_per_step`, `value`) is
        # the MEAN over all timed steps -- the contract's statistic, and the one BENCH_r01..r04 carry (round 5
        # reported the median of the batch means, which reads lower); the median is kept beside it in `timing`.
        nb = max(1, min(5, steps))
        sizes = [steps // nb + (1 if i < steps % nb else 0) for i in range(nb)]
        batch_ms = []
        for k in sizes:
            t0 = time.perf_counter()
            for _ in range(k):
                self.step(generic)
            torch.cuda.synchronize()
            batch_ms.append((time.perf_counter() - t0) / k * 1e3)
        ms = self.ms = float(np.dot(batch_ms, sizes) / steps)
        self.timing = {"statistic": "mean over all timed steps", "batches": sizes, "batch_ms": [round(b, 4) for b in batch_ms],
                       "mean_ms": round(ms, 4), "median_of_batch_means_ms": round(float(np.median(batch_ms)), 4),
                       "untimed_steps_before": extra + warmup, "warm_ms": WARM_MS}
        if not per_kernel:
            return {"ms_per_step": round(ms, 4), "mvox_per_s": round(self.vox / (ms * 1e-3) / 1e6, 1)}, None, None
        return self.kernel_times(ms, steps, generic)

    def kernel_times(self, ms, steps, generic=False):
        """Per-kernel durations with hipEvents on the launch stream, in profiled steps of their own after the timed ones;
        returns measure()'s summary (ms_per_step and the whole-job model fields) with them."""
        from edt import device
        device.set_profiling(True)
        acc = {}
        for _ in range(max(3, min(steps, 10))):
            self.step(generic)
            torch.cuda.synchronize()
            for name, t in device.pass_times():
                acc.setdefault(name, []).append(t)
        device.set_profiling(False)
        kernels = {k: float(np.mean(v)) for k, v in acc.items()}
        bpv = algorithmic_bytes_per_voxel(self.label_bytes, "x_bits" in kernels)
        whole = sum(bpv.values()) * self.vox / (ms * 1e-3) / 1e9
        return {
            "ms_per_step": round(ms, 4), "mvox_per_s": round(self.vox / (ms * 1e-3) / 1e6, 1),
            "kernel_ms": {k: round(v, 4) for k, v in kernels.items()},
            "whole_job_algorithmic_GBs": round(whole, 1), "whole_job_frac": round(whole / HBM_PEAK_GBS, 4),
        }, kernels, bpv


def voxel_graph_secondary(n, dev, steps, warmup, ref=None):
    """BASELINE configs[4]: the voxel-connectivity-graph transform of an n^3 uint8 blob volume (1 % of the +x links
    cut), device-resident.  Full-size parity of this path: tests/test_gpu_voxel_graph.py."""
    from edt import device
    rng = np.random.default_rng(5)
    small = (rng.random((n // 16,) * 3) < 0.6).astype(np.uint8)
    lab = torch.from_numpy(np.ascontiguousarray(small.repeat(16, 0).repeat(16, 1).repeat(16, 2))).to(dev)
    g = torch.full((n, n, n), 0b00111111, dtype=torch.uint8, device=dev)
    g[torch.rand((n, n, n), device=dev) < 0.01] = 0b00111110
    an = (30.0, 6.0, 6.0)  # (z, y, x)
    for _ in range(max(2, warmup // 4)):
        device.edtsq_voxel_graph(lab, g, anisotropy=an, black_border=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        device.edtsq_voxel_graph(lab, g, anisotropy=an, black_border=True)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    entry = {"config": "cfg5", "workload": f"{n}^3 uint8 blobs + voxel graph (1 % of the +x links cut), anisotropy (6, 6, 30), "
                                           "black_border=True, device-resident in/out, 1 GPU",
             "ms_per_step": round(ms, 4), "mvox_per_s": round(n ** 3 / (ms * 1e-3) / 1e6, 1), "output_verified": None}
    # A byte model for the NATIVE form (SURVEY 8(d)'s 202 B/voxel prices the reference's 8x up-sampled volume, which no longer
    # exists here): labels + graph read once by pass X (2 B) and once by each of the two bit-plane kernels (4 B); pass X
    # writes the even-X cells of the four doubled rows of a voxel row as 16-bit indices (8 B); pass Y reads them (8 B) and
    # writes its even rows compactly as fp32 (8 B); pass Z reads those (8 B) and writes the result (4 B): 42 B per voxel.
    model = VG_NATIVE_MODEL_BPV * n ** 3 / (ms * 1e-3) / 1e9
    entry.update({"model_bytes_per_voxel": VG_NATIVE_MODEL_BPV, "model_GBs": round(model, 1), "model_frac": round(model / HBM_PEAK_GBS, 4),
                  "model_note": "native even-cell form: X 2 + 8, bit planes 2 x 2, Y 8 + 8, Z 8 + 4 bytes per voxel"})
    if n == 512:
        entry.update(real_traffic_fields(ms, {}, None, "cfg5"))
    if ref is not None and os.environ.get("EDT_BENCH_VERIFY", "1") != "0":
        # the timed output against the compiled reference's own voxel-graph transform (single-threaded upstream:
        # about a minute at 512^3 -- src/edt_voxel_graph.hpp:120-214)
        got = device.edtsq_voxel_graph(lab, g, anisotropy=an, black_border=True).cpu().numpy().T
        lab_np, g_np = lab.cpu().numpy().T, g.cpu().numpy().T   # (sx, sy, sz) Fortran views
        t0 = time.perf_counter()
        want = ref.edtsq(lab_np, (6.0, 6.0, 30.0), True, voxel_graph=g_np)
        dt = time.perf_counter() - t0
        entry["output_verified"] = bool(np.array_equal(got, want))
        entry["verified_by"] = "compiled CPU reference (_edt3dsq_voxel_graph, 1 thread), %.1f s = %.1f Mvox/s" % (dt, n ** 3 / dt / 1e6)
    return entry


def sdf_secondary(n, dev, steps, warmup, ref=None):
    """The sdf leg of BASELINE configs[4]: sdf = edt(x) - edt(x == 0) (src/edt.pyx:121-158) of the n^3 uint8 blob volume,
    device-resident in and out.  Byte model of SURVEY 8(d): two transforms of 1-byte labels (3 x 1 + 5 x 4 = 23 B/voxel each)
    + the combine (two fields read, one written: 12 B/voxel) = 58 B/voxel.  Full-size parity of this path:
    tests/test_gpu_fullsize.py::test_cfg5_512_sdf_against_compiled_reference."""
    from edt import device
    from synth import config_volume
    lab_np, _, _ = config_volume("cfg5", n)
    an, bb = (6.0, 6.0, 30.0), True
    lab = torch.from_numpy(np.ascontiguousarray(lab_np.T)).to(dev)
    for _ in range(max(2, warmup // 2)):
        device.sdf(lab, anisotropy=an[::-1], black_border=bb)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        got_t = device.sdf(lab, anisotropy=an[::-1], black_border=bb)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    # (beside it: the definition executed literally -- two transforms, the background mask and the subtraction)
    for _ in range(2):
        device._signed(lab, an[::-1], bb, sqrt=True, one_transform=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(max(3, steps // 2)):
        device._signed(lab, an[::-1], bb, sqrt=True, one_transform=False)
    torch.cuda.synchronize()
    ms2 = (time.perf_counter() - t0) / max(3, steps // 2) * 1e3
    # Two byte models.  SURVEY 8(d) prices the DEFINITION: two transforms of 1-byte labels + the combine = 58 B/voxel.  The form
    # that runs is ONE transform whose last pass negates the background in its epilogue (3 x 1 + 5 x 4 = 23 B/voxel; the
    # foreground plane it reads for that is 1/8 byte per voxel) -- the fraction reported is against that one (against the
    # definition's bytes it reads above 1: the second transform is not executed).
    bpv_def = 2 * sum(algorithmic_bytes_per_voxel(1).values()) + 12
    bpv = sum(algorithmic_bytes_per_voxel(1).values())
    model = bpv * n ** 3 / (ms * 1e-3) / 1e9
    entry = {"config": "cfg5_sdf", "workload": f"{n}^3 uint8 blobs: sdf = edt(x) - edt(x == 0), anisotropy {an}, black_border={bb}, "
                                               "device-resident in/out, 1 GPU",
             "ms_per_step": round(ms, 4), "mvox_per_s": round(n ** 3 / (ms * 1e-3) / 1e6, 1),
             "model_bytes_per_voxel": bpv, "whole_job_algorithmic_GBs": round(model, 1), "whole_job_frac": round(model / HBM_PEAK_GBS, 4),
             "model_note": "one transform of 1-byte labels (3 x 1 + 5 x 4 B/voxel), the background's sign in the epilogue of its last pass",
             "definition_model_bytes_per_voxel": bpv_def,
             "definition_model_note": "SURVEY 8(d): 2 x (3 x 1 + 5 x 4) B/voxel for the two transforms of 1-byte labels + 12 B/voxel "
                                      "combine -- what two_transform_ms executes",
             "definition_model_frac_of_two_transform_run": round(bpv_def * n ** 3 / (ms2 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
             "form": "ONE transform (EDT_FLAG_SIGNED: label 0 measured like every label, its voxels negated by the last pass) -- "
                     "bit-identical to the definition; two_transform_ms: the definition executed literally on the device",
             "two_transform_ms": round(ms2, 4),
             "output_verified": None}
    if ref is not None and os.environ.get("EDT_BENCH_VERIFY", "1") != "0":
        cores = os.cpu_count() or 1
        t0 = time.perf_counter()
        want = ref.sdf(lab_np, an, bb, parallel=cores)
        dt = time.perf_counter() - t0
        entry["output_verified"] = bool(np.array_equal(got_t.cpu().numpy().T, want))
        entry["verified_by"] = "compiled CPU reference (edt(x) - edt(x == 0), %d threads), %.2f s = %.1f Mvox/s" % (cores, dt, n ** 3 / dt / 1e6)
    return entry


def snemi_like_secondary(dev, ref, kind):
    """The reference's own headline use case (README.md:335-355, Fig. 3: SNEMI3D 512x512x100, 334 labels): ONE
    multi-label EDT, then the per-label image `res * (labels == segid)` for every label.  Here: device-resident
    edt + edt.device.each (run table on the device, one streaming kernel per label over the label's span) against the
    same loop on the host (compiled reference edt with all threads + numpy masks, exactly the README's edt_test)."""
    from edt import device
    from synth import voronoi_full
    shape = (512, 512, 100)
    lab_np = voronoi_full(shape, 334, seed=7)
    an = (4.0, 4.0, 40.0)
    t = torch.from_numpy(np.ascontiguousarray(lab_np.T).view(np.int32)).to(dev)

    def gpu_job(keep=None):
        dt = device.edt(t, anisotropy=an[::-1], black_border=False)
        n = 0
        for key, img in device.each(t, dt, in_place=True):
            if keep is not None and int(key) in keep:
                keep[int(key)] = img.clone()
            n += 1
        torch.cuda.synchronize()
        return n

    gpu_job()
    t0 = time.perf_counter()
    nlab = gpu_job()
    gpu_s = time.perf_counter() - t0
    entry = {"config": "snemi_like", "workload": "512x512x100 uint32, 334 full-resolution Voronoi labels, anisotropy "
             "(4, 4, 40), black_border=False: ONE edt + the per-label image res * (labels == id) for EVERY label "
             "(reference README.md:335-355), device-resident",
             "labels": nlab, "gpu_seconds_total": round(gpu_s, 4), "gpu_ms_per_label": round(gpu_s / nlab * 1e3, 4)}
    if ref is not None and kind == "reference":
        cores = os.cpu_count() or 1
        t0 = time.perf_counter()
        res = np.sqrt(ref.raw3d(lab_np, 2, shape[0], shape[1], shape[2], an, False, parallel=cores)).reshape(shape, order="F")
        t_edt = time.perf_counter() - t0
        ids = np.unique(lab_np)
        ids = ids[ids != 0]
        rng = np.random.default_rng(1)
        check = {int(k): None for k in rng.choice(ids, size=5, replace=False)}
        t0 = time.perf_counter()
        host_imgs = {}
        for k in ids:
            img = res * (lab_np == k)
            if int(k) in check:
                host_imgs[int(k)] = img
        t_each = time.perf_counter() - t0
        gpu_job(check)
        entry.update({"host_seconds_total": round(t_edt + t_each, 3), "host_edt_seconds": round(t_edt, 3),
                      "host_note": f"compiled reference edt ({cores} threads) + numpy res * (labels == id) per label, 1 thread",
                      "speedup": round((t_edt + t_each) / gpu_s, 1),
                      "output_verified": bool(all(check[k] is not None and np.array_equal(check[k].cpu().numpy().T, host_imgs[k])
                                                  for k in check)),
                      "verified_by": "5 random labels, bit for bit against the host loop"})
    return entry


# ------------------------------------------------------------------------------------------
# the N > 1 leg: one process per GPU, the volume Z-sharded (edt/distributed.py)
# ------------------------------------------------------------------------------------------
def slab_labels(ext, zs, ze, dev, kind="cfg4"):
    """This rank's Z-slab [zs, ze) of the global benchmark volume, built on the device.

    cfg4 (BASELINE configs[3]): nearest-seed segmentation, 16 000 seeds per 1024^3 voxels on a grid four
    times coarser (seed 1), up-sampled x4 -- every rank queries only the coarse slices its slab needs."""
    if kind == "ones":
        return torch.ones((ze - zs, ext[1], ext[0]), dtype=torch.int32, device=dev)
    from synth import voronoi_coarse
    coarse = tuple(-(-e // 4) for e in ext)
    nseeds = max(8, int(round(16000 * (ext[0] * ext[1] * ext[2]) / 1024.0 ** 3)))
    c0, c1 = zs // 4, -(-ze // 4)
    lab = voronoi_coarse(coarse, nseeds, seed=1, zrange=(c0, c1))           # (cx, cy, c1-c0), Fortran order
    t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).to(dev)  # (cz, cy, cx)
    for ax in range(3):
        t = t.repeat_interleave(4, dim=ax)
    return t[zs - 4 * c0:ze - 4 * c0, :ext[1], :ext[0]].contiguous()


def sharded_main(args, rank, world, dev):
    import torch.distributed as dist
    from edt import _lib
    from edt.distributed import ShardedEDT, global_extents
    # Three readings of a --gpus N line (stated in the line itself: "scaling", "reading"):
    #   default               WEAK scaling on configs[3]: args.size^3 voxels of the multi-label segmentation per GPU
    #   --labels ones         WEAK scaling on the headline's workload (configs[1]: single label, (6,6,30), black border):
    #                         the series that continues the --gpus 1 headline
    #   --global-size S       STRONG scaling: ONE S^3 volume whatever N (the metric's "512^3 @ 1/2/4/8 GPU" read literally)
    kind = args.labels or os.environ.get("EDT_BENCH_LABELS", "cfg4")  # "ones": the single-label box (closed-form check)
    strong = args.global_size > 0
    ext = (args.global_size,) * 3 if strong else global_extents(world, args.size)
    an, bb = ((6.0, 6.0, 30.0), True) if kind == "ones" else ((1.0, 1.0, 1.0), False)
    if (args.selftest or world > 1) and not args.no_selftest:
        selftest(rank, world, dev, ext, kind)
    # Steps are independent transforms: `depth` of them are in flight, each on its own plan (its own buffers and scratch) and
    # its own stream, taken in turn -- the Z phase of step i then runs while the XY phase of step i + 1 feeds the links,
    # instead of the links idling through it.  Every rank issues the same collectives in the same order.  (--pipeline 1:
    # one plan, one stream, nothing of step i + 1 before step i has finished.)
    depth = args.pipeline if args.pipeline > 0 else (2 if world > 1 else 1)   # (one rank: nothing travels, nothing to hide)
    plans = [ShardedEDT(ext, _lib.U32, reuse_output=True) for _ in range(depth)]  # (a step's result is consumed before its plan's next)
    plan = plans[0]
    lanes = [torch.cuda.Stream(dev) for _ in range(depth)] if depth > 1 else [None]
    zs, ze = plan.local_z()
    labels = slab_labels(ext, zs, ze, dev, kind)
    torch.cuda.synchronize()
    turn = [0]

    def step():
        i = turn[0] % depth
        turn[0] += 1
        if lanes[i] is None:
            return plans[i].run(labels, an, black_border=bb)
        with torch.cuda.stream(lanes[i]):
            return plans[i].run(labels, an, black_border=bb)

    for _ in range(max(args.warmup, depth)):
        step()
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    host_enqueue = time.perf_counter() - t0   # (what the host spent inside run(): enqueueing, and waiting for the records' agreement)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    elapsed = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
    dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    elapsed = float(elapsed.item())

    # (everything below -- per-kernel times, the exposed exchange, the check -- on ONE plan and the current stream)
    last_plan = plans[(turn[0] - 1) % depth]
    depth_timed, depth, lanes[:] = depth, 1, [None]
    plans[0] = last_plan   # (`out` is its result)
    plan = last_plan
    # The other reading of the same job, in the same line: ONE volume at a time -- one plan, one stream, nothing of
    # step i + 1 before step i has finished -- i.e. the latency of a step, comparable with the --gpus 1 line and with the
    # SCALE records of earlier rounds; `value` / `ms_per_step` above are throughput with `steps_in_flight` steps in flight.
    serial = None
    if depth_timed > 1:
        n1 = max(3, min(args.steps, 50))
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(n1):
            out = step()
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()
        e1 = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
        dist.all_reduce(e1, op=dist.ReduceOp.MAX)
        serial = {"steps_in_flight": 1, "steps": n1, "ms_per_step": round(float(e1.item()) / n1 * 1e3, 4)}
    # per-kernel durations of one more step (hipEvents inside the library, this rank's stream)
    from edt import device
    acc = {}
    for _ in range(3):
        device.set_profiling(True)
        step()
        torch.cuda.synchronize()
        for name, ms in device.pass_times():
            acc.setdefault(name, []).append(ms)
    device.set_profiling(False)
    kernel_ms = {k: float(np.sum(v)) / 3 for k, v in acc.items()}  # chunks of a step add up
    dist.barrier()
    # exposed exchange: events on the compute stream around the waits for the records (edt/distributed.py), in steps of
    # their own (the per-kernel events above serialise the chunks' streams)
    exposed = []
    if plan.records:
        plan.measure_exchange = True
        for _ in range(5):
            step()
            torch.cuda.synchronize()
            exposed.append(plan.exposed_ms())
        plan.measure_exchange = False
    exposed_t = torch.tensor([float(np.mean(exposed[1:])) if len(exposed) > 1 else -1.0], dtype=torch.float64, device=dev)
    dist.all_reduce(exposed_t, op=dist.ReduceOp.MAX)
    dist.barrier()

    ys, ye = plan.local_y()
    # what travels: this rank's slab records for every OTHER rank (4 B x record length x its slices), max over ranks
    sent = 0
    if plan.records:
        # (16-bit rows where the integer kernel takes both column passes: 2.25 bytes per voxel instead of 4.25)
        rec = [(plan.ops.record16_words if plan.last_records16 else plan.ops.record_floats)(plan.sx, b - a) for a, b in plan.yparts]
        sent = 4 * (ze - zs) * sum(rec[h] for h in range(world) if h != rank)
    else:
        sent = 5 * sum((ze - zs) * (b - a) * plan.sx for h, (a, b) in enumerate(plan.yparts) if h != rank)
    sent_t = torch.tensor([sent], dtype=torch.int64, device=dev)
    dist.all_reduce(sent_t, op=dist.ReduceOp.MAX)
    ksum = torch.tensor([sum(kernel_ms.values())], dtype=torch.float64, device=dev)
    dist.all_reduce(ksum, op=dist.ReduceOp.MAX)
    cpu = None
    if kind == "ones":
        # correctness of the timed output: closed form of the all-ones box on this rank's y-slab
        idx = [torch.arange(e, device=dev, dtype=torch.float64) for e in ext]
        d = [torch.minimum(i + 1, e - i) * w for i, e, w in zip(idx, ext, an)]
        want = torch.minimum(torch.minimum((d[2] ** 2)[:, None, None], (d[1][ys:ye] ** 2)[None, :, None]),
                             (d[0] ** 2)[None, None, :]).to(torch.float32)
        ok = torch.tensor([1 if torch.equal(out, want) else 0], device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        verified, how = bool(ok.item()), "closed form of the box"
    else:
        verified, how, cpu = _verify_against_reference(plan, labels, out, ext, an, bb, rank, world, dev)

    # the SAME kind of volume on ONE GPU (args.size^3 voxels of the same segmentation density, single-device
    # path), timed on rank 0 while the others wait: what `value` of this weak-scaling line is to be compared with
    # (the --gpus 1 line's headline is the single-label box, a lighter workload)
    same_n1 = None
    if rank == 0:
        try:
            from edt import device as _dev
            cube = ext if strong else (args.size,) * 3   # strong scaling: the SAME volume on one GPU
            lab1 = slab_labels(cube, 0, cube[2], dev, kind)
            out1 = torch.empty(cube[::-1], dtype=torch.float32, device=dev)
            plan1 = _dev.Plan(cube, _lib.U32, dev)
            for _ in range(3):
                plan1.run(lab1, an, black_border=bb, out=out1)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(10):
                plan1.run(lab1, an, black_border=bb, out=out1)
            torch.cuda.synchronize()
            ms1 = (time.perf_counter() - t1) / 10 * 1e3
            vox1 = cube[0] * cube[1] * cube[2]
            same_n1 = {"ms_per_step": round(ms1, 4), "mvox_per_s": round(vox1 / ms1 / 1e3, 1),
                       "what": f"{cube[0]}x{cube[1]}x{cube[2]} voxels of the same workload on ONE GPU (single-device path), rank 0"}
            del lab1, out1, plan1
        except Exception as e:  # pragma: no cover
            same_n1 = {"error": repr(e)}
    dist.barrier()

    if rank == 0:
        vox = ext[0] * ext[1] * ext[2]
        # roofline of the dominant kernel ON ONE RANK: its algorithmic bytes (X reads
        # labels + writes fp32; Y and Z read labels + read / write fp32) over its summed duration
        bpv = {"x_pass": 4 + 4, "y_pass": 4 + 8, "z_pass": 4 + 8}
        roofline = None
        if any(k in kernel_ms for k in bpv):
            dom = max((k for k in kernel_ms if k in bpv), key=lambda k: kernel_ms[k])
            achieved = bpv[dom] * (vox / world) / (kernel_ms[dom] * 1e-3) / 1e9
            whole = 32.0 * vox / (elapsed / args.steps) / 1e9
            roofline = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 1), "peak": 8000.0,
                        "unit": "GB/s", "frac": round(achieved / 8000.0, 4), "traffic": None,
                        "kernel_ms": {k: round(v, 4) for k, v in kernel_ms.items()},
                        "whole_job_algorithmic_GBs": round(whole, 1),
                        "whole_job_frac": round(whole / (8000.0 * world), 4),
                        "note": "per rank; the exchange is not a kernel of this library and is not listed; "
                                "whole_job_frac = 32 B/voxel over ms_per_step against world x 8 TB/s"}
        value = round(vox / (elapsed / args.steps) / 1e6, 1)
        what = "single label (configs[1], the --gpus 1 headline's workload)" if kind == "ones" else \
            "multi-label segmentation, 16000 seeds per 1024^3 (configs[3])"
        if strong:
            reading = (f"STRONG scaling: the same {ext[0]}^3 volume ({what}) on {world} GPU(s); "
                       "scaling_efficiency = value / (n_gpus x the same volume's rate on one GPU)")
        elif kind == "ones":
            reading = (f"WEAK scaling on the headline workload: {args.size}^3 voxels per GPU of the single-label box; continues the "
                       "--gpus 1 headline; scaling_efficiency = value / (n_gpus x one GPU's rate on its share)")
        else:
            reading = (f"WEAK scaling on configs[3]: {args.size}^3 voxels per GPU of the multi-label segmentation -- NOT the --gpus 1 "
                       "headline's workload (single label); compare with single_gpu_same_workload, not with the N = 1 line; "
                       "scaling_efficiency = value / (n_gpus x single_gpu_same_workload.mvox_per_s)")
        if depth_timed > 1:
            reading += (f"; the K timed steps are independent transforms and {depth_timed} are in flight at a time (own plan and stream each: "
                        "the Z phase of one runs under the XY phase and exchange of the next; --pipeline 1 for strictly one after the other)")
        eff = None
        if same_n1 and same_n1.get("mvox_per_s"):
            eff = round(value / (world * same_n1["mvox_per_s"]), 4)
        line = {
            "metric": "Mvox/s edt3dsq 512^3 uint32", "value": value,
            "unit": "Mvox/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "reading": reading,
            # both readings of the job: `value` / `ms_per_step` = the first (what the K timed steps ran as)
            "readings": [{"steps_in_flight": depth_timed, "steps": args.steps, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
                          "mvox_per_s": value, "what": "throughput: independent transforms pipelined over plans / streams"
                          if depth_timed > 1 else "one volume at a time (latency = throughput)"}]
                        + ([dict(serial, mvox_per_s=round(vox / (serial["ms_per_step"] * 1e-3) / 1e6, 1),
                                 what="latency: one volume at a time, one plan, one stream")] if serial else []),
            "single_gpu_same_workload": same_n1,
            "scaling_efficiency": eff,
            "dtype": DTYPE, "data": "synthetic",
            "config": {"workload": f"{'STRONG' if strong else 'WEAK'} scaling: one {ext[0]}x{ext[1]}x{ext[2]} uint32 volume"
                                   f"{'' if strong else f' = {args.size}^3 voxels per GPU'} ({what}), "
                                   f"anisotropy {an}, black_border={bb}, Z-sharded over {world} GPUs, "
                                   "one all-to-all (Z-slabs -> Y-slabs) before the z pass",
                       "labels": kind, "global_extents": list(ext),
                       "form": ("slab records, 16-bit rows" if plan.last_records16 else "slab records, fp32 rows") if plan.records
                               else "byte flags",
                       "records16_fallbacks": getattr(plan, "fallbacks16", 0),
                       "steps_in_flight": depth_timed,
                       "chunks": getattr(plan, "nchunks", 1),
                       "output_verified": verified, "verified_by": how,
                       "single_gpu_same_workload": same_n1},
            "roofline": roofline,
            # how to read a SCALE curve: per-rank kernel time (rank 0, per step, chunks summed), the slowest rank's
            # kernel sum, the exposed part of the exchange (measured with events around the waits; ~0 when it hides
            # under the next chunk's kernels), and the bytes the busiest rank sends per step over xGMI
            # (7 links x 153.6 GB/s bidirectional = 76.8 GB/s per direction: bytes / (world - 1) per link)
            "per_rank": {"kernel_ms": {k: round(v, 4) for k, v in kernel_ms.items()},
                         "kernel_ms_note": "hipEvents per kernel, chunks summed; chunks run on two streams, so overlapping "
                                           "kernels are each timed at their stretched duration and the sum may exceed the step",
                         "kernel_ms_sum_max_over_ranks": round(float(ksum.item()), 4),
                         "exchange_ms_exposed": (round(float(exposed_t.item()), 4) if float(exposed_t.item()) >= 0 else None),
                         "exchange_ms_exposed_note": "events on the compute stream around the waits for the slab records: how long "
                                                     "the slowest rank sat between its last XY kernel and the last record's arrival",
                         "host_ms_per_step_in_run": round(host_enqueue / max(1, args.steps) * 1e3, 4),
                         "host_ms_note": "rank 0's wall time inside plan.run() per step (enqueue + the wait for the 16-bit records' "
                                         "agreement, which ends when the last exchange has landed): close to ms_per_step = the host is the bound",
                         "bytes_exchanged": int(sent_t.item()),
                         "link_floor_ms": round(int(sent_t.item()) / max(1, world - 1) / 76.8e9 * 1e3, 4) if world > 1 else 0.0},
        }
        if cpu is not None:
            line["cpu_baseline"] = cpu
    if rank == 0 and args.dump_outputs:
        line["outputs"] = {"dir": args.dump_outputs, "arrays": dump_outputs(args.dump_outputs, {"edtsq_rank0": out}),
                           "what": "edtsq_rank0: rank 0's (z, y-slab, x) float32 share of the last step's output, flattened"}
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        # RCCL prints a version banner through C stdio (buffered when stdout is a pipe): push it out first, so that the
        # JSON line is the LAST thing on stdout
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(json.dumps(line), flush=True)


def selftest(rank, world, dev, ext, kind):
    """Before anything is timed: what a failure on a multi-GPU box has to be diagnosed from.  Rank 0 prints (stdout, prefix
    [selftest]) the RCCL version, the peer-access matrix of the visible devices, the per-peer message sizes of the
    all-to-all of the run to come, and the result of one tiny sharded transform checked bit for bit against the CPU
    checker.  Any exception is printed with its rank and re-raised."""
    import torch.distributed as dist
    from edt import _lib
    from edt.distributed import ShardedEDT

    def say(*a):
        if rank == 0:
            print("[selftest]", *a, flush=True)

    try:
        try:
            nccl = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception as e:  # pragma: no cover
            nccl = f"unknown ({e!r})"
        say(f"torch {torch.__version__}, backend {dist.get_backend()}, RCCL/NCCL {nccl}, world {world}, "
            f"devices visible to rank 0: {torch.cuda.device_count()}, HSA_ENABLE_IPC_MODE_LEGACY={os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')}")
        ndev = torch.cuda.device_count()
        me = dev.index if dev.index is not None else torch.cuda.current_device()
        row = [1 if (j == me or torch.cuda.can_device_access_peer(me, j)) else 0 for j in range(ndev)]
        rows = [None] * world
        dist.all_gather_object(rows, (rank, me, torch.cuda.get_device_name(me), row))
        for r, d, name, acc in rows:
            say(f"rank {r}: cuda:{d} {name}, peer access to cuda:0..{len(acc) - 1}: {acc}")
        # message sizes of the real run (slab records): what rank r sends to rank h per chunk and per step
        plan = ShardedEDT(ext, _lib.U32)
        if plan.records:
            an = (6.0, 6.0, 30.0) if kind == "ones" else (1.0, 1.0, 1.0)  # (the voxel sizes of the run to come: sharded_leg)
            use16 = plan._use16(an)
            say(f"slab records with {'16-bit rows (2.25 B/voxel; a step that meets a tile beyond 16 bits is repeated with fp32 rows)' if use16 else 'fp32 rows (4.25 B/voxel)'}")
            rec = [(plan.ops.record16_words if use16 else plan.ops.record_floats)(plan.sx, b - a) for a, b in plan.yparts]
            for r in range(world):
                per_chunk = [[4 * (plan._chunk(r, k)[1] - plan._chunk(r, k)[0]) * rec[h] if h != r else 0 for h in range(world)]
                             for k in range(plan.nchunks)]
                if r == 0 or r == world - 1:
                    say(f"all_to_all of rank {r}: {plan.nchunks} chunk(s), bytes to each rank per chunk {per_chunk[0]}"
                        f"{' ... ' + str(per_chunk[-1]) if plan.nchunks > 1 else ''}, per step {sum(sum(c) for c in per_chunk)}")
        else:
            say("the slab-record form does not apply to these extents: byte-flag form (one group of point-to-point transfers)")
        say(f"y ranges per rank {plan.yparts}, z ranges per rank {plan.zparts}")
        del plan
        # one tiny sharded transform, verified: uneven cuts on purpose
        small = (96, 32 * world + 40, 8 * world + 5)
        tiny = ShardedEDT(small, _lib.U32, chunks=2)
        zs, ze = tiny.local_z()
        lab = slab_labels(small, zs, ze, dev, "cfg4")
        out = tiny.run(lab, (1.0, 1.0, 2.0), black_border=False)
        torch.cuda.synchronize()
        ok, how, _ = _verify_against_reference(tiny, lab, out, small, (1.0, 1.0, 2.0), False, rank, world, dev, force=True)
        say(f"tiny volume {small} over {world} rank(s), form {'slab records' if tiny.records else 'byte flags'}: "
            f"output_verified={ok} ({how})")
        dist.barrier()
        if rank == 0 and ok is False:
            raise SystemExit("[selftest] the tiny sharded transform differs from the CPU checker")
        # ... and one whose axes are long enough for the 16-bit records (97..1024 rows of y and z), at voxel sizes that share a quantum
        small16 = (64, 32 * world + 72, 8 * world + 97)
        tiny16 = ShardedEDT(small16, _lib.U32, chunks=2)
        zs, ze = tiny16.local_z()
        lab = slab_labels(small16, zs, ze, dev, "cfg4")
        out = tiny16.run(lab, (6.0, 6.0, 30.0), black_border=True)
        torch.cuda.synchronize()
        ok, how, _ = _verify_against_reference(tiny16, lab, out, small16, (6.0, 6.0, 30.0), True, rank, world, dev, force=True)
        say(f"tiny volume {small16} over {world} rank(s), 16-bit records used: {tiny16.last_records16} (fallbacks {tiny16.fallbacks16}): "
            f"output_verified={ok} ({how})")
        dist.barrier()
        if rank == 0 and ok is False:
            raise SystemExit("[selftest] the tiny sharded transform over 16-bit records differs from the CPU checker")
    except BaseException as e:
        print(f"[selftest] rank {rank} FAILED: {e!r}", flush=True)
        raise


def _verify_against_reference(plan, labels, out, ext, an, bb, rank, world, dev, force=False):
    """Bit-for-bit check of the timed multi-GPU output: rank 0 collects every rank's label slab and result
    slab and runs the CPU reference (oracle/_ref, test infrastructure) on the whole volume with all host
    threads.  Returns (verified | None, how, cpu_baseline | None).  EDT_BENCH_VERIFY=0 skips it."""
    import torch.distributed as dist
    if os.environ.get("EDT_BENCH_VERIFY", "1") == "0" and not force:
        return None, "skipped (EDT_BENCH_VERIFY=0)", None
    have = torch.tensor([0], device=dev)
    lib = None
    if rank == 0:
        try:
            from oracle import harness
            if harness.have_ref():
                lib = harness.ref(fast=True)
                have[0] = 1
            elif force and harness.have_port():  # (the self-test's tiny volume: the plain-C restatement serves)
                lib = harness.port()
                have[0] = 1
        except Exception:
            lib = None
    dist.broadcast(have, 0)
    if int(have.item()) == 0:
        return None, "skipped (oracle/_ref not present)", None
    sx, sy, sz = ext
    stage = dist.get_backend() == "gloo"

    def send(t):
        t = t.contiguous()
        dist.send(t.cpu() if stage else t, 0)

    def recv(shape, dtype, src):
        buf = torch.empty(shape, dtype=dtype, device="cpu" if stage else dev)
        dist.recv(buf, src)
        return buf.cpu()

    if rank != 0:
        send(labels)
        send(out)
        return None, "", None
    lab_full = np.empty((sz, sy, sx), dtype=np.int32)
    res_full = np.empty((sz, sy, sx), dtype=np.float32)
    for r in range(world):
        zs, ze = plan.zparts[r]
        ys, ye = plan.yparts[r]
        if r == 0:
            lab_r, out_r = labels.cpu(), out.contiguous().cpu()
        else:
            lab_r = recv((ze - zs, sy, sx), torch.int32, r)
            out_r = recv((sz, ye - ys, sx), torch.float32, r)
        lab_full[zs:ze] = lab_r.numpy()
        res_full[:, ys:ye, :] = out_r.numpy()
    cores = os.cpu_count() or 1
    t0 = time.perf_counter()
    want = lib.raw3d(lab_full.view(np.uint32), 2, sx, sy, sz, an, bb, parallel=cores)
    dt = time.perf_counter() - t0
    ok = bool(np.array_equal(want, res_full.reshape(-1)))
    model = cpu_model()
    cpu = {"value": round(sx * sy * sz / dt / 1e6, 2), "unit": "Mvox/s", "cores": physical_cores(), "host_threads": cores,
           "kind": "reference",
           "cpu": model, "sample": f"the whole {sx}x{sy}x{sz} volume of this run, one pass with {cores} threads "
                                   "(the pass that also checks the GPU output bit for bit)"}
    return ok, f"compiled CPU reference on the whole volume, {cores} threads", cpu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)   # 0.65 s of timed kernels: long enough for a busy-sampler to see
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, default=512, help="edge length of the per-GPU volume")
    from synth import SWEEP
    ap.add_argument("--config", default="cfg2", choices=["cfg1", "cfg2", "cfg3", "cfg3f", "cfg3m", "cfg4", "cfg5", "cfg3L", "cfg3La",
                                                        "cfg3M", "cfg3Ma"] + sorted(SWEEP))
    ap.add_argument("--secondary", default="", help="comma-separated subset of the secondary configurations")
    ap.add_argument("--labels", default="", choices=["", "cfg4", "ones"],
                    help="--gpus N > 1: the workload of the sharded leg -- cfg4 (default: the multi-label segmentation of "
                         "configs[3]) or ones (the single-label box of the --gpus 1 headline: an apples-to-apples series)")
    ap.add_argument("--global-size", type=int, default=0,
                    help="--gpus N > 1: STRONG scaling -- one volume of this edge length whatever N (0: weak scaling, "
                         "--size^3 voxels per GPU)")
    ap.add_argument("--pipeline", type=int, default=0,
                    help="N > 1 leg: independent steps in flight, each on its own plan and stream (default: 2 at N > 1; 1: strictly "
                         "one after the other)")
    ap.add_argument("--selftest", action="store_true", help="run the sharded leg's self-test also at world size 1")
    ap.add_argument("--no-selftest", action="store_true", help="skip the self-test of the sharded leg (default at N > 1: run it)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="headline configuration only")
    ap.add_argument("--generic", action="store_true", help="force the size-agnostic fallback kernels")
    ap.add_argument("--full", action="store_true",
                    help="--gpus 1: beyond the headline figure, also the per-kernel times and roofline, the check of the timed output, "
                         "the numpy round trip, the secondary configurations and the CPU baseline (off: set up, warm up, time "
                         "the steps, print the line)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32; outputs "
                         "larger than 32 MiB as a fixed seeded sample)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with {args.gpus} ranks")

    import edt  # noqa: F401
    from edt import _lib

    _lib.load()
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    if os.environ.get("EDT_BENCH_ONE_GPU") == "1":  # dry run of the N > 1 leg: every rank on cuda:0 (with gloo)
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    n = args.size
    if world > 1 or os.environ.get("EDT_BENCH_FORCE_SHARDED") == "1":  # (the env var: 1-rank dry run of the N > 1 leg)
        import torch.distributed as dist
        backend = os.environ.get("EDT_BENCH_BACKEND", "nccl")  # "gloo": dry run, transfers staged through the host
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        return sharded_main(args, rank, world, dev)

    head = DeviceRun(args.config, n, dev)
    summary, _, _ = head.measure(args.steps, args.warmup, args.generic, per_kernel=False)
    outputs = dump_outputs(args.dump_outputs, {"edtsq": head.last_out}) if args.dump_outputs else None
    result = {
        "metric": "Mvox/s edt3dsq 512^3 uint32", "value": summary["mvox_per_s"], "unit": "Mvox/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": summary["ms_per_step"],
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": DTYPE, "data": "synthetic",
        "config": {"workload": f"{args.config}: {n}^3 uint32 labels, anisotropy {tuple(head.an)}, "
                               f"black_border={head.bb}, device-resident in/out",
                   "path": "generic" if args.generic else "default", "output_verified": None},
        "timing": head.timing,
    }
    if outputs is not None:
        result["outputs"] = {"dir": args.dump_outputs, "arrays": outputs,
                             "what": "edtsq: the (sz, sy, sx) float32 output of the last timed step, flattened"}
    # --full: everything beyond the headline figure -- the per-kernel steps and the roofline, the check of the timed output,
    # the numpy round trip, the secondary configurations and the CPU baseline (each verified against the CPU reference)
    if args.full:
        summary, kernels, bpv = head.kernel_times(head.ms, args.steps, args.generic)
        dom = max((k for k in kernels if k in bpv), key=lambda k: kernels[k])
        achieved = bpv[dom] * head.vox / (kernels[dom] * 1e-3) / 1e9
        # `achieved` / `frac`: the WHOLE JOB against SURVEY 8(d)'s 32 B/voxel -- the only fraction of this line that is bounded by 1
        # whatever the kernels do (VERDICT r5 "What's weak" 4: the dominant pass against its own 12 B/voxel model can read above 1,
        # because that pass moves fewer bytes than the model charges it -- those per-pass model figures live under `passes` only).
        roofline = {
            "bound": "hbm", "kernel": "whole step (x_pass + y_pass + z_bits + z_pass)", "dominant_kernel": dom,
            "achieved": summary["whole_job_algorithmic_GBs"], "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": summary["whole_job_frac"], "traffic": whole_step_traffic(args.config),
            "frac_note": "algorithmic bytes (SURVEY 8(d): 32 B/voxel, the reference's data movement) over the step's time, against the 8 TB/s "
                         "spec; the kernels really move ~18.4 B/voxel (traffic), so on a fast box this model fraction can pass 1 without "
                         "any kernel exceeding the memory system: real_* price the bytes that moved",
            "dominant_kernel_traffic": measured_traffic(dom, args.config), "dominant_kernel_model_GBs": round(achieved, 1),
            "kernel_ms": summary["kernel_ms"],
            # every pass against its own model (the `kernel` above is simply the longest one: X and Z are within 2 % of each other
            # on the headline, so which of them it is can change from run to run)
            "passes": {k: {"algorithmic_bytes_per_voxel": bpv[k], "ms": round(kernels[k], 4),
                           "model_GBs": round(bpv[k] * head.vox / (kernels[k] * 1e-3) / 1e9, 1),
                           "frac": round(bpv[k] * head.vox / (kernels[k] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)} for k in kernels if k in bpv},
            "whole_job_algorithmic_GBs": summary["whole_job_algorithmic_GBs"],
            "whole_job_frac": summary["whole_job_frac"],  # 32 B/voxel model over ms_per_step
        }
        # `frac` / `whole_job_frac` are the SURVEY 8(d) model (algorithmic bytes: the reference's data movement).  What the
        # kernels really move is less (labels are read once, 16-bit indices between X and Y): the real_* fields price that.
        roofline.update(real_traffic_fields(summary["ms_per_step"], kernels, dom, args.config))

        # sanity: the timed output is the right answer (closed form for the all-ones box)
        if args.config in ("cfg1", "cfg2"):
            from synth import box_edtsq_closed_form
            ok = bool(np.array_equal(head.out.cpu().numpy().T, box_edtsq_closed_form(head.lab_np.shape, head.an)))
        else:
            ok = None
        head_lab, head_an, head_bb = head.lab_np, head.an, head.bb
        # (kept on the host for the comparison with the compiled reference's output on the same volume, below)
        head_out = head.out.cpu().numpy().reshape(-1) if (not args.no_cpu_baseline and head_lab is not None) else None

        # numpy in -> numpy out through the host-buffer entry point (C ABI, PCIe both ways); reported beside the
        # device-resident figure, never as `value`
        end_to_end = None
        if head_lab is not None and not args.generic:
            try:
                end_to_end = host_round_trip(head_lab, head_an, head_bb)
            except Exception as e:  # pragma: no cover
                end_to_end = {"error": repr(e)}

        lib = kind = None
        if not args.no_cpu_baseline:
            try:
                lib, kind = reference_lib()
            except Exception as e:  # pragma: no cover
                lib, kind = None, f"unavailable: {e}"
        cores = os.cpu_count() or 1
        threads = (1, cores) if kind == "reference" else (1,)

        secondary = []
        cpu_secondary = {}
        if not args.no_secondary and args.config == "cfg2" and not args.generic:
            del head
            torch.cuda.empty_cache()
            what = {"cfg1": "all-ones labels (BASELINE configs[0]: the reference's own CPU-runnable case, timed beside it with parallel=1)",
                    "cfg3": "2000 labels (up-sampled x4: cells ~34 voxels)", "cfg3m": "2000 labels + 5 % zero membranes",
                    "cfg3f": "the 2000 labels of cfg3 at voxel sizes whose multiples are not exact in fp32",
                    "cfg3L": "~60 full-resolution Voronoi cells (~130 voxels across)", "cfg3La": "~60 full-resolution cells",
                    "cfg3M": "~500 full-resolution Voronoi cells (~65 voxels across)", "cfg3Ma": "~500 full-resolution cells",
                    "cfg4": "the 1024^3 segmentation of configs[3] (16 000 seeds) on ONE GPU"}
            # the OBJECT-SIZE sweep (tests/synth.py: SWEEP -- its cells ~65 / ~130 are cfg3M / cfg3L above)
            sweep = {"sw26": "~7600 full-resolution Voronoi cells (~26 voxels across)", "sw256": "8 full-resolution Voronoi cells (~256 voxels across)",
                     "sphere250": "ONE ball of radius 250 in background", "onesF": "all-ones box WITHOUT a black border (no boundary anywhere: +inf)",
                     "onebg": "all-ones box with ONE background voxel (every z-column sees one finite row)",
                     "diag": "two half spaces cut by the plane x + y + z = const", "diagF": "the same two half spaces without a black border",
                     "sphere_slab": "the ball of radius 250 on the 8-GPU slab shape"}
            what.update(sweep)
            # the headline's volume WITHOUT the short cut for tiles that have no structure along the scan axis (debug bit 0x80: every
            # tile through scans, break bits and blocks): a single-label box is made of nothing but such tiles, so the headline is
            # also stated as what the same kernels take when they do their whole work on it
            what["cfg2_scans"] = "the headline's volume with the flat-tile short cut switched off (debug bit 0x80)"
            todo = [("cfg2_scans", n), ("cfg1", n), ("cfg3", n), ("cfg3f", n), ("cfg3m", n), ("cfg3L", n), ("cfg3La", n), ("cfg3M", n), ("cfg3Ma", n), ("cfg4", 2 * n)]
            todo += [(k, n) for k in sweep]
            only = [c for c in args.secondary.split(",") if c]
            verify = os.environ.get("EDT_BENCH_VERIFY", "1") != "0"
            for name, size in todo:
                if only and name not in only:
                    continue
                try:
                    if name == "cfg2_scans":
                        from edt import _lib as _edt_lib
                        _edt_lib.load().edt_hip_set_debug_mode(0x80)
                    run = DeviceRun("cfg2" if name == "cfg2_scans" else name, size, dev)
                    s, kern, _ = run.measure(max(5, min(args.steps, 200) // 2) if size > n else min(args.steps, 100 if name in sweep else 400),
                                             args.warmup)
                    entry = {"config": name,
                             "workload": f"{'x'.join(str(v) for v in run.shape)} uint32 {'single-label' if name in ('cfg1', 'cfg2_scans') else 'multi-label'}: {what[name]}, "
                                         f"anisotropy {tuple(run.an)}, black_border={run.bb}, device-resident in/out, 1 GPU", **s}
                    entry.update(real_traffic_fields(s["ms_per_step"], kern, None, run.name))
                    entry["output_verified"] = None
                    if lib is not None and verify:
                        # the timed output, bit for bit against the CPU reference on the same volume (all threads), timed as well
                        # (configs[0] asks for the reference with parallel=1: both thread counts there)
                        res, want = time_reference(lib, kind, run.host_labels(), tuple(run.an), run.bb,
                                                   threads if name == "cfg1" else threads[-1:])
                        got = run.out.cpu().numpy().reshape(-1)
                        entry["output_verified"] = bool(np.array_equal(got, want))
                        cpu_secondary[name] = {f"{p} thread(s)": round(v, 1) for p, v in res.items()}
                        del got, want
                    secondary.append(entry)
                    del run
                    torch.cuda.empty_cache()
                except Exception as e:  # pragma: no cover  (a secondary must never take the headline down)
                    secondary.append({"config": name, "error": repr(e)})
                finally:
                    if name == "cfg2_scans":
                        _edt_lib.load().edt_hip_set_debug_mode(int(os.environ.get("EDT_HIP_DEBUG_MODE", "0"), 0))
            if not only or "cfg5" in only:
                try:
                    secondary.append(voxel_graph_secondary(n, dev, max(5, min(args.steps, 200) // 4), args.warmup,
                                                           lib if kind == "reference" else None))
                except Exception as e:  # pragma: no cover
                    secondary.append({"config": "cfg5", "error": repr(e)})
            if not only or "cfg5_sdf" in only:
                try:
                    secondary.append(sdf_secondary(n, dev, max(5, min(args.steps, 200) // 4), args.warmup,
                                                   lib if kind == "reference" else None))
                except Exception as e:  # pragma: no cover
                    secondary.append({"config": "cfg5_sdf", "error": repr(e)})
            if not only or "snemi_like" in only:
                try:
                    secondary.append(snemi_like_secondary(dev, lib, kind))
                except Exception as e:  # pragma: no cover
                    secondary.append({"config": "snemi_like", "error": repr(e)})

        result["config"]["output_verified"] = ok
        result["roofline"] = roofline
        if end_to_end is not None:
            result["end_to_end"] = end_to_end
        if secondary:
            result["secondary"] = secondary
        if not args.no_cpu_baseline:
            if lib is None:
                result["cpu_baseline"] = {"value": None, "unit": "Mvox/s", "cores": 0, "kind": str(kind), "sample": ""}
            else:
                m = min(n, 512)
                lab = head_lab if head_lab is not None and head_lab.shape[0] == m else np.ones((m, m, m), np.uint32, order="F")
                res, want = time_reference(lib, kind, lab, tuple(head_an), head_bb, threads)
                if head_out is not None and lab is head_lab and want is not None:
                    # the timed headline output, bit for bit against what the CPU reference just computed on the very same volume
                    same = bool(np.array_equal(head_out, np.asarray(want).reshape(-1)))
                    result["config"]["output_verified_against_reference"] = same
                    result["config"]["output_verified"] = bool(result["config"]["output_verified"] is not False and same)
                    result["config"]["verified_by"] = ("closed form of the box + " if ok is not None else "") + (
                        "the compiled CPU reference on the whole volume" if kind == "reference" else "the CPU restatement (oracle port)")
                del want
                top = max(res, key=lambda k: res[k])
                result["cpu_baseline"] = {
                    # cores: the physical cores the fastest figure ran on (all of them when every hardware thread was used);
                    # host_threads: the threads of that run
                    "value": round(res[top], 2), "unit": "Mvox/s",
                    "cores": (physical_cores() if int(top) >= physical_cores() else int(top)), "kind": kind,
                    "cpu": cpu_model(), "host_threads": int(top), "hardware_threads": cores,
                    "sample": f"whole {m}^3 uint32 headline volume ({args.config}), anisotropy {tuple(head_an)}, "
                              "1 warm-up + best of 3; "
                              + ", ".join(f"{p} thread(s): {v:.1f} Mvox/s" for p, v in res.items()),
                    "secondary": cpu_secondary,
                }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
