"""Seeded slices of the randomised runs of the label operations (tools/fuzz_ops.py) inside the `-m gpu` tier: connected_components,
fill_holes, dust, label_stats, feature_transform and expand_labels through edt.device.* on device buffers at a random element
offset (every fifth case through the host module as well), against the numpy oracles of tests/, bit for bit.  The oracles
themselves are held against scipy and brute force on the same draws in the CPU tier (tests/test_fuzz_ops_cpu.py).  Every slice
is a fresh process: 60 cases, ten per operation.

A second family of slices, seeds 711..713, draws the field operations the same way: erode, opening, dilate, closing,
local_thickness (with its sizes) and medial_axis (with its radius on every second case), at voxel sizes that share a quantum and
radii that tie with the field on purpose.

A third family, seeds 721..723 and 64 cases each, draws voxel sizes the library finds no quantum for (tests/noquantum_cases.py):
feature_transform, expand_labels, dilate, closing and medial_axis on the fp64 kernels of csrc/edt_feature.hip, at sizes where
those are exact and the integer oracle holds bit for bit; erode, opening and local_thickness at those and at sizes whose squares
are not exact in fp32, against the compiled CPU transform."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (701, 702, 703)        # (tests/test_fuzz_ops_cpu.py draws the same)
FIELD_SEEDS = (711, 712, 713)  # (the same again)
NCASES = 60
OPS = ("connected_components", "fill_holes", "dust", "label_stats", "feature_transform", "expand_labels")
FIELD_OPS = ("erode", "opening", "dilate", "closing", "local_thickness", "medial_axis")
NOQUANTUM_SEEDS = (721, 722, 723)  # (and again)
NOQUANTUM_NCASES = 64
NOQUANTUM_OPS = ("feature_transform", "expand_labels", "dilate", "closing", "medial_axis", "erode", "opening", "local_thickness")


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_ops_slice(edt_gpu, seed):
    e = dict(os.environ)
    e.pop("EDT_HIP_DEBUG_MODE", None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_ops.py"), str(NCASES), str(seed)], cwd=ROOT, env=e,
                         capture_output=True, text=True, timeout=300)
    tail = (res.stdout + res.stderr)[-3000:]
    assert res.returncode == 0, tail
    assert "MISMATCH" not in res.stdout, tail
    lines = res.stdout.strip().splitlines()
    assert lines[-1].startswith(f"{NCASES} cases, 0 mismatches"), tail
    counts = dict(re.findall(r"(\w+)=(\d+)", next(line for line in lines if line.startswith("ops:"))))
    assert counts == {op: str(NCASES // len(OPS)) for op in OPS}, counts


@pytest.mark.parametrize("seed", FIELD_SEEDS)
def test_fuzz_field_ops_slice(edt_gpu, seed):
    e = dict(os.environ)
    e.pop("EDT_HIP_DEBUG_MODE", None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_ops.py"), str(NCASES), str(seed), "field"], cwd=ROOT,
                         env=e, capture_output=True, text=True, timeout=300)
    tail = (res.stdout + res.stderr)[-3000:]
    assert res.returncode == 0, tail
    assert "MISMATCH" not in res.stdout, tail
    lines = res.stdout.strip().splitlines()
    assert lines[-1].startswith(f"{NCASES} cases, 0 mismatches"), tail
    counts = dict(re.findall(r"(\w+)=(\d+)", next(line for line in lines if line.startswith("ops:"))))
    assert counts == {op: str(NCASES // len(FIELD_OPS)) for op in FIELD_OPS}, counts


@pytest.mark.parametrize("seed", NOQUANTUM_SEEDS)
def test_fuzz_noquantum_ops_slice(edt_gpu, seed):
    e = dict(os.environ)
    e.pop("EDT_HIP_DEBUG_MODE", None)
    n = NOQUANTUM_NCASES
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_ops.py"), str(n), str(seed), "noquantum"], cwd=ROOT,
                         env=e, capture_output=True, text=True, timeout=300)
    tail = (res.stdout + res.stderr)[-3000:]
    assert res.returncode == 0, tail
    assert "MISMATCH" not in res.stdout, tail
    lines = res.stdout.strip().splitlines()
    assert lines[-1].startswith(f"{n} cases, 0 mismatches"), tail
    counts = dict(re.findall(r"(\w+)=(\d+)", next(line for line in lines if line.startswith("ops:"))))
    assert counts == {op: str(n // len(NOQUANTUM_OPS)) for op in NOQUANTUM_OPS}, counts
