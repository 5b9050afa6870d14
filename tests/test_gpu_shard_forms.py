"""The three forms of the two sharded phases (csrc/edt_shard_api.hip: byte flags, slab records of fp32 rows, slab records of
16-bit rows) on ONE volume (`-m gpu`): the same bits from each, and the oracle's; and the passes the one XY record phase and the
one Z record phase log, for both record forms.

(36, 100, 97) are the smallest extents at which the phases can still go wrong: 36 columns are one full 32-column tile and a
partial one of 4, rows of whole 8-byte granules; 100 rows are four y-bands, the last one partial -- the least the integer kernel
takes -- cut into destinations of 64, 32 and 4 rows; 97 slices are four z-bands, the last one of a single row.  Three virtual
ranks with two chunks each: slabs of 33, 32 and 32 slices, uneven chunks."""
import numpy as np
import pytest

from synth import voronoi_labels

pytestmark = pytest.mark.gpu

SHAPE = (36, 100, 97)
WORLD, CHUNKS = 3, 2


def _pass_names():
    from edt import device
    return [name for name, _ in device.pass_times()]


def test_three_forms_of_the_sharded_phases_on_one_volume(edt_gpu, oracle_port):
    import torch
    from edt import _lib, device
    from edt.distributed import HipOps
    from virtual_ranks import flag_phases, record_phases

    sx, sy, sz = SHAPE
    dev = torch.device("cuda", 0)
    ops = HipOps()
    lab = voronoi_labels(SHAPE, nseeds=30, seed=36100097, upsample=4, membrane=0.04)
    assert lab.dtype == np.uint32
    t = torch.from_numpy(np.ascontiguousarray(lab.T).view(np.int32)).to(dev)  # (sz, sy, sx), x fastest
    assert ops.records_supported(_lib.U32, sx, sy, sz)
    for an, bb in (((6.0, 6.0, 30.0), True), ((1.0, 1.0, 1.0), False)):
        assert ops.lib.edt_hip_shard_records16_supported(_lib.U32, sx, sy, sz, *an) == 1
        flags = _lib.FLAG_BLACK_BORDER if bb else 0
        want = oracle_port.edtsq(lab, an, bb)
        by_flags = flag_phases(ops, t, _lib.U32, WORLD, an, flags).cpu().numpy().T
        by_fp32, _ = record_phases(ops, t, _lib.U32, WORLD, CHUNKS, an, flags)
        by_fp32 = by_fp32.cpu().numpy().T
        by_16, refused = record_phases(ops, t, _lib.U32, WORLD, CHUNKS, an, flags, rows16=True)
        assert np.array_equal(by_flags, want), (an, bb, "byte flags")
        assert np.array_equal(by_fp32, want), (an, bb, "records of fp32 rows")
        if bb:
            assert refused == 0   # (every row has a boundary, no value leaves 16 bits)
        if refused == 0:          # (else the 16-bit rows are unspecified: a driver repeats the step with fp32 rows)
            assert np.array_equal(by_16.cpu().numpy().T, want), (an, bb, "records of 16-bit rows")

    # the passes of one XY record phase and of one Z record phase, whichever record form: a slab of one rank
    an, flags = (6.0, 6.0, 30.0), _lib.FLAG_BLACK_BORDER
    device.set_profiling(True)   # (a fresh log)
    try:
        for rows16 in (False, True):
            words = ops.record16_words(sx, sy) if rows16 else ops.record_floats(sx, sy)
            records = torch.empty((sz, words), dtype=torch.int32 if rows16 else torch.float32, device=dev)
            if rows16:
                refused = torch.zeros(1, dtype=torch.int32, device=dev)
                ops.xy_records16(t, None, _lib.U32, an, flags, [0, sy], [records], refused)
            else:
                ops.xy_records(t, None, _lib.U32, an, flags, [0, sy], [records])
            torch.cuda.current_stream().synchronize()
            assert _pass_names()[-3:] == ["x_pass", "pack_bits", "y_pass"], (rows16, _pass_names())
            if rows16:
                ops.z_records16(records, torch.empty((sz, sy, sx), dtype=torch.float32, device=dev), an, flags)
            else:
                ops.z_records(records, sx, sy, an[2], flags, wxy=an[:2])
            torch.cuda.current_stream().synchronize()
            assert _pass_names()[-2:] == ["z_bits", "z_pass"], (rows16, _pass_names())
    finally:
        device.set_profiling(False)
