"""The two phases of the Z-sharded path driven as VIRTUAL ranks on one device -- a helper of the GPU tests and of tools/, not a
test: every rank's XY phase on its Z-slab (the previous rank's last slice as its label halo), the exchange as a copy, every
destination's Z phase on its Y-slab, the result assembled to the whole (sz, sy, sx) volume.  torch.distributed does the same
across GPUs (edt/distributed.py); `ops` is its HipOps."""
import torch

from edt import _lib
from edt.distributed import balanced_partition


def flag_phases(ops, t, code, world, an, flags, sqrt=False):
    """The byte-flag form (ops.xy / ops.z): slabs, one-slice label halo, the Z-slab -> Y-slab re-partition done with plain
    tensor slicing.  t: the (sz, sy, sx) labels on the device, x fastest.  Returns the assembled volume."""
    sz, sy, sx = t.shape
    zparts, yparts = balanced_partition(sz, world), balanced_partition(sy, world)
    partial, zflags = [], []
    for r, (zs, ze) in enumerate(zparts):
        halo = t[zs - 1].contiguous() if r > 0 else None  # the previous rank's last slice
        p, f = ops.xy(t[zs:ze].contiguous(), halo, code, an, flags)
        partial.append(p)
        zflags.append(f)
    partial, zflags = torch.cat(partial, 0), torch.cat(zflags, 0)
    zf = flags | (_lib.FLAG_SQRT if sqrt else 0)
    # the all-to-all: rank h receives (all z, its y range)
    outs = [ops.z(partial[:, ys:ye, :].contiguous(), zflags[:, ys:ye, :].contiguous(), an[2], zf, wxy=(an[0], an[1])).clone()
            for ys, ye in yparts]
    return torch.cat(outs, 1)


def record_phases(ops, t, code, world, chunks, an, flags, sqrt=False, rows16=False, fill=None, wxy_every=1):
    """The slab-record forms (rows16: records of 16-bit rows, else of fp32 rows): every rank writes its per-destination records
    chunk by chunk -- its own part straight into the receive buffer --, the exchange is a copy of the other blocks, and each
    destination runs the Z phase over the gathered records.  fill: what the record words nobody wrote hold (default: NaN, or
    -1 in 16-bit records).  wxy_every: fp32 rows -- the Z phase of every wxy_every-th destination is told the voxel sizes of
    the XY phase (integer column kernel / fp32 fma candidates, edt_hip.h), the others are not (the fp32 kernels with fp64
    candidates): the same bits.
    Returns (the assembled volume, the refused-tile count); the count is None with fp32 rows, and where it is not 0 the 16-bit
    rows are unspecified: no Z phase is run and the volume is None (a driver repeats the step with fp32 rows)."""
    sz, sy, sx = t.shape
    dev = t.device
    words = -(-sy // 32)
    zparts = balanced_partition(sz, world)
    yparts = [(32 * a, min(32 * b, sy)) for a, b in balanced_partition(words, world)]
    y_splits = [a for a, _ in yparts] + [sy]
    rec = [(ops.record16_words if rows16 else ops.record_floats)(sx, b - a) for a, b in yparts]
    dtype = torch.int32 if rows16 else torch.float32
    if fill is None:
        fill = -1 if rows16 else float("nan")
    dst = [torch.full((sz, rec[h]), fill, dtype=dtype, device=dev) for h in range(world)]
    refused = torch.zeros(1, dtype=torch.int32, device=dev) if rows16 else None
    for r, (zs, ze) in enumerate(zparts):
        halo = t[zs - 1] if r > 0 else None  # the previous rank's last slice
        for c0, c1 in balanced_partition(ze - zs, min(chunks, ze - zs)):
            blocks = [dst[h][zs + c0:zs + c1] if h == r else torch.empty((c1 - c0, rec[h]), dtype=dtype, device=dev)
                      for h in range(world)]
            if rows16:
                ops.xy_records16(t[zs + c0:zs + c1], halo, code, an, flags, y_splits, blocks, refused)
            else:
                ops.xy_records(t[zs + c0:zs + c1], halo, code, an, flags, y_splits, blocks)
            for h in range(world):
                if h != r:
                    dst[h][zs + c0:zs + c1].copy_(blocks[h])  # the exchange
            halo = t[zs + c1 - 1]
    if rows16 and int(refused.item()) != 0:
        return None, int(refused.item())
    zf = flags | (_lib.FLAG_SQRT if sqrt else 0)
    outs = []
    for h, (ys, ye) in enumerate(yparts):
        if rows16:
            out = torch.full((sz, ye - ys, sx), float("nan"), dtype=torch.float32, device=dev)
            ops.z_records16(dst[h], out, an, zf)
        else:
            ops.z_records(dst[h], sx, ye - ys, an[2], zf, wxy=(an[0], an[1]) if h % wxy_every == 0 else None)
            out = dst[h][:, :(ye - ys) * sx].reshape(sz, ye - ys, sx)
        outs.append(out)
    return torch.cat(outs, 1), (0 if rows16 else None)
