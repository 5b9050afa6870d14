// edt_moments.hip -- label_moments: per-label voxel count, exact raw first and second moments, centroid and population
// covariance, for every non-zero label at once, on device-resident data (include/edt_hip.h states the contract).
//
// This unit owns the sweep, MmEmit and the entry points.  The table (AccTable<10>: keys, the hash, the insertion, clear, add and
// flush), the walk over the flattened volume, the LDS claim and the finish are the table module's (edt_labeltable.h).  The ten
// sums of an x-run -- n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz -- have a closed form in the run's first voxel and its length
// (run_moments, edt_moments_math.h), so ONE lane per run posts all of them and nothing is scanned over lanes.  Every reduction
// is a 64-bit integer add: the table is the same bits on every run.
//
//   k_mm_sweep   one pass over the labels, nothing else is read.  A wave takes 4 x 64 consecutive voxels per step.  Run starts
//                (label change or start of an x-row) come from a neighbour compare and a ballot; the run's LAST lane knows
//                (x0, n, y, z) from the ballot alone and adds the run's ten sums to the workgroup's LDS table (kMmLdsSlots
//                slots of a key and ten u64, compare-and-swap on the key, 8 probes); a partial that finds no slot goes to the
//                global table directly.  A step that is one label inside one row is one partial of n = 256 from lane 0: no
//                ballot, no reduction.  Every workgroup owns a contiguous range of the volume and flushes its LDS table once.
//   MmEmit       writing an entry also derives centroid and covariance from its exact sums (moments_derive: 128-bit integers,
//                each value rounded once, by hand).
#include "edt_labeltable.h"
#include "edt_moments_math.h"

namespace edt_amd {
namespace {

constexpr int kMmLdsSlots = 256;   // 22.5 KiB of LDS per workgroup: 7 workgroups of 4 waves per compute unit
constexpr int kMmLdsProbes = 8;
constexpr int kMmBlocks = 256 * 7;

using MmTable = AccTable<kMmSums>;

struct MmOut : LabelOut {
  int64_t *counts, *sums;
  double *centroid, *central;
};

// ---- the sweep ------------------------------------------------------------------------------------------------------
// (7 waves per SIMD: as many workgroups as the LDS table admits have to fit the registers too -- 72 VGPRs)
template <typename T, bool BOOL>
__global__ __launch_bounds__(kLsThreads, 7) void k_mm_sweep(const T *__restrict__ labels, int64_t voxels, uint32_t sx, uint32_t sy,
                                                            int64_t tiles_per_block, MmTable t) {
  __shared__ u64 s_key[kMmLdsSlots], s_acc[kMmLdsSlots * kMmSums];
  for (int i = threadIdx.x; i < kMmLdsSlots; i += kLsThreads) s_key[i] = 0;
  for (int i = threadIdx.x; i < kMmLdsSlots * kMmSums; i += kLsThreads) s_acc[i] = 0;
  __syncthreads();

  // one run (x0 .. x0 + n - 1, y, z) of label k into the workgroup's table, or past it into the global one
  auto post = [&](u64 k, uint32_t x0, uint32_t n, uint32_t y, uint32_t z) {
    uint64_t m[kMmSums];
    run_moments(x0, n, y, z, m);
    const int slot = ls_lds_claim<kMmLdsSlots, kMmLdsProbes>(s_key, k);
    if (slot >= 0) {
#pragma unroll
      for (int j = 0; j < kMmSums; ++j) atomicAdd(&s_acc[slot * kMmSums + j], (u64)m[j]);
    } else {
      t.add(ls_find<true>(t, k), 0, m);
    }
  };

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const LsTiles bt = ls_block_tiles(voxels, tiles_per_block);
  int64_t tile = bt.t0 + wave;
  uint32_t bx, by, bz;  // coordinates of the wave's tile
  ls_tile_coords(tile, sx, sy, bx, by, bz);
  for (; tile < bt.t1; tile += kLsThreads / 64) {
    const int64_t base = tile * kLsTile + lane;
    u64 key[kLsGroups];
#pragma unroll
    for (int j = 0; j < kLsGroups; ++j) {
      const int64_t idx = base + j * 64;
      key[j] = idx < voxels ? ls_key<T, BOOL>(labels[idx]) : 0ull;
    }
    // the whole step one label inside one row (long runs, background): one partial of n = 256, nothing to reduce
    if (tile * kLsTile + kLsTile <= voxels && bx + (uint32_t)kLsTile <= sx) {
      const u64 k0 = __shfl(key[0], 0);
      if (__all(key[0] == k0 && key[1] == k0 && key[2] == k0 && key[3] == k0)) {
        if (k0 != 0 && lane == 0) post(k0, bx, (uint32_t)kLsTile, by, bz);
        ls_advance(sx, sy, bx, by, bz, (uint32_t)(kLsTile * (kLsThreads / 64)));
        continue;
      }
    }
    uint32_t x = bx, y = by, z = bz;
    ls_advance(sx, sy, x, y, z, (uint32_t)lane);
#pragma unroll
    for (int j = 0; j < kLsGroups; ++j) {
      const u64 k = key[j];
      const LsRun r = ls_run_bounds(k, lane, x == 0);
      if (r.end && k != 0)  // one partial per run: lanes r.s..lane of row (y, z)
        post(k, x - (uint32_t)(lane - r.s), (uint32_t)(lane - r.s + 1), y, z);
      ls_advance(sx, sy, x, y, z, 64u);
    }
    ls_advance(sx, sy, bx, by, bz, (uint32_t)(kLsTile * (kLsThreads / 64)));
  }
  __syncthreads();
  t.flush<kMmLdsSlots>(s_key, s_acc);
}

struct MmEmit {
  MmTable t;
  MmOut o;
  __device__ bool occupied(int64_t slot) const { return t.acc[slot * kMmSums + kMmN] != 0; }
  __device__ void operator()(int64_t slot, u64 key, int64_t rank) const {
    o.store_key(rank, key);
    uint64_t s[kMmSums];
#pragma unroll
    for (int k = 0; k < kMmSums; ++k) s[k] = t.acc[slot * kMmSums + k];
    double c[3], m[6];
    moments_derive(s, c, m);
    o.counts[rank] = (int64_t)s[kMmN];
#pragma unroll
    for (int k = 0; k < 9; ++k) o.sums[9 * rank + k] = (int64_t)s[kMmX + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o.centroid[3 * rank + k] = c[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) o.central[6 * rank + k] = m[k];
  }
};

template <typename T, bool BOOL>
int launch_mm_t(const T *labels, int64_t voxels, int64_t sx, int64_t sy, const MmEmit &e, hipStream_t stream) {
  if (const int rc = launch_acc_clear("label_moments clear", e.t, stream)) return rc;
  {
    ScopedPass sp("label_moments sweep", stream);
    const LsSweepGrid g = ls_sweep_grid(ceil_div(voxels, kLsTile), kMmBlocks);
    hipLaunchKernelGGL((k_mm_sweep<T, BOOL>), dim3(g.blocks), dim3(kLsThreads), 0, stream, labels, voxels, (uint32_t)sx, (uint32_t)sy,
                       g.per, e.t);
    EDT_HIP_TRY(hipGetLastError());
  }
  return launch_label_finish("label_moments finish", e, stream);
}

}  // namespace

// what both forms refuse after the shape: a bad max_labels, a volume past the range bound
int moments_check_args(int64_t sx, int64_t sy, int64_t sz, int64_t max_labels) {
  if (const int rc = label_table_check_args("label_moments", max_labels)) return rc;
  if (!moments_in_range(sx, sy, sz)) {
    set_error("label_moments: voxels * (largest extent - 1)^2 must stay below 2^63 (the second moments are exact int64)");
    return EDT_ERR_UNSUPPORTED;
  }
  return EDT_OK;
}

}  // namespace edt_amd

using namespace edt_amd;

extern "C" {

size_t edt_hip_label_moments_workspace_bytes(int dtype, int64_t voxels, int64_t max_labels) {
  if (!label_table_query_ok(dtype, voxels, max_labels)) return 0;
  return MmTable::carve(nullptr, dtype, ls_cap(voxels, max_labels)).bytes;
}

int edt_hip_label_moments_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz,
                                 int64_t max_labels, void *d_keys, int64_t *d_counts, int64_t *d_sums, double *d_centroid,
                                 double *d_central, int64_t *d_n_labels, void *d_scratch, size_t scratch_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int own = check_shape(dtype, ndim, sx, sy, sz);
  if (own == EDT_OK) own = moments_check_args(sx, sy, sz, max_labels);
  const int64_t voxels = own == EDT_OK ? sx * sy * sz : 0;
  int rc;
  if (!label_op_begin("label_moments", own, d_n_labels, 1, voxels,
                      !d_labels || !d_keys || !d_counts || !d_sums || !d_centroid || !d_central, false, d_scratch,
                      scratch_bytes, edt_hip_label_moments_workspace_bytes(dtype, voxels, max_labels),
                      "edt_hip_label_moments_workspace_bytes", stream, &rc))
    return rc;
  const MmEmit e = {MmTable::carve(d_scratch, dtype, ls_cap(voxels, max_labels)),
                    {label_out(d_keys, d_n_labels, dtype), d_counts, d_sums, d_centroid, d_central}};
  return with_label_key(dtype, [&](auto t, auto is_bool) -> int {
    using T = typename decltype(t)::type;
    return launch_mm_t<T, decltype(is_bool)::value>((const T *)d_labels, voxels, sx, sy, e, stream);
  });
}

}  // extern "C"
