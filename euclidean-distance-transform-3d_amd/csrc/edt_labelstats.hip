// edt_labelstats.hip -- label_stats: per-label voxel count, maximum of a float field, its first argmax and the bounding box,
// for every non-zero label at once, on device-resident data (include/edt_hip.h states the contract).
//
// This unit owns its payload (count, maximum, argmax index, bounding box: min / max reductions, so its own clear and flush), the
// two sweeps, LsEmit and the entry points.  Keys, the hash, the insertion, the walk over the flattened volume, the LDS claim and
// the finish are the table module's (edt_labeltable.h).  The float field is reduced through an order-preserving map to uint32
// (f2ord), so that every reduction is an integer min / max / add: the table does not depend on which thread arrived first.
//
//   k_ls_clear   the global table (clear-on-use: a reused workspace needs no memset)
//   k_ls_sweep1  count, max, bbox.  A wave takes 4 x 64 consecutive voxels per step, one voxel per lane and group.  Run starts
//                (label change or start of an x-row) come from a neighbour compare and a ballot; a segmented max-scan leaves the
//                run's maximum in its LAST lane, which also knows the run's length and x-range from the ballot alone.  That lane
//                adds the partial to the workgroup's LDS table (512 slots, compare-and-swap on the key, 8 probes); a partial that
//                finds no slot goes to the global table directly.  Every workgroup owns a contiguous range of the volume (few
//                labels per workgroup) and flushes its LDS table once: one set of global atomics per (workgroup, label).
//                A step that is one label inside one row (long runs, background) is one wave reduction and one partial.
//   k_ls_sweep2  argmax, form (a) of the issue: each run looks up its label's final maximum; the first lane of the run whose
//                value equals it does a 64-bit atomic min on the label's index -- after a plain read that drops the atomic when
//                the stored index is already smaller (the stored value only ever decreases, so a stale read only costs a
//                redundant atomic).  Look-ups go through the wave's last one, then a 256-entry LDS cache of the workgroup,
//                then the global table; a step that is one label throughout needs one look-up and one ballot per group.
#include "edt_labeltable.h"

namespace edt_amd {
namespace {

constexpr int kLsLdsSlots = 512;           // 22 KiB of LDS per workgroup
constexpr int kLsLdsProbes = 8;
constexpr int kLsBlocks1 = 256 * 7;         // sweep 1: the workgroups 256 compute units hold at 22 KiB of LDS each
constexpr int kLsBlocks2 = 256 * 8;         // sweep 2
constexpr int kLsCacheSlots = 256;          // sweep 2: look-ups a workgroup remembers (5 KiB of LDS)
constexpr int kLsCacheProbes = 4;

struct LsTable : LabelTable {
  u64 *counts = nullptr, *argidx = nullptr;
  uint32_t *maxord = nullptr;
  uint32_t *bbox = nullptr;  // 6 planes of `slots`: x0, x1, y0, y1, z0, z1
};

struct LsOut : LabelOut {
  int64_t *counts;
  float *max;
  int64_t *argmax;
  int32_t *bbox;
};

LsTable carve_ls(void *ws, int dtype, int64_t cap) {
  return carve_label_table<LsTable>(ws, dtype, cap, [](LsTable &t, Carver &c, size_t n) {
    t.counts = c.take<u64>(n);
    t.argidx = c.take<u64>(n);
    t.maxord = c.take<uint32_t>(n);
    t.bbox = c.take<uint32_t>(6 * n);
  });
}

// monotone updates: a plain read first, the atomic only when it may change the word (a stale read costs one redundant atomic)
__device__ __forceinline__ void ls_min(uint32_t *p, uint32_t v) { if (ls_peek(p) > v) atomicMin(p, v); }
__device__ __forceinline__ void ls_max(uint32_t *p, uint32_t v) { if (ls_peek(p) < v) atomicMax(p, v); }

__device__ void ls_global_add(const LsTable &t, u64 key, u64 count, uint32_t ord, uint32_t x0, uint32_t x1, uint32_t y0,
                              uint32_t y1, uint32_t z0, uint32_t z1) {
  const int64_t s = ls_find<true>(t, key);
  if (s < 0) return;
  atomicAdd(&t.counts[s], count);
  ls_max(&t.maxord[s], ord);
  ls_min(&t.bbox[s], x0);
  ls_max(&t.bbox[t.slots + s], x1);
  ls_min(&t.bbox[2 * t.slots + s], y0);
  ls_max(&t.bbox[3 * t.slots + s], y1);
  ls_min(&t.bbox[4 * t.slots + s], z0);
  ls_max(&t.bbox[5 * t.slots + s], z1);
}

__global__ __launch_bounds__(256) void k_ls_clear(LsTable t) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < 4) t.ctrl[i] = 0;
  if (i >= t.slots) return;
  t.keys[i] = 0;
  t.counts[i] = 0;
  t.argidx[i] = ~0ull;
  t.maxord[i] = 0;
  for (int k = 0; k < 6; ++k) t.bbox[k * t.slots + i] = (k & 1) ? 0u : 0xFFFFFFFFu;
}

// ---- sweep 1: count, max, bbox --------------------------------------------------------------------------------------
template <typename T, bool BOOL>
__global__ __launch_bounds__(kLsThreads) void k_ls_sweep1(const T *__restrict__ labels, const float *__restrict__ dt,
                                                          int64_t voxels, uint32_t sx, uint32_t sy, int64_t tiles_per_block,
                                                          LsTable t) {
  __shared__ u64 s_key[kLsLdsSlots], s_cnt[kLsLdsSlots];
  __shared__ uint32_t s_max[kLsLdsSlots], s_box[6][kLsLdsSlots];
  for (int i = threadIdx.x; i < kLsLdsSlots; i += kLsThreads) {
    s_key[i] = 0;
    s_cnt[i] = 0;
    s_max[i] = 0;
    for (int k = 0; k < 6; ++k) s_box[k][i] = (k & 1) ? 0u : 0xFFFFFFFFu;
  }
  __syncthreads();

  // one partial (a run, or a whole step of one label) into the workgroup's table, or past it into the global one
  auto post = [&](u64 k, u64 cnt, uint32_t v, uint32_t x0, uint32_t x1, uint32_t y, uint32_t z) {
    const int slot = ls_lds_claim<kLsLdsSlots, kLsLdsProbes>(s_key, k);
    if (slot >= 0) {
      atomicAdd(&s_cnt[slot], cnt);
      atomicMax(&s_max[slot], v);
      atomicMin(&s_box[0][slot], x0);
      atomicMax(&s_box[1][slot], x1);
      atomicMin(&s_box[2][slot], y);
      atomicMax(&s_box[3][slot], y);
      atomicMin(&s_box[4][slot], z);
      atomicMax(&s_box[5][slot], z);
    } else {
      ls_global_add(t, k, cnt, v, x0, x1, y, y, z, z);
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
    uint32_t od[kLsGroups];
#pragma unroll
    for (int j = 0; j < kLsGroups; ++j) {
      const int64_t idx = base + j * 64;
      key[j] = 0;
      od[j] = 0;
      if (idx < voxels) {
        key[j] = ls_key<T, BOOL>(labels[idx]);
        od[j] = f2ord(dt[idx]);
      }
    }
    // the whole step one label inside one row (long runs, background): one partial, no scan
    if (tile * kLsTile + kLsTile <= voxels && bx + (uint32_t)kLsTile <= sx) {
      const u64 k0 = __shfl(key[0], 0);
      if (__all(key[0] == k0 && key[1] == k0 && key[2] == k0 && key[3] == k0)) {
        if (k0 != 0) {
          uint32_t v = od[0];
          for (int j = 1; j < kLsGroups; ++j) v = od[j] > v ? od[j] : v;
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) {
            const uint32_t u = __shfl_xor(v, off);
            v = u > v ? u : v;
          }
          if (lane == 0) post(k0, (u64)kLsTile, v, bx, bx + (uint32_t)kLsTile - 1, by, bz);
        }
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
      uint32_t v = od[j];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(v, off);
        if (lane - off >= r.s && u > v) v = u;
      }
      if (r.end && k != 0)  // one partial per run: lanes r.s..lane of row (y, z)
        post(k, (u64)(lane - r.s + 1), v, x - (uint32_t)(lane - r.s), x, y, z);
      ls_advance(sx, sy, x, y, z, 64u);
    }
    ls_advance(sx, sy, bx, by, bz, (uint32_t)(kLsTile * (kLsThreads / 64)));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kLsLdsSlots; i += kLsThreads)
    if (s_key[i] != 0)
      ls_global_add(t, s_key[i], s_cnt[i], s_max[i], s_box[0][i], s_box[1][i], s_box[2][i], s_box[3][i], s_box[4][i],
                    s_box[5][i]);
}

// ---- sweep 2: the smallest index at which a label's field equals its maximum ----------------------------------------
template <typename T, bool BOOL>
__global__ __launch_bounds__(kLsThreads) void k_ls_sweep2(const T *__restrict__ labels, const float *__restrict__ dt,
                                                          int64_t voxels, int64_t tiles_per_block, LsTable t) {
  // look-ups of this workgroup: key -> (slot, maximum).  An entry is claimed by a compare-and-swap on its key and valid once
  // its slot word is written (last); a reader that finds it unfinished looks the key up itself.
  __shared__ u64 c_key[kLsCacheSlots], c_slot[kLsCacheSlots];
  __shared__ uint32_t c_max[kLsCacheSlots];
  for (int i = threadIdx.x; i < kLsCacheSlots; i += kLsThreads) {
    c_key[i] = 0;
    c_slot[i] = ~0ull;
  }
  __syncthreads();
  auto lookup = [&](u64 k, int64_t &slot, uint32_t &mx) {
    const uint32_t h0 = (uint32_t)(ls_hash(k) >> 40) & (kLsCacheSlots - 1);
    uint32_t h = h0;
    for (int p = 0; p < kLsCacheProbes; ++p, h = (h + 1) & (kLsCacheSlots - 1)) {
      const u64 cur = ((volatile u64 *)c_key)[h];
      if (cur == 0) break;
      if (cur == k) {
        const u64 sl = ((volatile u64 *)c_slot)[h];
        if (sl != ~0ull) {
          slot = (int64_t)sl;
          mx = ((volatile uint32_t *)c_max)[h];
          return;
        }
        break;
      }
    }
    slot = ls_find<false>(t, k);
    mx = slot >= 0 ? ls_peek(&t.maxord[slot]) : 0u;
    if (slot < 0) return;
    h = h0;
    for (int p = 0; p < kLsCacheProbes; ++p, h = (h + 1) & (kLsCacheSlots - 1)) {
      const u64 cur = atomicCAS(&c_key[h], 0ull, k);
      if (cur == k) return;  // (another lane is writing it)
      if (cur == 0) {
        ((volatile uint32_t *)c_max)[h] = mx;
        __threadfence_block();
        ((volatile u64 *)c_slot)[h] = (u64)slot;
        return;
      }
    }
  };
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const LsTiles bt = ls_block_tiles(voxels, tiles_per_block);
  u64 ckey = 0;  // the wave's last look-up (uniform)
  int64_t cslot = -1;
  uint32_t cmax = 0;
  for (int64_t tile = bt.t0 + wave; tile < bt.t1; tile += kLsThreads / 64) {
    const int64_t base = tile * kLsTile + lane;
    u64 key[kLsGroups];
    uint32_t od[kLsGroups];
#pragma unroll
    for (int j = 0; j < kLsGroups; ++j) {
      const int64_t idx = base + j * 64;
      key[j] = 0;
      od[j] = 0;
      if (idx < voxels) {
        key[j] = ls_key<T, BOOL>(labels[idx]);
        od[j] = f2ord(dt[idx]);
      }
    }
    {  // the whole step one label: one look-up, the first lane that holds the maximum
      const u64 k0 = __shfl(key[0], 0);
      if (__all(key[0] == k0 && key[1] == k0 && key[2] == k0 && key[3] == k0)) {
        if (k0 == 0) continue;
        if (k0 != ckey) {
          int64_t slot = -1;
          uint32_t mx = 0;
          if (lane == 0) lookup(k0, slot, mx);
          ckey = k0;
          cslot = __shfl(slot, 0);
          cmax = __shfl(mx, 0);
        }
        if (cslot < 0) continue;
        for (int j = 0; j < kLsGroups; ++j) {
          const uint64_t em = __ballot(od[j] == cmax && base + j * 64 < voxels);
          if (em) {
            if (lane == __builtin_ctzll(em)) {
              const u64 idx = (u64)(base + j * 64);
              if (ls_peek(&t.argidx[cslot]) > idx) atomicMin(&t.argidx[cslot], idx);
            }
            break;
          }
        }
        continue;
      }
    }
#pragma unroll
    for (int j = 0; j < kLsGroups; ++j) {
      const u64 k = key[j];
      const LsRun r = ls_run_bounds(k, lane, false);  // (the index is flat: a run goes on across the start of an x-row)
      const int s = r.s;
      int64_t slot = -1;
      uint32_t mx = 0;
      if (r.start && k != 0) {
        if (k == ckey) {
          slot = cslot;
          mx = cmax;
        } else {
          lookup(k, slot, mx);
        }
      }
      slot = __shfl(slot, s);
      mx = __shfl(mx, s);
      const bool eq = k != 0 && slot >= 0 && od[j] == mx;
      const uint64_t em = __ballot(eq);
      const uint64_t before = em & ~((1ull << s) - 1ull) & ((1ull << lane) - 1ull);  // equal lanes of my run below me
      if (eq && before == 0) {
        const u64 idx = (u64)(base + j * 64);
        if (ls_peek(&t.argidx[slot]) > idx) atomicMin(&t.argidx[slot], idx);
      }
      ckey = __shfl(k, 63);
      cslot = __shfl(slot, 63);
      cmax = __shfl(mx, 63);
    }
  }
}

struct LsEmit {
  LsTable t;
  LsOut o;
  __device__ bool occupied(int64_t slot) const { return t.counts[slot] != 0; }
  __device__ void operator()(int64_t slot, u64 key, int64_t rank) const {
    o.store_key(rank, key);
    o.counts[rank] = (int64_t)t.counts[slot];
    o.max[rank] = ord2f(t.maxord[slot]);
    o.argmax[rank] = (int64_t)t.argidx[slot];
    for (int k = 0; k < 6; ++k) o.bbox[6 * rank + k] = (int32_t)t.bbox[k * t.slots + slot];
  }
};

template <typename T, bool BOOL>
int launch_ls_t(const T *labels, const float *dt, int64_t voxels, int64_t sx, int64_t sy, const LsEmit &e, hipStream_t stream) {
  {
    ScopedPass sp("label_stats clear", stream);
    hipLaunchKernelGGL(k_ls_clear, dim3(label_clear_blocks(e.t)), dim3(256), 0, stream, e.t);
    EDT_HIP_TRY(hipGetLastError());
  }
  const int64_t ntiles = ceil_div(voxels, kLsTile);
  {
    ScopedPass sp("label_stats sweep 1", stream);
    const LsSweepGrid g = ls_sweep_grid(ntiles, kLsBlocks1);
    hipLaunchKernelGGL((k_ls_sweep1<T, BOOL>), dim3(g.blocks), dim3(kLsThreads), 0, stream, labels, dt, voxels, (uint32_t)sx,
                       (uint32_t)sy, g.per, e.t);
    EDT_HIP_TRY(hipGetLastError());
  }
  {
    ScopedPass sp("label_stats sweep 2", stream);
    const LsSweepGrid g = ls_sweep_grid(ntiles, kLsBlocks2);
    hipLaunchKernelGGL((k_ls_sweep2<T, BOOL>), dim3(g.blocks), dim3(kLsThreads), 0, stream, labels, dt, voxels, g.per, e.t);
    EDT_HIP_TRY(hipGetLastError());
  }
  return launch_label_finish("label_stats finish", e, stream);
}

}  // namespace
}  // namespace edt_amd

using namespace edt_amd;

static int ls_check_args(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int64_t max_labels) {
  const int rc = check_shape(dtype, ndim, sx, sy, sz);
  if (rc != EDT_OK) return rc;
  return label_table_check_args("label_stats", max_labels);
}

extern "C" {

size_t edt_hip_label_stats_workspace_bytes(int dtype, int64_t voxels, int64_t max_labels) {
  if (!label_table_query_ok(dtype, voxels, max_labels)) return 0;
  return carve_ls(nullptr, dtype, ls_cap(voxels, max_labels)).bytes;
}

int edt_hip_label_stats_device(const void *d_labels, int dtype, const float *d_dt, int ndim, int64_t sx, int64_t sy,
                               int64_t sz, int64_t max_labels, void *d_keys, int64_t *d_counts, float *d_max,
                               int64_t *d_argmax, int32_t *d_bbox, int64_t *d_n_labels, void *d_workspace,
                               size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int own = ls_check_args(dtype, ndim, sx, sy, sz, max_labels);
  const int64_t voxels = own == EDT_OK ? sx * sy * sz : 0;
  int rc;
  if (!label_op_begin("label_stats", own, d_n_labels, 1, voxels,
                      !d_labels || !d_dt || !d_keys || !d_counts || !d_max || !d_argmax || !d_bbox, false, d_workspace,
                      workspace_bytes, edt_hip_label_stats_workspace_bytes(dtype, voxels, max_labels),
                      "edt_hip_label_stats_workspace_bytes", stream, &rc))
    return rc;
  const LsEmit e = {carve_ls(d_workspace, dtype, ls_cap(voxels, max_labels)),
                    {label_out(d_keys, d_n_labels, dtype), d_counts, d_max, d_argmax, d_bbox}};
  return with_label_key(dtype, [&](auto t, auto is_bool) -> int {
    using T = typename decltype(t)::type;
    return launch_ls_t<T, decltype(is_bool)::value>((const T *)d_labels, d_dt, voxels, sx, sy, e, stream);
  });
}

}  // extern "C"
