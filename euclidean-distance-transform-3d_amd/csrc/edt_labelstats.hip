// edt_labelstats.hip -- label_stats: per-label voxel count, maximum of a float field, its first argmax and the bounding box,
// for every non-zero label at once, on device-resident data (include/edt_hip.h states the contract).
//
// Every label type is reduced to a 64-bit KEY (edt_labeltable.h, shared with label_moments: keys, the hash, the insertion, the
// walk over the flattened volume, the sort key).  The float field is reduced through an order-preserving map to uint32
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
//   finish       8/16-bit labels (direct table: slot = key): one workgroup scans the occupancy and writes the entries in slot
//                order.  Wider labels (open-addressing table): the occupied slots are appended to a list, every entry's rank is
//                the number of smaller sort keys (keys are distinct: the order of the list does not matter), and the entry is
//                written at its rank.  O(n^2) in the number of labels, off the hot path.
// Global table: struct of arrays over `slots` (direct: 256 / 65536; hashed: a power of two >= 2 * max_labels).  Insertion is a
// compare-and-swap on the key word with linear probing; the probe loop is bounded by the table size and leaves early once
// the overflow word is set (more than max_labels distinct keys, or no free slot): no lane ever waits for another.
#include "edt_labeltable.h"

namespace edt_amd {
namespace {

constexpr int kLsLdsSlots = 512;           // 22 KiB of LDS per workgroup
constexpr int kLsLdsProbes = 8;
constexpr int kLsBlocks1 = 256 * 7;         // sweep 1: the workgroups 256 compute units hold at 22 KiB of LDS each
constexpr int kLsBlocks2 = 256 * 8;         // sweep 2
constexpr int kLsCacheSlots = 256;          // sweep 2: look-ups a workgroup remembers (5 KiB of LDS)
constexpr int kLsCacheProbes = 4;

struct LsTable {
  u64 *keys = nullptr, *counts = nullptr, *argidx = nullptr;
  uint32_t *maxord = nullptr;
  uint32_t *bbox = nullptr;  // 6 planes of `slots`: x0, x1, y0, y1, z0, z1
  u64 *ctrl = nullptr;       // [0] distinct keys inserted, [1] overflow, [2] entries of `list`
  u64 *list = nullptr;       // hashed: the occupied slots, in no particular order
  int64_t slots = 0, cap = 0;
  int direct = 0;
  size_t bytes = 0;
};

struct LsOut {
  void *keys;
  int64_t *counts;
  float *max;
  int64_t *argmax;
  int32_t *bbox;
  int64_t *n;
  int key_bytes;
  int key_kind;  // 0: integer, 1: binary32 bits, 2: binary64 bits
};

LsTable carve_ls(void *ws, int dtype, int64_t cap) {
  LsTable t;
  t.cap = cap;
  t.direct = dtype_size(dtype) <= 2;
  t.slots = ls_slots(dtype, cap);
  Carver c(ws);
  const size_t n = (size_t)t.slots;
  t.keys = c.take<u64>(n);
  t.counts = c.take<u64>(n);
  t.argidx = c.take<u64>(n);
  t.maxord = c.take<uint32_t>(n);
  t.bbox = c.take<uint32_t>(6 * n);
  t.ctrl = c.take<u64>(4);
  if (!t.direct) t.list = c.take<u64>((size_t)cap);
  t.bytes = align_up(c.off, 256);
  return t;
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
    int slot = -1;
    uint32_t h = (uint32_t)(ls_hash(k) >> 40) & (kLsLdsSlots - 1);
    for (int p = 0; p < kLsLdsProbes; ++p, h = (h + 1) & (kLsLdsSlots - 1)) {
      u64 cur = ((volatile u64 *)s_key)[h];
      if (cur == 0) cur = atomicCAS(&s_key[h], 0ull, k);
      if (cur == 0 || cur == k) {
        slot = (int)h;
        break;
      }
    }
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
  const int64_t ntiles = (voxels + kLsTile - 1) / kLsTile;
  const int64_t t0 = blockIdx.x * tiles_per_block;
  const int64_t t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;
  int64_t tile = t0 + wave;
  uint32_t bx, by, bz;  // coordinates of the wave's tile
  {
    const int64_t base = tile * kLsTile, r = base / sx;
    bx = (uint32_t)(base - r * sx);
    by = (uint32_t)(r % sy);
    bz = (uint32_t)(r / sy);
  }
  for (; tile < t1; tile += kLsThreads / 64) {
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
      const u64 pk = __shfl_up(k, 1);
      const bool start = lane == 0 || pk != k || x == 0;
      const uint64_t m = __ballot(start);
      const int s = 63 - __builtin_clzll(m & ((2ull << lane) - 1ull));  // first lane of this lane's run (bit 0 is always set)
      uint32_t v = od[j];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(v, off);
        if (lane - off >= s && u > v) v = u;
      }
      const bool end = lane == 63 || ((m >> (lane + 1)) & 1ull);
      if (end && k != 0)  // one partial per run: lanes s..lane of row (y, z)
        post(k, (u64)(lane - s + 1), v, x - (uint32_t)(lane - s), x, y, z);
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
  const int64_t ntiles = (voxels + kLsTile - 1) / kLsTile;
  const int64_t t0 = blockIdx.x * tiles_per_block;
  const int64_t t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;
  u64 ckey = 0;  // the wave's last look-up (uniform)
  int64_t cslot = -1;
  uint32_t cmax = 0;
  for (int64_t tile = t0 + wave; tile < t1; tile += kLsThreads / 64) {
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
      const u64 pk = __shfl_up(k, 1);
      const bool start = lane == 0 || pk != k;
      const uint64_t m = __ballot(start);
      const int s = 63 - __builtin_clzll(m & ((2ull << lane) - 1ull));
      int64_t slot = -1;
      uint32_t mx = 0;
      if (start && k != 0) {
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

// ---- finish ---------------------------------------------------------------------------------------------------------
__device__ void ls_emit(const LsTable &t, const LsOut &o, int64_t slot, u64 key, int64_t rank) {
  ls_store_key(o.keys, o.key_bytes, rank, key);
  o.counts[rank] = (int64_t)t.counts[slot];
  o.max[rank] = ord2f(t.maxord[slot]);
  o.argmax[rank] = (int64_t)t.argidx[slot];
  for (int k = 0; k < 6; ++k) o.bbox[6 * rank + k] = (int32_t)t.bbox[k * t.slots + slot];
}

// direct table: one workgroup; thread i owns a contiguous range of slots, so ranks follow the keys
__global__ __launch_bounds__(1024) void k_ls_finish_direct(LsTable t, LsOut o) {
  __shared__ uint32_t s_scan[1024];
  const int tid = threadIdx.x;
  const int64_t per = (t.slots + 1023) / 1024;
  const int64_t lo = tid * per < t.slots ? tid * per : t.slots;
  const int64_t hi = lo + per < t.slots ? lo + per : t.slots;
  uint32_t mine = 0;
  for (int64_t i = lo; i < hi; ++i) mine += t.counts[i] != 0;
  s_scan[tid] = mine;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const uint32_t add = tid >= off ? s_scan[tid - off] : 0u;
    __syncthreads();
    s_scan[tid] += add;
    __syncthreads();
  }
  int64_t rank = (int64_t)(s_scan[tid] - mine);
  if (tid == 1023) *o.n = (int64_t)s_scan[1023];
  for (int64_t i = lo; i < hi; ++i)
    if (t.counts[i] != 0) {
      if (rank < t.cap) ls_emit(t, o, i, (u64)i, rank);
      ++rank;
    }
}

__global__ __launch_bounds__(256) void k_ls_compact(LsTable t) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= t.slots || t.keys[i] == 0) return;
  const u64 pos = atomicAdd(&t.ctrl[2], 1ull);
  if (pos < (u64)t.cap) t.list[pos] = (u64)i;
}

// hashed table: the rank of an entry is the number of entries with a smaller sort key
__global__ __launch_bounds__(256) void k_ls_rank(LsTable t, LsOut o) {
  __shared__ u64 s_k[256];
  const int tid = threadIdx.x;
  const u64 n = t.ctrl[0];
  if (blockIdx.x == 0 && tid == 0) *o.n = (int64_t)n;
  if (t.ctrl[1] != 0 || n > (u64)t.cap || (u64)blockIdx.x * 256 >= n) return;  // (uniform) overflow: contents unspecified
  const u64 i = (u64)blockIdx.x * 256 + tid;
  int64_t slot = 0;
  u64 key = 0, mine = 0;
  if (i < n) {
    slot = (int64_t)t.list[i];
    key = t.keys[slot];
    mine = ls_sort_key(key, o.key_kind);
  }
  int64_t rank = 0;
  for (u64 j0 = 0; j0 < n; j0 += 256) {
    __syncthreads();
    if (j0 + tid < n) s_k[tid] = ls_sort_key(t.keys[t.list[j0 + tid]], o.key_kind);
    __syncthreads();
    const int cnt = n - j0 < 256 ? (int)(n - j0) : 256;
    for (int j = 0; j < cnt; ++j) rank += s_k[j] < mine;
  }
  if (i < n) ls_emit(t, o, slot, key, rank);
}

template <typename T, bool BOOL>
int launch_ls_t(const T *labels, const float *dt, int64_t voxels, int64_t sx, int64_t sy, const LsTable &t, const LsOut &o,
                hipStream_t stream) {
  {
    ScopedPass sp("label_stats clear", stream);
    hipLaunchKernelGGL(k_ls_clear, dim3((unsigned)ceil_div(std::max<int64_t>(t.slots, 4), 256)), dim3(256), 0, stream, t);
    EDT_HIP_TRY(hipGetLastError());
  }
  const int64_t ntiles = ceil_div(voxels, kLsTile);
  const int waves = kLsThreads / 64;
  {
    ScopedPass sp("label_stats sweep 1", stream);
    const int64_t blocks = std::min<int64_t>(ceil_div(ntiles, waves), kLsBlocks1);
    const int64_t per = ceil_div(ceil_div(ntiles, blocks), waves) * waves;  // (contiguous ranges: few labels per workgroup)
    hipLaunchKernelGGL((k_ls_sweep1<T, BOOL>), dim3((unsigned)ceil_div(ntiles, per)), dim3(kLsThreads), 0, stream, labels, dt,
                       voxels, (uint32_t)sx, (uint32_t)sy, per, t);
    EDT_HIP_TRY(hipGetLastError());
  }
  {
    ScopedPass sp("label_stats sweep 2", stream);
    const int64_t blocks = std::min<int64_t>(ceil_div(ntiles, waves), kLsBlocks2);
    const int64_t per = ceil_div(ceil_div(ntiles, blocks), waves) * waves;
    hipLaunchKernelGGL((k_ls_sweep2<T, BOOL>), dim3((unsigned)ceil_div(ntiles, per)), dim3(kLsThreads), 0, stream, labels, dt,
                       voxels, per, t);
    EDT_HIP_TRY(hipGetLastError());
  }
  {
    ScopedPass sp("label_stats finish", stream);
    if (t.direct) {
      hipLaunchKernelGGL(k_ls_finish_direct, dim3(1), dim3(1024), 0, stream, t, o);
    } else {
      hipLaunchKernelGGL(k_ls_compact, dim3((unsigned)ceil_div(t.slots, 256)), dim3(256), 0, stream, t);
      EDT_HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_ls_rank, dim3((unsigned)ceil_div(t.cap, 256)), dim3(256), 0, stream, t, o);
    }
    EDT_HIP_TRY(hipGetLastError());
  }
  return EDT_OK;
}

}  // namespace
}  // namespace edt_amd

using namespace edt_amd;

static int ls_check_args(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int64_t max_labels) {
  const int rc = check_shape(dtype, ndim, sx, sy, sz);
  if (rc != EDT_OK) return rc;
  if (max_labels < 1) { set_error("label_stats: max_labels must be at least 1"); return EDT_ERR_BAD_ARG; }
  // (the rank kernel runs one thread per entry: its grid has to fit 32 bits)
  if (max_labels > (int64_t(1) << 38)) { set_error("label_stats: max_labels beyond 2^38"); return EDT_ERR_BAD_ARG; }
  return EDT_OK;
}

extern "C" {

size_t edt_hip_label_stats_workspace_bytes(int dtype, int64_t voxels, int64_t max_labels) {
  if (dtype_size(dtype) == 0 || voxels < 0 || max_labels < 1 || max_labels > (int64_t(1) << 38)) return 0;
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
  const LsTable t = carve_ls(d_workspace, dtype, ls_cap(voxels, max_labels));
  const LsOut o = {d_keys, d_counts, d_max, d_argmax, d_bbox, d_n_labels, dtype_size(dtype),
                   ls_key_kind(dtype)};
  switch (dtype) {
    case EDT_U8: return launch_ls_t<uint8_t, false>((const uint8_t *)d_labels, d_dt, voxels, sx, sy, t, o, stream);
    case EDT_BOOL: return launch_ls_t<uint8_t, true>((const uint8_t *)d_labels, d_dt, voxels, sx, sy, t, o, stream);
    case EDT_U16: return launch_ls_t<uint16_t, false>((const uint16_t *)d_labels, d_dt, voxels, sx, sy, t, o, stream);
    case EDT_U32: return launch_ls_t<uint32_t, false>((const uint32_t *)d_labels, d_dt, voxels, sx, sy, t, o, stream);
    case EDT_U64: return launch_ls_t<uint64_t, false>((const uint64_t *)d_labels, d_dt, voxels, sx, sy, t, o, stream);
    case EDT_F32: return launch_ls_t<float, false>((const float *)d_labels, d_dt, voxels, sx, sy, t, o, stream);
    case EDT_F64: return launch_ls_t<double, false>((const double *)d_labels, d_dt, voxels, sx, sy, t, o, stream);
    default: set_error("unknown dtype"); return EDT_ERR_BAD_ARG;
  }
}

}  // extern "C"
