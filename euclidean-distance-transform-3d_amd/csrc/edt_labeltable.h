// edt_labeltable.h -- the per-label table module: everything label_stats (edt_labelstats.hip), label_moments (edt_moments.hip)
// and label_topology (edt_topology.hip) share.  Header-only and internal: every unit instantiates its own kernels.
//
// Owned here: the 64-bit KEY of every label type and the dispatch over the types (with_label_key); the hash; LabelTable, the
// global table's keys / ctrl / list and its carving; the insertion by compare-and-swap (ls_find); AccTable<SUMS>, a table of
// SUMS u64 words per slot that are only ever added to (carve, clear kernel, add, the flush of a workgroup's LDS table); the claim
// of an LDS slot (ls_lds_claim); the walk over the flattened volume in 4 x 64 voxel steps (ls_sweep_grid, ls_block_tiles,
// ls_tile_coords, ls_run_bounds, ls_advance); the finish, which writes the entries in key order (k_label_finish_direct, or
// k_label_compact + k_label_rank: launch_label_finish); the max_labels checks of the entry points.
// Owned by the units: the payload of a slot and what a sweep adds to it, and an Emit -- {table t, outputs o, occupied(slot),
// operator()(slot, key, rank)} -- that writes one entry.
//
// KEY: the value itself for integers, 1 for any non-zero bool byte, the bit pattern for floats with -0.0 folded into 0 and NaN
// mapped to 0 (a NaN voxel belongs to no label).  Key 0 is background and the empty-slot marker.
// Global table: struct of arrays over `slots` (direct, 8- / 16-bit labels: 256 / 65536 and slot = key; hashed: a power of two
// >= 2 * max_labels).  Insertion is a compare-and-swap on the key word with linear probing; the probe loop is bounded by the
// table size and leaves early once the overflow word is set (more than max_labels distinct keys, or no free slot): no lane ever
// waits for another.  Finish: a direct table is scanned in slot order by one workgroup.  Of a hashed one the occupied slots are
// appended to a list, every entry's rank is the number of smaller sort keys (keys are distinct: the order of the list does not
// matter), and the entry is written at its rank.  O(n^2) in the number of labels, off the hot path.
#pragma once

#include <type_traits>

#include "edt_api_internal.h"

namespace edt_amd {
namespace {

typedef unsigned long long u64;

constexpr int kLsThreads = 256;            // 4 waves
constexpr int kLsGroups = 4;               // 64-voxel groups per wave and step
constexpr int kLsTile = 64 * kLsGroups;    // voxels per wave and step
constexpr int64_t kLsMinSlots = 1024;

// at most `voxels` labels exist: a larger max_labels buys nothing
inline int64_t ls_cap(int64_t voxels, int64_t max_labels) { return std::min(max_labels, std::max<int64_t>(voxels, 1)); }

// direct: 256 / 65536; hashed: a power of two >= 2 * cap
inline int64_t ls_slots(int dtype, int64_t cap) {
  if (dtype_size(dtype) <= 2) return dtype_size(dtype) == 1 ? 256 : 65536;
  int64_t slots = kLsMinSlots;
  while (slots < 2 * cap) slots *= 2;
  return slots;
}

// What every table has.  The payload of a slot lies between `keys` and `ctrl` in the workspace.
struct LabelTable {
  u64 *keys = nullptr;   // hashed: the key of a slot (direct: slot = key)
  u64 *ctrl = nullptr;   // [0] distinct keys inserted, [1] overflow, [2] entries of `list`
  u64 *list = nullptr;   // hashed: the occupied slots, in no particular order
  int64_t slots = 0, cap = 0;
  int direct = 0;
  size_t bytes = 0;
};

// payload(t, carver, slots): the unit's own arrays
template <typename Table, typename Payload>
Table carve_label_table(void *ws, int dtype, int64_t cap, Payload payload) {
  Table t;
  t.cap = cap;
  t.direct = dtype_size(dtype) <= 2;
  t.slots = ls_slots(dtype, cap);
  Carver c(ws);
  t.keys = c.take<u64>((size_t)t.slots);
  payload(t, c, (size_t)t.slots);
  t.ctrl = c.take<u64>(4);
  if (!t.direct) t.list = c.take<u64>((size_t)cap);
  t.bytes = align_up(c.off, 256);
  return t;
}

// What the entry points refuse after the shape, with the call's name in front.
inline int label_table_check_args(const char *who, int64_t max_labels) {
  if (max_labels < 1) { set_error(std::string(who) + ": max_labels must be at least 1"); return EDT_ERR_BAD_ARG; }
  // (the rank kernel runs one thread per entry: its grid has to fit 32 bits)
  if (max_labels > (int64_t(1) << 38)) { set_error(std::string(who) + ": max_labels beyond 2^38"); return EDT_ERR_BAD_ARG; }
  return EDT_OK;
}
// ... and what makes a *_workspace_bytes query answer 0
inline bool label_table_query_ok(int dtype, int64_t voxels, int64_t max_labels) {
  return dtype_size(dtype) != 0 && voxels >= 0 && max_labels >= 1 && max_labels <= (int64_t(1) << 38);
}

// The label type of a dtype code and whether it is read as bool, handed to `f` as tags: f(LabelType<T>{}, std::bool_constant<BOOL>{})
// -> int.  (with_label_type, edt_common.h, reads EDT_BOOL like EDT_U8; a key does not.)
template <typename F>
inline int with_label_key(int dtype, F &&f) {
  switch (dtype) {
    case EDT_U8: return f(LabelType<uint8_t>{}, std::false_type{});
    case EDT_BOOL: return f(LabelType<uint8_t>{}, std::true_type{});
    case EDT_U16: return f(LabelType<uint16_t>{}, std::false_type{});
    case EDT_U32: return f(LabelType<uint32_t>{}, std::false_type{});
    case EDT_U64: return f(LabelType<uint64_t>{}, std::false_type{});
    case EDT_F32: return f(LabelType<float>{}, std::false_type{});
    case EDT_F64: return f(LabelType<double>{}, std::false_type{});
    default: set_error("unknown dtype"); return EDT_ERR_BAD_ARG;
  }
}

// ---- keys and the ordered float map ---------------------------------------------------------------------------------
template <typename T, bool BOOL> __device__ __forceinline__ u64 ls_key(T v) { return BOOL ? (u64)(v != 0) : (u64)v; }
template <> __device__ __forceinline__ u64 ls_key<float, false>(float v) {
  return (v == v && v != 0.0f) ? (u64)__float_as_uint(v) : 0ull;
}
template <> __device__ __forceinline__ u64 ls_key<double, false>(double v) {
  return (v == v && v != 0.0) ? (u64)__double_as_longlong(v) : 0ull;
}

// a < b  <=>  f2ord(a) < f2ord(b) for all non-NaN floats (-0.0 sorts just below +0.0); every non-NaN value maps above 0
__device__ __forceinline__ uint32_t f2ord(float f) {
  const uint32_t b = __float_as_uint(f);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) { return __uint_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
__device__ __forceinline__ u64 d2ord(u64 b) { return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull); }

// what the entries are ordered by.  kind 0: integer, 1: binary32 bits, 2: binary64 bits
__device__ __forceinline__ u64 ls_sort_key(u64 key, int kind) {
  return kind == 0 ? key : kind == 1 ? (u64)f2ord(__uint_as_float((uint32_t)key)) : d2ord(key);
}
inline int ls_key_kind(int dtype) { return dtype == EDT_F32 ? 1 : dtype == EDT_F64 ? 2 : 0; }

// The outputs every table has: the keys under the label type, ascending, and the number of labels.  A unit's outputs derive from it.
struct LabelOut {
  void *keys;
  int64_t *n;
  int key_bytes;
  int key_kind;  // 0: integer, 1: binary32 bits, 2: binary64 bits
  __device__ __forceinline__ void store_key(int64_t rank, u64 key) const {
    switch (key_bytes) {
      case 1: ((uint8_t *)keys)[rank] = (uint8_t)key; break;
      case 2: ((uint16_t *)keys)[rank] = (uint16_t)key; break;
      case 4: ((uint32_t *)keys)[rank] = (uint32_t)key; break;
      default: ((uint64_t *)keys)[rank] = (uint64_t)key; break;
    }
  }
};
inline LabelOut label_out(void *keys, int64_t *n, int dtype) { return {keys, n, dtype_size(dtype), ls_key_kind(dtype)}; }

__device__ __forceinline__ u64 ls_hash(u64 h) {  // all 64 bits reach every bit of the result
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

template <typename V> __device__ __forceinline__ V ls_peek(const V *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// The slot of `key` (!= 0) in the global table, -1 if it has none (INSERT: and could get none -- the overflow word is set).
// The probe loop is bounded by the table size and leaves early once the overflow word is set: no lane ever waits for another.
template <bool INSERT>
__device__ int64_t ls_find(const LabelTable &t, u64 key) {
  if (t.direct) return (int64_t)key;
  const u64 mask = (u64)t.slots - 1;
  u64 h = ls_hash(key) & mask;
  for (int64_t p = 0; p < t.slots; ++p, h = (h + 1) & mask) {
    u64 k = ls_peek(&t.keys[h]);
    if (k == key) return (int64_t)h;
    if (k == 0) {
      if (!INSERT) return -1;
      k = atomicCAS(&t.keys[h], 0ull, key);
      if (k == 0) {
        if (atomicAdd(&t.ctrl[0], 1ull) + 1 > (u64)t.cap) atomicMax(&t.ctrl[1], 1ull);
        return (int64_t)h;
      }
      if (k == key) return (int64_t)h;
    }
    if ((p & 31) == 31 && ls_peek(&t.ctrl[1])) break;  // the table's contents no longer matter
  }
  if (INSERT) atomicMax(&t.ctrl[1], 1ull);
  return -1;
}

// (x, y, z) += o voxels along the flattened volume; extents are below 2^31 (check_shape) and o <= 1024: 32-bit throughout
__device__ __forceinline__ void ls_advance(uint32_t sx, uint32_t sy, uint32_t &x, uint32_t &y, uint32_t &z, uint32_t o) {
  x += o;
  if (x < sx) return;
  uint32_t q = x / sx;
  x -= q * sx;
  y += q;
  if (y < sy) return;
  q = y / sy;
  y -= q * sy;
  z += q;
}


// ---- the flat walk: a wave takes kLsTile consecutive voxels per step, a workgroup a contiguous range of tiles ----------------
// contiguous ranges (few labels per workgroup): at most `max_blocks` workgroups of `per` tiles each, a multiple of the waves
struct LsSweepGrid {
  int64_t per;
  unsigned blocks;
};
inline LsSweepGrid ls_sweep_grid(int64_t ntiles, int64_t max_blocks) {
  const int waves = kLsThreads / 64;
  const int64_t blocks = std::min<int64_t>(ceil_div(ntiles, waves), max_blocks);
  const int64_t per = ceil_div(ceil_div(ntiles, blocks), waves) * waves;
  return {per, (unsigned)ceil_div(ntiles, per)};
}

// the tiles [t0, t1) of this workgroup
struct LsTiles {
  int64_t t0, t1;
};
__device__ __forceinline__ LsTiles ls_block_tiles(int64_t voxels, int64_t tiles_per_block) {
  const int64_t ntiles = (voxels + kLsTile - 1) / kLsTile;
  const int64_t t0 = blockIdx.x * tiles_per_block;
  return {t0, t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles};
}

// coordinates of the first voxel of `tile`
__device__ __forceinline__ void ls_tile_coords(int64_t tile, uint32_t sx, uint32_t sy, uint32_t &bx, uint32_t &by, uint32_t &bz) {
  const int64_t base = tile * kLsTile, r = base / sx;
  bx = (uint32_t)(base - r * sx);
  by = (uint32_t)(r % sy);
  bz = (uint32_t)(r / sy);
}

// The runs of one 64-lane group: a run starts in lane 0, where the key changes and where the caller says a row starts
// (`row_start`: x == 0 for a sweep whose partials are per x-row, false for one that only needs equal keys).
struct LsRun {
  bool start;   // this lane is the first of its run
  uint64_t m;   // the ballot of `start`
  int s;        // first lane of this lane's run (bit 0 of m is always set)
  bool end;     // this lane is the last of its run
};
__device__ __forceinline__ LsRun ls_run_bounds(u64 k, int lane, bool row_start) {
  LsRun r;
  const u64 pk = __shfl_up(k, 1);
  r.start = lane == 0 || pk != k || row_start;
  r.m = __ballot(r.start);
  r.s = 63 - __builtin_clzll(r.m & ((2ull << lane) - 1ull));
  r.end = lane == 63 || ((r.m >> (lane + 1)) & 1ull);
  return r;
}

// The slot of `key` (!= 0) in a workgroup's LDS table of SLOTS keys, claimed by compare-and-swap within PROBES probes; -1: none,
// the partial goes past it into the global table.
template <int SLOTS, int PROBES>
__device__ __forceinline__ int ls_lds_claim(u64 *s_key, u64 key) {
  uint32_t h = (uint32_t)(ls_hash(key) >> 40) & (SLOTS - 1);
  for (int p = 0; p < PROBES; ++p, h = (h + 1) & (SLOTS - 1)) {
    u64 cur = ((volatile u64 *)s_key)[h];
    if (cur == 0) cur = atomicCAS(&s_key[h], 0ull, key);
    if (cur == 0 || cur == key) return (int)h;
  }
  return -1;
}

// ---- a table of sums: SUMS u64 words per slot side by side (a label's sums are one stretch), only ever added to ----------------
template <int SUMS>
struct AccTable : LabelTable {
  u64 *acc = nullptr;
  static AccTable carve(void *ws, int dtype, int64_t cap) {
    return carve_label_table<AccTable>(ws, dtype, cap, [](AccTable &t, Carver &c, size_t n) { t.acc = c.take<u64>(SUMS * n); });
  }
  // m[0 .. N) onto the words first .. first + N of slot s (s < 0: the key got no slot); a zero costs no atomic
  template <int N, typename W>
  __device__ __forceinline__ void add(int64_t s, int first, const W (&m)[N]) const {
    if (s < 0) return;
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (m[k] != 0) atomicAdd(&acc[s * SUMS + first + k], (u64)m[k]);
  }
  // A workgroup's LDS table (SLOTS keys, SUMS words of type W per key) into the global one, by all its threads, after a
  // barrier: a label's global slot once (it takes the key's place), then its sums side by side.
  template <int SLOTS, typename W>
  __device__ __forceinline__ void flush(u64 *s_key, const W *s_acc) const {
    for (int i = threadIdx.x; i < SLOTS; i += kLsThreads) s_key[i] = (u64)(s_key[i] != 0 ? ls_find<true>(*this, s_key[i]) : -1);
    __syncthreads();
    for (int e = threadIdx.x; e < SLOTS * SUMS; e += kLsThreads) {
      const int i = e / SUMS;
      const int64_t s = (int64_t)s_key[i];
      const W v = s_acc[e];
      if (s >= 0 && v != 0) atomicAdd(&acc[s * SUMS + (e - i * SUMS)], (u64)v);
    }
  }
};

// clear-on-use: a reused workspace needs no memset.  A block clears the keys of 256 slots and their sums as one stretch:
// consecutive lanes, consecutive words.
template <int SUMS>
__global__ __launch_bounds__(256) void k_acc_clear(AccTable<SUMS> t) {
  const int64_t b0 = blockIdx.x * (int64_t)blockDim.x, i = b0 + threadIdx.x;
  if (i < 4) t.ctrl[i] = 0;
  if (i < t.slots) t.keys[i] = 0;
  const int64_t words = t.slots * SUMS;
#pragma unroll
  for (int k = 0; k < SUMS; ++k) {
    const int64_t e = b0 * SUMS + k * 256 + threadIdx.x;
    if (e < words) t.acc[e] = 0;
  }
}

inline unsigned label_clear_blocks(const LabelTable &t) { return (unsigned)ceil_div(std::max<int64_t>(t.slots, 4), 256); }

template <int SUMS>
int launch_acc_clear(const char *pass, const AccTable<SUMS> &t, hipStream_t stream) {
  ScopedPass sp(pass, stream);
  hipLaunchKernelGGL(k_acc_clear<SUMS>, dim3(label_clear_blocks(t)), dim3(256), 0, stream, t);
  EDT_HIP_TRY(hipGetLastError());
  return EDT_OK;
}

// ---- the finish: the entries in key order, through the unit's Emit --------------------------------------------------------------
// direct table: one workgroup; thread i owns a contiguous range of slots, so ranks follow the keys
template <typename Emit>
__global__ __launch_bounds__(1024) void k_label_finish_direct(Emit e) {
  __shared__ uint32_t s_scan[1024];
  const int tid = threadIdx.x;
  const int64_t per = (e.t.slots + 1023) / 1024;
  const int64_t lo = tid * per < e.t.slots ? tid * per : e.t.slots;
  const int64_t hi = lo + per < e.t.slots ? lo + per : e.t.slots;
  uint32_t mine = 0;
  for (int64_t i = lo; i < hi; ++i) mine += e.occupied(i);
  s_scan[tid] = mine;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const uint32_t add = tid >= off ? s_scan[tid - off] : 0u;
    __syncthreads();
    s_scan[tid] += add;
    __syncthreads();
  }
  int64_t rank = (int64_t)(s_scan[tid] - mine);
  if (tid == 1023) *e.o.n = (int64_t)s_scan[1023];
  for (int64_t i = lo; i < hi; ++i)
    if (e.occupied(i)) {
      if (rank < e.t.cap) e(i, (u64)i, rank);
      ++rank;
    }
}

__global__ __launch_bounds__(256) void k_label_compact(LabelTable t) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= t.slots || t.keys[i] == 0) return;
  const u64 pos = atomicAdd(&t.ctrl[2], 1ull);
  if (pos < (u64)t.cap) t.list[pos] = (u64)i;
}

// hashed table: the rank of an entry is the number of entries with a smaller sort key
template <typename Emit>
__global__ __launch_bounds__(256) void k_label_rank(Emit e) {
  __shared__ u64 s_k[256];
  const int tid = threadIdx.x;
  const u64 n = e.t.ctrl[0];
  if (blockIdx.x == 0 && tid == 0) *e.o.n = (int64_t)n;
  if (e.t.ctrl[1] != 0 || n > (u64)e.t.cap || (u64)blockIdx.x * 256 >= n) return;  // (uniform) overflow: contents unspecified
  const u64 i = (u64)blockIdx.x * 256 + tid;
  int64_t slot = 0;
  u64 key = 0, mine = 0;
  if (i < n) {
    slot = (int64_t)e.t.list[i];
    key = e.t.keys[slot];
    mine = ls_sort_key(key, e.o.key_kind);
  }
  int64_t rank = 0;
  for (u64 j0 = 0; j0 < n; j0 += 256) {
    __syncthreads();
    if (j0 + tid < n) s_k[tid] = ls_sort_key(e.t.keys[e.t.list[j0 + tid]], e.o.key_kind);
    __syncthreads();
    const int cnt = n - j0 < 256 ? (int)(n - j0) : 256;
    for (int j = 0; j < cnt; ++j) rank += s_k[j] < mine;
  }
  if (i < n) e(slot, key, rank);
}

template <typename Emit>
int launch_label_finish(const char *pass, const Emit &e, hipStream_t stream) {
  ScopedPass sp(pass, stream);
  if (e.t.direct) {
    hipLaunchKernelGGL(k_label_finish_direct<Emit>, dim3(1), dim3(1024), 0, stream, e);
  } else {
    hipLaunchKernelGGL(k_label_compact, dim3((unsigned)ceil_div(e.t.slots, 256)), dim3(256), 0, stream, (LabelTable)e.t);
    EDT_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_label_rank<Emit>, dim3((unsigned)ceil_div(e.t.cap, 256)), dim3(256), 0, stream, e);
  }
  EDT_HIP_TRY(hipGetLastError());
  return EDT_OK;
}

}  // namespace
}  // namespace edt_amd
