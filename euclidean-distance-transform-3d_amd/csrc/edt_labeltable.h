// edt_labeltable.h -- what the per-label tables share: label_stats (edt_labelstats.hip) and label_moments (edt_moments.hip)
// reduce every label type to the same 64-bit KEY, hash it the same way, insert it into a global table by compare-and-swap on
// the key word, walk the flattened volume in the same 4 x 64 voxel steps and order their entries by the same sort key.
// Internal: nothing is exported.
//
// KEY: the value itself for integers, 1 for any non-zero bool byte, the bit pattern for floats with -0.0 folded into 0 and NaN
// mapped to 0 (a NaN voxel belongs to no label).  Key 0 is background and the empty-slot marker.
// A global table is any struct with `u64 *keys`, `u64 *ctrl` ([0] distinct keys inserted, [1] overflow), `int64_t slots, cap`
// and `int direct` (8- / 16-bit labels: slot = key).
#pragma once

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

__device__ __forceinline__ void ls_store_key(void *keys, int key_bytes, int64_t rank, u64 key) {
  switch (key_bytes) {
    case 1: ((uint8_t *)keys)[rank] = (uint8_t)key; break;
    case 2: ((uint16_t *)keys)[rank] = (uint16_t)key; break;
    case 4: ((uint32_t *)keys)[rank] = (uint32_t)key; break;
    default: ((uint64_t *)keys)[rank] = (uint64_t)key; break;
  }
}

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
template <bool INSERT, typename Table>
__device__ int64_t ls_find(const Table &t, u64 key) {
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

}  // namespace
}  // namespace edt_amd
