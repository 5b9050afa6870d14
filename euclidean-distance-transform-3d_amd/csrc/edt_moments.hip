// edt_moments.hip -- label_moments: per-label voxel count, exact raw first and second moments, centroid and population
// covariance, for every non-zero label at once, on device-resident data (include/edt_hip.h states the contract).
//
// Keys, the hash, the insertion into the global table, the walk over the flattened volume and the order of the entries are
// label_stats' (edt_labeltable.h).  What is new: the ten sums of an x-run -- n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz -- have a
// closed form in the run's first voxel and its length (run_moments, edt_moments_math.h), so ONE lane per run posts all of them
// and nothing is scanned over lanes.  Every reduction is a 64-bit integer add: the table is the same bits on every run.
//
//   k_mm_clear   the global table (clear-on-use: a reused workspace needs no memset)
//   k_mm_sweep   one pass over the labels, nothing else is read.  A wave takes 4 x 64 consecutive voxels per step.  Run starts
//                (label change or start of an x-row) come from a neighbour compare and a ballot; the run's LAST lane knows
//                (x0, n, y, z) from the ballot alone and adds the run's ten sums to the workgroup's LDS table (kMmLdsSlots
//                slots of a key and ten u64, compare-and-swap on the key, 8 probes); a partial that finds no slot goes to the
//                global table directly.  A step that is one label inside one row is one partial of n = 256 from lane 0: no
//                ballot, no reduction.  Every workgroup owns a contiguous range of the volume and flushes its LDS table once.
//   finish       as label_stats: 8/16-bit labels (direct table) are scanned in slot order by one workgroup; wider labels are
//                compacted into a list and written at their rank.  Writing an entry also derives centroid and covariance
//                from its exact sums (moments_derive: 128-bit integers, each value rounded once, by hand).
// Global table: keys[slots], then ten u64 per slot side by side (the flush adds a label's sums to one 80-byte stretch).
#include "edt_labeltable.h"
#include "edt_moments_math.h"

namespace edt_amd {
namespace {

constexpr int kMmLdsSlots = 256;   // 22.5 KiB of LDS per workgroup: 7 workgroups of 4 waves per compute unit
constexpr int kMmLdsProbes = 8;
constexpr int kMmBlocks = 256 * 7;

struct MmTable {
  u64 *keys = nullptr;   // hashed: the key of a slot (direct: unused, slot = key)
  u64 *acc = nullptr;    // kMmSums words per slot
  u64 *ctrl = nullptr;   // [0] distinct keys inserted, [1] overflow, [2] entries of `list`
  u64 *list = nullptr;   // hashed: the occupied slots, in no particular order
  int64_t slots = 0, cap = 0;
  int direct = 0;
  size_t bytes = 0;
};

struct MmOut {
  void *keys;
  int64_t *counts, *sums;
  double *centroid, *central;
  int64_t *n;
  int key_bytes;
  int key_kind;
};

MmTable carve_moments(void *ws, int dtype, int64_t cap) {
  MmTable t;
  t.cap = cap;
  t.direct = dtype_size(dtype) <= 2;
  t.slots = ls_slots(dtype, cap);
  Carver c(ws);
  const size_t n = (size_t)t.slots;
  t.keys = c.take<u64>(n);
  t.acc = c.take<u64>(kMmSums * n);
  t.ctrl = c.take<u64>(4);
  if (!t.direct) t.list = c.take<u64>((size_t)cap);
  t.bytes = align_up(c.off, 256);
  return t;
}

__global__ __launch_bounds__(256) void k_mm_clear(MmTable t) {
  const int64_t b0 = blockIdx.x * (int64_t)blockDim.x, i = b0 + threadIdx.x;
  if (i < 4) t.ctrl[i] = 0;
  if (i < t.slots) t.keys[i] = 0;
  const int64_t words = t.slots * kMmSums;   // the sums of the block's 256 slots are one stretch: consecutive lanes, consecutive words
#pragma unroll
  for (int k = 0; k < kMmSums; ++k) {
    const int64_t e = b0 * kMmSums + k * 256 + threadIdx.x;
    if (e < words) t.acc[e] = 0;
  }
}

__device__ __forceinline__ void mm_global_add(const MmTable &t, u64 key, const uint64_t (&m)[kMmSums]) {
  const int64_t s = ls_find<true>(t, key);
  if (s < 0) return;
#pragma unroll
  for (int k = 0; k < kMmSums; ++k)
    if (m[k] != 0) atomicAdd(&t.acc[s * kMmSums + k], (u64)m[k]);
}

// ---- the sweep ------------------------------------------------------------------------------------------------------
template <typename T, bool BOOL>
__global__ __launch_bounds__(kLsThreads) void k_mm_sweep(const T *__restrict__ labels, int64_t voxels, uint32_t sx, uint32_t sy,
                                                         int64_t tiles_per_block, MmTable t) {
  __shared__ u64 s_key[kMmLdsSlots], s_acc[kMmLdsSlots * kMmSums];
  for (int i = threadIdx.x; i < kMmLdsSlots; i += kLsThreads) s_key[i] = 0;
  for (int i = threadIdx.x; i < kMmLdsSlots * kMmSums; i += kLsThreads) s_acc[i] = 0;
  __syncthreads();

  // one run (x0 .. x0 + n - 1, y, z) of label k into the workgroup's table, or past it into the global one
  auto post = [&](u64 k, uint32_t x0, uint32_t n, uint32_t y, uint32_t z) {
    uint64_t m[kMmSums];
    run_moments(x0, n, y, z, m);
    int slot = -1;
    uint32_t h = (uint32_t)(ls_hash(k) >> 40) & (kMmLdsSlots - 1);
    for (int p = 0; p < kMmLdsProbes; ++p, h = (h + 1) & (kMmLdsSlots - 1)) {
      u64 cur = ((volatile u64 *)s_key)[h];
      if (cur == 0) cur = atomicCAS(&s_key[h], 0ull, k);
      if (cur == 0 || cur == k) {
        slot = (int)h;
        break;
      }
    }
    if (slot >= 0) {
#pragma unroll
      for (int j = 0; j < kMmSums; ++j) atomicAdd(&s_acc[slot * kMmSums + j], (u64)m[j]);
    } else {
      mm_global_add(t, k, m);
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
      const u64 pk = __shfl_up(k, 1);
      const bool start = lane == 0 || pk != k || x == 0;
      const uint64_t m = __ballot(start);
      const int s = 63 - __builtin_clzll(m & ((2ull << lane) - 1ull));  // first lane of this lane's run (bit 0 is always set)
      const bool end = lane == 63 || ((m >> (lane + 1)) & 1ull);
      if (end && k != 0)  // one partial per run: lanes s..lane of row (y, z)
        post(k, x - (uint32_t)(lane - s), (uint32_t)(lane - s + 1), y, z);
      ls_advance(sx, sy, x, y, z, 64u);
    }
    ls_advance(sx, sy, bx, by, bz, (uint32_t)(kLsTile * (kLsThreads / 64)));
  }
  __syncthreads();
  // the flush: a label's global slot once (it takes the key's place), then its ten sums side by side
  for (int i = threadIdx.x; i < kMmLdsSlots; i += kLsThreads) s_key[i] = (u64)(s_key[i] != 0 ? ls_find<true>(t, s_key[i]) : -1);
  __syncthreads();
  for (int e = threadIdx.x; e < kMmLdsSlots * kMmSums; e += kLsThreads) {
    const int i = e / kMmSums;
    const int64_t s = (int64_t)s_key[i];
    const u64 v = s_acc[e];
    if (s >= 0 && v != 0) atomicAdd(&t.acc[s * kMmSums + (e - i * kMmSums)], v);
  }
}

// ---- finish ---------------------------------------------------------------------------------------------------------
__device__ void mm_emit(const MmTable &t, const MmOut &o, int64_t slot, u64 key, int64_t rank) {
  ls_store_key(o.keys, o.key_bytes, rank, key);
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

// direct table: one workgroup; thread i owns a contiguous range of slots, so ranks follow the keys
__global__ __launch_bounds__(1024) void k_mm_finish_direct(MmTable t, MmOut o) {
  __shared__ uint32_t s_scan[1024];
  const int tid = threadIdx.x;
  const int64_t per = (t.slots + 1023) / 1024;
  const int64_t lo = tid * per < t.slots ? tid * per : t.slots;
  const int64_t hi = lo + per < t.slots ? lo + per : t.slots;
  uint32_t mine = 0;
  for (int64_t i = lo; i < hi; ++i) mine += t.acc[i * kMmSums + kMmN] != 0;
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
    if (t.acc[i * kMmSums + kMmN] != 0) {
      if (rank < t.cap) mm_emit(t, o, i, (u64)i, rank);
      ++rank;
    }
}

__global__ __launch_bounds__(256) void k_mm_compact(MmTable t) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= t.slots || t.keys[i] == 0) return;
  const u64 pos = atomicAdd(&t.ctrl[2], 1ull);
  if (pos < (u64)t.cap) t.list[pos] = (u64)i;
}

// hashed table: the rank of an entry is the number of entries with a smaller sort key
__global__ __launch_bounds__(256) void k_mm_rank(MmTable t, MmOut o) {
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
  if (i < n) mm_emit(t, o, slot, key, rank);
}

template <typename T, bool BOOL>
int launch_mm_t(const T *labels, int64_t voxels, int64_t sx, int64_t sy, const MmTable &t, const MmOut &o, hipStream_t stream) {
  {
    ScopedPass sp("label_moments clear", stream);
    hipLaunchKernelGGL(k_mm_clear, dim3((unsigned)ceil_div(std::max<int64_t>(t.slots, 4), 256)), dim3(256), 0, stream, t);
    EDT_HIP_TRY(hipGetLastError());
  }
  {
    ScopedPass sp("label_moments sweep", stream);
    const int64_t ntiles = ceil_div(voxels, kLsTile);
    const int waves = kLsThreads / 64;
    const int64_t blocks = std::min<int64_t>(ceil_div(ntiles, waves), kMmBlocks);
    const int64_t per = ceil_div(ceil_div(ntiles, blocks), waves) * waves;  // (contiguous ranges: few labels per workgroup)
    hipLaunchKernelGGL((k_mm_sweep<T, BOOL>), dim3((unsigned)ceil_div(ntiles, per)), dim3(kLsThreads), 0, stream, labels, voxels,
                       (uint32_t)sx, (uint32_t)sy, per, t);
    EDT_HIP_TRY(hipGetLastError());
  }
  {
    ScopedPass sp("label_moments finish", stream);
    if (t.direct) {
      hipLaunchKernelGGL(k_mm_finish_direct, dim3(1), dim3(1024), 0, stream, t, o);
    } else {
      hipLaunchKernelGGL(k_mm_compact, dim3((unsigned)ceil_div(t.slots, 256)), dim3(256), 0, stream, t);
      EDT_HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_mm_rank, dim3((unsigned)ceil_div(t.cap, 256)), dim3(256), 0, stream, t, o);
    }
    EDT_HIP_TRY(hipGetLastError());
  }
  return EDT_OK;
}

}  // namespace

// what both forms refuse after the shape: a bad max_labels, a volume past the range bound
int moments_check_args(int64_t sx, int64_t sy, int64_t sz, int64_t max_labels) {
  if (max_labels < 1) { set_error("label_moments: max_labels must be at least 1"); return EDT_ERR_BAD_ARG; }
  // (the rank kernel runs one thread per entry: its grid has to fit 32 bits)
  if (max_labels > (int64_t(1) << 38)) { set_error("label_moments: max_labels beyond 2^38"); return EDT_ERR_BAD_ARG; }
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
  if (dtype_size(dtype) == 0 || voxels < 0 || max_labels < 1 || max_labels > (int64_t(1) << 38)) return 0;
  return carve_moments(nullptr, dtype, ls_cap(voxels, max_labels)).bytes;
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
  const MmTable t = carve_moments(d_scratch, dtype, ls_cap(voxels, max_labels));
  const MmOut o = {d_keys, d_counts, d_sums, d_centroid, d_central, d_n_labels, dtype_size(dtype), ls_key_kind(dtype)};
  switch (dtype) {
    case EDT_U8: return launch_mm_t<uint8_t, false>((const uint8_t *)d_labels, voxels, sx, sy, t, o, stream);
    case EDT_BOOL: return launch_mm_t<uint8_t, true>((const uint8_t *)d_labels, voxels, sx, sy, t, o, stream);
    case EDT_U16: return launch_mm_t<uint16_t, false>((const uint16_t *)d_labels, voxels, sx, sy, t, o, stream);
    case EDT_U32: return launch_mm_t<uint32_t, false>((const uint32_t *)d_labels, voxels, sx, sy, t, o, stream);
    case EDT_U64: return launch_mm_t<uint64_t, false>((const uint64_t *)d_labels, voxels, sx, sy, t, o, stream);
    case EDT_F32: return launch_mm_t<float, false>((const float *)d_labels, voxels, sx, sy, t, o, stream);
    case EDT_F64: return launch_mm_t<double, false>((const double *)d_labels, voxels, sx, sy, t, o, stream);
    default: set_error("unknown dtype"); return EDT_ERR_BAD_ARG;
  }
}

}  // extern "C"
