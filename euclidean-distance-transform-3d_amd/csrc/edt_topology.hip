// edt_topology.hip -- label_topology: per-label cell counts of the closed cubical complex and of its interior, for every non-zero
// label at once, on device-resident data (include/edt_hip.h states the contract; edt_topology_math.h what one voxel adds).
//
// Keys, the hash, the insertion into the global table and the order of the entries are label_stats' (edt_labeltable.h); the
// clear-on-use table, the workgroup's LDS table and the finish follow label_moments (edt_moments.hip).  What is new is the sweep:
// every voxel needs the equality of its 26 neighbours, and the volume is still read about once.
//
//   k_tp_clear   the global table (clear-on-use: a reused scratch needs no memset)
//   k_tp_sweep   a workgroup takes a tile of 62 x 16 voxels in x and y and marches it along a z-chunk.  A wave holds six rows
//                (its four and one halo row either side) of the three current z-slices in registers, one column per lane:
//                lanes 1..62 own a voxel, lanes 0 and 63 hold the x-halo; positions outside the volume read as key 0.  The
//                nine compares against a voxel's own column stay in the lane; for the columns left and right the CENTRE key is
//                handed one lane over, compared there, and the nine bits are handed back: six lane exchanges per row of 62
//                voxels.  Each lane keeps the sixteen counts of the label it is in, per row, and posts them to the workgroup's
//                LDS table (kTpLdsSlots slots of a key and sixteen u32, compare-and-swap on the key, 8 probes; a partial that
//                finds no slot goes to the global table) when the label changes along z.  A step whose three slices are one
//                label over the whole wave is counted in a scalar and posted once as n * (1, ..., 1): the short cut for solid
//                tiles.  A row whose voxels all have a solid neighbourhood adds (1, ..., 1) per lane without the cell loop.
//   finish       as label_moments: direct tables are scanned in slot order by one workgroup; hashed ones are compacted into a
//                list and written at their rank.
// Global table: keys[slots], then sixteen u64 per slot side by side.  All arithmetic is integer.
#include "edt_labeltable.h"
#include "edt_topology_math.h"

namespace edt_amd {
namespace {

constexpr int kTpCols = 62;              // voxels per wave row: a wave's 64 lanes less the two halo columns
constexpr int kTpRows = 4;               // rows per wave
constexpr int kTpWaves = kLsThreads / 64;
constexpr int kTpTileY = kTpRows * kTpWaves;
constexpr int kTpLdsSlots = 256;         // 18 KiB of LDS per workgroup
constexpr int kTpLdsProbes = 8;
constexpr int64_t kTpMaxChunk = 65536;   // slices per z-chunk: a scalar step count times 248 stays below 2^32
constexpr int64_t kTpMaxBlocks = 1 << 20;
constexpr uint64_t kTpFlushVoxels = 1ull << 28;   // a workgroup's LDS counts are u32 and at most 8 per voxel

struct TpTable {
  u64 *keys = nullptr;   // hashed: the key of a slot (direct: unused, slot = key)
  u64 *acc = nullptr;    // kTpSums words per slot
  u64 *ctrl = nullptr;   // [0] distinct keys inserted, [1] overflow, [2] entries of `list`
  u64 *list = nullptr;   // hashed: the occupied slots, in no particular order
  int64_t slots = 0, cap = 0;
  int direct = 0;
  size_t bytes = 0;
};

struct TpOut {
  void *keys;
  int64_t *closed, *interior;
  int64_t *n;
  int key_bytes;
  int key_kind;
};

// tiles of 62 x 16 voxels in x and y, times chunks of `zlen` slices; tile = xi + xt * (yi + yt * zi)
struct TpGrid {
  int64_t xt, yt, zlen, tiles;
};

TpTable carve_topology(void *ws, int dtype, int64_t cap) {
  TpTable t;
  t.cap = cap;
  t.direct = dtype_size(dtype) <= 2;
  t.slots = ls_slots(dtype, cap);
  Carver c(ws);
  const size_t n = (size_t)t.slots;
  t.keys = c.take<u64>(n);
  t.acc = c.take<u64>(kTpSums * n);
  t.ctrl = c.take<u64>(4);
  if (!t.direct) t.list = c.take<u64>((size_t)cap);
  t.bytes = align_up(c.off, 256);
  return t;
}

TpGrid topology_grid(int64_t sx, int64_t sy, int64_t sz) {
  TpGrid g;
  g.xt = ceil_div(sx, kTpCols);
  g.yt = ceil_div(sy, kTpTileY);
  // enough tiles to fill the device, chunks of at least 16 slices (two of a chunk's slices are read again by its neighbours)
  int64_t zc = std::min(ceil_div(int64_t(4096), g.xt * g.yt), ceil_div(sz, int64_t(16)));
  zc = std::max(zc, ceil_div(sz, kTpMaxChunk));
  g.zlen = ceil_div(sz, zc);
  g.tiles = g.xt * g.yt * ceil_div(sz, g.zlen);
  return g;
}

__global__ __launch_bounds__(256) void k_tp_clear(TpTable t) {
  const int64_t b0 = blockIdx.x * (int64_t)blockDim.x, i = b0 + threadIdx.x;
  if (i < 4) t.ctrl[i] = 0;
  if (i < t.slots) t.keys[i] = 0;
  const int64_t words = t.slots * kTpSums;   // the sums of the block's 256 slots are one stretch
#pragma unroll
  for (int k = 0; k < kTpSums; ++k) {
    const int64_t e = b0 * kTpSums + k * 256 + threadIdx.x;
    if (e < words) t.acc[e] = 0;
  }
}

// ---- the sweep ------------------------------------------------------------------------------------------------------
// K: what a key is held as in registers -- 32 bits where the label type has no more
template <typename T, bool BOOL, typename K>
__global__ __launch_bounds__(kLsThreads) void k_tp_sweep(const T *__restrict__ labels, int64_t sx, int64_t sy, int64_t sz, TpGrid g,
                                                         TpTable t) {
  __shared__ u64 s_key[kTpLdsSlots];
  __shared__ uint32_t s_acc[kTpLdsSlots * kTpSums];
  auto clear = [&]() {
    for (int i = threadIdx.x; i < kTpLdsSlots; i += kLsThreads) s_key[i] = 0;
    for (int i = threadIdx.x; i < kTpLdsSlots * kTpSums; i += kLsThreads) s_acc[i] = 0;
  };
  // the workgroup's table into the global one: a label's global slot once (it takes the key's place), then its sixteen sums
  auto flush = [&]() {
    for (int i = threadIdx.x; i < kTpLdsSlots; i += kLsThreads) s_key[i] = (u64)(s_key[i] != 0 ? ls_find<true>(t, s_key[i]) : -1);
    __syncthreads();
    for (int e = threadIdx.x; e < kTpLdsSlots * kTpSums; e += kLsThreads) {
      const int64_t s = (int64_t)s_key[e / kTpSums];
      const uint32_t v = s_acc[e];
      if (s >= 0 && v != 0) atomicAdd(&t.acc[s * kTpSums + e % kTpSums], (u64)v);
    }
  };
  // the counts of label k into the workgroup's table, or past it into the global one
  auto post = [&](u64 k, const uint32_t (&c)[kTpTypes], const uint32_t (&in)[kTpTypes]) {
    int slot = -1;
    uint32_t h = (uint32_t)(ls_hash(k) >> 40) & (kTpLdsSlots - 1);
    for (int p = 0; p < kTpLdsProbes; ++p, h = (h + 1) & (kTpLdsSlots - 1)) {
      u64 cur = ((volatile u64 *)s_key)[h];
      if (cur == 0) cur = atomicCAS(&s_key[h], 0ull, k);
      if (cur == 0 || cur == k) {
        slot = (int)h;
        break;
      }
    }
    if (slot >= 0) {
#pragma unroll
      for (int j = 0; j < kTpTypes; ++j) {
        if (c[j] != 0) atomicAdd(&s_acc[slot * kTpSums + j], c[j]);
        if (in[j] != 0) atomicAdd(&s_acc[slot * kTpSums + kTpTypes + j], in[j]);
      }
    } else {
      const int64_t s = ls_find<true>(t, k);
      if (s < 0) return;
#pragma unroll
      for (int j = 0; j < kTpTypes; ++j) {
        if (c[j] != 0) atomicAdd(&t.acc[s * kTpSums + j], (u64)c[j]);
        if (in[j] != 0) atomicAdd(&t.acc[s * kTpSums + kTpTypes + j], (u64)in[j]);
      }
    }
  };

  clear();
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t since_flush = 0;
  for (int64_t tile = blockIdx.x; tile < g.tiles; tile += gridDim.x) {
    const int64_t xi = tile % g.xt, rest = tile / g.xt, yi = rest % g.yt, zi = rest / g.yt;
    const int64_t x = xi * kTpCols - 1 + lane;                    // this lane's column
    const int64_t y0 = yi * kTpTileY + wave * kTpRows - 1;        // the first of the wave's six rows
    const int64_t z0 = zi * g.zlen, z1 = z0 + g.zlen < sz ? z0 + g.zlen : sz;
    if (y0 + 1 < sy) {
      const bool x_in = x >= 0 && x < sx;
      const bool owner = lane >= 1 && lane <= kTpCols && x < sx;  // the lane owns the voxels of its column
      K s[3][kTpRows + 2];                                        // slices z - 1, z, z + 1
      K first[3];                                                 // a slice's key in lane 0, row 0 ...
      bool one[3];                                                // ... and whether the whole slice is that key
      auto load = [&](int64_t z, int d) {
        const bool z_in = z >= 0 && z < sz;
        bool same = true;
#pragma unroll
        for (int r = 0; r < kTpRows + 2; ++r) {
          const int64_t y = y0 + r;
          const bool in = x_in && z_in && y >= 0 && y < sy;
          s[d][r] = in ? (K)ls_key<T, BOOL>(labels[x + sx * (y + sy * z)]) : (K)0;
        }
        first[d] = __shfl(s[d][0], 0);
#pragma unroll
        for (int r = 0; r < kTpRows + 2; ++r) same = same && s[d][r] == first[d];
        one[d] = __all(same);
      };
      load(z0 - 1, 0);
      load(z0, 1);
      K cur[kTpRows];                                             // the label whose counts the lane holds, per row (0: none)
      uint32_t ac[kTpRows][kTpTypes], ai[kTpRows][kTpTypes];
#pragma unroll
      for (int r = 0; r < kTpRows; ++r) {
        cur[r] = 0;
#pragma unroll
        for (int j = 0; j < kTpTypes; ++j) ac[r][j] = ai[r][j] = 0;
      }
      K solid_key = 0;                                            // (wave-uniform) solid steps of this label, not yet posted
      uint32_t solid_steps = 0;
      auto post_solid = [&]() {
        if (solid_steps != 0 && lane == 0) {
          uint32_t n[kTpTypes];
#pragma unroll
          for (int j = 0; j < kTpTypes; ++j) n[j] = solid_steps * (uint32_t)(kTpCols * kTpRows);
          post((u64)solid_key, n, n);
        }
        solid_steps = 0;
      };
      // one step past the chunk: nothing is counted there, every lane posts what it holds
      for (int64_t z = z0; z <= z1; ++z) {
        const bool last = z == z1;
        if (!last) {
          load(z + 1, 2);
          // the three slices one label over the wave (then no position of them lies outside the volume, or the label is 0)
          if (one[0] && one[1] && one[2] && first[0] == first[1] && first[1] == first[2]) {
            if (first[1] != solid_key) {
              post_solid();
              solid_key = first[1];
            }
            if (first[1] != 0) ++solid_steps;
#pragma unroll
            for (int r = 0; r < kTpRows + 2; ++r) {
              s[0][r] = s[1][r];
              s[1][r] = s[2][r];
            }
            first[0] = first[1], first[1] = first[2], one[0] = one[1], one[1] = one[2];
            continue;
          }
        }
#pragma unroll
        for (int r = 0; r < kTpRows; ++r) {
          const K k = last ? (K)0 : s[1][r + 1];
          const bool act = owner && k != 0 && y0 + 1 + r < sy;
          uint32_t eq = 0;
          if (!last) {
            const K kl = __shfl_up(k, 1), kr = __shfl_down(k, 1);   // the centres one lane to the left and to the right
            uint32_t own = 0, for_left = 0, for_right = 0;
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
              for (int dy = 0; dy < 3; ++dy) {
                const K nk = s[d][r + dy];
                const int j = dy + 3 * d;
                own |= (uint32_t)(nk == k) << j;
                for_left |= (uint32_t)(nk == kl) << j;     // this column is the left centre's ex = +1
                for_right |= (uint32_t)(nk == kr) << j;    // and the right centre's ex = -1
              }
            eq = __shfl_up(for_right, 1) | own << 9 | __shfl_down(for_left, 1) << 18;
          }
          if ((act && k != cur[r]) || (last && cur[r] != 0)) {
            if (cur[r] != 0) post((u64)cur[r], ac[r], ai[r]);
#pragma unroll
            for (int j = 0; j < kTpTypes; ++j) ac[r][j] = ai[r][j] = 0;
            cur[r] = act ? k : (K)0;
          }
          if (!last) {
            if (__all(!act || topo_solid(eq))) {
#pragma unroll
              for (int j = 0; j < kTpTypes; ++j) {
                ac[r][j] += (uint32_t)act;
                ai[r][j] += (uint32_t)act;
              }
            } else if (act) {
              topo_voxel(eq, ac[r], ai[r]);
            }
          }
        }
        if (!last) {
#pragma unroll
          for (int r = 0; r < kTpRows + 2; ++r) {
            s[0][r] = s[1][r];
            s[1][r] = s[2][r];
          }
          first[0] = first[1], first[1] = first[2], one[0] = one[1], one[1] = one[2];
        }
      }
      post_solid();
    }
    since_flush += (uint64_t)(kTpCols * kTpTileY) * (uint64_t)g.zlen;
    if (since_flush >= kTpFlushVoxels) {   // (uniform over the workgroup)
      __syncthreads();
      flush();
      __syncthreads();
      clear();
      __syncthreads();
      since_flush = 0;
    }
  }
  __syncthreads();
  flush();
}

// ---- finish ---------------------------------------------------------------------------------------------------------
__device__ void tp_emit(const TpTable &t, const TpOut &o, int64_t slot, u64 key, int64_t rank) {
  ls_store_key(o.keys, o.key_bytes, rank, key);
#pragma unroll
  for (int k = 0; k < kTpTypes; ++k) {
    o.closed[kTpTypes * rank + k] = (int64_t)t.acc[slot * kTpSums + k];
    o.interior[kTpTypes * rank + k] = (int64_t)t.acc[slot * kTpSums + kTpTypes + k];
  }
}

constexpr int kTpVoxels = kTpTypes - 1;   // closed cells along all three axes: the label's voxels, never 0 for a label

// direct table: one workgroup; thread i owns a contiguous range of slots, so ranks follow the keys
__global__ __launch_bounds__(1024) void k_tp_finish_direct(TpTable t, TpOut o) {
  __shared__ uint32_t s_scan[1024];
  const int tid = threadIdx.x;
  const int64_t per = (t.slots + 1023) / 1024;
  const int64_t lo = tid * per < t.slots ? tid * per : t.slots;
  const int64_t hi = lo + per < t.slots ? lo + per : t.slots;
  uint32_t mine = 0;
  for (int64_t i = lo; i < hi; ++i) mine += t.acc[i * kTpSums + kTpVoxels] != 0;
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
    if (t.acc[i * kTpSums + kTpVoxels] != 0) {
      if (rank < t.cap) tp_emit(t, o, i, (u64)i, rank);
      ++rank;
    }
}

__global__ __launch_bounds__(256) void k_tp_compact(TpTable t) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= t.slots || t.keys[i] == 0) return;
  const u64 pos = atomicAdd(&t.ctrl[2], 1ull);
  if (pos < (u64)t.cap) t.list[pos] = (u64)i;
}

// hashed table: the rank of an entry is the number of entries with a smaller sort key
__global__ __launch_bounds__(256) void k_tp_rank(TpTable t, TpOut o) {
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
  if (i < n) tp_emit(t, o, slot, key, rank);
}

template <typename T, bool BOOL, typename K>
int launch_tp_t(const T *labels, int64_t sx, int64_t sy, int64_t sz, const TpTable &t, const TpOut &o, hipStream_t stream) {
  {
    ScopedPass sp("label_topology clear", stream);
    hipLaunchKernelGGL(k_tp_clear, dim3((unsigned)ceil_div(std::max<int64_t>(t.slots, 4), 256)), dim3(256), 0, stream, t);
    EDT_HIP_TRY(hipGetLastError());
  }
  {
    ScopedPass sp("label_topology sweep", stream);
    const TpGrid g = topology_grid(sx, sy, sz);
    hipLaunchKernelGGL((k_tp_sweep<T, BOOL, K>), dim3((unsigned)std::min(g.tiles, kTpMaxBlocks)), dim3(kLsThreads), 0, stream, labels,
                       sx, sy, sz, g, t);
    EDT_HIP_TRY(hipGetLastError());
  }
  {
    ScopedPass sp("label_topology finish", stream);
    if (t.direct) {
      hipLaunchKernelGGL(k_tp_finish_direct, dim3(1), dim3(1024), 0, stream, t, o);
    } else {
      hipLaunchKernelGGL(k_tp_compact, dim3((unsigned)ceil_div(t.slots, 256)), dim3(256), 0, stream, t);
      EDT_HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_tp_rank, dim3((unsigned)ceil_div(t.cap, 256)), dim3(256), 0, stream, t, o);
    }
    EDT_HIP_TRY(hipGetLastError());
  }
  return EDT_OK;
}

}  // namespace

// what both forms refuse after the shape: a bad max_labels
int topology_check_args(int64_t max_labels) {
  if (max_labels < 1) { set_error("label_topology: max_labels must be at least 1"); return EDT_ERR_BAD_ARG; }
  // (the rank kernel runs one thread per entry: its grid has to fit 32 bits)
  if (max_labels > (int64_t(1) << 38)) { set_error("label_topology: max_labels beyond 2^38"); return EDT_ERR_BAD_ARG; }
  return EDT_OK;
}

}  // namespace edt_amd

using namespace edt_amd;

extern "C" {

size_t edt_hip_label_topology_workspace_bytes(int dtype, int64_t voxels, int64_t max_labels) {
  if (dtype_size(dtype) == 0 || voxels < 0 || max_labels < 1 || max_labels > (int64_t(1) << 38)) return 0;
  return carve_topology(nullptr, dtype, ls_cap(voxels, max_labels)).bytes;
}

int edt_hip_label_topology_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int64_t max_labels,
                                  void *d_keys, int64_t *d_closed, int64_t *d_interior, int64_t *d_n_labels, void *d_scratch,
                                  size_t scratch_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int own = check_shape(dtype, ndim, sx, sy, sz);
  if (own == EDT_OK) own = topology_check_args(max_labels);
  const int64_t voxels = own == EDT_OK ? sx * sy * sz : 0;
  int rc;
  if (!label_op_begin("label_topology", own, d_n_labels, 1, voxels, !d_labels || !d_keys || !d_closed || !d_interior, false,
                      d_scratch, scratch_bytes, edt_hip_label_topology_workspace_bytes(dtype, voxels, max_labels),
                      "edt_hip_label_topology_workspace_bytes", stream, &rc))
    return rc;
  const TpTable t = carve_topology(d_scratch, dtype, ls_cap(voxels, max_labels));
  const TpOut o = {d_keys, d_closed, d_interior, d_n_labels, dtype_size(dtype), ls_key_kind(dtype)};
  switch (dtype) {
    case EDT_U8: return launch_tp_t<uint8_t, false, uint32_t>((const uint8_t *)d_labels, sx, sy, sz, t, o, stream);
    case EDT_BOOL: return launch_tp_t<uint8_t, true, uint32_t>((const uint8_t *)d_labels, sx, sy, sz, t, o, stream);
    case EDT_U16: return launch_tp_t<uint16_t, false, uint32_t>((const uint16_t *)d_labels, sx, sy, sz, t, o, stream);
    case EDT_U32: return launch_tp_t<uint32_t, false, uint32_t>((const uint32_t *)d_labels, sx, sy, sz, t, o, stream);
    case EDT_U64: return launch_tp_t<uint64_t, false, u64>((const uint64_t *)d_labels, sx, sy, sz, t, o, stream);
    case EDT_F32: return launch_tp_t<float, false, uint32_t>((const float *)d_labels, sx, sy, sz, t, o, stream);
    case EDT_F64: return launch_tp_t<double, false, u64>((const double *)d_labels, sx, sy, sz, t, o, stream);
    default: set_error("unknown dtype"); return EDT_ERR_BAD_ARG;
  }
}

}  // extern "C"
