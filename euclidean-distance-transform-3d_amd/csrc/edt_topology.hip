// edt_topology.hip -- label_topology: per-label cell counts of the closed cubical complex and of its interior, for every non-zero
// label at once, on device-resident data (include/edt_hip.h states the contract; edt_topology_math.h what one voxel adds).
//
// This unit owns its grid, the sweep, TpEmit and the entry points.  The table (AccTable<16>: keys, the hash, the insertion, clear,
// add and flush), the LDS claim and the finish are the table module's (edt_labeltable.h).  Every voxel needs the equality of its
// 26 neighbours, and the volume is still read about once.
//
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
// All arithmetic is integer.
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

using TpTable = AccTable<kTpSums>;

struct TpOut : LabelOut {
  int64_t *closed, *interior;
};

// tiles of 62 x 16 voxels in x and y, times chunks of `zlen` slices; tile = xi + xt * (yi + yt * zi)
struct TpGrid {
  int64_t xt, yt, zlen, tiles;
};

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

// ---- the sweep ------------------------------------------------------------------------------------------------------
template <typename T, bool BOOL>
__global__ __launch_bounds__(kLsThreads) void k_tp_sweep(const T *__restrict__ labels, int64_t sx, int64_t sy, int64_t sz, TpGrid g,
                                                         TpTable t) {
  using K = std::conditional_t<sizeof(T) <= 4, uint32_t, u64>;  // a key in registers: 32 bits where the label type has no more
  __shared__ u64 s_key[kTpLdsSlots];
  __shared__ uint32_t s_acc[kTpLdsSlots * kTpSums];
  auto clear = [&]() {
    for (int i = threadIdx.x; i < kTpLdsSlots; i += kLsThreads) s_key[i] = 0;
    for (int i = threadIdx.x; i < kTpLdsSlots * kTpSums; i += kLsThreads) s_acc[i] = 0;
  };
  // the counts of label k into the workgroup's table, or past it into the global one
  auto post = [&](u64 k, const uint32_t (&c)[kTpTypes], const uint32_t (&in)[kTpTypes]) {
    const int slot = ls_lds_claim<kTpLdsSlots, kTpLdsProbes>(s_key, k);
    if (slot >= 0) {
#pragma unroll
      for (int j = 0; j < kTpTypes; ++j) {
        if (c[j] != 0) atomicAdd(&s_acc[slot * kTpSums + j], c[j]);
        if (in[j] != 0) atomicAdd(&s_acc[slot * kTpSums + kTpTypes + j], in[j]);
      }
    } else {
      const int64_t s = ls_find<true>(t, k);
      t.add(s, 0, c);
      t.add(s, kTpTypes, in);
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
      t.flush<kTpLdsSlots>(s_key, s_acc);
      __syncthreads();
      clear();
      __syncthreads();
      since_flush = 0;
    }
  }
  __syncthreads();
  t.flush<kTpLdsSlots>(s_key, s_acc);
}

constexpr int kTpVoxels = kTpTypes - 1;   // closed cells along all three axes: the label's voxels, never 0 for a label

struct TpEmit {
  TpTable t;
  TpOut o;
  __device__ bool occupied(int64_t slot) const { return t.acc[slot * kTpSums + kTpVoxels] != 0; }
  __device__ void operator()(int64_t slot, u64 key, int64_t rank) const {
    o.store_key(rank, key);
#pragma unroll
    for (int k = 0; k < kTpTypes; ++k) {
      o.closed[kTpTypes * rank + k] = (int64_t)t.acc[slot * kTpSums + k];
      o.interior[kTpTypes * rank + k] = (int64_t)t.acc[slot * kTpSums + kTpTypes + k];
    }
  }
};

template <typename T, bool BOOL>
int launch_tp_t(const T *labels, int64_t sx, int64_t sy, int64_t sz, const TpEmit &e, hipStream_t stream) {
  if (const int rc = launch_acc_clear("label_topology clear", e.t, stream)) return rc;
  {
    ScopedPass sp("label_topology sweep", stream);
    const TpGrid g = topology_grid(sx, sy, sz);
    hipLaunchKernelGGL((k_tp_sweep<T, BOOL>), dim3((unsigned)std::min(g.tiles, kTpMaxBlocks)), dim3(kLsThreads), 0, stream, labels,
                       sx, sy, sz, g, e.t);
    EDT_HIP_TRY(hipGetLastError());
  }
  return launch_label_finish("label_topology finish", e, stream);
}

}  // namespace

// what both forms refuse after the shape: a bad max_labels
int topology_check_args(int64_t max_labels) { return label_table_check_args("label_topology", max_labels); }

}  // namespace edt_amd

using namespace edt_amd;

extern "C" {

size_t edt_hip_label_topology_workspace_bytes(int dtype, int64_t voxels, int64_t max_labels) {
  if (!label_table_query_ok(dtype, voxels, max_labels)) return 0;
  return TpTable::carve(nullptr, dtype, ls_cap(voxels, max_labels)).bytes;
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
  const TpEmit e = {TpTable::carve(d_scratch, dtype, ls_cap(voxels, max_labels)),
                    {label_out(d_keys, d_n_labels, dtype), d_closed, d_interior}};
  return with_label_key(dtype, [&](auto t, auto is_bool) -> int {
    using T = typename decltype(t)::type;
    return launch_tp_t<T, decltype(is_bool)::value>((const T *)d_labels, sx, sy, sz, e, stream);
  });
}

}  // extern "C"
