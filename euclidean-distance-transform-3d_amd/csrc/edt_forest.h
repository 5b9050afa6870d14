// edt_forest.h -- what the label operations share: connected_components (edt_components.hip), fill_holes (edt_fillholes.hip)
// and dust (edt_dust.hip) all stand on one union-find parent plane P.  launch_forest builds it: P[i] = the smallest idx of i's
// component -- its ROOT -- for a foreground voxel, a root holds itself, background holds kCcBg.  What an operation then keeps
// per component (a number, a cavity's state, a size) goes into the root's own word, under kCcTag.  Internal: nothing is exported.
#pragma once

#include "edt_api_internal.h"

namespace edt_amd {

// words of a parent plane: background, and the top bit that marks a root's word once it carries something else than itself
// (an idx is below 2^31, which is why a volume has at most kCcMaxVoxels voxels; a tagged rank is at most kCcTag | (2^31 - 2))
constexpr uint32_t kCcBg = 0xFFFFFFFFu;
constexpr uint32_t kCcTag = 0x80000000u;
constexpr int64_t kCcMaxVoxels = 0x7FFFFFFF;

template <typename T> __device__ __forceinline__ bool label_fg(T v) { return v != (T)0; }  // (-0.0 is background, NaN is not)
template <typename T> __device__ __forceinline__ bool label_conn(T a, T b, int binary) {
  return binary ? (label_fg(a) && label_fg(b)) : (a == b && label_fg(a));
}

// a parent word while other threads of the launch may be changing it
__device__ __forceinline__ uint32_t parent_peek(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the sum of v over the 64 lanes, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// The root rule, for a non-background voxel i of a flattened plane with p = P[i]: p >= i means i is a root and the word is its
// own, else p is the root and the word is P[p].  It holds whatever the operation has already added to or raised in a root's
// word: a root's word starts as the self-pointer i and only ever grows (atomicMax of a tagged state, atomicAdd of lengths and
// the tag, a tagged rank) without passing 2^32, so it is >= i at every moment; every other word is a root's idx below its own
// voxel's and is never written after the flatten.
__device__ __forceinline__ bool is_root(uint32_t i, uint32_t p) { return p >= i; }
// the root of voxel i, and the root's word, while roots' words are changing
__device__ __forceinline__ uint32_t root_of(const uint32_t *P, uint32_t i, uint32_t &word) {
  const uint32_t p = parent_peek(&P[i]);
  if (is_root(i, p)) {
    word = p;
    return i;
  }
  word = parent_peek(&P[p]);
  return p;
}

// rows, merge, flatten on `stream`, logged as "<who> rows", "<who> merge", "<who> flatten": the forest of `labels` in P (not the
// labels), the per-chunk root counts of the flatten in `chunks` (components_workspace_bytes).  binary, or dtype EDT_BOOL: every
// non-zero voxel is one class.  1 <= sx * sy * sz <= kCcMaxVoxels.  No numbering: that is launch_components' own.
int launch_forest(int dtype, const void *labels, int64_t sx, int64_t sy, int64_t sz, int connectivity, int binary, uint32_t *P,
                  void *chunks, const char *who, hipStream_t stream);

// The workspace of an operation that keeps a parent plane of its own (fill_holes, dust): the plane, then the chunk counts
inline size_t parent_plane_bytes(int64_t voxels) { return align_up((size_t)std::max<int64_t>(voxels, 1) * sizeof(uint32_t), 256); }
struct ForestWorkspace {
  uint32_t *P;
  void *chunks;
  ForestWorkspace(void *ws, int64_t voxels) : P(static_cast<uint32_t *>(ws)), chunks(static_cast<char *>(ws) + parent_plane_bytes(voxels)) {}
  static size_t bytes(int64_t voxels) { return parent_plane_bytes(voxels) + components_workspace_bytes(voxels); }
};

}  // namespace edt_amd
