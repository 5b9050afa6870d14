// edt_forest.h -- what the label operations share: connected_components (edt_components.hip), fill_holes (edt_fillholes.hip)
// and dust (edt_dust.hip) all stand on one union-find parent plane P.  launch_forest builds it: P[i] = the smallest idx of i's
// component -- its ROOT -- for a foreground voxel, a root holds itself, background holds kCcBg.  What an operation then keeps
// per component (a number, a cavity's state, a size) goes into the root's own word, under kCcTag.  watershed (edt_watershed.hip)
// builds a forest of its own on such a plane, with cc_union, and has it flattened and numbered here.  Internal: nothing is exported.
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

namespace {
// the root above i of a parent plane under construction (P[j] <= j, a root holds itself): strictly downhill (P[j] <= j), so at most i steps
__device__ __forceinline__ uint32_t cc_find(uint32_t *P, uint32_t i) {
  const uint32_t from = i;
  int steps = 0;
  for (;;) {
    const uint32_t p = parent_peek(&P[i]);
    if (p >= i) break;  // a root (p == i); p > i cannot be (background is never walked)
    i = p;
    ++steps;
  }
  if (steps > 2) atomicMin(&P[from], i);  // i is an ancestor of `from`: the old parent keeps its own path to it
  return i;
}

__device__ void cc_union(uint32_t *P, uint32_t a, uint32_t b) {
  a = cc_find(P, a);
  b = cc_find(P, b);
  while (a != b) {  // a + b strictly decreases
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicMin(&P[a], b);
    if (old == a) break;
    a = old;
  }
}
}  // namespace

// rows, merge, flatten on `stream`, logged as "<who> rows", "<who> merge", "<who> flatten": the forest of `labels` in P (not the
// labels), the per-chunk root counts of the flatten in `chunks` (components_workspace_bytes).  binary, or dtype EDT_BOOL: every
// non-zero voxel is one class.  1 <= sx * sy * sz <= kCcMaxVoxels.  No numbering: that is launch_components' own.
int launch_forest(int dtype, const void *labels, int64_t sx, int64_t sy, int64_t sz, int connectivity, int binary, uint32_t *P,
                  void *chunks, const char *who, hipStream_t stream);
// The two halves of that sequence an operation with unions of its own (watershed) runs by itself.  flatten, logged as `name`:
// P[i] = root(i), and the roots of every 2048-voxel chunk counted into `chunks`; it may run again after further unions.
int launch_forest_flatten(uint32_t *P, int64_t voxels, void *chunks, const char *name, hipStream_t stream);
// number and final, logged as "<who> number", "<who> final", on a plane and the chunk counts as the flatten left them: out[i] = 0
// for background, else 1..N in ascending order of the roots; N to *n (device).  connected_components' numbering, for all.
int launch_forest_number(uint32_t *out, int64_t voxels, void *chunks, int64_t *n, const char *who, hipStream_t stream);

// The workspace of an operation that keeps a parent plane of its own (fill_holes, dust): the plane, then the chunk counts
inline size_t parent_plane_bytes(int64_t voxels) { return align_up((size_t)std::max<int64_t>(voxels, 1) * sizeof(uint32_t), 256); }
struct ForestWorkspace {
  uint32_t *P;
  void *chunks;
  ForestWorkspace(void *ws, int64_t voxels) : P(static_cast<uint32_t *>(ws)), chunks(static_cast<char *>(ws) + parent_plane_bytes(voxels)) {}
  static size_t bytes(int64_t voxels) { return parent_plane_bytes(voxels) + components_workspace_bytes(voxels); }
};

}  // namespace edt_amd
