// edt_fillholes.hip -- fill_holes: the enclosed cavities of a multi-label volume take the label of their wall
// (include/edt_hip.h, "fill holes", states the contract).
//
// The background's components come from the union-find of edt_components.hip, run over the mask labels == 0
// (launch_forest: k_cc_rows / k_cc_merge / k_cc_flatten of one-byte labels, no numbering).  After it every background
// voxel i holds its component's root in P[i] -- the component's smallest idx -- and a root holds itself.
//
// Room for the state of a component: a root's own word.  It is only ever a self-pointer, and idx < 2^31, so the top bit of every
// parent is clear.  A root's word becomes  kCcTag | (0x7FFFFFFF - s)  with the state s:
//     s = 0        the component is open (touches the array's boundary) or mixed (its wall holds two labels): not filled
//     s = q + 1    q is the smallest idx seen so far of a wall voxel
// and every update is atomicMax of that word: an untagged self-pointer is below every tagged value (the first update replaces
// it), a smaller s is a larger word (the minimum of s survives), and s = 0 is the largest word there is (open and mixed are
// final).  The representative q lies below the root -- the root's x-1 neighbour exists in a cavity and is a wall voxel -- so
// q + 1 <= 2^31 - 2.  A voxel i is a root iff P[i] >= i (itself, or tagged: the root rule of edt_forest.h).
//
// The mask lives in the first sx*sy*sz bytes of the OUTPUT array, which nothing else uses until the last sweep writes it (by then
// the mask is dead), so the workspace is the parent plane alone.
//
//   mask           out-as-bytes[i] = (labels[i] == 0)                                         (k_is_background, edt_generic.hip)
//   rows, merge, flatten   the forest of the mask in P                                        (edt_components.hip)
//   k_fh_mark      every background voxel: on the boundary s = 0, else s = 1 + its smallest foreground neighbour under c
//   k_fh_check<T>  (multi-label only) every voxel of a component that is still closed compares its foreground neighbours'
//                  labels with the representative's: a mismatch (a NaN always is one) sets s = 0
//   k_fh_fill<T>   out = labels; a background voxel whose root has s > 0 takes labels[s - 1]; the filled voxels are counted by a
//                  wave reduction and one 64-bit atomicAdd per workgroup
// Phases are separate launches; no thread waits for another, every loop is bounded by its inputs, and every reduction is an
// integer max or add, so the result does not depend on which thread won an atomic.
#include "edt_forest.h"

namespace edt_amd {
namespace {

constexpr uint32_t kFhDone = 0xFFFFFFFFu;  // s = 0: open or mixed
constexpr uint32_t kFhNone = 0xFFFFFFFFu;  // "this lane has no update" (a root is at most 2^31 - 2)
constexpr int kFhThreads = 256;
constexpr int kFhBlocks = 256 * 8;         // grid of the striding sweeps

__device__ __forceinline__ uint32_t fh_word(uint32_t s) { return kCcTag | (0x7FFFFFFFu - s); }
__device__ __forceinline__ uint32_t fh_state(uint32_t word) { return 0x7FFFFFFFu - (word & 0x7FFFFFFFu); }

struct FhGeom {
  uint32_t voxels, sx, sy, sz;
  int ndim, c;
};

__device__ __forceinline__ bool fh_on_boundary(const FhGeom &g, uint32_t i) {
  const uint32_t row = i / g.sx, x = i - row * g.sx;
  const uint32_t z = row / g.sy, y = row - z * g.sy;
  return x == 0 || x + 1 == g.sx || (g.ndim >= 2 && (y == 0 || y + 1 == g.sy)) || (g.ndim >= 3 && (z == 0 || z + 1 == g.sz));
}

// f(q) for the neighbours q of an INTERIOR voxel i under g.c, in ascending q, until f returns true
template <typename F>
__device__ __forceinline__ void fh_neighbours(const FhGeom &g, uint32_t i, F &&f) {
  const int zr = g.ndim >= 3 ? 1 : 0, yr = g.ndim >= 2 ? 1 : 0;
  const int64_t sx = g.sx, sxy = (int64_t)g.sx * g.sy;
  bool done = false;
  for (int dz = -zr; dz <= zr && !done; ++dz)
    for (int dy = -yr; dy <= yr && !done; ++dy) {
      const int axes = (dz != 0) + (dy != 0);
      if (axes > g.c) continue;
      const int64_t q0 = (int64_t)i + dz * sxy + dy * sx;
      if (axes < g.c) done = f((uint32_t)(q0 - 1));
      if (axes > 0 && !done) done = f((uint32_t)q0);
      if (axes < g.c && !done) done = f((uint32_t)(q0 + 1));
    }
}

// P[r] = max(P[r], word) for the lanes with r != kFhNone; a wave whose lanes all name one root sends one atomic.
// Call with the whole wave converged.
__device__ __forceinline__ void fh_raise(uint32_t *P, uint32_t r, uint32_t word) {
  const bool has = r != kFhNone;
  const uint64_t m = __ballot(has);
  if (m == 0) return;
  const int first = __ffsll((unsigned long long)m) - 1;
  const uint32_t r0 = __shfl(r, first);
  if (__ballot(has && r != r0) == 0) {
    uint32_t best = has ? word : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = max(best, (uint32_t)__shfl_xor(best, off));
    if ((int)(threadIdx.x & 63) == first) atomicMax(&P[r0], best);
  } else if (has) {
    atomicMax(&P[r], word);
  }
}

// ---- open components and the smallest wall voxel --------------------------------------------------------------------------
__global__ __launch_bounds__(kFhThreads) void k_fh_mark(const uint8_t *__restrict__ bg, uint32_t *P, FhGeom g) {
  const uint32_t stride = gridDim.x * kFhThreads;
  // (wave-uniform loop: fh_raise needs every lane; voxels + stride < 2^32)
  for (uint32_t base = blockIdx.x * kFhThreads + (threadIdx.x & ~63u); base < g.voxels; base += stride) {
    const uint32_t i = base + (threadIdx.x & 63);
    uint32_t r = kFhNone, word = 0;
    if (i < g.voxels && bg[i]) {
      uint32_t cur;
      const uint32_t root = root_of(P, i, cur);
      if (cur != kFhDone) {
        if (fh_on_boundary(g, i)) {
          word = kFhDone;
        } else {
          fh_neighbours(g, i, [&](uint32_t q) {
            if (bg[q]) return false;
            word = fh_word(q + 1);
            return true;
          });
        }
        if (word > cur) r = root;  // (an untagged self-pointer is below every word; word == 0: no foreground neighbour)
      }
    }
    fh_raise(P, r, word);
  }
}

// ---- one label all around? ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kFhThreads) void k_fh_check(const T *__restrict__ labels, const uint8_t *__restrict__ bg, uint32_t *P,
                                                         FhGeom g) {
  const uint32_t stride = gridDim.x * kFhThreads;
  for (uint32_t base = blockIdx.x * kFhThreads + (threadIdx.x & ~63u); base < g.voxels; base += stride) {
    const uint32_t i = base + (threadIdx.x & 63);
    uint32_t r = kFhNone;
    if (i < g.voxels && bg[i]) {
      uint32_t cur;
      const uint32_t root = root_of(P, i, cur);
      if ((cur & kCcTag) && cur != kFhDone) {  // still closed, so i is interior: every neighbour exists
        const T ref = labels[fh_state(cur) - 1];
        fh_neighbours(g, i, [&](uint32_t q) {
          if (bg[q] || labels[q] == ref) return false;
          r = root;
          return true;
        });
      }
    }
    fh_raise(P, r, kFhDone);
  }
}

// ---- the fill -------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kFhThreads) void k_fh_fill(const T *__restrict__ labels, const uint32_t *__restrict__ P,
                                                        T *__restrict__ out, uint32_t voxels, unsigned long long *n_filled) {
  __shared__ uint32_t s_count[kFhThreads / 64];
  const uint32_t stride = gridDim.x * kFhThreads;
  uint32_t filled = 0;  // (a thread fills fewer than 2^31 voxels)
  for (uint32_t i = blockIdx.x * kFhThreads + threadIdx.x; i < voxels; i += stride) {
    T v = labels[i];
    if (!label_fg(v)) {
      const uint32_t p = P[i];
      const uint32_t word = is_root(i, p) ? p : P[p];
      if ((word & kCcTag) && word != kFhDone) {
        v = labels[fh_state(word) - 1];
        ++filled;
      }
    }
    out[i] = v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) filled += __shfl_xor(filled, off);  // (not wave_sum: the kernel's code would change)
  if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6] = filled;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long c = 0;
    for (int w = 0; w < kFhThreads / 64; ++w) c += s_count[w];
    if (c) atomicAdd(n_filled, c);
  }
}

int launch_fill_holes(int dtype, const void *labels, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity, int binary,
                      void *out, int64_t *n_filled, void *ws, hipStream_t stream) {
  const int64_t voxels = sx * sy * sz;
  const ForestWorkspace w(ws, voxels);
  uint32_t *P = w.P;
  uint8_t *bg = static_cast<uint8_t *>(out);
  int rc;
  {
    ScopedPass sp("fill_holes mask", stream);
    if ((rc = launch_fill_words(n_filled, 0u, sizeof(int64_t) / sizeof(uint32_t), stream)) != EDT_OK) return rc;
    if ((rc = launch_is_background(dtype, labels, bg, voxels, stream)) != EDT_OK) return rc;
  }
  if ((rc = launch_forest(EDT_U8, bg, sx, sy, sz, connectivity, 1, P, w.chunks, "fill_holes", stream)) != EDT_OK) return rc;
  const FhGeom g{(uint32_t)voxels, (uint32_t)sx, (uint32_t)sy, (uint32_t)sz, ndim, connectivity};
  const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(voxels, kFhThreads), kFhBlocks * 4);
  {
    ScopedPass sp("fill_holes mark", stream);
    hipLaunchKernelGGL(k_fh_mark, dim3(blocks), dim3(kFhThreads), 0, stream, bg, P, g);
    EDT_HIP_TRY(hipGetLastError());
  }
  return with_label_type(dtype, [&](auto t) -> int {
    using T = typename decltype(t)::type;
    if (!binary && dtype != EDT_BOOL) {
      ScopedPass sp("fill_holes check", stream);
      hipLaunchKernelGGL(k_fh_check<T>, dim3(blocks), dim3(kFhThreads), 0, stream, (const T *)labels, bg, P, g);
      EDT_HIP_TRY(hipGetLastError());
    }
    ScopedPass sp("fill_holes fill", stream);
    hipLaunchKernelGGL(k_fh_fill<T>, dim3(blocks), dim3(kFhThreads), 0, stream, (const T *)labels, P, (T *)out, g.voxels,
                       (unsigned long long *)n_filled);
    EDT_HIP_TRY(hipGetLastError());
    return EDT_OK;
  });
}

}  // namespace
}  // namespace edt_amd

using namespace edt_amd;

extern "C" {

size_t edt_hip_fill_holes_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz) {
  const size_t chunks = edt_hip_components_workspace_bytes(dtype, ndim, sx, sy, sz);  // (0: a bad dtype or shape, or past the limit)
  return chunks == 0 ? 0 : ForestWorkspace::bytes(sx * sy * sz);
}

int edt_hip_fill_holes_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity,
                              int binary, void *d_out, int64_t *d_n_filled, void *d_workspace, size_t workspace_bytes,
                              void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int own = components_check_args(dtype, ndim, sx, sy, sz, connectivity, "fill_holes");
  const int64_t voxels = own == EDT_OK ? sx * sy * sz : 0;
  int rc;
  if (!label_op_begin("fill_holes", own, d_n_filled, 1, voxels, !d_labels || !d_out,
                      d_labels == d_out, d_workspace, workspace_bytes,
                      ForestWorkspace::bytes(voxels), "edt_hip_fill_holes_workspace_bytes", stream, &rc))
    return rc;
  return launch_fill_holes(dtype, d_labels, ndim, sx, sy, sz, connectivity, binary, d_out, d_n_filled, d_workspace, stream);
}

}  // extern "C"
