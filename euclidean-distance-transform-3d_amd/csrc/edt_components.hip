// edt_components.hip -- connected_components: multi-label component labelling of device-resident data by a run-based
// union-find (include/edt_hip.h, "connected components", states the contract).
//
// The output array doubles as the PARENT array P of the union-find forest: P[i] <= i always, a root has P[i] == i, background
// holds the sentinel kCcBg.  The root of a component is its smallest idx, so the forest's final shape -- and with it the
// numbering -- does not depend on which thread won an atomic.  Phases are separate launches (everything is coherent at a
// kernel boundary); no thread ever waits for another, and every loop walks strictly downhill in idx.
//
//   k_cc_rows     P[i] = idx of the first voxel of i's x-run.  A wave takes 4 x 64 consecutive voxels per step; run starts come
//                 from a neighbour compare and a ballot, the start's lane from the ballot's highest set bit at or below the
//                 lane; a run that crosses a 64-voxel group keeps its parent through a carry.  x-adjacency costs no atomic.
//                 Runs are cut at the step's first voxel (idx % 256 == 0): k_cc_merge re-joins the cut.
//   k_cc_merge    every foreground voxel p looks at the PRECEDING neighbour rows only: (y-1, z), (y, z-1) -- dilated to
//                 x-1..x+1 for connectivity >= 2 -- and, in 3-D for connectivity >= 2, (y-1, z-1), (y+1, z-1) -- dilated for
//                 connectivity 3.  With L = "p-1 is connected to p" and m(i) = "voxel i of the other row is connected to p":
//                   not dilated:  union(p, x)    if m(x) and not (L and m(x-1))          [p-1 met the same run at x-1]
//                   dilated, L:   union(p, x+1)  if m(x+1) and not m(x)                  [p-1 is adjacent to x-1 and x, and
//                                                                                         x+1 continues x's run]
//                   dilated, !L:  union(p, x) if m(x), else union(p, x-1) if m(x-1) and union(p, x+1) if m(x+1)
//                 so a union is issued by the first voxel of an overlap only.  Union: find both roots, then
//                 old = atomicMin(&P[larger], smaller) until old == larger, continuing with old in place of larger: parents only
//                 decrease, every returned value is true, and a link that a racing atomicMin overwrote is re-established by
//                 the continuation.  find reads with relaxed agent-scope loads (a stale read is an older ancestor: an extra
//                 iteration, never a wrong result) and shortens a path of more than two links by an atomicMin, never by a store.
//   k_cc_flatten  P[i] = root(i), and the number of roots of every 2048-voxel chunk
//   k_cc_scan     exclusive scan of the chunk counts (one workgroup, 1024 chunks per round); the total is *d_n
//   k_cc_number   root i of rank k (0-based, ascending idx) gets P[i] = kCcTag | k
//   k_cc_final    out[i] = 0 for background, else the number of its root: (P[root] & ~kCcTag) + 1.  A root's own word is
//                 either still tagged or already its number; the top bit tells, so the sweep needs no second plane -- and
//                 this is why a volume has at most 2^31 - 1 voxels.
#include <type_traits>

#include "edt_forest.h"

namespace edt_amd {
namespace {

// (kCcBg, kCcTag, kCcMaxVoxels, label_fg, label_conn, parent_peek, wave_sum: edt_forest.h)
constexpr int kCcThreads = 256;
constexpr int kCcGroups = 4;                      // 64-voxel groups per wave and step (256-byte loads of 4-byte labels)
constexpr int kCcTile = 64 * kCcGroups;
constexpr int kCcBlocks = 256 * 8;                // grid of the striding sweeps
constexpr int kCcChunk = 2048;                    // voxels per workgroup of the numbering kernels
constexpr int kCcScan = 1024;                     // chunks per round of the scan

// the label of lane `src` / of the lane below, at any width
template <typename T> __device__ __forceinline__ T cc_shfl(T v, int src) {
  using B = std::conditional_t<sizeof(T) == 8, unsigned long long, unsigned int>;
  B b = 0;
  __builtin_memcpy(&b, &v, sizeof(T));
  b = __shfl(b, src);
  __builtin_memcpy(&v, &b, sizeof(T));
  return v;
}
template <typename T> __device__ __forceinline__ T cc_shfl_up1(T v) {
  using B = std::conditional_t<sizeof(T) == 8, unsigned long long, unsigned int>;
  B b = 0;
  __builtin_memcpy(&b, &v, sizeof(T));
  b = __shfl_up(b, 1);
  __builtin_memcpy(&v, &b, sizeof(T));
  return v;
}

// (cc_find, cc_union: edt_forest.h)

// ---- phase 1: x-runs ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kCcThreads) void k_cc_rows(const T *__restrict__ labels, uint32_t *__restrict__ P, uint32_t voxels,
                                                        uint32_t sx, int binary) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t ntiles = (voxels + kCcTile - 1) / kCcTile;
  for (uint32_t tile = blockIdx.x * (kCcThreads / 64) + wave; tile < ntiles; tile += gridDim.x * (kCcThreads / 64)) {
    const uint32_t base = tile * kCcTile;
    T v[kCcGroups];
#pragma unroll
    for (int j = 0; j < kCcGroups; ++j) {
      const uint32_t idx = base + j * 64 + lane;
      v[j] = idx < voxels ? labels[idx] : (T)0;
    }
    uint32_t carry = kCcBg;  // the parent of the previous group's last lane
#pragma unroll
    for (int j = 0; j < kCcGroups; ++j) {
      const uint32_t idx = base + j * 64 + lane;
      const uint32_t x = idx % sx;
      T pv = cc_shfl_up1(v[j]);
      if (j > 0) {
        const T last = cc_shfl(v[j - 1], 63);
        if (lane == 0) pv = last;
      }
      const bool cont = x != 0 && !(j == 0 && lane == 0) && label_conn(pv, v[j], binary);
      const uint64_t m = __ballot(!cont);
      const uint64_t below = m & ((2ull << lane) - 1ull);
      const uint32_t par = below ? base + j * 64 + (uint32_t)(63 - __builtin_clzll(below)) : carry;
      if (idx < voxels) P[idx] = label_fg(v[j]) ? par : kCcBg;
      carry = __shfl(par, 63);
    }
  }
}

// ---- phase 2: unions with the preceding rows ------------------------------------------------------------------------------
// q0: the voxel of the other row at p's x
template <typename T>
__device__ __forceinline__ void cc_visit(const T *__restrict__ labels, uint32_t *P, T v, uint32_t p, uint32_t q0, uint32_t x,
                                         uint32_t sx, bool L, bool dilate, int binary) {
  const bool mc = label_conn(v, labels[q0], binary);
  if (!dilate) {
    if (mc && !(L && label_conn(v, labels[q0 - 1], binary))) cc_union(P, p, q0);  // (L: x > 0)
    return;
  }
  const bool mr = x + 1 < sx && label_conn(v, labels[q0 + 1], binary);
  if (L) {
    if (mr && !mc) cc_union(P, p, q0 + 1);
    return;
  }
  if (mc) {
    cc_union(P, p, q0);
    return;
  }
  if (x > 0 && label_conn(v, labels[q0 - 1], binary)) cc_union(P, p, q0 - 1);
  if (mr) cc_union(P, p, q0 + 1);
}

template <typename T>
__global__ __launch_bounds__(kCcThreads) void k_cc_merge(const T *__restrict__ labels, uint32_t *P, uint32_t voxels, uint32_t sx,
                                                         uint32_t sy, int connectivity, int binary) {
  const uint32_t sxy = sx * sy;
  const bool near_dilate = connectivity >= 2, diag = connectivity >= 2, diag_dilate = connectivity >= 3;
  const uint32_t stride = gridDim.x * kCcThreads;
  for (uint32_t p = blockIdx.x * kCcThreads + threadIdx.x; p < voxels; p += stride) {  // (voxels + stride < 2^32)
    const T v = labels[p];
    if (!label_fg(v)) continue;
    const uint32_t row = p / sx, x = p - row * sx;
    const uint32_t z = row / sy, y = row - z * sy;
    const bool L = x > 0 && label_conn(labels[p - 1], v, binary);
    if (L && (p % kCcTile) == 0) cc_union(P, p, p - 1);  // the cut of k_cc_rows
    if (y > 0) cc_visit(labels, P, v, p, p - sx, x, sx, L, near_dilate, binary);
    if (z > 0) {
      cc_visit(labels, P, v, p, p - sxy, x, sx, L, near_dilate, binary);
      if (diag) {
        if (y > 0) cc_visit(labels, P, v, p, p - sxy - sx, x, sx, L, diag_dilate, binary);
        if (y + 1 < sy) cc_visit(labels, P, v, p, p - sxy + sx, x, sx, L, diag_dilate, binary);
      }
    }
  }
}

// ---- phase 3: every voxel to its root, roots counted per chunk ----------------------------------------------------------------
__global__ __launch_bounds__(kCcThreads) void k_cc_flatten(uint32_t *P, uint32_t voxels, uint32_t *__restrict__ chunk_count) {
  __shared__ uint32_t s_count[kCcThreads / 64];
  const uint32_t base = blockIdx.x * (uint32_t)kCcChunk;
  uint32_t roots = 0;
  for (int k = 0; k < kCcChunk / kCcThreads; ++k) {
    const uint32_t i = base + k * kCcThreads + threadIdx.x;
    if (i >= voxels) continue;
    const uint32_t p = parent_peek(&P[i]);
    if (p == kCcBg) continue;
    uint32_t r = p;
    if (p != i)
      for (;;) {  // strictly downhill
        const uint32_t n = parent_peek(&P[r]);
        if (n >= r) break;
        r = n;
      }
    if (r != p) P[i] = r;
    roots += r == i;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) roots += __shfl_xor(roots, off);  // (not wave_sum: the kernel's code would change)
  if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6] = roots;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t c = 0;
    for (int w = 0; w < kCcThreads / 64; ++w) c += s_count[w];
    chunk_count[blockIdx.x] = c;
  }
}

// ---- phase 4: numbers --------------------------------------------------------------------------------------------------
// exclusive prefix sum over the chunks, in place; the total goes to *total (32-bit sibling of k_runs_scan, edt_line.hip)
__global__ __launch_bounds__(kCcScan) void k_cc_scan(uint32_t *chunk, uint32_t nchunks, int64_t *total) {
  __shared__ uint32_t s_wave[kCcScan / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nchunks; base += kCcScan) {
    const uint32_t b = base + threadIdx.x;
    const uint32_t v = b < nchunks ? chunk[b] : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t u = __shfl_up(incl, off);
      if (lane >= off) incl += u;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
    for (int w = 0; w < kCcScan / 64; ++w) {
      const uint32_t c = s_wave[w];
      if (w < wave) before += c;
      sum += c;
    }
    __syncthreads();
    if (b < nchunks) chunk[b] = carry + before + incl - v;
    carry += sum;
  }
  if (threadIdx.x == 0) *total = (int64_t)carry;
}

__global__ __launch_bounds__(kCcThreads) void k_cc_number(uint32_t *P, uint32_t voxels, const uint32_t *__restrict__ chunk_off) {
  __shared__ uint32_t s_count[kCcThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t base = blockIdx.x * (uint32_t)kCcChunk;
  uint32_t rank = chunk_off[blockIdx.x];
  for (int k = 0; k < kCcChunk / kCcThreads; ++k) {  // (uniform: every thread meets both barriers)
    const uint32_t i = base + k * kCcThreads + threadIdx.x;
    const bool root = i < voxels && P[i] == i;
    const uint64_t m = __ballot(root);
    if (lane == 0) s_count[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, sum = 0;
    for (int w = 0; w < kCcThreads / 64; ++w) {
      const uint32_t c = s_count[w];
      if (w < wave) before += c;
      sum += c;
    }
    __syncthreads();
    if (root) P[i] = kCcTag | (rank + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
    rank += sum;
  }
}

__global__ __launch_bounds__(kCcThreads) void k_cc_final(uint32_t *P, uint32_t voxels) {
  const uint32_t i = blockIdx.x * (uint32_t)kCcThreads + threadIdx.x;
  if (i >= voxels) return;
  uint32_t p = P[i];
  if (p == kCcBg) {
    P[i] = 0u;
    return;
  }
  if (!(p & kCcTag)) p = parent_peek(&P[p]);  // the root's word: tagged rank, or (its own thread was here) already its number
  P[i] = (p & kCcTag) ? (p & ~kCcTag) + 1u : p;
}

}  // namespace

size_t components_workspace_bytes(int64_t voxels) {
  return align_up((size_t)ceil_div(std::max<int64_t>(voxels, 1), kCcChunk) * sizeof(uint32_t), 256);
}

// (contracts of the three launchers: edt_forest.h)
int launch_forest(int dtype, const void *labels, int64_t sx, int64_t sy, int64_t sz, int connectivity, int binary, uint32_t *P,
                  void *chunks, const char *who, hipStream_t stream) {
  const int64_t voxels64 = sx * sy * sz;
  if (voxels64 < 1 || voxels64 > kCcMaxVoxels) { set_error(std::string(who) + ": volume out of range"); return EDT_ERR_UNSUPPORTED; }
  const uint32_t voxels = (uint32_t)voxels64;
  const int bin = (binary || dtype == EDT_BOOL) ? 1 : 0;
  char rows[40], merge[40], flatten[40];  // (on the stack: the pass log copies the names it keeps)
  snprintf(rows, sizeof rows, "%s rows", who);
  snprintf(merge, sizeof merge, "%s merge", who);
  snprintf(flatten, sizeof flatten, "%s flatten", who);
  return with_label_type(dtype, [&](auto t) -> int {
    using T = typename decltype(t)::type;
    const int waves = kCcThreads / 64;
    {
      ScopedPass sp(rows, stream);
      const int64_t blocks = std::min<int64_t>(ceil_div(ceil_div(voxels64, kCcTile), waves), kCcBlocks);
      hipLaunchKernelGGL(k_cc_rows<T>, dim3((unsigned)blocks), dim3(kCcThreads), 0, stream, (const T *)labels, P, voxels,
                         (uint32_t)sx, bin);
      EDT_HIP_TRY(hipGetLastError());
    }
    {
      ScopedPass sp(merge, stream);
      const int64_t blocks = std::min<int64_t>(ceil_div(voxels64, kCcThreads), kCcBlocks * 4);
      hipLaunchKernelGGL(k_cc_merge<T>, dim3((unsigned)blocks), dim3(kCcThreads), 0, stream, (const T *)labels, P, voxels,
                         (uint32_t)sx, (uint32_t)sy, connectivity, bin);
      EDT_HIP_TRY(hipGetLastError());
    }
    return launch_forest_flatten(P, voxels64, chunks, flatten, stream);
  });
}

int launch_forest_flatten(uint32_t *P, int64_t voxels64, void *chunks, const char *name, hipStream_t stream) {
  ScopedPass sp(name, stream);
  hipLaunchKernelGGL(k_cc_flatten, dim3((unsigned)ceil_div(voxels64, kCcChunk)), dim3(kCcThreads), 0, stream, P, (uint32_t)voxels64,
                     static_cast<uint32_t *>(chunks));
  EDT_HIP_TRY(hipGetLastError());
  return EDT_OK;
}

int launch_forest_number(uint32_t *out, int64_t voxels64, void *chunks, int64_t *n, const char *who, hipStream_t stream) {
  const uint32_t voxels = (uint32_t)voxels64;
  uint32_t *chunk = static_cast<uint32_t *>(chunks);
  const uint32_t nchunks = (uint32_t)ceil_div(voxels64, kCcChunk);
  char number[40], final[40];
  snprintf(number, sizeof number, "%s number", who);
  snprintf(final, sizeof final, "%s final", who);
  {
    ScopedPass sp(number, stream);
    hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(kCcScan), 0, stream, chunk, nchunks, n);
    EDT_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cc_number, dim3(nchunks), dim3(kCcThreads), 0, stream, out, voxels, chunk);
    EDT_HIP_TRY(hipGetLastError());
  }
  {
    ScopedPass sp(final, stream);
    hipLaunchKernelGGL(k_cc_final, dim3((unsigned)ceil_div(voxels64, kCcThreads)), dim3(kCcThreads), 0, stream, out, voxels);
    EDT_HIP_TRY(hipGetLastError());
  }
  return EDT_OK;
}

int launch_components(int dtype, const void *labels, int64_t sx, int64_t sy, int64_t sz, int connectivity, int binary,
                      uint32_t *out, int64_t *n, void *ws, hipStream_t stream) {
  const int rc = launch_forest(dtype, labels, sx, sy, sz, connectivity, binary, out, ws, "components", stream);
  if (rc != EDT_OK) return rc;
  return launch_forest_number(out, sx * sy * sz, ws, n, "components", stream);
}

// sx * sy * sz <= 2^31 - 1, in 64-bit arithmetic (extents are at most 2^31 - 1 each: check_shape)
static bool cc_volume_fits(int64_t sx, int64_t sy, int64_t sz) {
  if (sx == 0 || sy == 0 || sz == 0) return true;
  if (sx > kCcMaxVoxels / sy) return false;
  return sx * sy <= kCcMaxVoxels / sz;
}

// shape, then the call's own arguments: what both entry points refuse before they look at a pointer (who: the caller's name in
// the message -- fill_holes refuses the same things in the same order)
int components_check_args(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity, const char *who) {
  const int rc = check_shape(dtype, ndim, sx, sy, sz);
  if (rc != EDT_OK) return rc;
  if (connectivity < 1 || connectivity > ndim) { set_error(std::string(who) + ": connectivity must be in 1..ndim"); return EDT_ERR_BAD_ARG; }
  if (!cc_volume_fits(sx, sy, sz)) {
    set_error(std::string(who) + ": more than 2^31 - 1 voxels (parents and numbers are 32-bit)");
    return EDT_ERR_UNSUPPORTED;
  }
  return EDT_OK;
}

}  // namespace edt_amd

using namespace edt_amd;

extern "C" {

size_t edt_hip_components_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz) {
  if (dtype_size(dtype) == 0 || ndim < 1 || ndim > 3 || sx < 0 || sy < 0 || sz < 0 || (ndim < 3 && sz != 1) ||
      (ndim < 2 && sy != 1) || sx > INT32_MAX || sy > INT32_MAX || sz > INT32_MAX || !cc_volume_fits(sx, sy, sz))
    return 0;
  return components_workspace_bytes(sx * sy * sz);
}

int edt_hip_connected_components_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz,
                                        int connectivity, int binary, uint32_t *d_out, int64_t *d_n, void *d_workspace,
                                        size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int own = components_check_args(dtype, ndim, sx, sy, sz, connectivity);
  const int64_t voxels = own == EDT_OK ? sx * sy * sz : 0;
  int rc;
  if (!label_op_begin("connected_components", own, d_n, 1, voxels, !d_labels || !d_out, false, d_workspace, workspace_bytes,
                      components_workspace_bytes(voxels), "edt_hip_components_workspace_bytes", stream, &rc))
    return rc;
  return launch_components(dtype, d_labels, sx, sy, sz, connectivity, binary, d_out, d_n, d_workspace, stream);
}

}  // extern "C"

// The label types in the order in which their kernels stand in the code object -- one-byte labels last, as measured in
// DESIGN 10-12.  Left to the order of first use they would come first and every other instantiation sit two kernels further on,
// and a kernel that moves is timed anew although no instruction of it changed.  Nothing but this list holds the order: a first
// use of k_cc_rows<T> or k_cc_merge<T> above it reorders them again.  To re-check after a change to this unit, compile it with
// the Makefile's flags plus  -S --cuda-device-only  at this commit and at the previous one and diff the two files: only the
// __hip_cuid lines may differ.
namespace edt_amd {
namespace {
#define EDT_CC_KERNELS(T)                                                                \
  template __global__ void k_cc_rows<T>(const T *, uint32_t *, uint32_t, uint32_t, int); \
  template __global__ void k_cc_merge<T>(const T *, uint32_t *, uint32_t, uint32_t, uint32_t, int, int);
EDT_CC_KERNELS(uint16_t) EDT_CC_KERNELS(uint32_t) EDT_CC_KERNELS(uint64_t) EDT_CC_KERNELS(float) EDT_CC_KERNELS(double) EDT_CC_KERNELS(uint8_t)
#undef EDT_CC_KERNELS
}  // namespace
}  // namespace edt_amd
