// edt_watershed.hip -- watershed: every label is split into the basins of a float32 field by steepest ascent, stated as the
// connected components of a graph (include/edt_hip.h, "watershed", states the contract; DESIGN.md 20 the reasons).
//
// The output array is the parent plane P of the union-find forest of edt_forest.h, as in connected_components; the one plane
// of the workspace holds the basins' peaks.  Phases are separate launches, no thread waits for another, every loop either walks
// a fixed stencil or walks P strictly downhill in idx (cc_find, cc_union), whatever the field holds.
//
//   k_ws_init     P[i] = i for foreground, kCcBg for background
//   k_ws_ascend   phase 1.  Voxel p reads the labels and the field of its up to 26 neighbours (plain cached loads: DESIGN 20).
//                 M = the greatest field value among the neighbours of one object with p, attained first -- in ascending idx --
//                 at q.  M > f(p): union(p, q).  Otherwise p is a TOP voxel: union(p, u) for every such neighbour u with
//                 f(u) == f(p).  With a peak plane (min_saliency > 0) a top voxel leaves the order-preserving image of f(p) in
//                 its own word of it, every other foreground voxel 0.
//   flatten       (edt_components.hip) P[i] = root(i): the phase-1 basins
//   k_ws_peaks    a top voxel that is not its basin's root raises the root's word of the peak plane to its own (atomicMax of
//                 uint32 images; a word already as high is left alone).  The greatest voxel of a basin is a top voxel.
//   k_ws_spread   peak[i] = peak[root(i)], in place: only roots' words are read, and a root writes nothing
//   k_ws_merge    phase 2.  Voxel p against its PRECEDING neighbours q of one object: union(p, q) iff
//                 min(f(p), f(q)) >= min(peak[p], peak[q]) - h, in float32 with one subtraction.  Nothing it evaluates depends on
//                 a union made: the peaks are those of phase 1.  A pair within one basin passes or not, and changes nothing.
//   flatten, number, final   (edt_components.hip) the numbering of connected_components
#include <cmath>

#include "edt_forest.h"

namespace edt_amd {
namespace {

constexpr int kWsThreads = 256;
constexpr int kWsBlocks = 256 * 32;  // grid of the striding sweeps

// float32 bits <-> uint32 in the order of the floats (-0.0 below +0.0; the least image, 0, is a negative NaN's)
__device__ __forceinline__ uint32_t ws_image(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ws_value(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

template <typename T>
__global__ __launch_bounds__(kWsThreads) void k_ws_init(const T *__restrict__ labels, uint32_t *__restrict__ P, uint32_t voxels) {
  const uint32_t stride = gridDim.x * kWsThreads;
  for (uint32_t p = blockIdx.x * kWsThreads + threadIdx.x; p < voxels; p += stride) P[p] = label_fg(labels[p]) ? p : kCcBg;
}

// the stencil of voxel (x, y, z): visit(k, q) for every neighbour q inside the volume under `connectivity`, k = 0..26 its place in
// the 3 x 3 x 3 block, in ascending idx; `upto`: 13 for the preceding neighbours only, 27 for all
template <typename Visit>
__device__ __forceinline__ void ws_stencil(uint32_t p, uint32_t x, uint32_t y, uint32_t z, uint32_t sx, uint32_t sy, uint32_t sz,
                                           int connectivity, int upto, Visit &&visit) {
  const uint32_t sxy = sx * sy;
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    if (k >= upto) break;
    const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
    const int axes = (dx != 0) + (dy != 0) + (dz != 0);
    if (axes == 0 || axes > connectivity) continue;
    if ((dx < 0 && x == 0) || (dx > 0 && x + 1 >= sx) || (dy < 0 && y == 0) || (dy > 0 && y + 1 >= sy) || (dz < 0 && z == 0) ||
        (dz > 0 && z + 1 >= sz))
      continue;
    visit(k, p + (uint32_t)(dz * (int)sxy + dy * (int)sx + dx));  // (inside the volume: below 2^31)
  }
}

template <typename T>
__global__ __launch_bounds__(kWsThreads) void k_ws_ascend(const T *__restrict__ labels, const float *__restrict__ field, uint32_t *P,
                                                          uint32_t *__restrict__ peak, uint32_t voxels, uint32_t sx, uint32_t sy,
                                                          uint32_t sz, int connectivity, int binary) {
  const uint32_t stride = gridDim.x * kWsThreads;
  for (uint32_t p = blockIdx.x * kWsThreads + threadIdx.x; p < voxels; p += stride) {  // (voxels + stride < 2^32)
    const T v = labels[p];
    if (!label_fg(v)) continue;
    const uint32_t row = p / sx, x = p - row * sx;
    const uint32_t z = row / sy, y = row - z * sy;
    const float fv = field[p];
    float best = 0.0f;
    uint32_t arg = kCcBg, equal = 0;  // equal: bit k, the neighbour at k is of one object with p and its value == f(p)
    ws_stencil(p, x, y, z, sx, sy, sz, connectivity, 27, [&](int k, uint32_t q) {
      if (!label_conn(v, labels[q], binary)) return;
      const float fu = field[q];
      if (arg == kCcBg || fu > best) {
        best = fu;
        arg = q;
      }
      if (fu == fv) equal |= 1u << k;
    });
    const bool top = !(arg != kCcBg && best > fv);
    if (peak) peak[p] = top ? ws_image(fv) : 0u;
    if (!top) {
      cc_union(P, p, arg);
      continue;
    }
    const uint32_t sxy = sx * sy;
    while (equal) {
      const int k = __builtin_ctz(equal);
      equal &= equal - 1;
      const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
      cc_union(P, p, p + (uint32_t)(dz * (int)sxy + dy * (int)sx + dx));
    }
  }
}

__global__ __launch_bounds__(kWsThreads) void k_ws_peaks(const uint32_t *__restrict__ P, uint32_t *peak, uint32_t voxels) {
  const uint32_t stride = gridDim.x * kWsThreads;
  for (uint32_t i = blockIdx.x * kWsThreads + threadIdx.x; i < voxels; i += stride) {
    const uint32_t r = P[i];
    if (r >= i) continue;  // background, or a root: its own image is in its word already
    const uint32_t mine = peak[i];  // (a word that is no root's: nobody writes it in this launch)
    if (mine != 0u && parent_peek(&peak[r]) < mine) atomicMax(&peak[r], mine);
  }
}

__global__ __launch_bounds__(kWsThreads) void k_ws_spread(const uint32_t *__restrict__ P, uint32_t *peak, uint32_t voxels) {
  const uint32_t stride = gridDim.x * kWsThreads;
  for (uint32_t i = blockIdx.x * kWsThreads + threadIdx.x; i < voxels; i += stride) {
    const uint32_t r = P[i];
    if (r < i) peak[i] = peak[r];
  }
}

template <typename T>
__global__ __launch_bounds__(kWsThreads) void k_ws_merge(const T *__restrict__ labels, const float *__restrict__ field, uint32_t *P,
                                                         const uint32_t *__restrict__ peak, uint32_t voxels, uint32_t sx, uint32_t sy,
                                                         uint32_t sz, int connectivity, int binary, float h) {
  const uint32_t stride = gridDim.x * kWsThreads;
  for (uint32_t p = blockIdx.x * kWsThreads + threadIdx.x; p < voxels; p += stride) {
    const T v = labels[p];
    if (!label_fg(v)) continue;
    const uint32_t row = p / sx, x = p - row * sx;
    const uint32_t z = row / sy, y = row - z * sy;
    const float fv = field[p], pv = ws_value(peak[p]);
    ws_stencil(p, x, y, z, sx, sy, sz, connectivity, 13, [&](int, uint32_t q) {
      if (!label_conn(v, labels[q], binary)) return;
      const float bar = fminf(pv, ws_value(peak[q])) - h;
      if (fminf(fv, field[q]) >= bar) cc_union(P, p, q);
    });
  }
}

}  // namespace

// what components_check_args refuses, then min_saliency negative or not finite
int watershed_check_args(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity, float min_saliency) {
  const int rc = components_check_args(dtype, ndim, sx, sy, sz, connectivity, "watershed");
  if (rc != EDT_OK) return rc;
  if (!(min_saliency >= 0.0f) || !std::isfinite(min_saliency)) { set_error("watershed: min_saliency must be finite and >= 0"); return EDT_ERR_BAD_ARG; }
  return EDT_OK;
}

// ws: ForestWorkspace, its plane the peaks'.  1 <= sx * sy * sz <= kCcMaxVoxels.
int launch_watershed(int dtype, const void *labels, int64_t sx, int64_t sy, int64_t sz, const float *field, int connectivity,
                     int binary, float h, uint32_t *out, int64_t *n, void *ws, hipStream_t stream) {
  const int64_t voxels64 = sx * sy * sz;
  const uint32_t voxels = (uint32_t)voxels64;
  const int bin = (binary || dtype == EDT_BOOL) ? 1 : 0;
  const ForestWorkspace w(ws, voxels64);
  uint32_t *const peak = h > 0.0f ? w.P : nullptr;
  const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(voxels64, kWsThreads), kWsBlocks);
  const uint32_t ex = (uint32_t)sx, ey = (uint32_t)sy, ez = (uint32_t)sz;
  int rc = with_label_type(dtype, [&](auto t) -> int {
    using T = typename decltype(t)::type;
    ScopedPass sp("watershed ascend", stream);
    hipLaunchKernelGGL(k_ws_init<T>, dim3(blocks), dim3(kWsThreads), 0, stream, (const T *)labels, out, voxels);
    EDT_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ws_ascend<T>, dim3(blocks), dim3(kWsThreads), 0, stream, (const T *)labels, field, out, peak, voxels, ex, ey,
                       ez, connectivity, bin);
    EDT_HIP_TRY(hipGetLastError());
    return EDT_OK;
  });
  if (rc != EDT_OK || (rc = launch_forest_flatten(out, voxels64, w.chunks, "watershed flatten", stream)) != EDT_OK) return rc;
  if (peak) {
    {
      ScopedPass sp("watershed peaks", stream);
      hipLaunchKernelGGL(k_ws_peaks, dim3(blocks), dim3(kWsThreads), 0, stream, out, peak, voxels);
      EDT_HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_ws_spread, dim3(blocks), dim3(kWsThreads), 0, stream, out, peak, voxels);
      EDT_HIP_TRY(hipGetLastError());
    }
    rc = with_label_type(dtype, [&](auto t) -> int {
      using T = typename decltype(t)::type;
      ScopedPass sp("watershed merge", stream);
      hipLaunchKernelGGL(k_ws_merge<T>, dim3(blocks), dim3(kWsThreads), 0, stream, (const T *)labels, field, out, peak, voxels, ex,
                         ey, ez, connectivity, bin, h);
      EDT_HIP_TRY(hipGetLastError());
      return EDT_OK;
    });
    if (rc != EDT_OK || (rc = launch_forest_flatten(out, voxels64, w.chunks, "watershed flatten", stream)) != EDT_OK) return rc;
  }
  return launch_forest_number(out, voxels64, w.chunks, n, "watershed", stream);
}

}  // namespace edt_amd

using namespace edt_amd;

extern "C" {

size_t edt_hip_watershed_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz) {
  const size_t chunks = edt_hip_components_workspace_bytes(dtype, ndim, sx, sy, sz);  // (0: a bad dtype or shape, or past the limit)
  return chunks == 0 ? 0 : ForestWorkspace::bytes(sx * sy * sz);
}

int edt_hip_watershed_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, const float *d_field,
                             int connectivity, int binary, float min_saliency, uint32_t *d_out, int64_t *d_n, void *d_workspace,
                             size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int own = watershed_check_args(dtype, ndim, sx, sy, sz, connectivity, min_saliency);
  const int64_t voxels = own == EDT_OK ? sx * sy * sz : 0;
  const size_t obytes = (size_t)voxels * sizeof(uint32_t);
  const bool aliased = d_labels && d_field && d_out &&
                       (ranges_overlap(d_out, obytes, d_labels, (size_t)voxels * dtype_size(dtype)) ||
                        ranges_overlap(d_out, obytes, d_field, (size_t)voxels * sizeof(float)));
  int rc;
  if (!label_op_begin("watershed", own, d_n, 1, voxels, !d_labels || !d_field || !d_out, aliased, d_workspace, workspace_bytes,
                      ForestWorkspace::bytes(voxels), "edt_hip_watershed_workspace_bytes", stream, &rc))
    return rc;
  return launch_watershed(dtype, d_labels, sx, sy, sz, d_field, connectivity, binary, min_saliency, d_out, d_n, d_workspace, stream);
}

}  // extern "C"
