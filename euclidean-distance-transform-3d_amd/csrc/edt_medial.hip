// edt_medial.hip -- the integer medial axis of every label at once (include/edt_hip.h, "medial axis"): one streaming stencil over
// the feature planes of edt_hip_feature_transform_device and the labels, and its device entry point.  The composition -- mask,
// feature transform, field, step -- lives one layer up: edt_hip_medial_axis_device (edt_fieldops.hip).
//
// Form.  A WAVE owns a tile of 62 x kRows x kMarch voxels (x, y, z) and marches along z; a workgroup is four such waves on
// consecutive tiles.  The 64 lanes sit on 64 consecutive x, so the x neighbours of the inner 62 are the adjacent lanes' registers
// (lanes 0 and 63 only carry them); a lane holds kRows + 2 rows of the current and of the next slice, so the y neighbours are its
// own registers (the two outer rows only carry them); the next slice becomes the current one, so a slice is loaded once per
// tile.  No LDS, no scratch.  What a tile loads beyond its own voxels -- two of 64 lanes, two of kRows + 2 rows, two of kMarch + 2
// slices -- its neighbours load at about the same time (tiles are numbered x fastest, then y, then z).
// Every PAIR of face neighbours is evaluated once: the two pruning tests are symmetric in (p, q) and crit is antisymmetric bit for
// bit (every product changes its sign and nothing else), so one evaluation tells p's side (crit >= 0) and q's side (crit <= 0).
// The pair (z, z + 1) is evaluated when z is the current slice and q's side carried to the next step; the pair (x, x + 1) by the
// lane of x, q's side handed to lane + 1.
// Every access is one element per lane (a wave instruction covers 64 consecutive elements), so any element offset of any pointer
// is served by the same code.  Labels travel as the unsigned integer of their width (a NaN keeps its payload).
#include <type_traits>

#include "edt_api_internal.h"

namespace edt_amd {
namespace {

constexpr int kMedialWaves = 4;     // waves of a workgroup, a tile each
constexpr int kMedialLanes = 62;    // x positions a wave decides (lanes 1..62)
constexpr int kMedialMarch = 16;    // slices of z a tile covers
template <int ND> constexpr int medial_rows() { return ND == 1 ? 1 : 4; }  // rows of y a tile covers

struct MedialParams {
  double A[3];      // squared voxel sizes
  double g2, ratio; // gamma^2, tan^2(theta / 2)
  int binary;       // every non-zero label is one object
  int border;       // EDT_FLAG_BLACK_BORDER: every voxel has a feature
};

template <typename U, bool FL>
__device__ __forceinline__ bool medial_nonzero(U bits) {
  return FL ? (U)(bits << 1) != 0 : bits != 0;
}

// labels[p] != 0 and labels[q] == labels[p] under the type's own comparison, on the bits: equal non-zero bits, and for floats not
// a NaN (the only floats that compare equal with different bits are the two zeros, and those are background)
template <typename U, bool FL>
__device__ __forceinline__ bool medial_same(U a, U b, int binary) {
  if (binary) return medial_nonzero<U, FL>(a) && medial_nonzero<U, FL>(b);
  if (!medial_nonzero<U, FL>(a) || a != b) return false;
  if constexpr (FL) {
    constexpr U kExp = sizeof(U) == 4 ? (U)0xFF000000u : (U)0xFFE0000000000000ull;
    return (U)(a << 1) <= kExp;
  }
  return true;
}

template <int ND>
__device__ __forceinline__ bool medial_has_feature(const int32_t (&f)[ND], int border) {
  if (border) return true;
  bool none = true;
#pragma unroll
  for (int c = 0; c < ND; ++c) none = none && f[c] == -1;
  return !none;
}

template <typename U>
__device__ __forceinline__ U lane_above(U v) {  // the value of lane + 1
  if constexpr (sizeof(U) == 8) return (U)__shfl_down((unsigned long long)v, 1);
  else return (U)__shfl_down((unsigned)v, 1);
}

// One pair p, q = p + e_axis.  two_p[c] = p_c + q_c.  on_p: q puts p on the axis; on_q: p puts q on the axis.
template <typename U, bool FL, int ND>
__device__ __forceinline__ void medial_pair(const int32_t (&fp)[ND], U lp, const int32_t (&fq)[ND], U lq, const uint32_t (&two_p)[ND],
                                            const MedialParams &P, bool &on_p, bool &on_q) {
  on_p = on_q = false;
  if (!medial_same<U, FL>(lp, lq, P.binary) || !medial_has_feature<ND>(fp, P.border) || !medial_has_feature<ND>(fq, P.border)) return;
  double sep = 0.0, h = 0.0, crit = 0.0;
#pragma unroll
  for (int c = 0; c < ND; ++c) {
    // (every integer here is below 2^33 in magnitude: the sums and differences are exact)
    const double a = (double)fp[c], b = (double)fq[c];
    const double d = __dsub_rn(a, b);
    const double s = __dsub_rn(__dadd_rn(a, b), (double)two_p[c]);
    const double t_sep = __dmul_rn(P.A[c], __dmul_rn(d, d));
    const double t_h = __dmul_rn(P.A[c], __dmul_rn(s, s));
    const double t_crit = __dmul_rn(P.A[c], __dmul_rn(d, s));
    sep = c == 0 ? t_sep : __dadd_rn(sep, t_sep);
    h = c == 0 ? t_h : __dadd_rn(h, t_h);
    crit = c == 0 ? t_crit : __dadd_rn(crit, t_crit);
  }
  const bool pass = sep > P.g2 && sep >= __dmul_rn(P.ratio, h);
  on_p = pass && crit >= 0.0;
  on_q = pass && crit <= 0.0;
}

template <typename U, bool FL, int ND, bool RADIUS>
__global__ __launch_bounds__(kMedialWaves * 64) void k_medial_axis(const U *__restrict__ labels, const int32_t *__restrict__ feat,
                                                                   U *__restrict__ out, const float *__restrict__ field,
                                                                   float *__restrict__ radius, int64_t sx, int64_t sy, int64_t sz,
                                                                   int64_t tiles_x, int64_t tiles_y, int64_t tiles, MedialParams P) {
  constexpr int TY = medial_rows<ND>(), R = TY + 2;
  const int lane = threadIdx.x & 63;
  const int64_t tile = (int64_t)blockIdx.x * kMedialWaves + (threadIdx.x >> 6);
  if (tile >= tiles) return;  // (the whole wave)
  const int64_t tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, tz = tile / (tiles_x * tiles_y);
  const int64_t x = tx * kMedialLanes - 1 + lane;
  const bool x_in = x >= 0 && x < sx;
  const bool x_own = x_in && lane >= 1 && lane <= kMedialLanes;
  const int64_t y0 = ty * TY - 1;  // row j of the registers is y0 + j
  const int64_t z0 = tz * kMedialMarch, z1 = z0 + kMedialMarch < sz ? z0 + kMedialMarch : sz;
  const int64_t voxels = sx * sy * sz;

  // rows j0 .. j1 - 1 of slice z; a voxel outside the volume reads as background
  const auto load = [&](int64_t z, int j0, int j1, int32_t (&f)[R][ND], U (&lab)[R]) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      if (j < j0 || j >= j1) continue;
      const int64_t y = y0 + j;
      lab[j] = 0;
#pragma unroll
      for (int c = 0; c < ND; ++c) f[j][c] = 0;
      if (x_in && y >= 0 && y < sy && z >= 0 && z < sz) {
        const int64_t i = x + sx * (y + sy * z);
        lab[j] = labels[i];
#pragma unroll
        for (int c = 0; c < ND; ++c) f[j][c] = feat[c * voxels + i];
      }
    }
  };
  const auto coords = [&](int64_t y, int64_t z, int axis, uint32_t (&two_p)[ND]) {
    const int64_t p[3] = {x, y, z};
#pragma unroll
    for (int c = 0; c < ND; ++c) two_p[c] = 2u * (uint32_t)p[c] + (c == axis ? 1u : 0u);
  };

  int32_t cf[R][ND], nf[R][ND];
  U cl[R], nl[R];
  load(z0, ND >= 2 ? 0 : 1, ND >= 2 ? R : 2, cf, cl);
  unsigned carry = 0;  // bit j - 1: the voxel below in z puts row j of the current slice on the axis
  if constexpr (ND == 3) {
    if (z0 > 0) {
      load(z0 - 1, 1, TY + 1, nf, nl);
#pragma unroll
      for (int j = 1; j <= TY; ++j) {
        uint32_t two_p[ND];
        coords(y0 + j, z0 - 1, 2, two_p);
        bool on_p, on_q;
        medial_pair<U, FL, ND>(nf[j], nl[j], cf[j], cl[j], two_p, P, on_p, on_q);
        carry |= on_q ? 1u << (j - 1) : 0u;
      }
    }
  }
  for (int64_t z = z0; z < z1; ++z) {
    if constexpr (ND == 3) load(z + 1, 0, R, nf, nl);
    unsigned on = carry, to_right = 0;
    // x: the pair (lane, lane + 1), the upper voxel's side handed on
#pragma unroll
    for (int j = 1; j <= TY; ++j) {
      int32_t qf[ND];
#pragma unroll
      for (int c = 0; c < ND; ++c) qf[c] = (int32_t)lane_above((uint32_t)cf[j][c]);
      const U ql = lane_above(cl[j]);
      uint32_t two_p[ND];
      coords(y0 + j, z, 0, two_p);
      bool on_p, on_q;
      medial_pair<U, FL, ND>(cf[j], cl[j], qf, ql, two_p, P, on_p, on_q);
      if (lane == 63) on_p = on_q = false;  // (lane 63 has no lane above: what came back is its own row)
      on |= on_p ? 1u << (j - 1) : 0u;
      to_right |= on_q ? 1u << (j - 1) : 0u;
    }
    on |= (unsigned)__shfl_up(to_right, 1) & (lane >= 1 ? ~0u : 0u);
    // y: the pairs (row j, row j + 1), the outer rows included
    if constexpr (ND >= 2) {
#pragma unroll
      for (int j = 0; j <= TY; ++j) {
        uint32_t two_p[ND];
        coords(y0 + j, z, 1, two_p);
        bool on_p, on_q;
        medial_pair<U, FL, ND>(cf[j], cl[j], cf[j + 1], cl[j + 1], two_p, P, on_p, on_q);
        if (j >= 1) on |= on_p ? 1u << (j - 1) : 0u;
        if (j < TY) on |= on_q ? 1u << j : 0u;
      }
    }
    // z: the pairs (current, next)
    carry = 0;
    if constexpr (ND == 3) {
#pragma unroll
      for (int j = 1; j <= TY; ++j) {
        uint32_t two_p[ND];
        coords(y0 + j, z, 2, two_p);
        bool on_p, on_q;
        medial_pair<U, FL, ND>(cf[j], cl[j], nf[j], nl[j], two_p, P, on_p, on_q);
        on |= on_p ? 1u << (j - 1) : 0u;
        carry |= on_q ? 1u << (j - 1) : 0u;
      }
    }
#pragma unroll
    for (int j = 1; j <= TY; ++j) {
      const int64_t y = y0 + j;
      if (x_own && y < sy) {
        const int64_t i = x + sx * (y + sy * z);
        const bool axis = (on >> (j - 1)) & 1u;
        out[i] = axis ? cl[j] : U(0);
        if constexpr (RADIUS) radius[i] = axis ? field[i] : 0.0f;
      }
    }
    if constexpr (ND == 3) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        cl[j] = nl[j];
#pragma unroll
        for (int c = 0; c < ND; ++c) cf[j][c] = nf[j][c];
      }
    }
  }
}

template <typename U, bool FL, int ND>
int launch_medial_typed(const void *labels, const int32_t *feat, void *out, const float *field, float *radius, int64_t sx, int64_t sy,
                        int64_t sz, const MedialParams &P, hipStream_t stream) {
  const int64_t tiles_x = ceil_div(sx, kMedialLanes), tiles_y = ceil_div(sy, medial_rows<ND>()), tiles_z = ceil_div(sz, kMedialMarch);
  const int64_t tiles = tiles_x * tiles_y * tiles_z, blocks = ceil_div(tiles, kMedialWaves);
  if (blocks > INT32_MAX) { set_error("medial_axis_step: the volume has more tiles than one grid holds"); return EDT_ERR_UNSUPPORTED; }
  const dim3 grid((unsigned)blocks), block(kMedialWaves * 64);
  if (radius)
    hipLaunchKernelGGL((k_medial_axis<U, FL, ND, true>), grid, block, 0, stream, (const U *)labels, feat, (U *)out, field, radius, sx, sy,
                       sz, tiles_x, tiles_y, tiles, P);
  else
    hipLaunchKernelGGL((k_medial_axis<U, FL, ND, false>), grid, block, 0, stream, (const U *)labels, feat, (U *)out, field, radius, sx, sy,
                       sz, tiles_x, tiles_y, tiles, P);
  EDT_HIP_TRY(hipGetLastError());
  return EDT_OK;
}

}  // namespace

int medial_check_params(double gamma, double ratio, const char *who, double *g2) {
  *g2 = gamma * gamma;
  if (!(gamma >= 0.0) || !(*g2 <= DBL_MAX)) {  // (NaN, negative, +inf, and a finite gamma whose square overflows)
    set_error(std::string(who) + ": gamma must be finite and >= 0 with a finite square");
    return EDT_ERR_BAD_ARG;
  }
  if (!(ratio >= 0.0) || !(ratio <= DBL_MAX)) {
    set_error(std::string(who) + ": ratio must be finite and >= 0");
    return EDT_ERR_BAD_ARG;
  }
  return EDT_OK;
}

int launch_medial_axis(int dtype, const void *labels, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                       const int32_t *feat, int flags, double g2, double ratio, void *out, const float *field, float *radius,
                       hipStream_t stream) {
  if (sx * sy * sz <= 0) return EDT_OK;
  MedialParams P;
  P.A[0] = (double)wx * (double)wx;
  P.A[1] = (double)wy * (double)wy;
  P.A[2] = (double)wz * (double)wz;
  P.g2 = g2;
  P.ratio = ratio;
  P.binary = ((flags & EDT_FLAG_MORPH_BINARY) || dtype == EDT_BOOL) ? 1 : 0;
  P.border = (flags & EDT_FLAG_BLACK_BORDER) ? 1 : 0;
  return with_label_type(dtype, [&](auto t) -> int {
    // (labels are compared and copied on their bits: a float label travels as the unsigned integer of its size)
    using T = typename decltype(t)::type;
    using U = std::conditional_t<sizeof(T) == 4, uint32_t, std::conditional_t<sizeof(T) == 8, uint64_t, T>>;
    constexpr bool FL = std::is_floating_point<T>::value;
    switch (ndim) {
      case 1: return launch_medial_typed<U, FL, 1>(labels, feat, out, field, radius, sx, sy, sz, P, stream);
      case 2: return launch_medial_typed<U, FL, 2>(labels, feat, out, field, radius, sx, sy, sz, P, stream);
      default: return launch_medial_typed<U, FL, 3>(labels, feat, out, field, radius, sx, sy, sz, P, stream);
    }
  });
}

}  // namespace edt_amd

using namespace edt_amd;

extern "C" {

int edt_hip_medial_axis_step_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                                    float wz, const int32_t *d_features, int flags, double gamma, double ratio, void *d_out,
                                    const float *d_field, float *d_radius, void *stream) {
  int rc = check_shape(dtype, ndim, sx, sy, sz);
  if (rc != EDT_OK) return rc;
  if (flags & ~(EDT_FLAG_BLACK_BORDER | EDT_FLAG_MORPH_BINARY)) {
    set_error("medial_axis_step takes EDT_FLAG_BLACK_BORDER and EDT_FLAG_MORPH_BINARY only");
    return EDT_ERR_UNSUPPORTED;
  }
  double g2;
  if ((rc = medial_check_params(gamma, ratio, "medial_axis_step", &g2)) != EDT_OK) return rc;
  if ((rc = check_voxel_sizes(ndim, wx, wy, wz)) != EDT_OK) return rc;
  if ((d_field != nullptr) != (d_radius != nullptr)) { set_error("medial_axis_step: d_field and d_radius come both or neither"); return EDT_ERR_BAD_ARG; }
  if (sx * sy * sz == 0) return EDT_OK;
  if (!d_labels || !d_features || !d_out) { set_error("medial_axis_step: null device pointer"); return EDT_ERR_BAD_ARG; }
  if (d_out == d_labels) { set_error("medial_axis_step: d_out may not alias d_labels"); return EDT_ERR_BAD_ARG; }
  if ((rc = require_device()) != EDT_OK) return rc;
  return launch_medial_axis(dtype, d_labels, ndim, sx, sy, sz, wx, wy, wz, d_features, flags, g2, ratio, d_out, d_field, d_radius,
                            (hipStream_t)stream);
}

}  // extern "C"
