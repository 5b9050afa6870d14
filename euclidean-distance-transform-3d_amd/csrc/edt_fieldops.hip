// edt_fieldops.hip -- the compositions of the field operations on device-resident data: spherical morphology, local thickness and
// the medial axis (include/edt_hip.h, the sections of those names).  Each is written once, here: which transform feeds which
// streaming kernel, on parts carved from ONE workspace.  The host-buffer entry points (edt_host.hip) are staging around these
// calls and edt/device.py is argument handling around them.  No kernel lives here: the transforms are run_device (edt_api.hip)
// and the feature transform (edt_feature.hip), the streaming kernels edt_morph.hip and edt_medial.hip.
#include <cmath>

#include "edt_api_internal.h"

namespace edt_amd {

int morphology_check_args(int op, double radius, int flags, double *r2) {
  if (op < EDT_MORPH_ERODE || op > EDT_MORPH_CLOSE) { set_error("morphology: op must be one of EDT_MORPH_*"); return EDT_ERR_BAD_ARG; }
  const bool measures = op == EDT_MORPH_ERODE || op == EDT_MORPH_OPEN;
  if (flags & ~(measures ? (EDT_FLAG_BLACK_BORDER | EDT_FLAG_MORPH_BINARY) : 0)) {
    set_error(measures ? "morphology: erode / opening take EDT_FLAG_BLACK_BORDER and EDT_FLAG_MORPH_BINARY only"
                       : "morphology: dilate / closing take no flags");
    return EDT_ERR_UNSUPPORTED;
  }
  return morph_radius_squared(radius, op == EDT_MORPH_DILATE, "morphology", r2);
}

int thickness_check_args(int flags, const double *radii, int64_t n_radii, double step) {
  if (flags & ~(EDT_FLAG_BLACK_BORDER | EDT_FLAG_MORPH_BINARY)) {
    set_error("local_thickness takes EDT_FLAG_BLACK_BORDER and EDT_FLAG_MORPH_BINARY only");
    return EDT_ERR_UNSUPPORTED;
  }
  double r2;
  if (!radii) {
    if (n_radii < 0) { set_error("local_thickness: n_radii < 0"); return EDT_ERR_BAD_ARG; }
    return thickness_radius_squared(step, "local_thickness (the ladder's step)", &r2);
  }
  if (n_radii < 1) { set_error("local_thickness: an explicit list needs n_radii >= 1"); return EDT_ERR_BAD_ARG; }
  for (int64_t j = 0; j < n_radii; ++j) {
    if (const int bad = thickness_radius_squared(radii[j], "local_thickness", &r2)) return bad;
    if (j > 0 && !(radii[j] > radii[j - 1])) { set_error("local_thickness: radii must be strictly ascending"); return EDT_ERR_BAD_ARG; }
  }
  return EDT_OK;
}

int medial_check_args(int flags, double gamma, double ratio, double *g2) {
  if (flags & ~(EDT_FLAG_BLACK_BORDER | EDT_FLAG_MORPH_BINARY)) {
    set_error("medial_axis takes EDT_FLAG_BLACK_BORDER and EDT_FLAG_MORPH_BINARY only");
    return EDT_ERR_UNSUPPORTED;
  }
  return medial_check_params(gamma, ratio, "medial_axis", g2);
}

namespace {

bool is_binary(int dtype, int flags) { return (flags & EDT_FLAG_MORPH_BINARY) || dtype == EDT_BOOL; }

// ---- the one workspace of each operation, carved (base == nullptr: only the size is wanted) ----
// `ws`: the scratch of the operation's transforms, the largest any of its steps needs (edt_hip_workspace_bytes_flags honours
// EDT_HIP_FORCE_GENERIC, and so does run_device).
struct MorphScratch { float *field; uint8_t *mask; void *ws; size_t ws_bytes, bytes; };
MorphScratch carve_morph(void *base, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int op, int flags) {
  const size_t voxels = (size_t)(sx * sy * sz);
  const bool measures = op == EDT_MORPH_ERODE || op == EDT_MORPH_OPEN;
  Carver c(base);
  MorphScratch s = {};
  if (op == EDT_MORPH_DILATE) {  // expand_labels alone
    s.ws_bytes = edt_hip_expand_labels_workspace_bytes(dtype, ndim, sx, sy, sz);
  } else {
    s.field = c.take<float>(voxels);
    s.mask = c.take<uint8_t>(voxels);
    s.ws_bytes = edt_hip_workspace_bytes_flags(EDT_U8, ndim, sx, sy, sz, 0);
    if (measures && !is_binary(dtype, flags)) s.ws_bytes = std::max(s.ws_bytes, edt_hip_workspace_bytes_flags(dtype, ndim, sx, sy, sz, 0));
    if (!measures) s.ws_bytes = std::max(s.ws_bytes, edt_hip_expand_labels_workspace_bytes(dtype, ndim, sx, sy, sz));
  }
  s.ws = c.take<char>(s.ws_bytes);
  s.bytes = align_up(c.off, 256);
  return s;
}

struct ThicknessScratch { float *S, *B; uint8_t *mask; uint32_t *smax; void *ws; size_t ws_bytes, bytes; };
ThicknessScratch carve_thickness(void *base, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags) {
  const size_t voxels = (size_t)(sx * sy * sz);
  Carver c(base);
  ThicknessScratch s = {};
  s.S = c.take<float>(voxels);
  s.B = c.take<float>(voxels);
  s.mask = c.take<uint8_t>(voxels);
  s.smax = c.take<uint32_t>(1);
  s.ws_bytes = edt_hip_workspace_bytes_flags(EDT_U8, ndim, sx, sy, sz, 0);
  if (!is_binary(dtype, flags)) s.ws_bytes = std::max(s.ws_bytes, edt_hip_workspace_bytes_flags(dtype, ndim, sx, sy, sz, 0));
  s.ws = c.take<char>(s.ws_bytes);
  s.bytes = align_up(c.off, 256);
  return s;
}

struct MedialScratch { int32_t *planes; uint8_t *mask; float *field; void *ws; size_t ws_bytes, bytes; };
MedialScratch carve_medial(void *base, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags, bool with_radius) {
  const size_t voxels = (size_t)(sx * sy * sz);
  const bool binary = is_binary(dtype, flags);
  const int of_dtype = binary ? EDT_U8 : dtype;  // what the transforms read: the mask, or the labels
  Carver c(base);
  MedialScratch s = {};
  s.planes = c.take<int32_t>(voxels * ndim);
  if (binary) s.mask = c.take<uint8_t>(voxels);
  if (with_radius) s.field = c.take<float>(voxels);
  s.ws_bytes = edt_hip_feature_workspace_bytes(of_dtype, ndim, sx, sy, sz, flags & EDT_FLAG_BLACK_BORDER);
  if (with_radius) s.ws_bytes = std::max(s.ws_bytes, edt_hip_workspace_bytes_flags(of_dtype, ndim, sx, sy, sz, 0));
  s.ws = c.take<char>(s.ws_bytes);
  s.bytes = align_up(c.off, 256);
  return s;
}

// What the three device entry points check before their first launch, in the order of their host siblings (host_prologue,
// edt_host.hip): the shape, the call's own arguments (own_check: its *_check_args), the voxel sizes, then for a volume that is
// not empty the pointers (null_data), aliasing (aliased: d_out is d_labels and the operation does not allow it), the workspace
// (`needed()` bytes, what `query` returns) and its alignment, and the device.  true: go on to the launches; false: return *rc --
// a refusal, or EDT_OK for an empty volume.
template <typename Own, typename Needed>
bool field_op_begin(const char *who, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float &wx, float &wy, float &wz,
                    Own own_check, bool null_data, bool aliased, const void *d_workspace, size_t workspace_bytes, Needed needed,
                    const char *query, int *rc) {
  const auto refuse = [&](const std::string &why) {
    set_error(std::string(who) + ": " + why);
    *rc = EDT_ERR_BAD_ARG;
    return false;
  };
  if ((*rc = check_shape(dtype, ndim, sx, sy, sz)) != EDT_OK || (*rc = own_check()) != EDT_OK ||
      (*rc = check_voxel_sizes(ndim, wx, wy, wz)) != EDT_OK)
    return false;
  if (sx * sy * sz == 0) return false;  // (*rc is EDT_OK)
  if (null_data) return refuse("null device pointer");
  if (aliased) return refuse("d_out may not alias d_labels");
  if (!d_workspace || workspace_bytes < needed()) return refuse(std::string("workspace missing or smaller than ") + query + "()");
  if ((*rc = check_workspace_alignment(d_workspace)) != EDT_OK) return false;
  return (*rc = require_device()) == EDT_OK;
}

// The length of the default ladder of local thickness: the j >= 1 with (j * step)^2 < smax, in fp64.  They are a prefix
// (rounding is monotone): estimate its length, then settle it on the very test.
int64_t ladder_length(double smax, double step) {
  const auto below = [&](int64_t j) { const double r = (double)j * step; return r * r < smax; };
  const double q = std::sqrt(smax) / step;
  if (q >= 9.0e15) return INT64_MAX;
  int64_t k = (int64_t)q;
  while (below(k + 1)) ++k;
  while (k > 0 && !below(k)) --k;
  return k;
}

}  // namespace
}  // namespace edt_amd

using namespace edt_amd;

extern "C" {

size_t edt_hip_morphology_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int op, int flags) {
  double r2;
  if (check_shape(dtype, ndim, sx, sy, sz) != EDT_OK || morphology_check_args(op, 0.0, flags, &r2) != EDT_OK) return 0;
  return carve_morph(nullptr, dtype, ndim, sx, sy, sz, op, flags).bytes;
}

int edt_hip_morphology_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                              float wz, int op, double radius, int flags, void *d_out, void *d_workspace, size_t workspace_bytes,
                              void *stream) {
  hipStream_t s = (hipStream_t)stream;
  double r2 = 0.0;
  int rc;
  if (!field_op_begin("morphology", dtype, ndim, sx, sy, sz, wx, wy, wz, [&] { return morphology_check_args(op, radius, flags, &r2); },
                      !d_labels || !d_out, d_out == d_labels && (op == EDT_MORPH_DILATE || op == EDT_MORPH_CLOSE), d_workspace,
                      workspace_bytes, [&] { return carve_morph(nullptr, dtype, ndim, sx, sy, sz, op, flags).bytes; },
                      "edt_hip_morphology_workspace_bytes", &rc))
    return rc;
  const int64_t voxels = sx * sy * sz;
  const MorphScratch m = carve_morph(d_workspace, dtype, ndim, sx, sy, sz, op, flags);
  const auto transform = [&](const void *of, int of_dtype, int border) {
    return run_device(of, of_dtype, ndim, sx, sy, sz, wx, wy, wz, border, m.field, m.ws, m.ws_bytes, s);
  };
  if (op == EDT_MORPH_ERODE || op == EDT_MORPH_OPEN) {
    // S: the transform of the labels, or of the mask labels != 0
    const int bb = flags & EDT_FLAG_BLACK_BORDER;
    if (is_binary(dtype, flags)) {
      if ((rc = launch_is_foreground(dtype, d_labels, m.mask, voxels, s)) != EDT_OK) return rc;
      rc = transform(m.mask, EDT_U8, bb);
    } else {
      rc = transform(d_labels, dtype, bb);
    }
    if (rc != EDT_OK) return rc;
    if (op == EDT_MORPH_ERODE) return launch_morph_select(dtype, d_labels, nullptr, m.field, r2, EDT_MORPH_FARTHER, d_out, nullptr, voxels, s);
    // z = not eroded, B = its transform without a border, out = the labels within r of the eroded set
    if ((rc = launch_morph_select(dtype, nullptr, nullptr, m.field, r2, EDT_MORPH_FARTHER, nullptr, m.mask, voxels, s)) != EDT_OK ||
        (rc = transform(m.mask, EDT_U8, 0)) != EDT_OK)
      return rc;
    return launch_morph_select(dtype, d_labels, nullptr, m.field, r2, EDT_MORPH_WITHIN, d_out, nullptr, voxels, s);
  }
  rc = edt_hip_expand_labels_device(d_labels, dtype, ndim, sx, sy, sz, wx, wy, wz, radius, d_out, m.ws, m.ws_bytes, stream);
  if (rc != EDT_OK || op == EDT_MORPH_DILATE) return rc;
  // closing: the dilation eroded again -- D kept where the labels were, or farther than r from what the dilation left empty
  if ((rc = launch_is_foreground(dtype, d_out, m.mask, voxels, s)) != EDT_OK || (rc = transform(m.mask, EDT_U8, 0)) != EDT_OK) return rc;
  return launch_morph_select(dtype, d_out, d_labels, m.field, r2, EDT_MORPH_FARTHER, d_out, nullptr, voxels, s);
}

size_t edt_hip_local_thickness_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags) {
  if (check_shape(dtype, ndim, sx, sy, sz) != EDT_OK || (flags & ~(EDT_FLAG_BLACK_BORDER | EDT_FLAG_MORPH_BINARY))) return 0;
  return carve_thickness(nullptr, dtype, ndim, sx, sy, sz, flags).bytes;
}

int edt_hip_local_thickness_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                                   float wz, int flags, const double *radii, int64_t n_radii, double step, float *d_thickness,
                                   int64_t *d_sizes, int64_t *n_used, void *d_workspace, size_t workspace_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (!field_op_begin("local_thickness", dtype, ndim, sx, sy, sz, wx, wy, wz, [&] { return thickness_check_args(flags, radii, n_radii, step); },
                      !d_labels || !d_thickness || !n_used || (n_radii > 0 && !d_sizes), false, d_workspace, workspace_bytes,
                      [&] { return carve_thickness(nullptr, dtype, ndim, sx, sy, sz, flags).bytes; },
                      "edt_hip_local_thickness_workspace_bytes", &rc))
    return rc;
  if (!radii && s) {  // (the legacy stream is never captured, and asking about it would disturb a capture elsewhere)
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    EDT_HIP_TRY(hipStreamIsCapturing(s, &capturing));
    if (capturing != hipStreamCaptureStatusNone) {
      set_error("local_thickness: the default ladder reads Smax back and cannot be captured into a graph; pass explicit radii");
      return EDT_ERR_UNSUPPORTED;
    }
  }
  const int64_t voxels = sx * sy * sz;
  const ThicknessScratch t = carve_thickness(d_workspace, dtype, ndim, sx, sy, sz, flags);
  const auto transform = [&](const void *of, int of_dtype, int border, float *field) {
    return run_device(of, of_dtype, ndim, sx, sy, sz, wx, wy, wz, border, field, t.ws, t.ws_bytes, s);
  };
  const int bb = flags & EDT_FLAG_BLACK_BORDER;
  if (is_binary(dtype, flags)) {
    if ((rc = launch_is_foreground(dtype, d_labels, t.mask, voxels, s)) != EDT_OK) return rc;
    rc = transform(t.mask, EDT_U8, bb, t.S);
  } else {
    rc = transform(d_labels, dtype, bb, t.S);
  }
  // the counters are zeroed by kernels of the stream: a captured memset does not replay
  if (rc != EDT_OK || (rc = launch_fill_words(d_sizes, 0u, (size_t)n_radii * (sizeof(int64_t) / sizeof(uint32_t)), s)) != EDT_OK) return rc;
  if (!radii && (rc = launch_fill_words(t.smax, 0u, 1, s)) != EDT_OK) return rc;
  // step 0: T = 0 and the mask of the first radius (the default ladder's first radius is its step, whatever Smax turns out to be)
  std::vector<double> ladder;
  const double first = radii ? radii[0] : step;
  double r2 = 0.0, next2 = first * first;
  if ((rc = launch_thickness_step(t.S, nullptr, 0.0, 0.0f, next2, d_thickness, t.mask, nullptr, radii ? nullptr : t.smax, voxels, s)) != EDT_OK)
    return rc;
  int64_t k = n_radii;
  if (!radii) {
    uint32_t bits = 0;
    EDT_HIP_TRY(hipMemcpyAsync(&bits, t.smax, sizeof(bits), hipMemcpyDeviceToHost, s));
    EDT_HIP_TRY(hipStreamSynchronize(s));
    float smax;
    std::memcpy(&smax, &bits, sizeof(smax));
    k = ladder_length((double)smax, step);
    if (k > n_radii) {
      *n_used = k;
      set_error("local_thickness: the default ladder has " + std::to_string(k) + " radii, sizes has room for " + std::to_string(n_radii));
      return EDT_ERR_BAD_ARG;
    }
    for (int64_t j = 1; j <= k; ++j) ladder.push_back((double)j * step);
    radii = ladder.data();
  }
  for (int64_t j = 0; j < k; ++j) {
    r2 = next2;
    const bool more = j + 1 < k;
    if (more) next2 = radii[j + 1] * radii[j + 1];
    if ((rc = transform(t.mask, EDT_U8, 0, t.B)) != EDT_OK ||
        (rc = launch_thickness_step(t.S, t.B, r2, (float)radii[j], next2, d_thickness, more ? t.mask : nullptr, d_sizes + j, nullptr, voxels, s)) != EDT_OK)
      return rc;
  }
  *n_used = k;
  return EDT_OK;
}

size_t edt_hip_medial_axis_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags, int with_radius) {
  if (check_shape(dtype, ndim, sx, sy, sz) != EDT_OK || (flags & ~(EDT_FLAG_BLACK_BORDER | EDT_FLAG_MORPH_BINARY))) return 0;
  return carve_medial(nullptr, dtype, ndim, sx, sy, sz, flags, with_radius != 0).bytes;
}

int edt_hip_medial_axis_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                               float wz, int flags, double gamma, double ratio, void *d_out, float *d_radius, void *d_workspace,
                               size_t workspace_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  double g2 = 0.0;
  int rc;
  if (!field_op_begin("medial_axis", dtype, ndim, sx, sy, sz, wx, wy, wz, [&] { return medial_check_args(flags, gamma, ratio, &g2); },
                      !d_labels || !d_out, d_out == d_labels, d_workspace, workspace_bytes,
                      [&] { return carve_medial(nullptr, dtype, ndim, sx, sy, sz, flags, d_radius != nullptr).bytes; },
                      "edt_hip_medial_axis_workspace_bytes", &rc))
    return rc;
  const int64_t voxels = sx * sy * sz;
  const MedialScratch m = carve_medial(d_workspace, dtype, ndim, sx, sy, sz, flags, d_radius != nullptr);
  const int bb = flags & EDT_FLAG_BLACK_BORDER;
  const void *of = d_labels;  // what the transforms read: the labels, or their mask
  int of_dtype = dtype;
  if (m.mask) {
    if ((rc = launch_is_foreground(dtype, d_labels, m.mask, voxels, s)) != EDT_OK) return rc;
    of = m.mask;
    of_dtype = EDT_U8;
  }
  if ((rc = edt_hip_feature_transform_device(of, of_dtype, ndim, sx, sy, sz, wx, wy, wz, bb, m.planes, m.ws, m.ws_bytes, stream)) != EDT_OK)
    return rc;
  if (d_radius && (rc = run_device(of, of_dtype, ndim, sx, sy, sz, wx, wy, wz, bb | EDT_FLAG_SQRT, m.field, m.ws, m.ws_bytes, s)) != EDT_OK)
    return rc;
  return launch_medial_axis(dtype, d_labels, ndim, sx, sy, sz, wx, wy, wz, m.planes, flags, g2, ratio, d_out, m.field, d_radius, s);
}

}  // extern "C"
