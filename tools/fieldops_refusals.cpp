// fieldops_refusals.cpp -- a stand-alone program for a HOST sanitizer run of the staging (csrc/edt_host.hip) and of the three
// compositions' host code (csrc/edt_fieldops.hip): it walks the refusing paths of morphology, local thickness and the medial axis
// -- bad arguments, overlapping buffers, workspaces that are missing, too small or misaligned, empty volumes -- through the host
// and the device entry points, and checks every code.  Nothing here needs a device or launches anything: every call returns before
// its first launch (a call that passes every check ends at EDT_ERR_NO_DEVICE on a host without a GPU, and is not made on one with).
//
// Build and run, from csrc/ after `make` (the two files under test and this one with the sanitizers, the rest as built):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -I../../include -I. -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -pthread -o /tmp/fieldops_refusals \
//         $(ls ../lib/obj/*.o | grep -v -e edt_host.o -e edt_fieldops.o) -x hip ../../tools/fieldops_refusals.cpp edt_host.hip edt_fieldops.hip \
//     && /tmp/fieldops_refusals
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "edt_hip.h"

static int failures = 0;
#define EXPECT(expr, want)                                                                                     \
  do {                                                                                                         \
    const long long got_ = (long long)(expr), want_ = (long long)(want);                                       \
    if (got_ != want_) {                                                                                       \
      ++failures;                                                                                              \
      std::fprintf(stderr, "%s:%d: %s = %lld, expected %lld (%s)\n", __FILE__, __LINE__, #expr, got_, want_, edt_hip_last_error()); \
    }                                                                                                          \
  } while (0)

int main() {
  constexpr int64_t sx = 9, sy = 7, sz = 5, n = sx * sy * sz;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const bool gpu = edt_hip_device_count() > 0;
  const int through = gpu ? EDT_OK : EDT_ERR_NO_DEVICE;   // what a call without a fault ends with (made only without a device)
  std::vector<uint32_t> labels(n, 1u), out(n, 0xA5A5A5A5u), big(2 * n, 1u);
  std::vector<float> field(n, -7.0f);
  std::vector<int64_t> sizes(4, -7);
  int64_t n_used = -7;
  const double radii[3] = {1.0, 2.0, 3.0}, descending[3] = {3.0, 2.0, 1.0};

  // ---- morphology
  for (int op = EDT_MORPH_ERODE; op <= EDT_MORPH_CLOSE; ++op) {
    const size_t need = edt_hip_morphology_workspace_bytes(EDT_U32, 3, sx, sy, sz, op, 0);
    EXPECT(need > 0 && need % 256 == 0, 1);
    void *ws = std::aligned_alloc(256, need + 256);
    for (const double r : {nan, -1.0, 1e200}) {
      EXPECT(edt_hip_morphology(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, op, r, 0, out.data()), EDT_ERR_BAD_ARG);
      EXPECT(edt_hip_morphology_device(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, op, r, 0, out.data(), ws, need, nullptr), EDT_ERR_BAD_ARG);
    }
    EXPECT(edt_hip_morphology(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, op, 2.0, 256, out.data()), EDT_ERR_UNSUPPORTED);
    EXPECT(edt_hip_morphology_device(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, op, 2.0, 256, out.data(), ws, need, nullptr), EDT_ERR_UNSUPPORTED);
    EXPECT(edt_hip_morphology(labels.data(), 9, 3, sx, sy, sz, 1, 1, 1, op, 2.0, 0, out.data()), EDT_ERR_BAD_ARG);
    EXPECT(edt_hip_morphology(labels.data(), EDT_U32, 3, sx, sy, sz, 0.0f, 1, 1, op, 2.0, 0, out.data()), EDT_ERR_BAD_ARG);
    EXPECT(edt_hip_morphology(nullptr, EDT_U32, 3, sx, sy, sz, 1, 1, 1, op, 2.0, 0, out.data()), EDT_ERR_BAD_ARG);
    EXPECT(edt_hip_morphology(big.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, op, 2.0, 0, big.data() + n - 1), EDT_ERR_BAD_ARG);
    EXPECT(edt_hip_morphology_device(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, op, 2.0, 0, nullptr, ws, need, nullptr), EDT_ERR_BAD_ARG);
    EXPECT(edt_hip_morphology_device(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, op, 2.0, 0, out.data(), nullptr, need, nullptr), EDT_ERR_BAD_ARG);
    EXPECT(edt_hip_morphology_device(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, op, 2.0, 0, out.data(), ws, need - 1, nullptr), EDT_ERR_BAD_ARG);
    EXPECT(edt_hip_morphology_device(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, op, 2.0, 0, out.data(), (char *)ws + 4, need, nullptr), EDT_ERR_BAD_ARG);
    if (op == EDT_MORPH_DILATE || op == EDT_MORPH_CLOSE)
      EXPECT(edt_hip_morphology_device(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, op, 2.0, 0, labels.data(), ws, need, nullptr), EDT_ERR_BAD_ARG);
    EXPECT(edt_hip_morphology(nullptr, EDT_U32, 3, sx, 0, sz, 1, 1, 1, op, 2.0, 0, nullptr), EDT_OK);
    EXPECT(edt_hip_morphology_device(nullptr, EDT_U32, 3, sx, 0, sz, 1, 1, 1, op, 2.0, 0, nullptr, nullptr, 0, nullptr), EDT_OK);
    if (!gpu) {
      EXPECT(edt_hip_morphology(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, op, 2.0, 0, out.data()), through);
      EXPECT(edt_hip_morphology_device(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, op, 2.0, 0, out.data(), ws, need, nullptr), through);
    }
    std::free(ws);
  }
  EXPECT(edt_hip_morphology_workspace_bytes(EDT_U32, 3, sx, sy, sz, 4, 0), 0);
  EXPECT(edt_hip_morphology_workspace_bytes(EDT_U32, 2, sx, sy, sz, EDT_MORPH_OPEN, 0), 0);

  // ---- local thickness
  {
    const size_t need = edt_hip_local_thickness_workspace_bytes(EDT_U32, 3, sx, sy, sz, 0);
    EXPECT(need > 0 && need % 256 == 0, 1);
    void *ws = std::aligned_alloc(256, need + 256);
    const auto host = [&](const double *r, int64_t k, double step, int flags) {
      return edt_hip_local_thickness(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, flags, r, k, step, field.data(), sizes.data(), &n_used);
    };
    const auto dev = [&](const double *r, int64_t k, double step, int flags, void *w, size_t wb) {
      return edt_hip_local_thickness_device(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, flags, r, k, step, field.data(), sizes.data(),
                                            &n_used, w, wb, nullptr);
    };
    EXPECT(host(descending, 3, 0.0, 0), EDT_ERR_BAD_ARG);
    EXPECT(dev(descending, 3, 0.0, 0, ws, need), EDT_ERR_BAD_ARG);
    EXPECT(host(radii, 0, 0.0, 0), EDT_ERR_BAD_ARG);
    EXPECT(dev(radii, 0, 0.0, 0, ws, need), EDT_ERR_BAD_ARG);
    EXPECT(host(nullptr, -1, 1.0, 0), EDT_ERR_BAD_ARG);
    EXPECT(dev(nullptr, -1, 1.0, 0, ws, need), EDT_ERR_BAD_ARG);
    for (const double step : {nan, 0.0, inf, 1e200}) {
      EXPECT(host(nullptr, 4, step, 0), EDT_ERR_BAD_ARG);
      EXPECT(dev(nullptr, 4, step, 0, ws, need), EDT_ERR_BAD_ARG);
    }
    EXPECT(host(radii, 3, 0.0, 2), EDT_ERR_UNSUPPORTED);
    EXPECT(dev(radii, 3, 0.0, 2, ws, need), EDT_ERR_UNSUPPORTED);
    EXPECT(dev(radii, 3, 0.0, 0, nullptr, need), EDT_ERR_BAD_ARG);
    EXPECT(dev(radii, 3, 0.0, 0, ws, need - 1), EDT_ERR_BAD_ARG);
    EXPECT(dev(nullptr, 4, 1.0, 0, (char *)ws + 4, need), EDT_ERR_BAD_ARG);
    EXPECT(edt_hip_local_thickness(big.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, 0, radii, 3, 0.0, (float *)big.data() + 1, sizes.data(), &n_used),
           EDT_ERR_BAD_ARG);
    EXPECT(edt_hip_local_thickness(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, 0, radii, 3, 0.0, field.data(), nullptr, &n_used), EDT_ERR_BAD_ARG);
    EXPECT(edt_hip_local_thickness(nullptr, EDT_U32, 3, 0, sy, sz, 1, 1, 1, 0, radii, 3, 0.0, nullptr, nullptr, nullptr), EDT_OK);
    EXPECT(edt_hip_local_thickness_device(nullptr, EDT_U32, 3, 0, sy, sz, 1, 1, 1, 0, nullptr, 0, 1.0, nullptr, nullptr, nullptr, nullptr, 0, nullptr),
           EDT_OK);
    if (!gpu) {
      EXPECT(host(radii, 3, 0.0, 1 | 128), through);
      EXPECT(dev(nullptr, 4, 0.5, 0, ws, need), through);
    }
    EXPECT(n_used, -7);
    std::free(ws);
  }
  EXPECT(edt_hip_local_thickness_workspace_bytes(9, 3, sx, sy, sz, 0), 0);

  // ---- medial axis
  for (int with_radius = 0; with_radius <= 1; ++with_radius) {
    float *radius = with_radius ? field.data() : nullptr;
    const size_t need = edt_hip_medial_axis_workspace_bytes(EDT_U32, 3, sx, sy, sz, 128, with_radius);
    EXPECT(need > 0 && need % 256 == 0, 1);
    void *ws = std::aligned_alloc(256, need + 256);
    const auto host = [&](double gamma, double ratio, int flags) {
      return edt_hip_medial_axis(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, flags, gamma, ratio, out.data(), radius);
    };
    const auto dev = [&](double gamma, double ratio, int flags, void *o, void *w, size_t wb) {
      return edt_hip_medial_axis_device(labels.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, flags, gamma, ratio, o, radius, w, wb, nullptr);
    };
    for (const double g : {nan, -1.0, inf, 1e200}) {
      EXPECT(host(g, 0.0, 128), EDT_ERR_BAD_ARG);
      EXPECT(dev(g, 0.0, 128, out.data(), ws, need), EDT_ERR_BAD_ARG);
    }
    EXPECT(host(1.0, -1.0, 128), EDT_ERR_BAD_ARG);
    EXPECT(dev(1.0, nan, 128, out.data(), ws, need), EDT_ERR_BAD_ARG);
    EXPECT(host(1.0, 0.0, 2), EDT_ERR_UNSUPPORTED);
    EXPECT(dev(1.0, 0.0, 2, out.data(), ws, need), EDT_ERR_UNSUPPORTED);
    EXPECT(dev(1.0, 0.0, 128, labels.data(), ws, need), EDT_ERR_BAD_ARG);
    EXPECT(dev(1.0, 0.0, 128, nullptr, ws, need), EDT_ERR_BAD_ARG);
    EXPECT(dev(1.0, 0.0, 128, out.data(), nullptr, need), EDT_ERR_BAD_ARG);
    EXPECT(dev(1.0, 0.0, 128, out.data(), ws, need - 1), EDT_ERR_BAD_ARG);
    EXPECT(dev(1.0, 0.0, 128, out.data(), (char *)ws + 4, need), EDT_ERR_BAD_ARG);
    EXPECT(edt_hip_medial_axis(big.data(), EDT_U32, 3, sx, sy, sz, 1, 1, 1, 0, 1.0, 0.0, big.data() + 1, radius), EDT_ERR_BAD_ARG);
    EXPECT(edt_hip_medial_axis(nullptr, EDT_U32, 3, sx, sy, 0, 1, 1, 1, 0, 1.0, 0.0, nullptr, nullptr), EDT_OK);
    EXPECT(edt_hip_medial_axis_device(nullptr, EDT_U32, 3, sx, sy, 0, 1, 1, 1, 0, 1.0, 0.0, nullptr, nullptr, nullptr, 0, nullptr), EDT_OK);
    if (!gpu) {
      EXPECT(host(1.0, 0.0, 1 | 128), through);
      EXPECT(dev(0.0, 3.0, 128, out.data(), ws, need), through);
    }
    std::free(ws);
  }
  EXPECT(edt_hip_medial_axis_workspace_bytes(EDT_U32, 3, sx, sy, sz, 2, 1), 0);

  for (const uint32_t v : out) failures += v != 0xA5A5A5A5u;
  for (const float v : field) failures += v != -7.0f;
  for (const int64_t v : sizes) failures += v != -7;
  edt_hip_release_cache();
  if (failures) std::printf("fieldops_refusals: %d FAILURES\n", failures);
  else std::printf("fieldops_refusals: ok\n");
  return failures ? 1 : 0;
}
