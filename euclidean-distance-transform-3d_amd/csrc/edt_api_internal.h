// edt_api_internal.h -- what the three translation units of the C ABI share: edt_api.hip (plan + dispatch on device-resident
// data), edt_host.hip (host-buffer staging) and edt_shard_api.hip (the Z-sharded phases).  The pass-X driver, edt_rowpass.hip,
// includes it too, for ScopedPass and make_geom_y.  Internal: nothing here is exported.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "edt_common.h"
#include "edt_kernels.h"

namespace edt_amd {

// ---- workspace carving -----------------------------------------------------------------
struct Carver {
  char *base;
  size_t off = 0;
  explicit Carver(void *p) : base((char *)p) {}
  template <typename T>
  T *take(size_t count) {
    off = align_up(off, 256);
    T *p = base ? (T *)(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
};

// The workspace contract of the public *_device entry points (include/edt_hip.h): the carver's granule.  Checked in the
// extern "C" wrappers only -- run_device and the launchers take carved parts of pooled buffers from internal callers.
constexpr size_t kWorkspaceAlign = 256;
int check_workspace_alignment(const void *d_workspace);

AxisGeom make_geom_y(int64_t sx, int64_t sy, int64_t sz);
AxisGeom make_geom_z(int64_t sx, int64_t sy, int64_t sz);
bool env_force_generic();  // EDT_HIP_FORCE_GENERIC=1: every call takes the fallback kernels (test hook)
int check_shape(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz);
int check_voxel_sizes(int naxes, float &wx, float &wy, float &wz);  // (drops the sign of wy / wz: they enter as squares)
int check_column_voxel_size(float &w);
bool signed_transform_supported(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags);  // EDT_FLAG_SIGNED
int require_device();
// What the device entry points of the label operations (connected_components, fill_holes, dust, label_stats) do before their
// launch, in this order: the call's own argument check (own_rc: its result), the scalar result pointer (d_result: result_words
// int64), then for a volume that is not empty the data pointers (null_data), aliasing (aliased: the output is the labels and the call
// does not allow it), the workspace (`needed` bytes, what `query` returns) and its alignment; the device; an empty volume zeroes the
// result words on `stream`; a new call in the pass log.  true: go on to the launch; false: return *rc -- a refusal, named
// "<who>: ...", or what became of the empty volume.
bool label_op_begin(const char *who, int own_rc, void *d_result, size_t result_words, int64_t voxels, bool null_data,
                    bool aliased, const void *d_workspace, size_t workspace_bytes, size_t needed, const char *query,
                    hipStream_t stream, int *rc);
// What morphology, local thickness and the medial axis refuse after the shape and before the voxel sizes, on host buffers and on
// device-resident data alike (edt_fieldops.hip): a bad op, flags the operation does not take, bad radii, gamma or ratio.
// *r2 = radius^2, *g2 = gamma^2.
int morphology_check_args(int op, double radius, int flags, double *r2);
int thickness_check_args(int flags, const double *radii, int64_t n_radii, double step);
int medial_check_args(int flags, double gamma, double ratio, double *g2);
// What label_moments refuses after the shape, on host buffers and on device-resident data alike (edt_moments.hip): a bad
// max_labels (EDT_ERR_BAD_ARG), a volume past the range bound of its exact sums (EDT_ERR_UNSUPPORTED).
int moments_check_args(int64_t sx, int64_t sy, int64_t sz, int64_t max_labels);
// What label_topology refuses after the shape, on host buffers and on device-resident data alike (edt_topology.hip): a bad
// max_labels (EDT_ERR_BAD_ARG).
int topology_check_args(int64_t max_labels);
// whether [p, p + pb) and [q, q + qb) share a byte (an empty range shares none)
inline bool ranges_overlap(const void *p, size_t pb, const void *q, size_t qb) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return pb > 0 && qb > 0 && a < b + qb && b < a + pb;
}
// the pass pipeline on device-resident data
int run_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
               int flags, float *d_out, void *d_ws, size_t ws_bytes, hipStream_t stream);
const char *last_error_cstr();

// ---- per-pass event timing (bench.py reads this through edt_hip_get_pass_times) ----------------
struct PassLog {
  std::atomic<bool> enabled{false};
  std::vector<hipEvent_t> pool;          // reused events
  std::vector<std::pair<int, int>> span;  // (start, stop) indices of the last call
  std::vector<std::string> names;
  int used = 0;
};
extern PassLog g_log;
extern std::mutex g_log_mutex;
hipEvent_t log_event();
void log_begin_call();

struct ScopedPass {
  hipStream_t stream;
  int start = -1;
  bool named;
  ScopedPass(const char *name, hipStream_t s) : stream(s), named(name != nullptr) {  // (no name: not a pass of its own)
    if (!named) return;
    if (debug_mode() & kDbgNamePasses) fprintf(stderr, "[edt_hip] pass start: %s\n", name);
    if (!g_log.enabled.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lock(g_log_mutex);  // (only while profiling is switched on)
    hipEvent_t e = log_event();
    if (!e) return;
    start = g_log.used - 1;
    (void)hipEventRecord(e, stream);
    g_log.names.push_back(name);
  }
  ~ScopedPass() {
    if (!named) return;
    if (debug_mode() & kDbgNamePasses) {  // diagnostics: name every pass as it completes
      const hipError_t e = hipStreamSynchronize(stream);
      fprintf(stderr, "[edt_hip] pass done: %s\n", hipGetErrorString(e));
    }
    if (start < 0) return;
    std::lock_guard<std::mutex> lock(g_log_mutex);
    hipEvent_t e = log_event();
    if (!e) return;
    (void)hipEventRecord(e, stream);
    g_log.span.push_back({start, g_log.used - 1});
  }
};


}  // namespace edt_amd
