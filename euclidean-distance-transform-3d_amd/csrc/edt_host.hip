// edt_host.hip -- the C ABI (include/edt_hip.h), part 2 of 3: the host-buffer entry points -- device memory kept between
// calls, first touch of the result pages while the labels travel, the device list of the one-process multi-GPU route, sdf and
// the voxel-graph transform on host buffers.  Every voxel is still touched by HIP kernels only (run_device, edt_api.hip).
#include <system_error>
#include <thread>

#include <sys/mman.h>

#include "edt_api_internal.h"

namespace edt_amd {

// ---- host-buffer staging -----------------------------------------------------------------
// Device memory of the host-buffer entry points is kept between calls: hipMalloc / hipFree of the
// gigabyte-sized label, output and scratch buffers cost more than the transfers (measured: 64 ms per
// 512^3 uint32 call with fresh allocations, of which 2 x 9.5 ms are PCIe and 0.7 ms kernels).  One
// process-wide pool, one host call at a time (the mutex is held for the whole call); released by
// edt_hip_release_cache() or at exit.  EDT_HIP_NO_CACHE=1 restores allocate-per-call.
// what a pooled buffer is for -- one slot each, so two roles never share memory within a call
enum Slot : int { kLabels, kOut, kWorkspace, kAux /* sdf's mask, the voxel graph, tables and counts */, kSecondField, kSlotCount };
struct DevicePool {
  static constexpr int kSlots = kSlotCount;
  void *p[kSlots] = {};
  size_t cap[kSlots] = {};
  std::mutex m;
  void release() {  // (call with the owning device current)
    for (int i = 0; i < kSlots; ++i) {
      if (p[i]) (void)hipFree(p[i]);
      p[i] = nullptr;
      cap[i] = 0;
    }
  }
  ~DevicePool() { /* the runtime may already be gone at static destruction: leak on purpose */ }
};
// one pool per device ordinal: a host-buffer call uses the pool of the device that is current on the
// calling thread, so buffers are never handed to kernels running on another device
constexpr int kMaxDevices = 64;
static DevicePool g_pools[kMaxDevices];

static DevicePool *current_pool() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return (dev >= 0 && dev < kMaxDevices) ? &g_pools[dev] : nullptr;
}

static bool pool_enabled() {
  const char *e = std::getenv("EDT_HIP_NO_CACHE");
  return !(e && e[0] == '1');
}

// First touch of a large, freshly allocated result array is what dominated the host-buffer path: the kernel
// zero-fills every page on its first write, one core at a time inside the device-to-host copy (measured:
// ~35 of the 57 ms of a 512^3 call, against 2 x 9.5 ms of PCIe and 0.7 ms of kernels).  The pages are
// therefore touched by a few threads WHILE the labels travel to the device and the kernels run; the copy
// back then proceeds at PCIe speed.  (Every byte of the buffer is overwritten by the result afterwards.)
struct Prefault {
  std::vector<std::thread> threads;
  void start(void *buf, size_t bytes) {
    constexpr size_t kPage = 4096, kMin = size_t(32) << 20;
    const char *off = std::getenv("EDT_HIP_NO_PREFAULT");
    if (bytes < kMin || (off && off[0] == '1')) return;
    unsigned n = std::thread::hardware_concurrency();
    n = n == 0 ? 4 : (n > 16 ? 16 : n);
    const size_t chunk = align_up((bytes + n - 1) / n, kPage);
    volatile char *base = static_cast<volatile char *>(buf);
#ifdef MADV_HUGEPAGE
    {
      // transparent huge pages for the part of the buffer that can have them (the box runs THP in
      // "madvise" mode): 2 MiB per fault instead of 4 KiB, and a cheaper unmap when the array is freed
      const char *thp = std::getenv("EDT_HIP_NO_THP");
      const uintptr_t lo = align_up(reinterpret_cast<uintptr_t>(buf), kPage);
      const uintptr_t hi = (reinterpret_cast<uintptr_t>(buf) + bytes) & ~(uintptr_t)(kPage - 1);
      if (hi > lo && !(thp && thp[0] == '1')) (void)madvise(reinterpret_cast<void *>(lo), hi - lo, MADV_HUGEPAGE);
    }
#endif
    for (unsigned t = 0; t < n; ++t) {
      const size_t lo = (size_t)t * chunk, hi = std::min(bytes, lo + chunk);
      if (lo >= hi) break;
      try {
        threads.emplace_back([base, lo, hi] {
          for (size_t o = lo; o < hi; o += kPage) base[o] = 0;
          base[hi - 1] = 0;
        });
      } catch (const std::system_error &) {
        break;  // no more threads to be had: the remaining pages are touched by the copy itself (slower, not wrong)
      }
    }
  }
  void join() {
    for (auto &t : threads) t.join();
    threads.clear();
  }
  ~Prefault() { join(); }
};

// The device side of one host-buffer call on the current device: the pool decision (EDT_HIP_NO_CACHE=1: private allocations,
// freed at return), the pool's lock for the whole call, the buffers by role, and the transfers.
struct Staging {
  DevicePool *pool = pool_enabled() ? current_pool() : nullptr;
  std::unique_lock<std::mutex> lock;
  void *p[kSlotCount] = {};
  Prefault touch;
  Staging() { if (pool) lock = std::unique_lock<std::mutex>(pool->m); }
  ~Staging() {
    if (!pool) for (void *q : p) if (q) (void)hipFree(q);
  }
  template <typename T = void> T *at(Slot s) const { return static_cast<T *>(p[s]); }
  // the pool's slot grows where it is too small; a failure gives everything back and lets the caller see it
  int alloc(Slot s, size_t bytes) {
    if (bytes == 0) bytes = 256;
    void **q = pool ? &pool->p[s] : &p[s];
    if (!pool || pool->cap[s] < bytes) {
      if (*q) (void)hipFree(*q);
      *q = nullptr;
      if (pool) pool->cap[s] = 0;
      const hipError_t e = hipMalloc(q, bytes);
      if (e != hipSuccess) {
        *q = nullptr;
        if (pool) { (void)hipGetLastError(); pool->release(); }
        set_error(std::string("hipMalloc failed: ") + hipGetErrorString(e));
        return EDT_ERR_NOMEM;
      }
      if (pool) pool->cap[s] = bytes;
    }
    p[s] = *q;
    return EDT_OK;
  }
  int alloc(std::initializer_list<std::pair<Slot, size_t>> want) {
    for (const auto &w : want)
      if (const int rc = alloc(w.first, w.second)) return rc;
    return EDT_OK;
  }
  int up(Slot s, const void *host, size_t bytes) {
    EDT_HIP_TRY(hipMemcpy(p[s], host, bytes, hipMemcpyHostToDevice));
    return EDT_OK;
  }
  // the result pages are touched while the labels travel and the kernels run (expect), and read back once they are (down)
  void expect(void *host, size_t bytes) { touch.start(host, bytes); }
  int down(void *host, Slot s, size_t bytes, size_t offset = 0) {
    touch.join();
    EDT_HIP_TRY(hipMemcpy(host, at<char>(s) + offset, bytes, hipMemcpyDeviceToHost));
    return EDT_OK;
  }
};

// Devices of the one-process multi-GPU route (edt_multi.hip); empty = single device.
static std::mutex g_devices_mutex;
static std::vector<int> g_devices = [] {
  std::vector<int> v;
  if (const char *e = std::getenv("EDT_HIP_DEVICES")) {
    const char *p = e;
    while (*p) {
      char *end = nullptr;
      const long d = std::strtol(p, &end, 10);
      if (end == p) break;
      v.push_back((int)d);
      p = (*end == ',') ? end + 1 : end;
    }
  }
  return v;
}();

// `device` (or, by default, the first device of the list: edt_hip_set_devices / EDT_HIP_DEVICES) for the duration of one
// host-buffer call that is not sharded; no list: the caller's current device stays.  rc: the switch failed -- the call returns it.
struct ListedDevice {
  int prev = -1, rc = EDT_OK;
  bool switched = false;
  static int first_listed() {
    std::lock_guard<std::mutex> lock(g_devices_mutex);
    return g_devices.empty() ? -1 : g_devices[0];
  }
  explicit ListedDevice(int device = first_listed()) {
    if (device >= 0) rc = enter(device);
  }
  int enter(int device) {
    EDT_HIP_TRY(hipGetDevice(&prev));
    if (prev == device) return EDT_OK;
    EDT_HIP_TRY(hipSetDevice(device));
    switched = true;
    return EDT_OK;
  }
  ~ListedDevice() {
    if (switched) (void)hipSetDevice(prev);
  }
};

// What every host-buffer entry point checks before it touches the device, in this order: shape, voxel sizes (w == nullptr: the
// call has none to check), empty volume (*empty: nothing to do), null pointers, device.  `own(After)`: the checks that belong to
// one entry point, made where they always were.
enum class After { shape, voxel_sizes, pointers };
static int no_own_checks(After) { return EDT_OK; }
template <typename Own = int (*)(After)>
static int host_prologue(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float *const *w, bool null_pointer, bool *empty,
                         Own own = no_own_checks) {
  *empty = false;
  int rc = check_shape(dtype, ndim, sx, sy, sz);
  if (rc != EDT_OK || (rc = own(After::shape)) != EDT_OK) return rc;
  if (w && (rc = check_voxel_sizes(ndim, *w[0], *w[1], *w[2])) != EDT_OK) return rc;
  if ((rc = own(After::voxel_sizes)) != EDT_OK) return rc;
  if (sx * sy * sz == 0) { *empty = true; return EDT_OK; }
  if (null_pointer) { set_error("null host pointer"); return EDT_ERR_BAD_ARG; }
  if ((rc = own(After::pointers)) != EDT_OK) return rc;
  return require_device();
}

// labels up, the transform on the current device, the field down
static int run_on_current_device(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                                 float wz, int flags, float *output) {
  const size_t lbytes = (size_t)(sx * sy * sz) * dtype_size(dtype), obytes = (size_t)(sx * sy * sz) * sizeof(float);
  const size_t wbytes = edt_hip_workspace_bytes_flags(dtype, ndim, sx, sy, sz, flags);
  Staging st;
  int rc = st.alloc({{kLabels, lbytes}, {kOut, obytes}, {kWorkspace, wbytes}});
  if (rc != EDT_OK) return rc;
  st.expect(output, obytes);
  if ((rc = st.up(kLabels, labels, lbytes)) != EDT_OK) return rc;
  rc = run_device(st.p[kLabels], dtype, ndim, sx, sy, sz, wx, wy, wz, flags, st.at<float>(kOut), st.p[kWorkspace], wbytes, nullptr);
  return rc != EDT_OK ? rc : st.down(output, kOut, obytes);
}

// first touch of the whole output, then the transform Z-sharded over `devices` (edt_multi.hip)
static int run_on_devices(const void *labels, int dtype, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz, int flags,
                          float *output, const int *devices, int n_devices) {
  Prefault touch;
  touch.start(output, (size_t)(sx * sy * sz) * sizeof(float));
  touch.join();
  return run_multi(labels, dtype, sx, sy, sz, wx, wy, wz, flags, output, devices, n_devices);
}

// every ordinal of a device list names a device of this host (the caller has refused a bad list in its own words)
static int check_device_ordinals(const int *devices, int n_devices) {
  const int have = edt_hip_device_count();
  for (int i = 0; i < n_devices; ++i)
    if (devices[i] < 0 || devices[i] >= have) { set_error("device ordinal out of range"); return EDT_ERR_BAD_ARG; }
  return EDT_OK;
}

static int run_host(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz,
                    float wx, float wy, float wz, int flags, float *output) {
  float *const w[3] = {&wx, &wy, &wz};
  bool empty;
  const int rc = host_prologue(dtype, ndim, sx, sy, sz, w, !labels || !output, &empty);
  if (rc != EDT_OK || empty) return rc;
  // The device list (edt_hip_set_devices / EDT_HIP_DEVICES) is honoured by EVERY host-buffer call: a 3-D volume the
  // slab-record form can cut is Z-sharded over the listed devices, everything else (1-D, 2-D, stacks of images, the binary
  // route, the forced generic kernels, volumes that cannot be cut) runs on the FIRST listed device.
  std::vector<int> devs;
  {
    std::lock_guard<std::mutex> lock(g_devices_mutex);
    devs = g_devices;
  }
  const bool shardable = ndim == 3 && !env_force_generic() &&
                         !(flags & (EDT_FLAG_FORCE_GENERIC | EDT_FLAG_BATCH_2D | EDT_FLAG_BINARY_YZ)) && devs.size() >= 2;
  if (shardable && multi_supported(dtype, sx, sy, sz, (int)devs.size()))
    return run_on_devices(labels, dtype, sx, sy, sz, wx, wy, wz, flags, output, devs.data(), (int)devs.size());
  // a one-entry list, or a call the slab-record form does not cover: the FIRST listed device does it alone
  if (shardable) {
    static std::atomic<bool> said{false};
    if (!said.exchange(true))
      fprintf(stderr, "[edt_hip] note: a %lld x %lld x %lld volume cannot be Z-sharded over %zu devices (slab records: "
                      "sx, sy and sz <= 2048, >= 1 z-slice and >= 32 y-rows per device); device %d runs it alone\n",
              (long long)sx, (long long)sy, (long long)sz, devs.size(), devs[0]);
  }
  ListedDevice on_listed_device(devs.empty() ? -1 : devs[0]);
  if (on_listed_device.rc != EDT_OK) return on_listed_device.rc;
  return run_on_current_device(labels, dtype, ndim, sx, sy, sz, wx, wy, wz, flags, output);
}

// sdf / sdfsq on host buffers in ONE round trip (reference: src/edt.pyx:121-202, two transforms and a
// subtraction on the host): labels up once, the SIGNED transform on the device (one transform: EDT_FLAG_SIGNED; shapes it does
// not serve: edt(labels), the background mask, edt(mask) and the subtraction), the difference down once.
static int sdf_host(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx,
                    float wy, float wz, int flags, float *output) {
  float *const w[3] = {&wx, &wy, &wz};
  bool empty;
  int rc = host_prologue(dtype, ndim, sx, sy, sz, w, !labels || !output, &empty);
  if (rc != EDT_OK || empty) return rc;
  ListedDevice on_listed_device;
  if (on_listed_device.rc != EDT_OK) return on_listed_device.rc;
  const int64_t voxels = sx * sy * sz;
  const size_t lbytes = (size_t)voxels * dtype_size(dtype), obytes = (size_t)voxels * sizeof(float);
  const size_t wbytes = std::max(edt_hip_workspace_bytes_flags(dtype, ndim, sx, sy, sz, flags),
                                 edt_hip_workspace_bytes_flags(EDT_U8, ndim, sx, sy, sz, flags));
  // ONE transform where the shape allows (EDT_FLAG_SIGNED, edt_api.hip): label 0 measured like every label, its voxels negated
  // at the end
  const bool one = signed_transform_supported(dtype, ndim, sx, sy, sz, flags);
  Staging st;
  if ((rc = st.alloc({{kLabels, lbytes}, {kOut, obytes}, {kWorkspace, wbytes}})) != EDT_OK) return rc;
  if (!one && (rc = st.alloc({{kAux, (size_t)voxels}, {kSecondField, obytes}})) != EDT_OK) return rc;
  float *const a = st.at<float>(kOut);
  st.expect(output, obytes);
  if ((rc = st.up(kLabels, labels, lbytes)) != EDT_OK) return rc;
  rc = run_device(st.p[kLabels], dtype, ndim, sx, sy, sz, wx, wy, wz, one ? flags | EDT_FLAG_SIGNED : flags, a, st.p[kWorkspace], wbytes, nullptr);
  if (rc == EDT_OK && !one) {
    rc = launch_is_background(dtype, st.p[kLabels], st.at<uint8_t>(kAux), voxels, nullptr);
    if (rc == EDT_OK)
      rc = run_device(st.p[kAux], EDT_U8, ndim, sx, sy, sz, wx, wy, wz, flags, st.at<float>(kSecondField), st.p[kWorkspace], wbytes, nullptr);
    if (rc == EDT_OK) rc = launch_subtract(a, st.at<float>(kSecondField), a, voxels, nullptr);
  }
  return rc != EDT_OK ? rc : st.down(output, kOut, obytes);
}

static int voxel_graph_host(const void *labels, int dtype, const uint8_t *graph, int ndim, int64_t sx,
                            int64_t sy, int64_t sz, float wx, float wy, float wz, int black_border,
                            float *output) {
  float *const w[3] = {&wx, &wy, &wz};
  bool empty;
  int rc = host_prologue(dtype, ndim, sx, sy, sz, w, !labels || !graph || !output, &empty);
  if (rc != EDT_OK || empty) return rc;
  ListedDevice on_listed_device;
  if (on_listed_device.rc != EDT_OK) return on_listed_device.rc;
  const size_t voxels = (size_t)(sx * sy * sz), lbytes = voxels * dtype_size(dtype), obytes = voxels * sizeof(float);
  const size_t wbytes = edt_hip_voxel_graph_workspace_bytes(ndim, sx, sy, sz);
  Staging st;
  if ((rc = st.alloc({{kLabels, lbytes}, {kOut, obytes}, {kWorkspace, wbytes}, {kAux, voxels}})) != EDT_OK) return rc;
  st.expect(output, obytes);
  if ((rc = st.up(kLabels, labels, lbytes)) != EDT_OK || (rc = st.up(kAux, graph, voxels)) != EDT_OK) return rc;
  rc = edt_hip_edtsq_voxel_graph_device(st.p[kLabels], dtype, st.at<const uint8_t>(kAux), ndim, sx, sy, sz, wx, wy, wz,
                                        black_border ? EDT_FLAG_BLACK_BORDER : 0, st.at<float>(kOut), st.p[kWorkspace], wbytes,
                                        nullptr);
  return rc != EDT_OK ? rc : st.down(output, kOut, obytes);
}

// The feature transform and expand_labels on host buffers (kernels: edt_feature.hip): labels up once, the passes on the
// device, the result down once (ndim int32 planes, or one label per voxel for expand_labels).
static int feature_host(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                        float wz, int flags, bool expand, double distance, void *output) {
  float *const w[3] = {&wx, &wy, &wz};
  bool empty;
  int rc = host_prologue(dtype, ndim, sx, sy, sz, w, !labels || !output, &empty, [&](After what) -> int {
    if (what == After::voxel_sizes && expand && !(distance >= 0.0)) { set_error("expand_labels: distance must be >= 0 (inf allowed)"); return EDT_ERR_BAD_ARG; }
    return EDT_OK;
  });
  if (rc != EDT_OK || empty) return rc;
  ListedDevice on_listed_device;
  if (on_listed_device.rc != EDT_OK) return on_listed_device.rc;
  const size_t voxels = (size_t)(sx * sy * sz), lbytes = voxels * dtype_size(dtype);
  const size_t obytes = expand ? lbytes : voxels * ndim * sizeof(int32_t);
  const size_t wbytes = expand ? edt_hip_expand_labels_workspace_bytes(dtype, ndim, sx, sy, sz)
                               : edt_hip_feature_workspace_bytes(dtype, ndim, sx, sy, sz, flags);
  Staging st;
  if ((rc = st.alloc({{kLabels, lbytes}, {kOut, obytes}, {kWorkspace, wbytes}})) != EDT_OK) return rc;
  st.expect(output, obytes);
  if ((rc = st.up(kLabels, labels, lbytes)) != EDT_OK) return rc;
  rc = expand ? edt_hip_expand_labels_device(st.p[kLabels], dtype, ndim, sx, sy, sz, wx, wy, wz, distance, st.p[kOut], st.p[kWorkspace],
                                             wbytes, nullptr)
              : edt_hip_feature_transform_device(st.p[kLabels], dtype, ndim, sx, sy, sz, wx, wy, wz, flags, st.at<int32_t>(kOut),
                                                 st.p[kWorkspace], wbytes, nullptr);
  return rc != EDT_OK ? rc : st.down(output, kOut, obytes);
}

// ---- the tables of label_stats, label_moments and label_topology on host buffers -------------------------------------------
// A table's output columns, the keys first (bytes per row: the label type's), then the columns of 8-byte items, then those of
// 4-byte items (`item`: 4).  On the device (kAux): keys | 8-byte columns | n | 4-byte columns, `cap` rows each.
struct TableColumn {
  void *host;
  size_t row_bytes;
  size_t item = 8;
};
struct DeviceTable {
  static constexpr int kMaxColumns = 6;
  TableColumn cols[kMaxColumns];   // (a copy: the caller's list may be a temporary)
  int ncols;
  char *base = nullptr;
  size_t off[kMaxColumns] = {}, o_n = 0, bytes = 0;
  DeviceTable(std::initializer_list<TableColumn> c, size_t cap) : ncols((int)c.size()) {
    if (ncols > kMaxColumns) abort();  // (a table of this file with more columns than it has room for)
    std::copy(c.begin(), c.end(), cols);
    size_t o = 0;
    bool n_placed = false;
    for (int i = 0; i < ncols; ++i) {
      if (i == 1) o = align_up(o, 8);
      if (i >= 1 && !n_placed && cols[i].item == 4) { o_n = o; o += 8; n_placed = true; }
      off[i] = o;
      o += cap * cols[i].row_bytes;
    }
    if (!n_placed) { o_n = o; o += 8; }
    bytes = o;
  }
  bool null_column() const { return std::any_of(cols, cols + ncols, [](const TableColumn &c) { return !c.host; }); }
  template <typename T = void> T *col(int i) const { return (T *)(base + off[i]); }
  int64_t *n() const { return (int64_t *)(base + o_n); }
  // n first; more than `cap` labels is not an error (the caller retries with more room) and brings nothing else back
  int down(Staging &st, int64_t cap, int64_t *n_labels) const {
    int rc = st.down(n_labels, kAux, sizeof(int64_t), o_n);
    if (rc != EDT_OK || *n_labels > cap || *n_labels == 0) return rc;
    for (int i = 0; i < ncols; ++i)
      if ((rc = st.down(cols[i].host, kAux, (size_t)*n_labels * cols[i].row_bytes, off[i])) != EDT_OK) return rc;
    return EDT_OK;
  }
};

// label_stats on host buffers (kernels: edt_labelstats.hip): labels up once (and the caller's field, if it brings one; else the
// ordinary transform runs here, with sqrt), the table pass on the device, and only the table comes back.
static int label_stats_host(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                            float wz, int black_border, const float *dt, int64_t max_labels, void *keys, int64_t *counts,
                            float *max, int64_t *argmax, int32_t *bbox, int64_t *n_labels) {
  int64_t cap = 0;
  size_t sbytes = 0;
  float *const w[3] = {&wx, &wy, &wz};
  bool empty;
  int rc = host_prologue(dtype, ndim, sx, sy, sz, dt ? nullptr : w, !labels || !keys || !counts || !max || !argmax || !bbox, &empty,
                         [&](After what) -> int {
    if (what == After::shape && max_labels < 1) { set_error("label_stats: max_labels must be at least 1"); return EDT_ERR_BAD_ARG; }
    if (what == After::voxel_sizes && !n_labels) { set_error("null host pointer"); return EDT_ERR_BAD_ARG; }
    if (what == After::pointers) {  // (the volume is not empty here)
      cap = std::min(max_labels, sx * sy * sz);
      sbytes = edt_hip_label_stats_workspace_bytes(dtype, sx * sy * sz, cap);
      if (sbytes == 0) { set_error("label_stats: max_labels out of range"); return EDT_ERR_BAD_ARG; }
    }
    return EDT_OK;
  });
  if (rc == EDT_OK && empty) *n_labels = 0;
  if (rc != EDT_OK || empty) return rc;
  ListedDevice on_listed_device;
  if (on_listed_device.rc != EDT_OK) return on_listed_device.rc;
  const int64_t voxels = sx * sy * sz;
  const int flags = (black_border ? EDT_FLAG_BLACK_BORDER : 0) | EDT_FLAG_SQRT;
  const size_t lbytes = (size_t)voxels * dtype_size(dtype), fbytes = (size_t)voxels * sizeof(float);
  const size_t tbytes = dt ? 0 : edt_hip_workspace_bytes_flags(dtype, ndim, sx, sy, sz, flags);
  const size_t wbytes = std::max(sbytes, tbytes);
  DeviceTable tab({{keys, (size_t)dtype_size(dtype)}, {counts, 8}, {argmax, 8}, {max, 4, 4}, {bbox, 24, 4}}, (size_t)cap);
  Staging st;
  if ((rc = st.alloc({{kLabels, lbytes}, {kOut, fbytes}, {kWorkspace, wbytes}, {kAux, tab.bytes}})) != EDT_OK) return rc;
  if ((rc = st.up(kLabels, labels, lbytes)) != EDT_OK) return rc;
  rc = dt ? st.up(kOut, dt, fbytes)
          : run_device(st.p[kLabels], dtype, ndim, sx, sy, sz, wx, wy, wz, flags, st.at<float>(kOut), st.p[kWorkspace], wbytes, nullptr);
  if (rc != EDT_OK) return rc;
  tab.base = st.at<char>(kAux);
  rc = edt_hip_label_stats_device(st.p[kLabels], dtype, st.at<const float>(kOut), ndim, sx, sy, sz, cap, tab.col(0),
                                  tab.col<int64_t>(1), tab.col<float>(3), tab.col<int64_t>(2), tab.col<int32_t>(4), tab.n(),
                                  st.p[kWorkspace], wbytes, nullptr);
  return rc != EDT_OK ? rc : tab.down(st, cap, n_labels);
}

// label_moments and label_topology on host buffers (kernels: edt_moments.hip, edt_topology.hip): labels up once, the sweep on the
// device, and only the table comes back.  own_check: what the call refuses after the shape (its *_check_args).  ws_query: its
// edt_hip_*_workspace_bytes.  cols: its output columns.  call(d_labels, cap, table, d_ws, ws_bytes): its device entry point.
template <typename Check, typename Call>
static int label_table_host(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int64_t max_labels,
                            size_t (*ws_query)(int, int64_t, int64_t), std::initializer_list<TableColumn> cols, int64_t *n_labels,
                            Check own_check, Call call) {
  int64_t cap = 0;
  size_t sbytes = 0;
  bool empty;
  int rc = host_prologue(dtype, ndim, sx, sy, sz, nullptr, !labels || DeviceTable(cols, 0).null_column(), &empty,
                         [&](After what) -> int {
    if (what == After::shape) return own_check();
    if (what == After::voxel_sizes && !n_labels) { set_error("null host pointer"); return EDT_ERR_BAD_ARG; }
    if (what == After::pointers) {  // (the volume is not empty here)
      cap = std::min(max_labels, sx * sy * sz);
      sbytes = ws_query(dtype, sx * sy * sz, cap);
    }
    return EDT_OK;
  });
  if (rc == EDT_OK && empty && (rc = require_device()) == EDT_OK) *n_labels = 0;  // (the device form's answer to an empty volume)
  if (rc != EDT_OK || empty) return rc;
  ListedDevice on_listed_device;
  if (on_listed_device.rc != EDT_OK) return on_listed_device.rc;
  const size_t lbytes = (size_t)(sx * sy * sz) * dtype_size(dtype);
  DeviceTable tab(cols, (size_t)cap);
  Staging st;
  if ((rc = st.alloc({{kLabels, lbytes}, {kWorkspace, sbytes}, {kAux, tab.bytes}})) != EDT_OK) return rc;
  if ((rc = st.up(kLabels, labels, lbytes)) != EDT_OK) return rc;
  tab.base = st.at<char>(kAux);
  rc = call(st.p[kLabels], cap, tab, st.p[kWorkspace], sbytes);
  return rc != EDT_OK ? rc : tab.down(st, cap, n_labels);
}

// connected_components, fill_holes and dust on host buffers (kernels: edt_components.hip, edt_fillholes.hip, edt_dust.hip):
// labels up once, the operation on the device, its output and its int64 results down once.  What tells the three apart:
enum class Alias { ignored /* the output is of another type */, refused, in_place /* the result pages are the labels', and being read: no first touch */ };
struct LabelOp {
  const char *who;   // the call's name in its own refusals
  size_t out_elem;   // bytes per voxel of the output
  int words;         // int64 results
  Alias alias;       // what out == labels means to it
  size_t (*ws_query)(int, int, int64_t, int64_t, int64_t);  // its edt_hip_*_workspace_bytes
};
// own_check: what the call refuses after the shape (its *_check_args).  call(d_labels, d_out, d_result, d_ws, ws_bytes): its
// device entry point.
template <typename Check, typename Call>
static int label_op_host(const LabelOp &op, const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, void *out,
                         int64_t *result, Check own_check, Call call) {
  bool empty;
  int rc = host_prologue(dtype, ndim, sx, sy, sz, nullptr, !labels || !out, &empty, [&](After what) -> int {
    if (what == After::shape) return own_check();
    if (what == After::voxel_sizes && !result) { set_error("null host pointer"); return EDT_ERR_BAD_ARG; }
    if (what == After::pointers && op.alias == Alias::refused && labels == out) {
      set_error(std::string(op.who) + ": the output may not alias the labels");
      return EDT_ERR_BAD_ARG;
    }
    return EDT_OK;
  });
  if (rc == EDT_OK && empty) std::fill(result, result + op.words, int64_t(0));
  if (rc != EDT_OK || empty) return rc;
  ListedDevice on_listed_device;
  if (on_listed_device.rc != EDT_OK) return on_listed_device.rc;
  const size_t voxels = (size_t)(sx * sy * sz), lbytes = voxels * dtype_size(dtype), obytes = voxels * op.out_elem;
  const size_t wbytes = op.ws_query(dtype, ndim, sx, sy, sz), rbytes = op.words * sizeof(int64_t);
  Staging st;
  if ((rc = st.alloc({{kLabels, lbytes}, {kOut, obytes}, {kWorkspace, wbytes}, {kAux, rbytes}})) != EDT_OK) return rc;
  if (!(op.alias == Alias::in_place && out == labels)) st.expect(out, obytes);
  if ((rc = st.up(kLabels, labels, lbytes)) != EDT_OK) return rc;
  rc = call(st.p[kLabels], st.p[kOut], st.at<int64_t>(kAux), st.p[kWorkspace], wbytes);
  if (rc != EDT_OK || (rc = st.down(out, kOut, obytes)) != EDT_OK) return rc;
  return st.down(result, kAux, rbytes);
}

}  // namespace edt_amd

using namespace edt_amd;

extern "C" {

int edt_hip_squared_edt_1d_multi_seg(const void *labels, int dtype, float *dest, int64_t n,
                                     int64_t stride, float anisotropy, int black_border) {
  if (stride != 1) {
    set_error("stride != 1 is not supported (no reference caller uses it)");
    return EDT_ERR_UNSUPPORTED;
  }
  return run_host(labels, dtype, 1, n, 1, 1, anisotropy, 1.0f, 1.0f,
                  black_border ? EDT_FLAG_BLACK_BORDER : 0, dest);
}

int edt_hip_edt2dsq(const void *labels, int dtype, int64_t sx, int64_t sy, float wx, float wy,
                    int black_border, int /*parallel*/, float *output) {
  return run_host(labels, dtype, 2, sx, sy, 1, wx, wy, 1.0f,
                  black_border ? EDT_FLAG_BLACK_BORDER : 0, output);
}

int edt_hip_edt3dsq(const void *labels, int dtype, int64_t sx, int64_t sy, int64_t sz, float wx,
                    float wy, float wz, int black_border, int /*parallel*/, float *output) {
  return run_host(labels, dtype, 3, sx, sy, sz, wx, wy, wz,
                  black_border ? EDT_FLAG_BLACK_BORDER : 0, output);
}

int edt_hip_edt2d(const void *labels, int dtype, int64_t sx, int64_t sy, float wx, float wy,
                  int black_border, int /*parallel*/, float *output) {
  return run_host(labels, dtype, 2, sx, sy, 1, wx, wy, 1.0f,
                  (black_border ? EDT_FLAG_BLACK_BORDER : 0) | EDT_FLAG_SQRT, output);
}

int edt_hip_edt3d(const void *labels, int dtype, int64_t sx, int64_t sy, int64_t sz, float wx,
                  float wy, float wz, int black_border, int /*parallel*/, float *output) {
  return run_host(labels, dtype, 3, sx, sy, sz, wx, wy, wz,
                  (black_border ? EDT_FLAG_BLACK_BORDER : 0) | EDT_FLAG_SQRT, output);
}

int edt_hip_binary_edtsq(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx,
                         float wy, float wz, int black_border, int take_sqrt, float *output) {
  if (ndim != 2 && ndim != 3) { set_error("binary route: ndim must be 2 or 3"); return EDT_ERR_BAD_ARG; }
  return run_host(labels, dtype, ndim, sx, sy, sz, wx, wy, wz,
                  (black_border ? EDT_FLAG_BLACK_BORDER : 0) | (take_sqrt ? EDT_FLAG_SQRT : 0) | EDT_FLAG_BINARY_YZ,
                  output);
}

int edt_hip_edt2dsq_batch(const void *labels, int dtype, int64_t sx, int64_t sy, int64_t count, float wx, float wy,
                          int black_border, int take_sqrt, float *output) {
  return run_host(labels, dtype, 3, sx, sy, count, wx, wy, 1.0f,
                  (black_border ? EDT_FLAG_BLACK_BORDER : 0) | (take_sqrt ? EDT_FLAG_SQRT : 0) | EDT_FLAG_BATCH_2D,
                  output);
}

int edt_hip_set_devices(const int *devices, int n_devices) {
  if (n_devices < 0 || (n_devices > 0 && !devices)) { set_error("bad device list"); return EDT_ERR_BAD_ARG; }
  if (const int rc = check_device_ordinals(devices, n_devices)) return rc;
  std::lock_guard<std::mutex> lock(g_devices_mutex);
  g_devices.assign(devices, devices + n_devices);
  return EDT_OK;
}

int edt_hip_edt3dsq_multi(const void *labels, int dtype, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                          float wz, int black_border, int take_sqrt, float *output, const int *devices,
                          int n_devices) {
  int rc = check_shape(dtype, 3, sx, sy, sz);
  if (rc != EDT_OK) return rc;
  if ((rc = check_voxel_sizes(3, wx, wy, wz)) != EDT_OK) return rc;
  if (sx == 0 || sy == 0 || sz == 0) return EDT_OK;
  if (!labels || !output || !devices || n_devices < 1) { set_error("null pointer / empty device list"); return EDT_ERR_BAD_ARG; }
  if ((rc = require_device()) != EDT_OK || (rc = check_device_ordinals(devices, n_devices)) != EDT_OK) return rc;
  const int flags = (black_border ? EDT_FLAG_BLACK_BORDER : 0) | (take_sqrt ? EDT_FLAG_SQRT : 0);
  if (n_devices >= 2 && !multi_supported(dtype, sx, sy, sz, n_devices)) {
    set_error("this volume cannot be Z-sharded over " + std::to_string(n_devices) + " devices (slab records: sx, sy "
              "and sz <= 2048, at least one z-slice and 32 y-rows per device; edt_hip_multi_supported tells)");
    return EDT_ERR_UNSUPPORTED;
  }
  if (n_devices == 1) {  // a list of one: that device does it
    ListedDevice on_that_device(devices[0]);
    if (on_that_device.rc != EDT_OK) return on_that_device.rc;
    return run_on_current_device(labels, dtype, 3, sx, sy, sz, wx, wy, wz, flags, output);
  }
  return run_on_devices(labels, dtype, sx, sy, sz, wx, wy, wz, flags, output, devices, n_devices);
}

int edt_hip_multi_supported(int dtype, int64_t sx, int64_t sy, int64_t sz, int n_devices) {
  if (check_shape(dtype, 3, sx, sy, sz) != EDT_OK) return 0;
  return (n_devices == 1 || multi_supported(dtype, sx, sy, sz, n_devices)) ? 1 : 0;
}

int edt_hip_sdf(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                float wz, int black_border, int squared, float *output) {
  return sdf_host(labels, dtype, ndim, sx, sy, sz, wx, wy, wz,
                  (black_border ? EDT_FLAG_BLACK_BORDER : 0) | (squared ? 0 : EDT_FLAG_SQRT), output);
}

int edt_hip_release_cache(void) {
  multi_release();
  int cur = 0;
  if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); return EDT_OK; }
  for (int d = 0; d < kMaxDevices; ++d) {
    std::lock_guard<std::mutex> lock(g_pools[d].m);
    bool any = false;
    for (int i = 0; i < DevicePool::kSlots; ++i) any = any || g_pools[d].p[i] != nullptr;
    if (!any) continue;
    if (hipSetDevice(d) != hipSuccess) { (void)hipGetLastError(); continue; }
    g_pools[d].release();
  }
  (void)hipSetDevice(cur);
  return EDT_OK;
}

int edt_hip_edt2dsq_voxel_graph(const void *labels, int dtype, const uint8_t *graph, int64_t sx,
                                int64_t sy, float wx, float wy, int black_border,
                                float *workspace) {
  return voxel_graph_host(labels, dtype, graph, 2, sx, sy, 1, wx, wy, 2.0f, black_border, workspace);
}

int edt_hip_edt3dsq_voxel_graph(const void *labels, int dtype, const uint8_t *graph, int64_t sx,
                                int64_t sy, int64_t sz, float wx, float wy, float wz,
                                int black_border, float *workspace) {
  return voxel_graph_host(labels, dtype, graph, 3, sx, sy, sz, wx, wy, wz, black_border, workspace);
}

int edt_hip_feature_transform(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx,
                              float wy, float wz, int black_border, int32_t *features) {
  return feature_host(labels, dtype, ndim, sx, sy, sz, wx, wy, wz, black_border ? EDT_FLAG_BLACK_BORDER : 0, false, 0.0,
                      features);
}

int edt_hip_expand_labels(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                          float wz, double distance, void *output) {
  return feature_host(labels, dtype, ndim, sx, sy, sz, wx, wy, wz, 0, true, distance, output);
}

int edt_hip_label_stats(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                        float wz, int black_border, const float *dt, int64_t max_labels, void *keys, int64_t *counts,
                        float *max, int64_t *argmax, int32_t *bbox, int64_t *n_labels) {
  return label_stats_host(labels, dtype, ndim, sx, sy, sz, wx, wy, wz, black_border, dt, max_labels, keys, counts, max,
                          argmax, bbox, n_labels);
}

int edt_hip_label_moments(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int64_t max_labels,
                          void *keys, int64_t *counts, int64_t *sums, double *centroid, double *central, int64_t *n_labels) {
  return label_table_host(
      labels, dtype, ndim, sx, sy, sz, max_labels, edt_hip_label_moments_workspace_bytes,
      {{keys, (size_t)dtype_size(dtype)}, {counts, 8}, {sums, 72}, {centroid, 24}, {central, 48}}, n_labels,
      [&] { return moments_check_args(sx, sy, sz, max_labels); },
      [&](const void *d_labels, int64_t cap, const DeviceTable &t, void *ws, size_t ws_bytes) {
        return edt_hip_label_moments_device(d_labels, dtype, ndim, sx, sy, sz, cap, t.col(0), t.col<int64_t>(1), t.col<int64_t>(2),
                                            t.col<double>(3), t.col<double>(4), t.n(), ws, ws_bytes, nullptr);
      });
}

int edt_hip_label_topology(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int64_t max_labels,
                           void *keys, int64_t *closed, int64_t *interior, int64_t *n_labels) {
  return label_table_host(
      labels, dtype, ndim, sx, sy, sz, max_labels, edt_hip_label_topology_workspace_bytes,
      {{keys, (size_t)dtype_size(dtype)}, {closed, 64}, {interior, 64}}, n_labels, [&] { return topology_check_args(max_labels); },
      [&](const void *d_labels, int64_t cap, const DeviceTable &t, void *ws, size_t ws_bytes) {
        return edt_hip_label_topology_device(d_labels, dtype, ndim, sx, sy, sz, cap, t.col(0), t.col<int64_t>(1), t.col<int64_t>(2),
                                             t.n(), ws, ws_bytes, nullptr);
      });
}

int edt_hip_connected_components(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz,
                                 int connectivity, int binary, uint32_t *out, int64_t *n) {
  return label_op_host(
      {"connected_components", sizeof(uint32_t), 1, Alias::ignored, edt_hip_components_workspace_bytes}, labels, dtype, ndim, sx, sy,
      sz, out, n, [&] { return components_check_args(dtype, ndim, sx, sy, sz, connectivity); },
      [&](const void *d_labels, void *d_out, int64_t *d_n, void *d_ws, size_t ws_bytes) {
        return edt_hip_connected_components_device(d_labels, dtype, ndim, sx, sy, sz, connectivity, binary, (uint32_t *)d_out, d_n,
                                                   d_ws, ws_bytes, nullptr);
      });
}

int edt_hip_fill_holes(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity, int binary,
                       void *out, int64_t *n_filled) {
  return label_op_host(
      {"fill_holes", (size_t)dtype_size(dtype), 1, Alias::refused, edt_hip_fill_holes_workspace_bytes}, labels, dtype, ndim, sx, sy, sz, out,
      n_filled, [&] { return components_check_args(dtype, ndim, sx, sy, sz, connectivity, "fill_holes"); },
      [&](const void *d_labels, void *d_out, int64_t *d_n, void *d_ws, size_t ws_bytes) {
        return edt_hip_fill_holes_device(d_labels, dtype, ndim, sx, sy, sz, connectivity, binary, d_out, d_n, d_ws, ws_bytes, nullptr);
      });
}

int edt_hip_dust(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity, int binary,
                 int64_t min_voxels, int64_t max_voxels, int invert, void *out, int64_t *counts) {
  return label_op_host(
      {"dust", (size_t)dtype_size(dtype), 3, Alias::in_place, edt_hip_dust_workspace_bytes}, labels, dtype, ndim, sx, sy, sz, out, counts,
      [&] { return dust_check_args(dtype, ndim, sx, sy, sz, connectivity, min_voxels, max_voxels); },
      [&](const void *d_labels, void *d_out, int64_t *d_counts, void *d_ws, size_t ws_bytes) {
        return edt_hip_dust_device(d_labels, dtype, ndim, sx, sy, sz, connectivity, binary, min_voxels, max_voxels, invert, d_out,
                                   d_counts, d_ws, ws_bytes, nullptr);
      });
}

// watershed on host buffers (kernels: edt_watershed.hip): labels up once -- and the caller's field, if it brings one; else the
// ordinary transform runs here, with sqrt, under `binary` on the mask labels != 0 --, the operation on the device, the basins
// and their number down once.
int edt_hip_watershed(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, const float *field, float wx,
                      float wy, float wz, int flags, int connectivity, int binary, float min_saliency, uint32_t *out, int64_t *n) {
  float *const w[3] = {&wx, &wy, &wz};
  bool empty;
  int rc = host_prologue(dtype, ndim, sx, sy, sz, field ? nullptr : w, !labels || !out, &empty, [&](After what) -> int {
    if (what == After::shape) {
      const int own = watershed_check_args(dtype, ndim, sx, sy, sz, connectivity, min_saliency);
      if (own != EDT_OK) return own;
      if (flags & ~EDT_FLAG_BLACK_BORDER) { set_error("watershed: flags other than EDT_FLAG_BLACK_BORDER"); return EDT_ERR_BAD_ARG; }
    }
    if (what == After::voxel_sizes && !n) { set_error("null host pointer"); return EDT_ERR_BAD_ARG; }
    return EDT_OK;
  });
  if (rc == EDT_OK && empty) *n = 0;
  if (rc != EDT_OK || empty) return rc;
  ListedDevice on_listed_device;
  if (on_listed_device.rc != EDT_OK) return on_listed_device.rc;
  const int64_t voxels = sx * sy * sz;
  const bool mask = !field && binary && dtype != EDT_BOOL;  // the transform of the mask, not of the labels
  const int tdtype = mask ? EDT_U8 : dtype;
  const int tflags = (flags & EDT_FLAG_BLACK_BORDER) | EDT_FLAG_SQRT;
  const size_t lbytes = (size_t)voxels * dtype_size(dtype), fbytes = (size_t)voxels * sizeof(float), obytes = (size_t)voxels * sizeof(uint32_t);
  const size_t sbytes = edt_hip_watershed_workspace_bytes(dtype, ndim, sx, sy, sz);
  const size_t wbytes = std::max(sbytes, field ? 0 : edt_hip_workspace_bytes_flags(tdtype, ndim, sx, sy, sz, tflags));
  constexpr size_t kMaskAt = 256;  // kAux: n, then the mask
  Staging st;
  if ((rc = st.alloc({{kLabels, lbytes}, {kSecondField, fbytes}, {kOut, obytes}, {kWorkspace, wbytes},
                      {kAux, kMaskAt + (mask ? (size_t)voxels : 0)}})) != EDT_OK)
    return rc;
  st.expect(out, obytes);
  if ((rc = st.up(kLabels, labels, lbytes)) != EDT_OK) return rc;
  if (field) {
    rc = st.up(kSecondField, field, fbytes);
  } else {
    const void *src = st.p[kLabels];
    if (mask) {
      rc = launch_is_foreground(dtype, st.p[kLabels], st.at<uint8_t>(kAux) + kMaskAt, voxels, nullptr);
      src = st.at<uint8_t>(kAux) + kMaskAt;
    }
    if (rc == EDT_OK)
      rc = run_device(src, tdtype, ndim, sx, sy, sz, wx, wy, wz, tflags, st.at<float>(kSecondField), st.p[kWorkspace], wbytes, nullptr);
  }
  if (rc != EDT_OK) return rc;
  rc = edt_hip_watershed_device(st.p[kLabels], dtype, ndim, sx, sy, sz, st.at<const float>(kSecondField), connectivity, binary,
                                min_saliency, st.at<uint32_t>(kOut), st.at<int64_t>(kAux), st.p[kWorkspace], wbytes, nullptr);
  if (rc != EDT_OK || (rc = st.down(out, kOut, obytes)) != EDT_OK) return rc;
  return st.down(n, kAux, sizeof(int64_t));
}

// erode / dilate / opening / closing, local thickness and the medial axis on host buffers (contracts: include/edt_hip.h,
// "morphology", "local thickness", "medial axis"): staging around the one composition of each, its *_device entry point
// (edt_fieldops.hip) -- labels up once, the call on the pooled buffers with one workspace, the outputs down once.  What the host
// entries refuse beyond their device siblings: every overlap of their buffers.
int edt_hip_morphology(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                       int op, double radius, int flags, void *output) {
  double r2;
  float *const w[3] = {&wx, &wy, &wz};
  bool empty;
  int rc = host_prologue(dtype, ndim, sx, sy, sz, w, !labels || !output, &empty, [&](After what) -> int {
    if (what == After::shape) return morphology_check_args(op, radius, flags, &r2);
    if (what == After::pointers) {
      const size_t bytes = (size_t)(sx * sy * sz) * dtype_size(dtype);
      if (ranges_overlap(labels, bytes, output, bytes)) { set_error("morphology: the output may not overlap the labels"); return EDT_ERR_BAD_ARG; }
    }
    return EDT_OK;
  });
  if (rc != EDT_OK || empty) return rc;
  ListedDevice on_listed_device;
  if (on_listed_device.rc != EDT_OK) return on_listed_device.rc;
  const size_t lbytes = (size_t)(sx * sy * sz) * dtype_size(dtype);
  const size_t wbytes = edt_hip_morphology_workspace_bytes(dtype, ndim, sx, sy, sz, op, flags);
  Staging st;
  if ((rc = st.alloc({{kLabels, lbytes}, {kOut, lbytes}, {kWorkspace, wbytes}})) != EDT_OK) return rc;
  st.expect(output, lbytes);
  if ((rc = st.up(kLabels, labels, lbytes)) != EDT_OK) return rc;
  rc = edt_hip_morphology_device(st.p[kLabels], dtype, ndim, sx, sy, sz, wx, wy, wz, op, radius, flags, st.p[kOut], st.p[kWorkspace],
                                 wbytes, nullptr);
  return rc != EDT_OK ? rc : st.down(output, kOut, lbytes);
}

// (the sizes travel in kAux: n_radii int64)
int edt_hip_local_thickness(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                            int flags, const double *radii, int64_t n_radii, double step, float *thickness, int64_t *sizes,
                            int64_t *n_used) {
  float *const w[3] = {&wx, &wy, &wz};
  bool empty;
  int rc = host_prologue(dtype, ndim, sx, sy, sz, w, !labels || !thickness || !n_used || (n_radii > 0 && !sizes), &empty, [&](After what) -> int {
    if (what == After::shape) return thickness_check_args(flags, radii, n_radii, step);
    if (what == After::pointers) {
      const size_t voxels = (size_t)(sx * sy * sz);
      const size_t lbytes = voxels * dtype_size(dtype), tbytes = voxels * sizeof(float), sbytes = (size_t)n_radii * sizeof(int64_t);
      if (ranges_overlap(labels, lbytes, thickness, tbytes) || ranges_overlap(labels, lbytes, sizes, sbytes) ||
          ranges_overlap(thickness, tbytes, sizes, sbytes)) {
        set_error("local_thickness: thickness, sizes and the labels may not overlap");
        return EDT_ERR_BAD_ARG;
      }
    }
    return EDT_OK;
  });
  if (rc != EDT_OK || empty) return rc;
  ListedDevice on_listed_device;
  if (on_listed_device.rc != EDT_OK) return on_listed_device.rc;
  const size_t voxels = (size_t)(sx * sy * sz), lbytes = voxels * dtype_size(dtype), fbytes = voxels * sizeof(float);
  const size_t wbytes = edt_hip_local_thickness_workspace_bytes(dtype, ndim, sx, sy, sz, flags);
  Staging st;
  if ((rc = st.alloc({{kLabels, lbytes}, {kOut, fbytes}, {kWorkspace, wbytes}, {kAux, (size_t)n_radii * sizeof(int64_t)}})) != EDT_OK) return rc;
  st.expect(thickness, fbytes);
  if ((rc = st.up(kLabels, labels, lbytes)) != EDT_OK) return rc;
  rc = edt_hip_local_thickness_device(st.p[kLabels], dtype, ndim, sx, sy, sz, wx, wy, wz, flags, radii, n_radii, step, st.at<float>(kOut),
                                      st.at<int64_t>(kAux), n_used, st.p[kWorkspace], wbytes, nullptr);
  if (rc != EDT_OK || (rc = st.down(thickness, kOut, fbytes)) != EDT_OK) return rc;
  return *n_used > 0 ? st.down(sizes, kAux, (size_t)*n_used * sizeof(int64_t)) : EDT_OK;
}

// (the radius travels in kSecondField)
int edt_hip_medial_axis(const void *labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                        int flags, double gamma, double ratio, void *out, float *radius) {
  double g2;
  float *const w[3] = {&wx, &wy, &wz};
  bool empty;
  int rc = host_prologue(dtype, ndim, sx, sy, sz, w, !labels || !out, &empty, [&](After what) -> int {
    if (what == After::shape) return medial_check_args(flags, gamma, ratio, &g2);
    if (what == After::pointers) {
      const size_t voxels = (size_t)(sx * sy * sz), lbytes = voxels * dtype_size(dtype), rbytes = radius ? voxels * sizeof(float) : 0;
      if (ranges_overlap(labels, lbytes, out, lbytes) || ranges_overlap(labels, lbytes, radius, rbytes) ||
          ranges_overlap(out, lbytes, radius, rbytes)) {
        set_error("medial_axis: out, radius and the labels may not overlap");
        return EDT_ERR_BAD_ARG;
      }
    }
    return EDT_OK;
  });
  if (rc != EDT_OK || empty) return rc;
  ListedDevice on_listed_device;
  if (on_listed_device.rc != EDT_OK) return on_listed_device.rc;
  const size_t voxels = (size_t)(sx * sy * sz), lbytes = voxels * dtype_size(dtype), fbytes = voxels * sizeof(float);
  const size_t wbytes = edt_hip_medial_axis_workspace_bytes(dtype, ndim, sx, sy, sz, flags, radius != nullptr);
  Staging st;
  if ((rc = st.alloc({{kLabels, lbytes}, {kOut, lbytes}, {kWorkspace, wbytes}})) != EDT_OK) return rc;
  if (radius && (rc = st.alloc(kSecondField, fbytes)) != EDT_OK) return rc;
  st.expect(out, lbytes);
  if ((rc = st.up(kLabels, labels, lbytes)) != EDT_OK) return rc;
  rc = edt_hip_medial_axis_device(st.p[kLabels], dtype, ndim, sx, sy, sz, wx, wy, wz, flags, gamma, ratio, st.p[kOut],
                                  radius ? st.at<float>(kSecondField) : nullptr, st.p[kWorkspace], wbytes, nullptr);
  if (rc != EDT_OK || (rc = st.down(out, kOut, lbytes)) != EDT_OK) return rc;
  return radius ? st.down(radius, kSecondField, fbytes) : EDT_OK;
}

}  // extern "C"
