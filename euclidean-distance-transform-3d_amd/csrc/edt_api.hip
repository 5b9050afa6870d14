// edt_api.hip -- the C ABI (include/edt_hip.h), part 1 of 3: the route of a call on device-resident data -- decided once, on
// the host, by route_of --, the workspace carved from it (make_plan), the launches it names (run_device), per-pass event timing,
// the device entry points that are not sharded.  Part 2: edt_host.hip (host-buffer staging); part 3: edt_shard_api.hip (the
// phases of the Z-sharded path).
// No compute happens on the host and there is no CPU fallback: every entry point needs a HIP device.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <system_error>
#include <thread>
#include <vector>

#include <sys/mman.h>

#include "edt_common.h"
#include "edt_kernels.h"

#include "edt_api_internal.h"

namespace edt_amd {

static thread_local std::string g_last_error = "";
// diagnostics mode: thread-local, preset per thread from EDT_HIP_DEBUG_MODE; see edt_common.h for the bits
#ifdef EDT_DIAG
constexpr int kDiagMask = ~0;
#else
constexpr int kDiagMask = kDiagFormBits;
#endif
static int env_debug_mode() {
  static const int v = [] {
    const char *e = std::getenv("EDT_HIP_DEBUG_MODE");
    return e ? (int)std::strtol(e, nullptr, 0) : 0;
  }();
  return v;
}
static thread_local int g_debug_mode = env_debug_mode() & kDiagMask;

void set_error(const std::string &msg) { g_last_error = msg; }
int debug_mode() { return g_debug_mode; }
void set_thread_debug_mode(int mode) { g_debug_mode = mode & kDiagMask; }



// ---- per-pass event timing (bench.py reads this): edt_api_internal.h ------------------
PassLog g_log;
std::mutex g_log_mutex;

hipEvent_t log_event() {
  if (g_log.used == (int)g_log.pool.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    g_log.pool.push_back(e);
  }
  return g_log.pool[g_log.used++];
}

void log_begin_call() {
  g_log.used = 0;
  g_log.span.clear();
  g_log.names.clear();
}




AxisGeom make_geom_y(int64_t sx, int64_t sy, int64_t sz) {
  AxisGeom g;
  g.sx = sx; g.n = sy; g.stride = sx; g.nouter = sz; g.outer_stride = sx * sy;
  g.nbands = ceil_div(sy, kBandRows);
  return g;
}
AxisGeom make_geom_z(int64_t sx, int64_t sy, int64_t sz) {
  AxisGeom g;
  g.sx = sx; g.n = sz; g.stride = sx * sy; g.nouter = sy; g.outer_stride = sx;
  g.nbands = ceil_div(sz, kBandRows);
  return g;
}


// Index form of pass 1 (edt_rowwave.hip C16 -> edt_colwave_kernel.h XF): pass 1 hands the first column pass 2 bytes
// per voxel instead of 4.  The indices live in the workspace, never more than kCodeSlabVoxels of them: passes X and
// Y touch one z-slice at a time, so larger volumes run them slab by slab (a slab of 2^27 voxels is a whole 512^3
// volume's worth of parallelism) -- 256 MiB of scratch whatever the volume.  Shapes: the register-resident pass 1
// and the wave column kernel, rows of whole 8-byte granules.  (debug bit 0x100000 switches the form off.)
constexpr int64_t kCodeSlabVoxels = (int64_t)1 << 27;
// Volumes of several slabs (1024^3: eight) keep the indices of EVERY slab where that costs at most this many bytes (2 GiB at
// 1024^3, against 288 GB of HBM): pass Y then leaves its results in the 16-bit plane there as well and pass Z reads 2 bytes per
// voxel instead of 4 (round 4 measured it at cfg4 and did not keep it for the workspace; round 6 does).  Passes X and Y still run
// slab by slab, so that a slab's indices are read back while they are warm.  EDT_HIP_WHOLE_INDEX_BYTES overrides the limit (0: off).
static int64_t whole_index_limit() {  // (read per route, like the pad below: the route table of the CPU tier sets it per case)
  const char *e = std::getenv("EDT_HIP_WHOLE_INDEX_BYTES");
  return e ? (int64_t)std::strtoll(e, nullptr, 0) : (int64_t)8 << 30;
}
// The pitch of the index buffer = of the 16-bit plane between passes Y and Z (round 6).  Pass Z walks columns whose rows are one
// slice apart: 2 * sx * sy bytes in the plane it reads, 4 * sx * sy in the caller's array it writes.  Where the plane's slice is a
// whole multiple of 1 MiB both streams of a tile fall onto the same few channels at once and the pass loses a third of its rate
// (tools/zorder_probe.hip, profiles/r06_zorder_probe.txt: the bare access pattern at 1024^3 2.10 ms, 1.36 with the plane's slices 8 KiB
// further apart; the caller's 4 MiB stride alone -- stores only -- costs nothing).  The caller's array is not ours; the plane is:
// slices that are a multiple of 2 MiB lie 8 KiB further apart, slices that are a multiple of 1 MiB 4 KiB (8 KiB is the one bad
// choice there), every other shape is left alone (512^3: 512 KiB slices are best as they are).  EDT_HIP_PLANE_PAD_BYTES overrides
// (0: never; a multiple of 8).
static int64_t plane_pad_elems(int64_t sx, int64_t sy) {
  // (read per plan, not once: the test tiers force a pad onto small shapes; a workspace sized under another value is refused
  // by the size check of the call, never overrun)
  const char *e = std::getenv("EDT_HIP_PLANE_PAD_BYTES");
  const int64_t forced = (e && *e) ? (int64_t)std::strtoll(e, nullptr, 0) : (int64_t)-1;
  if (forced >= 0) return (forced & ~(int64_t)7) / 2;
  const int64_t slice = sx * sy * (int64_t)sizeof(uint16_t);
  if (slice % ((int64_t)2 << 20) == 0) return 8192 / 2;
  if (slice % ((int64_t)1 << 20) == 0) return 4096 / 2;
  return 0;
}
constexpr int kQ16Slots = 256;  // counters of the 16-bit integer column kernel's hand-over lists (one per launch)

bool env_force_generic() {
  const char *e = std::getenv("EDT_HIP_FORCE_GENERIC");  // test hook: every call takes the fallback kernels
  return e && e[0] == '1';
}


int check_shape(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz) {
  if (dtype_size(dtype) == 0) { set_error("unknown dtype code"); return EDT_ERR_BAD_ARG; }
  if (ndim < 1 || ndim > 3) { set_error("ndim must be 1, 2 or 3"); return EDT_ERR_BAD_ARG; }
  if (sx < 0 || sy < 0 || sz < 0) { set_error("negative extent"); return EDT_ERR_BAD_ARG; }
  if ((ndim < 3 && sz != 1) || (ndim < 2 && sy != 1)) {
    set_error("unused extents must be 1");
    return EDT_ERR_BAD_ARG;
  }
  if (sx > INT32_MAX || sy > INT32_MAX || sz > INT32_MAX) {
    set_error("extent exceeds 2^31-1");
    return EDT_ERR_UNSUPPORTED;
  }
  return EDT_OK;
}

// Voxel sizes.  The reference does not validate them.  Along x a size enters pass 1 as itself (src/edt.hpp:86-113): a negative
// one makes the unguarded backward fminf sweep cross label boundaries, and NaN / inf / 0 give NaN or all-zero fields; no
// kernel here reproduces that, so such a call is refused instead of answered differently by different kernels.  Along y and
// z a size enters only as its square (w2 = anisotropy * anisotropy, src/edt.hpp:181, :258): a negative wy / wz gives the field
// of |w| there, and does here -- the sign is dropped before anything else looks at it.
static bool voxel_size_usable(float w) { return w > 0.0f && w <= FLT_MAX; }
int check_voxel_sizes(int naxes, float &wx, float &wy, float &wz) {
  float *w[3] = {&wx, &wy, &wz};
  for (int i = 0; i < naxes && i < 3; ++i) {
    if (i > 0) *w[i] = fabsf(*w[i]);
    if (!voxel_size_usable(*w[i])) {
      set_error(i == 0 ? "the voxel size along x must be positive and finite" : "voxel sizes (anisotropy) must be non-zero and finite");
      return EDT_ERR_BAD_ARG;
    }
  }
  return EDT_OK;
}
// the voxel size of a column pass on its own (the Z phase of the sharded path)
int check_column_voxel_size(float &w) {
  w = fabsf(w);
  if (!voxel_size_usable(w)) { set_error("voxel sizes (anisotropy) must be non-zero and finite"); return EDT_ERR_BAD_ARG; }
  return EDT_OK;
}

int check_workspace_alignment(const void *d_workspace) {
  if (reinterpret_cast<uintptr_t>(d_workspace) % kWorkspaceAlign == 0) return EDT_OK;
  set_error("d_workspace must be 256-byte aligned (the alignment of hipMalloc; include/edt_hip.h)");
  return EDT_ERR_BAD_ARG;
}

int require_device() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    set_error("no HIP device available (this library has no CPU fallback)");
    return EDT_ERR_NO_DEVICE;
  }
  return EDT_OK;
}

bool label_op_begin(const char *who, int own_rc, void *d_result, size_t result_words, int64_t voxels, bool null_data,
                    bool aliased, const void *d_workspace, size_t workspace_bytes, size_t needed, const char *query,
                    hipStream_t stream, int *rc) {
  const auto refuse = [&](const std::string &why) {
    set_error(std::string(who) + ": " + why);
    *rc = EDT_ERR_BAD_ARG;
    return false;
  };
  if ((*rc = own_rc) != EDT_OK) return false;
  if (!d_result) return refuse("null device pointer");
  if (voxels > 0) {
    if (null_data) return refuse("null device pointer");
    if (aliased) return refuse("the output may not alias the labels");
    if (!d_workspace || workspace_bytes < needed) return refuse(std::string("workspace missing or smaller than ") + query + "()");
    if ((*rc = check_workspace_alignment(d_workspace)) != EDT_OK) return false;
  }
  if ((*rc = require_device()) != EDT_OK) return false;
  if (voxels == 0) {
    *rc = launch_fill_words(d_result, 0u, result_words * sizeof(int64_t) / sizeof(uint32_t), stream);
    return false;
  }
  if (g_log.enabled.load(std::memory_order_relaxed)) {
    std::lock_guard<std::mutex> lock(g_log_mutex);
    log_begin_call();
  }
  return true;
}


// ---- the route of a call -----------------------------------------------------------------
// Everything a transform decides before its first launch: which kernels run and what lives in which region of the workspace.
// route_of fills it from the call's inputs, the thread's debug mode and the environment hooks, and touches no device; the
// workspace is carved from it (make_plan), run_device executes it, the size and support queries read it, and
// edt_hip_transform_route shows the exported part (include/edt_hip.h documents its fields; DESIGN.md "The route of a call").
struct Route {
  edt_hip_route r = {};
  bool empty = false;         // a volume without voxels: nothing to do
  int dtype = 0, ndim = 0;
  int64_t sx = 0, sy = 0, sz = 0;
  bool zpass = false;         // a 3-D volume that is not a stack of 2-D images: pass Z exists
  bool handover = false;      // the workspace holds the counters, map and id array of the integer column kernel
  bool signed_ok = false;     // EDT_FLAG_SIGNED is served (edt_hip_signed_supported)
  int bb = 0, last_epi = 0;   // the border rule; the epilogue of the call's last pass
  bool last_sqrt = false;
  Quantum Q;                  // the quantum of the voxel sizes, where a column pass may use it
};

// the carved pointers of a route
struct Plan {
  int64_t voxels;
  AxisGeom gy, gz;
  float *bufB = nullptr;
  int32_t *stack = nullptr;
  uint32_t *nz_y = nullptr, *rs_y = nullptr, *zs_y = nullptr, *nz_z = nullptr, *rs_z = nullptr;
  unsigned char *line_ws = nullptr;  // scratch of the line pipeline when pass 1 runs over rows no row kernel takes (> 4096 voxels)
  uint16_t *codes = nullptr;  // 16-bit distance indices of pass 1 (index form): one slab of route.slab slices, or the whole volume
                              // (codes_whole: volumes of several slabs, round 6) -- the 16-bit plane between passes Y and Z then
                              // exists there too
  // the tiles the 16-bit integer column kernel hands to the fp32 kernel (edt_colq16.hip): kQ16Slots counters, one per
  // column-pass launch of a call, and one array of tile ids
  HandOver q16;
  // which tiles of pass Y left their results in the 16-bit plane (= codes): one bit per (x-tile, z), behind the counters
  uint32_t *q16_map = nullptr;
  int q16_map_words = 0;  // words per x-tile
  size_t bytes = 0;
};

// What a call needs besides the bit planes: the second fp32 volume + hull stacks of the size-agnostic column pass (only when an
// axis is too long for the in-place LDS kernels, or the caller forces the generic kernels), and the 16-bit distance indices of
// the index form of pass 1.
static Plan make_plan(const Route &R, void *ws) {
  const edt_hip_route &r = R.r;
  const int64_t sx = R.sx, sy = R.sy, sz = R.sz;
  Plan p;
  p.voxels = sx * sy * sz;
  p.gy = make_geom_y(sx, sy, sz);
  p.gz = make_geom_z(sx, sy, sz);
  const size_t wy = (size_t)(p.gy.sx * p.gy.nbands * p.gy.nouter), wz = (size_t)(p.gz.sx * p.gz.nbands * p.gz.nouter);
  Carver c(ws);
  if (r.second_volume) {
    p.bufB = c.take<float>((size_t)p.voxels);
    p.stack = c.take<int32_t>((size_t)p.voxels);
  }
  if (R.ndim >= 2) {
    p.nz_y = c.take<uint32_t>(wy);
    p.rs_y = c.take<uint32_t>(wy);
  }
  if (R.zpass) {
    // the z-packed planes are built AFTER the y pass: its run-start plane is dead by then and lends its
    // storage to the z run starts (four planes in all: 1/8 byte per voxel each, 0.5 GiB for 1024^3)
    p.nz_z = c.take<uint32_t>(wz);
    if (wz <= wy) p.rs_z = p.rs_y;
    else p.rs_z = c.take<uint32_t>(wz);
    p.zs_y = c.take<uint32_t>(wy);
  }
  if (r.slab > 0) p.codes = c.take<uint16_t>((size_t)((r.codes_whole ? sz : r.slab) * r.code_pitch));
  if (R.handover) {
    // (ids in the fp32 kernel's geometry: 16-column tiles for axes of more than 512 rows)
    // (pass Y runs over all sz slices at once whenever the index form is not taken: sized for that)
    p.q16_map_words = (int)ceil_div(sz, 32);
    p.q16.slots = kQ16Slots;
    // (one region, two rules: the counters are zeroed on the stream before the first launch that may hand a tile over,
    // HandOver::zero; the map behind them never is -- every tile of a pass that writes the plane sets or clears its own bit)
    p.q16.counts = c.take<uint32_t>(kQ16Slots + (size_t)(ceil_div(sx, 32) * p.q16_map_words));
    p.q16_map = p.q16.counts ? p.q16.counts + kQ16Slots : nullptr;
    p.q16.capacity = std::max(HandOver::ids_of(sx, sz), HandOver::ids_of(sx, sy));
    p.q16.ids = c.take<uint32_t>((size_t)p.q16.capacity);
  }
  if (R.ndim == 1) (void)c.take<unsigned char>(line_workspace_bytes(sx));  // block scan + table of the 1-D pipeline
  // rows too long for the row kernels (more than 4096 voxels; more than 2048 where the wave kernel does not apply): pass 1
  // runs as the line pipeline over the stack of rows and needs its scratch
  if (R.ndim >= 2 && r.x_kernel == EDT_ROUTE_X_LINE) p.line_ws = c.take<unsigned char>(rows_line_workspace_bytes(sx, sy * sz));
  p.bytes = align_up(c.off, 256) + 256;
  return p;
}

// The one place that decides.  Returns what the call refuses with before its first launch, in the order the refusals always
// had: shape, voxel sizes (their signs dropped: wy, wz), [an empty volume: EDT_OK], the data pointers (null_data), the workspace,
// EDT_FLAG_SIGNED, EDT_FLAG_BATCH_2D.  ws_bytes: the workspace the caller brought (0: none).  out_misalignment: d_out's address
// modulo 16 -- all column_pass_q16_aligned needs: the workspace is 256-aligned (check_workspace_alignment; internal callers
// hand in carved regions) and every region of the carve is, and where the index form exists sx % 4 == 0, so a slab's part of
// the field (z0 * sx * sy floats: a multiple of 16 bytes) and of the index buffer (z0 * code_pitch indices: sx * sy and the pad
// are multiples of 4 elements, 8 bytes) keeps the alignment of its base.  What is filled when a refusal comes stays filled:
// the size and support queries read it.
static int route_of(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float &wx, float &wy, float &wz, int flags,
                    bool null_data, size_t ws_bytes, uint32_t out_misalignment, Route &R) {
  R = Route();
  int rc = check_shape(dtype, ndim, sx, sy, sz);
  if (rc != EDT_OK) return rc;
  if ((rc = check_voxel_sizes(ndim, wx, wy, wz)) != EDT_OK) return rc;
  if (sx == 0 || sy == 0 || sz == 0) { R.empty = true; return EDT_OK; }
  if (null_data) { set_error("null device pointer"); return EDT_ERR_BAD_ARG; }
  edt_hip_route &r = R.r;
  R.dtype = dtype; R.ndim = ndim; R.sx = sx; R.sy = sy; R.sz = sz;
  const int mode = g_debug_mode;
  const bool generic = (flags & EDT_FLAG_FORCE_GENERIC) != 0 || env_force_generic();
  // a stack of 2-D images is a volume without a z pass
  R.zpass = ndim == 3 && !(flags & EDT_FLAG_BATCH_2D);
  R.bb = (flags & EDT_FLAG_BLACK_BORDER) ? 1 : 0;
  R.last_sqrt = (flags & EDT_FLAG_SQRT) != 0;
  R.last_epi = last_pass_epi(R.bb, R.last_sqrt ? 1 : 0);
  const AxisGeom gy = make_geom_y(sx, sy, sz), gz = make_geom_z(sx, sy, sz);

  // The kernels the shape allows.  Pass 1 on the row kernels: the register kernel up to 4096 voxels per row, the
  // workgroup-phased one up to 2048 (debug bit 32: never the former); longer rows: the line pipeline; forced generic: a thread
  // per row.  Column passes are in place when an LDS-tiled kernel applies, otherwise they ping-pong between two volumes.
  const bool row_kernels = ndim >= 2 && row_pass_on_row_kernels(dtype, sx, sy, sz, generic);
  const bool register_x = row_kernels && row_pass_wave_supported(dtype, sx, sy, sz) && !(mode & kDbgTiledRows);
  const bool tiled_y = ndim >= 2 && !generic && column_inplace_supported(gy);
  const bool tiled_z = R.zpass && !generic && column_inplace_supported(gz);
  r.x_kernel = register_x ? EDT_ROUTE_X_REGISTER : row_kernels ? EDT_ROUTE_X_PHASED : generic ? EDT_ROUTE_X_SERIAL : EDT_ROUTE_X_LINE;
  r.planes_from_labels = ndim >= 2 && !row_kernels;
  r.second_volume = ndim >= 2 && (!tiled_y || (R.zpass && !tiled_z));
  R.handover = ndim >= 2 && !generic;
  // The one-transform form of sdf / sdfsq needs pass X on the register kernel (the only pass-X kernel that takes zero_label)
  // and in-place column passes (their kernels never look at label values: run-start bits and field values only).
  R.signed_ok = register_x && tiled_y && (!R.zpass || tiled_z) && !(flags & EDT_FLAG_BINARY_YZ);

  // The index buffer (see kCodeSlabVoxels): the register kernel of pass X and the wave column kernel, rows of whole 8-byte
  // granules.  Several slabs: whole words of the per-slice map of the 16-bit plane per slab.  A padded pitch only where the
  // plane exists -- a whole-volume buffer of a 3-D call; a single slice needs none.
  const auto index_buffer = [&](bool wanted) {
    r.slab = 0;
    if (wanted && register_x && sx % 4 == 0 && sx * sy <= kCodeSlabVoxels && column_pass_wave_supported(gy) &&
        !(mode & (kDbgFp32PassX | kDbgTiledColumns))) {
      r.slab = std::min(kCodeSlabVoxels / (sx * sy), sz);
      if (r.slab < sz && r.slab >= 32) r.slab &= ~(int64_t)31;
    }
    r.codes_whole = r.slab >= sz || (r.slab > 0 && r.slab % 32 == 0 && R.zpass && sx * sy * sz * (int64_t)sizeof(uint16_t) <= whole_index_limit());
    r.code_pitch = ndim >= 2 ? sx * sy + ((r.codes_whole && R.zpass && sz > 1) ? plane_pad_elems(sx, sy) : 0) : 0;
    r.workspace_bytes = make_plan(R, nullptr).bytes;
  };
  index_buffer(!(flags & EDT_FLAG_SMALL_WORKSPACE));
  // (a workspace sized while the index form of pass 1 was switched off still serves: fp32 form)
  if (ws_bytes != 0 && ws_bytes < r.workspace_bytes && r.slab > 0) {
    index_buffer(false);
    r.index_fallback = 1;
  }
  // (1-D: the parallel line pipeline needs its block-scan scratch; a call without any -- the ABI of round 1 -- is
  // served by the thread-per-row kernel instead of being refused)
  if (ws_bytes < r.workspace_bytes && ndim != 1) {
    set_error("workspace too small: need " + std::to_string(r.workspace_bytes) +
              " bytes (edt_hip_workspace_bytes_flags with the flags of this call)");
    return EDT_ERR_BAD_ARG;
  }
  // The SIGNED transform (EDT_FLAG_SIGNED; sdf / sdfsq of src/edt.pyx:121-202 = edt(x) - edt(x == 0)) as ONE transform: the
  // two fields have disjoint supports, and a voxel's value depends on nothing but the voxels of its own label runs -- so
  // measuring label 0 like every other label gives edt(x) on the foreground and edt(x == 0) on the background at once, bit
  // for bit; the background's sign follows in one streaming kernel.  Pass X's register kernel takes the flag (zero_label).
  const bool signed_tf = (flags & EDT_FLAG_SIGNED) != 0;
  if (signed_tf && !R.signed_ok) {
    set_error("EDT_FLAG_SIGNED: shape not served by the one-transform form (edt_hip_signed_supported)");
    return EDT_ERR_UNSUPPORTED;
  }
  if ((flags & EDT_FLAG_BATCH_2D) && ndim != 3) { set_error("EDT_FLAG_BATCH_2D needs ndim = 3 (sz = image count)"); return EDT_ERR_BAD_ARG; }
  r.slabs = 1;
  if (ndim == 1) {  // (pass X is the call's last pass; one thread for the whole line only where forced, or without scratch)
    if (ws_bytes < r.workspace_bytes) r.x_kernel = EDT_ROUTE_X_SERIAL;
    return EDT_OK;
  }
  // the reference's binary route for multi-valued labels: labels split runs in pass 1 only (edt_generic.hip:
  // k_planes_one_run).  Boolean input gives the same values either way and keeps the ordinary planes.
  r.binary_yz = (flags & EDT_FLAG_BINARY_YZ) != 0 && dtype != EDT_BOOL;
  // Start in the buffer that makes the last pass land in d_out.
  r.first_buffer = ((tiled_y ? 0 : 1) + ((R.zpass && !tiled_z) ? 1 : 0)) % 2;
  // Index form of pass 1: pass 1 stores 16-bit distance indices, the first column pass turns them into F while it fills its
  // tile -- 2 B less written and 2 B less read per voxel.  Bit-identical only where every multiple k * wx of the row is exact
  // in fp32 (row_codes_exact); other voxel sizes keep the fp32 form.
  r.index_form = r.slab > 0 && row_codes_exact(wx, sx);
  if (r.index_form) r.slabs = ceil_div(sz, r.slab);

  // The 16-bit integer form of the column passes (edt_colq16.hip): voxel sizes that share a quantum.  Every column pass is
  // then two launches: the integer kernel over all tiles, and the fp32 kernel over the list of tiles it refused -- unless the
  // host proves that list empty (q16_no_refusals): in the index form for pass Y, behind such a pass Y for pass Z.  The field a
  // pass works on: pass Y on the first buffer, an in-place pass Z on d_out.  Its counter: one per launch, pass Y's slabs first.
  if (R.handover) {
    const float w3[3] = {wx, wy, wz};
    R.Q = q16_quantum(w3, R.zpass ? 3 : 2);
  }
  static uint32_t planned;  // (the counters of the plan: column_pass_q16_applies asks whether they exist)
  HandOver h;
  h.counts = &planned;
  h.slots = kQ16Slots;
  h.slot = (int)std::min<int64_t>(r.slabs - 1, kQ16Slots);
  const bool out_aligned = out_misalignment % 16 == 0;
  const bool y_integer = tiled_y && (r.first_buffer == 1 || out_aligned) && column_pass_q16_applies(R.Q, gy, h);
  r.y_pass = !tiled_y ? EDT_ROUTE_COL_SERIAL : !y_integer ? EDT_ROUTE_COL_FP32
             : (r.index_form && q16_no_refusals(R.Q, 1, sx, sy, sy, R.bb)) ? EDT_ROUTE_COL_INTEGER_ALONE : EDT_ROUTE_COL_INTEGER_LIST;
  h.slot = y_integer ? (int)r.slabs : 0;
  const bool z_integer = tiled_z && out_aligned && column_pass_q16_applies(R.Q, gz, h);
  r.z_pass = !R.zpass ? EDT_ROUTE_COL_NONE : !tiled_z ? EDT_ROUTE_COL_SERIAL : !z_integer ? EDT_ROUTE_COL_FP32
             : (r.y_pass == EDT_ROUTE_COL_INTEGER_ALONE && q16_no_refusals(R.Q, 2, sx, sy, sz, R.bb)) ? EDT_ROUTE_COL_INTEGER_ALONE
                                                                                                     : EDT_ROUTE_COL_INTEGER_LIST;
  const bool integer_only = r.y_pass == EDT_ROUTE_COL_INTEGER_ALONE && r.z_pass == EDT_ROUTE_COL_INTEGER_ALONE;
  const bool keep_planes = (mode & kDbgKeepPlanes) != 0;
  // The 16-bit plane between passes Y and Z: where both run on the integer kernel and the indices of pass X cover the whole
  // volume, the tiles of pass Y that qualify write their results over their indices -- 2 bytes per voxel out of pass Y and
  // into pass Z instead of 4 -- and pass Z reads every row from wherever pass Y left it.  (debug bit 0x10000000: fp32 between
  // the passes.)  plane_inf_ok: may a tile of nothing but +inf stay there for pass Z?
  r.plane16 = r.index_form && r.codes_whole && y_integer && z_integer && !(mode & kDbgFp32Plane);
  r.plane_inf_ok = r.plane16 && q16_value_limit(R.Q.q, R.Q.a[2], sz, R.bb) != 0u;
  // The signed transform's sign as the EPILOGUE of pass Z (round 6): where both column passes provably run on the integer kernel
  // alone -- it never reads the foreground plane -- pass X keeps the TRUE label != 0 bits there (zero_label = 2), the transposer
  // carries them to the z axis, and the last pass negates the voxels whose bit is clear (kEpiSign): no pass of its own over
  // labels and field (1.2 GB at 512^3).  Anywhere else: all-ones planes and k_negate_background.  (debug bit 0x400: never.)
  r.sign = !signed_tf ? 0 : (integer_only && !keep_planes) ? 1 : 2;
  r.zero_label = !signed_tf ? 0 : r.sign == 1 ? 2 : 1;
  // ... and then nobody reads a foreground plane (the integer kernel knows background as N = 0): pass X does not write one, the
  // transposer carries the run starts alone -- 48 MiB less per 512^3 step (debug bit 0x400 keeps the planes)
  r.skip_nz = integer_only && !signed_tf && !r.binary_yz && !keep_planes;
  // ... and then the storage of the y foreground plane is nobody's: it takes the ROW FLAGS.  Pass X does not store the indices of
  // a row without a run start -- its indices follow from x alone -- and says so in two words per (z, band of 32 rows), [z][band]
  // [plain, plain_fg], the first 2 * bands * sz words of nz_y (which has sx words per (z, band): sx >= 4 here); pass Y puts the
  // indices back while it fills its tile (edt_colq16.hip: q16_plain_quad).  Written by pass X, both words of every group, so the
  // region needs no clearing.  Only where nothing else reads the indices: the integer kernel alone (the fp32 kernel reads them
  // too and knows nothing of the flags), unsigned and not binary_yz (skip_nz), one slab of indices, rows of one wave
  // (sx <= 1024).  Everything else hands both kernels nullptr and stores every row.  (debug bit 0x800000: every row is stored.)
  r.row_flags = r.skip_nz && r.slabs == 1 && sx <= 1024 && !(mode & kDbgStoreEveryRow);
  return EDT_OK;
}

// ---- the pass pipeline on device-resident data: the launches the route names, in order -----------------------------------
int run_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz,
                      float wx, float wy, float wz, int flags, float *d_out, void *d_ws,
                      size_t ws_bytes, hipStream_t stream) {
  Route R;
  int rc = route_of(dtype, ndim, sx, sy, sz, wx, wy, wz, flags, !d_labels || !d_out, d_ws ? ws_bytes : 0,
                    (uint32_t)(reinterpret_cast<uintptr_t>(d_out) % 16), R);
  if (rc != EDT_OK || R.empty) return rc;
  const edt_hip_route &r = R.r;
  Plan p = make_plan(R, d_ws);
  // lower bounds of the non-zero values passes Y and Z read (AxisGeom::fmin): pass X leaves fl32(T[k]^2) >= fl32(wx^2),
  // pass Y's results are at least the smaller of that and fl32(wy^2) (every candidate is its row's own value or carries
  // a c_d >= w2y; the border terms are >= w2y).  Not for the fused sqrt of a 2-D call (pass Z does not exist then).
  p.gy.fmin = edt_hip_field_floor(wx, wx);
  p.gz.fmin = edt_hip_field_floor(wx, wy);

  // the pass log is process-wide and only touched (under its mutex) while profiling is switched on
  if (g_log.enabled.load(std::memory_order_relaxed)) {
    std::lock_guard<std::mutex> lock(g_log_mutex);
    log_begin_call();
  }

  // a column pass of this call over the field at F, in place: run_column_pass (edt_colpass.hip) is handed what the route
  // decided -- the quantum only where the integer kernel is to run, `sure` only where it is to run alone -- and a pass that
  // did anything else is an internal error
  const auto column = [&](float *F, const uint32_t *nz, const uint32_t *rs, const AxisGeom &g, float w, int epi) {
    ColumnPass cp = column_pass(F, nz, rs, g, w, R.bb, epi, stream);
    cp.map = p.q16_map;
    cp.map_words = p.q16_map_words;
    return cp;
  };
  const auto run_column = [&](const ColumnPass &cp, int axis, int kind, Fp32Leg leg) -> int {
    TileList served;
    const int rc = run_column_pass(cp, kind >= EDT_ROUTE_COL_INTEGER_LIST ? R.Q : Quantum(), axis, p.q16, leg,
                                   kind == EDT_ROUTE_COL_INTEGER_ALONE, &served);
    if (rc != EDT_OK) return rc;
    if ((served.count != nullptr) == (kind >= EDT_ROUTE_COL_INTEGER_LIST) && served.none == (kind == EDT_ROUTE_COL_INTEGER_ALONE)) return EDT_OK;
    set_error(axis == 1 ? "internal: pass Y left its route" : "internal: pass Z left its route");
    return EDT_ERR_HIP;
  };

  // pass X of this call: the whole volume into the field at `out` (the index form below works slab by slab)
  RowPass rp = row_pass(dtype, d_labels, sx, sy, sz, wx, R.bb, stream);

  if (r.y_pass == EDT_ROUTE_COL_NONE) {  // (a line: pass X is the call's last pass)
    rp.out = d_out; rp.last = true; rp.last_sqrt = R.last_sqrt;
    return run_row_pass(rp, false, r.x_kernel == EDT_ROUTE_X_LINE ? d_ws : nullptr, true);
  }

  float *cur = r.first_buffer ? p.bufB : d_out;
  float *other = r.first_buffer ? d_out : p.bufB;
  const bool row_kernels = !r.planes_from_labels;
  const int y_epi = R.zpass ? 0 : R.last_epi;
  uint32_t *const nzy = r.skip_nz ? nullptr : p.nz_y, *const nzz = r.skip_nz ? nullptr : p.nz_z;
  uint32_t *const rowflags = r.row_flags ? p.nz_y : nullptr;
  if (r.index_form) {
    const int64_t sxy = sx * sy, wpl = p.gy.sx * p.gy.nbands;  // voxels / bit words per slice
    const size_t lsz = dtype_size(dtype);
    const bool one = r.slabs == 1;
    ScopedPass whole(one ? nullptr : "xy_pass", stream);
    for (int64_t z0 = 0; z0 < sz; z0 += r.slab) {
      const int64_t zc = std::min<int64_t>(r.slab, sz - z0);
      const char *lab = static_cast<const char *>(d_labels) + (size_t)(z0 * sxy) * lsz;
      // (one slab of indices taken in turn, or -- codes_whole -- every slab's own part of a whole-volume buffer: the 16-bit plane)
      uint16_t *slab_codes = p.codes + ((r.codes_whole && !one) ? z0 * r.code_pitch : 0);
      {
        // (slice 0 of a later slab compares against the slice below it through the halo pointer of the sharded path)
        ScopedPass t(one ? "x_pass" : nullptr, stream);
        RowPass slab = rp;
        slab.labels = lab; slab.halo = z0 > 0 ? lab - (size_t)sxy * lsz : nullptr; slab.sz = zc;
        slab.nz_y = nzy ? nzy + z0 * wpl : nullptr; slab.ys_y = p.rs_y + z0 * wpl; slab.zs_y = R.zpass ? p.zs_y + z0 * wpl : nullptr;
        slab.codes = slab_codes; slab.codes_pitch = r.code_pitch; slab.zero_label = r.zero_label;
        slab.rowflags = rowflags;
        if ((rc = launch_row_pass_wave(slab)) != EDT_OK) return rc;
        if (r.binary_yz) {
          AxisGeom gb = p.gy;
          gb.nouter = zc;
          rc = launch_planes_one_run(p.nz_y + z0 * wpl, p.rs_y + z0 * wpl, R.zpass ? p.zs_y + z0 * wpl : nullptr, gb, z0, stream);
          if (rc != EDT_OK) return rc;
        }
      }
      {
        ScopedPass t(one ? "y_pass" : nullptr, stream);
        ColumnPass cp = column(cur + z0 * sxy, p.nz_y + z0 * wpl, p.rs_y + z0 * wpl, p.gy, wy, y_epi);
        cp.g.nouter = zc;
        cp.codes = slab_codes;
        cp.codes_outer = r.code_pitch;  // (the index buffer's own pitch: the outer stride of codes -- and of the plane written over them)
        cp.wx = wx;
        cp.rowflags = rowflags;
        cp.plane = r.plane16 ? slab_codes : nullptr;
        // (the slab's first word in every x-tile's row of the plane's map: pass Y of the slabs after the first)
        if (r.codes_whole && !one) cp.map += z0 / 32;
        cp.plane_inf_ok = r.plane_inf_ok;
        if ((rc = run_column(cp, 1, r.y_pass, Fp32Leg::wave)) != EDT_OK) return rc;
      }
    }
  } else {
    // (the signed form -- the register kernel of pass X serves this shape -- measures label 0 too)
    rp.out = cur; rp.nz_y = p.nz_y; rp.ys_y = p.rs_y; rp.zs_y = (R.zpass && row_kernels) ? p.zs_y : nullptr; rp.zero_label = r.zero_label;
    if ((rc = run_row_pass(rp, row_kernels, p.line_ws, true)) != EDT_OK) return rc;
    if (r.binary_yz) rc = launch_planes_one_run(p.nz_y, p.rs_y, rp.zs_y, p.gy, 0, stream);
    if (rc != EDT_OK) return rc;
    ScopedPass t("y_pass", stream);
    if (r.y_pass == EDT_ROUTE_COL_SERIAL) {
      rc = launch_column_pass_serial(cur, other, p.nz_y, p.rs_y, p.stack, p.gy, wy, R.bb, y_epi, stream);
      std::swap(cur, other);
    } else {
      // (fp32 values of pass X: (k * wx)^2 need not be on the quantum grid for large k -- the list stays)
      rc = run_column(column(cur, p.nz_y, p.rs_y, p.gy, wy, y_epi), 1, r.y_pass, Fp32Leg::inplace);
    }
    if (rc != EDT_OK) return rc;
  }
  if (R.zpass) {
    // z-packed planes (after the y pass: rs_z may live in the y pass's run-start plane)
    ScopedPass t("z_bits", stream);
    if (row_kernels) rc = launch_bits_transpose_yz(nzy, p.zs_y, nzz, p.rs_z, sx, sy, sz, stream);
    else {
      rc = launch_axis_bits(dtype, d_labels, nullptr, p.nz_z, p.rs_z, p.gz, stream);
      if (rc == EDT_OK && r.binary_yz) rc = launch_planes_one_run(p.nz_z, p.rs_z, nullptr, p.gz, 0, stream);
    }
    if (rc != EDT_OK) return rc;
  }
  if (R.zpass) {
    ScopedPass t("z_pass", stream);
    if (r.z_pass == EDT_ROUTE_COL_SERIAL) {
      rc = launch_column_pass_serial(cur, other, p.nz_z, p.rs_z, p.stack, p.gz, wz, R.bb, R.last_epi, stream);
      std::swap(cur, other);
    } else {
      ColumnPass cp = column(cur, p.nz_z, p.rs_z, p.gz, wz, R.last_epi | (r.sign == 1 ? kEpiSign : 0));
      if (r.plane16) {  // (the index buffer's own pitch: the row stride of the plane pass Z reads)
        cp.plane = p.codes;
        cp.plane_stride = r.code_pitch;
        cp.plane_outer = sx;
      }
      cp.signbits = r.sign == 1 ? p.nz_z : nullptr;
      rc = run_column(cp, 2, r.z_pass, Fp32Leg::inplace);
    }
    if (rc != EDT_OK) return rc;
  }
  if (cur != d_out) { set_error("internal: result buffer mismatch"); return EDT_ERR_HIP; }
  if (r.sign == 2) {
    ScopedPass t("sign", stream);
    rc = launch_negate_background(dtype, d_labels, d_out, p.voxels, stream);
    if (rc != EDT_OK) return rc;
  }
  return EDT_OK;
}

// the route of the call with a workspace of whatever size it asks for (the size and support queries; voxel sizes play no part in either)
static Route route_for_query(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags) {
  Route R;
  float wx = 1.0f, wy = 1.0f, wz = 1.0f;
  (void)route_of(dtype, ndim, sx, sy, sz, wx, wy, wz, flags, false, SIZE_MAX, 0, R);
  return R;
}

bool signed_transform_supported(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags) {
  return route_for_query(dtype, ndim, sx, sy, sz, flags).signed_ok;
}

const char *last_error_cstr() { return g_last_error.c_str(); }

}  // namespace edt_amd

using namespace edt_amd;

extern "C" {

int edt_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

const char *edt_hip_last_error(void) { return last_error_cstr(); }

int edt_hip_index_form_exact(float wx, int64_t sx) { return (sx >= 1 && row_codes_exact(wx, sx)) ? 1 : 0; }

const char *edt_hip_version(void) { return "edt_hip 0.1 (gfx950)"; }

size_t edt_hip_workspace_bytes_flags(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags) {
  const Route R = route_for_query(dtype, ndim, sx, sy, sz, flags);
  return R.empty ? 256 : (size_t)R.r.workspace_bytes;  // (0: a shape every call refuses)
}

int edt_hip_signed_supported(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags) {
  return signed_transform_supported(dtype, ndim, sx, sy, sz, flags) ? 1 : 0;
}

int edt_hip_transform_route(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz, int flags,
                            size_t workspace_bytes, uint32_t out_misalignment, edt_hip_route *route) {
  Route R;
  const int rc = route_of(dtype, ndim, sx, sy, sz, wx, wy, wz, flags, false, workspace_bytes, out_misalignment, R);
  *route = rc == EDT_OK ? R.r : edt_hip_route{};
  return rc;
}

size_t edt_hip_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz) {
  return edt_hip_workspace_bytes_flags(dtype, ndim, sx, sy, sz, 0);
}

int edt_hip_edtsq_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy,
                         int64_t sz, float wx, float wy, float wz, int flags, float *d_output,
                         void *d_workspace, size_t workspace_bytes, void *stream) {
  if (check_workspace_alignment(d_workspace) != EDT_OK) return EDT_ERR_BAD_ARG;
  return run_device(d_labels, dtype, ndim, sx, sy, sz, wx, wy, wz, flags, d_output, d_workspace,
                    workspace_bytes, (hipStream_t)stream);
}

int edt_hip_set_debug_mode(int mode) {
  set_thread_debug_mode(mode);
  return EDT_OK;
}

int edt_hip_get_debug_mode(void) { return debug_mode(); }

int edt_hip_q16_no_refusals(int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz, int ndim, int black_border,
                            int *pass_y, int *pass_z) {
  if (pass_y) *pass_y = 0;
  if (pass_z) *pass_z = 0;
  if (ndim < 2 || ndim > 3 || sx < 1 || sy < 1 || (ndim == 3 && sz < 1)) return 0;
  const float w3[3] = {wx, wy, wz};
  const Quantum Q = q16_quantum(w3, ndim);
  if (!Q.ok) return 0;
  const bool y = q16_no_refusals(Q, 1, sx, sy, sy, black_border);
  const bool z = ndim == 3 && y && q16_no_refusals(Q, 2, sx, sy, sz, black_border);
  if (pass_y) *pass_y = y ? 1 : 0;
  if (pass_z) *pass_z = z ? 1 : 0;
  return 1;
}

int edt_hip_set_profiling(int enabled) {
  std::lock_guard<std::mutex> lock(g_log_mutex);
  g_log.enabled.store(enabled != 0);
  log_begin_call();  // the shard phases append to the log (several calls make one step): start clean
  return EDT_OK;
}

int edt_hip_get_pass_times(float *ms, int capacity) {
  std::lock_guard<std::mutex> lock(g_log_mutex);
  int n = (int)g_log.span.size();
  for (int i = 0; i < n && i < capacity; ++i) {
    float t = 0.0f;
    if (hipEventElapsedTime(&t, g_log.pool[g_log.span[i].first], g_log.pool[g_log.span[i].second]) !=
        hipSuccess) {
      (void)hipGetLastError();
      t = -1.0f;
    }
    ms[i] = t;
  }
  return n;
}

const char *edt_hip_get_pass_name(int index) {
  std::lock_guard<std::mutex> lock(g_log_mutex);
  if (index < 0 || index >= (int)g_log.names.size()) return "";
  return g_log.names[index].c_str();
}

// min(fl32(wx*wx), fl32(wy*wy)): what every non-zero value of a field is at least after passes X and Y (run_device has
// the argument); 0 where a voxel size is not a positive finite number
float edt_hip_field_floor(float wx, float wy) {
  const float a = wx * wx, b = wy * wy;
  if (!(a > 0.0f) || !(b > 0.0f) || !(a < INFINITY) || !(b < INFINITY)) return 0.0f;
  return a < b ? a : b;
}

int edt_hip_subtract_device(const float *d_a, const float *d_b, float *d_out, int64_t count,
                            void *stream) {
  return launch_subtract(d_a, d_b, d_out, count, (hipStream_t)stream);
}

// Voxel-graph transform on device-resident data.  Native form (edt_voxel_graph.hip: no doubled volume) where
// the wave column kernel covers the doubled axes, else the up-sampled form: workspace = [2x uint8 volume |
// its fp32 transform | the ordinary workspace of the 2x volume].  Debug bit 0x20000 forces the latter.
static bool vg_use_native(int ndim, int64_t sx, int64_t sy, int64_t sz) {
  return !(g_debug_mode & kDbgVgUpsampled) && vg_native_supported(ndim, sx, sy, sz);
}

size_t edt_hip_voxel_graph_workspace_bytes(int ndim, int64_t sx, int64_t sy, int64_t sz) {
  if (check_shape(EDT_U8, ndim, sx, sy, sz) != EDT_OK || ndim < 2) return 0;
  if (sx == 0 || sy == 0 || sz == 0) return 256;
  if (vg_use_native(ndim, sx, sy, sz)) return vg_native_workspace_bytes(ndim, sx, sy, sz);
  const int64_t X = 2 * sx, Y = 2 * sy, Z = (ndim == 3) ? 2 * sz : 1;
  const size_t big = (size_t)(X * Y * Z);
  return align_up(big, 256) + align_up(big * sizeof(float), 256) + edt_hip_workspace_bytes(EDT_U8, ndim, X, Y, Z) + 256;
}

int edt_hip_edtsq_voxel_graph_device(const void *d_labels, int dtype, const uint8_t *d_graph, int ndim,
                                     int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                                     int flags, float *d_output, void *d_workspace, size_t workspace_bytes,
                                     void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_shape(dtype, ndim, sx, sy, sz);
  if (rc != EDT_OK) return rc;
  if ((rc = check_voxel_sizes(ndim, wx, wy, wz)) != EDT_OK) return rc;
  if (ndim < 2) { set_error("voxel_graph needs a 2-D or 3-D volume"); return EDT_ERR_BAD_ARG; }
  if (sx == 0 || sy == 0 || sz == 0) return EDT_OK;
  if (!d_labels || !d_graph || !d_output) { set_error("null device pointer"); return EDT_ERR_BAD_ARG; }
  const size_t need = edt_hip_voxel_graph_workspace_bytes(ndim, sx, sy, sz);
  if (!d_workspace || workspace_bytes < need) {
    set_error("workspace too small: need " + std::to_string(need) + " bytes");
    return EDT_ERR_BAD_ARG;
  }
  if ((rc = check_workspace_alignment(d_workspace)) != EDT_OK) return rc;
  const int bb = (flags & EDT_FLAG_BLACK_BORDER) ? 1 : 0;
  if (vg_use_native(ndim, sx, sy, sz)) {
    ScopedPass t("voxel_graph", stream);
    return launch_vg_native(dtype, d_labels, d_graph, ndim, sx, sy, sz, wx, wy, wz, bb,
                            (flags & EDT_FLAG_SQRT) ? 1 : 0, d_output, d_workspace, stream);
  }
  const int64_t X = 2 * sx, Y = 2 * sy, Z = (ndim == 3) ? 2 * sz : 1;
  const size_t big = (size_t)(X * Y * Z);
  Carver c(d_workspace);
  uint8_t *d_big = c.take<uint8_t>(big);
  float *d_bigdt = c.take<float>(big);
  const size_t wbytes = edt_hip_workspace_bytes(EDT_U8, ndim, X, Y, Z);
  void *d_ws = c.take<unsigned char>(wbytes);
  rc = launch_vg_expand(dtype, d_labels, d_graph, d_big, sx, sy, sz, ndim, bb, stream);
  if (rc != EDT_OK) return rc;
  // half voxel size on the 2x grid (src/edt_voxel_graph.hpp:96-101, :189-193)
  rc = run_device(d_big, EDT_U8, ndim, X, Y, Z, wx / 2, wy / 2, wz / 2,
                  (bb ? EDT_FLAG_BLACK_BORDER : 0) | (flags & EDT_FLAG_SQRT), d_bigdt, d_ws, wbytes, stream);
  if (rc != EDT_OK) return rc;
  return launch_vg_gather(d_bigdt, d_output, sx, sy, sz, ndim, stream);
}

int edt_hip_select_label_device(const void *d_labels, int dtype, const float *d_dt, const void *key,
                                float *d_out, int64_t count, void *stream) {
  if (count < 0 || dtype_size(dtype) == 0) { set_error("bad argument"); return EDT_ERR_BAD_ARG; }
  if (count == 0) return EDT_OK;
  if (!d_labels || !d_dt || !d_out || !key) { set_error("null pointer"); return EDT_ERR_BAD_ARG; }
  return launch_select_label(dtype, d_labels, d_dt, d_out, key, count, (hipStream_t)stream);
}

size_t edt_hip_runs_workspace_bytes(int64_t count) { return count < 0 ? 0 : runs_workspace_bytes(count); }

int edt_hip_extract_runs_device(const void *d_labels, int dtype, int64_t count, int64_t *d_starts, int64_t capacity,
                                int64_t *d_count, void *d_workspace, size_t workspace_bytes, void *stream) {
  if (count < 0 || capacity < 0 || dtype_size(dtype) == 0) { set_error("bad argument"); return EDT_ERR_BAD_ARG; }
  if (!d_count) { set_error("null pointer"); return EDT_ERR_BAD_ARG; }
  if (count == 0) return launch_fill_words(d_count, 0u, sizeof(int64_t) / sizeof(uint32_t), (hipStream_t)stream);
  if (!d_labels || !d_workspace || workspace_bytes < runs_workspace_bytes(count)) {
    set_error("null pointer or workspace too small (edt_hip_runs_workspace_bytes)");
    return EDT_ERR_BAD_ARG;
  }
  if (check_workspace_alignment(d_workspace) != EDT_OK) return EDT_ERR_BAD_ARG;
  return launch_extract_runs(dtype, d_labels, count, d_starts, capacity, d_count, d_workspace, (hipStream_t)stream);
}

int edt_hip_is_background_device(const void *d_labels, int dtype, uint8_t *d_mask, int64_t count,
                                 void *stream) {
  return launch_is_background(dtype, d_labels, d_mask, count, (hipStream_t)stream);
}

}  // extern "C"
