// edt_shard_api.hip -- the C ABI (include/edt_hip.h), part 3 of 3: the two phases of the Z-sharded path as entry points
// on device-resident slabs (byte flags; slab records of fp32 rows; slab records of 16-bit rows).  The kernels are in
// edt_shard.hip and the column / row kernels; the driver above them is edt/distributed.py (one process per GPU) or
// edt_multi.hip (one process, several GPUs).
#include "edt_api_internal.h"

namespace edt_amd {

// ---- Z-sharded phases ------------------------------------------------------------------------
struct ShardPlan {
  float *bufB = nullptr;
  int32_t *stack = nullptr;
  uint32_t *nz = nullptr, *rs = nullptr;
  size_t bytes = 0;
};

static int check_shard_workspace(const void *ws, size_t have, size_t need) {
  if (ws && have >= need) return check_workspace_alignment(ws);
  set_error("shard workspace too small: need " + std::to_string(need) + " bytes");
  return EDT_ERR_BAD_ARG;
}

static ShardPlan make_shard_plan(int64_t sx, int64_t sy, int64_t sz, void *ws) {
  // sized for the larger of the two phases run on an (sx, sy, sz) block
  ShardPlan p;
  Carver c(ws);
  const int64_t voxels = sx * sy * sz;
  p.bufB = c.take<float>((size_t)voxels);
  p.stack = c.take<int32_t>((size_t)voxels);
  const AxisGeom gy = make_geom_y(sx, sy, sz), gz = make_geom_z(sx, sy, sz);
  const size_t words = (size_t)std::max(gy.sx * gy.nbands * gy.nouter, gz.sx * gz.nbands * gz.nouter);
  p.nz = c.take<uint32_t>(words);
  p.rs = c.take<uint32_t>(words);
  p.bytes = align_up(c.off, 256) + 256;
  return p;
}

// ---- slab records: the fast variant of the two sharded phases (edt_shard.hip) -------------------
static int64_t record_floats(int64_t sx, int64_t ylen) {
  return ylen * sx + 2 * ceil_div(ylen, kBandRows) * sx;
}

// (records of 16-bit values, where every pass runs on the integer column kernel: the rows as packed 16-bit pairs)
static int64_t record16_words(int64_t sx, int64_t ylen) {
  return ylen * sx / 2 + 2 * ceil_div(ylen, kBandRows) * sx;
}

// What tells the two forms of slab records apart -- all the XY and the Z record phase (xy_records, z_records) branch on.
struct RecordForm {
  int64_t (*words)(int64_t sx, int64_t ylen);  // 4-byte words per record
  bool rows16;          // the rows are packed 16-bit pairs (make_band_scatter), and what comes with that:
  int block_align;      // what check_y_splits asks of the destination blocks (0: non-null)
  bool index_required;  // pass X in index form whatever the call (its support check has seen to that), not only where it can be
  bool counts_refused;  // tiles without this form are counted in the caller's counter, not handed over through the plan's list
};
static constexpr RecordForm kRecordsF32 = {record_floats, false, 0, false, false};
static constexpr RecordForm kRecords16 = {record16_words, true, 8, true, true};

struct RecordPlan {
  float *F = nullptr;                                      // pass 1 output of the slab (XY phase)
  uint32_t *nz_y = nullptr, *ys_y = nullptr, *zs_y = nullptr;  // y-packed planes of the slab
  uint32_t *nz_z = nullptr, *rs_z = nullptr;               // z-packed planes (Z phase)
  BandScatter *table = nullptr;
  HandOver q16;                                            // hand-over list of the integer column kernel (one phase per call)
  uint32_t *ones_map = nullptr;                            // 16-bit records, Z phase: "every row of every tile is in the plane"
  size_t bytes = 0;
};

// sized for either phase on an (sx, sy, sz) block
static RecordPlan make_record_plan(int64_t sx, int64_t sy, int64_t sz, void *ws) {
  RecordPlan p;
  Carver c(ws);
  const size_t wy = (size_t)(sx * ceil_div(sy, kBandRows) * sz);
  const size_t wz = (size_t)(sx * ceil_div(sz, kBandRows) * sy);
  p.F = c.take<float>((size_t)(sx * sy * sz));
  p.nz_y = c.take<uint32_t>(wy);
  p.ys_y = c.take<uint32_t>(wy);
  p.zs_y = c.take<uint32_t>(wy);
  p.nz_z = c.take<uint32_t>(wz);
  p.rs_z = c.take<uint32_t>(wz);
  p.table = c.take<BandScatter>(1);
  p.q16.slots = 4;
  p.q16.counts = c.take<uint32_t>(4);
  p.q16.capacity = HandOver::ids_of(sx, std::max(sy, sz));
  p.q16.ids = c.take<uint32_t>((size_t)p.q16.capacity);
  p.ones_map = c.take<uint32_t>((size_t)(ceil_div(sx, 32) * ceil_div(std::max(sy, sz), 32)));
  p.bytes = align_up(c.off, 256) + 256;
  return p;
}

// the parts of y a slab's records go to: block h takes rows y_splits[h] .. y_splits[h + 1]
// (align 8 -- 16-bit records: 4-byte stores of packed pairs and bit words; the Z phase reads 8 bytes at a time: records are an
// even number of words)
static int check_y_splits(int nparts, const int64_t *y_splits, void *const *d_blocks, int64_t sy, int align) {
  if (y_splits[0] != 0 || y_splits[nparts] != sy) { set_error("y_splits must run from 0 to sy"); return EDT_ERR_BAD_ARG; }
  for (int h = 0; h < nparts; ++h) {
    if (y_splits[h + 1] <= y_splits[h] || (y_splits[h] % kBandRows) != 0) {
      set_error("y_splits must be increasing multiples of 32 (the last one is sy)");
      return EDT_ERR_BAD_ARG;
    }
    if (!d_blocks[h] || (align && (reinterpret_cast<uintptr_t>(d_blocks[h]) % align) != 0)) {
      set_error(align ? "destination blocks must be non-null and 8-byte aligned" : "null destination block");
      return EDT_ERR_BAD_ARG;
    }
  }
  return EDT_OK;
}

// destination map: every 32-row band of y lies inside one part.  Records of fp32 rows, or (rows16) in 4-byte words: a record =
// ylen * sx / 2 words of 16-bit pairs, then the two bit planes
static BandScatter make_band_scatter(const AxisGeom &gy, const int64_t *y_splits, void *const *d_blocks, const RecordForm &form) {
  BandScatter sc;
  const int64_t sx = gy.sx, per_word = form.rows16 ? 2 : 1;
  for (int b = 0, h = 0; b < BandScatter::kBands; ++b) {
    if (b >= gy.nbands) { sc.rows[b] = nullptr; sc.bits[b] = nullptr; sc.ostride[b] = 0; sc.plane[b] = 0; continue; }
    while ((int64_t)b * kBandRows >= y_splits[h + 1]) ++h;
    const int64_t ys = y_splits[h], ylen = y_splits[h + 1] - ys, words = ceil_div(ylen, kBandRows);
    float *blk = static_cast<float *>(d_blocks[h]);
    sc.rows[b] = blk + (((int64_t)b * kBandRows - ys) * sx) / per_word;
    sc.bits[b] = reinterpret_cast<uint32_t *>(blk + ylen * sx / per_word) + ((int64_t)b - ys / kBandRows) * sx;
    sc.ostride[b] = form.words(sx, ylen);
    sc.plane[b] = words * sx;
  }
  return sc;
}

// What every phase entry point checks before its first launch, in this order: shape, voxel sizes (an XY phase: *wx and w = wy; a
// Z phase, wx == nullptr: w = wz alone), empty volume (*empty: nothing to do), null arguments (null_text: the entry point's word
// for them), own(): the checks that belong to one entry point, in ITS order -- the order of the refusals is each entry point's own
// (tests/test_shard_refusals.py) --, then the workspace: *plan = make(extents, d_workspace), its bytes and its alignment.  What an
// entry point checks after the workspace, it checks after the prologue.  No step asks for a device.
static int no_own_checks() { return EDT_OK; }
template <typename Plan, typename Own = int (*)()>
static int phase_prologue(int dtype, int64_t sx, int64_t sy, int64_t sz, float *wx, float &w, bool null_argument, const char *null_text,
                          void *d_workspace, size_t workspace_bytes, bool *empty, Plan (*make)(int64_t, int64_t, int64_t, void *),
                          Plan *plan, Own own = no_own_checks) {
  *empty = false;
  int rc = check_shape(dtype, 3, sx, sy, sz);
  if (rc != EDT_OK) return rc;
  float w1 = 1.0f;
  if ((rc = wx ? check_voxel_sizes(2, *wx, w, w1) : check_column_voxel_size(w)) != EDT_OK) return rc;
  if (sx == 0 || sy == 0 || sz == 0) { *empty = true; return EDT_OK; }
  if (null_argument) { set_error(null_text); return EDT_ERR_BAD_ARG; }
  if ((rc = own()) != EDT_OK) return rc;
  *plan = make(sx, sy, sz, d_workspace);
  return check_shard_workspace(d_workspace, workspace_bytes, plan->bytes);
}

// The XY phase of a slab into records of `form`: pass X, the records' bit planes, pass Y scattering its rows.  Q: the quantum
// of the voxel sizes the entry point knows (the integer column kernel where they share one, edt_colq16.hip).  d_refused: the
// caller's counter of a form that counts_refused.
static int xy_records(const RecordForm &form, const void *d_labels, const void *d_halo, int dtype, int64_t sx, int64_t sy,
                      int64_t sz_local, float wx, float wy, int flags, const int64_t *y_splits, void *const *d_blocks,
                      const Quantum &Q, uint32_t *d_refused, RecordPlan &p, hipStream_t stream) {
  const int bb = (flags & EDT_FLAG_BLACK_BORDER) ? 1 : 0;
  AxisGeom gy = make_geom_y(sx, sy, sz_local);
  gy.fmin = edt_hip_field_floor(wx, wx);  // (pass Y reads the results of pass X: AxisGeom::fmin)
  const BandScatter sc = make_band_scatter(gy, y_splits, d_blocks, form);
  // (index form of pass 1 where the voxel size allows it, see run_device: the slab's pass-1 buffer then holds 16-bit
  // indices in its first half)
  const bool index_form = form.index_required || ((sx % 4) == 0 && !(debug_mode() & kDbgFp32PassX) && row_codes_exact(wx, sx));
  uint16_t *codes = index_form ? reinterpret_cast<uint16_t *>(p.F) : nullptr;
  int rc;
  {
    ScopedPass t("x_pass", stream);
    RowPass rp = row_pass(dtype, d_labels, sx, sy, sz_local, wx, bb, stream);
    rp.halo = d_halo; rp.out = p.F; rp.nz_y = p.nz_y; rp.ys_y = p.ys_y; rp.zs_y = p.zs_y; rp.codes = codes;
    if ((rc = launch_row_pass_wave(rp)) != EDT_OK) return rc;
  }
  {
    ScopedPass t("pack_bits", stream);
    rc = launch_pack_record_bits(p.nz_y, p.zs_y, sc, p.table, sx, gy.nbands, sz_local, stream);
    if (rc != EDT_OK) return rc;
  }
  ScopedPass t("y_pass", stream);
  // the integer column kernel where the voxel sizes share a quantum (edt_colq16.hip), the tiles it refuses to the fp32 kernel
  ColumnPass cp = column_pass(p.F, p.nz_y, p.ys_y, gy, wy, bb, 0, stream);
  cp.codes = codes;
  cp.wx = wx;
  cp.scatter = p.table;
  if (form.rows16) cp.plane = codes;  // (any non-null value selects the 16-bit output; the destinations are the table's)
  HandOver refused;  // (the caller's counter, which it zeroes and reads; no id array: the tiles are only counted)
  refused.counts = d_refused;
  refused.slots = 1;
  refused.zeroed = true;
  return run_column_pass(cp, Q, 1, form.counts_refused ? refused : p.q16, Fp32Leg::wave);
}

// The Z phase over gathered records of `form`: the z-packed bit planes from the tail of every record, then pass Z.  Rows of
// fp32 values are read and written in place in the records; 16-bit rows are read from the records as a plane and the results
// go to the dense d_out.  field_floor: what the XY phase guarantees about the values it left (AxisGeom::fmin; NaN and
// negatives: unknown).  Q: the quantum of the voxel sizes, where the entry point knows all three.
static int z_records(const RecordForm &form, void *d_records, float *d_out, int64_t sx, int64_t sy_local, int64_t sz, float wz,
                     float field_floor, const Quantum &Q, int flags, RecordPlan &p, hipStream_t stream) {
  const int bb = (flags & EDT_FLAG_BLACK_BORDER) ? 1 : 0;
  const int epi = last_pass_epi(bb, (flags & EDT_FLAG_SQRT) != 0);  // (the Z phase writes the call's results)
  const int64_t rec = form.words(sx, sy_local), words = ceil_div(sy_local, kBandRows);
  const uint32_t *nz_y = static_cast<const uint32_t *>(d_records) + rec - 2 * words * sx;
  int rc;
  {
    ScopedPass t("z_bits", stream);
    rc = launch_bits_transpose_yz(nz_y, nz_y + words * sx, p.nz_z, p.rs_z, sx, sy_local, sz, stream, rec);
    if (rc != EDT_OK) return rc;
  }
  AxisGeom gz = make_geom_z(sx, sy_local, sz);  // the dense output: z-columns one (sy_local, sx) slice apart
  if (!form.rows16) gz.stride = rec;            // z-columns of the record buffer: consecutive z are one record apart
  gz.fmin = field_floor > 0.0f ? field_floor : 0.0f;
  ScopedPass t("z_pass", stream);
  ColumnPass cp = column_pass(form.rows16 ? d_out : static_cast<float *>(d_records), p.nz_z, p.rs_z, gz, wz, bb, epi, stream);
  if (form.rows16) {
    // every row out of the records (16-bit elements: consecutive z are 2 * rec of them apart), results to the dense array; a
    // tile beyond THIS pass's limits gets its rows written there as fp32 values and goes to the fp32 kernel, in place
    cp.plane = static_cast<uint16_t *>(d_records);
    cp.map = p.ones_map;
    cp.map_words = (int)ceil_div(sz, 32);
    cp.plane_stride = 2 * rec;
    cp.plane_outer = sx;
    if ((rc = launch_fill_words(p.ones_map, ~0u, (size_t)(ceil_div(sx, 32) * cp.map_words), stream)) != EDT_OK) return rc;
  }
  TileList served;
  rc = run_column_pass(cp, Q, 2, p.q16, Fp32Leg::wave, false, &served);
  // (only this form promises the integer kernel: edt_hip_shard_records16_supported)
  if (rc == EDT_OK && form.rows16 && served.count == nullptr) { set_error("internal: the Z phase of 16-bit records left the integer kernel"); return EDT_ERR_HIP; }
  return rc;
}

}  // namespace edt_amd

using namespace edt_amd;

extern "C" {

size_t edt_hip_shard_workspace_bytes(int dtype, int64_t sx, int64_t sy, int64_t sz) {
  if (check_shape(dtype, 3, sx, sy, sz) != EDT_OK) return 0;
  if (sx == 0 || sy == 0 || sz == 0) return 256;
  return make_shard_plan(sx, sy, sz, nullptr).bytes;
}

int edt_hip_shard_xy_device(const void *d_labels, const void *d_halo, int dtype, int64_t sx,
                            int64_t sy, int64_t sz_local, float wx, float wy, int flags,
                            float *d_partial, uint8_t *d_zflags, void *d_workspace,
                            size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ShardPlan p;
  bool empty;
  int rc = phase_prologue(dtype, sx, sy, sz_local, &wx, wy, !d_labels || !d_partial || !d_zflags, "null device pointer", d_workspace,
                          workspace_bytes, &empty, make_shard_plan, &p);
  if (rc != EDT_OK || empty) return rc;
  const int bb = (flags & EDT_FLAG_BLACK_BORDER) ? 1 : 0;
  const bool force_generic = (flags & EDT_FLAG_FORCE_GENERIC) != 0;
  AxisGeom gy = make_geom_y(sx, sy, sz_local);
  gy.fmin = edt_hip_field_floor(wx, wx);  // (pass Y reads the results of pass X: AxisGeom::fmin)
  const bool tiled_y = !force_generic && column_inplace_supported(gy);
  RowPass rp = row_pass(dtype, d_labels, sx, sy, sz_local, wx, bb, stream);
  rp.out = tiled_y ? d_partial : p.bufB;  // the tiled y pass runs in place
  rp.nz_y = p.nz; rp.ys_y = p.rs;
  // rows no row kernel takes: the line pipeline (a thread per voxel), its scratch borrowed from the hull stacks, which only
  // the size-agnostic column pass uses -- later on this stream
  const bool borrow = !force_generic && rows_line_workspace_bytes(sx, sy * sz_local) <= (size_t)(sx * sy * sz_local) * sizeof(int32_t);
  if ((rc = run_row_pass(rp, row_pass_on_row_kernels(dtype, sx, sy, sz_local, force_generic), borrow ? p.stack : nullptr)) != EDT_OK) return rc;
  if (tiled_y) rc = launch_column_inplace(column_pass(d_partial, p.nz, p.rs, gy, wy, bb, 0, stream));
  else rc = launch_column_pass_serial(p.bufB, d_partial, p.nz, p.rs, p.stack, gy, wy, bb, 0, stream);
  if (rc != EDT_OK) return rc;
  return launch_zflags(dtype, d_labels, d_halo, d_zflags, sx * sy, sz_local, stream);
}

int edt_hip_shard_z_device(float *d_partial, const uint8_t *d_zflags, int64_t sx, int64_t sy_local,
                           int64_t sz, float wz, int flags, void *d_workspace,
                           size_t workspace_bytes, void *stream_) {
  return edt_hip_shard_z_device_ex(d_partial, d_zflags, sx, sy_local, sz, wz, 0.0f, flags, d_workspace, workspace_bytes,
                                   stream_);
}

int edt_hip_shard_z_device_ex(float *d_partial, const uint8_t *d_zflags, int64_t sx, int64_t sy_local,
                              int64_t sz, float wz, float field_floor, int flags, void *d_workspace,
                              size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ShardPlan p;
  bool empty;
  int rc = phase_prologue(EDT_U8, sx, sy_local, sz, nullptr, wz, !d_partial || !d_zflags, "null device pointer", d_workspace,
                          workspace_bytes, &empty, make_shard_plan, &p);
  if (rc != EDT_OK || empty) return rc;
  const int bb = (flags & EDT_FLAG_BLACK_BORDER) ? 1 : 0;
  const int epi = last_pass_epi(bb, (flags & EDT_FLAG_SQRT) != 0);  // (the Z phase writes the call's results)
  AxisGeom gz = make_geom_z(sx, sy_local, sz);
  gz.fmin = field_floor > 0.0f ? field_floor : 0.0f;  // (AxisGeom::fmin; NaN and negatives: unknown)
  rc = launch_bits_from_flags(d_zflags, p.nz, p.rs, gz, stream);
  if (rc != EDT_OK) return rc;
  if (!(flags & EDT_FLAG_FORCE_GENERIC) && column_inplace_supported(gz))
    return launch_column_inplace(column_pass(d_partial, p.nz, p.rs, gz, wz, bb, epi, stream));
  rc = launch_column_pass_serial(d_partial, p.bufB, p.nz, p.rs, p.stack, gz, wz, bb, epi, stream);
  if (rc != EDT_OK) return rc;
  EDT_HIP_TRY(hipMemcpyAsync(d_partial, p.bufB, (size_t)(sx * sy_local * sz) * sizeof(float),
                             hipMemcpyDeviceToDevice, stream));
  return EDT_OK;
}

int edt_hip_shard_records_supported(int dtype, int64_t sx, int64_t sy, int64_t sz) {
  if (dtype_size(dtype) == 0 || sx < 1 || sy < 1 || sz < 1) return 0;
  if (debug_mode() & (kDbgTiledRows | kDbgTiledColumns)) return 0;  // diagnostics: forced fallback kernels
  // pass 1 by the register-resident row kernel (two waves per row beyond 1024 voxels), both column passes by the wave kernel
  return (sx <= 2048 && row_pass_wave_supported(dtype, sx, sy, sz) && sy <= 2048 && sz <= 2048) ? 1 : 0;
}

size_t edt_hip_shard_record_floats(int64_t sx, int64_t y_rows) {
  if (sx < 0 || y_rows < 0) return 0;
  return (size_t)record_floats(sx, y_rows);
}

size_t edt_hip_shard_records_workspace_bytes(int dtype, int64_t sx, int64_t sy, int64_t sz) {
  if (check_shape(dtype, 3, sx, sy, sz) != EDT_OK) return 0;
  if (sx == 0 || sy == 0 || sz == 0) return 256;
  return make_record_plan(sx, sy, sz, nullptr).bytes;
}

int edt_hip_shard_xy_records_device(const void *d_labels, const void *d_halo, int dtype, int64_t sx,
                                    int64_t sy, int64_t sz_local, float wx, float wy, int flags,
                                    int nparts, const int64_t *y_splits, void *const *d_blocks,
                                    void *d_workspace, size_t workspace_bytes, void *stream_) {
  RecordPlan p;
  bool empty;
  const int rc = phase_prologue(dtype, sx, sy, sz_local, &wx, wy, !d_labels || !y_splits || !d_blocks || nparts < 1, "null argument",
                                d_workspace, workspace_bytes, &empty, make_record_plan, &p, [&]() -> int {
    if (!edt_hip_shard_records_supported(dtype, sx, sy, sz_local)) {
      set_error("slab records need sx <= 2048 and sy <= 2048 (use edt_hip_shard_xy_device)");
      return EDT_ERR_UNSUPPORTED;
    }
    if (const int bad = check_y_splits(nparts, y_splits, d_blocks, sy, kRecordsF32.block_align)) return bad;
    if (g_log.enabled.load(std::memory_order_relaxed)) {
      std::lock_guard<std::mutex> lock(g_log_mutex);
      if (g_log.used > 2048) log_begin_call();  // nobody is reading the log
    }
    return EDT_OK;
  });
  if (rc != EDT_OK || empty) return rc;
  // (the scattering column kernels store 16 bytes at a time where rows are whole granules)
  for (int h = 0; h < nparts && (sx % 4) == 0; ++h)
    if ((reinterpret_cast<uintptr_t>(d_blocks[h]) % 16) != 0) { set_error("destination blocks must be 16-byte aligned"); return EDT_ERR_BAD_ARG; }
  const float w2[2] = {wx, wy};  // (the quantum wx and wy share, if any)
  return xy_records(kRecordsF32, d_labels, d_halo, dtype, sx, sy, sz_local, wx, wy, flags, y_splits, d_blocks, q16_quantum(w2, 2), nullptr,
                    p, (hipStream_t)stream_);
}

int edt_hip_shard_z_records_device(float *d_records, int64_t sx, int64_t sy_local, int64_t sz, float wz,
                                   int flags, void *d_workspace, size_t workspace_bytes, void *stream_) {
  return edt_hip_shard_z_records_device_ex(d_records, sx, sy_local, sz, wz, 0.0f, flags, d_workspace, workspace_bytes,
                                           stream_);
}

// w3 != nullptr: the caller named all three voxel sizes -- the integer column kernel where they share a quantum
static int shard_z_records(float *d_records, int64_t sx, int64_t sy_local, int64_t sz, float wz, float field_floor,
                           const float *w3, int flags, void *d_workspace, size_t workspace_bytes, void *stream_) {
  RecordPlan p;
  bool empty;
  const int rc = phase_prologue(EDT_U8, sx, sy_local, sz, nullptr, wz, !d_records, "null device pointer", d_workspace, workspace_bytes,
                                &empty, make_record_plan, &p, [&]() -> int {
    if (edt_hip_shard_records_supported(EDT_U8, sx, sy_local, sz)) return EDT_OK;
    set_error("slab records need sx <= 2048 and sz <= 2048 (use edt_hip_shard_z_device)");
    return EDT_ERR_UNSUPPORTED;
  });
  if (rc != EDT_OK || empty) return rc;
  return z_records(kRecordsF32, d_records, nullptr, sx, sy_local, sz, wz, field_floor, w3 ? q16_quantum(w3, 3) : Quantum(), flags, p,
                   (hipStream_t)stream_);
}

int edt_hip_shard_z_records_device_ex(float *d_records, int64_t sx, int64_t sy_local, int64_t sz, float wz,
                                      float field_floor, int flags, void *d_workspace, size_t workspace_bytes,
                                      void *stream_) {
  return shard_z_records(d_records, sx, sy_local, sz, wz, field_floor, nullptr, flags, d_workspace, workspace_bytes, stream_);
}

int edt_hip_shard_z_records_device_w(float *d_records, int64_t sx, int64_t sy_local, int64_t sz, float wx, float wy,
                                     float wz, int flags, void *d_workspace, size_t workspace_bytes, void *stream_) {
  const float w3[3] = {wx, wy, wz};
  return shard_z_records(d_records, sx, sy_local, sz, wz, edt_hip_field_floor(wx, wy), w3, flags, d_workspace,
                         workspace_bytes, stream_);
}

// ---- slab records of 16-bit values ---------------------------------------------------------------------------------------
// Where the three voxel sizes share a quantum (edt_colq16.hip) and both column axes fit the integer kernel, the Y pass's
// results are integers N < 2^16 (in quanta): a record then carries its rows as 16-bit values -- 2.25 bytes per voxel over
// the links instead of 4.25 -- and the Z phase reads them as they are.  A tile the integer kernel cannot take (values beyond
// 16 bits, rows without a boundary) has no 16-bit form: the XY phase COUNTS such tiles in *d_refused (a device counter the
// caller zeroes and reads; it accumulates over calls) and leaves their rows unspecified -- a caller that finds it non-zero
// repeats the step with the fp32 records above (edt/distributed.py does).
static bool records16_common_ok(int64_t sx, float wx, float wy, float wz) {
  if (sx % 4 != 0 || (debug_mode() & (kDbgQ16Off | kDbgFp32PassX | kDbgNoQ16 | kDbgFp32Plane))) return false;
  if (!row_codes_exact(wx, sx)) return false;
  const float w3[3] = {wx, wy, wz};
  return q16_quantum(w3, 3).ok;
}
// the XY phase of a slab of sz_local slices / the Z phase of a slab of sy_local rows: the scan axis on the integer kernel
static bool records16_xy_ok(int dtype, int64_t sx, int64_t sy, int64_t sz_local, float wx, float wy, float wz) {
  if (!edt_hip_shard_records_supported(dtype, sx, sy, sz_local) || !records16_common_ok(sx, wx, wy, wz)) return false;
  const AxisGeom gy = make_geom_y(sx, sy, sz_local);
  return column_pass_q16_supported(gy) && column_pass_wave_supported(gy);
}
static bool records16_z_ok(int64_t sx, int64_t sy_local, int64_t sz, float wx, float wy, float wz) {
  if (!edt_hip_shard_records_supported(EDT_U8, sx, sy_local, sz) || !records16_common_ok(sx, wx, wy, wz)) return false;
  const AxisGeom gz = make_geom_z(sx, sy_local, sz);
  return column_pass_q16_supported(gz) && column_pass_wave_supported(gz);
}
// *Q: the quantum of a phase on 16-bit records; a call they do not apply to (phase_ok: its records16_*_ok) is refused
static int records16_quantum(bool phase_ok, float wx, float wy, float wz, Quantum *Q) {
  const float w3[3] = {wx, wy, wz};
  *Q = q16_quantum(w3, 3);
  if (phase_ok && Q->ok) return EDT_OK;
  set_error("16-bit slab records do not apply to these extents / voxel sizes (edt_hip_shard_records16_supported)");
  return EDT_ERR_UNSUPPORTED;
}

int edt_hip_shard_records16_supported(int dtype, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz) {
  if (dtype_size(dtype) == 0 || sx < 1 || sy < 1 || sz < 1) return 0;
  // (whatever part of z or y a rank holds, its scan axis is whole: sy for the XY phase, sz for the Z phase)
  return (records16_xy_ok(dtype, sx, sy, 1, wx, wy, wz) && records16_z_ok(sx, 32, sz, wx, wy, wz)) ? 1 : 0;
}

size_t edt_hip_shard_record16_words(int64_t sx, int64_t y_rows) {
  if (sx < 0 || y_rows < 0 || sx % 2 != 0) return 0;
  return (size_t)record16_words(sx, y_rows);
}

int edt_hip_shard_xy_records16_device(const void *d_labels, const void *d_halo, int dtype, int64_t sx, int64_t sy,
                                      int64_t sz_local, float wx, float wy, float wz, int flags, int nparts,
                                      const int64_t *y_splits, void *const *d_blocks, uint32_t *d_refused, void *d_workspace,
                                      size_t workspace_bytes, void *stream_) {
  RecordPlan p;
  Quantum Q;
  bool empty;
  const int rc = phase_prologue(dtype, sx, sy, sz_local, &wx, wy, !d_labels || !y_splits || !d_blocks || !d_refused || nparts < 1,
                                "null argument", d_workspace, workspace_bytes, &empty, make_record_plan, &p, [&]() -> int {
    if (const int bad = check_y_splits(nparts, y_splits, d_blocks, sy, kRecords16.block_align)) return bad;
    return records16_quantum(records16_xy_ok(dtype, sx, sy, sz_local, wx, wy, wz), wx, wy, wz, &Q);
  });
  if (rc != EDT_OK || empty) return rc;
  return xy_records(kRecords16, d_labels, d_halo, dtype, sx, sy, sz_local, wx, wy, flags, y_splits, d_blocks, Q, d_refused, p,
                    (hipStream_t)stream_);
}

int edt_hip_shard_z_records16_device(const void *d_records, float *d_out, int64_t sx, int64_t sy_local, int64_t sz, float wx,
                                     float wy, float wz, int flags, void *d_workspace, size_t workspace_bytes, void *stream_) {
  RecordPlan p;
  Quantum Q;
  bool empty;
  const int rc = phase_prologue(EDT_U8, sx, sy_local, sz, nullptr, wz, !d_records || !d_out, "null device pointer", d_workspace,
                                workspace_bytes, &empty, make_record_plan, &p, [&]() -> int {
    if (const int no = records16_quantum(records16_z_ok(sx, sy_local, sz, wx, wy, wz), wx, wy, wz, &Q)) return no;
    if (((reinterpret_cast<uintptr_t>(d_records) | reinterpret_cast<uintptr_t>(d_out)) % 16) == 0) return EDT_OK;
    set_error("the gathered records and d_out must be 16-byte aligned");
    return EDT_ERR_BAD_ARG;
  });
  if (rc != EDT_OK || empty) return rc;
  // (the records are only read: the results go to d_out)
  return z_records(kRecords16, const_cast<void *>(d_records), d_out, sx, sy_local, sz, wz, edt_hip_field_floor(wx, wy), Q, flags, p,
                   (hipStream_t)stream_);
}

}  // extern "C"
