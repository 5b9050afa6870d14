// edt_rowpass.hip -- the one driver of pass X: which kernel serves a stack of rows, and who writes the y planes.  run_device
// (edt_api.hip) and the XY phase of the Z-sharded path (edt_shard_api.hip) go through run_row_pass; what differs between them
// is data (RowPass, the scratch of the line pipeline, the forced-generic flag behind row_pass_on_row_kernels).
#include "edt_api_internal.h"

namespace edt_amd {

// (the register kernel up to 4096 voxels per row, the workgroup-phased one up to 2048)
bool row_pass_on_row_kernels(int dtype, int64_t sx, int64_t sy, int64_t sz, bool force_generic) {
  return !force_generic && (row_pass_tiled_supported(sx) || row_pass_wave_supported(dtype, sx, sy, sz));
}

int run_row_pass(const RowPass &rp, bool row_kernels, void *line_ws, bool log) {
  const bool wave = row_kernels && row_pass_wave_supported(rp.dtype, rp.sx, rp.sy, rp.sz) && !(debug_mode() & kDbgTiledRows);
  // (a last pass -- the one line of a 1-D call -- has no planes to emit, and the row kernels no square root)
  if ((row_kernels && rp.last) || (!wave && (rp.halo != nullptr || rp.codes != nullptr || rp.zero_label != 0))) {
    set_error("internal: only the register kernel of pass X takes a halo, the index form or zero_label, and no row kernel a last pass");
    return EDT_ERR_HIP;
  }
  // labels are read once: the row kernels also emit the run bit-planes of the y and z axes
  if (row_kernels) {
    ScopedPass t(log ? "x_pass" : nullptr, rp.stream);
    return wave ? launch_row_pass_wave(rp) : launch_row_pass_tiled(rp);
  }
  {
    // longer rows: one thread per VOXEL through the line pipeline (edt_line.hip); the thread-per-row kernel stays behind
    // EDT_FLAG_FORCE_GENERIC as the cross-check it is
    ScopedPass t(log ? "x_pass" : nullptr, rp.stream);
    const int rc = line_ws != nullptr ? launch_rows_line_pass(rp, line_ws) : launch_row_pass_serial(rp);
    if (rc != EDT_OK) return rc;
  }
  if (rp.last) return EDT_OK;
  ScopedPass t(log ? "y_bits" : nullptr, rp.stream);
  return launch_axis_bits(rp.dtype, rp.labels, nullptr, rp.nz_y, rp.ys_y, make_geom_y(rp.sx, rp.sy, rp.sz), rp.stream);
}

}  // namespace edt_amd
