// edt_kernels.h -- device helpers shared by the kernels + launcher declarations (internal).
#pragma once

#include "edt_common.h"

#pragma clang fp contract(off)

namespace edt_amd {

// (double)d squared, exact for |d| < 2^26  (reference: pyedt::sq, src/edt.hpp:34-37)
__device__ __forceinline__ double sqd(int64_t d) {
  const double x = (double)d;
  return x * x;
}

// Numerator of the abscissa where parabola q (height Fq) overtakes parabola p < q:
//   s(p,q) = hull_num / (2 * (q - p) * w2)
// Same operation order as the reference's `ff[i] - ff[v[k]] + factor1 * factor2`
// (src/edt.hpp:206-208).  Comparing s(b,i) <= s(a,b) is done by cross-multiplication,
// which needs no division:   hull_num(b,i) * (b-a)  <=  hull_num(a,b) * (i-b).
__device__ __forceinline__ double hull_num(double Fp, double Fq, int64_t p, int64_t q, double w2) {
  const double f1 = (double)(q - p) * w2;
  const double f2 = (double)(q + p);
  return (Fq - Fp) + f1 * f2;
}

// Last-pass epilogue: FLT_MAX sentinel back to +INF (toinfinite, src/edt.hpp:47-53) and the
// optional correctly rounded sqrt (src/edt.hpp:599-601 / np.sqrt at src/edt.pyx:242).
__device__ __forceinline__ float finish(float m, int epi) {
  if ((epi & kEpiToInf) && m >= FLT_MAX) m = INFINITY;
  if (epi & kEpiSqrt) m = sqrtf(m);
  return m;
}

// Pass X over a stack of sy * sz rows of sx voxels, whichever kernel serves it.  Every kernel writes `out`; the row kernels
// (edt_rowwave.hip, edt_rows.hip) also emit the y-packed bit planes [z][y-band][x] of the column passes, and only the register
// kernel of edt_rowwave.hip knows halo, codes and zero_label.
struct RowPass {
  int dtype = EDT_U8;
  const void *labels = nullptr;
  const void *halo = nullptr;  // the xy-slice below slice 0 (Z-sharded slabs, later slabs of a call); nullptr: slice 0 starts every z-run
  int64_t sx = 1, sy = 1, sz = 1;
  float w = 1.0f;              // voxel size along x
  int bb = 0;
  hipStream_t stream = nullptr;
  float *out = nullptr;        // the fp32 field (not touched where codes is given)
  uint32_t *nz_y = nullptr, *ys_y = nullptr, *zs_y = nullptr;  // foreground (nullptr: nobody reads one) / y-run starts / z-run starts (nullptr: no z pass)
  uint16_t *codes = nullptr;   // index form: 16-bit distance indices go here INSTEAD of `out` (see XFuse) ...
  int64_t codes_pitch = 0;     // ... their slices this many elements apart (0: sx * sy)
  int zero_label = 0;          // label 0 is measured like every label (the signed transform; 2: nz_y keeps the true label != 0 bits)
  // index form, rows of at most 1024 voxels, zero_label == 0: rows without a run start are not stored; two words per (z, band of
  // 32 rows) say which ([z][band][plain, plain_fg]: edt_rowwave.hip) and the first column pass takes them (ColumnPass::rowflags)
  uint32_t *rowflags = nullptr;
  // pass X is the call's LAST pass (a 1-D call): a row without a boundary keeps +inf, and the square root is taken here if asked
  bool last = false, last_sqrt = false;
  int64_t nrows() const { return sy * sz; }
  int to_finite() const { return (bb || last) ? 0 : 1; }  // FLT_MAX, not +inf, where a row has no boundary: a column pass follows
  int take_sqrt() const { return (last && last_sqrt) ? 1 : 0; }
};
inline RowPass row_pass(int dtype, const void *labels, int64_t sx, int64_t sy, int64_t sz, float w, int bb, hipStream_t stream) {
  RowPass rp;
  rp.dtype = dtype; rp.labels = labels; rp.sx = sx; rp.sy = sy; rp.sz = sz; rp.w = w; rp.bb = bb; rp.stream = stream;
  return rp;
}
// ---- generic (any extent) kernels: edt_generic.hip ------------------------------------
int launch_row_pass_serial(const RowPass &rp);  // a thread per row
// ---- the 1-D transform as a parallel pipeline for lines of any length: edt_line.hip -----------------
size_t line_workspace_bytes(int64_t n);
// pass 1 over rows of any length (sx > 2048), or the one line of a 1-D call: the line pipeline with a run start forced at
// every row's first voxel
size_t rows_line_workspace_bytes(int64_t sx, int64_t nrows);
int launch_rows_line_pass(const RowPass &rp, void *ws);
size_t runs_workspace_bytes(int64_t n);
int launch_extract_runs(int dtype, const void *labels, int64_t n, int64_t *starts, int64_t capacity, int64_t *total,
                        void *ws, hipStream_t stream);
int launch_axis_bits(int dtype, const void *labels, const void *halo, uint32_t *nz, uint32_t *rs,
                     const AxisGeom &g, hipStream_t stream);
// planes of the binary route (EDT_FLAG_BINARY_YZ): every column one all-foreground run
int launch_planes_one_run(uint32_t *nz, uint32_t *rs, uint32_t *zs, const AxisGeom &g, int64_t o0, hipStream_t stream);
int launch_column_pass_serial(const float *fin, float *fout, const uint32_t *nz, const uint32_t *rs,
                              int32_t *stack, const AxisGeom &g, float w, int bb, int epi,
                              hipStream_t stream);
int launch_subtract(const float *a, const float *b, float *out, int64_t count, hipStream_t stream);
int launch_is_background(int dtype, const void *labels, uint8_t *mask, int64_t count,
                         hipStream_t stream);
int launch_negate_background(int dtype, const void *labels, float *f, int64_t count, hipStream_t stream);  // f = labels == 0 ? -f : f
int launch_select_label(int dtype, const void *labels, const float *dt, float *out, const void *key,
                        int64_t count, hipStream_t stream);
// ---- the streaming kernels of the morphology operations: edt_morph.hip ------------------------------
// mask[i] = labels[i] != 0 (the type's own comparison: -0.0 is zero, a NaN is not)
int launch_is_foreground(int dtype, const void *labels, uint8_t *mask, int64_t count, hipStream_t stream);
// pass(i) = field[i] > r2 (EDT_MORPH_FARTHER) or <= r2 (EDT_MORPH_WITHIN), in fp64, or guard[i] != 0 where a guard is given;
// out[i] = pass ? values[i] : zero bits (out == values allowed), mask[i] = pass ? 0 : 1 -- either may be null, not both
int launch_morph_select(int dtype, const void *values, const void *guard, const float *field, double r2, int rule, void *out,
                        uint8_t *mask, int64_t count, hipStream_t stream);
// *r2 = radius * radius in fp64; EDT_ERR_BAD_ARG, named "<who>: ...", unless radius >= 0 and *r2 is finite (inf_allowed: or radius is +inf)
int morph_radius_squared(double radius, bool inf_allowed, const char *who, double *r2);
// one step of local thickness (include/edt_hip.h, "local thickness").  B != nullptr: T[i] = rf where S[i] > 0 && B[i] <= r2 (in
// fp64), *size += their number; B == nullptr: T[i] = 0, *smax_bits = max(*smax_bits, bits of the largest finite S[i]);
// mask != nullptr: mask[i] = S[i] > next2 ? 0 : 1.  size, smax_bits and mask may be null.
int launch_thickness_step(const float *S, const float *B, double r2, float rf, double next2, float *T, uint8_t *mask, int64_t *size,
                          uint32_t *smax_bits, int64_t count, hipStream_t stream);
// *r2 = radius * radius; EDT_ERR_BAD_ARG, named "<who>: ...", unless radius is finite and > 0 and *r2 is finite
int thickness_radius_squared(double radius, const char *who, double *r2);
// ---- the stencil of the integer medial axis: edt_medial.hip ------------------------------
// *g2 = gamma * gamma; EDT_ERR_BAD_ARG, named "<who>: ...", unless gamma >= 0 with *g2 finite and ratio is finite and >= 0
int medial_check_params(double gamma, double ratio, const char *who, double *g2);
// one step (include/edt_hip.h, "medial axis") over the ndim feature planes `feat` of the labels (or of their mask, under
// EDT_FLAG_MORPH_BINARY): out[p] = labels[p] on the axis, zero bits elsewhere; radius (with field; both may be null): field[p] on
// the axis, +0.0 elsewhere.  flags: EDT_FLAG_BLACK_BORDER (every voxel has a feature), EDT_FLAG_MORPH_BINARY.
int launch_medial_axis(int dtype, const void *labels, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                       const int32_t *feat, int flags, double g2, double ratio, void *out, const float *field, float *radius,
                       hipStream_t stream);

}  // namespace edt_amd

namespace edt_amd {
// ---- voxel-graph helpers: edt_voxel_graph.hip -----------------------------------------
int launch_vg_expand(int dtype, const void *labels, const uint8_t *graph, uint8_t *big, int64_t sx,
                     int64_t sy, int64_t sz, int ndim, int bb, hipStream_t stream);
int launch_vg_gather(const float *big, float *out, int64_t sx, int64_t sy, int64_t sz, int ndim,
                     hipStream_t stream);
// native form (no doubled volume): only the cells the result depends on are computed
bool vg_native_supported(int ndim, int64_t sx, int64_t sy, int64_t sz);
size_t vg_native_workspace_bytes(int ndim, int64_t sx, int64_t sy, int64_t sz);
int launch_vg_native(int dtype, const void *labels, const uint8_t *graph, int ndim, int64_t sx, int64_t sy,
                     int64_t sz, float wx, float wy, float wz, int bb, int want_sqrt, float *out, void *ws,
                     hipStream_t stream);
// ---- Z-sharded helpers: edt_shard.hip ---------------------------------------------------
int launch_zflags(int dtype, const void *labels, const void *halo, uint8_t *flags, int64_t sxy,
                  int64_t szl, hipStream_t stream);
int launch_bits_from_flags(const uint8_t *flags, uint32_t *nz, uint32_t *rs, const AxisGeom &g,
                           hipStream_t stream);
// y-packed planes [z][band][x] of a slab -> the bit part of the slab records; also publishes the
// destination map in device memory for the scattering column pass
int launch_pack_record_bits(const uint32_t *nz_y, const uint32_t *zs_y, const BandScatter &sc,
                            BandScatter *d_table, int64_t sx, int64_t nby, int64_t szl,
                            hipStream_t stream);
// ---- short axes (at most 32 rows): a thread per column, rows in registers: edt_short.hip ----
bool column_pass_short_supported(const AxisGeom &g);
int launch_column_pass_short(float *F, const uint32_t *nz, const uint32_t *rs, const AxisGeom &g, float w, int bb,
                             int epi, hipStream_t stream);
// ---- LDS-tiled column pass: edt_tiled.hip ---------------------------------------------------
bool column_pass_tiled_supported(const AxisGeom &g);
int launch_column_pass_tiled(float *F, const uint32_t *nz, const uint32_t *rs, const AxisGeom &g,
                             float w, int bb, int epi, hipStream_t stream);
// ---- wave-per-row-group pass 1 + bit-plane transposer: edt_rows.hip ---------------------------
bool row_pass_tiled_supported(int64_t sx);
int launch_row_pass_tiled(const RowPass &rp);
// in_zstride: words between consecutive z of the y-packed planes (0 = dense, nby * sx)
int launch_bits_transpose_yz(const uint32_t *nz_y, const uint32_t *zs_y, uint32_t *nz_z,
                             uint32_t *rs_z, int64_t sx, int64_t sy, int64_t sz, hipStream_t stream,
                             int64_t in_zstride = 0);
}  // namespace edt_amd

namespace edt_amd {
// Arguments of the index form of pass 1 (XF kernels of edt_colwave_kernel.h): pass 1 stored 16-bit distance
// indices k (edt_rowwave.hip, C16) instead of F; the first column pass rebuilds F = fl32(fl32(k * w)^2) while it fills
// its tile.  codes = nullptr: the ordinary in-place pass.
struct XFuse {
  const uint16_t *codes;  // [outer][row][x], same strides (in elements) as F ...
  int64_t c_outer;        // ... but for the outer stride where the index buffer has a padded pitch (0: g.outer_stride)
  float w;                // voxel size of pass 1 (k * w exact: row_codes_exact)
  int flim;               // bit pattern of FLT_MAX (tofinite) or +inf
};
// ---- wave-autonomous LDS-tiled column pass: edt_colwave.hip -----------------------------------
bool column_pass_wave_supported(const AxisGeom &g);
// Which rows of a column the caller reads again, and where they go (the doubled grids of the voxel-graph transform).
struct ColumnOut {
  int stride = 1;            // 2: only the even rows of every column are needed (tiles on the windowed path evaluate
                             // just those; tiles on the hull path evaluate every row)
  float *compact = nullptr;  // stride 2 only: the even rows are written HERE instead of in place -- row r of the
                             // column (x, outer index o) goes to compact[x + o * outer + (r / 2) * row2]
  int64_t outer = 0, row2 = 0;
};
// The tiles a launch of the fp32 column kernel serves: every tile of its grid (count = nullptr), or -- list mode -- the
// tiles the 16-bit integer kernel (edt_colq16.hip) handed over: workgroup b takes ids[b] if b < *count (device memory).
struct TileList {
  const uint32_t *count = nullptr;
  const uint32_t *ids = nullptr;
  bool none = false;  // the integer kernel served EVERY tile and the host can prove it (edt_colpass.hip): no fp32 launch at all
};
// One column pass (Y or Z), whichever kernel serves it: the fp32 wave kernel reads F, nz, rs (and codes), the 16-bit integer
// kernel F, rs (and codes / the plane).
struct ColumnPass {
  float *F = nullptr;                         // the field: read and written in place, unless an input form below says otherwise
  const uint32_t *nz = nullptr, *rs = nullptr;  // foreground / run-start bit planes of the scan axis
  AxisGeom g;
  float w = 1.0f;                             // voxel size along the scan axis
  int bb = 0, epi = 0;
  hipStream_t stream = nullptr;
  // input, index form: pass X left 16-bit distance indices (see XFuse) and F is only written
  const uint16_t *codes = nullptr;
  int64_t codes_outer = 0;  // outer stride of codes (and of the plane written over them), 0: g.outer_stride
  float wx = 0.0f;          // voxel size of pass X
  // ... and did not store its plain rows (RowPass::rowflags: [outer][band][2] words): the integer kernel puts their indices back
  // from the flags.  Only where no tile can reach the fp32 kernel, which reads codes and knows nothing of this.
  const uint32_t *rowflags = nullptr;
  // the 16-bit plane of the integer kernel (volumes whose indices fit one slab): with codes, the results stay 16-bit -- written
  // over the indices (plane == codes), the tile's bit set in map [x-tile][map_words]; without codes, every row is read from the
  // plane where map says so and from F elsewhere (the pass after such a pass).
  // Slab records of 16-bit values (edt_shard_api.hip): with codes, a scatter table AND a plane (any non-null value) the results go to
  // the table's destinations as 16-bit rows, refused tiles are only counted (no id array); without codes, a map of ones
  // and plane_stride > 0 every row is read from the plane at its own strides (16-bit elements) and F is only written.
  uint16_t *plane = nullptr;
  uint32_t *map = nullptr;
  int map_words = 0;
  int64_t plane_stride = 0, plane_outer = 0;
  int plane_inf_ok = 0;  // the pass that reads the 16-bit plane this one writes carries +inf
  // destination: see ColumnOut (default: every row, in place) -- (tiles on the windowed path evaluate and write just those;
  // tiles on the hull path still write every row); scatter != nullptr (device table): the rows are written to the slab
  // records instead of F (the caller guarantees 16-byte aligned destinations when sx % 4 == 0)
  ColumnOut out;
  const BandScatter *scatter = nullptr;
  const uint32_t *signbits = nullptr;  // kEpiSign: the true foreground plane of this axis
  int to_finite() const { return bb ? 0 : 1; }  // pass X left FLT_MAX (tofinite), not +inf, where a row has no boundary
};
inline ColumnPass column_pass(float *F, const uint32_t *nz, const uint32_t *rs, const AxisGeom &g, float w, int bb, int epi,
                              hipStream_t stream) {
  ColumnPass cp;
  cp.F = F; cp.nz = nz; cp.rs = rs; cp.g = g; cp.w = w; cp.bb = bb; cp.epi = epi; cp.stream = stream;
  return cp;
}
// the fp32 wave kernel over the tiles of `list`; codes != nullptr: reading pass 1 as 16-bit distance indices (see XFuse)
int launch_column_pass_wave(const ColumnPass &cp, const TileList &list);
// ---- 16-bit integer column pass: edt_colq16.hip ---------------------------------------------------
// the quantum of a call: w_i^2 = a[i] * q (ok false: the voxel sizes share none, the fp32 kernels keep the call)
struct Quantum {
  float q = 1.0f;
  uint32_t a[3] = {1u, 1u, 1u};
  bool ok = false;
};
Quantum q16_quantum(const float *w, int naxes);
bool column_pass_q16_supported(const AxisGeom &g);
// the largest value, in quanta, a tile of a pass with c_d = a * d^2 may hold and stay on the integer kernel (its 16-bit
// form, or the wide form: two half-tiles with 32-bit lanes) -- what a host that knows a bound of the field compares with
uint32_t q16_value_limit(float q, uint32_t a, int64_t n, int bb);
// the host's proof that the integer kernel refuses NO tile of a column pass of a call in the index form (axis 1: pass Y over
// columns of n = sy rows; axis 2: pass Z over n = sz rows behind a pass Y that could not refuse either) -- edt_colq16.hip
bool q16_no_refusals(const Quantum &Q, int axis, int64_t sx, int64_t sy, int64_t n, int bb);
// the kernel's vector accesses: 16-byte loads of fp32 rows, 8-byte stores of result pairs, 8-byte loads of index / plane
// rows (a 4-byte-aligned view handed in through DLPack stays on the fp32 kernel, which gates its vector accesses itself)
inline bool column_pass_q16_aligned(const float *F, const uint16_t *codes, const uint16_t *plane, const float *compact = nullptr) {
  return (reinterpret_cast<uintptr_t>(F) % 16) == 0 && (reinterpret_cast<uintptr_t>(codes) % 8) == 0 &&
         (reinterpret_cast<uintptr_t>(plane) % 8) == 0 && (reinterpret_cast<uintptr_t>(compact) % 8) == 0;
}
// `count` 32-bit words at p = value, by a KERNEL on the stream.  Every word an enqueue-only entry point sets on its stream is
// set this way and not with hipMemsetAsync: see DESIGN.md 13.3 (a captured call must replay like the call itself).
int launch_fill_words(void *p, uint32_t value, size_t count, hipStream_t stream);
// The hand-over from the integer kernel to the fp32 kernel: counters (one per launch: `slot` is the next free one) and one
// array of tile ids in the fp32 kernel's geometry (launches are stream-ordered: the array is reused).
struct HandOver {
  uint32_t *counts = nullptr, *ids = nullptr;
  int slots = 0;
  int64_t capacity = 0;  // tile ids `ids` holds (0 with ids == nullptr: refused tiles are only counted)
  int slot = 0;
  bool zeroed = false;   // the counters are zero on the stream (run_column_pass zeroes them before the first launch that needs it)
  // the ids a pass over nouter outer indices may write (16-column tiles for axes of more than 512 rows, XCD-aware tile order)
  static int64_t ids_of(int64_t sx, int64_t nouter) { return ceil_div(sx, 16) * (ceil_div(nouter, 8) * 8); }
  int zero(hipStream_t stream);  // all `slots` counters
};
// cp.codes != nullptr: pass X in index form (N = k^2 * Q.a[0]), F is only written; else F is read (N = F / q, verified) and
// written in place.  c_d = Q.a[axis] * d^2 quanta.  Tiles that do not qualify are appended to h's list (counter h.slot).
int launch_column_pass_q16(const ColumnPass &cp, const Quantum &Q, int axis, HandOver h);
// ---- the driver of a column pass: edt_colpass.hip ---------------------------------------------------
// In-place LDS-tiled column pass where one applies: the fp32 kernel for this axis (short / wave / workgroup-phased), or the
// wave kernel over `list`
bool column_inplace_supported(const AxisGeom &g);
int launch_column_inplace(const ColumnPass &cp, const TileList &list = TileList());
// will run_column_pass launch the integer kernel for this geometry?  (the shape and mode part of its test)
bool column_pass_q16_applies(const Quantum &Q, const AxisGeom &g, const HandOver &h);
// The integer kernel where it applies (Q.ok, modes, shape, alignment, capacity of h), then the fp32 kernel over the tiles it
// refused -- or over every tile -- through `leg`: the wave kernel, or launch_column_inplace's choice.  sure: the caller vouches
// for what the pass reads (see edt_colpass.hip).  served: count != nullptr -- the integer kernel ran; none -- its list is
// provably empty and no fp32 launch was made.  A hand-over without an id array only counts: no fp32 launch.
enum class Fp32Leg { wave, inplace };
int run_column_pass(const ColumnPass &cp, const Quantum &Q, int axis, HandOver &h, Fp32Leg leg, bool sure = false,
                    TileList *served = nullptr);
}  // namespace edt_amd

namespace edt_amd {
// ---- register-resident pass 1 (rows up to 512 voxels): edt_rowwave.hip -------------------------
bool row_pass_wave_supported(int dtype, int64_t sx, int64_t sy, int64_t sz);
int launch_row_pass_wave(const RowPass &rp);
// k * w exact for every k of a row of sx voxels: the 16-bit index form (codes) is bit-identical
bool row_codes_exact(float w, int64_t sx);
// ---- the driver of pass X: edt_rowpass.hip ---------------------------------------------------
// The one place that picks the pass-X kernel: the register kernel or the workgroup-phased one (debug bit kDbgTiledRows) where
// rows are short enough and the call is not forced onto the generic kernels; else the line pipeline if the caller has scratch
// for it (line_ws, rows_line_workspace_bytes), else a thread per row -- and then the y planes by launch_axis_bits, which the
// row kernels emit themselves.  row_kernels: the answer of row_pass_on_row_kernels for this call, which the caller needs itself
// (which planes exist, the index form) and therefore asks once and hands in; false for the one line of a 1-D call.
// log: the pass log names x_pass (and y_bits).
bool row_pass_on_row_kernels(int dtype, int64_t sx, int64_t sy, int64_t sz, bool force_generic);
int run_row_pass(const RowPass &rp, bool row_kernels, void *line_ws, bool log = false);

}  // namespace edt_amd

namespace edt_amd {
// ---- one process, several GPUs (host buffers): edt_multi.hip ----------------------------------------
bool multi_supported(int dtype, int64_t sx, int64_t sy, int64_t sz, int n_devices);
void multi_release();  // frees the per-slot pool (edt_hip_release_cache)
int run_multi(const void *labels, int dtype, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
              int flags, float *output, const int *devices, int n_devices);
}  // namespace edt_amd

namespace edt_amd {
// ---- connected components (run-based union-find, the output array is the parent array): edt_components.hip ----------
size_t components_workspace_bytes(int64_t voxels);  // the per-chunk root counts of the numbering scan
// shape, connectivity in 1..ndim, sx * sy * sz <= 2^31 - 1: what both entry points refuse before they look at a pointer
int components_check_args(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity,
                          const char *who = "connected_components");
// the forest (launch_forest, edt_forest.h), then scan, number, final on `stream`; out: sx * sy * sz uint32 (not the labels), n: one int64, both on the device
int launch_components(int dtype, const void *labels, int64_t sx, int64_t sy, int64_t sz, int connectivity, int binary,
                      uint32_t *out, int64_t *n, void *ws, hipStream_t stream);
// ---- dust (components kept or removed by size; sizes in the roots' own words of the parent plane): edt_dust.hip ----------
// what components_check_args refuses, then min_voxels < 0 and max_voxels < min_voxels
int dust_check_args(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity, int64_t min_voxels,
                    int64_t max_voxels);
// ---- watershed (the basins of a field by steepest ascent, as the components of a graph): edt_watershed.hip ----------
// what components_check_args refuses, then min_saliency negative or not finite
int watershed_check_args(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity, float min_saliency);
}  // namespace edt_amd
