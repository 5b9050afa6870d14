// edt_feature.hip -- the feature transform (nearest-boundary indices) and expand_labels on device-resident data.
//
// What is computed (include/edt_hip.h states the contract): for a foreground voxel p of label L, a voxel q with
// label(q) != L that minimises D(p,q) = wx^2 (px-qx)^2 + wy^2 (py-qy)^2 + wz^2 (pz-qz)^2, chosen by a separable tie rule.
// Three passes, X then Y then Z, each carrying the features of the previous one forward:
//   pass X (k_ft_rows, one wave per row): the nearer neighbour of p's run ends (a-1 on a tie), value ax * d^2;
//   pass Y/Z (k_ft_cols, one thread per column): per run [a,b] of one non-zero label along the column, the lower envelope
//     of the parabolas F[j] + a * (y-j)^2 over the rows j of the run with a finite F, then the border sites a-1 (wins ties)
//     and b+1 (loses ties).  The winner's carried coordinates plus its row are p's feature.
// Values are exact integers in quanta (int64) when the voxel sizes share one (q16_quantum: w_i^2 = a_i q), fp64 otherwise.
// The envelope is built on integer abscissae: the last row a candidate j keeps against a later candidate q is
// floor((F[q] - F[j] + a (q^2 - j^2)) / (2 a (q - j))), so ties go to the smaller row; no atomics, every column is one
// thread: the output does not depend on scheduling.
// The hull state (vertex row, first owned row) and each run's last row live in global memory at the volume's own
// addressing (entry k of column c at c + k * stride: lanes that agree on k access it coalesced), as in edt_generic.hip.
// The last pass either writes the features (int32 planes x, y, z) or, for expand_labels, gathers the label of the feature
// and applies the distance threshold -- the coordinates then never reach memory.
#include "edt_api_internal.h"

#pragma clang fp contract(off)

namespace edt_amd {
namespace {

// ---- value arithmetic: int64 quanta or fp64 ---------------------------------------------------------------------
template <typename V> __device__ __forceinline__ V v_inf();
template <> __device__ __forceinline__ int64_t v_inf<int64_t>() { return INT64_MAX; }
template <> __device__ __forceinline__ double v_inf<double>() { return __builtin_huge_val(); }

// a * d^2 (d >= 0 is a distance in voxels)
__device__ __forceinline__ int64_t v_cost(int64_t a, int64_t d) { return a * (d * d); }
__device__ __forceinline__ double v_cost(double a, int64_t d) { return a * (double)(d * d); }

// Candidate j (value fj) is at least as good as the later candidate q > j (value fq) at row y iff
// fj + a (y-j)^2 <= fq + a (y-q)^2  <=>  y <= num / den,  num = fq - fj + a (q^2 - j^2),  den = 2 a (q - j) > 0.
// The hull compares num with t * den instead of dividing (floor(num / den) < t  <=>  num < t * den); the one division a
// push needs (floor(num / den), known to lie in [0, n)) is an fp64 estimate corrected by one step in exact arithmetic.
// (The host keeps every |num| and t * den of the int64 path below 2^62: integer_values.)
__device__ __forceinline__ void kept_frac(int64_t fj, int64_t j, int64_t fq, int64_t q, int64_t a, int64_t &num, int64_t &den) {
  num = (fq - fj) + a * ((q - j) * (q + j));
  den = 2 * a * (q - j);
}
__device__ __forceinline__ void kept_frac(double fj, int64_t j, double fq, int64_t q, double a, double &num, double &den) {
  num = (fq - fj) + a * (double)((q - j) * (q + j));
  den = 2.0 * a * (double)(q - j);
}
__device__ __forceinline__ bool frac_below(int64_t num, int64_t den, int64_t t) { return num < t * den; }
__device__ __forceinline__ bool frac_below(double num, double den, int64_t t) { return num < (double)t * den; }
__device__ __forceinline__ int64_t frac_floor(int64_t num, int64_t den) {
  int64_t t = (int64_t)floor((double)num / (double)den);
  if (t * den > num) --t;
  else if ((t + 1) * den <= num) ++t;
  return t;
}
__device__ __forceinline__ int64_t frac_floor(double num, double den) { return (int64_t)floor(num / den); }

// ---- the last pass's output --------------------------------------------------------------------------------------
// FT: ndim int32 planes (x, y, z) of `voxels` each.  expand_labels: out[p] = labels[f] if f exists and
// D(p, f) <= d2 (fp64, the terms added in the order x, y, z; no fma), else labels[p] -- bit copies of the label type.
template <typename T>
struct FinalOut {
  int32_t *feat;      // FT planes (nullptr: expand_labels)
  const T *labels;    // expand_labels: the ORIGINAL labels (the transform runs on their background mask)
  T *out;
  int64_t voxels, sx, sy;
  int ndim;
  double w2x, w2y, w2z, d2;
};

template <typename T, bool EXPAND>
__device__ __forceinline__ void final_write(const FinalOut<T> &fo, int64_t p, int64_t px, int64_t py, int64_t pz,
                                            int32_t fx, int32_t fy, int32_t fz) {
  if (!EXPAND) {
    fo.feat[p] = fx;
    if (fo.ndim > 1) fo.feat[fo.voxels + p] = fy;
    if (fo.ndim > 2) fo.feat[2 * fo.voxels + p] = fz;
  } else {
    T v = fo.labels[p];
    if (fx >= 0) {
      const int64_t dx = px - fx, dy = py - fy, dz = pz - fz;
      const double D = (fo.w2x * (double)(dx * dx) + fo.w2y * (double)(dy * dy)) + fo.w2z * (double)(dz * dz);
      if (D <= fo.d2) v = fo.labels[fx + fo.sx * (fy + fo.sy * (int64_t)fz)];
    }
    fo.out[p] = v;
  }
}

// ---- pass X: one wave per row ---------------------------------------------------------------------------------------
// Sweep 1 (left to right, 64 voxels per step): the start of every voxel's run from the ballot of run starts, kept in
// `fx` for the moment.  Sweep 2 (right to left): the end of the run likewise, then the nearer bordered end's neighbour.
// FINAL (1-D calls): the result goes through final_write instead of (v, fx).
template <typename T, typename TO, typename V, bool FINAL, bool EXPAND>
__global__ __launch_bounds__(256) void k_ft_rows(const T *__restrict__ labels, int64_t sx, int64_t nrows, V ax, int bb,
                                                 V *__restrict__ vout, int32_t *__restrict__ fx, FinalOut<TO> fo) {
  const int lane = threadIdx.x & 63;
  const int64_t row = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= nrows) return;  // (uniform across the wave)
  const T *L = labels + row * sx;
  int32_t *F = fx + row * sx;
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < sx; c0 += 64) {
    const int64_t x = c0 + lane;
    bool st = false;
    if (x < sx) st = x == 0 || !(L[x - 1] == L[x]);
    const uint64_t m = __ballot(st) & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
    const int64_t start = m ? c0 + 63 - __builtin_clzll(m) : carry;
    if (x < sx) F[x] = (int32_t)start;
    carry = __shfl(start, 63);
  }
  int64_t carry_end = sx - 1;
  for (int64_t c0 = ((sx - 1) >> 6) << 6; c0 >= 0; c0 -= 64) {
    const int64_t x = c0 + lane;
    T lab = 0;
    bool en = false;
    if (x < sx) {
      lab = L[x];
      en = x == sx - 1 || !(L[x + 1] == lab);
    }
    const uint64_t m = __ballot(en) & (~0ull << lane);
    const int64_t end = m ? c0 + __builtin_ctzll(m) : carry_end;
    carry_end = __shfl(end, 0);
    if (x < sx) {
      V v;
      int64_t f;
      if (lab == 0) {
        v = 0;
        f = x;
      } else {
        const int64_t a = F[x], b = end;
        const bool left = bb || a > 0, right = bb || b < sx - 1;
        const int64_t dl = x - a + 1, dr = b + 1 - x;
        if (left && (!right || dl <= dr)) { v = v_cost(ax, dl); f = a - 1; }
        else if (right) { v = v_cost(ax, dr); f = b + 1; }
        else { v = v_inf<V>(); f = -1; }
      }
      if (FINAL) {
        final_write<TO, EXPAND>(fo, row * sx + x, x, 0, 0, (int32_t)f, f < 0 ? -1 : 0, f < 0 ? -1 : 0);
      } else {
        vout[row * sx + x] = v;
        F[x] = (int32_t)f;
      }
    }
  }
}

// ---- passes Y and Z: one thread per column ----------------------------------------------------------------------
// AXIS 1 (pass Y): column (x, z), rows y; candidates carry fx.  AXIS 2 (pass Z): column (x, y), rows z; they carry
// (fx, fy).  Sweep 1 builds the envelope of every run and records the run's last row at its first row (`re`); entries that
// can win no row of their run are dropped when the run closes, so the first-owned rows of the whole stack ascend and
// sweep 2 walks it with one index.  Sweep 2 evaluates every row: envelope vertex, then border a-1 (<=), border b+1 (<).
template <typename T, typename TO, typename V, int AXIS, bool FINAL, bool EXPAND>
__global__ __launch_bounds__(256) void k_ft_cols(const T *__restrict__ labels, AxisGeom g, V a, int bb,
                                                 const V *__restrict__ vin, const int32_t *__restrict__ fxin,
                                                 const int32_t *__restrict__ fyin, V *__restrict__ vout,
                                                 int32_t *__restrict__ fxout, int32_t *__restrict__ fyout,
                                                 int32_t *__restrict__ sv, int32_t *__restrict__ ss,
                                                 int32_t *__restrict__ re, FinalOut<TO> fo) {
  const int64_t col = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (col >= g.sx * g.nouter) return;
  const int64_t x = col % g.sx, o = col / g.sx;
  const int64_t base = x + o * g.outer_stride, st = g.stride, n = g.n;
  const T *lab = labels + base;
  const V *f = vin + base;
  int32_t *SV = sv + base, *SS = ss + base, *RE = re + base;

  // ---- sweep 1 ----
  int64_t top = -1, kb = 0;         // stack top, first entry of the current run
  int64_t tv = 0, ts = 0;           // cached top entry: row, first row it owns
  V tf = 0;                         //                   its value
  int64_t a0 = 0;
  bool fg = false;
  T prev = 0;
  for (int64_t i = 0; i <= n; ++i) {
    T li = 0;
    bool start = true;
    if (i < n) {
      li = lab[i * st];
      start = i == 0 || !(li == prev);
    }
    if (start) {
      if (i > 0 && fg) {  // close the run [a0, i-1]
        const int64_t b0 = i - 1;
        RE[a0 * st] = (int32_t)b0;
        while (top >= kb && ts > b0) {
          --top;
          if (top >= kb) ts = SS[top * st];
        }
      }
      if (i == n) break;
      a0 = i;
      fg = !(li == 0);
      kb = top + 1;
    }
    prev = li;
    if (!fg) continue;
    const V fi = f[i * st];
    if (fi == v_inf<V>()) continue;
    int64_t s = a0;
    bool wins = true;
    while (top >= kb) {
      V num, den;
      kept_frac(tf, tv, fi, i, a, num, den);
      if (!frac_below(num, den, ts)) {  // the top keeps row ts against i: i starts at floor(num / den) + 1
        if (frac_below(num, den, n - 1)) s = frac_floor(num, den) + 1;
        else wins = false;  // wins no row of the column (the entries below keep every row from it)
        break;
      }
      --top;
      if (top >= kb) {
        tv = SV[top * st];
        ts = SS[top * st];
        tf = f[tv * st];
      }
    }
    if (!wins) continue;
    ++top;
    SV[top * st] = (int32_t)i;
    SS[top * st] = (int32_t)s;
    tv = i; ts = s; tf = fi;
  }

  // ---- sweep 2 ----
  int64_t k = -1;
  int64_t next_s = top >= 0 ? SS[0] : INT64_MAX;
  int64_t cv = -1;
  V cf = 0;
  int32_t cfx = 0, cfy = 0;
  int64_t b0 = -1;
  a0 = 0;
  fg = false;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t p = base + i * st;
    if (i > b0) {
      a0 = i;
      fg = !(lab[i * st] == 0);
      b0 = fg ? (int64_t)RE[i * st] : i;
    }
    // own coordinates
    const int32_t px = (int32_t)x;
    const int32_t py = AXIS == 1 ? (int32_t)i : (int32_t)o;
    const int32_t pz = AXIS == 1 ? (int32_t)o : (int32_t)i;
    int32_t rx, ry, rz;
    V best;
    if (!fg) {
      best = 0; rx = px; ry = py; rz = pz;
    } else {
      while (next_s <= i) {
        ++k;
        cv = SV[k * st];
        cf = f[cv * st];
        cfx = fxin[base + cv * st];
        if (AXIS == 2) cfy = fyin[base + cv * st];
        next_s = k < top ? SS[(k + 1) * st] : INT64_MAX;
      }
      best = v_inf<V>();
      int src = 0;  // 0: none, 1: envelope vertex, 2: border a0-1, 3: border b0+1
      if (k >= 0 && cv >= a0) { best = cf + v_cost(a, i - cv); src = 1; }
      if (bb || a0 > 0) {
        const V bl = v_cost(a, i - a0 + 1);
        if (bl <= best) { best = bl; src = 2; }
      }
      if (bb || b0 < n - 1) {
        const V br = v_cost(a, b0 + 1 - i);
        if (br < best) { best = br; src = 3; }
      }
      const int32_t row = src == 1 ? (int32_t)cv : src == 2 ? (int32_t)(a0 - 1) : (int32_t)(b0 + 1);
      if (src == 0) {
        rx = ry = rz = -1;
      } else if (AXIS == 1) {
        rx = src == 1 ? cfx : px; ry = row; rz = pz;
      } else {
        rx = src == 1 ? cfx : px; ry = src == 1 ? cfy : py; rz = row;
      }
    }
    if (FINAL) {
      final_write<TO, EXPAND>(fo, p, px, py, pz, rx, ry, rz);
    } else {
      vout[p] = best;
      fxout[p] = rx;
      fyout[p] = ry;
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
struct FtBuffers {
  void *va = nullptr, *vb = nullptr;                                   // pass values (8 bytes per voxel)
  int32_t *fxa = nullptr, *fxb = nullptr, *fyb = nullptr;              // carried coordinates
  int32_t *sv = nullptr, *ss = nullptr, *re = nullptr;                 // hull stacks, run ends
  size_t bytes = 0;
};

FtBuffers carve_ft(void *ws, int ndim, int64_t voxels) {
  Carver c(ws);
  FtBuffers b;
  const size_t nv = (size_t)voxels;
  b.fxa = c.take<int32_t>(nv);
  if (ndim >= 2) {
    b.va = c.take<int64_t>(nv);
    b.sv = c.take<int32_t>(nv);
    b.ss = c.take<int32_t>(nv);
    b.re = c.take<int32_t>(nv);
  }
  if (ndim == 3) {
    b.vb = c.take<int64_t>(nv);
    b.fxb = c.take<int32_t>(nv);
    b.fyb = c.take<int32_t>(nv);
  }
  b.bytes = align_up(c.off, 256);
  return b;
}

struct FtCall {
  int ndim;
  int64_t sx, sy, sz;
  float w[3];
  int bb;
};

// T: the labels whose runs the passes follow; TO: the label type of expand_labels' output (uint8_t for the FT: unused).
// Only the last pass reads `fo`: the passes before it are the same kernels for the FT and for expand_labels (TO = uint8_t).
template <typename T, typename TO, typename V, bool EXPAND>
int launch_ft_t(const T *labels, const FtCall &c, const V av[3], const FtBuffers &b, const FinalOut<TO> &fo,
                hipStream_t stream) {
  const FinalOut<uint8_t> none = {};
  const int64_t nrows = c.sy * c.sz;
  {
    ScopedPass sp(EXPAND ? "expand pass X" : "ft pass X", stream);
    const unsigned blocks = (unsigned)ceil_div(nrows, 4);
    if (c.ndim == 1)
      hipLaunchKernelGGL((k_ft_rows<T, TO, V, true, EXPAND>), dim3(blocks), dim3(256), 0, stream, labels, c.sx, nrows, av[0],
                         c.bb, (V *)b.va, b.fxa, fo);
    else
      hipLaunchKernelGGL((k_ft_rows<T, uint8_t, V, false, false>), dim3(blocks), dim3(256), 0, stream, labels, c.sx, nrows,
                         av[0], c.bb, (V *)b.va, b.fxa, none);
    EDT_HIP_TRY(hipGetLastError());
  }
  if (c.ndim == 1) return EDT_OK;
  {
    ScopedPass sp(EXPAND ? "expand pass Y" : "ft pass Y", stream);
    const AxisGeom g = make_geom_y(c.sx, c.sy, c.sz);
    const unsigned blocks = (unsigned)ceil_div(g.sx * g.nouter, 256);
    if (c.ndim == 2)
      hipLaunchKernelGGL((k_ft_cols<T, TO, V, 1, true, EXPAND>), dim3(blocks), dim3(256), 0, stream, labels, g, av[1], c.bb,
                         (const V *)b.va, b.fxa, nullptr, nullptr, nullptr, nullptr, b.sv, b.ss, b.re, fo);
    else
      hipLaunchKernelGGL((k_ft_cols<T, uint8_t, V, 1, false, false>), dim3(blocks), dim3(256), 0, stream, labels, g, av[1],
                         c.bb, (const V *)b.va, b.fxa, nullptr, (V *)b.vb, b.fxb, b.fyb, b.sv, b.ss, b.re, none);
    EDT_HIP_TRY(hipGetLastError());
  }
  if (c.ndim == 2) return EDT_OK;
  {
    ScopedPass sp(EXPAND ? "expand pass Z" : "ft pass Z", stream);
    const AxisGeom g = make_geom_z(c.sx, c.sy, c.sz);
    const unsigned blocks = (unsigned)ceil_div(g.sx * g.nouter, 256);
    hipLaunchKernelGGL((k_ft_cols<T, TO, V, 2, true, EXPAND>), dim3(blocks), dim3(256), 0, stream, labels, g, av[2], c.bb,
                       (const V *)b.vb, b.fxb, b.fyb, nullptr, nullptr, nullptr, b.sv, b.ss, b.re, fo);
    EDT_HIP_TRY(hipGetLastError());
  }
  return EDT_OK;
}

// Where the voxel sizes share a quantum and every value of the call (the pass values, and the numerators of the envelope
// intersections: at most 4 * sum a_i (s_i + 1)^2) stays below 2^62, the passes run on exact int64 quanta.
bool integer_values(const FtCall &c, int64_t a[3]) {
  const Quantum Q = q16_quantum(c.w, c.ndim);
  if (!Q.ok) return false;
  const int64_t s[3] = {c.sx, c.sy, c.sz};
  double bound = 0.0;
  for (int i = 0; i < c.ndim; ++i) bound += (double)Q.a[i] * (double)(s[i] + 1) * (double)(s[i] + 1);
  if (4.0 * bound >= 4.0e18) return false;
  for (int i = 0; i < 3; ++i) a[i] = Q.a[i];
  return true;
}

template <typename T, typename TO, bool EXPAND>
int launch_ft_typed(const T *labels, const FtCall &c, const FtBuffers &b, const FinalOut<TO> &fo, hipStream_t stream) {
  int64_t ai[3] = {1, 1, 1};
  if (integer_values(c, ai)) return launch_ft_t<T, TO, int64_t, EXPAND>(labels, c, ai, b, fo, stream);
  const double ad[3] = {(double)c.w[0] * (double)c.w[0], (double)c.w[1] * (double)c.w[1], (double)c.w[2] * (double)c.w[2]};
  return launch_ft_t<T, TO, double, EXPAND>(labels, c, ad, b, fo, stream);
}

template <typename T>
FinalOut<T> final_out(const FtCall &c, int32_t *feat, const T *labels, T *out, double distance) {
  FinalOut<T> fo;
  fo.feat = feat;
  fo.labels = labels;
  fo.out = out;
  fo.voxels = c.sx * c.sy * c.sz;
  fo.sx = c.sx;
  fo.sy = c.sy;
  fo.ndim = c.ndim;
  fo.w2x = (double)c.w[0] * (double)c.w[0];
  fo.w2y = c.ndim > 1 ? (double)c.w[1] * (double)c.w[1] : 0.0;
  fo.w2z = c.ndim > 2 ? (double)c.w[2] * (double)c.w[2] : 0.0;
  fo.d2 = distance * distance;
  return fo;
}

int launch_ft(int dtype, const void *labels, const FtCall &c, const FtBuffers &b, int32_t *feat, hipStream_t stream) {
  const FinalOut<uint8_t> fo = final_out<uint8_t>(c, feat, nullptr, nullptr, 0.0);
  switch (dtype) {
    case EDT_U8: case EDT_BOOL: return launch_ft_typed<uint8_t, uint8_t, false>((const uint8_t *)labels, c, b, fo, stream);
    case EDT_U16: return launch_ft_typed<uint16_t, uint8_t, false>((const uint16_t *)labels, c, b, fo, stream);
    case EDT_U32: return launch_ft_typed<uint32_t, uint8_t, false>((const uint32_t *)labels, c, b, fo, stream);
    case EDT_U64: return launch_ft_typed<uint64_t, uint8_t, false>((const uint64_t *)labels, c, b, fo, stream);
    case EDT_F32: return launch_ft_typed<float, uint8_t, false>((const float *)labels, c, b, fo, stream);
    case EDT_F64: return launch_ft_typed<double, uint8_t, false>((const double *)labels, c, b, fo, stream);
    default: set_error("unknown dtype"); return EDT_ERR_BAD_ARG;
  }
}

// expand_labels: the transform runs on the background mask (uint8, label 1 = background of `labels`); the last pass
// copies labels bit for bit, so T is the unsigned type of the label's width
template <typename T>
int launch_expand_t(const uint8_t *mask, const void *labels, void *out, const FtCall &c, const FtBuffers &b, double distance,
                    hipStream_t stream) {
  return launch_ft_typed<uint8_t, T, true>(mask, c, b, final_out<T>(c, nullptr, (const T *)labels, (T *)out, distance), stream);
}

}  // namespace
}  // namespace edt_amd

using namespace edt_amd;

static int ft_validate(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float &wx, float &wy, float &wz) {
  int rc = check_shape(dtype, ndim, sx, sy, sz);
  if (rc != EDT_OK) return rc;
  return check_voxel_sizes(ndim, wx, wy, wz);
}

extern "C" {

size_t edt_hip_feature_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int flags) {
  if (check_shape(dtype, ndim, sx, sy, sz) != EDT_OK) return 0;
  if (flags & ~(EDT_FLAG_BLACK_BORDER | EDT_FLAG_FORCE_GENERIC)) return 0;
  return carve_ft(nullptr, ndim, sx * sy * sz).bytes;
}

int edt_hip_feature_transform_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx,
                                     float wy, float wz, int flags, int32_t *d_features, void *d_workspace,
                                     size_t workspace_bytes, void *stream) {
  int rc = ft_validate(dtype, ndim, sx, sy, sz, wx, wy, wz);
  if (rc != EDT_OK) return rc;
  if (flags & ~(EDT_FLAG_BLACK_BORDER | EDT_FLAG_FORCE_GENERIC)) {
    set_error("feature transform: flags other than EDT_FLAG_BLACK_BORDER / EDT_FLAG_FORCE_GENERIC");
    return EDT_ERR_UNSUPPORTED;
  }
  const int64_t voxels = sx * sy * sz;
  if (voxels == 0) return EDT_OK;
  if (!d_labels || !d_features) { set_error("null device pointer"); return EDT_ERR_BAD_ARG; }
  const size_t need = carve_ft(nullptr, ndim, voxels).bytes;
  if (!d_workspace || workspace_bytes < need) {
    set_error("feature transform: workspace missing or smaller than edt_hip_feature_workspace_bytes()");
    return EDT_ERR_BAD_ARG;
  }
  if ((rc = check_workspace_alignment(d_workspace)) != EDT_OK) return rc;
  const FtCall c = {ndim, sx, sy, sz, {wx, wy, wz}, (flags & EDT_FLAG_BLACK_BORDER) ? 1 : 0};
  if (g_log.enabled.load(std::memory_order_relaxed)) {
    std::lock_guard<std::mutex> lock(g_log_mutex);
    log_begin_call();
  }
  return launch_ft(dtype, d_labels, c, carve_ft(d_workspace, ndim, voxels), d_features, (hipStream_t)stream);
}

size_t edt_hip_expand_labels_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz) {
  if (check_shape(dtype, ndim, sx, sy, sz) != EDT_OK) return 0;
  const int64_t voxels = sx * sy * sz;
  return align_up((size_t)voxels, 256) + carve_ft(nullptr, ndim, voxels).bytes;
}

int edt_hip_expand_labels_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx,
                                 float wy, float wz, double distance, void *d_out, void *d_workspace, size_t workspace_bytes,
                                 void *stream) {
  int rc = ft_validate(dtype, ndim, sx, sy, sz, wx, wy, wz);
  if (rc != EDT_OK) return rc;
  if (!(distance >= 0.0)) { set_error("expand_labels: distance must be >= 0 (inf allowed)"); return EDT_ERR_BAD_ARG; }
  const int64_t voxels = sx * sy * sz;
  if (voxels == 0) return EDT_OK;
  if (!d_labels || !d_out) { set_error("null device pointer"); return EDT_ERR_BAD_ARG; }
  if (d_out == d_labels) { set_error("expand_labels: d_out may not alias d_labels"); return EDT_ERR_BAD_ARG; }
  const size_t mbytes = align_up((size_t)voxels, 256);
  if (!d_workspace || workspace_bytes < mbytes + carve_ft(nullptr, ndim, voxels).bytes) {
    set_error("expand_labels: workspace missing or smaller than edt_hip_expand_labels_workspace_bytes()");
    return EDT_ERR_BAD_ARG;
  }
  if ((rc = check_workspace_alignment(d_workspace)) != EDT_OK) return rc;
  const FtCall c = {ndim, sx, sy, sz, {wx, wy, wz}, 0};
  hipStream_t s = (hipStream_t)stream;
  if (g_log.enabled.load(std::memory_order_relaxed)) {
    std::lock_guard<std::mutex> lock(g_log_mutex);
    log_begin_call();
  }
  uint8_t *mask = (uint8_t *)d_workspace;
  const FtBuffers b = carve_ft((char *)d_workspace + mbytes, ndim, voxels);
  {
    ScopedPass sp("expand mask", s);
    if ((rc = launch_is_background(dtype, d_labels, mask, voxels, s)) != EDT_OK) return rc;
  }
  return with_label_type(dtype, [&](auto t) {
    // (labels are only copied: a float label travels as the unsigned integer of its size)
    using T = typename decltype(t)::type;
    using U = std::conditional_t<sizeof(T) == 4, uint32_t, std::conditional_t<sizeof(T) == 8, uint64_t, T>>;
    return launch_expand_t<U>(mask, d_labels, d_out, c, b, distance, s);
  });
}

}  // extern "C"
