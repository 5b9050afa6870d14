// edt_morph.hip -- the two streaming kernels of the morphology operations (include/edt_hip.h, "morphology") and their device
// entry points: the mask labels != 0, and the select that turns a squared-distance field into an eroded / opened / closed label
// volume (or into the mask of the voxels that did not pass).  The composition -- which transform feeds which select -- lives one
// layer up: edt_hip_morphology (edt_host.hip) and edt/device.py own the field and the mask.
//
// Form.  Both kernels move 2 to 29 bytes per voxel and compute next to nothing: a fixed grid of 2048 workgroups of 256 threads
// and a stride loop.  A thread takes FOUR consecutive voxels per trip: one 16-byte piece of the fp32 field, 4 / 8 / 16 / 2 x 16
// bytes of labels of 1 / 2 / 4 / 8 bytes and 4 bytes of mask, so that every wave instruction covers one contiguous stretch of
// memory -- where every pointer of the call has the alignment of its piece; otherwise a thread takes one voxel per trip.  The
// same bits either way.  Measured at 512^3: whole 16-byte pieces of 1-byte labels -- sixteen voxels and four
// strided field loads per thread -- ran the select at 4.5 TB/s, eight voxels at 5.9, four at 6.4; 4-byte labels are the same
// kernel in all three.  The field is read once and by nobody after the select: its loads are non-temporal (plain loads: 6 %
// slower on 4-byte labels, 17 % on 1-byte labels).
//
// Labels travel as the unsigned integer of their width, so that a NaN keeps its payload and nothing depends on the denormal mode;
// "!= 0" with the type's own comparison is, on those bits: any bit set (integers, bool bytes), any bit but the sign set (floats:
// -0.0 is zero, a NaN and a denormal are not).
#include <type_traits>

#include "edt_api_internal.h"

namespace edt_amd {
namespace {

constexpr int kMorphThreads = 256;
constexpr int64_t kMorphBlocks = 2048;  // 8 workgroups on each of the 256 CUs; the stride loop takes the rest

template <typename U, bool FL>
__device__ __forceinline__ bool label_nonzero(U bits) {
  return FL ? (U)(bits << 1) != 0 : bits != 0;
}

// the four voxels a thread takes per trip of the vector form, as label pieces of at most 16 bytes
template <typename U>
struct Chunk {
  static constexpr int kVoxels = 4;
  static constexpr int kPiece = 4 * (int)sizeof(U) <= 16 ? 4 : 16 / (int)sizeof(U);   // labels in one piece
  static constexpr int kPieceBytes = kPiece * (int)sizeof(U);
};

template <typename U>
__device__ __forceinline__ void load_labels(U (&v)[Chunk<U>::kVoxels], const U *p) {
  typedef U piece_t __attribute__((ext_vector_type(Chunk<U>::kPiece)));
#pragma unroll
  for (int q = 0; q < Chunk<U>::kVoxels / Chunk<U>::kPiece; ++q) {
    const piece_t t = reinterpret_cast<const piece_t *>(p)[q];
#pragma unroll
    for (int k = 0; k < Chunk<U>::kPiece; ++k) v[q * Chunk<U>::kPiece + k] = t[k];
  }
}

template <typename U>
__device__ __forceinline__ void store_labels(U *p, const U (&v)[Chunk<U>::kVoxels]) {
  typedef U piece_t __attribute__((ext_vector_type(Chunk<U>::kPiece)));
#pragma unroll
  for (int q = 0; q < Chunk<U>::kVoxels / Chunk<U>::kPiece; ++q) {
    piece_t t;
#pragma unroll
    for (int k = 0; k < Chunk<U>::kPiece; ++k) t[k] = v[q * Chunk<U>::kPiece + k];
    reinterpret_cast<piece_t *>(p)[q] = t;
  }
}

template <int N>
__device__ __forceinline__ void store_mask(uint8_t *p, const uint8_t (&m)[N]) {
  typedef uint8_t mask_t __attribute__((ext_vector_type(N)));
  mask_t t;
#pragma unroll
  for (int k = 0; k < N; ++k) t[k] = m[k];
  *reinterpret_cast<mask_t *>(p) = t;
}

__device__ __forceinline__ bool field_passes(float f, double r2, int within) {
  return within ? (double)f <= r2 : (double)f > r2;
}

// mask[i] = labels[i] != 0
template <typename U, bool FL, bool VEC>
__global__ __launch_bounds__(kMorphThreads) void k_is_foreground(const U *__restrict__ labels, uint8_t *__restrict__ mask,
                                                                 int64_t count) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  int64_t done = 0;
  if constexpr (VEC) {
    constexpr int V = Chunk<U>::kVoxels;
    const int64_t chunks = count / V;
    for (int64_t c = tid; c < chunks; c += step) {
      U v[V];
      uint8_t m[V];
      load_labels<U>(v, labels + c * V);
#pragma unroll
      for (int k = 0; k < V; ++k) m[k] = label_nonzero<U, FL>(v[k]) ? 1 : 0;
      store_mask<V>(mask + c * V, m);
    }
    done = chunks * V;
  }
  for (int64_t i = done + tid; i < count; i += step) mask[i] = label_nonzero<U, FL>(labels[i]) ? 1 : 0;
}

// pass(i) = field[i] > r2 (within = 0) or field[i] <= r2 (within = 1), compared in fp64; guard: pass |= guard[i] != 0;
// out[i] = pass ? values[i] : 0 (out == values allowed: a thread reads the voxels it writes, and only those); mask[i] = !pass.
// values is read only where out is written.
template <typename U, bool FL, bool VEC>
__global__ __launch_bounds__(kMorphThreads) void k_morph_select(const U *values, const U *guard,
                                                                const float *__restrict__ field, double r2, int within, U *out,
                                                                uint8_t *__restrict__ mask, int64_t count) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  int64_t done = 0;
  if constexpr (VEC) {
    constexpr int V = Chunk<U>::kVoxels;
    typedef float f4_t __attribute__((ext_vector_type(4)));
    const int64_t chunks = count / V;
    for (int64_t c = tid; c < chunks; c += step) {
      const int64_t i = c * V;
      bool pass[V];
      // the field is read once and by nobody after this kernel: it need not stay in the caches
#pragma unroll
      for (int q = 0; q < V / 4; ++q) {
        const f4_t f = __builtin_nontemporal_load(reinterpret_cast<const f4_t *>(field + i) + q);
#pragma unroll
        for (int k = 0; k < 4; ++k) pass[4 * q + k] = field_passes(f[k], r2, within);
      }
      if (guard) {
        U g[V];
        load_labels<U>(g, guard + i);
#pragma unroll
        for (int k = 0; k < V; ++k) pass[k] = pass[k] || label_nonzero<U, FL>(g[k]);
      }
      if (out) {
        U v[V];
        load_labels<U>(v, values + i);
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = pass[k] ? v[k] : U(0);
        store_labels<U>(out + i, v);
      }
      if (mask) {
        uint8_t m[V];
#pragma unroll
        for (int k = 0; k < V; ++k) m[k] = pass[k] ? 0 : 1;
        store_mask<V>(mask + i, m);
      }
    }
    done = chunks * V;
  }
  for (int64_t i = done + tid; i < count; i += step) {
    bool pass = field_passes(field[i], r2, within);
    if (guard) pass = pass || label_nonzero<U, FL>(guard[i]);
    if (out) out[i] = pass ? values[i] : U(0);
    if (mask) mask[i] = pass ? 0 : 1;
  }
}

bool aligned(const void *p, int bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }  // (a null pointer is aligned: it is not used)

unsigned morph_blocks(int64_t items) {
  const int64_t blocks = ceil_div(items, kMorphThreads);
  return (unsigned)(blocks > kMorphBlocks ? kMorphBlocks : blocks);
}

// f(carrier type tag, is-float tag): the unsigned integer of the labels' width, and whether "!= 0" ignores the sign bit
template <typename F>
int with_carrier(int dtype, F &&f) {
  switch (dtype) {
    case EDT_U8: case EDT_BOOL: return f(LabelType<uint8_t>{}, std::false_type{});
    case EDT_U16: return f(LabelType<uint16_t>{}, std::false_type{});
    case EDT_U32: return f(LabelType<uint32_t>{}, std::false_type{});
    case EDT_U64: return f(LabelType<uint64_t>{}, std::false_type{});
    case EDT_F32: return f(LabelType<uint32_t>{}, std::true_type{});
    case EDT_F64: return f(LabelType<uint64_t>{}, std::true_type{});
    default: set_error("unknown dtype code"); return EDT_ERR_BAD_ARG;
  }
}

}  // namespace

int launch_is_foreground(int dtype, const void *labels, uint8_t *mask, int64_t count, hipStream_t stream) {
  if (count <= 0) return EDT_OK;
  return with_carrier(dtype, [&](auto t, auto fl) -> int {
    using U = typename decltype(t)::type;
    constexpr bool FL = decltype(fl)::value;
    const bool vec = aligned(labels, Chunk<U>::kPieceBytes) && aligned(mask, Chunk<U>::kVoxels);
    if (vec)
      hipLaunchKernelGGL((k_is_foreground<U, FL, true>), dim3(morph_blocks(ceil_div(count, Chunk<U>::kVoxels))), dim3(kMorphThreads), 0,
                         stream, (const U *)labels, mask, count);
    else
      hipLaunchKernelGGL((k_is_foreground<U, FL, false>), dim3(morph_blocks(count)), dim3(kMorphThreads), 0, stream, (const U *)labels,
                         mask, count);
    EDT_HIP_TRY(hipGetLastError());
    return EDT_OK;
  });
}

int launch_morph_select(int dtype, const void *values, const void *guard, const float *field, double r2, int rule, void *out,
                        uint8_t *mask, int64_t count, hipStream_t stream) {
  if (count <= 0) return EDT_OK;
  const int within = rule == EDT_MORPH_WITHIN ? 1 : 0;
  return with_carrier(dtype, [&](auto t, auto fl) -> int {
    using U = typename decltype(t)::type;
    constexpr bool FL = decltype(fl)::value;
    constexpr int kLabels = Chunk<U>::kPieceBytes;
    const bool vec = aligned(values, kLabels) && aligned(guard, kLabels) && aligned(out, kLabels) && aligned(field, 16) &&
                     aligned(mask, Chunk<U>::kVoxels);
    if (vec)
      hipLaunchKernelGGL((k_morph_select<U, FL, true>), dim3(morph_blocks(ceil_div(count, Chunk<U>::kVoxels))), dim3(kMorphThreads), 0,
                         stream, (const U *)values, (const U *)guard, field, r2, within, (U *)out, mask, count);
    else
      hipLaunchKernelGGL((k_morph_select<U, FL, false>), dim3(morph_blocks(count)), dim3(kMorphThreads), 0, stream, (const U *)values,
                         (const U *)guard, field, r2, within, (U *)out, mask, count);
    EDT_HIP_TRY(hipGetLastError());
    return EDT_OK;
  });
}

int morph_radius_squared(double radius, bool inf_allowed, const char *who, double *r2) {
  *r2 = radius * radius;
  if (!(radius >= 0.0) || (!(*r2 <= DBL_MAX) && !(inf_allowed && radius > DBL_MAX))) {  // (a finite radius whose square overflows is refused)
    set_error(std::string(who) + ": radius must be >= 0 and its square finite" + (inf_allowed ? " (+inf allowed)" : ""));
    return EDT_ERR_BAD_ARG;
  }
  return EDT_OK;
}

}  // namespace edt_amd

using namespace edt_amd;

extern "C" {

int edt_hip_is_foreground_device(const void *d_labels, int dtype, uint8_t *d_mask, int64_t count, void *stream) {
  if (count < 0 || dtype_size(dtype) == 0) { set_error("is_foreground: bad count or dtype code"); return EDT_ERR_BAD_ARG; }
  if (count == 0) return EDT_OK;
  if (!d_labels || !d_mask) { set_error("is_foreground: null device pointer"); return EDT_ERR_BAD_ARG; }
  if (const int rc = require_device()) return rc;
  return launch_is_foreground(dtype, d_labels, d_mask, count, (hipStream_t)stream);
}

int edt_hip_morph_select_device(const void *d_values, const void *d_guard, int dtype, const float *d_field, double radius, int rule,
                                void *d_out, uint8_t *d_mask, int64_t count, void *stream) {
  if (count < 0 || dtype_size(dtype) == 0) { set_error("morph_select: bad count or dtype code"); return EDT_ERR_BAD_ARG; }
  if (rule != EDT_MORPH_FARTHER && rule != EDT_MORPH_WITHIN) { set_error("morph_select: rule must be EDT_MORPH_FARTHER or EDT_MORPH_WITHIN"); return EDT_ERR_BAD_ARG; }
  double r2;
  if (const int rc = morph_radius_squared(radius, false, "morph_select", &r2)) return rc;
  if (!d_out && !d_mask) { set_error("morph_select: at least one of d_out and d_mask"); return EDT_ERR_BAD_ARG; }
  if (count == 0) return EDT_OK;
  if (!d_field || (d_out && !d_values)) { set_error("morph_select: null device pointer"); return EDT_ERR_BAD_ARG; }
  if (const int rc = require_device()) return rc;
  return launch_morph_select(dtype, d_values, d_guard, d_field, r2, rule, d_out, d_mask, count, (hipStream_t)stream);
}

}  // extern "C"
