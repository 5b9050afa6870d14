// edt_morph.hip -- the two streaming kernels of the morphology operations (include/edt_hip.h, "morphology") and their device
// entry points: the mask labels != 0, and the select that turns a squared-distance field into an eroded / opened / closed label
// volume (or into the mask of the voxels that did not pass).  The composition -- which transform feeds which select -- lives one
// layer up: edt_hip_morphology_device (edt_fieldops.hip) carves the field and the mask.  Further down, in the same form: the
// step kernel of local thickness (include/edt_hip.h, "local thickness") and its device entry point.
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

// One step of local thickness (include/edt_hip.h, "local thickness"), in k_morph_select's form: four consecutive voxels per thread
// -- 16 bytes of S, B and T, 4 of the mask -- where every pointer allows it.  STEP0 (no B): T = 0 and the largest finite S, as its
// bits.  Otherwise T = rf where the voxel lies in the opening of this radius (foreground, and within r of what the erosion left),
// untouched elsewhere, and the number of those voxels.  Either way the mask of the next radius, if there is one.  B is read once
// and by nobody afterwards (non-temporal); S is read again by every step (plain loads).  The counters: summed in the wave, across
// the workgroup through LDS, one atomic per workgroup.
// S > 0 is taken on the bits (0 < bits <= those of +inf), so that a denormal is foreground whatever the denormal mode.
__device__ __forceinline__ bool field_positive(float s) { return __float_as_uint(s) - 1u < 0x7F800000u; }
__device__ __forceinline__ uint32_t finite_bits(float s) {   // the bits of a finite s >= 0, else 0
  const uint32_t b = __float_as_uint(s);
  return b < 0x7F800000u ? b : 0u;
}

template <bool VEC, bool STEP0>
__global__ __launch_bounds__(kMorphThreads) void k_thickness_step(const float *__restrict__ S, const float *__restrict__ B, double r2,
                                                                  float rf, double next2, float *__restrict__ T,
                                                                  uint8_t *__restrict__ mask, unsigned long long *size,
                                                                  uint32_t *smax_bits, int64_t count) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  unsigned long long n_in = 0;
  uint32_t top = 0;
  int64_t done = 0;
  if constexpr (VEC) {
    typedef float f4_t __attribute__((ext_vector_type(4)));
    const int64_t chunks = count / 4;
    for (int64_t c = tid; c < chunks; c += step) {
      const int64_t i = c * 4;
      const f4_t s = *reinterpret_cast<const f4_t *>(S + i);
      if constexpr (STEP0) {
        *reinterpret_cast<f4_t *>(T + i) = f4_t{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 4; ++k) top = max(top, finite_bits(s[k]));
      } else {
        const f4_t b = __builtin_nontemporal_load(reinterpret_cast<const f4_t *>(B + i));
        bool in[4];
        int n = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          in[k] = field_positive(s[k]) && (double)b[k] <= r2;
          n += in[k] ? 1 : 0;
        }
        // the thread's own four voxels of T are loaded, blended and stored in one piece (measured against one 16-byte store where
        // all four are in and single stores otherwise, which moves fewer bytes: 17 - 20 % slower)
        if (n) {
          f4_t t = *reinterpret_cast<const f4_t *>(T + i);
#pragma unroll
          for (int k = 0; k < 4; ++k) t[k] = in[k] ? rf : t[k];
          *reinterpret_cast<f4_t *>(T + i) = t;
        }
        n_in += (unsigned)n;
      }
      if (mask) {
        uint8_t m[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = (double)s[k] > next2 ? 0 : 1;
        store_mask<4>(mask + i, m);
      }
    }
    done = chunks * 4;
  }
  for (int64_t i = done + tid; i < count; i += step) {
    const float s = S[i];
    if constexpr (STEP0) {
      T[i] = 0.0f;
      top = max(top, finite_bits(s));
    } else {
      if (field_positive(s) && (double)B[i] <= r2) {
        T[i] = rf;
        ++n_in;
      }
    }
    if (mask) mask[i] = (double)s > next2 ? 0 : 1;
  }
  constexpr int kWaves = kMorphThreads / 64;
  if constexpr (STEP0) {
    if (smax_bits) {
      __shared__ uint32_t s_top[kWaves];
      for (int m = 32; m >= 1; m >>= 1) top = max(top, (uint32_t)__shfl_xor(top, m));
      if ((threadIdx.x & 63) == 0) s_top[threadIdx.x >> 6] = top;
      __syncthreads();
      if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) top = max(top, s_top[w]);
        if (top) atomicMax(smax_bits, top);
      }
    }
  } else {
    if (size) {
      __shared__ unsigned long long s_in[kWaves];
      for (int m = 32; m >= 1; m >>= 1) n_in += __shfl_xor(n_in, m);
      if ((threadIdx.x & 63) == 0) s_in[threadIdx.x >> 6] = n_in;
      __syncthreads();
      if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) n_in += s_in[w];
        if (n_in) atomicAdd(size, n_in);
      }
    }
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

int launch_thickness_step(const float *S, const float *B, double r2, float rf, double next2, float *T, uint8_t *mask, int64_t *size,
                          uint32_t *smax_bits, int64_t count, hipStream_t stream) {
  if (count <= 0) return EDT_OK;
  const bool vec = aligned(S, 16) && aligned(B, 16) && aligned(T, 16) && aligned(mask, 4);
  const dim3 grid(morph_blocks(vec ? ceil_div(count, 4) : count)), block(kMorphThreads);
  unsigned long long *const n = reinterpret_cast<unsigned long long *>(size);
  if (vec && !B) hipLaunchKernelGGL((k_thickness_step<true, true>), grid, block, 0, stream, S, B, r2, rf, next2, T, mask, n, smax_bits, count);
  else if (vec) hipLaunchKernelGGL((k_thickness_step<true, false>), grid, block, 0, stream, S, B, r2, rf, next2, T, mask, n, smax_bits, count);
  else if (!B) hipLaunchKernelGGL((k_thickness_step<false, true>), grid, block, 0, stream, S, B, r2, rf, next2, T, mask, n, smax_bits, count);
  else hipLaunchKernelGGL((k_thickness_step<false, false>), grid, block, 0, stream, S, B, r2, rf, next2, T, mask, n, smax_bits, count);
  EDT_HIP_TRY(hipGetLastError());
  return EDT_OK;
}

int thickness_radius_squared(double radius, const char *who, double *r2) {
  *r2 = radius * radius;
  if (!(radius > 0.0) || !(*r2 <= DBL_MAX)) {  // (NaN, zero, negative, +inf, and a finite radius whose square overflows)
    set_error(std::string(who) + ": every radius must be finite and > 0 with a finite square");
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

int edt_hip_thickness_step_device(const float *d_S, const float *d_B, double radius, double next_radius, float *d_T, uint8_t *d_mask,
                                  int64_t *d_size, uint32_t *d_smax_bits, int64_t count, void *stream) {
  if (count < 0) { set_error("thickness_step: bad count"); return EDT_ERR_BAD_ARG; }
  double r2 = 0.0, next2 = 0.0;
  if (d_B) if (const int rc = thickness_radius_squared(radius, "thickness_step", &r2)) return rc;
  const bool has_next = !(next_radius < 0.0);  // (a NaN is a next radius, and a bad one)
  if (has_next) if (const int rc = thickness_radius_squared(next_radius, "thickness_step", &next2)) return rc;
  if (has_next != (d_mask != nullptr)) { set_error("thickness_step: d_mask goes with a next radius, and a next radius with d_mask"); return EDT_ERR_BAD_ARG; }
  if ((d_size && !d_B) || (d_smax_bits && d_B)) { set_error("thickness_step: d_size belongs to a step with d_B, d_smax_bits to the step without"); return EDT_ERR_BAD_ARG; }
  if (!d_S || !d_T) { set_error("thickness_step: null device pointer"); return EDT_ERR_BAD_ARG; }
  if (count == 0) return EDT_OK;
  if (const int rc = require_device()) return rc;
  return launch_thickness_step(d_S, d_B, r2, (float)radius, next2, d_T, d_mask, d_size, d_smax_bits, count, (hipStream_t)stream);
}

}  // extern "C"
