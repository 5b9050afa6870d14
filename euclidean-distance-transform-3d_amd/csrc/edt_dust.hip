// edt_dust.hip -- dust: connected components are kept or removed by their voxel count (include/edt_hip.h, "dust", states the
// contract).
//
// The components come from the union-find of edt_components.hip, run over the labels themselves (launch_forest:
// k_cc_rows / k_cc_merge / k_cc_flatten, no numbering).  After it every foreground voxel i holds its component's root in P[i] --
// the component's smallest idx -- a root holds itself, and background holds kCcBg.
//
// Room for the size of a component: its root's own word, as fill_holes keeps a cavity's state there.  A root's word ends as
// kCcTag | size  (size <= voxels <= 2^31 - 1 fits below the tag).  It gets there by unsigned 32-bit atomic adds alone: the word
// starts as the self-pointer r; every stretch of the component adds its length, and the one stretch that begins at voxel r -- r is
// the component's smallest idx, so r - 1 is never of r's component and r always begins a stretch -- adds  kCcTag - r  on top.  The
// sum is the same in every order: r + (kCcTag - r) + size.  While the adds are in flight the word of root r is r + (part of the
// size) with or without the tag, in any case >= r and below 2^32; every other foreground word is a root's idx < i and never
// changes.  So the count kernel tells a root by P[i] >= i (the root rule of edt_forest.h), whatever has been added already, and
// reads nothing but P[i] itself.
//
//   rows, merge, flatten   the forest of the labels in P                                      (edt_components.hip)
//   k_dust_count   a wave walks EDT_HIP_DUST_COUNT_SPAN consecutive voxels, 64 at a time.  A stretch is a maximal range of
//                  consecutive idx with one root; its first voxel (a neighbour compare and a ballot, as k_cc_rows finds run
//                  starts) knows the stretch's length from the next set bit of the ballot.  A stretch that crosses a 64-voxel
//                  group stays open in the wave (its root and first idx are wave-uniform) until a later group closes it, at the
//                  latest the end of the span.  The lengths do not go to memory one by one: the wave keeps the sums of up to
//                  four roots to itself (dust_combine: lanes with one root are summed by shuffles) and sends each with ONE
//                  atomic when the span ends or another root needs the slot.  So a component costs a wave one add however it
//                  is cut up -- one solid label over 512^3, or a checkerboard joined through its corners, sends 2^27 / span =
//                  16 384 adds to its root's word, not 2^27 or 2^26 -- and a lane sends an atomic of its own only where a group
//                  holds stretches of more than six different roots, which then are different words.
//   k_dust_filter<T>  out[i] = labels[i] for background and for a voxel whose root's size passes the test, else all-zero bits; thread i
//                  reads labels[i] and writes out[i] and no other voxel, which is why the output may BE the labels.  Roots found,
//                  roots kept and voxels removed are reduced over the workgroup and added to d_counts with at most three 64-bit
//                  atomics per workgroup.
// Phases are separate launches; no thread waits for another, every loop is bounded by its inputs, and every reduction is an
// integer add, so the result does not depend on which thread won an atomic.
#include "edt_forest.h"

namespace edt_amd {
namespace {

constexpr int kDustThreads = 256;
constexpr int kDustBlocks = 256 * 8;                    // grid of the striding sweep
constexpr int kDustSpan = EDT_HIP_DUST_COUNT_SPAN;      // voxels per wave of k_dust_count
constexpr int kDustBatch = 4;                           // 64-voxel groups loaded together
constexpr int kDustSlots = 4;                           // roots whose adds a wave of k_dust_count keeps to itself
constexpr int kDustAdopt = 2;                           // slots a 64-voxel group may take over
constexpr uint32_t kDustNone = 0xFFFFFFFEu;             // "no voxel before this one": neither a root (< 2^31) nor kCcBg
static_assert(kDustSpan % (64 * kDustBatch) == 0, "a span is whole batches of groups");

// what the stretch [first, first + len) of root r adds to the root's word
__device__ __forceinline__ uint32_t dust_amount(uint32_t r, uint32_t first, uint32_t len) {
  return r == first ? len + (kCcTag - r) : len;
}

// The adds a wave has not sent yet: kDustSlots roots (wave-uniform) and what their stretches came to so far.
struct DustSlots {
  uint32_t root[kDustSlots], sum[kDustSlots];
};

// The lanes with `pending` each have `amount` to add to the word of root r.  Lanes whose root sits in a slot add there; then
// up to kDustAdopt times the root of the first lane left takes over the slot with the smallest sum, whose own sum is sent
// (one atomic: an empty slot has sum 0 and goes first); whoever is left after that sends its own atomic.  Call with the
// whole wave converged.
__device__ __forceinline__ void dust_combine(uint32_t *P, DustSlots &s, bool pending, uint32_t r, uint32_t amount) {
  if (__ballot(pending) == 0) return;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < kDustSlots; ++k) {
    const bool match = pending && r == s.root[k];  // (an empty slot holds kDustNone, which is nobody's root)
    if (__ballot(match)) {
      s.sum[k] += (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_sum(match ? amount : 0u));
      pending = pending && !match;
    }
  }
  uint64_t left = __ballot(pending);
  for (int j = 0; j < kDustAdopt && left; ++j) {
    const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(r, __ffsll((unsigned long long)left) - 1));
    const bool match = pending && r == c;
    const uint32_t sum = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_sum(match ? amount : 0u));
    int victim = 0;
    uint32_t least = s.sum[0];
#pragma unroll
    for (int k = 1; k < kDustSlots; ++k)
      if (s.sum[k] < least) {
        least = s.sum[k];
        victim = k;
      }
#pragma unroll
    for (int k = 0; k < kDustSlots; ++k)
      if (k == victim) {
        if (lane == 0 && s.sum[k] != 0) atomicAdd(&P[s.root[k]], s.sum[k]);
        s.root[k] = c;
        s.sum[k] = sum;
      }
    pending = pending && !match;
    left = __ballot(pending);
  }
  if (pending) atomicAdd(&P[r], amount);
}

// ---- sizes ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDustThreads) void k_dust_count(uint32_t *P, uint32_t voxels) {
  const int lane = threadIdx.x & 63;
  const uint64_t span = ((uint64_t)blockIdx.x * (kDustThreads / 64) + (threadIdx.x >> 6)) * (uint64_t)kDustSpan;
  if (span >= voxels) return;  // (wave-uniform)
  const uint32_t base0 = (uint32_t)span;
  DustSlots slots;
#pragma unroll
  for (int k = 0; k < kDustSlots; ++k) {
    slots.root[k] = kDustNone;
    slots.sum[k] = 0;
  }
  uint32_t open_root = kDustNone, open_first = 0;  // the stretch that reaches the end of the groups seen so far (wave-uniform)
  for (int b = 0; b < kDustSpan / 64; b += kDustBatch) {
    const uint32_t bbase = base0 + (uint32_t)b * 64u;  // (< 2^31 + span: no wrap)
    if (bbase >= voxels) break;
    uint32_t root[kDustBatch];
#pragma unroll
    for (int j = 0; j < kDustBatch; ++j) {
      const uint32_t i = bbase + j * 64 + lane;
      uint32_t r = kCcBg;  // (past the end: background)
      if (i < voxels) {
        const uint32_t p = parent_peek(&P[i]);
        r = p == kCcBg ? kCcBg : (is_root(i, p) ? i : p);  // a root's word: itself plus what has been added so far
      }
      root[j] = r;
    }
#pragma unroll
    for (int j = 0; j < kDustBatch; ++j) {
      const uint32_t gbase = bbase + j * 64;
      const uint32_t r = root[j];
      uint32_t prev = __shfl_up(r, 1);
      if (lane == 0) prev = open_root;
      const uint64_t m = __ballot(r != prev);  // the heads of this group
      if (m == 0) continue;                    // the open stretch goes on
      const int first = __ffsll((unsigned long long)m) - 1, last = 63 - __builtin_clzll(m);
      if (open_root < kCcTag)                  // (a root: neither kDustNone nor background) the open stretch ends at `first`
        dust_combine(P, slots, lane == first, open_root, dust_amount(open_root, open_first, gbase + first - open_first));
      // every head but the last: its stretch ends at the next head
      const uint64_t above = m & ~((2ull << lane) - 1ull);  // (lane 63: 2 << 63 wraps to 0, the mask is all ones, above = 0)
      const uint32_t len = above ? (uint32_t)(__ffsll((unsigned long long)above) - 1 - lane) : 0u;
      dust_combine(P, slots, ((m >> lane) & 1) && above && r != kCcBg, r, dust_amount(r, gbase + lane, len));
      open_root = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(r, last));
      open_first = gbase + last;
    }
  }
  if (open_root < kCcTag) {
    const uint64_t end = span + kDustSpan;
    dust_combine(P, slots, lane == 0, open_root,
                 dust_amount(open_root, open_first, (uint32_t)(end < voxels ? end : voxels) - open_first));
  }
#pragma unroll
  for (int k = 0; k < kDustSlots; ++k)
    if (lane == k && slots.sum[k] != 0) atomicAdd(&P[slots.root[k]], slots.sum[k]);
}

// ---- the filter -----------------------------------------------------------------------------------------------------------
// (labels and out may be one array: no __restrict__)
template <typename T>
__global__ __launch_bounds__(kDustThreads) void k_dust_filter(const T *labels, const uint32_t *__restrict__ P, T *out, uint32_t voxels,
                                                              int64_t min_voxels, int64_t max_voxels, int invert,
                                                              unsigned long long *counts) {
  __shared__ unsigned long long s_count[kDustThreads / 64][3];
  const uint32_t stride = gridDim.x * kDustThreads;
  uint32_t found = 0, kept = 0, removed = 0;  // (a thread sees fewer than 2^31 voxels)
  for (uint32_t i = blockIdx.x * kDustThreads + threadIdx.x; i < voxels; i += stride) {  // (voxels + stride < 2^32)
    T v = labels[i];
    if (label_fg(v)) {
      const uint32_t p = P[i];
      // (a foreground word is a root's idx < 2^31, or a root's tagged size: here the tag says what the root rule of edt_forest.h
      // says, and the kernel keeps the test it was compiled with)
      const bool tagged = (p & kCcTag) != 0;
      const int64_t size = (int64_t)((tagged ? p : P[p]) & ~kCcTag);
      const bool keep = (size >= min_voxels && size < max_voxels) != (invert != 0);
      found += tagged;
      kept += tagged && keep;
      if (!keep) {
        ++removed;
        __builtin_memset(&v, 0, sizeof(T));
      }
    }
    out[i] = v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {  // (three sums in step, not wave_sum: the kernel's code would change)
    found += __shfl_xor(found, off);
    kept += __shfl_xor(kept, off);
    removed += __shfl_xor(removed, off);
  }
  if ((threadIdx.x & 63) == 0) {
    s_count[threadIdx.x >> 6][0] = found;
    s_count[threadIdx.x >> 6][1] = kept;
    s_count[threadIdx.x >> 6][2] = removed;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long c = 0;
    for (int w = 0; w < kDustThreads / 64; ++w) c += s_count[w][threadIdx.x];
    if (c) atomicAdd(&counts[threadIdx.x], c);
  }
}

int launch_dust(int dtype, const void *labels, int64_t sx, int64_t sy, int64_t sz, int connectivity, int binary, int64_t min_voxels,
                int64_t max_voxels, int invert, void *out, int64_t *counts, void *ws, hipStream_t stream) {
  const int64_t voxels = sx * sy * sz;
  const ForestWorkspace w(ws, voxels);
  uint32_t *P = w.P;
  int rc;
  if ((rc = launch_forest(dtype, labels, sx, sy, sz, connectivity, binary, P, w.chunks, "dust", stream)) != EDT_OK) return rc;
  {
    ScopedPass sp("dust count", stream);
    if ((rc = launch_fill_words(counts, 0u, 3 * sizeof(int64_t) / sizeof(uint32_t), stream)) != EDT_OK) return rc;
    const int64_t spans = ceil_div(voxels, kDustSpan);
    hipLaunchKernelGGL(k_dust_count, dim3((unsigned)ceil_div(spans, kDustThreads / 64)), dim3(kDustThreads), 0, stream, P,
                       (uint32_t)voxels);
    EDT_HIP_TRY(hipGetLastError());
  }
  return with_label_type(dtype, [&](auto t) -> int {
    using T = typename decltype(t)::type;
    ScopedPass sp("dust filter", stream);
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(voxels, kDustThreads), kDustBlocks * 4);
    hipLaunchKernelGGL(k_dust_filter<T>, dim3(blocks), dim3(kDustThreads), 0, stream, (const T *)labels, P, (T *)out,
                       (uint32_t)voxels, min_voxels, max_voxels, invert, (unsigned long long *)counts);
    EDT_HIP_TRY(hipGetLastError());
    return EDT_OK;
  });
}

}  // namespace

// shape, connectivity and the size limit as connected_components, then the call's own two
int dust_check_args(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity, int64_t min_voxels,
                    int64_t max_voxels) {
  const int rc = components_check_args(dtype, ndim, sx, sy, sz, connectivity, "dust");
  if (rc != EDT_OK) return rc;
  if (min_voxels < 0) { set_error("dust: min_voxels must be >= 0"); return EDT_ERR_BAD_ARG; }
  if (max_voxels < min_voxels) { set_error("dust: max_voxels must be >= min_voxels"); return EDT_ERR_BAD_ARG; }
  return EDT_OK;
}

}  // namespace edt_amd

using namespace edt_amd;

extern "C" {

size_t edt_hip_dust_workspace_bytes(int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz) {
  const size_t chunks = edt_hip_components_workspace_bytes(dtype, ndim, sx, sy, sz);  // (0: a bad dtype or shape, or past the limit)
  return chunks == 0 ? 0 : ForestWorkspace::bytes(sx * sy * sz);
}

int edt_hip_dust_device(const void *d_labels, int dtype, int ndim, int64_t sx, int64_t sy, int64_t sz, int connectivity, int binary,
                        int64_t min_voxels, int64_t max_voxels, int invert, void *d_out, int64_t *d_counts, void *d_workspace,
                        size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int own = dust_check_args(dtype, ndim, sx, sy, sz, connectivity, min_voxels, max_voxels);
  const int64_t voxels = own == EDT_OK ? sx * sy * sz : 0;
  int rc;
  if (!label_op_begin("dust", own, d_counts, 3, voxels, !d_labels || !d_out, false, d_workspace, workspace_bytes,
                      ForestWorkspace::bytes(voxels), "edt_hip_dust_workspace_bytes", stream, &rc))
    return rc;
  return launch_dust(dtype, d_labels, sx, sy, sz, connectivity, binary, min_voxels, max_voxels, invert, d_out, d_counts,
                     d_workspace, stream);
}

}  // extern "C"
