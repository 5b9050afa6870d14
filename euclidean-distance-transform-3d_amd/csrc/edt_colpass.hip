// edt_colpass.hip -- the one driver of a column pass (Y or Z) on the in-place kernels: does the 16-bit integer kernel
// (edt_colq16.hip) take the pass?  If so it runs over all tiles, and the fp32 kernel over the list of tiles it refused --
// unless the host can prove that list empty.  Every entry point's column passes go through run_column_pass.
#include "edt_common.h"
#include "edt_kernels.h"

namespace edt_amd {

// In-place LDS-tiled column pass: the wave-autonomous kernel where the axis fits its register
// budget, the workgroup-phased kernel for longer axes.  (debug bit 64 forces the latter.)
bool column_inplace_supported(const AxisGeom &g) {
  return column_pass_wave_supported(g) || column_pass_tiled_supported(g);
}
int launch_column_inplace(const ColumnPass &cp, const TileList &list) {
  const AxisGeom &g = cp.g;
  // (a list -- the tiles the 16-bit integer kernel refused -- only exists for axes of the wave kernel)
  if (list.count != nullptr) return launch_column_pass_wave(cp, list);
  // axes of at most 32 rows with many columns: a thread per column (edt_short.hip); the LDS-tiled kernels would
  // launch a single-wave workgroup per 32 columns.  (debug bit 0x1000000 keeps them on the wave kernel.)
  if (column_pass_short_supported(g) && g.sx * g.nouter >= 4096 && !(debug_mode() & (kDbgTiledColumns | kDbgShortOnWave)))
    return launch_column_pass_short(cp.F, cp.nz, cp.rs, g, cp.w, cp.bb, cp.epi, cp.stream);
  if (column_pass_wave_supported(g) && !(debug_mode() & kDbgTiledColumns)) return launch_column_pass_wave(cp, list);
  return launch_column_pass_tiled(cp.F, cp.nz, cp.rs, g, cp.w, cp.bb, cp.epi, cp.stream);
}

namespace {
__global__ void k_fill_words(uint32_t *__restrict__ p, uint32_t value, size_t count) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < count) p[i] = value;
}
}  // namespace

int launch_fill_words(void *p, uint32_t value, size_t count, hipStream_t stream) {
  if (count == 0) return EDT_OK;
  hipLaunchKernelGGL(k_fill_words, dim3((unsigned)ceil_div((int64_t)count, 256)), dim3(256), 0, stream, static_cast<uint32_t *>(p), value,
                     count);
  EDT_HIP_TRY(hipGetLastError());
  return EDT_OK;
}

int HandOver::zero(hipStream_t stream) {
  const int rc = launch_fill_words(counts, 0u, (size_t)slots, stream);
  if (rc != EDT_OK) return rc;
  zeroed = true;
  return EDT_OK;
}

// the shape and mode part of the decision (buffers: column_pass_q16_aligned)
bool column_pass_q16_applies(const Quantum &Q, const AxisGeom &g, const HandOver &h) {
  // (the bits that force one form of the fp32 kernel on every tile -- the test tiers' way to cover them -- keep the call there)
  if (!Q.ok || h.counts == nullptr || h.slot >= h.slots || (debug_mode() & kDbgQ16Off)) return false;
  if (!column_pass_q16_supported(g) || !column_pass_wave_supported(g)) return false;
  // (the id array was sized for these tile counts; a hand-over without one only counts the refused tiles)
  return h.ids == nullptr || HandOver::ids_of(g.sx, g.nouter) <= h.capacity;
}

int run_column_pass(const ColumnPass &cp, const Quantum &Q, int axis, HandOver &h, Fp32Leg leg, bool sure, TileList *served) {
  TileList list;
  if (column_pass_q16_applies(Q, cp.g, h) && column_pass_q16_aligned(cp.F, cp.codes, cp.plane, cp.out.compact)) {
    // Where the integer kernel provably refuses no tile (index form, bounded values: q16_no_refusals, edt_colq16.hip) and
    // everything the pass reads was written by pass X or by an integer pass that could not refuse either (`sure`: the caller
    // vouches for that), the fp32 launch over the hand-over list has nothing to do and is not made -- nor is the list's
    // counter zeroed.  (the volume's sy: the scan axis of pass Y, the outer axis of pass Z)
    sure = sure && q16_no_refusals(Q, axis, cp.g.sx, axis == 1 ? cp.g.n : cp.g.nouter, cp.g.n, cp.bb);
    int rc = (sure || h.zeroed) ? EDT_OK : h.zero(cp.stream);
    if (rc == EDT_OK) rc = launch_column_pass_q16(cp, Q, axis, h);
    if (rc != EDT_OK) return rc;
    list.count = h.counts + h.slot++;
    list.ids = h.ids;
    list.none = sure;
  }
  if (served) *served = list;
  if (h.ids == nullptr) {  // (nothing is handed over: the caller reads the counter)
    if (list.count == nullptr) { set_error("internal: a pass that only counts refused tiles left the integer kernel"); return EDT_ERR_HIP; }
    return EDT_OK;
  }
  if (list.none) return EDT_OK;
  return leg == Fp32Leg::inplace ? launch_column_inplace(cp, list) : launch_column_pass_wave(cp, list);
}

}  // namespace edt_amd
