// Host shim over csrc/edt_moments_math.h for tests/test_moments_cpu.py: the closed form of a run's moments, the hand-rounded
// 128-bit conversion and what the finish derives from a label's sums, compiled with the host compiler.
#include "edt_moments_math.h"

extern "C" {

void moments_run(uint64_t x0, uint64_t n, uint64_t y, uint64_t z, uint64_t *out) { edt_amd::run_moments(x0, n, y, z, out); }

double moments_u128_to_double(uint64_t hi, uint64_t lo) {
  return edt_amd::u128_to_double(((unsigned __int128)hi << 64) | lo);
}

void moments_derive(const uint64_t *sums, double *centroid, double *central) { edt_amd::moments_derive(sums, centroid, central); }

int moments_in_range(int64_t sx, int64_t sy, int64_t sz) { return edt_amd::moments_in_range(sx, sy, sz) ? 1 : 0; }

}  // extern "C"
