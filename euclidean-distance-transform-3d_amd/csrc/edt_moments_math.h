// edt_moments_math.h -- the arithmetic of label_moments (include/edt_hip.h, "label_moments") that needs no device: the raw
// moments of one x-run in closed form, the range bound, and what the finish derives from a label's exact sums -- centroid and
// population covariance, each value rounded once from an exact integer.  Host and device code alike (the CPU test tier compiles
// it with the host compiler: tests/moments_shim.cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define EDT_MM_HD __host__ __device__ inline
#else
#define EDT_MM_HD inline
#endif

namespace edt_amd {

// the order of a label's ten sums: the count, then the nine of the ABI
enum { kMmN = 0, kMmX, kMmY, kMmZ, kMmXX, kMmYY, kMmZZ, kMmXY, kMmXZ, kMmYZ, kMmSums };

// The sums over the n voxels (x0 .. x0 + n - 1, y, z) of one run, 1 <= n.  u64 arithmetic that may wrap: every result is the
// exact sum modulo 2^64, and below the range bound the sums of a whole label fit int64, so adding partials modulo 2^64 ends
// exact.  The two divisions are of products of consecutive integers (exact); for them n must stay below 2^21 (n <= 256 here).
EDT_MM_HD void run_moments(uint64_t x0, uint64_t n, uint64_t y, uint64_t z, uint64_t out[kMmSums]) {
  const uint64_t t1 = n * (n - 1) / 2;                // 0 + 1 + ... + (n - 1)
  const uint64_t t2 = (n - 1) * n * (2 * n - 1) / 6;  // 0 + 1 + 4 + ... + (n - 1)^2
  const uint64_t sx = n * x0 + t1, sy = n * y, sz = n * z;
  out[kMmN] = n;
  out[kMmX] = sx;
  out[kMmY] = sy;
  out[kMmZ] = sz;
  out[kMmXX] = n * x0 * x0 + 2 * x0 * t1 + t2;
  out[kMmYY] = y * sy;
  out[kMmZZ] = z * sz;
  out[kMmXY] = y * sx;
  out[kMmXZ] = z * sx;
  out[kMmYZ] = y * sz;
}

// voxels * (E - 1)^2 < 2^63, E the largest extent: every sum then fits int64 (a second moment is at most voxels * (E - 1)^2)
// and every n * S_ab - S_a * S_b fits 128 bits.  Extents are below 2^31 and voxels below 2^63: the product is below 2^125.
EDT_MM_HD bool moments_in_range(int64_t sx, int64_t sy, int64_t sz) {
  const int64_t e = sx > sy ? (sx > sz ? sx : sz) : (sy > sz ? sy : sz);
  if (e <= 1) return true;
  const unsigned __int128 v = (unsigned __int128)(uint64_t)sx * (uint64_t)sy * (uint64_t)sz;
  return v * (uint64_t)(e - 1) * (uint64_t)(e - 1) < ((unsigned __int128)1 << 63);
}

// fl(v): the binary64 nearest to the integer v, ties to even.  By hand -- normalise to 53 bits, round on the remainder, set the
// exponent -- because a 128-bit conversion left to the compiler is a library call.  v < 2^128: no overflow, no subnormals.
EDT_MM_HD double u128_to_double(unsigned __int128 v) {
  if (v == 0) return 0.0;
  const uint64_t hi = (uint64_t)(v >> 64), lo = (uint64_t)v;
  int top = hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo);  // position of the leading one
  uint64_t mant;
  if (top <= 52) {
    mant = lo << (52 - top);
  } else {
    const int shift = top - 52;
    mant = (uint64_t)(v >> shift);
    const unsigned __int128 rem = v & (((unsigned __int128)1 << shift) - 1), half = (unsigned __int128)1 << (shift - 1);
    if (rem > half || (rem == half && (mant & 1))) ++mant;
    if (mant >> 53) {  // rounded up to the next power of two
      mant >>= 1;
      ++top;
    }
  }
  const uint64_t bits = ((uint64_t)(top + 1023) << 52) | (mant & ((1ull << 52) - 1));
  union { uint64_t u; double d; } c;
  c.u = bits;
  return c.d;
}

// centroid[a] = fl(fl(S_a) / fl(n));  central[ab] = fl(fl(fl(M_ab) / fl(n)) / fl(n)) with M_ab = n * S_ab - S_a * S_b taken
// exactly as a signed 128-bit integer (magnitude and sign apart): nothing subtracts two rounded numbers.  sums: the ten of a
// label, n >= 1.  central in the order xx, yy, zz, xy, xz, yz.
EDT_MM_HD void moments_derive(const uint64_t sums[kMmSums], double centroid[3], double central[6]) {
  const uint64_t n = sums[kMmN];
  const double fn = u128_to_double(n);
  for (int a = 0; a < 3; ++a) centroid[a] = u128_to_double(sums[kMmX + a]) / fn;
  const int ia[6] = {kMmX, kMmY, kMmZ, kMmX, kMmX, kMmY}, ib[6] = {kMmX, kMmY, kMmZ, kMmY, kMmZ, kMmZ};
  for (int k = 0; k < 6; ++k) {
    const unsigned __int128 p = (unsigned __int128)n * sums[kMmXX + k], q = (unsigned __int128)sums[ia[k]] * sums[ib[k]];
    const double m = p >= q ? u128_to_double(p - q) : -u128_to_double(q - p);
    central[k] = m / fn / fn;
  }
}

}  // namespace edt_amd
