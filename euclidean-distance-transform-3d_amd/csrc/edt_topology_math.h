// edt_topology_math.h -- the arithmetic of label_topology (include/edt_hip.h, "label_topology") that needs no device: what ONE
// voxel adds to its label's sixteen cell counts, from the equality of its 26 neighbours alone.  Host and device code alike (the
// CPU test tier compiles it with the host compiler: tests/topology_shim.cpp).
//
// NEIGHBOURHOOD WORD: bit topo_bit(ex, ey, ez) = (ey + 1) + 3 * (ez + 1) + 9 * (ex + 1) of `eq` says that the voxel at offset
// (ex, ey, ez) lies inside the volume and carries the centre's label.  x is the SLOWEST digit: the sweep gets the nine bits of
// one ex from one lane exchange and places them with one shift.  Bit 13, the centre itself, is ignored.
// TYPE of a cell c in {-1, 0, +1}^3: bit a is set where c_a = 0, the axes the cell extends along (bit 0 = x, 1 = y, 2 = z).
// OWNERSHIP: the total order is the memory order idx = x + sx * (y + sy * z).  For the closed complex a voxel owns a cell when
// no incident voxel BEFORE it carries its label; for the interior it owns the cells with c >= 0 whose incident voxels all do.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define EDT_TP_HD __host__ __device__ inline
#else
#define EDT_TP_HD inline
#endif

namespace edt_amd {

enum { kTpTypes = 8, kTpSums = 16 };   // a label's sums: closed[0..7], then interior[0..7]; closed[7] = interior[7] = the voxels
constexpr uint32_t kTpFull = 0x7FFFFFFu & ~(1u << 13);   // all 26 neighbours carry the label

constexpr int topo_bit(int ex, int ey, int ez) { return (ey + 1) + 3 * (ez + 1) + 9 * (ex + 1); }

// the incident voxels of cell (cx, cy, cz) other than the centre: every one (before = false) or those before the centre
constexpr uint32_t topo_incident(int cx, int cy, int cz, bool before) {
  uint32_t m = 0;
  for (int ez = (cz < 0 ? cz : 0); ez <= (cz > 0 ? cz : 0); ++ez)
    for (int ey = (cy < 0 ? cy : 0); ey <= (cy > 0 ? cy : 0); ++ey)
      for (int ex = (cx < 0 ? cx : 0); ex <= (cx > 0 ? cx : 0); ++ex) {
        if (ex == 0 && ey == 0 && ez == 0) continue;
        const bool first = ez != 0 ? ez < 0 : ey != 0 ? ey < 0 : ex < 0;   // (z, y, x): the memory order
        if (!before || first) m |= 1u << topo_bit(ex, ey, ez);
      }
  return m;
}

// cell i = (cx + 1) + 3 * (cy + 1) + 9 * (cz + 1): its type and its two masks, worked out by the compiler
struct TopoCells {
  uint32_t before[27] = {}, all[27] = {};
  int type[27] = {};
  bool forward[27] = {};   // c >= 0: a candidate for the interior
  constexpr TopoCells() {
    for (int i = 0; i < 27; ++i) {
      const int cx = i % 3 - 1, cy = i / 3 % 3 - 1, cz = i / 9 - 1;
      type[i] = (cx == 0 ? 1 : 0) | (cy == 0 ? 2 : 0) | (cz == 0 ? 4 : 0);
      before[i] = topo_incident(cx, cy, cz, true);
      all[i] = topo_incident(cx, cy, cz, false);
      forward[i] = cx >= 0 && cy >= 0 && cz >= 0;
    }
  }
};

// closed[t] and interior[t] += the cells of type t that this voxel owns.  Counters of any unsigned width.
template <typename C>
EDT_TP_HD void topo_voxel(uint32_t eq, C closed[kTpTypes], C interior[kTpTypes]) {
  constexpr TopoCells cells;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 27; ++i) {
    closed[cells.type[i]] += (C)((eq & cells.before[i]) == 0);
    if (cells.forward[i]) interior[cells.type[i]] += (C)((eq & cells.all[i]) == cells.all[i]);
  }
}

// a voxel whose whole neighbourhood carries its label owns exactly one cell of each type in both tables
EDT_TP_HD bool topo_solid(uint32_t eq) { return (eq & kTpFull) == kTpFull; }

}  // namespace edt_amd
