// Host shim over csrc/edt_topology_math.h for tests/test_topology_cpu.py: what one voxel adds to its label's sixteen counts,
// from its neighbourhood word, compiled with the host compiler.
#include "edt_topology_math.h"

extern "C" {

// out[0..7] += closed, out[8..15] += interior
void topology_voxel(uint32_t eq, uint32_t *out) { edt_amd::topo_voxel(eq, out, out + edt_amd::kTpTypes); }

int topology_solid(uint32_t eq) { return edt_amd::topo_solid(eq) ? 1 : 0; }

int topology_bit(int ex, int ey, int ez) { return edt_amd::topo_bit(ex, ey, ez); }

}  // extern "C"
