// edt_colwave_cw32.hip -- the column-pass kernels of the wave shape CW = 32 (2 bands per column) in their
// own translation unit / device code object (see edt_colwave_kernel.h).
#include "edt_colwave_kernel.h"

namespace edt_amd {
template int launch_wave_c<32>(const ColumnPass &, const TileList &);
}  // namespace edt_amd
