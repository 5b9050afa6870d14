// edt_colwave_cw8.hip -- the column-pass kernels of the wave shape CW = 8 (8 bands per column) in their
// own translation unit / device code object (see edt_colwave_kernel.h).
#include "edt_colwave_kernel.h"

namespace edt_amd {
template int launch_wave_c<8>(const ColumnPass &, const TileList &);
}  // namespace edt_amd
