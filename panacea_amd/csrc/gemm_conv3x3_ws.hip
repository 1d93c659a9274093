// gemm_conv3x3_ws.hip — PNC_A_CONV3X3 instantiations of the GEMM kernel template WITH the weight part (pnc_gemm_wsplit_f16); the
// variants of dispatch_conv3x3 (gemm_conv3x3.hip).  The halo-tile kernel has its own form of the part (gemm_stencil_tile.hip).
#include "gemm_kernel.h"

namespace pnc_gemm {

int dispatch_conv3x3_tiles_ws(const PncGemmParams& p, unsigned epi, int geometry, hipStream_t st, const void* wlo16);

int dispatch_conv3x3_ws(const PncGemmParams& p, unsigned epi, hipStream_t st, const void* wlo16) {
    constexpr int AM = PNC_A_CONV3X3;
    if (const int geometry = conv3x3_tile_geometry(p, epi)) return dispatch_conv3x3_tiles_ws(p, epi, geometry, st, wlo16);
    const TileChoice tc = choose_tile(p);
    if (tc.tile == T_128x32 && epi != E_O16 && epi != E_O32) epi = E_GENERIC;
    switch (epi) {
        case E_O16: return launch_tile<AM, E_O16, true>(p, st, tc, wlo16);
        case E_O32: return launch_tile<AM, E_O32, true>(p, st, tc, wlo16);
        case E_O32 | E_O16: return launch_tile<AM, E_O32 | E_O16, true>(p, st, tc, wlo16);
        case E_R1 | E_O32: return launch_tile<AM, E_R1 | E_O32, true>(p, st, tc, wlo16);
        case E_R1 | E_O32 | E_O16: return launch_tile<AM, E_R1 | E_O32 | E_O16, true>(p, st, tc, wlo16);
        default: return launch_tile<AM, E_GENERIC, true>(p, st, tc, wlo16);
    }
}

}  // namespace pnc_gemm

PNC_DEFINE_TU_COLLECT(gemm_conv3x3_ws)
