// gemm_plain_ws.hip — PNC_A_PLAIN instantiations of the GEMM kernel template WITH the weight part (pnc_gemm_wsplit_f16: the fp16 lo
// plane of the weights beside the parameter block, gemm_kernel.h: gemm_glds_ws_kernel).  The tile choice and the epilogue
// variants are dispatch_plain's (gemm_plain.hip), so a launch and its twin without the plane run the same tiles in the same K
// order.  The persistent GEGLU kernel has the part too (PNC_OPT_GEMM_PERSIST bit 0); the persistent plain-A kernel has none: its
// launches run gemm_glds_ws_kernel on the tile it would have used.
#include "gemm_kernel.h"

namespace pnc_gemm {

template <unsigned EPI>
static int launch_ln_ws(const PncGemmParams& p, hipStream_t st, TileChoice tc, const void* wlo16) {
    if (tc.tile == T_256x320) return launch<PNC_A_PLAIN, 256, 320, 4, 2, 2, false, EPI, true>(p, st, 1, wlo16);
    return launch<PNC_A_PLAIN, 128, 128, 2, 2, 2, true, EPI, true>(p, st, 1, wlo16);
}

int dispatch_plain_ws(const PncGemmParams& p, unsigned epi, hipStream_t st, bool* ln_fused, const void* wlo16) {
    constexpr int AM = PNC_A_PLAIN;
    const TileChoice tc = choose_tile(p);
    if (epi & E_LN) {
        if (ln_whole_rows(p, tc)) *ln_fused = true;
        else epi &= ~E_LN;                      // the caller runs the LayerNorm kernel after this GEMM instead
    }
    if (tc.tile == T_128x32 && epi != E_O16 && epi != E_O32) epi = E_GENERIC;
    switch (epi) {
        case E_O16: return launch_tile<AM, E_O16, true>(p, st, tc, wlo16);
        case E_O16 | E_VT: return launch_tile<AM, E_O16 | E_VT, true>(p, st, tc, wlo16);
        case E_O32: return launch_tile<AM, E_O32, true>(p, st, tc, wlo16);
        case E_O32 | E_O16: return launch_tile<AM, E_O32 | E_O16, true>(p, st, tc, wlo16);
        case E_R1 | E_O32: return launch_tile<AM, E_R1 | E_O32, true>(p, st, tc, wlo16);
        case E_R1 | E_O32 | E_O16: return launch_tile<AM, E_R1 | E_O32 | E_O16, true>(p, st, tc, wlo16);
        case E_R1 | E_O16: return launch_tile<AM, E_R1 | E_O16, true>(p, st, tc, wlo16);
        case E_RB | E_O32: return launch_tile<AM, E_RB | E_O32, true>(p, st, tc, wlo16);
        case E_O32 | E_LN: return launch_ln_ws<E_O32 | E_LN>(p, st, tc, wlo16);
        case E_RB | E_O32 | E_LN: return launch_ln_ws<E_RB | E_O32 | E_LN>(p, st, tc, wlo16);
        case E_R1 | E_O32 | E_LN: return launch_ln_ws<E_R1 | E_O32 | E_LN>(p, st, tc, wlo16);
        case E_GEGLU | E_O16:                                                       // ff1: the persistent kernel has the part
            if (tc.tile == T_256x256 && geglu_persist_ok(p)) return launch_geglu_persist<256, 256, 4, 2, true>(p, st, wlo16);
            return launch_tile<AM, E_GEGLU | E_O16, true>(p, st, tc, wlo16);
        default: return launch_tile<AM, E_GENERIC, true>(p, st, tc, wlo16);         // (incl. the text tower's GELU variant)
    }
}

}  // namespace pnc_gemm

PNC_DEFINE_TU_COLLECT(gemm_plain_ws)
