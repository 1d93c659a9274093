// gemm_dispatch.h — the tile and epilogue-variant choice of the three A-gather modes, ONE template per mode for the launches
// with and without the weight part (WS; pnc_gemm_wsplit_f16: wlo16 = the fp16 lo plane of W beside the parameter block, NULL
// without).  A launch and its twin with the plane go through the same statements, so they run the same tiles in the same K
// order: on fp16-representable weights (a zero plane) the twin gives the bits of the launch without it.  Where the twin
// deliberately differs, an `if constexpr (!WS)` says so here.
//
// Each template is instantiated explicitly in two translation units — gemm_<mode>.hip (WS = false) and gemm_<mode>_ws.hip
// (WS = true) — which is where its kernels are compiled; gemm.hip sees the declarations only.
#pragma once
#include "gemm_kernel.h"

namespace pnc_gemm {

// E_LN variants exist for the two geometries whose workgroup can own a whole row of the path's widths
template <unsigned EPI, bool WS>
static int launch_ln(const PncGemmParams& p, hipStream_t st, TileChoice tc, const void* wlo16) {
    if (tc.tile == T_256x320) return launch<PNC_A_PLAIN, 256, 320, 4, 2, 2, false, EPI, WS>(p, st, 1, wlo16);
    return launch<PNC_A_PLAIN, 128, 128, 2, 2, 2, true, EPI, WS>(p, st, 1, wlo16);
}

// PNC_A_PLAIN (nn.Linear / 1x1 conv call-sites, include/panacea_hip.h §1): one instantiation per (tile geometry, epilogue variant)
// the denoising path uses; everything else runs E_GENERIC
template <bool WS>
int dispatch_plain(const PncGemmParams& p, unsigned epi, hipStream_t st, bool* ln_fused, const void* wlo16) {
    constexpr int AM = PNC_A_PLAIN;
    const TileChoice tc = choose_tile(p);
    if (epi & E_LN) {
        // fuse only when ONE column tile covers the row (level-0 width 320 on 256x320; <= 128 on 128x128)
        if (ln_whole_rows(p, tc)) *ln_fused = true;
        else epi &= ~E_LN;                      // the caller runs the LayerNorm kernel after this GEMM instead
    }
    if (tc.tile == T_128x32 && epi != E_O16 && epi != E_O32) epi = E_GENERIC;     // narrow-N: two fast variants
    if constexpr (!WS) {                        // gemm_persist_kernel has no weight part: the twin runs gemm_glds_ws_kernel on the same 256x320 tiles
        if (tc.tile == T_256x320 && tc.ksplit == 1 && plain_persist_ok(p, epi)) {
            // level-0 launches of the fp32-epilogue families: one persistent workgroup per CU, next tile's first K tile under the epilogue
            switch (epi) {
                case E_O16: return launch_plain_persist<E_O16>(p, st);
                case E_O16 | E_VT: return launch_plain_persist<E_O16 | E_VT>(p, st);
                case E_O32: return launch_plain_persist<E_O32>(p, st);
                case E_R1 | E_O32: return launch_plain_persist<E_R1 | E_O32>(p, st);
                case E_R1 | E_O16: return launch_plain_persist<E_R1 | E_O16>(p, st);
                case E_O32 | E_LN: return launch_plain_persist<E_O32 | E_LN>(p, st);
                case E_RB | E_O32 | E_LN: return launch_plain_persist<E_RB | E_O32 | E_LN>(p, st);
                case E_R1 | E_O32 | E_LN: return launch_plain_persist<E_R1 | E_O32 | E_LN>(p, st);
                default: break;
            }
        }
    }
    if (epi == (E_O16 | E_GELU)) {
        bool variant = false;
        if constexpr (!WS) variant = tc.tile == T_256x256 || tc.tile == T_128x128;   // the text tower's weights are not split: no twin of the erff variant
        if (!variant) epi = E_GENERIC;
    }
    switch (epi) {
        case E_O16: return launch_tile<AM, E_O16, WS>(p, st, tc, wlo16);                       // q (text), qkv (temporal), text K
        case E_O16 | E_VT: return launch_tile<AM, E_O16 | E_VT, WS>(p, st, tc, wlo16);         // qkv of the view attention, text V^T
        case E_O32: return launch_tile<AM, E_O32, WS>(p, st, tc, wlo16);                       // proj_in, skip 1x1, zero convs
        case E_O32 | E_O16: return launch_tile<AM, E_O32 | E_O16, WS>(p, st, tc, wlo16);
        case E_R1 | E_O32: return launch_tile<AM, E_R1 | E_O32, WS>(p, st, tc, wlo16);         // to_out, ff2, proj_out (+ residual, in place)
        case E_R1 | E_O32 | E_O16: return launch_tile<AM, E_R1 | E_O32 | E_O16, WS>(p, st, tc, wlo16);
        case E_R1 | E_O16: return launch_tile<AM, E_R1 | E_O16, WS>(p, st, tc, wlo16);         // ff2 of the last block: fp16 for proj_out
        case E_RB | E_O32: return launch_tile<AM, E_RB | E_O32, WS>(p, st, tc, wlo16);         // proj_in_temporal + position table
        case E_O32 | E_LN: return launch_ln<E_O32 | E_LN, WS>(p, st, tc, wlo16);               // proj_in + norm1
        case E_RB | E_O32 | E_LN: return launch_ln<E_RB | E_O32 | E_LN, WS>(p, st, tc, wlo16); // proj_in_temporal + pos + norm1
        case E_R1 | E_O32 | E_LN: return launch_ln<E_R1 | E_O32 | E_LN, WS>(p, st, tc, wlo16); // to_out + residual + norm2 / norm3
        case E_GEGLU | E_O16:                                                                  // ff1 (the persistent kernel has the part too)
            if (tc.tile == T_256x256 && geglu_persist_ok(p)) return launch_geglu_persist<256, 256, 4, 2, WS>(p, st, wlo16);
            return launch_tile<AM, E_GEGLU | E_O16, WS>(p, st, tc, wlo16);
        case E_O16 | E_GELU:                                                                   // text-tower c_fc + GELU (two geometries)
            if constexpr (!WS) {
                if (tc.tile == T_256x256) return launch<AM, 256, 256, 4, 2, 2, true, E_O16 | E_GELU>(p, st);
                return launch<AM, 128, 128, 2, 2, 2, true, E_O16 | E_GELU>(p, st);
            }
            break;                                                                             // (WS: sent to E_GENERIC above)
        default: break;
    }
    return launch_tile<AM, E_GENERIC, WS>(p, st, tc, wlo16);
}

// PNC_A_CONV3X3 (nn.Conv2d 3x3 call-sites incl. stride-2 / nearest-x2 gathers, include/panacea_hip.h §1).  The halo-tile kernel
// has its own form of the weight part (gemm_stencil_tile.hip)
template <bool WS>
int dispatch_conv3x3(const PncGemmParams& p, unsigned epi, hipStream_t st, const void* wlo16) {
    constexpr int AM = PNC_A_CONV3X3;
    if (const int geometry = conv3x3_tile_geometry(p, epi)) return dispatch_conv3x3_tiles<WS>(p, epi, geometry, st, wlo16);
    const TileChoice tc = choose_tile(p);
    if (tc.tile == T_128x32 && epi != E_O16 && epi != E_O32) epi = E_GENERIC;
    switch (epi) {
        case E_O16: return launch_tile<AM, E_O16, WS>(p, st, tc, wlo16);                       // hint stem (SiLU, fp16 between layers)
        case E_O32: return launch_tile<AM, E_O32, WS>(p, st, tc, wlo16);                       // ResBlock3D in/out layers
        case E_O32 | E_O16: return launch_tile<AM, E_O32 | E_O16, WS>(p, st, tc, wlo16);       // Down/Upsample feeding a conv
        case E_R1 | E_O32: return launch_tile<AM, E_R1 | E_O32, WS>(p, st, tc, wlo16);         // first-stage ResnetBlock conv2 + skip
        case E_R1 | E_O32 | E_O16: return launch_tile<AM, E_R1 | E_O32 | E_O16, WS>(p, st, tc, wlo16);
        default: return launch_tile<AM, E_GENERIC, WS>(p, st, tc, wlo16);                      // 4 / 3-channel output heads
    }
}

// PncGemmParams.gn_part out of the epilogue: the 256x320 tile's waves (64 rows x 160 columns) own whole groups of N/32 = 10, 20
// or 40 channels, their 64 rows are pixels of one frame, every row and column of a tile exists
static inline bool gn_stats_in_epilogue(const PncGemmParams& p, const TileChoice& tc) {
    const int cpg = p.N / 32;
    return tc.tile == T_256x320 && (p.N % 320) == 0 && (160 % cpg) == 0 && (cpg % 2) == 0 && (p.Npix % 64) == 0 && (p.M % 64) == 0 &&
           pnc_get_option(PNC_OPT_GEMM_GN_STATS) != 0;
}

// PNC_A_CONV1D_T (temporal nn.Conv1d k=3 of ResBlock3D, openaimodel.py:418,469)
template <bool WS>
int dispatch_conv1d(const PncGemmParams& p, unsigned epi, hipStream_t st, const void* wlo16) {
    constexpr int AM = PNC_A_CONV1D_T;
    TileChoice tc = choose_tile(p);
    if (tc.tile == T_128x32) epi = E_GENERIC;
    if (p.gn_part) {
        if (gn_stats_in_epilogue(p, tc)) {
            switch (epi) {
                case E_R1 | E_RB | E_O32: return launch<AM, 256, 320, 4, 2, 2, false, E_R1 | E_RB | E_O32 | E_GS, WS>(p, st, 1, wlo16);
                case E_R1 | E_R2 | E_O32: return launch<AM, 256, 320, 4, 2, 2, false, E_R1 | E_R2 | E_O32 | E_GS, WS>(p, st, 1, wlo16);
                case E_R1 | E_R2 | E_O32 | E_O16: return launch<AM, 256, 320, 4, 2, 2, false, E_R1 | E_R2 | E_O32 | E_O16 | E_GS, WS>(p, st, 1, wlo16);
                default: break;
            }
        }
        // statistics not fused: the same launch without gn_part, then the statistics kernel over its fp32 output
        PncGemmParams q = p;
        q.gn_part = nullptr;
        const int rc = dispatch_conv1d<WS>(q, epi, st, wlo16);
        if (rc != PNC_OK) return rc;
        return pnc_groupnorm_stats(p.out32, p.ldc32, p.M / p.Npix, p.Npix, p.N, 64, p.gn_part, st);
    }
    switch (epi) {
        case E_R1 | E_RB | E_O32: return launch_tile<AM, E_R1 | E_RB | E_O32, WS>(p, st, tc, wlo16);             // h + conv1d + emb row
        case E_R1 | E_R2 | E_O32: return launch_tile<AM, E_R1 | E_R2 | E_O32, WS>(p, st, tc, wlo16);             // g + conv1d + skip
        case E_R1 | E_R2 | E_O32 | E_O16: return launch_tile<AM, E_R1 | E_R2 | E_O32 | E_O16, WS>(p, st, tc, wlo16);
        default: return launch_tile<AM, E_GENERIC, WS>(p, st, tc, wlo16);
    }
}

}  // namespace pnc_gemm
