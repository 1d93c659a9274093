// gemm_stencil_tile.hip — 3x3 conv (stride 1, pad 1, Cin % 64 == 0) as implicit GEMM over SPATIAL output tiles that
// contain their stencil neighbours.
//
// The per-tap gather (gemm_conv3x3.hip) DMAs, for every 64-channel slice of the input, nine A tiles — one per tap — that are
// the same pixels shifted by one: 9 x 32 KB per 256 output pixels, every byte of it through the L2 -> LDS path whose cost
// adds to the MFMAs' (DESIGN.md §4 "where the time goes").  Here a workgroup owns a TH x TW block of output pixels of one
// frame (16 x 16, or 8 x 32 where the image height is no multiple of 16), stages the block plus its halo —
// (TH + 2) x (TW + 2) pixels, 41-43 KB — ONCE per slice, and the nine taps read their A fragments from it at shifted LDS
// rows.  Per slice and 256 x 320 output tile: 41 + 9 x 40 KB instead of 9 x 32 + 9 x 40 KB — 1.6x fewer DMA bytes, same MFMAs,
// same LDS fragment reads.  Measured (MI355X, profiles/round2/kbench_r2k_stencil_tiles.log): level-0 convs 790-925 ->
// 915-1050 TFLOP/s, first-stage decoder convs 800 -> 960-1020.
// (The temporal k = 3 conv was built on the same scheme — 32 pixels x all 8 frames per tile, 1.4x fewer DMA bytes — and
// measured no faster: at K = 3 C its time is the two-stream fp32 epilogue's, not the operand path's.  Not kept.)
//
// BN = NI x 64 (320 where N is a multiple of 320, else 256), 8 waves as 4 x 2, wave tile 64 x (NI x 32).
// LDS: two halo buffers (slice c + 1 arrives, one 1-KB piece per wave and iteration, while slice c is consumed) and a ring of
// three W HALF tiles — 32 of the 64 channels of one (slice, tap) pair, BN rows x 64 B: 2 x 41 + 3 x 20 = 142 KB at BN = 320
// (whole 64-channel W stages would need 2 x 41.5 + 2 x 40 = 163 KB).  Counted vmcnt waits + one raw s_barrier per half
// tile, placed in the middle of its MFMA stream (software pipeline below): two half tiles in flight, one landed.
// The K order (slice, tap, channel) is the per-tap kernel's, so are the products: results are bit-identical to its
// (precise operands included: the lo plane's pass runs first, the accumulators are scaled by 2^-11, then the hi plane's; with split
// weights — PncGemmParams.W_lo — the lo pass is two runs of the slices, (A lo, W) then (A hi, W lo), ahead of the one scaling).
// The epilogue is gemm_kernel.h's epi_fast with a row map (RowHalo): tile-local row -> pixel of the frame.
#include "gemm_kernel.h"

namespace pnc_gemm {

// gemm_stencil_tile_body.inc is the kernel body, shared as TEXT by the two kernels below (see gemm_kernel.h on why not a function).
// WS (compile time; pnc_gemm_wsplit_f16, A_lo == NULL — the `gn_res` convs, which `precise` does not split): `wlo16` is the fp16 lo
// plane of the weights, in W's layout, beside the parameter block.  Two passes over the slices: (A, W lo), the one 2^-11 scaling,
// (A, W).  A zero plane leaves +0 in the accumulators: the bits of WS = false.
template <int TWS, int NI, unsigned EPI>     // TW = 2^TWS columns per spatial tile; BN = NI * 64
__global__ __launch_bounds__(512) void stencil_tile_kernel(const PncGemmParams pin, const int group_m, const int nfull, const int tail_f,
                                                           const int stagger) {
    constexpr bool WS = false;
    const void* const wlo16 = nullptr;
#include "gemm_stencil_tile_body.inc"
}

template <int TWS, int NI, unsigned EPI>
__global__ __launch_bounds__(512) void stencil_tile_ws_kernel(const PncGemmParams pin, const int group_m, const int nfull, const int tail_f,
                                                              const int stagger, const void* __restrict__ wlo16) {
    constexpr bool WS = true;
#include "gemm_stencil_tile_body.inc"
}

template <int TWS, int NI>
constexpr int stencil_lds_bytes() {
    constexpr int TW = 1 << TWS, TH = 256 / TW, HROWS = (TH + 2) * (TW + 2);
    return 2 * ((HROWS + 7) / 8) * 1024 + 3 * NI * 64 * 64;
}

template <int TWS, int NI, unsigned EPI, bool WS>
static int launch_stencil(const PncGemmParams& p, hipStream_t st, const void* wlo16) {
    constexpr int TW = 1 << TWS, TH = 256 / TW, BN = NI * 64;
    constexpr int lds = stencil_lds_bytes<TWS, NI>();
    static std::atomic<unsigned char> attr_done[64];
    const auto kern = [] {
        if constexpr (WS) return stencil_tile_ws_kernel<TWS, NI, EPI>;
        else return stencil_tile_kernel<TWS, NI, EPI>;
    }();
    set_dynamic_lds_once(attr_done, current_device(), kern, lds);
    const int tiles_m = (p.M / (p.Hout * p.Wout)) * (p.Hout / TH) * (p.Wout >> TWS), tiles_n = (p.N + BN - 1) / BN;
    int group_m = grouped_tile_order(tiles_m, tiles_n);
    if (group_m == 1) group_m = 0;                     // (this kernel's plain order is 0 alone)
    int nfull = tiles_m * tiles_n, tail_f = 1;
    tail_split<256, 4, lds>(tiles_m * tiles_n, nfull, tail_f);            // one workgroup per CU: 256 slots per round
    const int stagger = pnc_get_option(PNC_OPT_GEMM_STAGGER) == 1 ? 1 : (((pnc_get_option(PNC_OPT_STENCIL_TILES) & 4) ? 2 : 0) | ((pnc_get_option(PNC_OPT_GEMM_FUSE_LN) & 2) ? 4 : 0));
    const dim3 grid(nfull + (tiles_m * tiles_n - nfull) * tail_f);
    launch_kernel<WS>(kern, grid, dim3(512), lds, st, wlo16, p, group_m, nfull, tail_f, stagger);
    // (stagger = 1: the staggered schedule, measured 5-15 % slower than the pipeline, only on request; + 2: the pipeline with the fragment
    // addresses computed next to the reads, as in round 5; + 4: the fp32-only epilogue staged through LDS, as in round 5)
    return pnc_launch_status();
}

template <int TWS, int NI, bool WS>
static int dispatch_epi(const PncGemmParams& p, unsigned epi, hipStream_t st, const void* wlo16) {
    switch (epi) {
        case E_O16: return launch_stencil<TWS, NI, E_O16, WS>(p, st, wlo16);
        case E_O32: return launch_stencil<TWS, NI, E_O32, WS>(p, st, wlo16);
        case E_O32 | E_O16: return launch_stencil<TWS, NI, E_O32 | E_O16, WS>(p, st, wlo16);
        case E_R1 | E_O32: return launch_stencil<TWS, NI, E_R1 | E_O32, WS>(p, st, wlo16);
        case E_R1 | E_O32 | E_O16: return launch_stencil<TWS, NI, E_R1 | E_O32 | E_O16, WS>(p, st, wlo16);
        default: return PNC_EINVAL;
    }
}

// Geometry code the tile kernel would use for this problem — (TWS << 4) | NI — or 0 when the per-tap gather serves it: stride 2 /
// nearest-x2 gathers, narrow or ragged channel counts, images that do not tile, ragged epilogues, and (unless
// PNC_OPT_STENCIL_TILES = 2: tests) grids of fewer than 160 tiles: the per-tap kernels have split K for those (level 2, 192 tiles:
// +8 % on the tile kernel; a sparse last round — level 1: 384 tiles = 1.5 rounds — is tail-split here as there).
int conv3x3_tile_geometry(const PncGemmParams& p, unsigned epi) {
    const int opt = pnc_get_option(PNC_OPT_STENCIL_TILES) & 3;   // 0 off, 1 auto, 2 wherever the shape allows
    if (!opt) return 0;
    if (p.stride != 1 || p.upsample || p.conv_pad_br || (p.Cin & 63) || p.Hin != p.Hout || p.Win != p.Wout) return 0;
    if (p.K != 9 * p.Cin || p.M % (p.Hout * p.Wout)) return 0;
    // the tile kernel's lo pass reads fp16 planes (same MFMA as the hi pass): an e4m3 A_lo / W_lo pair is never selected here and
    // runs on the per-tap kernel, where W_lo keeps its e4m3 meaning
    if (p.A_lo && p.a_lo_fmt != PNC_LO_F16) return 0;
    if (epi != E_O16 && epi != E_O32 && epi != (E_O32 | E_O16) && epi != (E_R1 | E_O32) && epi != (E_R1 | E_O32 | E_O16)) return 0;
    int tws = 0;
    if ((p.Hout % 16) == 0 && (p.Wout % 16) == 0) tws = 4;
    else if ((p.Hout % 8) == 0 && (p.Wout % 32) == 0) tws = 5;
    if (!tws) return 0;
    int ni = (p.N % 320 == 0) ? 5 : 4;
    if (ni == 5 && (p.N & 255) == 0) {
        // a grid that fits one round either way: 256-column tiles fill more of the chip (level 2: 48 x 5 = 240 workgroups of
        // 256x256 instead of 48 x 4 = 192 of 256x320)
        const long t5 = (long)(p.M / 256) * (p.N / 320), t4 = (long)(p.M / 256) * (p.N / 256);
        if (t5 < 256 && t4 <= 256) ni = 4;
    }
    if (opt == 1) {
        const long tiles = (long)(p.M / 256) * ((p.N + ni * 64 - 1) / (ni * 64));
        if (tiles < 160 || p.N < 256) return 0;
    }
    return (tws << 4) | ni;
}

// WS: the same geometries with the weight part (pnc_gemm_wsplit_f16)
template <bool WS>
int dispatch_conv3x3_tiles(const PncGemmParams& p, unsigned epi, int geometry, hipStream_t st, const void* wlo16) {
    if constexpr (WS) {
        if (p.A_lo) return PNC_EINVAL;          // the tile kernel's weight part is the two-pass form for A_lo == NULL (the `gn_res` convs)
    }
    switch (geometry) {
        case (4 << 4) | 5: return dispatch_epi<4, 5, WS>(p, epi, st, wlo16);
        case (4 << 4) | 4: return dispatch_epi<4, 4, WS>(p, epi, st, wlo16);
        case (5 << 4) | 5: return dispatch_epi<5, 5, WS>(p, epi, st, wlo16);
        case (5 << 4) | 4: return dispatch_epi<5, 4, WS>(p, epi, st, wlo16);
        default: return PNC_EINVAL;
    }
}
template int dispatch_conv3x3_tiles<false>(const PncGemmParams&, unsigned, int, hipStream_t, const void*);
template int dispatch_conv3x3_tiles<true>(const PncGemmParams&, unsigned, int, hipStream_t, const void*);

}  // namespace pnc_gemm

PNC_DEFINE_TU_COLLECT(gemm_stencil_tile)
