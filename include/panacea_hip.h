/*
 * panacea_hip.h — C-ABI of libpanacea_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the Panacea denoising hot path.  The reference
 * (wenyuqing/panacea) ships no native code: every arithmetic call-site on the
 * path is a PyTorch / xformers / cuDNN / cuBLAS call.  Each entry point below
 * replaces one family of those call-sites; the citation after each prototype is
 * the reference call-site (path relative to the reference root) it stands in for.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers (HBM);
 *   - `stream` is a hipStream_t passed as void*; work is only enqueued, never
 *     synchronised; no allocation, no global state -> safe under hipGraph capture;
 *   - return value: 0 on success, a hipError_t (>0) from the launch, or a negative
 *     PNC_E* code for an argument the kernel family does not support;
 *   - activations are channels-last token matrices: row m = (frame f, y, x),
 *     m = (f*H + y)*W + x, columns = channels.  fp16 operands, fp32 residual
 *     stream ("h32") — see DESIGN.md §3.
 */
#ifndef PANACEA_HIP_H
#define PANACEA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNC_OK 0
#define PNC_EINVAL (-1)   /* unsupported shape / argument */
#define PNC_EALIGN (-2)   /* pointer or leading dimension not 16-byte aligned */
#define PNC_EABI (-3)     /* parameter struct compiled against another version of this header */

/* library / build identification: returns "panacea_hip <version> gfx950" */
const char* pnc_version(void);
/* ABI revision of this header (bumped whenever a parameter struct, a prototype or the option list changes): 7
 * (round 4: + pnc_groupnorm_combine, + PNC_OPT_ATTN_DEFER_MAX, PNC_OPT_GEMM_PERSIST is a bit set, - pnc_ff_chain_*;
 *  round 5 (5, 6): + pnc_concat_add_stats, + PNC_OPT_GEMM_STAGGER, + pnc_linear_smallm_segments;
 *  round 6 (7): + PNC_OPT_ATTN_SUM_TRIGGER;
 *  8: + pnc_cfg_sampler_step / PncSamplerStepParams;
 *  still 8 (additive, no struct / prototype / option changes): PncGemmParams.W_lo next to an fp16 A_lo is the fp16 lo plane of the
 *  weights, + pnc_linear_smallm_split / pnc_linear_smallm_segments_split.  One check is stricter for existing callers: a non-NULL
 *  PncGemmParams.W_lo with A_lo = NULL, which pnc_gemm_f16 used to ignore, is now PNC_EINVAL — clear the field with A_lo;
 *  still 8 (additive): + pnc_attn_uses_text_kernel.  One dispatch is narrower: the few-key kernel takes key buffers whose row count
 *  kvH * kvW is a multiple of 8 only, a ragged buffer (77 rows) runs on the general kernel — same attention, see PncAttnParams.kv_valid;
 *  still 8 (additive): + pnc_gemm_wsplit_f16;
 *  still 8 (additive): + pnc_frames_renoise;
 *  still 8 (additive): + pnc_latent_renoise_masked, + pnc_mask_pool_u8, + pnc_u8_select) */
#define PNC_ABI_VERSION 8
int pnc_abi_version(void);
/* hex SHA-256 of the sources + compile flags the library was built from (panacea_amd/build.py computes the same digest over
 * the checkout): a loader compares the two and refuses a library built from other sources instead of calling it with
 * shifted argument lists */
const char* pnc_build_digest(void);

/* Tuning / test switches (process-global, read with one relaxed atomic load per launch; results never depend on them
 * beyond what each option states).  Returns the previous value, or PNC_EINVAL for an unknown option. */
enum {
    PNC_OPT_GEMM_TAIL_SPLIT = 0,  /* 1 (default): run a sparse last round of output tiles as half / quarter-row workgroups
                                     (bit-identical to 0: rows of a GEMM are independent) */
    PNC_OPT_GEMM_TILE = 1,        /* 0 (default): score-based tile choice; 1 = 128x128, 2 = 256x128, 3 = 256x320,
                                     4 = 256x256 force a geometry where the shape allows it (kernel micro-benchmarks) */
    PNC_OPT_ATTN_VARIANT = 2,     /* 0 (default): by view size; 41 / 81 / 42 / 82 = (waves, query blocks per wave); 42 (large views, default) runs two independent
                                     4-wave workgroups per CU (<= 256 registers); 1 = by view size with 82 (round 3's choice) in the place of 42;
                                     43 = the single-pass few-key kernel (round 6: 64 < kv_valid <= 96 keys shared by all queries of a group —
                                     the text tokens; default there when the grid fills the chip) wherever it applies; any other non-zero
                                     value keeps attn_views_kernel for those launches too (A/B) */
    PNC_OPT_ATTN_DMA = 3,         /* 1 (default): LDS-DMA staging of K / V^T tiles where alignment allows, tile addresses kept as lane constant +
                                     wave-uniform offset; 2 = LDS-DMA with per-tile recomputed addresses (A/B); 0 = register staging.  Same results.
                                     + 4 (round 6, A/B): the few-key launches stay on attn_views_kernel instead of attn_text_kernel */
    PNC_OPT_GEMM_FUSE_LN = 4,     /* bit 0, 1 (default): PncGemmParams.ln_* is reduced in the GEMM epilogue where a workgroup owns whole
                                     rows; 0 = always the LayerNorm kernel after the GEMM (A/B measurements; same result).
                                     + 2 (round 6, A/B): fp32-only epilogues (out32 = acc + bias [+ res1]) of full 256-row tiles go through
                                     the LDS staging, as in round 5, instead of straight from the accumulators.  Bit-identical */
    PNC_OPT_GEMM_GROUP_M = 5,     /* 0 (default): tiles of a GEMM with more than 8 column tiles are walked in groups of 4 row panels
                                     (L2 reuse of W where it exceeds the cache); k > 1 forces groups of k; 1 = plain order.  Results
                                     do not depend on it (same tiles, same arithmetic) */
    PNC_OPT_STENCIL_TILES = 6,    /* 1 (default): stride-1 3x3 convs with Cin % 64 == 0 on grids that fill the chip stage ONE spatial tile of
                                     the input incl. its halo per 64-channel slice and read the nine taps from it (gemm_stencil_tile.hip);
                                     0 = always one gathered A tile per tap; 2 = wherever the shape allows (tests); + 4 (round 6, A/B): the
                                     tile kernel computes its fragment addresses next to the reads (round 5) instead of one MFMA batch
                                     ahead of them.  Bit-identical results either way */
    PNC_OPT_GEMM_PERSIST = 7,     /* bit set, 3 (default).  Bit 0: GEGLU GEMMs of >= 512 full 256x256 tiles run as ONE persistent workgroup
                                     per CU that requests the next output tile's first K tile before its epilogue; bit 1 (round 4): the
                                     same for plain-A launches of >= 512 full 256x320 tiles with a row-major epilogue (residual in place,
                                     fused LayerNorm, fp16 / channel-major outputs, e4m3 lo pass).  Same results either way; 0 = one
                                     tile per workgroup */
    PNC_OPT_ATTN_DEFER_MAX = 8,   /* k (default 8): pnc_attn_views_f16 keeps a query's running softmax maximum — and skips the
                                     rescaling of its accumulators — until some query of the wave exceeds it by more than k in the
                                     exp2 domain (probabilities then reach at most 2^k: fp16-safe up to 15); 0 = rescale whenever a
                                     maximum grows.  Same softmax, other roundings of P (not bit-identical across values) */
    PNC_OPT_GEMM_GN_STATS = 9,    /* 1 (default): PncGemmParams.gn_part comes out of the temporal conv's epilogue where its waves own whole
                                     groups; 0 = always the statistics kernel after the GEMM (same records up to fp32 summation order) */
    PNC_OPT_GEMM_STAGGER = 10,    /* k (default 4 since round 6 — level-0 FF1, K = 320 = 5 tiles, measured 434 -> 420 us staggered; 8 in round 5): the
                                     persistent GEGLU GEMM runs K loops of at least k tiles in the STAGGERED schedule —
                                     four phases per K tile {fragment reads + a third of the next tile's DMA | barrier | MFMAs | barrier},
                                     waves 4-7 one barrier behind waves 0-3, so that on every SIMD one wave multiplies while the other
                                     reads (FF1 at levels 1-2: +5-6 %); 0 = never (round 4's loops); 1 = everywhere the schedule exists —
                                     also the plain-A 8-wave two-stage kernels and the stencil-tile conv kernel, where it measured no
                                     faster (tests, A/B tools).  Same K and MFMA order per accumulator: bit-identical results.
                                     + 256 (round 6, A/B): the persistent GEGLU kernel's products go through its LDS slab (round 3) instead
                                     of straight from the registers through two-byte buffer stores.  Same values */
    PNC_OPT_ATTN_SUM_TRIGGER = 11, /* k (default 12; round 6): after a query block's first K/V tile pnc_attn_views_f16 forms the probabilities
                                     against the running maximum AS IT IS and lets the row sum (needed anyway) tell whether that was safe — a
                                     lane's probabilities are each <= their sum, so sum < 2^k bounds every P below 2^k (fp16-safe up to 14) —
                                     and only a tile whose sum reaches 2^k (or is not finite) computes the row maximum and rescales; 0 = the
                                     row maximum of every tile (round 5).  Same softmax, other roundings of P (as PNC_OPT_ATTN_DEFER_MAX) */
    PNC_OPT_COUNT = 12
};
int pnc_set_option(int option, int value);

/* ------------------------------------------------------------------------- *
 * 1. MFMA GEMM family:  C[M,N] = gatherA[M,K] (fp16) x W[N,K]^T (fp16), fp32 acc
 *
 *   a_mode PNC_A_PLAIN   : A row-major [M][lda]
 *     -> nn.Linear call-sites (sgm/modules/attention.py:94,107,113,220-225,
 *        398-403,509-514,959,980,1040-1059) and 1x1 convs
 *        (sgm/modules/diffusionmodules/openaimodel.py:486, controlmodel.py:81-84)
 *   a_mode PNC_A_CONV3X3 : implicit GEMM over an NHWC fp16 image
 *        [F][Hin][Win][Cin], K = 9*Cin, pad 1, stride 1|2, optional nearest x2
 *        upsample of the input.  K order of W: (ky,kx,ci) when Cin % 64 != 0, else
 *        (ci/64, ky, kx, ci%64) — the nine taps of a 64-channel slice are adjacent
 *        K tiles, so their reads of one pixel neighbourhood hit L1/L2
 *     -> nn.Conv2d 3x3 (openaimodel.py:413,459,125 (Upsample),187 (Downsample),
 *        974 (stem), 1251 (out); controlmodel.py:44-58 (hint stem))
 *   a_mode PNC_A_CONV1D_T: temporal conv1d k=3 pad 1 over frames of one pixel,
 *        rows m = (b*T+t)*Npix + p, K = 3*C ordered (dt,ci), or (ci/64, dt, ci%64) when C % 64 == 0
 *     -> nn.Conv1d (openaimodel.py:418,469) applied on "(b h w) c t"
 *
 *   epilogue (all optional, applied in this order):
 *     v = acc + bias[n] + rowbias[((m / rb_rows) % rb_mod)*N + n]
 *     if geglu: v = value * gelu_erf(gate) on interleaved 32-column blocks
 *               (attention.py:91-98); output has N/2 columns
 *     if act == PNC_ACT_SILU: v = v*sigmoid(v);  PNC_ACT_GELU: v = v*Phi(v)
 *     v += res1[m*ldr1+n] + res2[m*ldr2+n]          (fp32 residual stream)
 *     out32[m*ldc32+n] = v;  out16[m*ldc16+n] = (fp16)v  for n <  n_split
 *     out16t[(m/t_rows)*t_gstride + (n-n_split)*ldt + m%t_rows] = (fp16)v for n >= n_split
 *   RANGE of the operands: every finite fp16 value, subnormals included — nothing is flushed.  The accumulation is fp32 with an
 *   error relative to sum |a| |w|, with one exception the MI355X's fp16 MFMA makes: a product with an fp16-SUBNORMAL factor
 *   (below 2^-14) is exact going in but is aligned in the adder as if that factor were 2^-14, so its truncation is relative to
 *   2^-14 |other factor|, not to the product.  A row of A that lies entirely at 2^-24 therefore keeps ~14 of fp32's 24 bits; from
 *   2^-14 on the full precision holds.  (tests/test_gemm_range_gpu.py; tests/gemm_ref64.py MFMA_UNNORMALISED_SUBNORMALS.)
 * ------------------------------------------------------------------------- */
enum { PNC_A_PLAIN = 0, PNC_A_CONV3X3 = 1, PNC_A_CONV1D_T = 2 };
/* Storage format of the lo plane of a precise ("split") operand, r = (v - fp16(v)) * 2^11  (PncGemmParams.A_lo):
 *   PNC_LO_F16  : fp16(r), two bytes per element, same leading dimension as the hi plane
 *   PNC_LO_E4M3 : OCP fp8 e4m3 of r clamped to +-448, ONE byte per element, same leading dimension IN ELEMENTS.  |r| <= |v|, so
 *                 no block scale is needed: e4m3 resolves r to 2^-4, i.e. the pair to ~2^-15 of v, and what falls below its
 *                 smallest subnormal (2^-9) is below 2^-20 absolute.  The consumer GEMM runs the lo K loop on the block-scaled
 *                 fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, twice the fp16 rate on half the bytes) with the 2^-11 as the A scale.
 *                 RANGE: r reaches 2^e for |v| in [2^e, 2^(e+1)), so from |v| >= 512 on the clamp at 448 can bite: there the pair
 *                 degrades gracefully (no NaN / Inf) from ~2^-15 of v towards the plain fp16 operand's 2^-11 — for |v| in
 *                 [512, 1024) only the residuals in the top eighth of the rounding interval clamp, from 2048 on most do.
 *                 The denoiser's split operands are normalised activations and fp16 copies of the residual stream; the three
 *                 parity pins (synthetic weights) do not probe the range, and the published checkpoint is not available offline
 *                 to measure its stream.  A caller whose operands reach the hundreds keeps PNC_LO_F16 for them
 *                 (engine.Precision(lo8=False), policy "precise-f16lo").  tests/test_lo8_gpu.py holds values of 700, 1200, 60000;
 *                 tests/test_gemm_range_gpu.py holds the GEMM family over the whole range below 65504: as a CONSUMER (A_lo bytes from
 *                 e4m3's subnormals to the +-448 of a clamped producer, w_lo_exp from 96 to 130) and as a PRODUCER — a launch that
 *                 writes out32 next to an e4m3 out16_lo writes out16 = fp16(out32) and the byte e4m3(clamp((out32 - out16) * 2^11))
 *                 exactly, at any magnitude; beyond the clamp |v - (out16 + 2^-11 out16_lo)| <= |v - out16|, and no written byte is
 *                 the NaN code 0x7F / 0xFF. */
enum { PNC_LO_F16 = 0, PNC_LO_E4M3 = 1 };
enum { PNC_ACT_NONE = 0, PNC_ACT_SILU = 1, PNC_ACT_GELU = 2 /* erf GELU: open_clip text-tower MLP */ };

typedef struct PncGemmParams {
    const void* A;          /* fp16 */
    const void* W;          /* fp16 [N][K] row-major (K contiguous) */
    int32_t M, N, K;
    int32_t lda;            /* PNC_A_PLAIN: elements between rows of A */
    int32_t a_mode;
    /* PNC_A_CONV3X3 */
    int32_t Cin, Hin, Win, Hout, Wout, stride, upsample;
    /* PNC_A_CONV1D_T (Cin = channels) */
    int32_t T, Npix;
    /* epilogue */
    const float* bias;      /* [N] or NULL */
    const float* rowbias;   /* [rb_mod][N] or NULL */
    int32_t rb_rows, rb_mod;
    const float* res1; int32_t ldr1;
    const float* res2; int32_t ldr2;
    float*  out32;  int32_t ldc32;
    void*   out16;  int32_t ldc16;
    void*   out16t; int32_t ldt; int32_t t_rows; int64_t t_gstride;
    int32_t n_split;        /* multiple of 128 (or >= N when out16t == NULL) */
    int32_t act;
    int32_t geglu;
    /* split-K workspace, caller-owned (NULL / 0: K is never split).  Small-M shapes (the 4x48 level: M = 3072)
     * fill only 60-120 of the 256 CUs with one K loop per output tile; with a workspace of
     * pnc_gemm_workspace_floats() floats the library runs `s` K-slices per tile and sums the fp32 partials in a
     * fixed order (deterministic) in a second launch that also applies the epilogue. */
    float*  ws;
    int64_t ws_floats;
    /* PNC_A_CONV3X3: 0 = one zero row/column on every side (Conv2d padding=1); 1 = zero padding on the bottom / right
     * only, i.e. F.pad(x, (0,1,0,1)) + Conv2d(padding=0) — the stride-2 Downsample of the first-stage encoder
     * (sgm/modules/diffusionmodules/model.py:108-112) */
    int32_t conv_pad_br;
    /* sizeof(PncGemmParams) as the CALLER compiled it.  pnc_gemm_f16 / pnc_gemm_workspace_floats return PNC_EABI when
     * it differs from the library's, instead of reading past a shorter struct (ABI version 4: 320 bytes). */
    int32_t struct_bytes;
    /* Precise ("split") activation operands.  An fp16 operand v is carried as two fp16 planes,
     *     hi = fp16(v),   lo = fp16((v - hi) * 2^11)        (a 22-bit operand; the 2^11 keeps lo out of the subnormals)
     * A_lo   : lo plane of A (same layout / lda / gather as A), or NULL for a plain fp16 operand.  The kernel runs the
     *          K loop over the lo plane first, scales the accumulators by 2^-11, then runs the hi plane: twice the MFMA
     *          work of the call-site, W is read from L2 twice.
     * out16_lo : lo plane written next to out16 (same ldc16), or NULL.
     * Used by the call-sites whose operand rounding dominates the eps error: the reference
     * computes these contractions in fp32 on CPU / fp16 autocast on GPU (wrappers.py:37-70). */
    const void* A_lo;
    void* out16_lo;
    /* elements between rows of W (0 = K: dense [N][K]).  A strided W lets the K matrix of one attention head, a column
     * block of a [tokens][C] projection buffer, serve as the second operand of S = Q K^T (text tower, first-stage mid block) */
    int32_t ldw;
    /* LayerNorm of the fp32 output rows, fused (attention.py:726-747: x = attn(norm(x)) + x followed by the next norm):
     *   ln_out16[m*ldln + n] = fp16( (out32[m][n] - mean_m) * rstd_m * ln_gamma[n] + ln_beta[n] ),  statistics over the N columns.
     * ln_out16 NULL = off.  Needs out32 and no GEGLU / V^T.  When one workgroup owns whole rows (N <= its tile width: the
     * level-0 width 320) the row statistics are reduced in the epilogue and the normalised fp16 row is written by the GEMM
     * itself (the LayerNorm launch and its 4-byte read of the stream disappear); otherwise the library runs its LayerNorm
     * kernel right after the GEMM on the same stream — same result either way. */
    float ln_eps;
    const float* ln_gamma;
    const float* ln_beta;
    void* ln_out16;
    int32_t ldln;
    /* formats of A_lo / out16_lo (PNC_LO_*).  a_lo_fmt = PNC_LO_E4M3 needs the weight side of the lo pass as well:
     *   W_lo     : e4m3 [N][ldw_lo] bytes, W_lo[n][k] = e4m3(W[n][k] * 2^(127 - w_lo_exp)) in the K order of W
     *   w_lo_exp : E8M0 exponent byte of the tensor, 1..254 (W ~ W_lo * 2^(w_lo_exp - 127)); the packer picks it so that the
     *              tensor maximum lands in [224, 448] — e4m3's 17 binades below that cover every weight that matters
     * and 16-byte chunks of 16 consecutive k: PNC_A_PLAIN lda % 16 == 0 and K % 16 == 0; the conv gathers Cin % 64 == 0. */
    int32_t a_lo_fmt;
    int32_t out_lo_fmt;
    /* SPLIT WEIGHTS (a_lo_fmt = PNC_LO_F16, A_lo != NULL): a non-NULL W_lo is the fp16 lo plane of the weights,
     *   the weights w = W_hi + 2^-11 * W_lo,  W_hi = W = fp16(w),  W_lo[n][k] = fp16((w - fp16(w)) * 2^11),
     * in W's layout, K order and leading dimension, 16-byte aligned; w_lo_exp is ignored.  The lo pass then runs a second set of K
     * tiles, A's hi plane against W_lo, into the same accumulators ahead of the one 2^-11 scaling:
     *   A w ~= A_hi W_hi + 2^-11 (A_lo W_hi + A_hi W_lo)      (the 2^-22 A_lo W_lo term is dropped; valid for |w| < 65504)
     * — three times the MFMA work of the plain launch.  A misaligned W_lo is PNC_EALIGN.  A non-NULL W_lo without A_lo is
     * PNC_EINVAL whatever a_lo_fmt says (before split weights such a pointer was ignored: callers that reuse a struct clear it).
     * Next to an e4m3 A_lo, W_lo is the e4m3 plane described above in every kernel; the 3x3 halo-tile kernel has no e4m3 pass and is
     * not selected for such a launch (the per-tap kernel runs it).
     * ldw_lo has the unit of the plane it strides.  e4m3 W_lo: BYTES between its rows, 0 = K.  fp16 W_lo: ELEMENTS between its
     * rows, and since the plane has W's leading dimension the only accepted values are 0 and ldw (K when ldw = 0); anything else
     * is PNC_EINVAL. */
    int32_t ldw_lo;
    const void* W_lo;
    int32_t w_lo_exp;
    /* PNC_A_CONV1D_T: 1 = A (and A_lo) hold T + 2 frames per sample, row (b, t, pixel) at ((b (T + 2) + t + 1) Npix + pixel): the
     * frame before the first and after the last of the T frames the rows speak of are present — a frame group's halo frames
     * (engine.FrameShard: the neighbour rank's frame, zeros at the two ends of the clip) — and no tap is padded */
    int32_t t_halo;
    /* PNC_A_CONV3X3 over a BAND of a wider image (engine.ViewShard: a rank's columns of the panorama): 0 = off; otherwise the
     * element offset from A (and from A_lo, in its own elements) to a block [2][frames][Hin][Cin] holding image column -1 (side
     * 0) and column Win (side 1) of every row — the neighbour ranks' edge columns, zeros at the two ends of the panorama.  The
     * taps that leave the band on the left / right read it instead of zero padding; rows above / below the image stay padded.
     * Band, block and everything between them must lie within 2^31 bytes of each frame's origin. */
    int64_t x_halo_off;
    /* PNC_A_CONV1D_T: GroupNorm(32) statistics of the fp32 output, from the GEMM (util.py:276-283: the GroupNorm that follows
     * every temporal conv of a ResBlock3D reads what this launch writes).  NULL = off; otherwise [frames][ceil(Npix / 64)][32][3]
     * floats that receive the {n, mean, M2} records pnc_groupnorm_stats(out32, ldc32, frames, Npix, N, 64, gn_part) would
     * write — frames = M / Npix, channels = N — for pnc_groupnorm_apply(..., n_records = ceil(Npix / 64)).  When a workgroup's
     * waves own whole groups (N % 320 == 0 on the 256x320 tile, Npix % 64 == 0) the records come out of the epilogue, one per
     * (64-row block, group), in a fixed summation order; otherwise the library launches its statistics kernel after the GEMM
     * on the same stream.  Needs out32 (ldc32 % 4 == 0), N % 64 == 0. */
    float* gn_part;
} PncGemmParams;

int pnc_gemm_f16(const PncGemmParams* p, void* stream);
/* pnc_gemm_f16 with SPLIT WEIGHTS BESIDE the parameter block (the `precise-ckpt` operand policy: the operand classes and e4m3 lo planes
 * of `precise`, on an fp32 checkpoint).  W_lo16[n][k] = fp16((w - fp16(w)) * 2^11) is the fp16 lo plane of the weights as in
 * PncGemmParams.W_lo: W's layout, K order and leading dimension (p->ldw), 16-byte aligned.  *p is validated exactly as by pnc_gemm_f16
 * and keeps every meaning it has there — p->W_lo stays the e4m3 copy that goes with an e4m3 A_lo, and is NULL otherwise.
 *   p->A_lo NULL or e4m3: the weight part runs FIRST — the K tiles (of the slice, when K is split) with A's hi plane against W_lo16 into
 *     zeroed accumulators, then the one exact 2^-11 scaling — followed by the launch as pnc_gemm_f16 runs it (the e4m3 lo tiles, whose
 *     block scale lands their products at their final weight, then the hi pass):
 *         A w ~= A_hi W_hi + 2^-11 (A_lo W_hi [if A_lo] + A_hi W_lo16)
 *     One more fp16 pass over K.  With W_lo16 all zero the result is bit-identical to pnc_gemm_f16(p).  The tile and split-K choice,
 *     pnc_gemm_workspace_floats and pnc_gemm_fuses_layernorm answer for this launch what they answer for pnc_gemm_f16(p); the
 *     persistent GEGLU kernel (PNC_OPT_GEMM_PERSIST bit 0) runs the part in the same order; the persistent plain-A kernel (bit 1) has
 *     none: its launches run one tile per workgroup on the same tiles.
 *   p->A_lo fp16: FORWARDED to pnc_gemm_f16 with W_lo = W_lo16 (the three-part launch described at PncGemmParams.W_lo); a non-NULL
 *     p->W_lo next to it is PNC_EINVAL.
 * W_lo16 NULL: PNC_EINVAL.  W_lo16 not 16-byte aligned: PNC_EALIGN. */
int pnc_gemm_wsplit_f16(const PncGemmParams* p, const void* W_lo16, void* stream);
/* 1 when pnc_gemm_f16 would reduce p->ln_* inside the GEMM epilogue for this problem, 0 when it would launch its LayerNorm
 * kernel after the GEMM (a caller that times kernel families separately can then issue pnc_layernorm itself) */
int pnc_gemm_fuses_layernorm(const PncGemmParams* p);
/* floats of workspace with which pnc_gemm_f16 would split K for this problem (0: it would not) */
int64_t pnc_gemm_workspace_floats(const PncGemmParams* p);

/* ------------------------------------------------------------------------- *
 * 2. View-sliced flash attention, head dim 64, fp16 in/out, fp32 softmax/acc.
 *    q rows/kv rows live in token matrices (row m = (group g, y, x)); the query
 *    grid of one group is H x W split along the width into `views` equal slices.
 *    For query view v the key set is the concatenation of kv views
 *    seg[v][0..nseg[v]) of kv group (g / q_per_kv).
 *    K is row-major [rows][ldk]; V is channel-major ("V^T"):
 *        vt[kvg*vt_gstride + (head*64+d)*ldvt + token]
 *    Only the first kv_valid keys of each kv view exist (rest masked).
 *     -> xformers.ops.memory_efficient_attention (attention.py:469 intra-view,
 *        :590 inter-view incl. the view-5 quirk, :363) and
 *        F.scaled_dot_product_attention (attention.py:281) for text keys; with `causal`, the attention of the OpenCLIP
 *        text tower's residual blocks (all heads of all prompts in one launch).
 * ------------------------------------------------------------------------- */
typedef struct PncAttnParams {
    const void* q;  int32_t ldq;    /* fp16, head h at column h*64 */
    const void* k;  int32_t ldk;
    const void* vt; int32_t ldvt; int64_t vt_gstride;
    void* o;        int32_t ldo;
    int32_t groups;                 /* number of q groups (frames) */
    int32_t heads;
    int32_t H, W, views;            /* q grid per group, W % views == 0 */
    int32_t kvH, kvW, kv_views;     /* kv grid per kv group */
    int32_t kv_rows_per_group;      /* rows of K per kv group */
    int32_t q_per_kv;               /* kv group = g / q_per_kv */
    int32_t kv_valid;               /* valid keys per kv view (<= kvH*kvW/kv_views).  PADDING CONTRACT, Nkv = kvH*kvW/kv_views keys per view:
                                       the K rows and V^T entries of keys kv_valid .. Nkv - 1 of a view ARE read and must be finite (a
                                       probability of exactly 0 does not silence a NaN or Inf); their values do not influence the output,
                                       not by one bit.  Nothing at or beyond key Nkv of a view, and no row at or beyond row kvH*kvW of a
                                       group's K, is read: a V^T row may end at its last key, whatever ldvt says */
    int32_t nseg[8];                /* per q view */
    int32_t seg[8][2];              /* kv view ids */
    float scale;                    /* softmax scale (d^-0.5) */
    int32_t causal;                 /* 1: query i of a view attends keys j <= i of each kv view only (view-local indices) —
                                       the text tower's causal mask (open_clip build_attention_mask; modules.py:559-632); 0 else */
    /* ABI 5 (round 5): HALO views of a band of views (engine.ViewShard: the cross-view attention of a rank that holds n of the six
     * views attends one view of each neighbour rank as well, attention.py:545-559).  NULL = off.  Otherwise kv view id -1 in seg[][]
     * reads k_halo[0] / vt_halo[0], id kv_views reads k_halo[1] / vt_halo[1]: buffers of EXACTLY the band's geometry (ldk, kvW,
     * kv_rows_per_group, ldvt, vt_gstride) whose view column 0 holds the neighbour's view (the rest is never read).  The band's own
     * K / V^T stay where the QKV GEMM wrote them: no (n + 2)-view copy of keys and values. */
    const void* k_halo[2];
    const void* vt_halo[2];
} PncAttnParams;

int pnc_attn_views_f16(const PncAttnParams* p, void* stream);
/* 1 when pnc_attn_views_f16 would launch its single-pass few-key kernel (PNC_OPT_ATTN_VARIANT: 43) for these parameters under the
 * current options, 0 when the general kernel runs or the parameters are refused — answered by the dispatch's own predicate.  The
 * few-key kernel needs: one view, one segment, not causal, kvH * kvW <= 96 and a multiple of 8, 64 < kv_valid <= 96, ldvt /
 * vt_gstride / ldk multiples of 8; unforced, also 16 or more workgroups per group (query tiles of 128 x groups of 5 heads) */
int pnc_attn_uses_text_kernel(const PncAttnParams* p);

/* Temporal self-attention over the T frames of one pixel (head dim 64), 1 <= T <= 16:
 *   row m = (b*T+t)*Npix + p; q/k/v fp16 with leading dims; out fp16.
 *   T <= 8: VALU kernel, 8 lanes per (frame, head); 9 <= T <= 16: one wave per (b, pixel, head) on the 16x16 MFMA
 *   (B * Npix * heads < 2^31).  No row beyond frame T - 1 of a sample is read.  Other T: PNC_EINVAL.
 *    -> CrossAttention self-attn on "(b h w) t c" (attention.py:229-291, 1106-1134) */
int pnc_attn_temporal_f16(const void* q, int ldq, const void* k, int ldk,
                          const void* v, int ldv, void* o, int ldo,
                          int B, int T, int Npix, int heads, float scale, void* stream);

/* Attention on SPLIT operands (the `precise-wide` operand policy: every operand carried as v ~ hi + lo * 2^-11, both planes fp16,
 * valid up to |v| < 65504).  Products on the MFMA, fp32 accumulation and softmax:
 *   S = Qh.Kh + 2^-11 (Qh.Kl + Ql.Kh)          (lo.lo dropped)
 *   P = softmax(scale * S),  P = Ph + 2^-11 Pl  (fp16 pair)
 *   O = Ph.Vh + 2^-11 (Ph.Vl + Pl.Vh),  written as hi + fp16 lo planes.
 * Every lo plane has the leading dimension of its hi plane; pointers 8-byte aligned, leading dimensions % 4 == 0.
 *
 * pnc_attn_views_split_f16: the geometries of pnc_attn_views_f16 (intra-view, cross-view with one or two kv segments, text keys
 * masked per key with kv_valid) EXCEPT that V is read ROW-major, laid out like K: `a.vt` points at V[key row][channel] with
 * leading dimension `a.ldvt` (the QKV GEMM's out16 + out16_lo form; no lo plane exists for the transposed out16t store) and
 * `a.vt_gstride` is ignored.  causal = 1 and the halo views (k_halo / vt_halo) are not supported (PNC_EINVAL).
 * Returns PNC_EABI when struct_bytes != sizeof(PncAttnSplitParams). */
typedef struct PncAttnSplitParams {
    int32_t struct_bytes;   /* sizeof(PncAttnSplitParams) as the caller compiled it */
    PncAttnParams a;
    const void* q_lo;
    const void* k_lo;
    const void* v_lo;
    void* o_lo;
} PncAttnSplitParams;
int pnc_attn_views_split_f16(const PncAttnSplitParams* p, void* stream);
/* temporal self-attention of pnc_attn_temporal_f16 on split operands (T <= 16) */
int pnc_attn_temporal_split_f16(const void* q, const void* q_lo, int ldq, const void* k, const void* k_lo, int ldk,
                                const void* v, const void* v_lo, int ldv, void* o, void* o_lo, int ldo,
                                int B, int T, int Npix, int heads, float scale, void* stream);

/* ------------------------------------------------------------------------- *
 * 3. Normalisations (fp32 stream in, fp16 operand out).  y16_lo (may be NULL) receives the lo plane of a precise
 *    operand, same layout as y16 (see PncGemmParams.A_lo), in the format lo_fmt (PNC_LO_*; pnc_layernorm: fp16 only).
 * ------------------------------------------------------------------------- */
/* Spatial GroupNorm(32,C) over one frame's (H*W, C/32) slab, two launches.
 *   stats: partial[(f*nchunk + chunk)*32 + g] = {count, mean, M2}
 *   apply: y = (x-mean)*rstd*gamma+beta, optional SiLU, -> fp16 [F*Npix][ldy].  n_records: records per frame in `partial`
 *          (0 = ceil(Npix / pix_per_chunk), what pnc_groupnorm_stats with the same chunking wrote; another count when they come
 *          from elsewhere: PncGemmParams.gn_part writes ceil(Npix / 64) per frame) — pix_per_chunk only shapes the apply's own grid
 *    -> nn.GroupNorm (diffusionmodules/util.py:283 eps 1e-5; attention.py:129-132 eps 1e-6) + nn.SiLU */
int pnc_groupnorm_stats(const float* x, int ldx, int F, int Npix, int C,
                        int pix_per_chunk, float* partial, void* stream);
int pnc_groupnorm_apply(const float* x, int ldx, int F, int Npix, int C,
                        int pix_per_chunk, const float* partial,
                        const float* gamma, const float* beta, float eps, int silu,
                        void* y16, int ldy, void* y16_lo, int lo_fmt, int n_records, void* stream);
/* Chan-combine `parts` sets of chunk records, in[((s*F + f)*nchunk + c)*32 + g] = {count, mean, M2} (the all-gathered
 * pnc_groupnorm_stats records of the bands of a view group), per (frame, group), in the fixed order (s, c):
 * out[(f*nchunk + 0)*32 + g] = the combined record, every other slot of the frame {0, 0, 0} — an empty record leaves the
 * combination of pnc_groupnorm_apply unchanged, so that kernel normalises a band with the statistics of the whole panorama.
 *    -> nn.GroupNorm over the (H, 6w) panorama when its views live on several ranks (diffusionmodules/util.py:276-283) */
int pnc_groupnorm_combine(const float* in, int parts, int F, int nchunk, float* out, void* stream);
/* Temporal GroupNorm(32,C)+SiLU: statistics over the (C/32, T) slab of ONE pixel, 1 <= T <= 16 (other T: PNC_EINVAL),
 * C % 64 == 0, C <= 2048
 *    -> nn.GroupNorm applied on "(b h w) c t" (openaimodel.py:409-419,509-515) */
int pnc_groupnorm_temporal_silu(const float* x, int B, int T, int Npix, int C,
                                const float* gamma, const float* beta, float eps,
                                void* y16, void* y16_lo, int lo_fmt, void* stream);
/* The same split over the ranks of a frame group (engine.FrameShard, round 4), for the T local frames of every pixel
 * (1 <= T <= 16 local frames; T_total >= T has no upper limit here — it only enters as the count n of the normalisation —
 * the product itself builds networks of at most 16 frames):
 *   mode 1: stats[((b*Npix + p)*32 + g)*2 + {0,1}] = {sum, sum of squares} over the (C/32, T) values this rank holds;
 *   mode 2: normalise + SiLU with `stats` = those sums added over the ranks and T_total = frames per sample over all ranks;
 *           t_pad = 1 writes y into the (T + 2)-frame layout PncGemmParams.t_halo reads (frame t at slot t + 1).
 *    -> the same nn.GroupNorm on "(b h w) c t" when the T frames of a pixel live on several ranks
 * The exchanged sums are raw moments (they have to add up over the ranks), so mode 2 forms var = E[x^2] - mean^2 in fp32: its
 * relative error grows as r^2 * 2^-24 times the growth of the accumulation, r = |mean| / std of a (pixel, group).  The frame-sharded
 * path inherits that law; pnc_groupnorm_temporal_silu (every frame local) subtracts the mean before it squares and does not. */
int pnc_groupnorm_temporal_part(const float* x, int B, int T, int Npix, int C,
                                const float* gamma, const float* beta, float eps,
                                float* stats, int mode, int T_total,
                                void* y16, void* y16_lo, int lo_fmt, int t_pad, void* stream);
/* LayerNorm over C (eps 1e-5) -> nn.LayerNorm (attention.py:699-701) */
int pnc_layernorm(const float* x, int ldx, int M, int C,
                  const float* gamma, const float* beta, float eps,
                  void* y16, int ldy, void* y16_lo, void* stream);

/* ------------------------------------------------------------------------- *
 * 4. Small helpers
 * ------------------------------------------------------------------------- */
/* out[m][n] = sum_k f(a[m][k]) * W[n][k] + bias[n], f = SiLU if silu_in; a fp32,
 * W fp16, M <= 16.  -> time_embed / emb_layers Linear (openaimodel.py:936-943,440-447) */
int pnc_linear_smallm(const float* a, int lda, const void* W, const float* bias,
                      float* out, int ldo, int M, int N, int K, int silu_in, int silu_out,
                      void* stream);
/* pnc_linear_smallm with SPLIT WEIGHTS: W_lo (fp16 [N][K], or NULL = pnc_linear_smallm bit for bit) is the lo plane of W as in
 * PncGemmParams.W_lo; the kernel joins w = W + 2^-11 W_lo in fp32 before the products (the activations are fp32 here) */
int pnc_linear_smallm_split(const float* a, int lda, const void* W, const void* W_lo, const float* bias,
                            float* out, int ldo, int M, int N, int K, int silu_in, int silu_out, void* stream);
/* The same linear for nseg sites in ONE launch (ABI 6): W [N][K] holds the sites' weight rows back to back, seg_start[0 .. nseg]
 * (HOST array, ascending, seg_start[0] = 0, seg_start[nseg] = N, every entry % 4 == 0, nseg <= PNC_SMALLM_MAX_SEGS) names each
 * site's column range, and the output is one contiguous [Mtot][width_s] block per site, blocks back to back:
 *     out[seg_start[s] * Mtot + (m0 + m) * width_s + (n - seg_start[s])],  m < M <= 16 rows of this call, m0 + M <= Mtot
 * — the [rows][N_site] row-bias operand each site's GEMM epilogue reads.  Per column bit-identical to pnc_linear_smallm.
 * -> the emb_layers Linear of every ResBlock of a network after one time_embed (openaimodel.py:440-447, 1296-1298) */
#define PNC_SMALLM_MAX_SEGS 64
int pnc_linear_smallm_segments(const float* a, int lda, const void* W, const float* bias, float* out, int M,
                               int m0, int Mtot, int N, int K, const int32_t* seg_start, int nseg, int silu_in,
                               int silu_out, void* stream);
/* ... and with split weights (W_lo as in pnc_linear_smallm_split; NULL = pnc_linear_smallm_segments bit for bit) */
int pnc_linear_smallm_segments_split(const float* a, int lda, const void* W, const void* W_lo, const float* bias, float* out,
                                     int M, int m0, int Mtot, int N, int K, const int32_t* seg_start, int nseg, int silu_in,
                                     int silu_out, void* stream);
/* sinusoidal timestep embedding out[f] = [cos(t*freqs) | sin(t*freqs)], fp32; freqs[dim/2] is
 * tabulated by the caller  (diffusionmodules/util.py:224-248) */
int pnc_timestep_embedding(const int64_t* t, int F, int dim, const float* freqs,
                           float* out, void* stream);
/* the same embedding from FLOAT timesteps: the c_noise of the continuous Denoiser (denoiser.py:6-28), of
 * DiscreteDenoiser(quantize_c_noise=False) (denoiser.py:59-63) and of EDMScaling (0.25 * log(sigma), denoiser_scaling.py:12),
 * which the reference's timestep_embedding takes as they are (util.py:224-248: `timesteps[:, None].float() * freqs[None]`).
 * Per element the arithmetic of pnc_timestep_embedding after its conversion float(t): bit-identical to it for integer-valued t. */
int pnc_timestep_embedding_f32(const float* t, int F, int dim, const float* freqs,
                               float* out, void* stream);
/* NCHW (fp32) -> channels-last fp16 with optional second source (channel concat) and zero padding to Cpad:
 *   out[f][p][c] = c<C1 ? a[f % a_frames][c][p]*a_scale[f] : c<C1+C2 ? b[f][c-C1][p] : 0
 * a_scale NULL = 1: the per-frame c_in of DiscreteDenoiser (denoiser.py:27-28) folded into the conversion; a_frames < F:
 * `a` holds the latent once and both CFG halves read it (torch.cat([x] * 2), guiders.py:36, without the copy)
 *    -> torch.cat in wrappers.py:41 + layout change */
int pnc_nchw_to_tokens_f16(const float* a, int C1, const float* a_scale, int a_frames, const float* b, int C2,
                           int F, int Npix, int Cpad, void* out16, void* out16_lo, void* stream);
/* Exit of one sampler step on the network's channels-last eps, one pass, reference rounding order:
 *   D_h    = eps_h * c_out + x                       DiscreteDenoiser + EpsScaling: c_out = -sigma snapped to the table,
 *                                                    c_skip = 1 (denoiser.py:22-28, denoiser_scaling.py:16-22)
 *   D      = D_u + scale * (D_c - D_u)               VanillaCFG (guiders.py:25-29); cfg = 0: D = D_c, one half only
 *   x_next = x + (sigma_next - sigma) * ((x - D) / sigma)      EulerEDMSampler.sampler_step (sampling.py:96-133)
 * eps_tok [(cfg ? 2 : 1) * T * Npix][ld] fp32, uncond frames first; x, x_next NCHW [T][C][Npix]; c_out, sigma, sigma_next [T].
 * This is the HEUN1 update of pnc_cfg_sampler_step below with v = {sigma, sigma_next}, out = x_next and no out_aux, and it runs as
 * exactly that: the same kernel, so the same bits as HEUN1's `out`. */
int pnc_cfg_euler_step(const float* eps_tok, int ld, int T, int Npix, int C, int cfg, float scale,
                       const float* x, const float* c_out, const float* sigma, const float* sigma_next, float* x_next,
                       void* stream);
/* Exit of one step of the other samplers of sampling.py (Heun, ancestral Euler, DPM++ 2S ancestral, DPM++ 2M, LMS), one pass:
 * denoised D is formed as in pnc_cfg_euler_step, then the sampler's update follows in the reference's rounding order (no FMA
 * contraction).  Per-frame scalars are [T] fp32 device vectors v[0..5] computed by the caller with the reference's torch ops;
 * x, x0, aux, hist[], noise, out, out_aux are NCHW [T][C][Npix] fp32 (out / out_aux may alias x0 / aux / hist[] element for
 * element: each element is read before it is written).  Per mode (x = the latent the network saw):
 *   HEUN1    v = {sigma_hat, next_sigma}             d = (x - D) / sigma_hat;  out = x + (next_sigma - sigma_hat) * d  (x_euler);
 *                                                    out_aux = d                                    (sampling.py:85-107)
 *   HEUN2    v = {sigma_hat, next_sigma}             x = x_euler, x0 = x_hat, aux = d:  d_new = (x - D) / next_sigma,
 *                                                    out = next_sigma > 0 ? x0 + ((aux + d_new) / 2) * (next_sigma - sigma_hat) : x
 *                                                                                                   (sampling.py:221-237)
 *   EULER_A  v = {sigma, sigma_down, sigma_up, next_sigma}   y = x + (sigma_down - sigma) * ((x - D) / sigma);
 *                                                    out = next_sigma > 0 ? y + noise * s_noise * sigma_up : y   (sampling.py:135-172,240-247)
 *   DPM2S_1  v = {sigma, sigma_down, mult1, mult2}   out = mult1 * x - mult2 * D  (x2);  out_aux = the ancestral Euler y (x_euler)
 *   DPM2S_2  v = {mult3, mult4, sigma_down, sigma_up, next_sigma}   x = x2, x0 = x, aux = x_euler:
 *                                                    y = sigma_down > 0 ? mult3 * x0 - mult4 * D : aux;  then the noise term of
 *                                                    EULER_A                                        (sampling.py:250-287)
 *   DPM2M    v = {mult1, mult2, mult3, mult4, next_sigma}   s = mult1 * x - mult2 * D;  aux = previous D or NULL (first / last
 *                                                    step: out = s);  otherwise out = next_sigma > 0 ? mult1 * x - mult2 *
 *                                                    (mult3 * D - mult4 * aux) : s;  out_aux = D   (sampling.py:290-365)
 *   LMS      v = {sigma, coeff_0 .. coeff_n_hist}    d = (x - D) / sigma;  out = x + (((0 + coeff_0 d) + coeff_1 hist[0]) + ...)
 *                                                    with hist[] the previous d newest first;  out_aux = d  (sampling.py:176-211)
 * Returns PNC_EABI when struct_bytes != sizeof(PncSamplerStepParams), PNC_EINVAL for a missing operand of the mode. */
enum {
    PNC_SAMPLER_HEUN1 = 0, PNC_SAMPLER_HEUN2 = 1, PNC_SAMPLER_EULER_A = 2, PNC_SAMPLER_DPM2S_1 = 3, PNC_SAMPLER_DPM2S_2 = 4,
    PNC_SAMPLER_DPM2M = 5, PNC_SAMPLER_LMS = 6
};
typedef struct PncSamplerStepParams {
    int32_t struct_bytes;   /* sizeof(PncSamplerStepParams) as the caller compiled it */
    int32_t mode;           /* PNC_SAMPLER_* */
    const float* eps_tok;   /* [(cfg ? 2 : 1) * T * Npix][ld], uncond frames first */
    int32_t ld, T, Npix, C;
    int32_t cfg;
    float scale;
    const float* x;
    const float* c_out;     /* [T] */
    const float* x0;
    const float* aux;
    const float* hist[4];
    int32_t n_hist;         /* LMS: 0..3 */
    float s_noise;
    const float* noise;
    const float* v[6];
    float* out;
    float* out_aux;
} PncSamplerStepParams;
int pnc_cfg_sampler_step(const PncSamplerStepParams* p, void* stream);
/* The two exit kernels with a general skip term, for the parameterisations whose c_skip is not 1 — VScaling (v-prediction) and
 * EDMScaling (denoiser_scaling.py:4-13, 25-31) under Denoiser / DiscreteDenoiser (denoiser.py:22-28):
 *   D_h = eps_h * c_out + x * c_skip                 two products, each rounded on its own, then the sum (denoiser.py:28)
 * c_skip [T] fp32 on the device; everything after D_h (CFG combine, the sampler's update, every operand and mode) is that of
 * pnc_cfg_euler_step / pnc_cfg_sampler_step.  All four entries run ONE kernel, compiled with and without the skip term, whose D
 * comes from one device function: c_skip = 1 gives the bits of the entries above (x * 1 is exact), and pnc_cfg_euler_step_skip is
 * HEUN1 of pnc_cfg_sampler_step_skip as pnc_cfg_euler_step is of pnc_cfg_sampler_step.  A NULL c_skip is
 * PNC_EINVAL (it is never read as 1: the eps path is the two entries above); PNC_EABI as pnc_cfg_sampler_step. */
int pnc_cfg_euler_step_skip(const float* eps_tok, int ld, int T, int Npix, int C, int cfg, float scale,
                            const float* x, const float* c_skip, const float* c_out, const float* sigma,
                            const float* sigma_next, float* x_next, void* stream);
int pnc_cfg_sampler_step_skip(const PncSamplerStepParams* p, const float* c_skip, void* stream);
/* Known frames put back at a noise level: the start of a schedule from a recorded clip and, after every step, the frames the
 * caller keeps (clip editing).  Additive under ABI 8.  z, noise, x, out NCHW [T][C][Npix] fp32 — the latent layout of the exit
 * entries above; sigma, keep [T] fp32 on the device.  For frame t
 *   keep[t] > 0   : out[t] = z[t] + noise[t] * sigma[t]     the product rounded to fp32, then the sum (no FMA contraction, as the
 *                                                           exits above); where sigma[t] == 0 out[t] is z[t] bit for bit and
 *                                                           noise[t] is not read (NaN noise is inert there)
 *   otherwise     : out[t] = x[t] bit for bit               keep[t] 0.0, -0.0, negative or NaN; with out == x the frame is not
 *                                                           touched at all
 * keep == NULL keeps every frame; x may be NULL only then.  out may alias x element for element, never z or noise.  A frame's
 * C * Npix floats are one contiguous run: it moves in 16-byte loads and stores between the 16-byte boundaries of out[t] when
 * z[t] (x[t]) and noise[t] sit at out[t]'s offset from a boundary, with up to three single elements either side, and element
 * by element otherwise; Npix need not be a multiple of 4.  Checked in this order, nothing is launched on a refusal:
 *   PNC_EINVAL  a NULL z, noise, sigma or out (the selector lives on the device: the host never knows that nothing is kept), a
 *               keep without x, T < 1, C < 1, Npix < 1, C * Npix > 2^40, T * ceil(C * Npix / 1024) >= 2^31;
 *   PNC_EALIGN  any pointer not 4-byte aligned.
 *    -> the noising `input + noise * append_dims(sigmas, input.ndim)` (sgm/modules/diffusionmodules/loss.py:61), which is also the
 *       point a deterministic Euler step (sampling.py:96-133) reaches from z + noise * sigma when the denoised frame is z; the
 *       reference has no sampling entry that starts from a clip */
int pnc_frames_renoise(const float* z, const float* noise, const float* sigma, const float* keep, const float* x, float* out,
                       int T, int C, int64_t Npix, void* stream);
/* channels-last fp32 [F*Npix][ld] -> NCHW fp32 (first C columns) */
int pnc_tokens_to_nchw_f32(const float* x, int ld, int F, int Npix, int C,
                           float* out, void* stream);
/* out32[m][0:C1] = a[m][:], out32[m][C1:C1+C2] = s[m][:] + c[m][:]; optional fp16 copy
 *    -> th.cat([h, hs.pop() + control.pop()], dim=1)  (controlmodel.py:193-195) */
int pnc_concat_add(const float* a, int C1, const float* s, const float* c, int C2,
                   int64_t M, float* out32, void* out16, void* out16_lo, int lo_fmt, void* stream);
/* the same concatenation over F frames of Npix pixels (M = F * Npix rows) that ALSO writes the GroupNorm(32) statistics of its output —
 * records {n, mean, M2} [F][ceil(Npix / pix_per_chunk)][32][3] as pnc_groupnorm_stats(..., pix_per_chunk, ...) would, for
 * pnc_groupnorm_apply(..., n_records = ceil(Npix / pix_per_chunk)): the first GroupNorm of the ResBlock3D that follows the concat
 * (openaimodel.py:1311-1314 -> 499-503) then needs no statistics launch.  (C1 + C2) % 64 == 0.  Deterministic (no float atomics).
 * ABI 5 (round 5). */
int pnc_concat_add_stats(const float* a, int C1, const float* s, const float* c, int C2, int F, int Npix, int pix_per_chunk,
                         float* out32, void* out16, void* out16_lo, int lo_fmt, float* partial, void* stream);
/* y = x + a (fp32, may be in place); optional fp16 copy of y
 *    -> h += guided_hint / h += control.pop()  (controlmodel.py:127,192) */
int pnc_add_f32(const float* x, const float* a, int64_t n, float* y32, void* y16, void* y16_lo, int lo_fmt,
                void* stream);
/* fp32 -> fp16 (+ lo plane in lo_fmt) */
int pnc_cast_f16(const float* x, int64_t n, void* y16, void* y16_lo, int lo_fmt, void* stream);
/* Second half of a nearest-x2 Upsample conv computed at SOURCE resolution (openaimodel.py:106-142).  P holds, per
 * source pixel (row (f * Hin + sy) * Win + sx, ldp floats between rows), the nine tap products of the 3x3 conv: column
 * (u * 3 + v) * Cout + n = sum_k x[src][k] * W[n][k][u][v] (a plain-A GEMM against the weight as [9 * Cout][Cin]).  For output pixel
 * (y, x) of the [F][2 Hin][2 Win][Cout] map
 *     acc = bias[n];  for u = 0..2, v = 0..2 in this order:  yy = y + u - 1, xx = x + v - 1;
 *                     if 0 <= yy < 2 Hin and 0 <= xx < 2 Win:  acc += P[(f, yy >> 1, xx >> 1)][(u * 3 + v) * Cout + n]
 * Taps outside the upsampled image are the conv's zero padding and are not read.  The order of the additions is the one written, so
 * the result does not depend on the launch geometry.  out32 receives acc; out16 / out16_lo (optional; a lo plane needs out16) its
 * fp16 plane and lo plane in lo_fmt (PNC_LO_*), packed like every other writer of the `stream` class (range monitor included).
 * bias may be NULL (0).  Cout % 4 == 0, ldp % 4 == 0, ldp >= 9 * Cout (PNC_EINVAL); P, bias, out32, out16, out16_lo 16-byte aligned
 * (PNC_EALIGN); both are answered before any launch.  Additive to ABI 8. */
int pnc_upsample_combine(const float* P, int64_t ldp, const float* bias, int F, int Hin, int Win, int Cout, float* out32,
                         void* out16, void* out16_lo, int lo_fmt, void* stream);

/* Range monitor (round 6; ABI 7).  The eps contract of the `precise` operand policy is written for a residual stream inside the e4m3
 * lo plane's range (|v| < 512: beyond it the lo plane of a split operand saturates at +-448 and the operand falls back to fp16's 11
 * bits — UNetModel3D.eps_contract; the reference has no counterpart: its fp32 CPU path has no such range and its
 * autocast fp16 path overflows at 65504 without notice, sgm/modules/diffusionmodules/wrappers.py:37-70).  Every kernel that packs an
 * e4m3 lo plane counts the packed quads that clamped; this call ADDS the counts since the previous call to *out (a device word the
 * caller zeroes) on `stream` and resets them — a handful of one-thread launches, once per network evaluation.  0 = the evaluation
 * stayed inside the range its contract is written for.
 * UNIT.  (count > 0) == (a packed residual was beyond +-448) is the contract; the number itself is in the unit of the writer.  The
 * vector writers — the helpers, every fast GEMM epilogue and the split-K reduce — pack ALIGNED QUADS (columns 4 q .. 4 q + 3 of a row)
 * and count a quad once, however many of its four residuals clamp.  The generic GEMM epilogue (N % 8 != 0, leading dimensions or
 * pointers outside the vector contract, option sets without a specialised variant such as GELU next to out32) packs one element per
 * call and counts clamped ELEMENTS.  tests/test_gemm_range_gpu.py holds both, from the launch's own out32. */
int pnc_range_monitor_collect(unsigned int* out, void* stream);

/* Range profile of ONE contraction operand (a diagnostic pass: UNetModel3D.profile_ranges; the denoising path never launches it).
 * Where the monitor above answers "did a lo plane clamp, anywhere", this states where an operand sits in fp16's range.
 *   hi  : fp16 plane, `rows` rows of `cols` elements, `ld` elements between rows
 *   lo  : NULL, or the lo plane of the operand in lo_fmt (PNC_LO_*), same ld IN ELEMENTS
 * Elements at column positions cols .. ld - 1 of a row are padding and are never read.
 * rec : PNC_STATS_WORDS 64-bit words on the device.  The kernel ADDS to them (atomic add; atomic max for word 32), so one record sums
 *       any number of launches on any streams without a host synchronisation; the caller zeroes it.
 *   rec[0..31]  elements per fp16 binade: index = exponent field (bits >> 10) & 31 of hi.  Bin 0: zeros and subnormals; bin 31: Inf
 *               and NaN; |v| >= 512 — where an e4m3 lo plane clamps — is bins 24..31
 *   rec[32]     maximum of (bits & 0x7FFF) over the elements: NaN > Inf > every finite value, so a NaN cannot hide
 *   rec[33]     lo elements at the END of their format: e4m3 (byte & 0x7F) >= 0x7E (+-448 and the NaN code), fp16 non-finite; an
 *               upper bound of the elements that clamped (a residual of exactly 448 counts, too).  lo = NULL adds nothing
 *   rec[34]     NaN elements of hi
 *   rec[35]     elements counted (rows * cols)
 * Checked before any launch: NULL hi / rec, rows < 1, cols < 1, ld < cols, lo != NULL with an unknown lo_fmt, a plane of more than
 * 2^43 elements (a wave of the kernel counts in 32 bits before it widens) -> PNC_EINVAL;
 * cols % 8, ld % 8, hi not 16-byte aligned, lo not aligned to 8 elements of its format, rec not 8-byte aligned -> PNC_EALIGN. */
#define PNC_STATS_WORDS 36
int pnc_operand_stats_f16(const void* hi, const void* lo, int lo_fmt, int64_t rows, int cols, int64_t ld,
                          unsigned long long* rec, void* stream);

/* ------------------------------------------------------------------------- *
 * 5. First-stage decoder: row softmax of a materialised score
 *    matrix, p[m][:] = softmax(scale * s[m][:]) (fp32 in, fp32 statistics, fp16
 *    out), N % 4 == 0.  A row is kept in registers: N <= 16384 is THIS kernel's limit, not the attention block's (section 6
 *    serves longer frames).  Columns >= n_valid (n_valid <= 0: N) are masked; causal != 0 also masks columns
 *    j > m (row m = query m of ONE sequence: the OpenCLIP text tower's attn_mask, sgm/modules/encoders/modules.py:608).
 *    The masks are predicates, for every scale >= 0 (0 and denormal-small ones included: the visible columns are then uniform): a
 *    masked column receives +0 and takes no part in the row sum; its score may hold anything, NaN and +-Inf included, and does not
 *    influence the output by one bit.  Every column j < N of every row m < M of p is written (a row m >= N under a causal mask sees
 *    all n_valid columns); columns N .. lds - 1 of s are never read, columns N .. ldp - 1 of p never written.  For frames
 *    of up to 16384 tokens the single-head d = 512 attention of the VAE
 *    mid block runs as  S = Q K^T (pnc_gemm_f16, fp32 out) -> this -> O = P V
 *    (pnc_gemm_f16 against the channel-major V^T).
 *     -> AttnBlock / MemoryEfficientAttnBlock.attention
 *        (sgm/modules/diffusionmodules/model.py:393-408, 444-472)
 * ------------------------------------------------------------------------- */
int pnc_softmax_rows_f16(const float* s, int64_t lds, int M, int N, float scale, int causal, int n_valid,
                         void* p16, int64_t ldp, void* stream);

/* ------------------------------------------------------------------------- *
 * 6. First-stage attention, fused: single-head self-attention over the N tokens of each of F frames, head dim C, with an
 *    online softmax — no N x N matrix, no workspace, ONE launch for all frames, any N.
 *        o = softmax(scale * q k^T) v      per frame, fp16 in / out
 *    q, k, o : fp16 token rows; the row of (frame f, token i) is f*N + i, element c at [(f*N + i)*ld + c], c < C
 *    vt      : V channel-major per frame ("V^T"): vt[f*vt_fstride + c*ldvt + j] for key j < N, c < C
 *    Every token of a frame attends to all N tokens of the same frame and to nothing else.  Scores are accumulated in fp32, the
 *    running maximum, the row sum and the output accumulators are fp32; probabilities are rounded to fp16 against the running
 *    maximum before the P V product (as section 2 does) and the result is normalised once at the end.
 *    ONLY the named elements are read or written: row padding between C and ld, V^T columns between N and ldvt and rows after
 *    the last frame may hold anything (NaN included) and a buffer may end right after its last named element; o's padding is
 *    left as it was.  Deterministic: no atomics, the same bits on every run.  o must not overlap q, k or vt.
 *    Accepted: C in {128, 256, 512}; F >= 1; N >= 8, N % 8 == 0; F * ceil(N / 64) < 2^31; ldq, ldk, ldo >= C, ldvt >= N,
 *    vt_fstride >= 0; anything else -> PNC_EINVAL.  ldq, ldk, ldo, ldvt, vt_fstride multiples of 8 elements and q, k, vt, o
 *    16-byte aligned, else PNC_EALIGN.  Checked in this order: null pointers, ranges, leading dimensions, pointer alignment;
 *    nothing is launched on a refusal.
 *     -> AttnBlock / MemoryEfficientAttnBlock.attention
 *        (sgm/modules/diffusionmodules/model.py:393-408, 444-472)
 * ------------------------------------------------------------------------- */
int pnc_attn_frame_f16(const void* q, int64_t ldq, const void* k, int64_t ldk,
                       const void* vt, int64_t ldvt, int64_t vt_fstride,
                       void* o, int64_t ldo, int F, int N, int C, float scale, void* stream);

/* ------------------------------------------------------------------------- *
 * 6b. First-stage attention on SPLIT operands: the geometry of section 6 (F frames of N tokens, one head of dim C, one launch, online
 *    softmax, no N x N matrix, no workspace) on the operands of the split attention kernels of section 2.  Additive under ABI 8.
 *    Every operand x is an fp16 pair x = x_hi + 2^-11 x_lo (PncGemmParams.A_lo):
 *        S = Qh.Kh + 2^-11 (Qh.Kl + Ql.Kh)                   the lo.lo products are dropped; fp32 accumulation
 *        P = softmax(scale * S) per row, online;  P = Ph + 2^-11 Pl, an fp16 pair rounded against the running maximum
 *        O = Ph.Vh + 2^-11 (Ph.Vl + Pl.Vh)                   normalised once at the end, written as o = fp16(O), o_lo = fp16((O - o) * 2^11)
 *    q, k, v, o : fp16 token rows, hi planes; the row of (frame f, token i) is f*N + i, element c at [(f*N + i)*ld + c], c < C
 *    q_lo .. o_lo : the lo planes, each with the layout and the leading dimension of its hi plane
 *    V is ROW-major, laid out like K — what a QKV projection writes as out16 + out16_lo (the transposed out16t store of the GEMM has
 *    no lo plane); the kernel transposes on its way to the MFMA.
 *    Every token of a frame attends to all N tokens of the same frame and to nothing else.  The hi.hi and the cross products are
 *    accumulated apart in fp32 and meet once, scaled by 2^-11; the running maximum and the row sum are fp32.
 *    ONLY the named elements are read or written: row padding between C and ld (of either plane) and rows after the last frame may
 *    hold anything (NaN included) and a buffer may end right after its last named element; the padding of o and o_lo is left as it
 *    was.  Keys >= N of the last key tile are never loaded and are masked after the partial scores are added.  Deterministic: no
 *    atomics, the same bits on every run.  o and o_lo must not overlap each other or any input.
 *    Accepted: C in {128, 256, 512}; F >= 1; N >= 8, N % 8 == 0; F * ceil(N / 32) < 2^31; ldq, ldk, ldv, ldo >= C; anything else ->
 *    PNC_EINVAL.  ldq, ldk, ldv, ldo multiples of 8 elements and all eight pointers 16-byte aligned, else PNC_EALIGN.  Checked in
 *    this order: null pointers, ranges, leading dimensions, pointer alignment; nothing is launched on a refusal.
 *     -> AttnBlock / MemoryEfficientAttnBlock.attention under the first stage's split policies
 *        (sgm/modules/diffusionmodules/model.py:393-408, 444-472)
 * ------------------------------------------------------------------------- */
int pnc_attn_frame_split_f16(const void* q, const void* q_lo, int64_t ldq, const void* k, const void* k_lo, int64_t ldk,
                             const void* v, const void* v_lo, int64_t ldv, void* o, void* o_lo, int64_t ldo,
                             int F, int N, int C, float scale, void* stream);

/* ------------------------------------------------------------------------- *
 * 6c. Text-tower attention on SPLIT operands: the causal self-attention of the OpenCLIP text tower, all heads of all prompts in one
 *    launch, on the operands and with the formulae of section 6b.  Additive under ABI 8.
 *    A prompt is a group of Lp token rows; the row of (prompt g, token i) is g*Lp + i; head h takes columns 64h .. 64h+63 (head
 *    dim 64); element c of head h of that row is at [(g*Lp + i)*ld + 64h + c], c < 64.
 *    Every operand x is an fp16 pair x = x_hi + 2^-11 x_lo; q_lo .. o_lo have the layout and the leading dimension of their hi plane.
 *    V is ROW-major like K — what a QKV projection writes as out16 + out16_lo with N = 3 W and no out16t; q, k and v may be column
 *    blocks of that one buffer (ld = 3 W).
 *        S = Qh.Kh + 2^-11 (Qh.Kl + Ql.Kh)                   the lo.lo products are dropped; fp32 accumulation, the hi.hi and the
 *                                                            cross sums kept apart and met once
 *        query i attends key j  iff  j <= i  and  j < kv_valid
 *        P = softmax(scale * S) over the attended keys;  P = Ph + 2^-11 Pl, an fp16 pair rounded against the row's maximum (two
 *                                                            passes over the row: no running maximum, no rescale)
 *        O = Ph.Vh + 2^-11 (Ph.Vl + Pl.Vh)                   normalised once, written as o = fp16(O), o_lo = fp16((O - o) * 2^11)
 *    Query rows kv_valid <= i < Lp are padding: they attend all keys < kv_valid and ARE written (finite when their q row is finite);
 *    the caller drops them.  Key and value rows >= kv_valid may hold anything, NaN included: they are never loaded.
 *    ONLY the named elements are read or written: row padding between 64*heads and ld and rows after groups*Lp keep their bits, and
 *    a buffer may end right after its last named element.  Deterministic: no atomics, the same bits on every run.  o and o_lo must
 *    not overlap each other or any input.
 *    Accepted: groups >= 1; heads >= 1; groups*heads < 2^31; Lp % 8 == 0, 8 <= Lp <= 96; 1 <= kv_valid <= Lp; ldq, ldk, ldv, ldo >=
 *    64*heads; anything else -> PNC_EINVAL.  ldq, ldk, ldv, ldo multiples of 8 elements and all eight pointers 16-byte aligned, else
 *    PNC_EALIGN.  Checked in this order: null pointers, ranges, leading dimensions, pointer alignment; nothing is launched on a
 *    refusal.
 *     -> FrozenOpenCLIPEmbedder.encode_with_transformer / text_transformer_forward under the tower's split policies: the attention
 *        of every residual block (sgm/modules/encoders/modules.py:604-616)
 * ------------------------------------------------------------------------- */
int pnc_attn_text_split_f16(const void* q, const void* q_lo, int64_t ldq, const void* k, const void* k_lo, int64_t ldk,
                            const void* v, const void* v_lo, int64_t ldv, void* o, void* o_lo, int64_t ldo,
                            int groups, int heads, int Lp, int kv_valid, float scale, void* stream);

/* ------------------------------------------------------------------------- *
 * 7. Image boundary: 8-bit channels-last frames in and out.  Additive under ABI 8.  Both entries
 *    launch on the caller's stream, allocate nothing and do not synchronise; nothing is launched on a refusal.
 *
 *    pnc_u8_to_tokens_f16: uint8 [F][Npix][C] (contiguous, at ANY byte address) -> fp16 tokens [F*Npix][Cpad] through a table
 *        v = lut[src[f][p][c]]         lut: 256 fp32 values on the device
 *        c <  C        : out16 = (half)v,  out16_lo = (half)((v - (float)out16) * 2^11)      (out16_lo may be NULL)
 *        C <= c < Cpad : out16 = out16_lo = +0
 *    which is what pnc_nchw_to_tokens_f16 writes for a float input that holds v.  The table carries the scaling: the reference
 *    scales on the host with IEEE fp32 divisions (`source.astype(np.float32) / 255.0` for the 19-channel BEV layout,
 *    `target.astype(np.float32) / 127.5 - 1.0` for the frames; sgm/data/nuscenes_video/nuscenes_datasets_video.py:542-552), and a
 *    table built with those very expressions over the 256 bytes reproduces them bit for bit; the kernel has no arithmetic of its own.
 *    Only the F*Npix*C bytes of src are read: aligned vector loads never reach outside [src, src + F*Npix*C).
 *    PNC_EINVAL: a null src / lut / out16, F < 1, Npix < 1, C < 1, C > 4096, Cpad % 8 != 0, Cpad < C.  PNC_EALIGN: out16 or
 *    out16_lo not 16-byte aligned.
 *
 *    pnc_tokens_to_u8: fp32 tokens, M rows of C <= 8 columns with row stride ld >= C -> uint8 [M][C] (contiguous)
 *        t = fminf(fmaxf(x, -1), 1);  t = (t + 1.0f) * 0.5f;  t = t * 255.0f;  out = (uint8)(int)t
 *    every operation rounded on its own, in this order (no FMA contraction); (t + 1) * 0.5f has the bits of (t + 1) / 2.  NaN -> 0
 *    (a choice: the reference's numpy cast of NaN is undefined).  The decoder's last conv writes [F*H*W][3] tokens, which already
 *    are H x W x 3 frames: this is `torch.clamp(x, -1, 1); (x + 1) / 2; (x * 255).astype(np.uint8)` of inference.py:189-193
 *    without the transposes to planes and back.  Exactly M * C bytes are written.
 *    PNC_EINVAL: a null pointer, M < 1, C < 1, C > 8, ld < C.  PNC_EALIGN: x or out not 4-byte aligned.
 * ------------------------------------------------------------------------- */
int pnc_u8_to_tokens_f16(const uint8_t* src, const float* lut, int F, int Npix, int C, int Cpad,
                         void* out16, void* out16_lo, void* stream);
int pnc_tokens_to_u8(const float* x, int ld, int64_t M, int C, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------- *
 * 8. Region editing: camera views and pixel regions of a recorded clip kept instead of whole frames (pnc_frames_renoise with the
 *    selector per pixel, and the two byte kernels around it).  Additive under ABI 8.  All three entries launch 256-thread
 *    workgroups on the caller's stream, allocate nothing and do not synchronise; every store is an ordinary vector store; nothing
 *    is launched on a refusal, and PNC_EINVAL is checked before PNC_EALIGN.  The reference has no counterpart: it has no sampling
 *    entry that starts from a clip (see pnc_frames_renoise).
 *
 *    pnc_latent_renoise_masked: z, noise, x, out contiguous fp32 [T][C][Npix] (the latent layout of pnc_frames_renoise), sigma [T]
 *    fp32, mask [T][Npix] fp32, all on the device; row t of the mask serves each of the C planes of frame t.  Element (t, c, p) is
 *    KEPT iff mask[t][p] > 0 — 0.0, -0.0, negative and NaN do not keep, the rule of pnc_frames_renoise's keep[t]:
 *        kept, sigma[t] == 0 (either sign) : out = z bit for bit, the noise is not read
 *        kept, otherwise                   : out = z + (noise * sigma[t])      the product rounded to fp32 on its own, then the sum
 *                                                                               (no FMA contraction, as pnc_frames_renoise)
 *        not kept                          : out = x bit for bit
 *    A select, never an arithmetic blend: the operand that is not selected is inert — NaN in noise or z at elements that are not
 *    kept, NaN noise in frames with sigma 0 and NaN x at kept elements leave no trace in out.  out may be x (every element is
 *    read before it is written, and only by the thread that writes it), never z, noise or mask.  mask and x are both required:
 *    the launch that keeps everything without them is pnc_frames_renoise.  A plane moves in 16-byte loads and stores between the
 *    16-byte boundaries of its run in out when its runs in z, noise and x sit at the same offset from a boundary, with up to three
 *    single elements either side, and element by element otherwise; every 4-byte alignment and every Npix works (with
 *    Npix % 4 != 0 the planes of a frame start at different offsets, and the mask index starts again at 0 in every plane).
 *      PNC_EINVAL  a NULL z, noise, sigma, mask, x or out, T < 1, C < 1, Npix < 1, C * Npix > 2^40,
 *                  T * C * ceil(Npix / 1024) >= 2^31;
 *      PNC_EALIGN  any pointer not 4-byte aligned.
 *
 *    pnc_mask_pool_u8: a pixel mask uint8 [T][H][W] (contiguous, at ANY byte address; nonzero = this pixel is kept) -> the latent
 *    selector fp32 [T][H/f][W/f]:
 *        out[t][y][x] = 1.0f iff EVERY one of the f x f bytes mask_u8[t][y*f .. y*f+f-1][x*f .. x*f+f-1] is nonzero, else 0.0f
 *    so a latent cell that the first stage computed partly from pixels that will be regenerated never counts as known.
 *      PNC_EINVAL  a NULL pointer, T < 1, H < 1, W < 1, f < 1, f > 16, H % f != 0, W % f != 0, T * (H/f) * (W/f) > 2^38;
 *      PNC_EALIGN  out not 4-byte aligned.
 *
 *    pnc_u8_select: src, gen, out uint8 [npix][C] (contiguous, at ANY byte address), mask_u8 uint8 [npix], 1 <= C <= 4:
 *        out[p][c] = mask_u8[p] != 0 ? src[p][c] : gen[p][c]          the mask is per PIXEL: all C bytes of a pixel go together
 *    out may be gen (bytes are read before they are written, by the thread that writes them); out == src is refused.  Exactly
 *    npix * C bytes are written.
 *      PNC_EINVAL  a NULL pointer, npix < 1, npix > 2^40, C < 1, C > 4, out == src.
 * ------------------------------------------------------------------------- */
int pnc_latent_renoise_masked(const float* z, const float* noise, const float* sigma, const float* mask, const float* x, float* out,
                              int T, int C, int64_t Npix, void* stream);
int pnc_mask_pool_u8(const uint8_t* mask_u8, float* out, int T, int H, int W, int f, void* stream);
int pnc_u8_select(const uint8_t* src, const uint8_t* gen, const uint8_t* mask_u8, uint8_t* out, int64_t npix, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PANACEA_HIP_H */
