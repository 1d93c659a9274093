// misc.hip — small HBM-bound helpers of the denoising path: time-embedding MLP (small-M fp32
// linear), sinusoidal embedding, NCHW <-> channels-last conversion, skip/control concat-add.
#include "common.h"
#include <atomic>

namespace {

constexpr int SM_MAXM = 16;

// one wave per output column n: out[m][n] = sum_k f(a[m][k]) W[n][k] + bias[n]
__global__ __launch_bounds__(256) void linear_smallm_kernel(const float* __restrict__ a, int lda,
                                                            const half_t* __restrict__ W,
                                                            const half_t* __restrict__ W_lo,
                                                            const float* __restrict__ bias,
                                                            float* __restrict__ out, int ldo, int M, int N,
                                                            int K, int silu_in, int silu_out) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float acc[SM_MAXM];
#pragma unroll
    for (int m = 0; m < SM_MAXM; ++m) acc[m] = 0.0f;
    for (int k0 = lane * 8; k0 < K; k0 += 64 * 8) {
        const half8v w = *reinterpret_cast<const half8v*>(W + (int64_t)n * K + k0);
        float wf[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) wf[e] = (float)w[e];
        if (W_lo) {             // (uniform) split weights: W = W_hi + 2^-11 W_lo, joined in fp32 (the activations are fp32 here)
            const half8v wl = *reinterpret_cast<const half8v*>(W_lo + (int64_t)n * K + k0);
#pragma unroll
            for (int e = 0; e < 8; ++e) wf[e] = fmaf((float)wl[e], 1.0f / 2048.0f, wf[e]);
        }
#pragma unroll
        for (int m = 0; m < SM_MAXM; ++m) {
            if (m < M) {
                const f32x4 x0 = *reinterpret_cast<const f32x4*>(a + (int64_t)m * lda + k0);
                const f32x4 x1 = *reinterpret_cast<const f32x4*>(a + (int64_t)m * lda + k0 + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float u0 = silu_in ? silu_f(x0[e]) : x0[e];
                    const float u1 = silu_in ? silu_f(x1[e]) : x1[e];
                    acc[m] = fmaf(u0, wf[e], acc[m]);
                    acc[m] = fmaf(u1, wf[e + 4], acc[m]);
                }
            }
        }
    }
    const float b = bias ? bias[n] : 0.0f;
#pragma unroll
    for (int m = 0; m < SM_MAXM; ++m) {
        if (m < M) {
            float v = wave_sum(acc[m]) + b;
            if (silu_out) v = silu_f(v);
            if (lane == 0) out[(int64_t)m * ldo + n] = v;
        }
    }
}

// The same linear for MANY sites in one launch (round 5): W holds the sites' weight rows back to back (N = sum of the sites'
// widths), the output is laid out one contiguous [Mtot x width] block per site (segment), blocks back to back — what each site's
// consumer (the row-bias operand of its GEMM epilogue: [rows][N_site]) reads.  One wave per SEG_NC consecutive columns: the 16 x K
// activation rows are read once per wave instead of once per column.  Per column the K order, the fma chain and the wave
// reduction are those of linear_smallm_kernel: bit-identical to one launch per site.
constexpr int SEG_NC = 4;
struct SmallmSegs {
    int nseg;
    int start[PNC_SMALLM_MAX_SEGS + 1];
};

__global__ __launch_bounds__(256) void linear_smallm_seg_kernel(const float* __restrict__ a, int lda,
                                                                const half_t* __restrict__ W,
                                                                const half_t* __restrict__ W_lo,
                                                                const float* __restrict__ bias,
                                                                float* __restrict__ out, int M, int m0, int Mtot, int N,
                                                                int K, int silu_in, int silu_out, SmallmSegs segs) {
    const int lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * SEG_NC;
    if (n0 >= N) return;
    float acc[SEG_NC][SM_MAXM];
#pragma unroll
    for (int c = 0; c < SEG_NC; ++c)
#pragma unroll
        for (int m = 0; m < SM_MAXM; ++m) acc[c][m] = 0.0f;
    for (int k0 = lane * 8; k0 < K; k0 += 64 * 8) {
        float wf[SEG_NC][8];
#pragma unroll
        for (int c = 0; c < SEG_NC; ++c) {
            const half8v w = *reinterpret_cast<const half8v*>(W + (int64_t)(n0 + c) * K + k0);
#pragma unroll
            for (int e = 0; e < 8; ++e) wf[c][e] = (float)w[e];
            if (W_lo) {         // (uniform) split weights, as in linear_smallm_kernel
                const half8v wl = *reinterpret_cast<const half8v*>(W_lo + (int64_t)(n0 + c) * K + k0);
#pragma unroll
                for (int e = 0; e < 8; ++e) wf[c][e] = fmaf((float)wl[e], 1.0f / 2048.0f, wf[c][e]);
            }
        }
#pragma unroll
        for (int m = 0; m < SM_MAXM; ++m) {
            if (m < M) {
                const f32x4 x0 = *reinterpret_cast<const f32x4*>(a + (int64_t)m * lda + k0);
                const f32x4 x1 = *reinterpret_cast<const f32x4*>(a + (int64_t)m * lda + k0 + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float u0 = silu_in ? silu_f(x0[e]) : x0[e];
                    const float u1 = silu_in ? silu_f(x1[e]) : x1[e];
#pragma unroll
                    for (int c = 0; c < SEG_NC; ++c) {
                        acc[c][m] = fmaf(u0, wf[c][e], acc[c][m]);
                        acc[c][m] = fmaf(u1, wf[c][e + 4], acc[c][m]);
                    }
                }
            }
        }
    }
    int s = 0;                                              // wave-uniform: a wave's columns lie in one segment (widths % SEG_NC == 0)
    while (s + 1 < segs.nseg && n0 >= segs.start[s + 1]) ++s;
    const int s0 = segs.start[s], len = segs.start[s + 1] - s0;
    float* o = out + (int64_t)s0 * Mtot + (int64_t)m0 * len + (n0 - s0);
#pragma unroll
    for (int c = 0; c < SEG_NC; ++c) {
        const float b = bias ? bias[n0 + c] : 0.0f;
#pragma unroll
        for (int m = 0; m < SM_MAXM; ++m) {
            if (m < M) {
                float v = wave_sum(acc[c][m]) + b;
                if (silu_out) v = silu_f(v);
                if (lane == 0) o[(int64_t)m * len + c] = v;
            }
        }
    }
}

// TS = int64_t (table indices: quantised c_noise) or float (a continuous c_noise: Denoiser, quantize_c_noise = False): the same
// arithmetic after the conversion float(t), so integer-valued float timesteps give the int64 kernel's bits
template <typename TS>
__global__ void timestep_embedding_kernel(const TS* __restrict__ t, int F, int dim,
                                          const float* __restrict__ freqs, float* __restrict__ out) {
    const int half = dim / 2;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F * half) return;
    const int f = i / half, j = i - f * half;
    // freqs[j] = exp(-ln(max_period) * j / half) is tabulated by the host exactly as
    // diffusionmodules/util.py:236-241 does (fp32), so only cos/sin run here.
    const float arg = (float)t[f] * freqs[j];
    out[(int64_t)f * dim + j] = cosf(arg);
    out[(int64_t)f * dim + half + j] = sinf(arg);
    if ((dim & 1) && j == 0) out[(int64_t)f * dim + dim - 1] = 0.0f;
}

// thread per (f, pixel): gather channels (stride Npix), write Cpad fp16 contiguous
__global__ __launch_bounds__(256) void nchw_to_tokens_kernel(const float* __restrict__ a, int C1,
                                                             const float* __restrict__ a_scale, int a_frames,
                                                             const float* __restrict__ b, int C2, int F,
                                                             int Npix, int Cpad, half_t* __restrict__ out,
                                                             half_t* __restrict__ out_lo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)F * Npix) return;
    const int64_t f = i / Npix, pix = i - f * Npix;
    const int64_t fa = f % a_frames;                 // CFG batch doubling: both halves read the same latent
    const float sa = a_scale ? a_scale[f] : 1.0f;
    half_t* o = out + i * Cpad;
    for (int c0 = 0; c0 < Cpad; c0 += 8) {
        half8v h, l;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = c0 + e;
            float v = 0.0f;
            if (c < C1) v = a[(fa * C1 + c) * Npix + pix] * sa;
            else if (c < C1 + C2) v = b[(f * C2 + (c - C1)) * Npix + pix];
            h[e] = (half_t)v;
            l[e] = (half_t)((v - (float)h[e]) * PNC_LO_SCALE);
        }
        *reinterpret_cast<half8v*>(o + c0) = h;
        if (out_lo) *reinterpret_cast<half8v*>(out_lo + i * Cpad + c0) = l;
    }
}

__global__ __launch_bounds__(256) void tokens_to_nchw_kernel(const float* __restrict__ x, int ld, int F,
                                                             int Npix, int C, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)F * Npix) return;
    const int64_t f = i / Npix, pix = i - f * Npix;
    for (int c = 0; c < C; ++c) out[(f * C + c) * Npix + pix] = x[i * ld + c];
}

// float4 granularity over the concatenated row
__global__ __launch_bounds__(256) void concat_add_kernel(const float* __restrict__ a, int C1,
                                                         const float* __restrict__ s,
                                                         const float* __restrict__ c, int C2, int64_t M,
                                                         float* __restrict__ out32, half_t* __restrict__ out16,
                                                         void* __restrict__ out16_lo, int lo_fmt) {
    const int CT = C1 + C2, V = CT >> 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * V) return;
    const int64_t m = i / V;
    const int ch = (int)(i - m * V) * 4;
    f32x4 v;
    if (ch < C1) {
        v = *reinterpret_cast<const f32x4*>(a + m * C1 + ch);
    } else {
        const int c2 = ch - C1;
        v = *reinterpret_cast<const f32x4*>(s + m * C2 + c2);
        if (c) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(c + m * C2 + c2);
            v += w;
        }
    }
    if (out32) *reinterpret_cast<f32x4*>(out32 + m * CT + ch) = v;
    if (out16) {
        half4v h = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
        *reinterpret_cast<half4v*>(out16 + m * CT + ch) = h;
        if (out16_lo) {
            const float o[4] = {v[0], v[1], v[2], v[3]};
            store_lo4(out16_lo, lo_fmt, m * CT + ch, o, h);
        }
    }
}

__global__ __launch_bounds__(256) void add_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                  int64_t n4, float* __restrict__ y32, half_t* __restrict__ y16,
                                                  void* __restrict__ y16_lo, int lo_fmt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
    if (a) { const f32x4 w = *reinterpret_cast<const f32x4*>(a + i * 4); v += w; }
    if (y32) *reinterpret_cast<f32x4*>(y32 + i * 4) = v;
    if (y16) {
        half4v h = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
        *reinterpret_cast<half4v*>(y16 + i * 4) = h;
        if (y16_lo) {
            const float o[4] = {v[0], v[1], v[2], v[3]};
            store_lo4(y16_lo, lo_fmt, i * 4, o, h);
        }
    }
}

// pnc_upsample_combine (include/panacea_hip.h): the nine tap products of a nearest-x2 Upsample conv, computed per SOURCE pixel by a
// plain-A GEMM, summed into the output pixels.  A work item owns the 2 x 2 output pixels of one source pixel (sy, sx) for 4 channels.
// Along y they read, per tap row u, the source rows  y = 2 sy: (u0, sy-1) (u1, sy) (u2, sy);  y = 2 sy + 1: (u0, sy) (u1, sy) (u2, sy+1)
// — five distinct (tap row, source row) slots, and the same five along x: 25 float4 loads, all issued ahead of the adds, for four
// output quads of nine terms each.  A workgroup is a UC_TH x UC_TW tile of source pixels x UC_TQ channel quads (512 contiguous bytes
// of a P row per tap): every P element is wanted by four output pixels, which sit in at most two neighbouring work items per axis, so
// the repeats are L1 / L2 hits of the same or the neighbouring workgroup (the block order keeps neighbours on one XCD).
constexpr int UC_TQ = 32, UC_TW = 4, UC_TH = 2;
static_assert(UC_TQ * UC_TW * UC_TH == 256, "one work item per thread of the 256-thread workgroup");

__global__ __launch_bounds__(256) void upsample_combine_kernel(const float* __restrict__ P, int64_t ldp,
                                                               const float* __restrict__ bias, int Hin, int Win, int Cout,
                                                               int tiles_x, int tiles_y, int qslices,
                                                               float* __restrict__ out32, half_t* __restrict__ out16,
                                                               void* __restrict__ out16_lo, int lo_fmt) {
    // block -> (frame, channel slice, tile row, tile column), tile column fastest
    int b = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y; b /= tiles_y;
    const int qs = b % qslices;
    const int f = b / qslices;
    const int tid = threadIdx.x;
    const int q = qs * UC_TQ + (tid & (UC_TQ - 1));
    const int pix = tid / UC_TQ;
    const int sx = tx * UC_TW + (pix % UC_TW), sy = ty * UC_TH + (pix / UC_TW);
    if (q * 4 >= Cout || sx >= Win || sy >= Hin) return;
    const int n = q * 4;
    // slot i of an axis: tap index SU[i] at source offset SD[i]; output parity d reads the slots SEL[d][0..2] for u = 0, 1, 2
    constexpr int SU[5] = {0, 0, 1, 2, 2}, SD[5] = {-1, 0, 0, 0, 1};
    constexpr int SEL[2][3] = {{0, 2, 3}, {1, 2, 4}};
    const bool rv[5] = {sy > 0, true, true, true, sy + 1 < Hin};       // a slot outside the image is zero padding: never read
    const bool cv[5] = {sx > 0, true, true, true, sx + 1 < Win};
    const float* Pn = P + n;
    f32x4 v[5][5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            if (rv[i] && cv[j]) {
                const int64_t row = ((int64_t)f * Hin + (sy + SD[i])) * Win + (sx + SD[j]);
                v[i][j] = *reinterpret_cast<const f32x4*>(Pn + row * ldp + (int64_t)(SU[i] * 3 + SU[j]) * Cout);
            } else {
                v[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
        }
    }
    const f32x4 bv = bias ? *reinterpret_cast<const f32x4*>(bias + n) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            f32x4 acc = bv;
#pragma unroll
            for (int u = 0; u < 3; ++u) {
#pragma unroll
                for (int w = 0; w < 3; ++w) {
                    const int i = SEL[dy][u], j = SEL[dx][w];
                    if (rv[i] && cv[j]) acc += v[i][j];              // (a skipped tap adds nothing: not even a +0 to a -0)
                }
            }
            const int64_t o = (((int64_t)f * (2 * Hin) + (2 * sy + dy)) * (2 * Win) + (2 * sx + dx)) * Cout + n;
            *reinterpret_cast<f32x4*>(out32 + o) = acc;
            if (out16) {
                half4v h = {(half_t)acc[0], (half_t)acc[1], (half_t)acc[2], (half_t)acc[3]};
                *reinterpret_cast<half4v*>(out16 + o) = h;
                if (out16_lo) {
                    const float r[4] = {acc[0], acc[1], acc[2], acc[3]};
                    store_lo4(out16_lo, lo_fmt, o, r, h);
                }
            }
        }
    }
}

// Exit of a sampler step: eps tokens of the CFG batch -> next latent, one pass.  The arithmetic
// follows the reference's sequence of fp32 roundings (no contraction into FMAs), so a trajectory matches the reference's
// sampler to the last few ulps.  Every product and sum is rounded on its own, like the reference's separate elementwise kernels:
// the operators are written out under `fp contract(off)` (HIP's __fmul_rn / __fadd_rn are plain inline operators compiled under
// the default contract(fast), so they DO fuse into FMAs).  The pragma is lexical — each function states its own; the kernel's does
// not reach into a function inlined into it.
//
// The guided denoised D of one element, the ONE copy every exit entry point runs.  SKIP: the general-skip form (x * c_skip[t]
// rounded on its own, then the sum: denoiser.py:28) of VScaling / EDMScaling; SKIP = false is the eps path (c_skip = 1, x enters
// the sum as it is) and never looks at cs.  eu, ec: the element's eps of the uncond / cond half (guiders.py:36; eu is unused
// without cfg).
template <bool SKIP>
__device__ __forceinline__ float guided_denoised(float xv, float eu, float ec, float co, float cs, int cfg, float scale) {
#pragma clang fp contract(off)
    const float xs = SKIP ? xv * cs : xv;                                // x * c_skip   (eps path: c_skip = 1)
    const float pc = ec * co;
    float D = pc + xs;                                                   // eps * c_out + x * c_skip
    if (cfg) {
        const float pu = eu * co;
        const float du = pu + xs;
        const float g = scale * (D - du);
        D = du + g;                                                      // x_u + scale * (x_c - x_u)
    }
    return D;
}

// The exit kernel of every sampler (include/panacea_hip.h: pnc_cfg_sampler_step): the denoised above, then the mode's update,
// every operation rounded on its own in the reference's order.  SKIP as above.  The Euler exit (pnc_cfg_euler_step) is HEUN1
// without out_aux: x + (sigma_next - sigma) * ((x - D) / sigma) is what HEUN1 writes to `out`.
template <bool SKIP>
__global__ __launch_bounds__(256) void cfg_sampler_step_kernel(const PncSamplerStepParams p, const float* __restrict__ c_skip) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)p.T * p.Npix) return;
    const int64_t t = i / p.Npix, pix = i - t * p.Npix;
    const float co = p.c_out[t];
    const float cs = SKIP ? c_skip[t] : 1.0f;
    const float v0 = p.v[0] ? p.v[0][t] : 0.f, v1 = p.v[1] ? p.v[1][t] : 0.f, v2 = p.v[2] ? p.v[2][t] : 0.f;
    const float v3 = p.v[3] ? p.v[3][t] : 0.f, v4 = p.v[4] ? p.v[4][t] : 0.f;
    const float* eu = p.eps_tok + i * p.ld;
    const float* ec = p.eps_tok + ((int64_t)(p.cfg ? p.T : 0) * p.Npix + i) * p.ld;
    for (int c = 0; c < p.C; ++c) {
        const int64_t o = (t * p.C + c) * p.Npix + pix;
        const float xv = p.x[o];
        const float D = guided_denoised<SKIP>(xv, eu[c], ec[c], co, cs, p.cfg, p.scale);
        float y;
        switch (p.mode) {
        case PNC_SAMPLER_HEUN1: {
            const float d = (xv - D) / v0;
            const float dt = v1 - v0;
            const float stp = dt * d;
            y = xv + stp;
            if (p.out_aux) p.out_aux[o] = d;                             // (launch-uniform) NULL: the Euler exit keeps no d
            break;
        }
        case PNC_SAMPLER_HEUN2: {
            const float d_new = (xv - D) / v1;
            const float sum = p.aux[o] + d_new;
            const float dp = sum / 2.0f;
            const float dt = v1 - v0;
            const float stp = dp * dt;
            const float xc = p.x0[o] + stp;
            y = v1 > 0.f ? xc : xv;
            break;
        }
        case PNC_SAMPLER_EULER_A:
        case PNC_SAMPLER_DPM2S_1: {
            const float d = (xv - D) / v0;
            const float dt = v1 - v0;
            const float stp = dt * d;
            const float xe = xv + stp;
            if (p.mode == PNC_SAMPLER_DPM2S_1) {
                const float a = v2 * xv;
                const float b = v3 * D;
                y = a - b;
                p.out_aux[o] = xe;
            } else {
                const float ns = p.noise[o] * p.s_noise;
                const float up = ns * v2;
                y = v3 > 0.f ? xe + up : xe;
            }
            break;
        }
        case PNC_SAMPLER_DPM2S_2: {
            const float a = v0 * p.x0[o];
            const float b = v1 * D;
            const float xd = a - b;
            const float xsel = v2 > 0.f ? xd : p.aux[o];
            const float ns = p.noise[o] * p.s_noise;
            const float up = ns * v3;
            y = v4 > 0.f ? xsel + up : xsel;
            break;
        }
        case PNC_SAMPLER_DPM2M: {
            const float a = v0 * xv;
            const float b = v1 * D;
            const float xst = a - b;
            y = xst;
            if (p.aux) {
                const float m3 = v2 * D;
                const float m4 = v3 * p.aux[o];
                const float dd = m3 - m4;
                const float b2 = v1 * dd;
                const float xa = a - b2;
                y = v4 > 0.f ? xa : xst;
            }
            p.out_aux[o] = D;
            break;
        }
        default: {                                                   // PNC_SAMPLER_LMS
            const float d = (xv - D) / v0;
            float acc = 0.0f + v1 * d;                               // sum() starts from the int 0
            if (p.n_hist > 0) { const float e = v2 * p.hist[0][o]; acc = acc + e; }
            if (p.n_hist > 1) { const float e = v3 * p.hist[1][o]; acc = acc + e; }
            if (p.n_hist > 2) { const float e = v4 * p.hist[2][o]; acc = acc + e; }
            y = xv + acc;
            p.out_aux[o] = d;
            break;
        }
        }
        p.out[o] = y;
    }
}

// pnc_frames_renoise (include/panacea_hip.h): known frames put back at a noise level.  A frame is ONE contiguous run of L = C * Npix
// floats (its C planes lie back to back), and a workgroup owns RN_SLICE consecutive elements of one frame: the selector, the sigma
// and the alignment case are workgroup-uniform.  The run is cut at the 16-byte boundaries of `out`: up to three head elements, a
// body of float4s, up to three tail elements.  The body runs as 16-byte loads and stores when the frame's operands sit at out's
// offset from a boundary (the sampler's tensors do: same shape, allocator-aligned bases, whatever Npix is); operands at other
// offsets take the frame element by element.  Every element is read before it is written and only by the thread that writes it,
// so out may be x.  The product is rounded on its own, then the sum (guided_denoised's discipline).
constexpr int RN_SLICE = 1024;

__device__ __forceinline__ float renoised(float a, float n, float s) {
#pragma clang fp contract(off)
    const float p = n * s;
    return a + p;
}

__global__ __launch_bounds__(256) void frames_renoise_kernel(const float* __restrict__ z, const float* __restrict__ noise,
                                                             const float* __restrict__ sigma, const float* __restrict__ keep,
                                                             const float* x, float* out, int64_t L, int slices) {
    const int t = (int)(blockIdx.x / (unsigned)slices), b = (int)(blockIdx.x - (unsigned)t * (unsigned)slices);
    const int tid = threadIdx.x;
    const bool kept = keep ? keep[t] > 0.0f : true;                  // 0.0, -0.0, negative, NaN: not kept
    if (!kept && x == out) return;                                   // the frame is where it belongs: not touched
    const float s = kept ? sigma[t] : 0.0f;
    const bool add = kept && s != 0.0f;                              // sigma 0: z's bits, the noise is not read
    const float* a = (kept ? z : x) + (int64_t)t * L;
    const float* n = noise + (int64_t)t * L;
    float* o = out + (int64_t)t * L;
    const unsigned off = (unsigned)((uintptr_t)o & 15);
    const bool vec = ((uintptr_t)a & 15) == off && (!add || ((uintptr_t)n & 15) == off);
    if (!vec) {                                                      // element by element, a slice per workgroup
#pragma unroll
        for (int k = 0; k < RN_SLICE / 256; ++k) {
            const int64_t j = (int64_t)b * RN_SLICE + k * 256 + tid;
            if (j < L) o[j] = add ? renoised(a[j], n[j], s) : a[j];
        }
        return;
    }
    const int64_t head = min((int64_t)((16 - off) & 15) >> 2, L);   // elements in front of out's first 16-byte boundary
    const int64_t nv = (L - head) >> 2;                             // whole float4s behind it (<= slices * 256)
    const int64_t i = (int64_t)b * 256 + tid;
    if (i < nv) {
        const int64_t j = head + i * 4;
        f32x4 v = *reinterpret_cast<const f32x4*>(a + j);
        if (add) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(n + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = renoised(v[e], w[e], s);
        }
        *reinterpret_cast<f32x4*>(o + j) = v;
    }
    if (b == 0 && tid < 8) {                                         // lanes 0..3: the head, lanes 4..7: the tail
        const int64_t j = tid < 4 ? tid : head + nv * 4 + (tid - 4);
        if (tid < 4 ? j < head : j < L) o[j] = add ? renoised(a[j], n[j], s) : a[j];
    }
}

inline hipStream_t hip_stream(void* stream) { return reinterpret_cast<hipStream_t>(stream); }

// every launch of this file: 256-thread workgroups over n threads' worth of work (a thread per item: n items; a wave per item:
// 64 n; a workgroup per item: 256 n) on the caller's stream
template <typename... Sig, typename... Args>
int launch_1d(void (*kernel)(Sig...), int64_t n, void* stream, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hip_stream(stream), args...);
    return pnc_launch_status();
}

// The one launch of the four exit entry points.  `euler_exit`: HEUN1 may come without out_aux — how the two Euler entries reach
// the kernel, not a mode of the public struct entries.
int cfg_sampler_step_launch(const PncSamplerStepParams* pp, const float* c_skip, bool skip, bool euler_exit, void* stream) {
    if (!pp || pp->struct_bytes != (int32_t)sizeof(PncSamplerStepParams)) return PNC_EABI;
    const PncSamplerStepParams& p = *pp;
    if (!p.eps_tok || !p.x || !p.c_out || !p.out || p.T < 1 || p.Npix < 1 || p.C < 1 || p.ld < p.C) return PNC_EINVAL;
    if (skip && !c_skip) return PNC_EINVAL;                          // never "c_skip = 1": the eps path is the entry without _skip
    int nv = 0;                                                      // per-frame vectors the mode reads
    bool ok = true;
    switch (p.mode) {
    case PNC_SAMPLER_HEUN1: nv = 2; ok = p.out_aux || euler_exit; break;
    case PNC_SAMPLER_HEUN2: nv = 2; ok = p.x0 && p.aux; break;
    case PNC_SAMPLER_EULER_A: nv = 4; ok = p.noise; break;
    case PNC_SAMPLER_DPM2S_1: nv = 4; ok = p.out_aux; break;
    case PNC_SAMPLER_DPM2S_2: nv = 5; ok = p.x0 && p.aux && p.noise; break;
    case PNC_SAMPLER_DPM2M: nv = p.aux ? 5 : 2; ok = p.out_aux; break;
    case PNC_SAMPLER_LMS:
        nv = 2 + p.n_hist;
        ok = p.out_aux && p.n_hist >= 0 && p.n_hist <= 3;
        for (int k = 0; ok && k < p.n_hist; ++k) ok = p.hist[k] != nullptr;
        break;
    default: return PNC_EINVAL;
    }
    for (int k = 0; ok && k < nv; ++k) ok = p.v[k] != nullptr;
    if (!ok) return PNC_EINVAL;
    return launch_1d(skip ? cfg_sampler_step_kernel<true> : cfg_sampler_step_kernel<false>, (int64_t)p.T * p.Npix, stream, p,
                     c_skip);
}

// the Euler exit: HEUN1 with v = {sigma, sigma_next} into x_next, no d kept
int cfg_euler_step_launch(const float* eps_tok, int ld, int T, int Npix, int C, int cfg, float scale, const float* x,
                          const float* c_out, const float* sigma, const float* sigma_next, float* x_next, const float* c_skip,
                          bool skip, void* stream) {
    PncSamplerStepParams p = {};
    p.struct_bytes = (int32_t)sizeof(PncSamplerStepParams);
    p.mode = PNC_SAMPLER_HEUN1;
    p.eps_tok = eps_tok, p.ld = ld, p.T = T, p.Npix = Npix, p.C = C, p.cfg = cfg, p.scale = scale;
    p.x = x, p.c_out = c_out, p.v[0] = sigma, p.v[1] = sigma_next, p.out = x_next;
    return cfg_sampler_step_launch(&p, c_skip, skip, true, stream);
}

}  // namespace

extern "C" int pnc_cfg_euler_step(const float* eps_tok, int ld, int T, int Npix, int C, int cfg, float scale,
                                  const float* x, const float* c_out, const float* sigma, const float* sigma_next,
                                  float* x_next, void* stream) {
    return cfg_euler_step_launch(eps_tok, ld, T, Npix, C, cfg, scale, x, c_out, sigma, sigma_next, x_next, nullptr, false, stream);
}

extern "C" int pnc_cfg_euler_step_skip(const float* eps_tok, int ld, int T, int Npix, int C, int cfg, float scale,
                                       const float* x, const float* c_skip, const float* c_out, const float* sigma,
                                       const float* sigma_next, float* x_next, void* stream) {
    return cfg_euler_step_launch(eps_tok, ld, T, Npix, C, cfg, scale, x, c_out, sigma, sigma_next, x_next, c_skip, true, stream);
}

extern "C" int pnc_cfg_sampler_step(const PncSamplerStepParams* pp, void* stream) {
    return cfg_sampler_step_launch(pp, nullptr, false, false, stream);
}

extern "C" int pnc_cfg_sampler_step_skip(const PncSamplerStepParams* pp, const float* c_skip, void* stream) {
    return cfg_sampler_step_launch(pp, c_skip, true, false, stream);
}

extern "C" int pnc_frames_renoise(const float* z, const float* noise, const float* sigma, const float* keep, const float* x,
                                  float* out, int T, int C, int64_t Npix, void* stream) {
    // the selector lives on the device: the host never knows that nothing is kept, so z and noise are always wanted
    if (!z || !noise || !sigma || !out || (keep && !x) || T < 1 || C < 1 || Npix < 1) return PNC_EINVAL;
    if (Npix > ((int64_t)1 << 40) / C) return PNC_EINVAL;            // a frame of at most 2^40 elements ...
    const int64_t L = (int64_t)C * Npix, slices = (L + RN_SLICE - 1) / RN_SLICE;
    if ((int64_t)T * slices >= ((int64_t)1 << 31)) return PNC_EINVAL;  // ... and a grid the launch can count
    if (((uintptr_t)z | (uintptr_t)noise | (uintptr_t)sigma | (uintptr_t)keep | (uintptr_t)x | (uintptr_t)out) & 3) return PNC_EALIGN;
    return launch_1d(frames_renoise_kernel, (int64_t)T * slices * 256, stream, z, noise, sigma, keep, x, out, L, (int)slices);
}

extern "C" const char* pnc_version(void) { return "panacea_hip 0.4.0 gfx950"; }
// the digest of the sources this object was compiled from (panacea_amd/build.py passes it to this translation unit)
#ifndef PNC_BUILD_DIGEST
#define PNC_BUILD_DIGEST "unstamped"
#endif
// (stored behind a marker so that build.py can read it from the FILE: dlopen-ing a library to ask it would pin the old image in
// the asking process and make a rebuild + load in the same process see the stale one)
static const char k_build_digest[] = "pnc-build-digest:" PNC_BUILD_DIGEST;
extern "C" const char* pnc_build_digest(void) { return k_build_digest + 17; }

static std::atomic<int> g_options[PNC_OPT_COUNT] = {{1}, {0}, {0}, {1}, {1}, {0}, {1}, {3}, {8}, {1}, {4}, {12}};

int pnc_get_option(int option) { return g_options[option].load(std::memory_order_relaxed); }

extern "C" int pnc_set_option(int option, int value) {
    if (option < 0 || option >= PNC_OPT_COUNT) return PNC_EINVAL;
    return g_options[option].exchange(value, std::memory_order_relaxed);
}

extern "C" int pnc_linear_smallm_split(const float* a, int lda, const void* W, const void* W_lo, const float* bias,
                                       float* out, int ldo, int M, int N, int K, int silu_in, int silu_out,
                                       void* stream) {
    if (!a || !W || !out || M < 1 || M > SM_MAXM || N < 1 || K < 8) return PNC_EINVAL;
    if (K % 8 || lda % 4) return PNC_EINVAL;
    if (((uintptr_t)a | (uintptr_t)W | (uintptr_t)W_lo) & 15) return PNC_EALIGN;
    return launch_1d(linear_smallm_kernel, (int64_t)N * 64, stream, a, lda, f16p(W), f16p(W_lo), bias, out, ldo, M, N, K, silu_in,
                     silu_out);                                  // a wave per column
}

extern "C" int pnc_linear_smallm(const float* a, int lda, const void* W, const float* bias,
                                 float* out, int ldo, int M, int N, int K, int silu_in, int silu_out,
                                 void* stream) {
    return pnc_linear_smallm_split(a, lda, W, nullptr, bias, out, ldo, M, N, K, silu_in, silu_out, stream);
}

extern "C" int pnc_linear_smallm_segments(const float* a, int lda, const void* W, const float* bias, float* out, int M,
                                          int m0, int Mtot, int N, int K, const int32_t* seg_start, int nseg, int silu_in,
                                          int silu_out, void* stream) {
    return pnc_linear_smallm_segments_split(a, lda, W, nullptr, bias, out, M, m0, Mtot, N, K, seg_start, nseg, silu_in, silu_out, stream);
}

extern "C" int pnc_linear_smallm_segments_split(const float* a, int lda, const void* W, const void* W_lo, const float* bias,
                                                float* out, int M, int m0, int Mtot, int N, int K, const int32_t* seg_start,
                                                int nseg, int silu_in, int silu_out, void* stream) {
    if (!a || !W || !out || !seg_start || M < 1 || M > SM_MAXM || m0 < 0 || m0 + M > Mtot || N < 1 || K < 8) return PNC_EINVAL;
    if (K % 8 || lda % 4 || nseg < 1 || nseg > PNC_SMALLM_MAX_SEGS) return PNC_EINVAL;
    if (((uintptr_t)a | (uintptr_t)W | (uintptr_t)W_lo) & 15) return PNC_EALIGN;
    SmallmSegs segs;
    segs.nseg = nseg;
    if (seg_start[0] != 0 || seg_start[nseg] != N) return PNC_EINVAL;
    for (int i = 0; i <= nseg; ++i) {
        if (seg_start[i] % SEG_NC || (i > 0 && seg_start[i] <= seg_start[i - 1])) return PNC_EINVAL;
        segs.start[i] = seg_start[i];
    }
    return launch_1d(linear_smallm_seg_kernel, (int64_t)(N / SEG_NC) * 64, stream, a, lda, f16p(W), f16p(W_lo), bias, out, M, m0, Mtot,
                     N, K, silu_in, silu_out, segs);             // a wave per SEG_NC columns
}

template <typename TS>
static int timestep_embedding(const TS* t, int F, int dim, const float* freqs, float* out, void* stream) {
    if (!t || !out || !freqs || F < 1 || dim < 2) return PNC_EINVAL;
    return launch_1d(timestep_embedding_kernel<TS>, F * (dim / 2), stream, t, F, dim, freqs, out);
}

extern "C" int pnc_timestep_embedding(const int64_t* t, int F, int dim, const float* freqs,
                                      float* out, void* stream) {
    return timestep_embedding(t, F, dim, freqs, out, stream);
}

extern "C" int pnc_timestep_embedding_f32(const float* t, int F, int dim, const float* freqs,
                                          float* out, void* stream) {
    return timestep_embedding(t, F, dim, freqs, out, stream);
}

extern "C" int pnc_nchw_to_tokens_f16(const float* a, int C1, const float* a_scale, int a_frames, const float* b, int C2,
                                      int F, int Npix, int Cpad, void* out16, void* out16_lo, void* stream) {
    if (!a || !out16 || F < 1 || Npix < 1 || C1 < 1 || C2 < 0 || (C2 > 0 && !b)) return PNC_EINVAL;
    if (a_frames < 1 || a_frames > F) return PNC_EINVAL;
    if (Cpad % 8 || Cpad < C1 + C2) return PNC_EINVAL;
    if (((uintptr_t)out16 | (uintptr_t)out16_lo) & 15) return PNC_EALIGN;
    return launch_1d(nchw_to_tokens_kernel, (int64_t)F * Npix, stream, a, C1, a_scale, a_frames, b, C2, F, Npix, Cpad, f16p(out16),
                     f16p(out16_lo));
}

extern "C" int pnc_tokens_to_nchw_f32(const float* x, int ld, int F, int Npix, int C,
                                      float* out, void* stream) {
    if (!x || !out || F < 1 || Npix < 1 || C < 1 || ld < C) return PNC_EINVAL;
    return launch_1d(tokens_to_nchw_kernel, (int64_t)F * Npix, stream, x, ld, F, Npix, C, out);
}

extern "C" int pnc_concat_add(const float* a, int C1, const float* s, const float* c, int C2,
                              int64_t M, float* out32, void* out16, void* out16_lo, int lo_fmt, void* stream) {
    if (!a || !s || M < 1 || C1 % 4 || C2 % 4 || C1 < 4 || C2 < 4) return PNC_EINVAL;
    if (lo_fmt != PNC_LO_F16 && lo_fmt != PNC_LO_E4M3) return PNC_EINVAL;
    if ((!out32 && !out16) || (out16_lo && !out16)) return PNC_EINVAL;
    return launch_1d(concat_add_kernel, M * ((C1 + C2) / 4), stream, a, C1, s, c, C2, M, out32, f16p(out16), out16_lo, lo_fmt);
}

extern "C" int pnc_add_f32(const float* x, const float* a, int64_t n, float* y32, void* y16, void* y16_lo, int lo_fmt,
                           void* stream) {
    if (!x || n < 4 || n % 4 || (!y32 && !y16) || (y16_lo && !y16)) return PNC_EINVAL;
    if (lo_fmt != PNC_LO_F16 && lo_fmt != PNC_LO_E4M3) return PNC_EINVAL;
    return launch_1d(add_kernel, n / 4, stream, x, a, n / 4, y32, f16p(y16), y16_lo, lo_fmt);
}

extern "C" int pnc_upsample_combine(const float* P, int64_t ldp, const float* bias, int F, int Hin, int Win, int Cout, float* out32,
                                    void* out16, void* out16_lo, int lo_fmt, void* stream) {
    if (!P || !out32 || F < 1 || Hin < 1 || Win < 1 || Cout < 4 || Cout % 4 || ldp % 4 || ldp < 9 * (int64_t)Cout) return PNC_EINVAL;
    if (lo_fmt != PNC_LO_F16 && lo_fmt != PNC_LO_E4M3) return PNC_EINVAL;
    if (out16_lo && !out16) return PNC_EINVAL;
    if (((uintptr_t)P | (uintptr_t)bias | (uintptr_t)out32 | (uintptr_t)out16 | (uintptr_t)out16_lo) & 15) return PNC_EALIGN;
    const int tiles_x = (Win + UC_TW - 1) / UC_TW, tiles_y = (Hin + UC_TH - 1) / UC_TH, qslices = (Cout / 4 + UC_TQ - 1) / UC_TQ;
    const int64_t blocks = (int64_t)F * tiles_y * tiles_x * qslices;
    if (blocks >= ((int64_t)1 << 31)) return PNC_EINVAL;
    return launch_1d(upsample_combine_kernel, blocks * 256, stream, P, ldp, bias, Hin, Win, Cout, tiles_x, tiles_y, qslices, out32,
                     f16p(out16), out16_lo, lo_fmt);                  // a workgroup per (frame, channel slice, source tile)
}

// row softmax: one 256-thread block per row, the row lives in registers (<= 16 x float4 per thread), one HBM read
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ s, int64_t lds, int N, float scale,
                                                           int causal, int n_valid,
                                                           half_t* __restrict__ p, int64_t ldp) {
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = s + (int64_t)blockIdx.x * lds;
    half_t* prow = p + (int64_t)blockIdx.x * ldp;
    const int nv = N >> 2;
    // keys this row may see: the first n_valid columns, and with a causal mask only those up to the row's own index
    const int lim = causal ? min(n_valid, (int)blockIdx.x + 1) : n_valid;
    f32x4 v[16];
    float m = -3.0e38f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = tid + j * 256;
        if (c < nv) {
            v[j] = *reinterpret_cast<const f32x4*>(row + c * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[j][e] = (c * 4 + e < lim) ? v[j][e] : -3.0e38f;      // masked: out of the maximum
            m = fmaxf(fmaxf(fmaxf(v[j][0], v[j][1]), fmaxf(v[j][2], v[j][3])), m);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float sc = scale * 1.44269504088896340736f;
    const float off = m * sc;
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = tid + j * 256;
        if (c < nv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // the mask is a predicate: exp2 of the -3.0e38 stand-in is 0 only while 3e38 * sc is huge, and at scale = 0 (or a
                // tiny one) fmaf(-3e38, sc, -off) is 0 or small.  A masked element adds +0 to the sum and stores +0, whatever the scale;
                // a visible one is computed as before, so unmasked launches keep their bits
                const float pe = __builtin_amdgcn_exp2f(fmaf(v[j][e], sc, -off));
                v[j][e] = (c * 4 + e < lim) ? pe : 0.0f;
                sum += v[j][e];
            }
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float inv = 1.0f / (((red[4] + red[5]) + red[6]) + red[7]);     // fixed order: deterministic
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = tid + j * 256;
        if (c < nv) {
            half4v h;
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = (half_t)(v[j][e] * inv);
            *reinterpret_cast<half4v*>(prow + c * 4) = h;
        }
    }
}

extern "C" int pnc_softmax_rows_f16(const float* s, int64_t lds, int M, int N, float scale, int causal, int n_valid,
                                    void* p16, int64_t ldp, void* stream) {
    if (!s || !p16 || M < 1 || N < 4 || N > 16384 || (N & 3) || n_valid > N) return PNC_EINVAL;
    if (n_valid <= 0) n_valid = N;
    if ((lds & 3) || (ldp & 3) || lds < N || ldp < N) return PNC_EINVAL;
    if (((uintptr_t)s & 15) || ((uintptr_t)p16 & 7)) return PNC_EALIGN;
    return launch_1d(softmax_rows_kernel, (int64_t)M * 256, stream, s, lds, N, scale, causal, n_valid, f16p(p16), ldp);   // a workgroup per row
}

extern "C" int pnc_cast_f16(const float* x, int64_t n, void* y16, void* y16_lo, int lo_fmt, void* stream) {
    return pnc_add_f32(x, nullptr, n, nullptr, y16, y16_lo, lo_fmt, stream);
}

// The translation units that pack e4m3 lo planes, each with a PNC_DEFINE_TU_COLLECT(name) of its own (common.h): the one list
// their accessors are declared and called from
#define PNC_TU_COLLECTS(X)                                                                                                       \
    X(gemm) X(gemm_plain) X(gemm_conv3x3) X(gemm_conv1d) X(gemm_stencil_tile) X(gemm_plain_ws) X(gemm_conv3x3_ws) X(gemm_conv1d_ws) \
    X(norm) X(misc)
#define PNC_TU_DECLARE(name) void pnc_tu_collect_##name(unsigned int*, hipStream_t);
#define PNC_TU_CALL(name) pnc_tu_collect_##name(out, st);
PNC_TU_COLLECTS(PNC_TU_DECLARE)
PNC_DEFINE_TU_COLLECT(misc)

extern "C" int pnc_range_monitor_collect(unsigned int* out, void* stream) {
    if (!out) return PNC_EINVAL;
    hipStream_t st = hip_stream(stream);
    PNC_TU_COLLECTS(PNC_TU_CALL)
    return pnc_launch_status();
}
