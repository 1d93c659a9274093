// attn_split.hip — attention on split operands (include/panacea_hip.h: pnc_attn_views_split_f16 / pnc_attn_temporal_split_f16).
//
// The `precise-wide` operand policy carries q, k, v and the attention output as fp16 pairs v ~ hi + lo * 2^-11.  One wave owns a
// tile of 16 queries of one head and walks the keys 16 at a time on v_mfma_f32_16x16x16_f16:
//   S^T = K . Q^T   (A = 16 keys x 16 channels, B = 16 channels x 16 queries)
// so that the score accumulator, key = 4 * (lane >> 4) + reg and query = lane & 15, IS the B fragment of P^T in
//   O^T = V^T . P^T (A = 16 channels x 16 keys, B = 16 keys x 16 queries)
// and every per-query quantity of the online softmax (running max, sum, rescale) is one value per lane.  The hi.hi products and the
// cross products accumulate in separate fp32 registers and meet once, scaled by 2^-11, in fp32.
// Correctness first: K / Q fragments are 8-byte row loads, V^T fragments 2-byte gathers (no LDS staging, no tuning).
#include "common.h"
#include "attn_check.h"

namespace {

// v_mfma_f32_16x16x16_f16 fragment maps (wave64):
//   A[i][k]: lane i + 16 * (k / 4), element k % 4;   B[k][j]: lane j + 16 * (k / 4), element k % 4
//   D[i][j]: lane j + 16 * (i / 4), register i % 4
__device__ __forceinline__ f32x4 mfma16(half4v a, half4v b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ half4v load4(const half_t* base, int64_t idx, bool ok) {
    if (!ok) return half4v{0, 0, 0, 0};
    return *reinterpret_cast<const half4v*>(base + idx);
}

constexpr float LO_INV = 1.0f / PNC_LO_SCALE;

// Online-softmax state and output accumulators of one 16-query tile (one query per lane column, lane & 15)
struct SplitTile {
    half4v qh[4], ql[4];               // Q^T fragments, 4 k-steps of 16 channels
    f32x4 o[4], ox[4];                 // O^T: hi.hi products / cross products, channel block db = 16 channels
    float m, l;

    __device__ void init(const half_t* q, const half_t* q_lo, int64_t qrow, bool qok, int ldq, int lane) {
        const int c0 = 4 * (lane >> 4);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            qh[s] = load4(q, qrow * ldq + s * 16 + c0, qok);
            ql[s] = load4(q_lo, qrow * ldq + s * 16 + c0, qok);
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
            ox[d] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        m = -INFINITY;
        l = 0.f;
    }

    // one block of 16 keys.  krow[r]: row of key 4 * (lane >> 4) + r (the V^T gather), kvalid[r] its validity; my_krow / my_kok:
    // the key of row lane & 15 (the K fragment).  Invalid keys read zeros (padding may hold anything, NaN included) and score -inf.
    __device__ void step(const half_t* k, const half_t* k_lo, int ldk, const half_t* v, const half_t* v_lo, int ldv,
                         int64_t my_krow, bool my_kok, const int64_t (&krow)[4], const bool (&kok)[4], float scale, int lane) {
        const int c0 = 4 * (lane >> 4);
        f32x4 shh = {0.f, 0.f, 0.f, 0.f}, sx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const half4v kh = load4(k, my_krow * ldk + s * 16 + c0, my_kok);
            const half4v kl = load4(k_lo, my_krow * ldk + s * 16 + c0, my_kok);
            shh = mfma16(kh, qh[s], shh);
            sx = mfma16(kl, qh[s], sx);
            sx = mfma16(kh, ql[s], sx);
        }
        float sc[4];
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sc[r] = kok[r] ? (shh[r] + sx[r] * LO_INV) * scale : -INFINITY;
            mt = fmaxf(mt, sc[r]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float mn = fmaxf(m, mt);                 // finite: every block holds at least one valid key
        const float alpha = expf(m - mn);
        float p[4], ls = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[r] = kok[r] ? expf(sc[r] - mn) : 0.f;
            ls += p[r];
        }
        ls += __shfl_xor(ls, 16, 64);
        ls += __shfl_xor(ls, 32, 64);
        l = l * alpha + ls;
        m = mn;
        half4v ph, pl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ph[r] = (half_t)p[r];
            pl[r] = (half_t)((p[r] - (float)ph[r]) * PNC_LO_SCALE);
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            half4v vh, vl;
            const int ch = d * 16 + (lane & 15);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                vh[e] = kok[e] ? v[krow[e] * ldv + ch] : (half_t)0;
                vl[e] = kok[e] ? v_lo[krow[e] * ldv + ch] : (half_t)0;
            }
            o[d] *= alpha;
            ox[d] *= alpha;
            o[d] = mfma16(vh, ph, o[d]);
            ox[d] = mfma16(vl, ph, ox[d]);
            ox[d] = mfma16(vh, pl, ox[d]);
        }
    }

    __device__ void store(half_t* out, half_t* out_lo, int64_t orow, bool ok, int ldo, int lane) const {
        if (!ok) return;
        const float inv = 1.0f / l;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            float val[4];
            half4v hi;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                val[r] = (o[d][r] + ox[d][r] * LO_INV) * inv;
                hi[r] = (half_t)val[r];
            }
            const int64_t idx = orow * ldo + d * 16 + 4 * (lane >> 4);
            *reinterpret_cast<half4v*>(out + idx) = hi;
            *reinterpret_cast<half4v*>(out_lo + idx) = lo_plane4(val, hi);
        }
    }
};

struct ViewsGeom {
    int groups, heads, H, W, views, Wv, Nq, nqt;
    int kvW, kvWv, kv_rows, q_per_kv, kv_valid;
    int nseg[8], seg[8][2];
};

__global__ __launch_bounds__(256) void attn_views_split_kernel(
        const half_t* __restrict__ q, const half_t* __restrict__ q_lo, int ldq,
        const half_t* __restrict__ k, const half_t* __restrict__ k_lo, int ldk,
        const half_t* __restrict__ v, const half_t* __restrict__ v_lo, int ldv,
        half_t* __restrict__ o, half_t* __restrict__ o_lo, int ldo, ViewsGeom G, float scale, int64_t ntiles) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntiles) return;                       // wave-uniform; no barriers below
    const int h = (int)(tile % G.heads);
    int64_t rest = tile / G.heads;
    const int qt = (int)(rest % G.nqt);
    rest /= G.nqt;
    const int vw = (int)(rest % G.views);
    const int g = (int)(rest / G.views);
    const int kg = g / G.q_per_kv;

    const int qi = qt * 16 + (lane & 15);
    const bool qok = qi < G.Nq;
    const int64_t qrow = qok ? (int64_t)g * G.H * G.W + (int64_t)(qi / G.Wv) * G.W + vw * G.Wv + qi % G.Wv : 0;

    SplitTile t;
    t.init(q + h * 64, q_lo + h * 64, qrow, qok, ldq, lane);
    const half_t* kh = k + h * 64;
    const half_t* klo = k_lo + h * 64;
    const half_t* vh = v + h * 64;
    const half_t* vlo = v_lo + h * 64;
    const int64_t kbase = (int64_t)kg * G.kv_rows;
    for (int sgi = 0; sgi < G.nseg[vw]; ++sgi) {
        const int u = G.seg[vw][sgi];
        for (int j0 = 0; j0 < G.kv_valid; j0 += 16) {
            const int jm = j0 + (lane & 15);
            const bool mok = jm < G.kv_valid;
            const int64_t mrow = mok ? kbase + (int64_t)(jm / G.kvWv) * G.kvW + u * G.kvWv + jm % G.kvWv : 0;
            int64_t krow[4];
            bool kok[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + 4 * (lane >> 4) + r;
                kok[r] = j < G.kv_valid;
                krow[r] = kok[r] ? kbase + (int64_t)(j / G.kvWv) * G.kvW + u * G.kvWv + j % G.kvWv : 0;
            }
            t.step(kh, klo, ldk, vh, vlo, ldv, mrow, mok, krow, kok, scale, lane);
        }
    }
    t.store(o + h * 64, o_lo + h * 64, qrow, qok, ldo, lane);
}

__global__ __launch_bounds__(256) void attn_temporal_split_kernel(
        const half_t* __restrict__ q, const half_t* __restrict__ q_lo, int ldq,
        const half_t* __restrict__ k, const half_t* __restrict__ k_lo, int ldk,
        const half_t* __restrict__ v, const half_t* __restrict__ v_lo, int ldv,
        half_t* __restrict__ o, half_t* __restrict__ o_lo, int ldo, int T, int Npix, int heads, float scale, int64_t ntiles) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const int h = (int)(tile % heads);
    const int64_t bp = tile / heads;                  // b * Npix + p
    const int64_t b = bp / Npix, p = bp % Npix;
    const int64_t row0 = b * T * Npix + p;            // frame t of this pixel: row0 + t * Npix

    const int ti = lane & 15;
    const bool qok = ti < T;
    const int64_t qrow = qok ? row0 + (int64_t)ti * Npix : 0;
    SplitTile t;
    t.init(q + h * 64, q_lo + h * 64, qrow, qok, ldq, lane);
    int64_t krow[4];
    bool kok[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = 4 * (lane >> 4) + r;
        kok[r] = j < T;
        krow[r] = kok[r] ? row0 + (int64_t)j * Npix : 0;
    }
    t.step(k + h * 64, k_lo + h * 64, ldk, v + h * 64, v_lo + h * 64, ldv, qrow, qok, krow, kok, scale, lane);
    t.store(o + h * 64, o_lo + h * 64, qrow, qok, ldo, lane);
}

}  // namespace

extern "C" int pnc_attn_views_split_f16(const PncAttnSplitParams* sp, void* stream) {
    if (!sp) return PNC_EINVAL;
    if (sp->struct_bytes != (int32_t)sizeof(PncAttnSplitParams)) return PNC_EABI;
    const PncAttnParams& p = sp->a;
    if (!p.q || !p.k || !p.vt || !p.o || !sp->q_lo || !sp->k_lo || !sp->v_lo || !sp->o_lo) return PNC_EINVAL;
    if (p.causal != 0 || p.k_halo[0] || p.k_halo[1] || p.vt_halo[0] || p.vt_halo[1]) return PNC_EINVAL;
    if (!pnc_attn::views_ok(p) || !pnc_attn::counts_ok(p)) return PNC_EINVAL;           // the rules shared with pnc_attn_views_f16
    if (p.H < 1 || p.kvH < 1 || p.kv_rows_per_group < p.kvH * p.kvW) return PNC_EINVAL;
    for (int v = 0; v < p.views; ++v) {
        if (!pnc_attn::nseg_ok(p, v)) return PNC_EINVAL;
        for (int s = 0; s < p.nseg[v]; ++s)
            if (p.seg[v][s] < 0 || p.seg[v][s] >= p.kv_views) return PNC_EINVAL;
    }
    if (p.ldq % 4 || p.ldk % 4 || p.ldvt % 4 || p.ldo % 4) return PNC_EALIGN;
    if (((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.vt | (uintptr_t)p.o | (uintptr_t)sp->q_lo | (uintptr_t)sp->k_lo | (uintptr_t)sp->v_lo |
         (uintptr_t)sp->o_lo) & 7) return PNC_EALIGN;
    ViewsGeom G{};
    G.groups = p.groups; G.heads = p.heads; G.H = p.H; G.W = p.W; G.views = p.views; G.Wv = p.W / p.views;
    G.Nq = p.H * G.Wv; G.nqt = (G.Nq + 15) / 16;
    G.kvW = p.kvW; G.kvWv = p.kvW / p.kv_views; G.kv_rows = p.kv_rows_per_group; G.q_per_kv = p.q_per_kv; G.kv_valid = p.kv_valid;
    for (int v = 0; v < 8; ++v) {
        G.nseg[v] = p.nseg[v];
        G.seg[v][0] = p.seg[v][0];
        G.seg[v][1] = p.seg[v][1];
    }
    const int64_t ntiles = (int64_t)p.groups * p.views * G.nqt * p.heads;
    const int64_t blocks = (ntiles + 3) / 4;
    hipLaunchKernelGGL(attn_views_split_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       f16p(p.q), f16p(sp->q_lo), p.ldq, f16p(p.k), f16p(sp->k_lo), p.ldk, f16p(p.vt), f16p(sp->v_lo), p.ldvt,
                       f16p(p.o), f16p(sp->o_lo), p.ldo, G, p.scale, ntiles);
    return pnc_launch_status();
}

extern "C" int pnc_attn_temporal_split_f16(const void* q, const void* q_lo, int ldq, const void* k, const void* k_lo, int ldk,
                                           const void* v, const void* v_lo, int ldv, void* o, void* o_lo, int ldo,
                                           int B, int T, int Npix, int heads, float scale, void* stream) {
    if (!q || !k || !v || !o || !q_lo || !k_lo || !v_lo || !o_lo) return PNC_EINVAL;
    if (T < 1 || T > 16 || B < 1 || Npix < 1 || heads < 1) return PNC_EINVAL;
    if (ldq % 4 || ldk % 4 || ldv % 4 || ldo % 4) return PNC_EALIGN;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)q_lo | (uintptr_t)k_lo | (uintptr_t)v_lo | (uintptr_t)o_lo) & 7)
        return PNC_EALIGN;
    const int64_t ntiles = (int64_t)B * Npix * heads;
    const int64_t blocks = (ntiles + 3) / 4;
    hipLaunchKernelGGL(attn_temporal_split_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       f16p(q), f16p(q_lo), ldq, f16p(k), f16p(k_lo), ldk, f16p(v), f16p(v_lo), ldv, f16p(o), f16p(o_lo), ldo,
                       T, Npix, heads, scale, ntiles);
    return pnc_launch_status();
}
