// attn_text_split.hip — the causal self-attention of the text tower on SPLIT operands (include/panacea_hip.h §6c,
// pnc_attn_text_split_f16): q, k, v and o are fp16 pairs x ~ hi + 2^-11 lo, a prompt is a group of Lp <= 96 token rows, a head 64
// columns, V is ROW-major like K (what the QKV GEMM writes as out16 + out16_lo with N = 3 W).
//
//   S = Qh.Kh + 2^-11 (Qh.Kl + Ql.Kh)        P = Ph + 2^-11 Pl        O = Ph.Vh + 2^-11 (Ph.Vl + Pl.Vh)
//   query i attends key j  iff  j <= i and j < kv_valid
//
// Form.  One workgroup per (prompt, head), four waves.  The four planes K hi / lo and V hi / lo of the head are fetched from global
// memory ONCE, with 16-byte loads, into LDS (rows of keys >= kv_valid are written as zeros, never loaded).  Wave w owns the query
// tiles w and w + 4 of 16 queries; a query tile visits the key tiles up to its own and up to the last valid key — the tiles above the
// diagonal are skipped, not masked.  As in attn_split.hip the scores are formed transposed on v_mfma_f32_16x16x16_f16,
//   S^T = K . Q^T   (A = 16 keys x 16 channels, B = 16 channels x 16 queries),
// so the score accumulator — key 4 (lane >> 4) + reg, query lane & 15 — IS the B fragment of P^T in O^T = V^T . P^T and every softmax
// quantity is one value per lane.  At most six key tiles = 24 scores per lane stay in registers: an exact two-pass softmax (maximum,
// then exp2), no running maximum, no rescale.  The V^T fragments come out of the row-major LDS image through ds_read_b64_tr_b16
// (attn_temporal_wide_kernel reads its V the same way).  The hi.hi products and the cross products accumulate in separate fp32
// registers and meet once, scaled by 2^-11.  The launch is a few dozen workgroups: bound by latency, the schedule is not tuned.
#include "common.h"

namespace {

constexpr int TS_MAXL = 96;                      // most token rows of a prompt
constexpr int TS_TILES = TS_MAXL / 16;           // most key tiles, and query tiles, of a prompt
constexpr int TS_ROW = 144;                      // bytes of an LDS row: 64 halves + 16 bytes, so the 16 rows of a K fragment read spread over the banks
constexpr int TS_PLANE = TS_MAXL * TS_ROW;
constexpr float TS_LO_INV = 1.0f / PNC_LO_SCALE;
static_assert(4 * TS_PLANE <= 64 * 1024, "attn_text_split_kernel: LDS beyond 64 KB");
static_assert(TS_ROW % 16 == 0, "attn_text_split_kernel: 16-byte LDS stores, 8-byte transposed reads");

typedef __fp16 ts_tr_half4v __attribute__((__vector_size__(4 * sizeof(__fp16))));      // ds_read_tr16_b64's own vector type
typedef __attribute__((address_space(3))) ts_tr_half4v ts_lds_half4v;

__device__ __forceinline__ f32x4 ts_mfma(half4v a, half4v b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }

__global__ __launch_bounds__(256, 1) void attn_text_split_kernel(
        const half_t* __restrict__ Q, const half_t* __restrict__ Qlo, const int64_t ldq, const half_t* __restrict__ K,
        const half_t* __restrict__ Klo, const int64_t ldk, const half_t* __restrict__ V, const half_t* __restrict__ Vlo, const int64_t ldv,
        half_t* __restrict__ O, half_t* __restrict__ Olo, const int64_t ldo, const int heads, const int Lp, const int kv_valid,
        const float scale) {
    __shared__ __attribute__((aligned(16))) char smem[4 * TS_PLANE];
    char* const skh = smem;
    char* const skl = smem + TS_PLANE;
    char* const svh = smem + 2 * TS_PLANE;
    char* const svl = smem + 3 * TS_PLANE;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = blockIdx.x / heads, h = blockIdx.x - g * heads;
    const int64_t row0 = (int64_t)g * Lp;        // first token row of the prompt
    const int col0 = 64 * h;                     // first column of the head

    // ---- the head's K and V, both planes, once: rows below kv_valid from global memory, the rest of the last key tile as zeros ----
    const int nkt_all = (kv_valid + 15) >> 4;    // key tiles that hold a valid key (<= 6: kv_valid <= Lp <= 96)
    for (int c = tid; c < nkt_all * 16 * 8; c += 256) {
        const int r = c >> 3, ch = c & 7;
        half8v kh = {0, 0, 0, 0, 0, 0, 0, 0}, kl = kh, vh = kh, vl = kh;
        if (r < kv_valid) {
            const int64_t ko = (row0 + r) * ldk + col0 + ch * 8, vo = (row0 + r) * ldv + col0 + ch * 8;
            kh = *reinterpret_cast<const half8v*>(K + ko);
            kl = *reinterpret_cast<const half8v*>(Klo + ko);
            vh = *reinterpret_cast<const half8v*>(V + vo);
            vl = *reinterpret_cast<const half8v*>(Vlo + vo);
        }
        const int off = r * TS_ROW + ch * 16;
        *reinterpret_cast<half8v*>(skh + off) = kh;
        *reinterpret_cast<half8v*>(skl + off) = kl;
        *reinterpret_cast<half8v*>(svh + off) = vh;
        *reinterpret_cast<half8v*>(svl + off) = vl;
    }
    __syncthreads();

    const int nqt = (Lp + 15) >> 4;
    const int qn = lane & 15, kg = lane >> 4;    // this lane's query inside a tile; its four keys inside a key tile are 4 kg + r
    const float sc = scale * 1.44269504088896340736f;      // exp2 domain
    // transposed V read: lane 4 q + p of a 16-lane group gives the address of key 4 kg + q, channels 4 p .. 4 p + 3 of a 16-channel block
    const int tr_off = (4 * kg + ((lane >> 2) & 3)) * TS_ROW + 8 * (lane & 3);

    for (int qt = wave; qt < nqt; qt += 4) {     // wave-uniform: every lane of a wave takes part in every transposed read
        const int nkt = min(qt + 1, nkt_all);    // key tiles up to the diagonal and up to the last valid key
        const int qi = qt * 16 + qn;             // this lane's query
        const bool qok = qi < Lp;                // (Lp % 16 == 8: the last tile is half a tile; its rows are not named)
        const int64_t qrow = row0 + (qok ? qi : Lp - 1);
        half4v qh[4], ql[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            qh[s] = *reinterpret_cast<const half4v*>(Q + qrow * ldq + col0 + s * 16 + 4 * kg);
            ql[s] = *reinterpret_cast<const half4v*>(Qlo + qrow * ldq + col0 + s * 16 + 4 * kg);
        }

        // ---- S^T = K Q^T of every visited key tile; x = scale * S in the exp2 domain, masked keys at -1e30 ----
        float x[TS_TILES][4];
        float m = -1e30f;
#pragma unroll
        for (int kt = 0; kt < TS_TILES; ++kt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) x[kt][r] = -1e30f;
            if (kt < nkt) {
                f32x4 shh = {0.f, 0.f, 0.f, 0.f}, sx = {0.f, 0.f, 0.f, 0.f};
                const int koff = (kt * 16 + qn) * TS_ROW + 8 * kg;        // key kt 16 + (lane & 15), channels 16 s + 4 kg ..
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const half4v kh = *reinterpret_cast<const half4v*>(skh + koff + 32 * s);
                    const half4v kl = *reinterpret_cast<const half4v*>(skl + koff + 32 * s);
                    shh = ts_mfma(kh, qh[s], shh);
                    sx = ts_mfma(kl, qh[s], sx);
                    sx = ts_mfma(kh, ql[s], sx);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kt * 16 + 4 * kg + r;
                    const float v = (shh[r] + sx[r] * TS_LO_INV) * sc;
                    x[kt][r] = (key <= qi && key < kv_valid) ? v : -1e30f;
                    m = fmaxf(m, x[kt][r]);
                }
            }
        }
        // the query's keys are spread over the four lanes qn, qn + 16, qn + 32, qn + 48; key 0 is attended by every query
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));

        // ---- P = exp2(x - m) as an fp16 pair against the row's maximum; O^T += V^T P^T ----
        f32x4 oh[4], ox[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) oh[cb] = ox[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        float l = 0.0f;
#pragma unroll
        for (int kt = 0; kt < TS_TILES; ++kt) {
            if (kt < nkt) {
                half4v ph, pl;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(x[kt][r] - m);          // masked: exp2(-huge) = 0
                    l += p;
                    ph[r] = (half_t)p;
                    pl[r] = (half_t)((p - (float)ph[r]) * PNC_LO_SCALE);
                }
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const int voff = kt * 16 * TS_ROW + tr_off + 32 * cb;
                    const half4v vh = __builtin_bit_cast(half4v, __builtin_amdgcn_ds_read_tr16_b64_v4f16((ts_lds_half4v*)(svh + voff)));
                    const half4v vl = __builtin_bit_cast(half4v, __builtin_amdgcn_ds_read_tr16_b64_v4f16((ts_lds_half4v*)(svl + voff)));
                    oh[cb] = ts_mfma(vh, ph, oh[cb]);
                    ox[cb] = ts_mfma(vl, ph, ox[cb]);
                    ox[cb] = ts_mfma(vh, pl, ox[cb]);
                }
            }
        }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.0f / l;              // l >= 1: the row's maximum is attended

        // ---- normalise once and store the pair: lane owns its query, channels 16 cb + 4 kg + r ----
        if (qok) {
            half_t* orow = O + qrow * ldo + col0 + 4 * kg;
            half_t* olrow = Olo + qrow * ldo + col0 + 4 * kg;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                float val[4];
                half4v hi;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    val[r] = (oh[cb][r] + ox[cb][r] * TS_LO_INV) * inv;
                    hi[r] = (half_t)val[r];
                }
                *reinterpret_cast<half4v*>(orow + 16 * cb) = hi;
                *reinterpret_cast<half4v*>(olrow + 16 * cb) = lo_plane4(val, hi);
            }
        }
    }
}

}  // namespace

extern "C" int pnc_attn_text_split_f16(const void* q, const void* q_lo, int64_t ldq, const void* k, const void* k_lo, int64_t ldk,
                                       const void* v, const void* v_lo, int64_t ldv, void* o, void* o_lo, int64_t ldo,
                                       int groups, int heads, int Lp, int kv_valid, float scale, void* stream) {
    if (!q || !q_lo || !k || !k_lo || !v || !v_lo || !o || !o_lo) return PNC_EINVAL;
    if (groups < 1 || heads < 1 || (int64_t)groups * heads > 0x7fffffff) return PNC_EINVAL;      // one workgroup per (prompt, head)
    if (Lp < 8 || Lp > TS_MAXL || Lp % 8) return PNC_EINVAL;
    if (kv_valid < 1 || kv_valid > Lp) return PNC_EINVAL;
    const int64_t W = 64 * (int64_t)heads;
    if (ldq < W || ldk < W || ldv < W || ldo < W) return PNC_EINVAL;                             // rows hold their named elements
    if (ldq % 8 || ldk % 8 || ldv % 8 || ldo % 8) return PNC_EALIGN;
    if (((uintptr_t)q | (uintptr_t)q_lo | (uintptr_t)k | (uintptr_t)k_lo | (uintptr_t)v | (uintptr_t)v_lo | (uintptr_t)o | (uintptr_t)o_lo) & 15)
        return PNC_EALIGN;
    hipLaunchKernelGGL(attn_text_split_kernel, dim3((unsigned)(groups * heads)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       f16p(q), f16p(q_lo), ldq, f16p(k), f16p(k_lo), ldk, f16p(v), f16p(v_lo), ldv, f16p(o), f16p(o_lo), ldo,
                       heads, Lp, kv_valid, scale);
    return pnc_launch_status();
}
