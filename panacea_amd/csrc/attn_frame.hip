// attn_frame.hip — fused single-head attention over the tokens of one frame, head dim C = 128 / 256 / 512 (gfx950): the mid-block
// attention of the first-stage networks (include/panacea_hip.h §6) without its N x N score matrix.
//
// With d = 512 one wave cannot hold both its Q rows and a full-width O accumulator, so the CHANNELS are split over the waves:
//   * a workgroup of 4 waves owns 64 query rows (two blocks of 32) of one frame; wave w owns channels [w C/4, (w+1) C/4);
//   * per 32-key tile every wave forms the PARTIAL S^T = K Q^T over its own slice of the contraction (Q slice in registers);
//   * the four partials meet in LDS; each wave adds them (wave 0 + 1 + 2 + 3) for 16 of the 64 rows, runs the online softmax of
//     those rows (running maximum and row sum live in that wave alone) and hands P (fp16) and the rows' rescale factors back
//     through LDS — one softmax per row, not four;
//   * each wave accumulates O^T = V^T P^T for its own C/4 output channels only (128 accumulator registers at C = 512).
// Everything is computed transposed, as in attn_views_kernel (attn.hip): one lane owns one query, K rows are fed to the MFMA in
// the order kperm() so that a lane half holds 16 consecutive keys and P is the B operand of the second product as it stands.
// K and V^T tiles arrive by LDS-DMA, one tile ahead, two stages; three barriers per tile (partials published / P published /
// stage recycled).
// Only named elements are read: K rows and V^T chunks of keys >= N come from a zero chunk, and their scores are masked by select
// AFTER the partials are added — a probability of exactly 0 would not silence a NaN, so nothing behind the last key is ever loaded.
#include "common.h"

namespace {

constexpr int FA_QT = 64;            // query rows per workgroup: two 32-query blocks, shared by the four waves
constexpr int FA_KT = 32;            // keys per tile
constexpr float FA_DEFER = 8.0f;     // exp2 domain: the accumulators are rescaled only when a row maximum rises by more (P <= 2^8)
constexpr int FA_XCH = 4 * 2 * 16 * 64 * 4;      // the partial scores of 4 waves x 2 query blocks x 16 registers x 64 lanes, fp32

__device__ __forceinline__ int fa_kperm(int i) { return 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3); }

__device__ __attribute__((aligned(16))) half_t g_frame_zero_chunk[8];   // zero-initialised: DMA source of chunks behind the last key

// LDS images of a stage.  K tile: 32 rows (keys) of C fp16, the 16-byte chunk index XORed with (row & 15): the 16 lanes of a
// ds_read_b128 group read one logical chunk of 16 rows whose (row & 15) differ (kperm order) -> 16 distinct slots of the 256-byte
// bank row.  V^T tile: C rows (channels) of 32 keys = 4 chunks, chunk index XORed with ((row >> 2) & 3): a group's 16 rows are four
// runs of 4 with distinct (row >> 2) & 3.  The DMA image of a wave instruction is lane-linear (1 KB), so the XOR is applied to the
// SOURCE chunk.
template <int C>
__global__ __launch_bounds__(256, 1) void attn_frame_kernel(const half_t* __restrict__ Q, const int64_t ldq, const half_t* __restrict__ K,
                                                           const int64_t ldk, const half_t* __restrict__ VT, const int64_t ldvt,
                                                           const int64_t vt_fstride, half_t* __restrict__ O, const int64_t ldo,
                                                           const int N, const int nqt, const float scale) {
    constexpr int CW = C / 4;                    // channels per wave
    constexpr int KS = CW / 16;                  // k-steps of the partial K Q^T
    constexpr int DB = CW / 32;                  // 32-channel blocks of the wave's O^T
    constexpr int CPR = C / 8;                   // 16-byte chunks per K row
    constexpr int TILE = FA_KT * C * 2;          // bytes of a K tile, and of a V^T tile
    constexpr int STAGE = 2 * TILE;
    constexpr int DMA_PER_WAVE = C / 64;         // 1-KB DMA instructions per wave, tile and operand
    static_assert(2 * STAGE + FA_XCH <= 160 * 1024, "attn_frame_kernel: LDS beyond 160 KB");
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE + FA_XCH];
    char* const xch = smem + 2 * STAGE;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = lane >> 5, frow = lane & 31;
    // the query tiles of one frame read the same K / V^T: consecutive virtual ids inside one XCD (as attn_views_kernel)
    const int vb = xcd_remap(blockIdx.x, gridDim.x);
    const int f = vb / nqt, qtile = vb - f * nqt;
    const half_t* __restrict__ Qf = Q + (int64_t)f * N * ldq;
    const half_t* __restrict__ Kf = K + (int64_t)f * N * ldk;
    const half_t* __restrict__ VTf = VT + (int64_t)f * vt_fstride;
    half_t* __restrict__ Of = O + (int64_t)f * N * ldo;

    // ---- this lane's two queries (columns of S^T / O^T) and the wave's channel slice of their rows ----
    bool qok[2];
    int64_t qrow[2];
    half8v qf[2][KS];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const int ql = qtile * FA_QT + qb * 32 + frow;
        qok[qb] = ql < N;
        qrow[qb] = qok[qb] ? ql : N - 1;
#pragma unroll
        for (int ds = 0; ds < KS; ++ds)
            qf[qb][ds] = *reinterpret_cast<const half8v*>(Qf + qrow[qb] * ldq + wave * CW + ds * 16 + grp * 8);
    }

    auto dma_tile = [&](int t, int stage) {
        const int key0 = t * FA_KT;
        char* sk = smem + stage * STAGE;
        char* sv = sk + TILE;
#pragma unroll
        for (int ii = 0; ii < DMA_PER_WAVE; ++ii) {
            const int i = wave * DMA_PER_WAVE + ii;
            const int g = i * 64 + lane;                       // physical chunk of the tile image
            {   // K: row = key, chunk = 8 channels
                const int kr = g / CPR, lc = (g % CPR) ^ (kr & 15);
                const int key = key0 + kr;
                const half_t* src = key < N ? Kf + (int64_t)key * ldk + lc * 8 : g_frame_zero_chunk;
                glds16(src, sk + i * 1024);
            }
            {   // V^T: row = channel, chunk = 8 consecutive keys (N % 8 == 0: a chunk is whole or absent)
                const int d = g >> 2, lc = (g & 3) ^ ((d >> 2) & 3);
                const int kc = key0 + lc * 8;
                const half_t* src = kc < N ? VTf + (int64_t)d * ldvt + kc : g_frame_zero_chunk;
                glds16(src, sv + i * 1024);
            }
        }
    };

    f32x16 oacc[2][DB];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[qb][db][r] = 0.0f;
    // softmax ownership: wave w forms P for 16 of the 64 rows — query block w >> 1, columns 16 (w & 1) .. + 15 — with lane = (column,
    // kq = group of 8 keys); (kq >> 1, column) is the lane of the S^T / P^T fragments that holds those keys, kq & 1 the k-step
    const int oqb = wave >> 1, kq = lane >> 4, oss = kq & 1;
    const int oslot = (((kq >> 1) << 5) | (16 * (wave & 1) + (lane & 15))) * 16;
    float mrun = -1e30f, lrun = 0.0f;          // of this lane's row; lrun over the lane's own keys
    const float sc = scale * 1.44269504088896340736f;   // exp2 domain
    const int ntiles = (N + FA_KT - 1) / FA_KT;

    dma_tile(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    const int krow = fa_kperm(frow);
    for (int t = 0; t < ntiles; ++t) {
        if (t + 1 < ntiles) dma_tile(t + 1, (t + 1) & 1);
        const char* sk = smem + (t & 1) * STAGE;
        const char* sv = sk + TILE;
        const int key0 = t * FA_KT;

        // ---- partial S^T = K Q^T over this wave's channels; every K fragment feeds both query blocks ----
        f32x16 s[2];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[qb][r] = 0.0f;
#pragma unroll
        for (int ds = 0; ds < KS; ++ds) {
            const half8v kf = *reinterpret_cast<const half8v*>(sk + krow * (C * 2) + (((wave * (CW / 8) + 2 * ds + grp) ^ (krow & 15)) << 4));
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) s[qb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[qb][ds], s[qb], 0, 0, 0);
        }
        // ---- the four partials meet in LDS ----
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4)
                *reinterpret_cast<f32x4*>(xch + ((wave * 2 + qb) * 4 + r4) * 1024 + lane * 16) =
                    f32x4{s[qb][4 * r4], s[qb][4 * r4 + 1], s[qb][4 * r4 + 2], s[qb][4 * r4 + 3]};
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");

        // ---- this wave's quarter of the scores = partial 0 + 1 + 2 + 3, online softmax of its 16 rows; lane holds keys key0 + 8 kq + j ----
        {
            float x[8];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                f32x4 a = *reinterpret_cast<const f32x4*>(xch + ((0 * 2 + oqb) * 4 + 2 * oss + e) * 1024 + oslot);
#pragma unroll
                for (int w = 1; w < 4; ++w) a += *reinterpret_cast<const f32x4*>(xch + ((w * 2 + oqb) * 4 + 2 * oss + e) * 1024 + oslot);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[4 * e + j] = a[j] * sc;
            }
            if (key0 + FA_KT > N) {          // the last, partial tile: keys at or beyond N do not exist
                int lim = N - key0 - kq * 8;
                asm volatile("" : "+v"(lim));          // (kept opaque: the compare chain stays inside the branch)
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j >= lim) x[j] = -1e30f;
            }
            float tmax = -1e30f;
#pragma unroll
            for (int j = 0; j < 8; ++j) tmax = fmaxf(tmax, x[j]);
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            // the first tile always moves the maximum (mrun starts at -1e30); later ones only when the row's maximum rose by more than
            // FA_DEFER: until then alpha is exactly 1 and P <= 2^FA_DEFER
            const float mnew = tmax > mrun + FA_DEFER ? tmax : mrun;
            const float alpha = __builtin_amdgcn_exp2f(mrun - mnew);
            mrun = mnew;
            float psum = 0.0f;
            half8v p8;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float pv = __builtin_amdgcn_exp2f(x[j] - mrun);      // masked: exp2(-huge) = 0
                psum += pv;
                p8[j] = (half_t)pv;
            }
            lrun = lrun * alpha + psum;
            // P and alpha go where this wave's own quarter of wave 0's partials was (registers 0 .. 11 of its lanes' slots): nobody
            // else reads those, and this wave's reads above are complete
            *reinterpret_cast<half8v*>(xch + (oqb * 4 + oss) * 1024 + oslot) = p8;
            *reinterpret_cast<float*>(xch + (oqb * 4 + 2) * 1024 + oslot + oss * 4) = alpha;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");

        // ---- every wave takes all of P (the B operand as it stands) and the rows' rescale factors ----
        half8v pf[2][2];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) pf[qb][ss] = *reinterpret_cast<const half8v*>(xch + (qb * 4 + ss) * 1024 + lane * 16);
            const float alpha = *reinterpret_cast<const float*>(xch + (qb * 4 + 2) * 1024 + lane * 16);
            if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
                for (int db = 0; db < DB; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[qb][db][r] *= alpha;
            }
        }

        // ---- O^T += V^T P^T for this wave's channels; every V^T fragment feeds both query blocks ----
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const int d = wave * CW + db * 32 + frow;
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const half8v vf = *reinterpret_cast<const half8v*>(sv + d * 64 + (((2 * grp + ss) ^ ((d >> 2) & 3)) << 4));
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) oacc[qb][db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[qb][ss], oacc[qb][db], 0, 0, 0);
            }
        }
        // tile t + 1 has landed; the barrier publishes every wave's part of it and retires all reads of this stage and of the partials
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }

    // ---- normalise once and store: lane owns its queries, channels wave * CW + 32 db + mfma32_row(r, lane) ----
    {
        float ltot = lrun + __shfl_xor(lrun, 16, 64);
        ltot += __shfl_xor(ltot, 32, 64);
        *reinterpret_cast<float*>(xch + (oqb * 4 + 3) * 1024 + oslot + oss * 4) = ltot > 0.0f ? 1.0f / ltot : 0.0f;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const float inv = *reinterpret_cast<const float*>(xch + (qb * 4 + 3) * 1024 + lane * 16);
        half_t* orow = Of + qrow[qb] * ldo + wave * CW;
        // one xor-32 exchange per pair of r4 gives each lane 8 consecutive channels: 16-byte stores (attn_views_kernel's epilogue)
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int rp = 0; rp < 2; ++rp) {
                half4v he, ho;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    he[q] = (half_t)(oacc[qb][db][(2 * rp) * 4 + q] * inv);
                    ho[q] = (half_t)(oacc[qb][db][(2 * rp + 1) * 4 + q] * inv);
                }
                union { half4v h; int2 i; } snd, rcv;
                snd.h = grp ? he : ho;
                rcv.i.x = __shfl_xor(snd.i.x, 32, 64);
                rcv.i.y = __shfl_xor(snd.i.y, 32, 64);
                half8v o8;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    o8[q] = grp ? rcv.h[q] : he[q];
                    o8[4 + q] = grp ? ho[q] : rcv.h[q];
                }
                if (qok[qb]) *reinterpret_cast<half8v*>(orow + db * 32 + 8 * (2 * rp + grp)) = o8;
            }
    }
}

template <int C>
void launch_frame(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt, int64_t vt_fstride, void* o,
                  int64_t ldo, int F, int N, float scale, hipStream_t st) {
    const int nqt = (N + FA_QT - 1) / FA_QT;
    hipLaunchKernelGGL(attn_frame_kernel<C>, dim3((unsigned)F * (unsigned)nqt), dim3(256), 0, st, f16p(q), ldq, f16p(k), ldk, f16p(vt), ldvt,
                       vt_fstride, f16p(o), ldo, N, nqt, scale);
}

}  // namespace

extern "C" int pnc_attn_frame_f16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt,
                                  int64_t vt_fstride, void* o, int64_t ldo, int F, int N, int C, float scale, void* stream) {
    if (!q || !k || !vt || !o) return PNC_EINVAL;
    if (C != 128 && C != 256 && C != 512) return PNC_EINVAL;
    if (F < 1 || N < 8 || N % 8) return PNC_EINVAL;
    if ((int64_t)F * (((int64_t)N + FA_QT - 1) / FA_QT) > 0x7fffffff) return PNC_EINVAL;      // one workgroup per 64 queries of a frame
    if (ldq < C || ldk < C || ldo < C || ldvt < N || vt_fstride < 0) return PNC_EINVAL;       // rows hold their named elements
    if (ldq % 8 || ldk % 8 || ldo % 8 || ldvt % 8 || vt_fstride % 8) return PNC_EALIGN;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)o) & 15) return PNC_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (C) {
        case 128: launch_frame<128>(q, ldq, k, ldk, vt, ldvt, vt_fstride, o, ldo, F, N, scale, st); break;
        case 256: launch_frame<256>(q, ldq, k, ldk, vt, ldvt, vt_fstride, o, ldo, F, N, scale, st); break;
        default: launch_frame<512>(q, ldq, k, ldk, vt, ldvt, vt_fstride, o, ldo, F, N, scale, st);
    }
    return pnc_launch_status();
}
