// attn_frame_split.hip — the fused single-head frame attention of attn_frame.hip on SPLIT operands (include/panacea_hip.h §6b):
// q, k, v and o are fp16 pairs x ~ hi + 2^-11 lo, V is read ROW-major (laid out like K: what the QKV GEMM writes as out16 + out16_lo).
//
//   S = Qh.Kh + 2^-11 (Qh.Kl + Ql.Kh)        P = Ph + 2^-11 Pl        O = Ph.Vh + 2^-11 (Ph.Vl + Pl.Vh)
//
// The hi.hi products and the cross products accumulate in separate fp32 registers and meet once, scaled by 2^-11, in fp32 (as
// attn_split.hip does) — three MFMAs per product of the single-plane kernel.
//
// Form.  Split operands double the operand bytes, so attn_frame_kernel's two stages of K and V^T tiles do not fit: ONE resident
// set {K hi, K lo, V hi, V lo} of 32-key tiles (4 x 32 KB at C = 512) whose K half and V half are recycled independently —
//   * K(t + 1) is fetched by LDS-DMA as soon as the scores of tile t are formed, and lands under the softmax and the P V products;
//   * V(t + 1) is fetched as soon as the P V products of tile t are done, and lands under the scores of tile t + 1 —
// so a DMA is in flight under every MFMA phase.  The channels are split over the four waves as in attn_frame_kernel (wave w owns
// channels [w C/4, (w+1) C/4) of the contraction and of the output), but a workgroup owns ONE block of 32 queries: Q hi + lo and the
// two sets of O accumulators of a second block would not fit the register file at C = 512.  The four partial score tiles meet in LDS
// (16 KB); every wave adds them in the same order (wave 0 + 1 + 2 + 3) and runs the online softmax of all 32 rows itself — the same
// bits in every wave, and P^T is the B operand of the second product as it stands (key order fs_kperm), so there is no second
// exchange: three barriers per tile (partials published and K half free / V landed / V half and partials free, K landed).
// V is transposed on its way to the MFMA by ds_read_b64_tr_b16: a 16-lane group reads 4 keys x 16 channels of the row-major tile
// and receives them channel-major (attn_temporal_wide_kernel in attn.hip reads its V the same way).
// Only named elements are read: K / V rows of keys >= N come from a zero chunk, and their scores are masked by select AFTER the
// partials are added — a probability of exactly 0 would not silence a NaN, so nothing behind the last key is ever loaded.
#include "common.h"

namespace {

constexpr int FS_QT = 32;            // query rows per workgroup, shared by the four waves
constexpr int FS_KT = 32;            // keys per tile
constexpr float FS_DEFER = 8.0f;     // exp2 domain: the accumulators are rescaled only when a row maximum rises by more (P <= 2^8)
constexpr int FS_XCH = 4 * 16 * 64 * 4;          // the partial scores of 4 waves x 16 registers x 64 lanes, fp32
constexpr float FS_LO_INV = 1.0f / PNC_LO_SCALE;

__device__ __forceinline__ int fs_kperm(int i) { return 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3); }

__device__ __attribute__((aligned(16))) half_t g_frame_split_zero_chunk[8];   // zero-initialised: DMA source of rows behind the last key

typedef __fp16 fs_tr_half4v __attribute__((__vector_size__(4 * sizeof(__fp16))));      // ds_read_tr16_b64's own vector type
typedef __attribute__((address_space(3))) fs_tr_half4v fs_lds_half4v;

template <int NW>
__device__ __forceinline__ void fs_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW) : "memory"); }

// LDS images.  K tile (hi, lo): 32 rows (keys) of C fp16, the 16-byte chunk index XORed with (row & 15) — attn_frame_kernel's K
// image.  V tile (hi, lo): 32 rows (keys) of C fp16, chunk index XORed with 4 (row & 3): the 32 lanes of a transposed read touch
// the same four chunks (64 bytes) of four consecutive keys, which the XOR spreads over the four 64-byte quarters of the 256-byte
// bank row.  The DMA image of a wave instruction is lane-linear (1 KB), so either XOR is applied to the SOURCE chunk.
template <int C>
__global__ __launch_bounds__(256, 1) void attn_frame_split_kernel(
        const half_t* __restrict__ Q, const half_t* __restrict__ Qlo, const int64_t ldq, const half_t* __restrict__ K,
        const half_t* __restrict__ Klo, const int64_t ldk, const half_t* __restrict__ V, const half_t* __restrict__ Vlo, const int64_t ldv,
        half_t* __restrict__ O, half_t* __restrict__ Olo, const int64_t ldo, const int N, const int nqt, const float scale) {
    constexpr int CW = C / 4;                    // channels per wave
    constexpr int KS = CW / 16;                  // k-steps of the partial K Q^T
    constexpr int DB = CW / 32;                  // 32-channel blocks of the wave's O^T
    constexpr int CPR = C / 8;                   // 16-byte chunks per K / V row
    constexpr int TILE = FS_KT * C * 2;          // bytes of one plane of a K tile, and of a V tile
    constexpr int DMA_PER_WAVE = C / 64;         // 1-KB DMA instructions per wave, tile and plane
    constexpr int DMA_PAIR = 2 * DMA_PER_WAVE;   // ... per wave and operand (hi + lo): what one dma_k / dma_v leaves in flight
    static_assert(4 * TILE + FS_XCH <= 160 * 1024, "attn_frame_split_kernel: LDS beyond 160 KB");
    static_assert(DMA_PAIR <= 32, "attn_frame_split_kernel: the counted vmcnt wait");
    __shared__ __attribute__((aligned(16))) char smem[4 * TILE + FS_XCH];
    char* const skh = smem;
    char* const skl = smem + TILE;
    char* const svh = smem + 2 * TILE;
    char* const svl = smem + 3 * TILE;
    char* const xch = smem + 4 * TILE;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = lane >> 5, frow = lane & 31;
    // the query tiles of one frame read the same K / V: consecutive virtual ids inside one XCD (as attn_frame_kernel)
    const int vb = xcd_remap(blockIdx.x, gridDim.x);
    const int f = vb / nqt, qtile = vb - f * nqt;
    const half_t* __restrict__ Kf = K + (int64_t)f * N * ldk;
    const half_t* __restrict__ Klf = Klo + (int64_t)f * N * ldk;
    const half_t* __restrict__ Vf = V + (int64_t)f * N * ldv;
    const half_t* __restrict__ Vlf = Vlo + (int64_t)f * N * ldv;

    // ---- this lane's query (a column of S^T / O^T) and the wave's channel slice of its row, both planes ----
    const int ql = qtile * FS_QT + frow;
    const bool qok = ql < N;
    const int64_t qrow = (int64_t)f * N + (qok ? ql : N - 1);
    half8v qh[KS], qlo[KS];
#pragma unroll
    for (int ds = 0; ds < KS; ++ds) {
        qh[ds] = *reinterpret_cast<const half8v*>(Q + qrow * ldq + wave * CW + ds * 16 + grp * 8);
        qlo[ds] = *reinterpret_cast<const half8v*>(Qlo + qrow * ldq + wave * CW + ds * 16 + grp * 8);
    }

    auto dma_k = [&](int t) {
        const int key0 = t * FS_KT;
#pragma unroll
        for (int ii = 0; ii < DMA_PER_WAVE; ++ii) {
            const int i = wave * DMA_PER_WAVE + ii;
            const int g = i * 64 + lane;                       // physical chunk of the tile image
            const int kr = g / CPR, lc = (g % CPR) ^ (kr & 15);
            const int key = key0 + kr;
            const int64_t off = (int64_t)key * ldk + lc * 8;
            glds16(key < N ? Kf + off : g_frame_split_zero_chunk, skh + i * 1024);
            glds16(key < N ? Klf + off : g_frame_split_zero_chunk, skl + i * 1024);
        }
    };
    auto dma_v = [&](int t) {
        const int key0 = t * FS_KT;
#pragma unroll
        for (int ii = 0; ii < DMA_PER_WAVE; ++ii) {
            const int i = wave * DMA_PER_WAVE + ii;
            const int g = i * 64 + lane;
            const int kr = g / CPR, lc = (g % CPR) ^ ((kr & 3) << 2);
            const int key = key0 + kr;
            const int64_t off = (int64_t)key * ldv + lc * 8;
            glds16(key < N ? Vf + off : g_frame_split_zero_chunk, svh + i * 1024);
            glds16(key < N ? Vlf + off : g_frame_split_zero_chunk, svl + i * 1024);
        }
    };

    f32x16 oh[DB], ox[DB];                       // O^T: hi.hi products / cross products
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) oh[db][r] = ox[db][r] = 0.0f;
    float mrun = -1e30f, lrun = 0.0f;            // of this lane's query; lrun over the lane's own 16 keys of every tile
    const float sc = scale * 1.44269504088896340736f;   // exp2 domain
    const int ntiles = (N + FS_KT - 1) / FS_KT;

    dma_k(0);
    dma_v(0);
    fs_wait_vm<DMA_PAIR>();                      // K(0) has landed; V(0) may still be in flight
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    const int krow = fs_kperm(frow);
    // transposed V read: lane 4 q + p of a 16-lane group gives the address of key 4 j + q, channels 4 p .. 4 p + 3 of the group's 16
    const int tq = (lane >> 2) & 3;
    const int tcol = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);      // first of the lane's 4 channels inside a 32-channel block
    for (int t = 0; t < ntiles; ++t) {
        const int key0 = t * FS_KT;
        const bool more = t + 1 < ntiles;

        // ---- partial S^T = K Q^T over this wave's channels: hi.hi and the two cross products ----
        f32x16 shh, sx;
#pragma unroll
        for (int r = 0; r < 16; ++r) shh[r] = sx[r] = 0.0f;
#pragma unroll
        for (int ds = 0; ds < KS; ++ds) {
            const int off = krow * (C * 2) + (((wave * (CW / 8) + 2 * ds + grp) ^ (krow & 15)) << 4);
            const half8v kh = *reinterpret_cast<const half8v*>(skh + off);
            const half8v kl = *reinterpret_cast<const half8v*>(skl + off);
            shh = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[ds], shh, 0, 0, 0);
            sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[ds], sx, 0, 0, 0);
            sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qlo[ds], sx, 0, 0, 0);
        }
        // ---- the four partials meet in LDS ----
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            f32x4 pv;
#pragma unroll
            for (int j = 0; j < 4; ++j) pv[j] = shh[4 * r4 + j] + sx[4 * r4 + j] * FS_LO_INV;
            *reinterpret_cast<f32x4*>(xch + (wave * 4 + r4) * 1024 + lane * 16) = pv;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (more) dma_k(t + 1);                  // the K half is free: every wave has formed its scores

        // ---- all 32 rows in every wave: scores = partial 0 + 1 + 2 + 3; this lane holds keys key0 + 16 grp + r of its query ----
        float x[16];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            f32x4 a = *reinterpret_cast<const f32x4*>(xch + (0 * 4 + r4) * 1024 + lane * 16);
#pragma unroll
            for (int w = 1; w < 4; ++w) a += *reinterpret_cast<const f32x4*>(xch + (w * 4 + r4) * 1024 + lane * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) x[4 * r4 + j] = a[j] * sc;
        }
        if (key0 + FS_KT > N) {                  // the last, partial tile: keys at or beyond N do not exist
            int lim = N - key0 - grp * 16;
            asm volatile("" : "+v"(lim));        // (kept opaque: the compare chain stays inside the branch)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (r >= lim) x[r] = -1e30f;
        }
        float tmax = -1e30f;
#pragma unroll
        for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, x[r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        // the first tile always moves the maximum (mrun starts at -1e30); later ones only when the row's maximum rose by more than
        // FS_DEFER: until then alpha is exactly 1 and P <= 2^FS_DEFER
        const float mnew = tmax > mrun + FS_DEFER ? tmax : mrun;
        const float alpha = __builtin_amdgcn_exp2f(mrun - mnew);
        mrun = mnew;
        float psum = 0.0f;
        half8v ph[2], pl[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float pv = __builtin_amdgcn_exp2f(x[r] - mrun);          // masked: exp2(-huge) = 0
            psum += pv;
            const half_t h = (half_t)pv;
            ph[r >> 3][r & 7] = h;
            pl[r >> 3][r & 7] = (half_t)((pv - (float)h) * PNC_LO_SCALE);
        }
        lrun = lrun * alpha + psum;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    oh[db][r] *= alpha;
                    ox[db][r] *= alpha;
                }
        }
        // V(t) was issued ahead of K(t + 1): all but the newest DMA_PAIR instructions of this wave have landed
        if (more) fs_wait_vm<DMA_PAIR>();
        else fs_wait_vm<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");

        // ---- O^T += V^T P^T for this wave's channels, V transposed by the read: keys key0 + 16 grp + 8 ss + j, j = 0 .. 7 ----
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const int ch = wave * CW + db * 32 + tcol;
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                half8v vh, vl;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int kr = 16 * grp + 8 * ss + 4 * e + tq;
                    const int off = kr * (C * 2) + (((ch >> 3) ^ ((kr & 3) << 2)) << 4) + ((ch & 7) << 1);
                    const half4v a = __builtin_bit_cast(half4v, __builtin_amdgcn_ds_read_tr16_b64_v4f16((fs_lds_half4v*)(svh + off)));
                    const half4v b = __builtin_bit_cast(half4v, __builtin_amdgcn_ds_read_tr16_b64_v4f16((fs_lds_half4v*)(svl + off)));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        vh[4 * e + j] = a[j];
                        vl[4 * e + j] = b[j];
                    }
                }
                oh[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph[ss], oh[db], 0, 0, 0);
                ox[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph[ss], ox[db], 0, 0, 0);
                ox[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl[ss], ox[db], 0, 0, 0);
            }
        }
        // K(t + 1) has landed; the barrier publishes every wave's part of it and retires all reads of the V half and of the partials
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (more) dma_v(t + 1);
    }

    // ---- normalise once and store the pair: lane owns its query, channels wave * CW + 32 db + mfma32_row(r, lane) ----
    const float ltot = lrun + __shfl_xor(lrun, 32, 64);
    const float inv = ltot > 0.0f ? 1.0f / ltot : 0.0f;
    if (qok) {
        half_t* orow = O + qrow * ldo + wave * CW;
        half_t* olrow = Olo + qrow * ldo + wave * CW;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                float val[4];
                half4v hi;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    val[j] = (oh[db][4 * r4 + j] + ox[db][4 * r4 + j] * FS_LO_INV) * inv;
                    hi[j] = (half_t)val[j];
                }
                const int c = db * 32 + 8 * r4 + 4 * grp;
                *reinterpret_cast<half4v*>(orow + c) = hi;
                *reinterpret_cast<half4v*>(olrow + c) = lo_plane4(val, hi);
            }
    }
}

template <int C>
void launch_frame_split(const void* q, const void* q_lo, int64_t ldq, const void* k, const void* k_lo, int64_t ldk, const void* v,
                        const void* v_lo, int64_t ldv, void* o, void* o_lo, int64_t ldo, int F, int N, float scale, hipStream_t st) {
    const int nqt = (N + FS_QT - 1) / FS_QT;
    hipLaunchKernelGGL(attn_frame_split_kernel<C>, dim3((unsigned)F * (unsigned)nqt), dim3(256), 0, st, f16p(q), f16p(q_lo), ldq, f16p(k),
                       f16p(k_lo), ldk, f16p(v), f16p(v_lo), ldv, f16p(o), f16p(o_lo), ldo, N, nqt, scale);
}

}  // namespace

extern "C" int pnc_attn_frame_split_f16(const void* q, const void* q_lo, int64_t ldq, const void* k, const void* k_lo, int64_t ldk,
                                        const void* v, const void* v_lo, int64_t ldv, void* o, void* o_lo, int64_t ldo,
                                        int F, int N, int C, float scale, void* stream) {
    if (!q || !q_lo || !k || !k_lo || !v || !v_lo || !o || !o_lo) return PNC_EINVAL;
    if (C != 128 && C != 256 && C != 512) return PNC_EINVAL;
    if (F < 1 || N < 8 || N % 8) return PNC_EINVAL;
    if ((int64_t)F * (((int64_t)N + FS_QT - 1) / FS_QT) > 0x7fffffff) return PNC_EINVAL;      // one workgroup per 32 queries of a frame
    if (ldq < C || ldk < C || ldv < C || ldo < C) return PNC_EINVAL;                          // rows hold their named elements
    if (ldq % 8 || ldk % 8 || ldv % 8 || ldo % 8) return PNC_EALIGN;
    if (((uintptr_t)q | (uintptr_t)q_lo | (uintptr_t)k | (uintptr_t)k_lo | (uintptr_t)v | (uintptr_t)v_lo | (uintptr_t)o | (uintptr_t)o_lo) & 15)
        return PNC_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (C) {
        case 128: launch_frame_split<128>(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, o, o_lo, ldo, F, N, scale, st); break;
        case 256: launch_frame_split<256>(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, o, o_lo, ldo, F, N, scale, st); break;
        default: launch_frame_split<512>(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, o, o_lo, ldo, F, N, scale, st);
    }
    return pnc_launch_status();
}
