// image.hip — the 8-bit image boundary of the per-sample path (include/panacea_hip.h section 9): uint8 channels-last frames ->
// the fp16 token planes the first convs read, and the decoder's fp32 token matrix -> uint8 channels-last frames.  Both kernels
// only move data: the scaling of the input side is a 256-entry table the host builds with the reference's own numpy expressions
// (nuscenes_datasets_video.py:542-552), the quantiser of the output side is inference.py:189-193 per element.
#include "common.h"

namespace {

// ---- uint8 [P][C] -> fp16 [P][Cpad] (+ lo plane) through a table ----------------------------------------------------------------
// Chosen form.  A pixel of C bytes (19 for the BEV layout) starts at every offset of a 16-byte chunk, so no lane can own "its"
// pixel with aligned vector loads.  A workgroup therefore copies the contiguous byte run of a tile of pixels into LDS with aligned
// 16-byte loads (the run's first and last chunk are the only ones that can reach outside the array: those two are assembled from
// guarded byte loads, everything else is one dwordx4 per lane), and then works per (pixel, 8-channel chunk): three aligned LDS
// dwords around the chunk's first byte, a funnel shift to the byte offset, eight lookups in the (hi, lo) table the workgroup
// expanded once, one 16-byte store per plane.  Consecutive lanes own consecutive 16-byte chunks of the output, so every store
// instruction of a wave writes 1 KiB contiguously; the thread-per-pixel form of nchw_to_tokens_kernel writes 16 bytes per lane at a
// stride of 2 Cpad bytes.  The kernel has no arithmetic besides the table expansion, which is nchw_to_tokens_kernel's.
constexpr int U8_STAGE = 16384;                    // LDS bytes of a tile's byte run, head misalignment included
constexpr int U8_MAX_C = 4096;                     // widest pixel: four of them still fit a tile
constexpr int U8_MAX_TILE_PIX = 2048;

__global__ __launch_bounds__(256) void u8_to_tokens_kernel(const uint8_t* __restrict__ src, const float* __restrict__ lut,
                                                           int64_t P, int C, int Cpad, int tile_pix,
                                                           half_t* __restrict__ out, half_t* __restrict__ out_lo) {
    __shared__ uint32_t pair[256];                                       // fp16 bits: hi | lo << 16
    __shared__ __attribute__((aligned(16))) uint8_t stage[U8_STAGE + 16];
    const int tid = threadIdx.x;
    {
        const float v = lut[tid];
        const half_t h = (half_t)v;
        const half_t l = (half_t)((v - (float)h) * PNC_LO_SCALE);
        pair[tid] = (uint32_t)__builtin_bit_cast(uint16_t, h) | ((uint32_t)__builtin_bit_cast(uint16_t, l) << 16);
    }
    const int nchunk = Cpad >> 3;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), s1 = s0 + (uint64_t)P * C;
    const int64_t ntile = (P + tile_pix - 1) / tile_pix;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t pix0 = tile * tile_pix;
        const int npx = (int)min((int64_t)tile_pix, P - pix0);
        const uintptr_t a0 = s0 + (uint64_t)pix0 * C;
        const int head = (int)(a0 & 15);
        const uintptr_t base = a0 - head;                                // aligned down: may lie up to 15 bytes before src
        const int nld = (head + npx * C + 15) >> 4;                      // <= U8_STAGE / 16 (the host sizes tile_pix for it)
        __syncthreads();                                                 // the table is written / the previous tile is consumed
        for (int k = tid; k < nld; k += 256) {
            const uintptr_t g = base + 16 * (uintptr_t)k;
            uint4 w;
            if (g >= s0 && g + 16 <= s1) {
                w = *reinterpret_cast<const uint4*>(g);
            } else {                                                     // the array's first / last chunk: only bytes inside it
                uint32_t q[4] = {0u, 0u, 0u, 0u};
                for (int b = 0; b < 16; ++b) {
                    const uintptr_t a = g + b;
                    if (a >= s0 && a < s1) q[b >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(a) << (8 * (b & 3));
                }
                w = make_uint4(q[0], q[1], q[2], q[3]);
            }
            *reinterpret_cast<uint4*>(stage + 16 * k) = w;
        }
        __syncthreads();
        const int items = npx * nchunk;
        for (int j = tid; j < items; j += 256) {
            const int p = j / nchunk, c0 = (j - p * nchunk) * 8;
            uint4 h = make_uint4(0u, 0u, 0u, 0u), l = h;                 // channels C .. Cpad - 1: +0 in both planes
            if (c0 < C) {
                const int o = head + p * C + c0;                         // o < head + npx * C: the three dwords end inside `stage`
                const uint32_t* wp = reinterpret_cast<const uint32_t*>(stage + (o & ~3));
                const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2];
                const int sh = (o & 3) * 8;
                const uint32_t by[2] = {(uint32_t)((((uint64_t)w1 << 32) | w0) >> sh), (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh)};
                uint32_t pr[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint32_t v = pair[(by[e >> 2] >> (8 * (e & 3))) & 255u];
                    pr[e] = (c0 + e < C) ? v : 0u;                       // bytes past the pixel belong to the next one (or to nobody)
                }
                h = make_uint4((pr[0] & 0xffffu) | (pr[1] << 16), (pr[2] & 0xffffu) | (pr[3] << 16),
                               (pr[4] & 0xffffu) | (pr[5] << 16), (pr[6] & 0xffffu) | (pr[7] << 16));
                l = make_uint4((pr[0] >> 16) | (pr[1] & 0xffff0000u), (pr[2] >> 16) | (pr[3] & 0xffff0000u),
                               (pr[4] >> 16) | (pr[5] & 0xffff0000u), (pr[6] >> 16) | (pr[7] & 0xffff0000u));
            }
            const int64_t at = (pix0 + p) * Cpad + c0;
            *reinterpret_cast<uint4*>(out + at) = h;
            if (out_lo) *reinterpret_cast<uint4*>(out_lo + at) = l;
        }
    }
}

// ---- fp32 tokens [M][ld] (first C columns) -> uint8 [M][C] ----------------------------------------------------------------------
// inference.py:189-193 per element, every operation rounded on its own in that order: clamp to [-1, 1], (t + 1) / 2 (the halving
// is exact, so * 0.5f gives the division's bits), * 255, truncation.  NaN -> 0, a stated choice (numpy's cast of NaN is undefined).
__device__ __forceinline__ uint32_t quantise_u8(float x) {
#pragma clang fp contract(off)
    float t = fminf(fmaxf(x, -1.0f), 1.0f);
    t = (t + 1.0f) * 0.5f;
    t = t * 255.0f;
    return x == x ? (uint32_t)(int)t : 0u;
}

// ld == C: the matrix is one float stream of n elements.  A thread owns 4 consecutive floats (one 16-byte load, a wave reads 1 KiB
// per instruction) and writes them as one dword; the last n % 4 elements are written bytewise by the thread that owns them.
__global__ __launch_bounds__(256) void tokens_to_u8_stream_kernel(const float* __restrict__ x, int64_t n, uint8_t* __restrict__ out) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 4 <= n) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + i);
        *reinterpret_cast<uint32_t*>(out + i) = quantise_u8(v[0]) | (quantise_u8(v[1]) << 8) | (quantise_u8(v[2]) << 16) |
                                                (quantise_u8(v[3]) << 24);
    } else {
        for (int64_t e = i; e < n; ++e) out[e] = (uint8_t)quantise_u8(x[e]);
    }
}

// any ld >= C (and any 4-byte aligned x): a thread still owns 4 consecutive OUTPUT bytes, each read from its own (row, column)
__global__ __launch_bounds__(256) void tokens_to_u8_rows_kernel(const float* __restrict__ x, int ld, int64_t n, int C,
                                                                uint8_t* __restrict__ out) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    int64_t m = i / C;
    int c = (int)(i - m * C);
    uint32_t q[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        q[e] = i + e < n ? quantise_u8(x[m * ld + c]) : 0u;
        if (++c == C) { c = 0; ++m; }
    }
    if (i + 4 <= n) {
        *reinterpret_cast<uint32_t*>(out + i) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    } else {
        for (int e = 0; i + e < n; ++e) out[i + e] = (uint8_t)q[e];
    }
}

inline hipStream_t hip_stream(void* stream) { return reinterpret_cast<hipStream_t>(stream); }

}  // namespace

extern "C" int pnc_u8_to_tokens_f16(const uint8_t* src, const float* lut, int F, int Npix, int C, int Cpad, void* out16,
                                    void* out16_lo, void* stream) {
    if (!src || !lut || !out16 || F < 1 || Npix < 1 || C < 1 || C > U8_MAX_C) return PNC_EINVAL;
    if (Cpad % 8 || Cpad < C) return PNC_EINVAL;
    if (((uintptr_t)out16 | (uintptr_t)out16_lo) & 15) return PNC_EALIGN;
    const int64_t P = (int64_t)F * Npix;
    int tile_pix = (U8_STAGE - 16) / C;                              // head (<= 15) + tile_pix * C <= U8_STAGE - 1
    if (tile_pix > U8_MAX_TILE_PIX) tile_pix = U8_MAX_TILE_PIX;
    const int64_t ntile = (P + tile_pix - 1) / tile_pix;
    const unsigned grid = (unsigned)(ntile < 2048 ? ntile : 2048);   // 8 workgroups per CU; the kernel strides over the tiles
    hipLaunchKernelGGL(u8_to_tokens_kernel, dim3(grid), dim3(256), 0, hip_stream(stream), src, lut, P, C, Cpad, tile_pix,
                       f16p(out16), f16p(out16_lo));
    return pnc_launch_status();
}

extern "C" int pnc_tokens_to_u8(const float* x, int ld, int64_t M, int C, uint8_t* out, void* stream) {
    if (!x || !out || M < 1 || C < 1 || C > 8 || ld < C) return PNC_EINVAL;
    if (((uintptr_t)x & 3) || ((uintptr_t)out & 3)) return PNC_EALIGN;
    const int64_t n = M * C, threads = (n + 3) / 4;
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (ld == C && !((uintptr_t)x & 15))
        hipLaunchKernelGGL(tokens_to_u8_stream_kernel, grid, dim3(256), 0, hip_stream(stream), x, n, out);
    else
        hipLaunchKernelGGL(tokens_to_u8_rows_kernel, grid, dim3(256), 0, hip_stream(stream), x, ld, n, C, out);
    return pnc_launch_status();
}
