// region.hip — region editing (include/panacea_hip.h section 8): the per-pixel forms of clip editing's kernels.  A recorded clip's
// camera views or pixel regions are kept instead of whole frames: pnc_latent_renoise_masked is pnc_frames_renoise (misc.hip) with
// the selector per latent pixel, pnc_mask_pool_u8 makes that selector from a pixel mask, pnc_u8_select puts the recorded bytes back
// into the decoded frames.  All three only select and move data; the one arithmetic line is misc.hip's `renoised`.
#include "common.h"

namespace {

// ---- pnc_latent_renoise_masked ---------------------------------------------------------------------------------------------------
// A PLANE (t, c) is one contiguous run of Npix floats of z, noise, x and out, and row t of the mask lies over each of a frame's C
// planes.  A workgroup owns RM_SLICE consecutive pixels of one plane: the sigma and the alignment case are workgroup-uniform, the
// selector is per element.  As in frames_renoise_kernel the run is cut at the 16-byte boundaries of `out`: up to three head
// elements, a body of float4s, up to three tail elements; the body moves in 16-byte loads and stores when the plane's z, noise and x
// sit at out's offset from a boundary, and element by element otherwise.  With Npix % 4 != 0 the planes of a frame start at
// different offsets while the mask row stays where it is, so the mask is a 16-byte load only for the planes whose offset it shares
// and four 4-byte loads for the others.
// Loads that cannot matter are not issued: x where all four elements are kept, z and the noise where none is (the noise neither at
// sigma 0), and with out == x a float4 without a kept element is not touched at all.  What is loaded and not selected stays out of
// the result: the last line is a select.  Every element is read before it is written and only by the thread that writes it, so out
// may be x.
constexpr int RM_SLICE = 1024;

__device__ __forceinline__ float renoised(float a, float n, float s) {
#pragma clang fp contract(off)
    const float p = n * s;
    return a + p;
}

__device__ __forceinline__ float masked_one(float m, bool add, float s, const float* z, const float* n, const float* x, int64_t j) {
    if (!(m > 0.0f)) return x[j];                                    // 0.0, -0.0, negative, NaN: not kept
    return add ? renoised(z[j], n[j], s) : z[j];                     // sigma 0: z's bits, the noise is not read
}

__global__ __launch_bounds__(256) void latent_renoise_masked_kernel(const float* __restrict__ z, const float* __restrict__ noise,
                                                                    const float* __restrict__ sigma, const float* __restrict__ mask,
                                                                    const float* x, float* out, int C, int64_t Npix, int slices) {
    const int64_t pl = blockIdx.x / (unsigned)slices;                // the plane t * C + c
    const int b = (int)(blockIdx.x - (unsigned)pl * (unsigned)slices);
    const int t = (int)(pl / C), tid = threadIdx.x;
    const float s = sigma[t];
    const bool add = s != 0.0f;
    const float* zp = z + pl * Npix;
    const float* np = noise + pl * Npix;
    const float* xp = x + pl * Npix;
    const float* mp = mask + (int64_t)t * Npix;
    float* o = out + pl * Npix;
    const unsigned off = (unsigned)((uintptr_t)o & 15);
    const bool vec = ((uintptr_t)zp & 15) == off && ((uintptr_t)np & 15) == off && ((uintptr_t)xp & 15) == off;
    if (!vec) {                                                      // element by element, a slice per workgroup
#pragma unroll
        for (int k = 0; k < RM_SLICE / 256; ++k) {
            const int64_t j = (int64_t)b * RM_SLICE + k * 256 + tid;
            if (j < Npix) o[j] = masked_one(mp[j], add, s, zp, np, xp, j);
        }
        return;
    }
    const int64_t head = min((int64_t)((16 - off) & 15) >> 2, Npix);  // elements in front of out's first 16-byte boundary
    const int64_t nv = (Npix - head) >> 2;                           // whole float4s behind it (<= slices * 256)
    const int64_t i = (int64_t)b * 256 + tid;
    if (i < nv) {
        const int64_t j = head + i * 4;
        f32x4 m;
        if (((uintptr_t)mp & 15) == off) {
            m = *reinterpret_cast<const f32x4*>(mp + j);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = mp[j + e];
        }
        const bool k0 = m[0] > 0.0f, k1 = m[1] > 0.0f, k2 = m[2] > 0.0f, k3 = m[3] > 0.0f;
        const bool any = k0 || k1 || k2 || k3, all = k0 && k1 && k2 && k3;
        if (any || xp != o) {
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f}, w = v, u = v;
            if (any) v = *reinterpret_cast<const f32x4*>(zp + j);
            if (any && add) w = *reinterpret_cast<const f32x4*>(np + j);
            if (!all) u = *reinterpret_cast<const f32x4*>(xp + j);
            f32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float kept = add ? renoised(v[e], w[e], s) : v[e];
                r[e] = m[e] > 0.0f ? kept : u[e];
            }
            *reinterpret_cast<f32x4*>(o + j) = r;
        }
    }
    if (b == 0 && tid < 8) {                                         // lanes 0..3: the head, lanes 4..7: the tail
        const int64_t j = tid < 4 ? tid : head + nv * 4 + (tid - 4);
        if (tid < 4 ? j < head : j < Npix) o[j] = masked_one(mp[j], add, s, zp, np, xp, j);
    }
}

// ---- pnc_mask_pool_u8 --------------------------------------------------------------------------------------------------------------
// A thread per latent cell; consecutive lanes own consecutive cells of a row, so the f bytes a lane reads per mask row follow its
// neighbour's.  f == 8 on an 8-byte aligned mask (W % 8 == 0 keeps every row of every cell aligned then) reads a cell's row as one
// 8-byte load and tests its bytes at once: (v - 0x01..01) & ~v & 0x80..80 is nonzero iff some byte of v is zero.
template <bool ROW8>
__global__ __launch_bounds__(256) void mask_pool_u8_kernel(const uint8_t* __restrict__ mask, float* __restrict__ out, int64_t cells,
                                                           int H, int W, int f) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const int w = W / f, h = H / f;
    const int64_t row = i / w;                                       // t * h + y
    const int xc = (int)(i - row * w);
    const int64_t t = row / h;
    const int y = (int)(row - t * h);
    const uint8_t* p = mask + ((t * H + (int64_t)y * f) * W + (int64_t)xc * f);
    bool every = true;
    if (ROW8) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const uint64_t v = *reinterpret_cast<const uint64_t*>(p + (int64_t)r * W);
            every = every && ((v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull) == 0;
        }
    } else {
        for (int r = 0; r < f; ++r)
            for (int c = 0; c < f; ++c) every = every && p[(int64_t)r * W + c] != 0;
    }
    out[i] = every ? 1.0f : 0.0f;
}

// ---- pnc_u8_select -----------------------------------------------------------------------------------------------------------------
// The frames are one run of n = npix * C bytes.  It is cut at the 16-byte boundaries of `out`: up to 15 head bytes, a body of
// 16-byte chunks, up to 15 tail bytes.  With src and gen at out's offset from a boundary a thread owns one chunk — two 16-byte loads,
// the mask bytes of the (at most 16) pixels the chunk touches, one 16-byte store; at other offsets a thread owns 16
// single bytes.  Every byte is read before it is written and only by the thread that writes it, so out may be gen.
constexpr int SEL_SLICE = 4096;                    // bytes of a workgroup

template <int C>                                   // channels per pixel, 1 .. 4: divisions by a constant, loops of a known length
__global__ __launch_bounds__(256) void u8_select_kernel(const uint8_t* __restrict__ src, const uint8_t* gen,
                                                        const uint8_t* __restrict__ mask, uint8_t* out, int64_t n) {
    constexpr int SEL_MAX_PIX = (C - 1 + 15) / C + 1;                // pixels under a 16-byte chunk that starts inside a pixel
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const unsigned off = (unsigned)((uintptr_t)out & 15);
    const bool vec = ((uintptr_t)src & 15) == off && ((uintptr_t)gen & 15) == off;
    if (!vec) {
#pragma unroll
        for (int k = 0; k < SEL_SLICE / 256; ++k) {
            const int64_t j = b * SEL_SLICE + k * 256 + tid;
            if (j < n) out[j] = mask[j / C] ? src[j] : gen[j];
        }
        return;
    }
    const int64_t head = min((int64_t)((16 - off) & 15), n);         // bytes in front of out's first 16-byte boundary
    const int64_t nv = (n - head) >> 4;                              // whole chunks behind it (<= blocks * 256)
    const int64_t i = b * 256 + tid;
    if (i < nv) {
        const int64_t j = head + i * 16;
        const int64_t p0 = j / C;
        const int r0 = (int)(j - p0 * C), npx = (r0 + 15) / C + 1;   // the chunk's bytes lie in pixels p0 .. p0 + npx - 1 < npix
        uint32_t keep = 0;                                           // bit q: pixel p0 + q is kept
#pragma unroll
        for (int q = 0; q < SEL_MAX_PIX; ++q)
            if (q < npx && mask[p0 + q]) keep |= 1u << q;
        const uint4 sv = *reinterpret_cast<const uint4*>(src + j), gv = *reinterpret_cast<const uint4*>(gen + j);
        const uint32_t sw[4] = {sv.x, sv.y, sv.z, sv.w}, gw[4] = {gv.x, gv.y, gv.z, gv.w};
        uint32_t rw[4];
        int q = 0, r = r0;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t sel = 0;                                        // 0xff in the bytes taken from src
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if ((keep >> q) & 1u) sel |= 0xffu << (8 * e);
                if (++r == C) { r = 0; ++q; }
            }
            rw[d] = (sw[d] & sel) | (gw[d] & ~sel);
        }
        *reinterpret_cast<uint4*>(out + j) = make_uint4(rw[0], rw[1], rw[2], rw[3]);
    }
    if (b == 0 && tid < 32) {                                        // lanes 0..15: the head, lanes 16..31: the tail
        const int64_t j = tid < 16 ? tid : head + nv * 16 + (tid - 16);
        if (tid < 16 ? j < head : j < n) out[j] = mask[j / C] ? src[j] : gen[j];
    }
}

inline hipStream_t hip_stream(void* stream) { return reinterpret_cast<hipStream_t>(stream); }

// every launch of this file: `blocks` 256-thread workgroups on the caller's stream (misc.hip's launch_1d, counted in workgroups)
template <typename... Sig, typename... Args>
int launch_blocks(void (*kernel)(Sig...), int64_t blocks, void* stream, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, hip_stream(stream), args...);
    return pnc_launch_status();
}

constexpr int64_t GRID_MAX = (int64_t)1 << 31;     // workgroups a launch can count

}  // namespace

extern "C" int pnc_latent_renoise_masked(const float* z, const float* noise, const float* sigma, const float* mask, const float* x,
                                         float* out, int T, int C, int64_t Npix, void* stream) {
    if (!z || !noise || !sigma || !mask || !x || !out || T < 1 || C < 1 || Npix < 1) return PNC_EINVAL;
    if (Npix > ((int64_t)1 << 40) / C) return PNC_EINVAL;            // a frame of at most 2^40 elements ...
    const int64_t slices = (Npix + RM_SLICE - 1) / RM_SLICE;
    if ((int64_t)T * C * slices >= GRID_MAX) return PNC_EINVAL;      // ... and a grid the launch can count
    if (((uintptr_t)z | (uintptr_t)noise | (uintptr_t)sigma | (uintptr_t)mask | (uintptr_t)x | (uintptr_t)out) & 3) return PNC_EALIGN;
    return launch_blocks(latent_renoise_masked_kernel, (int64_t)T * C * slices, stream, z, noise, sigma, mask, x, out, C, Npix,
                         (int)slices);
}

extern "C" int pnc_mask_pool_u8(const uint8_t* mask_u8, float* out, int T, int H, int W, int f, void* stream) {
    if (!mask_u8 || !out || T < 1 || H < 1 || W < 1 || f < 1 || f > 16 || H % f || W % f) return PNC_EINVAL;
    const int64_t hw = (int64_t)(H / f) * (W / f);                   // < 2^62
    if (hw > ((int64_t)1 << 38) / T) return PNC_EINVAL;              // a selector of at most 2^38 cells: a grid the launch can count
    const int64_t cells = T * hw, blocks = (cells + 255) / 256;
    if ((uintptr_t)out & 3) return PNC_EALIGN;
    if (f == 8 && !((uintptr_t)mask_u8 & 7)) return launch_blocks(mask_pool_u8_kernel<true>, blocks, stream, mask_u8, out, cells, H, W, f);
    return launch_blocks(mask_pool_u8_kernel<false>, blocks, stream, mask_u8, out, cells, H, W, f);
}

extern "C" int pnc_u8_select(const uint8_t* src, const uint8_t* gen, const uint8_t* mask_u8, uint8_t* out, int64_t npix, int C,
                             void* stream) {
    if (!src || !gen || !mask_u8 || !out || npix < 1 || C < 1 || C > 4 || out == src) return PNC_EINVAL;
    if (npix > ((int64_t)1 << 40)) return PNC_EINVAL;
    const int64_t n = npix * C, blocks = (n + SEL_SLICE - 1) / SEL_SLICE;
    if (blocks >= GRID_MAX) return PNC_EINVAL;
    switch (C) {
    case 1: return launch_blocks(u8_select_kernel<1>, blocks, stream, src, gen, mask_u8, out, n);
    case 2: return launch_blocks(u8_select_kernel<2>, blocks, stream, src, gen, mask_u8, out, n);
    case 3: return launch_blocks(u8_select_kernel<3>, blocks, stream, src, gen, mask_u8, out, n);
    default: return launch_blocks(u8_select_kernel<4>, blocks, stream, src, gen, mask_u8, out, n);
    }
}
