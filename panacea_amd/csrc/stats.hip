// stats.hip — range profile of a contraction operand (include/panacea_hip.h: pnc_operand_stats_f16): one bandwidth-bound pass over
// the planes of an operand that ADDS a binade histogram, a maximum and saturation counts to a 36-word device record.  A diagnostic
// pass (UNetModel3D.profile_ranges); nothing on the denoising path launches it.
#include "common.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int ST_THREADS = 256;
constexpr int ST_MAX_BLOCKS = 1024;       // four workgroups per CU of the 256: the global atomics stay <= 36 x 1024 per launch
constexpr int ST_WORDS = PNC_STATS_WORDS;

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

// A chunk = 8 consecutive elements of one row (16 bytes of hi); chunk i of the plane is (row, c) = (i / cpr, i % cpr), cpr = cols / 8:
// only columns < cols are ever addressed.  A thread walks chunks i0, i0 + S, ... (S = all threads of the grid) with (row, c) kept
// incrementally: (sr, sc) = (S / cpr, S % cpr) from the host, no division inside the loop.
// Histogram: lane b (< 32) of every wave holds the wave's count of bin b in a register.  Per element slot the wave peels the bins
// that occur — ballot of the lanes that share the first remaining lane's bin, popcount, one add — so an activation plane that sits
// in three or four binades costs three or four rounds per slot, and nothing touches LDS or memory until the wave is done.
// LO: 0 = no lo plane, 1 = fp16, 2 = e4m3 bytes.
template <int LO>
__global__ __launch_bounds__(ST_THREADS) void operand_stats_kernel(const half_t* __restrict__ hi, const void* __restrict__ lo,
                                                                   int64_t rows, int cpr, int64_t ld, int64_t sr, int sc,
                                                                   unsigned long long* __restrict__ rec) {
    __shared__ unsigned long long acc[ST_WORDS];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < ST_WORDS) acc[tid] = 0ull;
    __syncthreads();

    const int64_t i0 = (int64_t)blockIdx.x * ST_THREADS + tid;
    int64_t row = i0 / cpr;
    int c = (int)(i0 - row * cpr);
    unsigned cnt = 0;             // lane b < 32: elements of this wave in bin b
    unsigned vmax = 0, n_nan = 0, n_lo = 0, n_el = 0;
    // the trip count is wave-uniform up to the tail: a lane without a chunk stays in the loop with valid = false, so that the ballots
    // below run with every lane of the wave present
    for (;;) {
        const bool valid = row < rows;
        if (!__any(valid)) break;
        u32x4 w = {0u, 0u, 0u, 0u};
        if (valid) {
            const int64_t off = row * ld + (int64_t)c * 8;
            w = *reinterpret_cast<const u32x4*>(hi + off);
            if (LO == 1) {
                const u32x4 l = *reinterpret_cast<const u32x4*>(reinterpret_cast<const half_t*>(lo) + off);
#pragma unroll
                for (int j = 0; j < 4; ++j)      // exponent field all ones (Inf / NaN): 0x7C00 + 0x0400 carries into bit 15, never beyond
                    n_lo += __popc(((l[j] & 0x7C007C00u) + 0x04000400u) & 0x80008000u);
            } else if (LO == 2) {
                const u32x2 l = *reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned char*>(lo) + off);
#pragma unroll
                for (int j = 0; j < 2; ++j)      // (byte & 0x7F) >= 0x7E: + 2 carries into bit 7, never beyond
                    n_lo += __popc(((l[j] & 0x7F7F7F7Fu) + 0x02020202u) & 0x80808080u);
            }
            n_el += 8;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned a = ((e & 1) ? (w[e >> 1] >> 16) : w[e >> 1]) & 0x7FFFu;
            vmax = max(vmax, a);                 // (zeros of an invalid lane change neither the maximum nor the NaN count)
            n_nan += a > 0x7C00u ? 1u : 0u;
            const int bin = (int)(a >> 10);
            unsigned long long rem = __ballot(valid);
            while (rem) {                        // wave-uniform
                const int leader = __ffsll((long long)rem) - 1;
                const int b = __builtin_amdgcn_readlane(bin, leader);
                const unsigned long long m = __ballot(valid && bin == b);
                cnt += lane == b ? (unsigned)__popcll(m) : 0u;
                rem &= ~m;
            }
        }
        row += sr;
        c += sc;
        if (c >= cpr) { c -= cpr; ++row; }
    }
    vmax = wave_max_u32(vmax);
    n_nan = wave_sum_u32(n_nan);
    n_lo = wave_sum_u32(n_lo);
    n_el = wave_sum_u32(n_el);
    if (lane < 32 && cnt) atomicAdd(&acc[lane], (unsigned long long)cnt);
    if (lane == 0) {
        atomicMax(&acc[32], (unsigned long long)vmax);
        if (n_lo) atomicAdd(&acc[33], (unsigned long long)n_lo);
        if (n_nan) atomicAdd(&acc[34], (unsigned long long)n_nan);
        atomicAdd(&acc[35], (unsigned long long)n_el);
    }
    __syncthreads();
    if (tid < ST_WORDS) {                        // one flush per workgroup: at most 36 global 64-bit atomics
        const unsigned long long v = acc[tid];
        if (v) {
            if (tid == 32) atomicMax(rec + 32, v);
            else atomicAdd(rec + tid, v);
        }
    }
}

}  // namespace

extern "C" int pnc_operand_stats_f16(const void* hi, const void* lo, int lo_fmt, int64_t rows, int cols, int64_t ld,
                                     unsigned long long* rec, void* stream) {
    if (!hi || !rec || rows < 1 || cols < 1 || ld < cols) return PNC_EINVAL;
    if (lo && lo_fmt != PNC_LO_F16 && lo_fmt != PNC_LO_E4M3) return PNC_EINVAL;
    if (rows > (INT64_MAX >> 4) / ld) return PNC_EINVAL;              // byte offsets stay inside int64
    // a wave counts in 32-bit registers and widens at the LDS merge: at most 4 x ST_MAX_BLOCKS waves share the plane, so 2^40
    // chunks (2^43 elements, 16 TB of fp16) keep every wave below 2^32 elements
    if (rows > (((int64_t)1 << 40) / (cols / 8 > 0 ? cols / 8 : 1))) return PNC_EINVAL;
    if ((cols % 8) || (ld % 8)) return PNC_EALIGN;
    if (((uintptr_t)hi & 15) || ((uintptr_t)rec & 7)) return PNC_EALIGN;
    if (lo && ((uintptr_t)lo & (lo_fmt == PNC_LO_E4M3 ? 7 : 15))) return PNC_EALIGN;
    const int cpr = cols / 8;
    const int64_t chunks = rows * cpr;
    const int64_t want = (chunks + ST_THREADS - 1) / ST_THREADS;
    const int blocks = (int)(want < ST_MAX_BLOCKS ? want : ST_MAX_BLOCKS);
    const int64_t S = (int64_t)blocks * ST_THREADS;
    const int64_t sr = S / cpr;
    const int sc = (int)(S - sr * cpr);
    const auto kernel = !lo ? operand_stats_kernel<0> : lo_fmt == PNC_LO_F16 ? operand_stats_kernel<1> : operand_stats_kernel<2>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(ST_THREADS), 0, reinterpret_cast<hipStream_t>(stream), f16p(hi), lo, rows, cpr, ld, sr,
                       sc, rec);
    return pnc_launch_status();
}
