// gemm_glds_body.inc — the body of gemm_glds_kernel / gemm_glds_ws_kernel (gemm_kernel.h), included as text inside both.  In scope:
// the kernels' template parameters and arguments, `constexpr bool WS` and `const void* wlo16` (NULL when !WS).
    PncGemmParams p = pin;
    constexpr int NW = WGM * WGN;                          // waves per workgroup
    constexpr int MI = BM / WGM / 32, NI = BN / WGN / 32;
    constexpr int RPI = NW * 8;                            // rows staged per DMA iteration (8 rows per wave)
    constexpr int A_IT = BM / RPI, B_IT = BN / RPI;
    constexpr int LOADS = A_IT + B_IT;                     // DMA instructions per thread per K tile
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
    static_assert(BM % RPI == 0 && BN % RPI == 0, "tile rows must be a multiple of the DMA row group");
    constexpr int ENI = NI < 2 ? NI : 2;                   // column blocks staged per epilogue pass
    constexpr int EPITCH = ENI * 32 + 4;                   // floats per staged epilogue row
    constexpr bool GEGLU = (EPI & E_GEGLU) != 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const half_t* __restrict__ A = reinterpret_cast<const half_t*>(p.A);
    const half_t* __restrict__ A_lo = reinterpret_cast<const half_t*>(p.A_lo);
    const half_t* __restrict__ Wt = reinterpret_cast<const half_t*>(p.W);

    const int tiles_n = (p.N + BN - 1) / BN;
    const int tiles_m = (p.M + BM - 1) / BM;
    // split K (ksplit > 1): block b = (slice, tile); slice s runs K tiles [s*nt/S, (s+1)*nt/S) and writes its raw fp32
    // accumulators to ws[s][M][N] (the host launches the E_O32 variant with the epilogue options cleared);
    // splitk_reduce_kernel sums the slices in order and applies the epilogue.
    // Tail split (tail_f = 2 or 4): the last (ntile_mn - nfull) output tiles - the partial round that would leave most
    // CUs idle - are each run by tail_f workgroups that own BM / tail_f rows of the tile: the waves of the other row
    // groups skip their MFMAs and epilogue (their A rows are DMA'd as out-of-bounds offsets = zeros), all waves still stage W.  Rows are
    // independent in a GEMM, so the result does not depend on the split.
    const int ntile_mn = tiles_m * tiles_n;
    int kslice = 0, tile, part = 0;
    if (ksplit > 1) {
        const int blk = xcd_remap(blockIdx.x, ntile_mn * ksplit);
        kslice = blk / ntile_mn; tile = blk - kslice * ntile_mn;
    } else if ((int)blockIdx.x < nfull) {
        tile = xcd_remap(blockIdx.x, nfull);
    } else {
        const int j = (int)blockIdx.x - nfull;
        tile = nfull + j / tail_f; part = j - (j / tail_f) * tail_f;
    }
    const bool split_rows = (ksplit == 1) && ((int)blockIdx.x >= nfull) && (tail_f > 1);
    // Tile id -> (tm, tn).  Default: tn fastest, so the ~32 tiles an XCD runs at once are 32 / tiles_n row panels x all
    // column tiles.  With many column tiles (FF1: 10-40, QKV at C = 1280: 12-15) that is ONE panel against the whole of W,
    // and where W exceeds the 4 MB L2 (every level but 0) W is re-streamed from the fabric once per row panel: 1.26 GB per
    // FF1 launch at every level (profiles/round2/pmc_precise_fetch_by_kernel.txt: 52 GB per step in the GEGLU kernel alone).
    // group_m > 0: walk group_m row panels x the column tiles instead (tm fastest inside a group), so the concurrent set
    // is group_m x (32 / group_m) tiles and each W column tile is fetched once per GROUP of panels.  Same tiles, same
    // arithmetic: results are bit-identical.
    int tn, tm;
    if (group_m > 0) {
        const int width = group_m * tiles_n;
        const int gid = tile / width, first_m = gid * group_m;
        const int gsz = min(tiles_m - first_m, group_m);
        const int in = tile - gid * width;
        tm = first_m + in % gsz; tn = in / gsz;
    } else {
        tn = tile % tiles_n; tm = tile / tiles_n;
    }
    if constexpr (AMODE == PNC_A_CONV1D_T) {
        // Temporal conv: the three taps of a row panel are the panels of frames t - 1, t, t + 1 at the SAME pixels — with the row
        // panels in memory order (frame-major) the panel of frame t is fetched again, ~48 panels later and mostly on another
        // XCD, for frame t + 1 and t - 1: the operand crossed the fabric three times (profiles/round4: 11.2 GB per step for the
        // first temporal site against 6.2 GB of operands).  Walk the panels FRAME-FASTEST instead (pixel block outer): the
        // consecutive tile ids one XCD works through are the frames of one pixel block, and two of the three reads hit its L2.
        // A permutation of the row panels: same tiles, same arithmetic.
        const int pb_n = p.Npix / BM;                        // row panels per frame
        if (pb_n * BM == p.Npix && pb_n > 1) {
            const int nbt = tiles_m / pb_n;                  // frames (b, t) of the launch
            tm = (tm % nbt) * pb_n + tm / nbt;
        }
    }
    const int m0 = tm * BM, n0 = tn * BN;
    const int ntiles_all = (p.K + BK - 1) / BK;
    const int kt_begin = (int)((int64_t)kslice * ntiles_all / ksplit);
    const int ntiles = (int)((int64_t)(kslice + 1) * ntiles_all / ksplit) - kt_begin;
    if (ksplit > 1) p.out32 = p.ws + (int64_t)kslice * p.M * p.N;
    // precise operand: the lo plane's K tiles run first.  fp16 lo plane: the same K tiles as the hi plane, then the accumulators
    // are scaled by 2^-11.  e4m3 lo plane (lo8): 128 k per 128-byte LDS row -> half the tiles, DMA pieces and barriers; the
    // block-scaled fp8 MFMA carries the 2^-11 as its A scale and the weight row's exponent as its B scale, so the lo products
    // land in the accumulators at their final weight and the hi pass simply continues.
    const bool lo8 = A_lo && p.a_lo_fmt == PNC_LO_E4M3;
    const int nlo_all = lo8 ? (p.K + BK8 - 1) / BK8 : ntiles_all;
    const int kt_begin_lo = (int)((int64_t)kslice * nlo_all / ksplit);
    const int nt_alo = A_lo ? (int)((int64_t)(kslice + 1) * nlo_all / ksplit) - kt_begin_lo : 0;
    // split weights (fp16 W_lo next to an fp16 A_lo): the lo pass runs the slice's K tiles a second time, A's hi plane against W_lo,
    // before the scaling — a slice of a split-K launch runs its own K range in all three parts
    const bool wl16 = !WS && A_lo && !lo8 && p.W_lo != nullptr;
    const int nt_lo = wl16 ? 2 * nt_alo : nt_alo;
    // WS: the weight part's tiles come first in the tile counter (the slice's own K range once more), then the lo tiles, then the hi tiles
    const int nt_w = WS ? ntiles : 0;
    const int ntot = nt_w + ntiles + nt_lo;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // scalar: LDS-DMA destinations (M0) and wave-row tests stay on the SALU
    const int wm = wave / WGN, wn = wave % WGN;

    // DMA assignment: lane l of wave w fills slot (l&7) of row i*32 + w*8 + (l>>3); the slot holds the
    // chunk slot ^ ((row>>1)&7), and (row>>1)&7 does not depend on i
    const int srow = wave * 8 + (lane >> 3);
    const int schunk = (lane & 7) ^ ((srow >> 1) & 7);
    const int rows_lo = split_rows ? part * (BM / tail_f) : 0;                 // tile-local row range of this workgroup
    const int rows_hi = split_rows ? rows_lo + BM / tail_f : BM;
    const bool wave_on = (wm * (MI * 32) >= rows_lo) && (wm * (MI * 32) < rows_hi);
    RowState rows[A_IT];
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int r = i * RPI + srow;
        rows[i] = make_row<AMODE>(p, m0 + r, m0);
        rows[i].valid = rows[i].valid && (r >= rows_lo) && (r < rows_hi);
    }
    // buffer resources: the A plane(s) from the tile's window origin, W from the tile's first row.  A row's offset is fixed over
    // the K loop for plain A and for W (the K tile enters as the scalar offset); the gathers recompute theirs per K tile.
    const int64_t a_origin = a_window_origin<AMODE>(p, m0);
    const buffer_rsrc_t rs_a = make_rsrc(A + a_origin, 0x7FFFFF00u);
    const buffer_rsrc_t rs_alo = make_rsrc(lo8 ? static_cast<const void*>(reinterpret_cast<const char*>(p.A_lo) + a_origin)
                                               : static_cast<const void*>((A_lo ? A_lo : A) + a_origin), 0x7FFFFF00u);
    const buffer_rsrc_t rs_whi = make_rsrc(Wt + (int64_t)n0 * p.ldw, 0x7FFFFF00u);
    const buffer_rsrc_t rs_wlo = make_rsrc(lo8 ? static_cast<const void*>(reinterpret_cast<const char*>(p.W_lo) + (int64_t)n0 * p.ldw_lo)
                                               : static_cast<const void*>((wl16 ? reinterpret_cast<const half_t*>(p.W_lo) : Wt) + (int64_t)n0 * p.ldw),
                                           0x7FFFFF00u);
    unsigned woff[B_IT], aoff[A_IT];
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
        const int nl = i * RPI + srow;
        woff[i] = (n0 + nl < p.N) ? (unsigned)(nl * p.ldw + schunk * 8) * 2u : PNC_BUF_OOB;
    }
#pragma unroll
    for (int i = 0; i < A_IT; ++i)
        aoff[i] = (AMODE == PNC_A_PLAIN && rows[i].valid) ? (unsigned)(rows[i].rel + schunk * 8) * 2u : PNC_BUF_OOB;
    const buffer_rsrc_t rs_w16 = make_rsrc((WS ? reinterpret_cast<const half_t*>(wlo16) : Wt) + (int64_t)n0 * p.ldw, 0x7FFFFF00u);
    const int kt_tail = (p.K & (BK - 1)) ? ntiles_all - 1 : -1;      // the one K tile with chunks beyond K, if any
    // DMA pieces [Q0, Q1) of K tile kt_local into `stage` (pieces 0 .. A_IT-1: the A row groups, A_IT .. LOADS-1: the W row groups;
    // the range is compile-time so that the staggered schedule below can spread a tile's pieces over its phases)
    auto issue_part = [&](int kt_local, int stage, auto q0_, auto q1_) __attribute__((always_inline)) {
        constexpr int Q0 = decltype(q0_)::value, Q1 = decltype(q1_)::value;
        const bool wpart = WS && kt_local < nt_w;        // (uniform) a tile of the weight part: (A hi plane, W's fp16 lo plane)
        if constexpr (WS) kt_local -= wpart ? 0 : nt_w;
        const bool lo = !wpart && kt_local < nt_lo;
        char* sa = smem + stage * STAGE + wave * 1024;
        char* sb = sa + A_BYTES;
        if (lo && lo8) {                                 // (uniform) e4m3 tile: chunk = 16 k, byte offsets = element offsets
            // The lane offsets of this branch are derived from the hi pass's on the spot.  Opaque copies of the two lane constants
            // keep hipcc from hoisting them out of the K loop as a second set of loop invariants: next to 160 accumulator
            // registers the kernel has ~12 VGPRs to spare, and 9-20 more invariants spilled 100-300 registers (round 3).
            int schunk8 = schunk, srow8 = srow;
            asm volatile("" : "+v"(schunk8), "+v"(srow8));
            const int kt8 = kt_begin_lo + kt_local;
            const int kc8 = kt8 * BK8 + schunk8 * 16;
            const unsigned ks8 = (unsigned)kt8 * BK8;
            const bool k_on = kc8 < p.K;                 // false only in the chunks of the last tile beyond K
#pragma unroll
            for (int i = 0; i < A_IT; ++i) {
                if (i < Q0 || i >= Q1) continue;
                if constexpr (AMODE == PNC_A_PLAIN)      // (rel + 8 schunk) * 2 -> rel + 16 schunk
                    glds16_buf(rs_alo, (k_on && aoff[i] != PNC_BUF_OOB) ? (aoff[i] >> 1) + (unsigned)schunk8 * 8u : PNC_BUF_OOB, ks8,
                               sa + i * (RPI * 128));
                else glds16_buf(rs_alo, a_chunk_off<AMODE, 1u>(p, rows[i], kc8), 0u, sa + i * (RPI * 128));
            }
#pragma unroll
            for (int i = 0; i < B_IT; ++i) {
                if (A_IT + i < Q0 || A_IT + i >= Q1) continue;
                glds16_buf(rs_wlo, (k_on && woff[i] != PNC_BUF_OOB) ? (unsigned)((i * RPI + srow8) * p.ldw_lo + schunk8 * 16) : PNC_BUF_OOB,
                           ks8, sb + i * (RPI * 128));
            }
            return;
        }
        const bool wl = lo && kt_local >= nt_alo;        // (uniform) second part of an fp16 lo pass: (A hi plane, W lo plane)
        const int kt = (wpart ? kt_begin : (lo ? kt_begin_lo - (wl ? nt_alo : 0) : kt_begin - nt_lo)) + kt_local;
        // (one flat select per resource on a precomputed flag: with a short-circuit condition or a nested select here hipcc kept the
        // closure, and with it the parameter block, in scratch memory — 624 B per lane in every variant)
        const bool alo = lo & !wl;
        const buffer_rsrc_t rs = alo ? rs_alo : rs_a;
        const buffer_rsrc_t rs_w = WS ? (wpart ? rs_w16 : rs_whi) : (wl ? rs_wlo : rs_whi);
        const int kc = kt * BK + schunk * 8;
        const unsigned ks = (unsigned)kt * (BK * 2);     // the K tile as the scalar byte offset of plain rows
        if (kt != kt_tail) {                             // (uniform) no per-lane predicate on the K index
#pragma unroll
            for (int i = 0; i < A_IT; ++i) {
                if (i < Q0 || i >= Q1) continue;
                if constexpr (AMODE == PNC_A_PLAIN) glds16_buf(rs, aoff[i], ks, sa + i * (RPI * 128));
                else glds16_buf(rs, a_chunk_off<AMODE>(p, rows[i], kc), 0u, sa + i * (RPI * 128));
            }
#pragma unroll
            for (int i = 0; i < B_IT; ++i) {
                if (A_IT + i < Q0 || A_IT + i >= Q1) continue;
                glds16_buf(rs_w, woff[i], ks, sb + i * (RPI * 128));
            }
        } else {
            const bool k_on = kc < p.K;
#pragma unroll
            for (int i = 0; i < A_IT; ++i) {
                if (i < Q0 || i >= Q1) continue;
                if constexpr (AMODE == PNC_A_PLAIN) glds16_buf(rs, k_on ? aoff[i] : PNC_BUF_OOB, ks, sa + i * (RPI * 128));
                else glds16_buf(rs, a_chunk_off<AMODE>(p, rows[i], kc), 0u, sa + i * (RPI * 128));
            }
#pragma unroll
            for (int i = 0; i < B_IT; ++i) {
                if (A_IT + i < Q0 || A_IT + i >= Q1) continue;
                glds16_buf(rs_w, k_on ? woff[i] : PNC_BUF_OOB, ks, sb + i * (RPI * 128));
            }
        }
    };
    auto issue_tile = [&](int kt_local, int stage) __attribute__((always_inline)) {
        issue_part(kt_local, stage, std::integral_constant<int, 0>{}, std::integral_constant<int, LOADS>{});
    };

    // GEGLU: the Phi table rides into LDS (behind the operand ring) with the first K tile
    constexpr int RING_BYTES = STAGES * STAGE;
    if constexpr (GEGLU) {
        const char* tab = reinterpret_cast<const char*>(phi_g);
#pragma unroll
        for (int c = wave; c < PHI_BYTES / 1024; c += NW)
            glds16(reinterpret_cast<const half_t*>(tab + c * 1024 + lane * 16), smem + RING_BYTES + c * 1024);
    }

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int frow = lane & 31, fk = lane >> 5;
    auto compute = [&](int stage, int mid_issue = -1) {
        const char* sa = smem + stage * STAGE;
        const char* sb = sa + A_BYTES;
        if (PIPE) {
            // fragments of k-step ks+1 are read while the MFMAs of k-step ks run (register double buffer)
            half8v af[2][MI], bf[2][NI];
            auto frags = [&](int ks, int b) {
#pragma unroll
                for (int i = 0; i < MI; ++i)
                    af[b][i] = *reinterpret_cast<const half8v*>(
                        sa + lds_off128(wm * (MI * 32) + i * 32 + frow, ks * 2 + fk));
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    bf[b][j] = *reinterpret_cast<const half8v*>(
                        sb + lds_off128(wn * (NI * 32) + j * 32 + frow, ks * 2 + fk));
            };
            frags(0, 0);
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                if (ks + 1 < BK / 16) frags(ks + 1, (ks + 1) & 1);
                // keep the reads of k-step ks+1 AHEAD of the MFMAs of k-step ks (hipcc otherwise sinks them behind the
                // MFMAs and then waits lgkmcnt(0) right after issuing them, exposing the LDS latency every k-step)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[ks & 1][i], bf[ks & 1][j], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (ks == 1 && mid_issue >= 0) { issue_tile(mid_issue, mid_issue & 1); __builtin_amdgcn_sched_barrier(0); }
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                half8v af[MI], bf[NI];
#pragma unroll
                for (int i = 0; i < MI; ++i)
                    af[i] = *reinterpret_cast<const half8v*>(
                        sa + lds_off128(wm * (MI * 32) + i * 32 + frow, ks * 2 + fk));
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    bf[j] = *reinterpret_cast<const half8v*>(
                        sb + lds_off128(wn * (NI * 32) + j * 32 + frow, ks * 2 + fk));
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
                if (ks == 1 && mid_issue >= 0) issue_tile(mid_issue, mid_issue & 1);
            }
        }
    };
    // e4m3 lo tile: two MFMA windows of 64 k (the last tile of K = 320 holds one).  Lane (row r, group g) supplies bytes
    // 32 g .. 32 g + 31 of the window for both operands (element j of a lane group pairs with element j of the same group of the
    // other operand: tools/exp/mx_mfma_probe.hip) = chunks 2g, 2g+1 of the window: two ds_read_b128 per fragment, same swizzle.
    auto compute8 = [&](int stage, int kt_local) {
        const char* sa = smem + stage * STAGE;
        const char* sb = sa + A_BYTES;
        const int nwin = (p.K - (kt_begin_lo + kt_local) * BK8) > 64 ? 2 : 1;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            if (w < nwin) {
                i32x8 af[MI];
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    const int row = wm * (MI * 32) + i * 32 + frow;
                    const i32x4 a0 = *reinterpret_cast<const i32x4*>(sa + lds_off128(row, w * 4 + fk * 2));
                    const i32x4 a1 = *reinterpret_cast<const i32x4*>(sa + lds_off128(row, w * 4 + fk * 2 + 1));
                    af[i] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
                }
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    const int row = wn * (NI * 32) + j * 32 + frow;
                    const i32x4 b0 = *reinterpret_cast<const i32x4*>(sb + lds_off128(row, w * 4 + fk * 2));
                    const i32x4 b1 = *reinterpret_cast<const i32x4*>(sb + lds_off128(row, w * 4 + fk * 2 + 1));
                    const i32x8 bf = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                    for (int i = 0; i < MI; ++i)
                        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[i], bf, acc[i][j], 0, 0, 0, E8M0_LO_INV, 0, p.w_lo_exp);
                    // one B fragment (8 registers) in flight: hipcc otherwise hoists the reads of all NI column blocks (40 registers
                    // at NI = 5) above the first MFMA and spills next to the 160 accumulator registers
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    };
    auto scale_lo = [&]() {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] *= LO_INV;
    };

    // The second-dispatched half of an 8-wave workgroup loses every issue arbitration by age (MI355X_MICROARCH.md, two waves per
    // SIMD): static priority for it.  Plain-A GEMMs -1.9 ms per step in a same-box A/B; the gathers (+0.3 / +0.4 ms) keep age order.
    // STAGGERED schedule (round 5; 8-wave geometries on two stages, PNC_OPT_GEMM_STAGGER): a K tile is four PHASES, one per k-step —
    //     fragment reads of the k-step + a third of the NEXT tile's DMA pieces | s_barrier | MI x NI MFMAs | s_barrier
    // and waves 4-7 (the second wave of every SIMD) run ONE barrier behind waves 0-3: while one wave of a SIMD is in its MFMA
    // cluster the other reads its fragments and issues its DMA, and the barriers hold that alternation (the two-group form of the
    // HIP guide's 256^2 8-phase template on this kernel's stages).  vmcnt(0) once per K tile, before the first barrier of phase 3 — a
    // whole MFMA cluster after the last DMA issue —, together with lgkmcnt(0): the OTHER group is one barrier away from reading the
    // next tile / overwriting this one.  Same K order and MFMA order per accumulator as the loops below: bit-identical results.
    // Measured.  In a stand-alone probe of this geometry under SUSTAINED load (tools/exp/gemm_phase_probe.hip, back-to-back launches,
    // profiles/round5/gemm_phase_probe_r5a.log, ..._r5c_*.log): +6 .. +19 % on every K >= 640 shape, warm and cold operands alike (L1
    // conv-K 907 -> 1082 TFLOP/s, L2 FF2 1104 -> 1259 = the vendor GEMM's 1259); the group offset is the whole effect (phases without
    // it: -2 %), priority flips around the MFMA clusters are flat, DMA inside the MFMA clusters is 40 % slower, a finer ring of k-half
    // units with counted vmcnt is slower than full-tile stages.  IN THIS KERNEL it does not carry over: the library's launches, timed
    // alone, already run the loops below at 1.14-1.30 PFLOP/s marginal (profiles/round5/stagger_ksweep_r5f.log; the probe's copy of the
    // same loop, throttled by its own sustained load, ran 0.9-1.1), the staggered loop adds +3-4 % of marginal rate where W is wide
    // (N = 1280, operands from L2) and LOSES 16 % where one column tile streams A from HBM (N = 320: its DMA has at most one K tile
    // to land); whole network 157.31 -> 157.15 ms (stagger_ab_whole_network_r5e.log).  So: ON in the persistent GEGLU kernel (FF1
    // at levels 1-2: +5-6 % in the network, +11 % alone — wide N, A from L2, the next output tile's first K tile requested inside
    // the phases), here only on request (PNC_OPT_GEMM_STAGGER = 1: the bit-identity tests and the A/B tools).
    // Where it can run: plain A (the gathers' per-piece address arithmetic sits on the critical path of a phase: the per-tap conv3x3 /
    // temporal conv launches measured 4-20 % SLOWER staggered, profiles/round5/stagger_kbench_r5c_generic_issue_path.log), K a
    // multiple of 64, no fp16 lo plane, and not in the row-split workgroups of a sparse last round (one of the two groups idles there).
    const bool direct_epi = (stagger_min_in & 0x100) != 0;
    const int stagger_min = stagger_min_in & 0xFF;
    bool staggered = false;
    if constexpr (STAGES == 2 && NW == 8 && AMODE == PNC_A_PLAIN)
        staggered = !WS && stagger_min == 1 && kt_tail < 0 && (!A_lo || lo8) && !split_rows && ksplit == 1;
    if (AMODE == PNC_A_PLAIN && NW == 8 && wave >= 4 && !staggered) __builtin_amdgcn_s_setprio(1);
    if (staggered) {
        if constexpr (STAGES == 2 && NW == 8 && AMODE == PNC_A_PLAIN) {
            constexpr int Q0 = (LOADS + 2) / 3, Q1 = (LOADS - Q0 + 1) / 2;
            const int grp = wave >> 2;
            half8v af[MI], bf[NI];
            i32x8 af8[MI], bf8[NI];
            auto rd = [&](int stage, int ks) {
                const char* sa = smem + stage * STAGE;
                const char* sb = sa + A_BYTES;
#pragma unroll
                for (int i = 0; i < MI; ++i)
                    af[i] = *reinterpret_cast<const half8v*>(sa + lds_off128(wm * (MI * 32) + i * 32 + frow, ks * 2 + fk));
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    bf[j] = *reinterpret_cast<const half8v*>(sb + lds_off128(wn * (NI * 32) + j * 32 + frow, ks * 2 + fk));
            };
            auto rd8 = [&](int stage, int w) {
                const char* sa = smem + stage * STAGE;
                const char* sb = sa + A_BYTES;
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    const int row = wm * (MI * 32) + i * 32 + frow;
                    const i32x4 a0 = *reinterpret_cast<const i32x4*>(sa + lds_off128(row, w * 4 + fk * 2));
                    const i32x4 a1 = *reinterpret_cast<const i32x4*>(sa + lds_off128(row, w * 4 + fk * 2 + 1));
                    af8[i] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
                }
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    const int row = wn * (NI * 32) + j * 32 + frow;
                    const i32x4 b0 = *reinterpret_cast<const i32x4*>(sb + lds_off128(row, w * 4 + fk * 2));
                    const i32x4 b1 = *reinterpret_cast<const i32x4*>(sb + lds_off128(row, w * 4 + fk * 2 + 1));
                    bf8[j] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
                }
            };
            // first barrier of a phase (+ this wave's fragment reads have returned), second barrier
            auto bar1 = [&]() {
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
            };
            auto bar2 = [&]() {
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
            };
            issue_tile(0, 0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const int n8 = lo8 ? nt_lo : 0;
            if (grp == 1) __builtin_amdgcn_s_barrier();               // group 1 runs one barrier behind group 0 from here on
            for (int kt = 0; kt < n8; ++kt) {                         // e4m3 lo tiles: one phase per 64-k MFMA window
                const int st = kt & 1;
                const int nwin = (p.K - (kt_begin_lo + kt) * BK8) > 64 ? 2 : 1;
#pragma unroll
                for (int w = 0; w < 2; ++w) {
                    if (w < nwin) {
                        rd8(st, w);
                        if (w == 0 && kt + 1 < ntot) issue_tile(kt + 1, st ^ 1);
                        if (w == nwin - 1) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                        bar1();
#pragma unroll
                        for (int j = 0; j < NI; ++j)
#pragma unroll
                            for (int i = 0; i < MI; ++i)
                                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af8[i], bf8[j], acc[i][j], 0, 0, 0, E8M0_LO_INV, 0, p.w_lo_exp);
                        bar2();
                    }
                }
            }
            for (int kt = n8; kt < ntot; ++kt) {
                const int st = kt & 1;
                const bool nxt = kt + 1 < ntot;
                static_for<4>([&](auto ph_) {
                    constexpr int ph = decltype(ph_)::value;
                    rd(st, ph);
                    if (nxt) {
                        // the next tile is a plain fp16 tile inside K: lane offsets fixed over the loop, the K tile as the scalar offset —
                        // no per-piece test on this path (the general issue_part() with its uniform branches on lo / K tail made the
                        // phase's load part longer than its MFMA part: measured 5-10 % slower than the un-staggered loop)
                        const unsigned ks = (unsigned)(kt_begin - nt_lo + kt + 1) * (BK * 2);
                        char* sa = smem + (st ^ 1) * STAGE + wave * 1024;
                        char* sb = sa + A_BYTES;
                        constexpr int QA = ph == 0 ? 0 : (ph == 1 ? Q0 : Q0 + Q1), QB = ph == 0 ? Q0 : (ph == 1 ? Q0 + Q1 : (ph == 2 ? LOADS : 0));
#pragma unroll
                        for (int q = QA; q < QB; ++q) {
                            if (q < A_IT) glds16_buf(rs_a, aoff[q < A_IT ? q : 0], ks, sa + q * (RPI * 128));
                            else glds16_buf(rs_whi, woff[q >= A_IT ? q - A_IT : 0], ks, sb + (q - A_IT) * (RPI * 128));
                        }
                    }
                    if (ph == 3) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    bar1();
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NI; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
                    bar2();
                });
            }
            if (grp == 0) __builtin_amdgcn_s_barrier();               // group 0 waits for group 1's last phase
        }
    } else if (STAGES == 2) {
        // one tile in flight: the plain barrier carries the vmcnt(0) that lands the DMA
        issue_tile(0, 0);
        __syncthreads();
        // The second-dispatched half of the waves (4-7: one per SIMD, the arbitration losers) issues its share of the
        // next tile's DMA in the MIDDLE of its MFMA stream instead of together with waves 0-3 right after the barrier
        // (s_memtime timeline: 1870 vs 690 cycles per tile in the issue segment, with waves 0-3 then idling ~1400
        // cycles at the barrier): each SIMD then has one wave issuing DMA while the other runs MFMAs.
        const bool late = NW == 8 && wave >= 4 && wave_on && ntot >= 8;   // 2-5 % at long K
        // The e4m3 lo tiles run in a loop of their own (same pipeline, same tile counter): one MFMA kind per loop keeps the
        // register allocator from moving accumulator blocks between the two passes (a shared loop spilled 170 registers).
        const int n8 = nt_w + (lo8 ? nt_lo : 0);
        if constexpr (WS) {
            for (int kt = 0; kt < nt_w; ++kt) {        // the weight part: fp16 tiles in a loop of their own, then the one scaling
                if (!late) issue_tile(kt + 1, (kt + 1) & 1);          // (a hi tile always follows: kt + 1 < ntot)
                if (wave_on) {
                    compute(kt & 1, late ? kt + 1 : -1);
                    if (kt + 1 == nt_w) scale_lo();
                }
                __syncthreads();
            }
        }
        for (int kt = nt_w; kt < n8; ++kt) {           // (no mid-stream DMA issue here: the lo pass is 3-20 short tiles)
            if (kt + 1 < ntot) issue_tile(kt + 1, (kt + 1) & 1);
            if (wave_on) compute8(kt & 1, kt - nt_w);
            __syncthreads();
        }
        for (int kt = n8; kt < ntot; ++kt) {
            const bool nxt = kt + 1 < ntot;
            if (nxt && !late) issue_tile(kt + 1, (kt + 1) & 1);
            if (wave_on) {
                compute(kt & 1, (nxt && late) ? kt + 1 : -1);
                if (!WS && !lo8 && kt + 1 == nt_lo) scale_lo();
            }
            __syncthreads();
        }
    } else {
        // ring of three stages, TWO tiles in flight.  Counted waits: after issuing tile kt+2 only its LOADS
        // DMA instructions may stay outstanding, i.e. tile kt+1 has landed; the raw s_barrier (no compiler
        // vmcnt(0)) then publishes every wave's part of it and retires all reads of the stage being recycled.
        issue_tile(0, 0);
        if (ntot > 1) {
            issue_tile(1, 1);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LOADS) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        int st = 0;
        const int n8 = nt_w + (lo8 ? nt_lo : 0);
        if constexpr (WS) {
            for (int kt = 0; kt < nt_w; ++kt) {                       // the weight part (see the two-stage loop)
                const bool ahead = (kt + 2) < ntot;
                if (ahead) issue_tile(kt + 2, st == 0 ? 2 : st - 1);
                if (wave_on) {
                    compute(st);
                    if (kt + 1 == nt_w) scale_lo();
                }
                if (ahead) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LOADS) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                st = (st == 2) ? 0 : st + 1;
            }
        }
        for (int kt = nt_w; kt < n8; ++kt) {                          // e4m3 lo tiles (see the two-stage loop)
            const bool ahead = (kt + 2) < ntot;
            if (ahead) issue_tile(kt + 2, st == 0 ? 2 : st - 1);
            if (wave_on) compute8(st, kt - nt_w);
            if (ahead) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LOADS) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            st = (st == 2) ? 0 : st + 1;
        }
        for (int kt = n8; kt < ntot; ++kt) {
            const bool ahead = (kt + 2) < ntot;
            if (ahead) issue_tile(kt + 2, st == 0 ? 2 : st - 1);      // (kt + 2) % 3
            if (wave_on) {
                compute(st);
                if (!WS && !lo8 && kt + 1 == nt_lo) scale_lo();
            }
            if (ahead) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LOADS) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            st = (st == 2) ? 0 : st + 1;
        }
    }

    // ------------------------------ epilogue ------------------------------
    if (!wave_on) return;                       // row group of another workgroup (tail split)
    const int mw = m0 + wm * (MI * 32), nw = n0 + wn * (NI * 32);
    if constexpr ((EPI & E_GENERIC) != 0) {
        epi_generic<MI, NI>(p, acc, lane, mw, nw);
    } else {
        if constexpr ((EPI & E_VT) != 0) {
            if (n0 >= p.n_split) { epi_vt<MI, NI>(p, acc, lane, mw, nw); return; }
        }
        if constexpr (EPI == (E_R1 | E_O32) || EPI == E_O32) {
            // (uniform) full tile, no activation: the direct epilogue (round 6; PNC_OPT_GEMM_FUSE_LN + 2, A/B: the staged one)
            if (direct_epi && p.act == PNC_ACT_NONE && m0 + BM <= p.M && n0 + BN <= p.N && !split_rows && ksplit == 1) {
                epi_direct_o32<MI, NI, (EPI & E_R1) != 0>(p, acc, lane, RowLinear{mw}, nw);
                return;
            }
        }
        float* ep = reinterpret_cast<float*>(smem) + wave * (32 * EPITCH);
        __syncthreads();                        // every wave is done reading operand tiles from LDS
        if constexpr (GEGLU) {
            epi_geglu<MI, NI>(p, acc, ep, lane, mw, nw, reinterpret_cast<const float*>(smem + RING_BYTES));
        } else {
            if constexpr ((EPI & E_LN) != 0) {
                static_assert(WGN == 2, "the fused LayerNorm pairs the two waves of a row");
                float2* lnb = reinterpret_cast<float2*>(reinterpret_cast<float*>(smem) + NW * (32 * EPITCH));
                epi_fast<MI, NI, EPI>(p, acc, ep, lane, RowLinear{mw}, nw, p.N, lnb + wave * 64, lnb + (wave ^ 1) * 64);
            } else {
                float* gs_tab = reinterpret_cast<float*>(smem) + NW * (32 * EPITCH) + wave * (NI * 16);
                epi_fast<MI, NI, (EPI & ~E_VT)>(p, acc, ep, lane, RowLinear{mw}, nw, (EPI & E_VT) ? p.n_split : p.N, nullptr, nullptr,
                                                (EPI & E_GS) ? gs_tab : nullptr);   // E_GELU rides along
            }
        }
    }
