// gemm_geglu_persist_body.inc — the body of gemm_geglu_persist_kernel / gemm_geglu_persist_ws_kernel (gemm_kernel.h), included as text
// inside both.  In scope: the kernels' template parameters and arguments, `constexpr bool WS` and `const void* wlo16` (NULL when !WS).
    PncGemmParams p = pin;
    constexpr int NW = WGM * WGN, MI = BM / WGM / 32, NI = BN / WGN / 32, RPI = NW * 8, A_IT = BM / RPI, B_IT = BN / RPI;
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES, RING_BYTES = 2 * STAGE;
    static_assert(BM % RPI == 0 && BN % RPI == 0, "tile rows must be a multiple of the DMA row group");
    static_assert(NI % 2 == 0, "GEGLU pairs value / gate column blocks inside a wave");
    extern __shared__ __attribute__((aligned(16))) char smem[];         // the operand ring: the ONLY memory LDS-DMA writes
    // Everything the epilogue reads lives in LDS objects of its own: hipcc puts s_waitcnt vmcnt(0) in front of any LDS access that
    // may alias an LDS-DMA in flight — with the staging inside the ring (as in gemm_glds_kernel) the epilogue would wait for the
    // prefetched K tile before its first table read.  160 KB = ring 128 + table 16 + one 2 KB slab of staging per wave 16.
    __shared__ __attribute__((aligned(16))) float s_phi[PHI_BYTES / 4];
    __shared__ __attribute__((aligned(16))) half_t s_stage[NW][32 * 32];
    const half_t* __restrict__ A = reinterpret_cast<const half_t*>(p.A);
    const half_t* __restrict__ Wt = reinterpret_cast<const half_t*>(p.W);
    const int tiles_n = p.N / BN, tiles_m = p.M / BM, ntile = tiles_m * tiles_n;
    // WS: the K loop of an output tile runs 2 nk1 VIRTUAL K tiles — the weight part (A, W's fp16 lo plane) over the nk1 tiles of K, the
    // one 2^-11 scaling, then (A, W) over the same tiles: the order of parts of gemm_glds_ws_kernel
    const int nk1 = p.K / BK, nk = WS ? 2 * nk1 : nk1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;
    const int srow = wave * 8 + (lane >> 3);
    const int schunk = (lane & 7) ^ ((srow >> 1) & 7);
    const int frow = lane & 31, fk = lane >> 5;

    // virtual block v -> output tile: the XCD-contiguous ranges and the grouped (tm, tn) order of gemm_glds_kernel
    auto tile_origin = [&](int v, int& m0, int& n0) {
        const int tile = xcd_remap(v, ntile);
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
        m0 = tm * BM; n0 = tn * BN;
    };
    unsigned aoff[A_IT], woff[B_IT];                       // per-lane byte offsets inside a tile's windows: the same for every tile
#pragma unroll
    for (int i = 0; i < A_IT; ++i) aoff[i] = (unsigned)((i * RPI + srow) * p.lda + schunk * 8) * 2u;
#pragma unroll
    for (int i = 0; i < B_IT; ++i) woff[i] = (unsigned)((i * RPI + srow) * p.ldw + schunk * 8) * 2u;
    auto issue_part = [&](int m0, int n0, int kt, int stage, auto q0_, auto q1_) __attribute__((always_inline)) {
        constexpr int Q0 = decltype(q0_)::value, Q1 = decltype(q1_)::value;       // DMA pieces [Q0, Q1): A row groups, then W row groups
        const buffer_rsrc_t rs_a = make_rsrc(A + (int64_t)m0 * p.lda, 0x7FFFFF00u);
        const bool wpart = WS && kt < nk1;                   // (uniform) a virtual tile of the weight part
        const buffer_rsrc_t rs_w = make_rsrc((wpart ? reinterpret_cast<const half_t*>(wlo16) : Wt) + (int64_t)n0 * p.ldw, 0x7FFFFF00u);
        char* sa = smem + stage * STAGE + wave * 1024;
        char* sb = sa + A_BYTES;
        const unsigned ks = (unsigned)(WS && !wpart ? kt - nk1 : kt) * (BK * 2);
#pragma unroll
        for (int i = 0; i < A_IT; ++i)
            if (i >= Q0 && i < Q1) glds16_buf(rs_a, aoff[i], ks, sa + i * (RPI * 128));
#pragma unroll
        for (int i = 0; i < B_IT; ++i)
            if (A_IT + i >= Q0 && A_IT + i < Q1) glds16_buf(rs_w, woff[i], ks, sb + i * (RPI * 128));
    };
    auto issue = [&](int m0, int n0, int kt, int stage) __attribute__((always_inline)) {
        issue_part(m0, n0, kt, stage, std::integral_constant<int, 0>{}, std::integral_constant<int, A_IT + B_IT>{});
    };

    for (int i = tid; i < PHI_BYTES / 16; i += 64 * NW)                 // the Phi table: once per workgroup, by plain stores
        reinterpret_cast<f32x4*>(s_phi)[i] = reinterpret_cast<const f32x4*>(phi_g)[i];
    f32x16 acc[MI][NI];
    auto compute = [&](int stage) {
        const char* sa = smem + stage * STAGE;
        const char* sb = sa + A_BYTES;
        half8v af[2][MI], bf[2][NI];
        auto frags = [&](int ks, int b) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
                af[b][i] = *reinterpret_cast<const half8v*>(sa + lds_off128(wm * (MI * 32) + i * 32 + frow, ks * 2 + fk));
#pragma unroll
            for (int j = 0; j < NI; ++j)
                bf[b][j] = *reinterpret_cast<const half8v*>(sb + lds_off128(wn * (NI * 32) + j * 32 + frow, ks * 2 + fk));
        };
        frags(0, 0);
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            if (ks + 1 < BK / 16) frags(ks + 1, (ks + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[ks & 1][i], bf[ks & 1][j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
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

    const bool direct16 = (stagger_min_in & 256) == 0;     // (+ 256, A/B: the round-3 epilogue through a 2 KB LDS slab per wave)
    const int stagger_min = stagger_min_in & 255;
    if (NW == 8 && wave >= 4 && !(stagger_min > 0 && nk >= stagger_min)) __builtin_amdgcn_s_setprio(1);
    int v = blockIdx.x;
    if (v >= ntile) return;
    int m0, n0, sp = 0;
    tile_origin(v, m0, n0);
    float pb[NI], pbn[NI];
    auto load_bias = [&](int n0_, float (&dst)[NI]) {
#pragma unroll
        for (int j = 0; j < NI; ++j) dst[j] = p.bias ? p.bias[n0_ + wn * (NI * 32) + j * 32 + (lane & 31)] : 0.0f;
    };
    load_bias(n0, pb);
    issue(m0, n0, 0, 0);
    // staggered schedule of the K loop (gemm_glds_kernel; PNC_OPT_GEMM_STAGGER): waves 4-7 one barrier behind waves 0-3 inside an
    // output tile's K loop, both groups aligned again before the epilogue (their epilogues run together, as before; run one behind
    // the other they would serialise: a group can do ONE phase while the other is in its epilogue).  The next output tile's first K
    // tile is requested in phases 0-2 of the LAST K tile instead of in front of the epilogue.
    const bool staggered = NW == 8 && stagger_min > 0 && nk >= (stagger_min == 1 ? 1 : stagger_min);
    const int grp = wave >> 2;
    while (true) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
        const int ls = (sp + nk - 1) & 1;       // the stage of the last K tile: every wave is done with it -> the epilogue's staging
        const int vn = v + gridDim.x;
        int m1 = 0, n1 = 0;
        if (staggered) {
            constexpr int LOADS = A_IT + B_IT, Q0 = (LOADS + 2) / 3, Q1 = (LOADS - Q0 + 1) / 2;
            const std::integral_constant<int, 0> C0{};
            const std::integral_constant<int, Q0> CQ0{};
            const std::integral_constant<int, Q0 + Q1> CQ1{};
            const std::integral_constant<int, LOADS> CQ2{};
            if (v == (int)blockIdx.x) {          // (uniform) first output tile: its K tile 0 was requested above (+ the Phi table's stores)
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            }                                    // (later tiles: landed and published by the previous tile's last phase)
            if (grp == 1) __builtin_amdgcn_s_barrier();
            if (vn < ntile) tile_origin(vn, m1, n1);
            half8v af[MI], bf[NI];
            for (int kt = 0; kt < nk; ++kt) {
                const int st = (sp + kt) & 1;
                const bool last = kt + 1 == nk;
                const bool nxt = !last || vn < ntile;
                const int nm0 = last ? m1 : m0, nn0 = last ? n1 : n0, nkt = last ? 0 : kt + 1;
#pragma unroll
                for (int ph = 0; ph < 4; ++ph) {
                    const char* sa = smem + st * STAGE;
                    const char* sb = sa + A_BYTES;
#pragma unroll
                    for (int i = 0; i < MI; ++i)
                        af[i] = *reinterpret_cast<const half8v*>(sa + lds_off128(wm * (MI * 32) + i * 32 + frow, ph * 2 + fk));
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        bf[j] = *reinterpret_cast<const half8v*>(sb + lds_off128(wn * (NI * 32) + j * 32 + frow, ph * 2 + fk));
                    if (nxt) {
                        if (ph == 0) {
                            if (last) load_bias(n1, pbn);         // BEFORE the DMA (vmcnt is in order)
                            issue_part(nm0, nn0, nkt, st ^ 1, C0, CQ0);
                        } else if (ph == 1) issue_part(nm0, nn0, nkt, st ^ 1, CQ0, CQ1);
                        else if (ph == 2) issue_part(nm0, nn0, nkt, st ^ 1, CQ1, CQ2);
                    }
                    if (ph == 3) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_barrier();
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NI; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_barrier();
                }
                if constexpr (WS) {
                    if (kt + 1 == nk1) scale_lo();
                }
            }
            if (grp == 0) __builtin_amdgcn_s_barrier();          // both groups past their last phase: the epilogues start together
        } else {
        __syncthreads();                        // K tile 0 of this output tile has landed; the previous epilogue's staging is retired
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + 1 < nk) issue(m0, n0, kt + 1, (sp + kt + 1) & 1);
            compute((sp + kt) & 1);
            if constexpr (WS) {
                if (kt + 1 == nk1) scale_lo();
            }
            __syncthreads();
        }
        if (vn < ntile) {                       // (uniform) the next output tile's first K tile, into the other stage
            tile_origin(vn, m1, n1);
            load_bias(n1, pbn);                 // BEFORE the DMA: nothing in the epilogue below may wait on vmcnt
            issue(m1, n1, 0, ls ^ 1);
        }
        }
        {   // epi_geglu's register path, slab by slab (same operations in the same order: bit-identical)
            half_t* out16 = reinterpret_cast<half_t*>(p.out16);
            typedef half_t __attribute__((may_alias)) half_st;
            typedef int4 __attribute__((may_alias)) int4_st;
            half_st* sb = reinterpret_cast<half_st*>(&s_stage[wave][0]);
            const int c = lane & 31, cl = lane & 3, rl = lane >> 2;
            const int mw = m0 + wm * (MI * 32), nw = n0 + wn * (NI * 32);
            static_for<NI / 2>([&](auto jc_) {
                constexpr int jc = decltype(jc_)::value * 2;
                const float bv = pb[jc], bg = pb[jc + 1];
                const int ncol0 = (nw + jc * 32) >> 1;
                static_for<MI>([&](auto i_) {
                    constexpr int i = decltype(i_)::value;
                    float gx[16], fr[16];
                    int ix[16];
                    float2 e[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        gx[r] = acc[i][jc + 1][r] + bg;
                        float t = fmaf(gx[r], PHI_SCALE, -PHI_X0 * PHI_SCALE);
                        t = __builtin_amdgcn_fmed3f(t, 0.0f, (float)PHI_N - 0.001f);
                        ix[r] = (int)t;
                        fr[r] = t - (float)ix[r];
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) e[r] = *reinterpret_cast<const float2*>(s_phi + 2 * ix[r]);
                    if (direct16) {
                        // round 6: the products leave through two-byte buffer stores straight from the registers (a lane holds one column of
                        // rows 8 q + 4 h + e: two 64-byte row pieces per instruction, the row inside the block as the scalar offset) instead of
                        // through the slab (16 two-byte staging writes + 2 reads + 2 sixteen-byte stores per
                        // block): FF1 −0.5 … −1.7 % at every level, step −0.3 ms (profiles/round6/ff1_direct_stores_r6.log).  Same values.
                        const buffer_rsrc_t ro = make_rsrc(out16 + (int64_t)(mw + i * 32) * p.ldc16, 0x7FFFFF00u);
                        const int vo = (4 * (lane >> 5) * p.ldc16 + ncol0 + c) * 2;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float prod = (acc[i][jc][r] + bv) * (gx[r] * fmaf(fr[r], e[r].y, e[r].x));
                            asm("" : "+v"(prod));
                            const half_t hp = (half_t)prod;
                            __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, hp), ro, vo, ((r & 3) + 8 * (r >> 2)) * p.ldc16 * 2, 0);
                        }
                    } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float prod = (acc[i][jc][r] + bv) * (gx[r] * fmaf(fr[r], e[r].y, e[r].x));
                        asm("" : "+v"(prod));
                        sb[mfma32_row(r, lane) * 32 + c] = (half_t)prod;
                    }
#pragma unroll
                    for (int ps = 0; ps < 2; ++ps) {
                        const int row = ps * 16 + rl;
                        const int4 v4 = *reinterpret_cast<const int4_st*>(sb + row * 32 + cl * 8);
                        *reinterpret_cast<int4_st*>(out16 + (int64_t)(mw + i * 32 + row) * p.ldc16 + ncol0 + cl * 8) = v4;
                    }
                    }
                });
            });
        }
        if (vn >= ntile) break;
        v = vn; m0 = m1; n0 = n1; sp = ls ^ 1;
#pragma unroll
        for (int j = 0; j < NI; ++j) pb[j] = pbn[j];
    }
