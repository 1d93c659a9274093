// gemm_stencil_tile_body.inc — the body of stencil_tile_kernel / stencil_tile_ws_kernel (gemm_stencil_tile.hip), included as text
// inside both.  In scope: the kernels' template parameters and arguments, `constexpr bool WS` and `const void* wlo16` (NULL when !WS).
    const PncGemmParams& p = pin;
    constexpr int TW = 1 << TWS, TH = 256 / TW;
    constexpr int IPS = 18;                                 // half-tile iterations per 64-channel slice: 9 taps x 2
    constexpr int HW2 = TW + 2, HROWS = (TH + 2) * HW2;
    constexpr int HBLK = (HROWS + 7) / 8;                   // 1-KB DMA pieces (8 halo rows of 128 B)
    constexpr int HBYTES = HBLK * 1024;
    constexpr int BN = NI * 64, NW = 8, WGN = 2, MI = 2;
    constexpr int WHB = BN * 64;                            // bytes of a W half tile: BN rows x 32 channels
    constexpr int WBLK = WHB / 1024;                        // its 1-KB DMA pieces (16 W rows x 64 B each): 16 / 20
    constexpr int W_IT = (WBLK + NW - 1) / NW;
    constexpr int H_IT = (HBLK + NW - 1) / NW;              // halo pieces per wave and slice: 6
    constexpr int ENI = 2, EPITCH = ENI * 32 + 4;
    static_assert(HW2 % 2 == 0, "the halo swizzle takes the address parity from the halo column");
    static_assert(2 * HBYTES + 3 * WHB <= 160 * 1024, "LDS budget");
    static_assert(2 * HBYTES + 3 * WHB >= NW * 32 * EPITCH * 4, "epilogue staging fits the operand buffers");
    static_assert(H_IT <= IPS, "one halo piece per wave and half-tile iteration");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const halo = smem;
    char* const wring = smem + 2 * HBYTES;

    const half_t* __restrict__ A = reinterpret_cast<const half_t*>(p.A);
    const half_t* __restrict__ A_lo = reinterpret_cast<const half_t*>(p.A_lo);
    const half_t* __restrict__ Wt = reinterpret_cast<const half_t*>(p.W);

    const int tiles_x = p.Wout >> TWS, per_frame = (p.Hout / TH) * tiles_x;
    const int tiles_m = (p.M / (p.Hout * p.Wout)) * per_frame, tiles_n = (p.N + BN - 1) / BN;
    // Tail split (as in gemm_kernel.h): the tiles of a sparse last round are each run by tail_f workgroups that own 256 / tail_f of
    // the tile's pixels (whole tile rows); the waves of the other rows skip their reads, MFMAs and epilogue, only the halo rows
    // the part needs are staged, all waves still stage W.  Rows of a GEMM are independent: bit-identical to the unsplit launch.
    int tile, part = 0;
    if ((int)blockIdx.x < nfull) {
        tile = xcd_remap(blockIdx.x, nfull);
    } else {
        const int j = (int)blockIdx.x - nfull;
        tile = nfull + j / tail_f; part = j - (j / tail_f) * tail_f;
    }
    const bool split = (int)blockIdx.x >= nfull && tail_f > 1;
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
    const int f = tm / per_frame, trem = tm - f * per_frame;
    const int ty = trem / tiles_x, tx = trem - ty * tiles_x;
    const int Y0 = ty * TH, X0 = tx << TWS, n0 = tn * BN;       // halo row hy / column hx = image row Y0 - 1 + hy, column X0 - 1 + hx
    const int64_t img_base = (int64_t)f * p.Hin * p.Win * p.Cin;
    const int base_m = (f * p.Hout + Y0) * p.Wout + X0;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;
    const int rows_lo = split ? part * (256 / tail_f) : 0, rows_hi = split ? rows_lo + 256 / tail_f : 256;
    const bool wave_on = (wm * 64 >= rows_lo) && (wm * 64 < rows_hi);
    // halo pieces (8 halo rows each) that hold tile rows rows_lo / TW - 1 .. rows_hi / TW: the others are never read
    const int pc_lo = ((rows_lo >> TWS) * HW2) >> 3, pc_hi = (((rows_hi >> TWS) + 2) * HW2 + 7) >> 3;

    // Operands reach LDS through buffer resources (common.h: glds16_buf; 4-7 % over per-lane 64-bit pointers on every conv shape):
    // base = this tile's frame of each activation plane / the tile's first weight row, per-lane 32-bit byte offsets that do not
    // change along K (the slice / half tile enters as the scalar offset); PNC_BUF_OOB offsets read as zero (padding, N tail).
    // x_halo_off (a view band): image columns -1 and Win are read from the block [2][frames][Hin][Cin] at A + x_halo_off, beyond the frame
    const bool xh = p.x_halo_off != 0;
    const unsigned frame_bytes = xh ? 0x7FFFFF00u : (unsigned)(p.Hin * p.Win * p.Cin) * 2u;
    const int64_t xh_rel = p.x_halo_off - img_base + (int64_t)f * p.Hin * p.Cin;      // this frame's rows of the left column
    const int64_t xh_side = (int64_t)(p.M / (p.Hout * p.Wout)) * p.Hin * p.Cin;        // ... of the right column, from there
    const buffer_rsrc_t rs_a = make_rsrc(A + img_base, frame_bytes);
    const buffer_rsrc_t rs_lo = make_rsrc((A_lo ? A_lo : A) + img_base, frame_bytes);
    const buffer_rsrc_t rs_w = make_rsrc(Wt + (int64_t)n0 * p.ldw, 0x7FFFFF00u);
    // split weights: W's lo plane (W's layout and leading dimension), read by the second run of the lo pass
    const bool wl16 = !WS && A_lo && p.W_lo != nullptr;
    const buffer_rsrc_t rs_wlo = make_rsrc((WS ? reinterpret_cast<const half_t*>(wlo16) : (wl16 ? reinterpret_cast<const half_t*>(p.W_lo) : Wt)) +
                                               (int64_t)n0 * p.ldw, 0x7FFFFF00u);

    // ---- halo DMA: piece b = halo rows 8b .. 8b+7; lane l fills slot (l&7) of row 8b + (l>>3) with the source chunk
    // slot ^ ((hx>>1)&7), hx = the row's halo COLUMN.  The 16 lanes of a ds_read_b128 group read 16 consecutive pixels of
    // one or two tile rows = 16 consecutive halo columns (whatever the tap), i.e. all 16 (parity, hx>>1) pairs.
    auto halo_off = [&](int b) -> unsigned {            // this lane's byte offset of piece b inside the frame (the same for every slice)
        const int hr = b * 8 + (lane >> 3);
        const int hy = hr / HW2, hx = hr - hy * HW2;
        const int c8 = (lane & 7) ^ ((hx >> 1) & 7);
        const int iy = Y0 - 1 + hy, ix = X0 - 1 + hx;
        const bool yok = (hr < HROWS) && (iy >= 0) && (iy < p.Hin), xin = (ix >= 0) && (ix < p.Win);
        const bool ok = yok && (xin || (xh && ix >= -1 && ix <= p.Win));
        unsigned off = ok ? (unsigned)((iy * p.Win + ix) * p.Cin + c8 * 8) * 2u : PNC_BUF_OOB;           // out of the image: zeros
        if (ok && !xin) off = (unsigned)(xh_rel + (ix < 0 ? 0 : xh_side) + iy * p.Cin + c8 * 8) * 2u;
        return off;
    };
    auto request_halo = [&](bool lo_plane, int cc, int buf, int b, unsigned off) {
        glds16_buf(lo_plane ? rs_lo : rs_a, off, (unsigned)cc << 7, halo + buf * HBYTES + b * 1024);
    };
    auto issue_halo = [&](bool lo_plane, int cc, int buf, int b) { request_halo(lo_plane, cc, buf, b, halo_off(b)); };
    // ---- W DMA: half tile k = 32 channels of K tile k/2 = k offset 32 k of the packed [N][(ci/64, tap, ci%64)] weights.
    // LDS row R (128 B) = W rows 2R, 2R+1; slot = (n&1)*4 + (c ^ ((R>>1)&3)), c = 16-byte chunk of the 64-byte half row.
    const int nW = WBLK / NW + (wave < (WBLK % NW) ? 1 : 0);      // DMA instructions of this wave per half tile
    unsigned woff[W_IT];
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
        const int R = (wave + NW * i) * 8 + (lane >> 3), slot = lane & 7;
        const int nl = 2 * R + (slot >> 2);
        const int c4 = (slot & 3) ^ ((R >> 1) & 3);
        woff[i] = (n0 + nl < p.N) ? (unsigned)(nl * p.ldw + c4 * 8) * 2u : PNC_BUF_OOB;
    }
    auto issue_w = [&](int k, int stage, bool wlo = false) {      // wlo (uniform): the half tile of W's lo plane
        char* sb = wring + stage * WHB + wave * 1024;
        const buffer_rsrc_t rs = wlo ? rs_wlo : rs_w;
#pragma unroll
        for (int i = 0; i < W_IT; ++i)
            if (wave + NW * i < WBLK) glds16_buf(rs, woff[i], (unsigned)k << 6, sb + i * (NW * 1024));
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // this lane's fragment rows.  A: tile-local output row R -> halo row / column of tap 0; B: W row -> LDS row, slot
    const int frow = lane & 31, fk = lane >> 5;
    int hp0[MI], hx0[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int R = wm * 64 + i * 32 + frow;
        hx0[i] = R & (TW - 1);
        hp0[i] = (R >> TWS) * HW2 + hx0[i];
    }
    const int b_row = ((wn * (NI * 32) + frow) >> 1) * 128 + ((frow & 1) << 6);
    const int b_swz = (frow >> 2) & 3;                 // (R>>1)&3: blocks of 32 W rows shift R by 16

    // Fragments of one k-step (16 channels) of half tile (hbuf, tap, half, stage) -> register buffer b.  Explicit
    // ds_read_b128: the compiler's counter model waits lgkmcnt(0) across the loop's back edge, which would expose the latency of
    // the reads just issued (A/B on the device: 2-4 % at long K); the waits for these reads are written out in the loop below.
    half8v af[2][MI], bf[2][NI];
    // LDS addresses of those fragments (the pipeline computes them one batch AHEAD of the reads: round 6) ...
    auto frag_addr = [&](int hbuf, int tap, int half, int stage, int ks, unsigned (&a_addr)[MI], unsigned& b_addr) {
        const char* sa = halo + hbuf * HBYTES;
        const char* sb = wring + stage * WHB + b_row;
        const int ky = tap / 3, kx = tap - ky * 3;
        const int toff = ky * HW2 + kx;
        const int c4 = ks * 2 + fk;
#pragma unroll
        for (int i = 0; i < MI; ++i)
            a_addr[i] = (unsigned)(uintptr_t)(sa + (hp0[i] + toff) * 128 + (((half * 4 + c4) ^ (((hx0[i] + kx) >> 1) & 7)) << 4));
        b_addr = (unsigned)(uintptr_t)(sb + ((c4 ^ b_swz) << 4));
    };
    // ... and the reads
    auto frag_read = [&](const unsigned (&a_addr)[MI], unsigned b_addr, auto b_) {
        constexpr int b = decltype(b_)::value;
#pragma unroll
        for (int i = 0; i < MI; ++i) asm volatile("ds_read_b128 %0, %1" : "=v"(af[b][i]) : "v"(a_addr[i]));
#define PNC_STENCIL_RD_B(J)                                                                                            \
    if constexpr (NI > J)                                                                                              \
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bf[b][J < NI ? J : 0]) : "v"(b_addr), "n"(J * 16 * 128));
        PNC_STENCIL_RD_B(0) PNC_STENCIL_RD_B(1) PNC_STENCIL_RD_B(2) PNC_STENCIL_RD_B(3) PNC_STENCIL_RD_B(4)
#undef PNC_STENCIL_RD_B
    };
    auto frags = [&](int hbuf, int tap, int half, int stage, int ks, auto b_) {
        unsigned a_addr[MI], b_addr;
        frag_addr(hbuf, tap, half, stage, ks, a_addr, b_addr);
        frag_read(a_addr, b_addr, b_);
    };
    auto mfmas = [&](auto b_) {
        constexpr int b = decltype(b_)::value;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[b][i], bf[b][j], acc[i][j], 0, 0, 0);
    };
    const std::integral_constant<int, 0> B0{};
    const std::integral_constant<int, 1> B1{};

    // counted wait: everything but this wave's most recent W group (nW instructions) has landed
    auto wait_all_but_last_w = [&]() {
        if (nW == W_IT) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(W_IT) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(W_IT - 1) : "memory");
    };

    // Slices in execution order: with a precise operand the lo plane's nslices first, then the hi plane's; with split weights the
    // hi plane's slices run twice — against W's lo plane (still part of the lo pass), then against W
    const int nslices = p.Cin >> 6, nq1 = nslices * IPS;              // half tiles of one pass
    const int npass = WS ? 2 : (A_lo ? (wl16 ? 3 : 2) : 1);
    const int wlo_pass = WS ? 0 : 1;                                  // the pass that reads W's lo plane, where there is one
    const int ns_tot = npass * nslices, nq = ns_tot * IPS;
    const int nq_lo = (npass - 1) * nq1;                              // half tiles of the lo pass: the accumulators are scaled after them
    auto slice_plane = [&](int gs) { return !WS && A_lo && gs < nslices; };      // true: the lo plane
    auto slice_cc = [&](int gs) { return gs >= 2 * nslices ? gs - 2 * nslices : (gs >= nslices ? gs - nslices : gs); };
    int wpass = 0;                                                    // pass of the W half tile the loops issue next (1 = W's lo plane when wl16)

    // STAGGERED schedule (round 5, PNC_OPT_GEMM_STAGGER; gemm_kernel.h has the story): one PHASE per k-step —
    //     fragment reads of the k-step [+ DMA in the odd phases] | s_barrier | MI x NI MFMAs | s_barrier —
    // with waves 4-7 one barrier behind waves 0-3.  The odd phase of half tile q issues one halo piece of the next slice (as the
    // pipeline below does) and W half tile q + 2 into the ring stage of q - 1: every wave of BOTH groups finished its reads of that
    // stage two barriers earlier (its last reads sat in phase (q - 1, 1); the other group's lgkmcnt(0) after the first barrier of
    // that phase is passed by the time this group is behind the second barrier of phase (q, 0)).  The counted wait in the same
    // phase leaves only the W group just issued in flight: W(q + 1), read from the next phase on, has landed.  Same K order
    // and MFMA order per accumulator: bit-identical to the pipeline below.
    if (stagger == 1) {
        const int grp = wave >> 2;
#pragma unroll
        for (int i = 0; i < H_IT; ++i)
            if (wave + NW * i >= pc_lo && wave + NW * i < pc_hi && wave + NW * i < HBLK) issue_halo(slice_plane(0), 0, 0, wave + NW * i);
        issue_w(0, 0, WS);
        if (nq > 1) issue_w(1, 1, WS);                          // (nq1 >= 18: the first three half tiles are of pass 0)
        if (nq > 2) issue_w(2, 2, WS);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (grp == 1) __builtin_amdgcn_s_barrier();
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
        int st = 0, gs = 0, r = 0, w2 = 3 % nq1;              // w2 = (q + 2) mod nq1 at the issue point of iteration q >= 1
        for (int q = 0; q < nq; ++q) {
            if (wave_on) frags(gs & 1, r >> 1, r & 1, st, 0, B0);
            bar1();
            if (wave_on) mfmas(B0);
            bar2();
            if (wave_on) frags(gs & 1, r >> 1, r & 1, st, 1, B1);
            if (r < H_IT && gs + 1 < ns_tot && wave + NW * r >= pc_lo && wave + NW * r < pc_hi && wave + NW * r < HBLK)
                issue_halo(slice_plane(gs + 1), slice_cc(gs + 1), (gs + 1) & 1, wave + NW * r);
            if (q >= 1) {
                if (q + 2 < nq) {
                    issue_w(w2, st == 0 ? 2 : st - 1, (WS || wl16) && wpass == wlo_pass);         // the stage of half tile q - 1 = (q + 2) mod 3
                    wait_all_but_last_w();
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                if (++w2 == nq1) { w2 = 0; ++wpass; }
            }
            bar1();
            if (wave_on) mfmas(B1);
            bar2();
            if ((WS || A_lo) && q + 1 == nq_lo) {
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[i][j][e] *= LO_INV;
            }
            if (++r == IPS) { r = 0; ++gs; }
            st = (st == 2) ? 0 : st + 1;
        }
        if (grp == 0) __builtin_amdgcn_s_barrier();
    } else {
    // Software pipeline over half tiles q (two k-steps each), the barrier in the MIDDLE of q's MFMA stream:
    //   reads(q, ks1) | MFMA(q, ks0) | wait: W(q+1) landed, own reads of q done | s_barrier | DMA: halo piece, W(q+3) -> stage of q |
    //   reads(q+1, ks0) | MFMA(q, ks1)
    // so every fragment read runs under the other k-step's MFMAs and three half tiles are landed / in flight.
#pragma unroll
    for (int i = 0; i < H_IT; ++i)
        if (wave + NW * i >= pc_lo && wave + NW * i < pc_hi && wave + NW * i < HBLK) issue_halo(slice_plane(0), 0, 0, wave + NW * i);
    issue_w(0, 0, WS);
    issue_w(1, 1, WS);
    wait_all_but_last_w();
    __builtin_amdgcn_s_barrier();
    issue_w(2, 2, WS);
    if (wave_on) frags(0, 0, 0, 0, 0, B0);
    int st = 0, gs = 0, r = 0, w3 = 3;              // w3 = (q + 3) mod nq1: the W half tile issued in iteration q
    // Round 6: the fragment ADDRESSES are computed one batch ahead of the reads (ta / tb: the reads at the top of the next iteration, under
    // the second MFMA batch; na / nb: the reads behind the barrier, under the first), so that only the ds_reads themselves sit between
    // two MFMA batches: 3-5 % on every level-0 / level-1 shape (profiles/round6/stencil_dma_late_r6.log; requesting the DMA behind the
    // second batch instead of in front of it bought 2-3 % alone and nothing on top of this).  stagger & 2 (A/B): the round-5 placement
    const bool addr_late = (stagger & 2) != 0;
    unsigned ta[MI], tb, na[MI], nb;
    if (!addr_late) frag_addr(0, 0, 0, 0, 1, ta, tb);
    for (int q = 0; q < nq; ++q) {
        // next half tile's coordinates
        int r1 = r + 1, gs1 = gs;
        if (r1 == IPS) { r1 = 0; ++gs1; }
        const int st1 = (st == 2) ? 0 : st + 1;
        if (wave_on) {
            if (addr_late) frags(gs & 1, r >> 1, r & 1, st, 1, B1);
            else frag_read(ta, tb, B1);
            asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(MI + NI) : "memory");   // buffer 0 (the older reads) is in
            __builtin_amdgcn_sched_barrier(0);
            mfmas(B0);
            __builtin_amdgcn_sched_barrier(0);
            if (!addr_late) frag_addr(gs1 & 1, r1 >> 1, r1 & 1, st1, 0, na, nb);
        }
        // (the halo piece's offset arithmetic — a division, the image-edge tests — under the batch too)
        const bool halo_on = r < H_IT && gs + 1 < ns_tot && wave + NW * r >= pc_lo && wave + NW * r < pc_hi && wave + NW * r < HBLK;
        unsigned hoff = 0;
        if (halo_on && !addr_late) hoff = halo_off(wave + NW * r);
        __builtin_amdgcn_sched_barrier(0);
        if (q + 2 < nq) wait_all_but_last_w();                 // in flight: W(q+1), [halo piece, W(q+2)]
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // this wave has read everything it needs of stage st
        __builtin_amdgcn_s_barrier();
        // halo buffer (gs+1)&1 was last read in slice gs-1; stage st by half tile q (all waves are past their reads of it)
        if (halo_on) {
            if (addr_late) issue_halo(slice_plane(gs + 1), slice_cc(gs + 1), (gs + 1) & 1, wave + NW * r);
            else request_halo(slice_plane(gs + 1), slice_cc(gs + 1), (gs + 1) & 1, wave + NW * r, hoff);
        }
        if (q + 3 < nq) issue_w(w3, st, (WS || wl16) && wpass == wlo_pass);
        if (++w3 == nq1) { w3 = 0; ++wpass; }
        if (wave_on) {
            if (q + 1 < nq) {
                if (addr_late) frags(gs1 & 1, r1 >> 1, r1 & 1, st1, 0, B0);
                else frag_read(na, nb, B0);
            }
            __builtin_amdgcn_sched_barrier(0);
            mfmas(B1);
            __builtin_amdgcn_sched_barrier(0);
            if (!addr_late) frag_addr(gs1 & 1, r1 >> 1, r1 & 1, st1, 1, ta, tb);
        }
        __builtin_amdgcn_sched_barrier(0);
        if ((WS || A_lo) && q + 1 == nq_lo) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] *= LO_INV;
        }
        st = st1; r = r1; gs = gs1;
    }
    }
    __syncthreads();                            // every wave is done with the operand buffers
    if (!wave_on) return;                       // rows of another workgroup (tail split)

    // ------------------------------ epilogue ------------------------------
    if constexpr (EPI == E_O32) {
        if (!(stagger & 4) && p.act == PNC_ACT_NONE && n0 + BN <= p.N) {
            // fp32 output straight from the accumulators (round 6): lane (column c, half h) of a 32x32 block holds rows 8 q + 4 h + e of column
            // c, so one store instruction writes two whole 128-byte row pieces — no LDS round trip (160 four-byte staging writes + 40 reads
            // per wave), same bytes to memory.  1.4-3.3 % per launch (profiles/round6/stencil_direct_epilogue_r6.log); acc + bias as in
            // epi_fast: bit-identical.  stagger & 4 (A/B, PNC_OPT_GEMM_FUSE_LN + 2): the staged epilogue
            epi_direct_o32<MI, NI, false>(p, acc, lane, RowHalo<TWS>{base_m, p.Wout, wm * 64}, n0 + wn * (NI * 32));
            return;
        }
    }
    float* ep = reinterpret_cast<float*>(smem) + wave * (32 * EPITCH);
    epi_fast<MI, NI, EPI>(p, acc, ep, lane, RowHalo<TWS>{base_m, p.Wout, wm * 64}, n0 + wn * (NI * 32), p.N);
