// adsb_scan_fast_body.inc -- the body of the fast scan's kernels, k_scan_fast, k_scan_fix and k_scan_fix2
// (adsb_scan_fast.hip), included into each of them; not a header.  In scope: the kernel's template parameters FROM_MAG,
// SELFTEST, FUSED, FIELDS, U8, its `p` and LDS (s, fs, hf), the constexpr flags FIX and FIX2 and `fixt` (the
// single-bit repair table in LDS when FIX, else null).
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const uint32_t n_tiles = p.n_chunks * kTilesPerChunk;
    FSTAMP(0);
    if constexpr (FUSED) {
        if (blockIdx.x == 0 && tid == 0) {
            const unsigned long long t0 = (unsigned long long)wall_clock64();
            st_shared<true>(&p.ctr->t_start[0], (uint32_t)t0);
            st_shared<true>(&p.ctr->t_start[1], (uint32_t)(t0 >> 32));
        }
        for (int i = tid; i < 3 * 256; i += kThreads) fs.x56[i] = p.tables[kTabX56 * 256 + i];
        if (tid < 168) fs.bits[tid] = p.tables[kTabBitsOff + tid];
        // an icao_flush retired a bitmap: every workgroup clears its share (k_records does it for the
        // passes of three launches)
        if (p.clean_bitmap) bitmap_clear(p.clean_bitmap, p.bitmap_lg, blockIdx.x * kThreads + tid, gridDim.x * kThreads);
        // ... or (a context for passes of a few buffers: folded bitmaps) the pass starts on the NEXT bitmap of the
        // rotation and clears it itself: the first workgroup does -- 64 KB written through, acknowledged, then the
        // flag -- and every other one checks the flag behind its first tile's loads, long before it first sets or
        // tests a bit (bitmap_wait below).  Nobody else is using that bitmap: there is one more than passes in flight.
        if (p.bitmap_fresh && blockIdx.x == 0) {
            const uint32_t words = bitmap_alloc_words(p.bitmap_lg), bits = bitmap_words(p.bitmap_lg);
            for (uint32_t v = (uint32_t)tid; v < words; v += kThreads)
                st_shared<true>(&p.bitmap[v], (v == 0u || v == bits) ? 1u : 0u);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) st_shared<true>(&p.ctr->bitmap_ready, 1u);
        }
    }

    // ---------------------------------------------------------------- P0 once per workgroup
    for (int i = tid; i < 3 * 256; i += kThreads) s.tab[i] = p.tables[kTabF * 256 + i];
    for (int i = tid; i < 316; i += kThreads) {
        const uint32_t v = p.tables[kTabR16Off + i];
        if (i < 16)
            s.r16[i] = v;
        else  // plane row byte offset -> its LDS address, so that the trial stage adds nothing
            s.field[i - 16] = v + (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)s.plane;
    }
    if (tid < kPlanes) s.plane[tid * kPlaneDw + kPlaneDw - 1] = 0;  // read slack
    if (tid < 2) s.nhit[tid] = 0;
    uint32_t fix_mult = 0;
    if constexpr (FIX) {   // (read by the trials, behind the first tile's barriers)
        for (int i = tid; i < kFixSlots; i += kThreads) fixt[i] = p.tables[kTabFixOff + i];
        fix_mult = p.tables[kTabFixOff + kFixSlots];
    }
    // FIX2: the pair table stays in global memory (L2); only its two multipliers are read here
    const uint4 *fix2 = nullptr;
    uint32_t fix2_m0 = 0, fix2_m1 = 0;
    if constexpr (FIX2) {
        fix2_m0 = p.tables[kTabFix2Off];
        fix2_m1 = p.tables[kTabFix2Off + 1];
        fix2 = (const uint4 *)(p.tables + kTabFix2Off + 4);
    }
    if constexpr (U8) {   // the widening table, read by P1 of the first tile already
        for (int i = tid; i < 256; i += kThreads) u8_table_lds()[i] = (float)(int16_t)p.u8_table[i];
        __syncthreads();
    }

    const uint32_t seg_cap = p.seg_cap;
    const uint32_t my_seg = blockIdx.x * kWaves + (uint32_t)(tid >> 6);
    uint64_t *const seg = p.ap + (uint64_t)my_seg * seg_cap;  // this wave's own AP segment
    uint32_t ap_count = 0, cand_count = 0;  // wave-uniform running totals of this wave

    uint4 pre[kLoadsPerThread];
    // Which tiles this workgroup walks.  Blocks b, b + 8, b + 16, ... run on the same XCD (observed
    // placement, used for speed only), so each XCD gets one contiguous eighth of the tiles and its
    // blocks walk it side by side: the 368 samples two neighbouring tiles share are then read from
    // HBM once and found in that XCD's L2 by the neighbour.  Any other grid: plain round robin.
    uint32_t t_first = blockIdx.x, t_end = n_tiles, t_stride = gridDim.x;
    // (a one-launch pass: tile = block -- its workgroups publish and wait for each other in tile order by their
    // block index, and a pass of a few buffers has nothing to gain from the placement)
    if (!FUSED && (gridDim.x & 7u) == 0 && n_tiles >= gridDim.x) {
        const uint32_t x = blockIdx.x & 7u;
        t_first = ((x * n_tiles) >> 3) + (blockIdx.x >> 3);
        t_end = ((x + 1u) * n_tiles) >> 3;
        t_stride = gridDim.x >> 3;
    }
    if constexpr (FUSED && !FROM_MAG) {
        // The samples may still be on their way into the pinned buffer (adsb_demod_iq copies them there while this
        // launch travels to the device): wait until the host has copied what this tile reads.  One thread polls
        // the host's word over the link (~1.5 us a poll; the whole copy is ~10 us); bounded -- a host that never
        // finishes is reported as an overflow, and the pass is redone once the call has all its samples.
        if (p.src_ready != nullptr && t_first < t_end) {
            const TileRef r0 = tile_ref<FROM_MAG>(p, t_first);
            const long long last = min((long long)r0.len, (long long)r0.jbase - kPad - kLead + kAllocSlots);
            const unsigned long long need = (unsigned long long)r0.chunk * kChunkSamples + (unsigned long long)max(last, 0ll);
            if (tid == 0) {
                uint32_t polls = 0;
                while (__hip_atomic_load(p.src_ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < need) {
                    if (++polls > 40000u) {   // tens of milliseconds
                        atomicOr(&p.ctr->overflow, 32u);
                        break;
                    }
                    __builtin_amdgcn_s_sleep(8);
                }
            }
            __syncthreads();
        }
    }
    // A tile read in place from host memory keeps kTrickle of its eight loads in flight, not all of them: every
    // request waits its turn in the same L2 queues as everything else on the device, and four passes side by
    // side with 512 KB each outstanding put ~36 us of link time in front of any other miss -- the tables of a
    // pass that is just starting, the address bits and list entries of one that is matching (seen: 17 us for
    // the tables instead of 2).  Two loads per thread in flight already fill the link (tools/pcie_read_probe.hip); three measured best.
    bool trickle = false;
    if constexpr (FUSED && !FROM_MAG) trickle = p.src_host != 0u && p.carry == nullptr;
    if (t_first < t_end) {
        if (trickle) {
#pragma unroll
            for (int i = 0; i < kTrickle; i++) load_tile_iq_one<U8>(p, tile_ref<FROM_MAG>(p, t_first), tid, pre, i);
        } else {
            load_tile_iq<FROM_MAG, U8>(p, tile_ref<FROM_MAG>(p, t_first), tid, pre);
        }
    }

    // Workgroups that share a CU start a fraction of a tile period apart, so that the
    // VALU-dense phases of one overlap the latency-bound phases of the others instead of
    // all of them marching through the same phase together.
#ifdef ADSB_TUNING
    if (p.stagger_ticks) {
        const uint32_t k = (blockIdx.x * 4u) / gridDim.x;  // 0..3: which quarter of the grid
        const unsigned long long until = clock64() + (unsigned long long)k * p.stagger_ticks;
        while ((unsigned long long)clock64() < until) __builtin_amdgcn_s_sleep(8);
    }
#endif

#ifdef ADSB_KERNEL_ACCT
    const bool acct = ADSB_STOP_AT(p, 100) && p.timeline != nullptr;
    unsigned long long acc_t[8] = {0, 0, 0, 0, 0, 0, 0, 0}, acc_last = acct ? clock64() : 0;
#endif

    const bool late_prio = ADSB_PRIO_LATE != 0 && (ADSB_PRIO_LATE_DENSE != 0 || p.order_cnt == nullptr);
    FSTAMP(1);
    uint32_t iter = 0;
    for (uint32_t t = t_first; t < t_end; t += t_stride, iter++) {
    const TileRef cur = tile_ref<FROM_MAG>(p, t);
    STAMP(0);
    const uint32_t chunk = cur.chunk;
    const int len = cur.len, jbase = cur.jbase;
    const int jn = min(kTile, len - jbase);  // <= 0 for tiles past the end of a short chunk

    const uint32_t par = iter & 1u;  // which copy of the tile counters this tile uses

    // ---------------------------------------------------------------- P1 magnitudes
    if constexpr (U8) {
        // (the tile's first and last loads decide, once per tile, whether any sample needs its position checked:
        // all but the first and last tiles of a buffer take the loop without the checks)
        const int shift = p.carry != nullptr && (chunk > 0 || p.lead_from_src) ? kCarrySamples : 0;
        const int k_first = jbase - kPad - kLead + shift;
        if (k_first >= 0 && k_first + 4 * kThreads * kLoadsPerThread <= len + shift)
            p1_u8<true, FUSED>(p, s, cur, tid, pre, trickle);
        else
            p1_u8<false, FUSED>(p, s, cur, tid, pre, trickle);
    } else {
#pragma unroll
    for (int i = 0; i < kLoadsPerThread; i++) {
        if constexpr (FUSED && !FROM_MAG) {
            if (trickle && i + kTrickle < kLoadsPerThread) {   // load i has arrived: the next one may go
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kTrickle - 1) : "memory");
                load_tile_iq_one(p, cur, tid, pre, i + kTrickle);
            }
        }
        const int g = tid + i * kThreads;
        if (g < kAllocSlots / 4) *(uint2 *)(s.mag + 4 * g) = FROM_MAG ? make_uint2(pre[i].x, pre[i].y) : mag4_of(pre[i]);
    }
    }
    if (t + t_stride < t_end) load_tile_iq<FROM_MAG, U8>(p, tile_ref<FROM_MAG>(p, t + t_stride), tid, pre);
    ACCT(0);
    if constexpr (FUSED) {
        // (bitmap_wait) behind an icao_flush the first workgroup clears the pass's bitmap: it has, by the time this
        // workgroup's first tile has arrived -- one look, bounded like the other waits of a one-launch pass (a first
        // workgroup that has not been given a CU yet: the pass is reported as overflowed and redone)
        if (p.bitmap_fresh && iter == 0 && blockIdx.x != 0 && tid == 0) {
            uint32_t polls = 0;
            while (ld_shared<true>(&p.ctr->bitmap_ready) == 0u) {
                if (++polls > 20000u) {
                    atomicOr(&p.ctr->overflow, 64u);
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
        }
    }
    lds_barrier();
    // every thread is past the previous tile's epilogue: its counters can be zeroed for the next
    // tile (this tile counts in the other copy), so the tile needs no barrier at its end
    if (tid == 0) s.nhit[par ^ 1u] = 0;
    ACCT(1);
    STAMP(1);
    if (jn <= 0 || ADSB_STOP_AT(p, 1)) {
        lds_barrier();
        continue;
    }

    // ---------------------------------------------------------------- P2 sign planes
    // item = (g, kw): residues 4g..4g+3, plane bits k = 8kw..8kw+7, i.e. samples
    // 12k + 4g + {0..3} (+3 of look-ahead).  Bit k of plane (kind, r) is the sign taken
    // at sample 12k + r.  Walking k downwards leaves bit (k & 7) of the byte = k.
    for (int item = tid; item < kItems2; item += kThreads) {
        constexpr int R = kResPerItem, G = 12 / R;
        const int g = item % G, kw = item / G;
        const uint16_t *base = s.mag + 96 * kw + R * g;  // 4-byte aligned (R even)
        uint32_t acc[6][R];
#pragma unroll
        for (int q = 0; q < 6; q++)
#pragma unroll
            for (int r = 0; r < R; r++) acc[q][r] = 0;
#pragma unroll
        for (int kk = 8; kk >= 0; --kk) {
            // m[0 .. R+2]: the R samples of this lane and three of look-ahead.  Explicit
            // 8-byte reads (the address is 8-byte aligned, no more): left to itself the
            // compiler merges dword reads into one 16-byte read, and an LDS access off its
            // natural alignment is replayed at 64 cycles (SQ_LDS_UNALIGNED_STALL).
            int m[R + 4];
            if constexpr (R == 4) {
                const uint2 lo = *(const uint2 *)(base + 12 * kk);
                const uint2 hi = *(const uint2 *)(base + 12 * kk + 4);
                m[0] = (int)(lo.x & 0xFFFFu);
                m[1] = (int)(lo.x >> 16);
                m[2] = (int)(lo.y & 0xFFFFu);
                m[3] = (int)(lo.y >> 16);
                m[4] = (int)(hi.x & 0xFFFFu);
                m[5] = (int)(hi.x >> 16);
                m[6] = (int)(hi.y & 0xFFFFu);
                m[7] = (int)(hi.y >> 16);
            } else {  // R == 2: 4-byte aligned, three separate dword reads
                typedef const volatile __attribute__((address_space(3))) uint32_t *lds_u32_ptr;
                lds_u32_ptr src = (lds_u32_ptr)(base + 12 * kk);
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const uint32_t w = src[d];
                    m[2 * d] = (int)(w & 0xFFFFu);
                    m[2 * d + 1] = (int)(w >> 16);
                }
            }
            int e[R + 2];  // first differences m[s+1] - m[s]
#pragma unroll
            for (int i = 0; i < R + 2; i++) e[i] = m[i + 1] - m[i];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int ea = e[r], eb = e[r + 1], ec = e[r + 2];
                if (kk < 8) {
                    // slicer value D(ph) at this sample (demod_2400.rs:72-83), negated so that
                    // "D > 0" is the sign bit: with a = m0-m1 = -e0, b = m1-m2 = -e1, c = m2-m3:
                    //   D0 = 5a+2b  D1 = 4a+3b  D2 = 3a+4b  D3 = 2a+5b  D4 = a+6b+c
                    const int n0 = __mul24(ea, 5) + (eb + eb);
                    const int u = eb - ea;
                    const int n1 = n0 + u, n2 = n1 + u, n3 = n2 + u;
                    const int n4 = n3 + u + ec;  // a + 6b + c = (2a + 5b) + (b - a) + c: one add3
                    acc[0][r] = push_sign(acc[0][r], n0);
                    acc[1][r] = push_sign(acc[1][r], n1);
                    acc[2][r] = push_sign(acc[2][r], n2);
                    acc[3][r] = push_sign(acc[3][r], n3);
                    acc[4][r] = push_sign(acc[4][r], n4);
                }
                // kk == 8 is one plane bit beyond the byte, for GT only: it completes the "advanced
                // by one bit" copies that P3 addresses as residues 12..23.  There is no "<" plane:
                // P3 works with "<=" (the complement of ">") and the gates re-check strictness.
                acc[5][r] = push_sign(acc[5][r], ea);   // GT: m[s] > m[s+1]
            }
        }
        uint8_t *pb = (uint8_t *)s.plane;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int res = R * g + r;
#pragma unroll
            for (int q = 0; q < 5; q++) pb[(q * 12 + res) * (kPlaneDw * 4) + kw] = (uint8_t)acc[q][r];
            // 9 bits: k = 8kw .. 8kw+8.  Residue res holds bits 0..7, residue res+12 (the
            // same plane advanced one bit) holds bits 1..8.
            pb[(kPlaneGT + res) * (kPlaneDw * 4) + kw] = (uint8_t)acc[5][r];
            pb[(kPlaneGT + 12 + res) * (kPlaneDw * 4) + kw] = (uint8_t)(acc[5][r] >> 1);
        }
    }
    ACCT(2);
    lds_barrier();
    ACCT(3);
    STAMP(2);
    if (ADSB_STOP_AT(p, 2)) continue;
    // The wave-private stages are chains of LDS round trips with few instructions between them:
    // at a raised issue priority they get through their dependent steps without queueing behind the
    // other workgroups' P1 / P2 on the same SIMD, which have instructions to spare for every slot
    // those chains leave (measured: pipelined -2 %, a launch on its own 105 -> 100 us; levels 1, 2
    // and 3 alike).  Not on dense streams: there the tail kernels beside the scan are the ones that
    // must not wait (adsb_aux.hip: TAIL_PRIO), and the step got 3 % longer.
    if (late_prio) __builtin_amdgcn_s_setprio(ADSB_PRIO_LATE);

    // ================================================================ P3..P5, wave-private
    // From here to the end of the tile every wave works alone on the positions of its own
    // P3 items: matches, candidates and trials stay in the wave's own LDS regions, so there
    // is no workgroup barrier and no shared counter between the stages, the waves of a
    // workgroup drift apart, and their latency-bound stages overlap the VALU-dense ones of
    // the others.  Nothing here can overflow: a wave with more matches than its region
    // holds takes them in rounds of a few plane bits, and candidates are flushed through
    // the trial stage whenever their region fills.
    {
    const int wave = tid >> 6;
    uint16_t *const wpat = s.pat + wave * kPatPerWave;
    uint16_t *const wcand = s.cand + wave * kCandPerWave;

    // ---------------------------------------------------------------- P3 preamble patterns
    // item = (res, w): the 32 positions with slot = 12*(32w + bit) + res.
    // (with 512 threads an item is half a dword, so that all eight waves own positions)
    constexpr int kHalves = kThreads / 256;
    uint32_t b[5] = {0u, 0u, 0u, 0u, 0u};
    const int ptid = tid % 256, phalf = tid / 256;
    const int pres = ptid % 12, pw = ptid / 12;
    if (ptid < kItems3) {
        const int res = pres, w = pw;
        const uint32_t *GT = s.plane + (kPlaneGT + res) * kPlaneDw + w;
#define GTO(o) GT[(o) * kPlaneDw]     // p[o] > p[o+1]
#define LTO(o) (~GT[(o) * kPlaneDw])  // p[o] <= p[o+1]: a superset of the reference's "<"; the
                                      // gates test the strict form of the branch they are handed
        // positions that are real j of this tile: kPad <= slot < kPad + jn
        // (x + 11) / 12 with a 24-bit multiply (x < 16384), not the 32-bit mul_hi the compiler would use
        const int kmin = (int)(__umul24((uint32_t)(kPad - res + 11), 10923u) >> 17),
                  kmax = (int)(__umul24((uint32_t)(kPad + jn - res + 11), 10923u) >> 17);
        uint32_t ok = lowmask(kmax - 32 * w) & ~lowmask(kmin - 32 * w);
        if (kHalves == 2) ok &= phalf ? 0xFFFF0000u : 0x0000FFFFu;
        ok &= LTO(0) & GTO(12);                               // demod_2400.rs:221
        const uint32_t A = GTO(1) & LTO(2);                   // p1>p2 p2<p3
        const uint32_t C = LTO(8) & GTO(9);                   // p8<p9 p9>p10
        const uint32_t E = GTO(4) & LTO(9) & GTO(10) & LTO(11);
        const uint32_t b1 = ok & A & GTO(3) & C & LTO(10);                    // :227
        const uint32_t b2 = ok & A & GTO(3) & C & LTO(11) & ~b1;              // :242
        const uint32_t b3 = ok & A & GTO(4) & LTO(8) & GTO(10) & LTO(11) & ~(b1 | b2);  // :262
        const uint32_t b4 = ok & GTO(1) & LTO(3) & E & ~(b1 | b2 | b3);       // :280
        const uint32_t b5 = ok & GTO(2) & LTO(3) & E & ~(b1 | b2 | b3 | b4);  // :300
#undef LTO
#undef GTO
        b[0] = b1;
        b[1] = b2;
        b[2] = b3;
        b[3] = b4;
        b[4] = b5;
    }
    const uint32_t slot0 = (uint32_t)(12 * 32 * pw + pres);
    const uint32_t any_all = b[0] | b[1] | b[2] | b[3] | b[4];
    // which branch matched, as three planes of a 3-bit code (0..4), so that compaction is one
    // loop over the union instead of one per branch
    const uint32_t code0 = b[1] | b[3], code1 = b[2] | b[3], code2 = b[4];
    const uint32_t cnt_all = (uint32_t)__popc(any_all);
    const uint32_t incl_all = wave_inclusive_scan(cnt_all);
    const uint32_t total_all = (uint32_t)__builtin_amdgcn_readlane((int)incl_all, 63);
    // all matches in one round when they fit the wave's region (the normal case: ~90 of
    // 256), else rounds of kRoundBits plane bits: at most 64 lanes x kRoundBits matches each
    const int nrounds = total_all <= (uint32_t)kPatPerWave ? 1 : 32 / kRoundBits;
    uint32_t ncand_w = 0;  // candidates waiting in wcand (wave-uniform)
    if (ADSB_STOP_AT(p, 3)) goto tile_end;  // profiling: patterns only

    // One loop, one copy of each stage: take the next round of matches when the previous one
    // is used up, run one 64-lane pass of the gates, and run the trials whenever the
    // candidate region could not take another pass's worth (or nothing else is left).
    int round = 0;
    uint32_t npat_w = 0, base = 0;
    bool in_round = false;
    for (;;) {
        if (round < nrounds) {
            if (!in_round) {
                // ---- compaction of this round's matches into wpat: exclusive scan of the lane
                // counts (DPP, no LDS traffic), then every lane writes its own
                const uint32_t rmask = nrounds == 1 ? 0xFFFFFFFFu
                                                    : (((1u << kRoundBits) - 1u) << (round * kRoundBits));
                uint32_t cnt = cnt_all, incl = incl_all;
                npat_w = total_all;
                if (nrounds != 1) {
                    cnt = (uint32_t)__popc(any_all & rmask);
                    incl = wave_inclusive_scan(cnt);
                    npat_w = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                }
                if (npat_w == 0) {
                    round++;
                    continue;
                }
                compact_matches(any_all & rmask, code0, code1, code2, slot0, wpat, incl - cnt);
                wave_lds_fence();
                in_round = true;
                base = 0;
                if (ADSB_STOP_AT(p, 6)) {  // profiling: patterns + compaction, no gates
                    in_round = false;
                    round++;
                    continue;
                }
            }

            // ------------------------------------------------------------ P4 value gates
            // one lane per pattern match (gate_pass)
            {
                const uint32_t idx = base + (uint32_t)lane;
                gate_pass<SELFTEST>(p, s, wpat[min(idx, npat_w - 1u)], idx < npat_w, wcand, ncand_w, jbase, chunk);
            }
            base += 64;
            if (base >= npat_w) {
                in_round = false;
                round++;
            }
            // room for another pass of the gates and more of them to come: not yet
            if (round < nrounds && ncand_w + 64 <= (uint32_t)kCandPerWave) continue;
        }
        if (ncand_w == 0) {
            if (round >= nrounds) break;
            continue;
        }
        wave_lds_fence();
        if (ADSB_STOP_AT(p, 4)) {  // profiling: gates only
            ncand_w = 0;
            if (round >= nrounds) break;
            continue;
        }

        // ---------------------------------------------------------------- P5 trials
        // lane = (candidate, try_phase) (trial_pass)
        {
            const uint32_t ntrial = ncand_w * 5u;
            cand_count += ncand_w;
            ncand_w = 0;
            for (uint32_t tb = 0; tb < ntrial; tb += 64) {
                const uint32_t t5 = tb + (uint32_t)lane;
                uint32_t c, tpi;
                split5(min(t5, ntrial - 1u), c, tpi);
                trial_pass<FUSED, FIELDS, FIX, FIX2>(p, s, hf, cand_entry(wcand[c]), tpi, t5 < ntrial, jbase, chunk, seg, seg_cap,
                                                     ap_count, lane, par, fixt, fix_mult, fix2, fix2_m0, fix2_m1);
            }
            wave_lds_fence();  // wcand is reused by the next passes of the gates
        }
        if (round >= nrounds) break;
    }
    }
tile_end:
    if (late_prio) __builtin_amdgcn_s_setprio(0);
    ACCT(4);
    lds_barrier();
    ACCT(5);
    STAMP(5);
    if (ADSB_STOP_AT(p, 5)) {
        lds_barrier();
        continue;
    }

    // ---------------------------------------------------------------- tile epilogue
    // (the AP fill counts are registers; they are written back when the workgroup retires)
    const uint32_t nhit = min(s.nhit[par], (uint32_t)kHitCap);
    if constexpr (FUSED && FIELDS) {
        // one-launch pass: the staged hits' records are built here and now, a wave a hit (emit_record); only what
        // did not fit the staging went to the hit list (stage_hit), for the record builder at the end
        const uint32_t nstaged = min(s.nhit[par], (uint32_t)(kHitCap + kFusedExtraHits));
        for (uint32_t i = (uint32_t)(tid >> 6); i < nstaged; i += (uint32_t)kWaves) {
            const bool extra = i >= (uint32_t)kHitCap;   // (wave-uniform)
            const uint64_t me = extra ? hf.xhit[i - kHitCap] : s.hit[i];
            uint32_t ff[5];
#pragma unroll
            for (int r = 0; r < 5; r++) ff[r] = extra ? hf.xf[i - kHitCap][r] : hf.f[i][r];
            emit_record(p, s, ff, (uint32_t)((int)entry_j(me) - (jbase - kPad)), me, entry_value(me), lane);
        }
    } else
    if (nhit) {  // sparse streams: a handful per buffer; dense ones: most tiles
        // Dense stream: the hits of a tile go into the tile's own part of its buffer's bucket.  This workgroup is that
        // part's only writer during the scan, so unless the staging overflowed (more than kHitCap hits in one tile:
        // the rest went in one by one, stage_hit) they take places 0 .. nhit - 1 and the count is a plain store:
        // nothing to wait for, no barrier.  Sparse stream (one flat list): a place from the list's counter.
        const bool dense = p.order_cnt != nullptr;
        const uint32_t tile_g = chunk * (uint32_t)kTilesPerChunk + (uint32_t)cur.tile;
        const bool alone = dense && s.nhit[par] <= (uint32_t)kHitCap;   // (uniform)
        uint64_t *const dst = dense ? p.order_tmp + (size_t)chunk * kOrderBucket + (size_t)cur.tile * kTileBucket : p.hits;
        const uint32_t dst_cap = dense ? kTileBucket : p.hits_cap;
        uint32_t hit_base = 0;
        if (alone) {
            if (tid == 0) {
                atomicAdd(&p.ctr->n_hits, nhit);   // (no value taken: fire and forget)
                p.order_cnt[tile_g] = nhit;
            }
        } else {
            if (tid == 0) {
                const uint32_t at = atomicAdd(&p.ctr->n_hits, nhit);
                s.hit_base = dense ? atomicAdd(&p.order_cnt[tile_g], nhit) : at;
            }
            lds_barrier();
            hit_base = s.hit_base;
        }
        if (hit_base + nhit > dst_cap) {
            if (tid == 0) atomicOr(&p.ctr->overflow, 1u);
        } else {
            for (uint32_t i = tid; i < nhit; i += kThreads) {
                st_shared<FUSED>(&dst[hit_base + i], s.hit[i]);
                if constexpr (FIELDS)
                    put_hit_fields<FUSED>(p, (size_t)(dst - (dense ? p.order_tmp : p.hits)) + hit_base + i, hf.f[i]);
            }
        }
    }
    ACCT(6);
    STAMP(6);
    }  // tile loop
#ifdef ADSB_KERNEL_ACCT
    if (acct && lane == 0)
        for (int k = 0; k < 8; k++) p.timeline[((size_t)blockIdx.x * kWaves + (tid >> 6)) * 8 + k] = acc_t[k];
#endif
    // candidate counts were kept per wave (diagnostic): lane 0 of each wave adds its own
    if (lane == 0 && cand_count) atomicAdd(&p.ctr->seg_cand[blockIdx.x], cand_count);
    if (lane == 0) {
        if (ap_count > seg_cap) atomicOr(&p.ctr->overflow, 2u);
        st_shared<FUSED>(&p.ctr->seg_ap[my_seg], min(ap_count, seg_cap));
    }
    if constexpr (FUSED) {
        // ============================================================ the tail of a one-launch pass
        // (a) Publish this tile -- its address bits, list entries and counts -- and wait, for a bounded time,
        // until every tile BEFORE it in the buffer order has done the same: a trial must see what earlier
        // positions taught the filter (src/mode_s/mod.rs:71,115,130 read what :83,99 wrote), and workgroups
        // finish in any order.  Workgroups only ever wait for tiles in front of them and publish before they
        // wait, so the chain cannot close on itself; the wait is bounded anyway (a workgroup in front may
        // not have been given a CU yet): whoever gives up says so, and then the last workgroup looks at
        // every list once more (c).
        FSTAMP(2);
        static_assert(kFusedMaxTiles >= 16 * kTilesPerChunk, "tile flags of the largest one-launch pass");
        // (release: everything this workgroup wrote for others went through to the memory side -- st_shared,
        // atomics -- and is acknowledged from there; no cache write-back: adsb_tail_dev.h, st_shared)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(&p.ctr->tile_done[blockIdx.x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid < 64) {
            bool ordered = true;
            for (uint32_t spins = 0;; spins++) {
                bool all = true;
                for (uint32_t k = (uint32_t)lane; k < blockIdx.x; k += 64u)
                    all = all && __hip_atomic_load(&p.ctr->tile_done[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
                if (__all(all)) break;
                if (spins >= p.order_polls) {  // 200: ~0.2 ms
                    ordered = false;
                    break;
                }
                __builtin_amdgcn_s_sleep(4);
            }
            if (lane == 0 && !ordered) atomicOr(&p.ctr->unordered, 1u);
        }
        __syncthreads();
        // Each wave matches its own address/parity entries against the bitmap as it stands now: it holds
        // every address of the passes before this one (stream order; the host redoes a pass whose
        // predecessor on another scan stream turns out to have learned one: adsb_collect.cpp), what the
        // tiles before this one learned, and whatever else this pass has learned so far (harmless: the host
        // replay scores in order).
        {
            // (a match's record is built here and now: this workgroup's tile is still in LDS -- emit_records)
            const uint32_t n_mine = min(ap_count, seg_cap);
            const int slot0 = tile_ref<FROM_MAG>(p, blockIdx.x).jbase - kPad;   // data index of LDS slot 0 (one tile per workgroup)
            for (uint32_t i0 = 0; i0 < n_mine; i0 += 64u) {
                const uint32_t i = i0 + (uint32_t)lane;
                const uint64_t e = i < n_mine ? ld_shared<true>(&seg[i]) : (15ull << 24);
                const uint32_t code = entry_code(e);
                uint32_t c = entry_value(e);
                if (code >= 5u && code < 10u) c = gf_apply(fs.x56, c);
                // (agent scope: bits other workgroups of this launch have set, not a line this CU's cache holds)
                const uint32_t at = bitmap_index(c, p.bitmap_lg);
                const bool hit = code != 15u && ((ld_shared<true>(&p.bitmap[at >> 5]) >> (at & 31u)) & 1u) != 0u;
                const unsigned long long mm = __ballot(hit);
                if (mm) {
                    const uint32_t cs = hit ? (uint32_t)((int)entry_j(e) - slot0) : (uint32_t)kPad;
                    Trial tr;
                    trial_eval(s, cand_entry(cs), code % 5u, tr);
                    emit_records(p, s, mm, tr.f, cs, e, c, lane);
                    if (hit) st_shared<true>(&seg[i], e | (15ull << 24));   // the second look must not report it again
                }
            }
        }
        // (b) The last workgroup to get here runs the rest alone: release what the match wrote (hits, marks;
        // usually nothing -- the tile itself was published above), count this workgroup in, acquire what
        // the others wrote.
        FSTAMP(3);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // what the match wrote (hits, marks) has arrived
        __syncthreads();
        if (tid == 0) fs.is_last = atomicAdd(&p.ctr->scan_blocks_done, 1u) == gridDim.x - 1u ? 1u : 0u;
        __syncthreads();
        if (!fs.is_last) return;
        // (acquire: nothing -- from here on what the other workgroups wrote is read with ld_shared)
        FSTAMP(4);
        // (c) The fallback: some workgroup matched without having seen all the tiles before it, and an
        // address bit that was clear when the pass began was set on the way -- its entries may have missed
        // it.  Once more over every segment, marked entries skipped.
        const uint32_t n_new = __hip_atomic_load(&p.ctr->learned_new, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_new && __hip_atomic_load(&p.ctr->unordered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            const uint32_t nseg = gridDim.x * (uint32_t)kWaves;
            // every segment's fill count into LDS first (one round trip for all of them), then each wave
            // takes its segments nine at a time, their entries in flight together; with a handful of new
            // addresses an entry is compared with those directly (no trip to the bitmap)
            uint32_t *const cnt = s.plane;
            static_assert(sizeof(s.plane) / 4 >= 4 * 16 * kTilesPerChunk, "fill counts of the largest one-launch pass");
            for (uint32_t g = (uint32_t)tid; g < nseg; g += kThreads) cnt[g] = min(ld_shared<true>(&p.ctr->seg_ap[g]), seg_cap);
            uint32_t fresh[kNewAddrCap];
            const bool by_list = n_new <= (uint32_t)kNewAddrCap;
#pragma unroll
            for (int k = 0; k < kNewAddrCap; k++)
                fresh[k] = by_list && (uint32_t)k < n_new ? ld_shared<true>(&p.ctr->new_addr[k]) : 0xFFFFFFFFu;
            lds_barrier();
            FSTAMP(8);
            constexpr uint32_t U = 9;
            for (uint32_t g0 = (uint32_t)(tid >> 6) * U; g0 < nseg; g0 += kWaves * U) {
                uint32_t n[U], nmax = 0;
#pragma unroll
                for (uint32_t u = 0; u < U; u++) {
                    n[u] = g0 + u < nseg ? cnt[g0 + u] : 0u;
                    nmax = max(nmax, n[u]);
                }
                for (uint32_t i = (uint32_t)lane; i < nmax; i += 64u) {
                    uint64_t e[U];
#pragma unroll
                    for (uint32_t u = 0; u < U; u++) e[u] = i < n[u] ? ld_shared<true>(&p.ap[(uint64_t)(g0 + u) * seg_cap + i]) : (15ull << 24);
#pragma unroll
                    for (uint32_t u = 0; u < U; u++) {
                        if (!by_list) {
                            fused_match_entry(p, fs.x56, &p.ap[(uint64_t)(g0 + u) * seg_cap + i], e[u]);
                            continue;
                        }
                        const uint32_t code = entry_code(e[u]);
                        uint32_t c = entry_value(e[u]);
                        if (code >= 5u && code < 10u) c = gf_apply(fs.x56, c);
                        bool hit = false;
#pragma unroll
                        for (int k = 0; k < kNewAddrCap; k++) hit = hit || c == fresh[k];
                        if (hit && code != 15u) {
                            const uint32_t idx = atomicAdd(&p.ctr->n_hits, 1u);
                            if (idx < p.hits_cap) {
                                st_shared<true>(&p.hits[idx], e[u]);
                                if (p.hit_fields) st_shared<true>(&p.hit_fields[(size_t)idx * kHitFieldWords + 5], 0u);
                            } else {
                                atomicOr(&p.ctr->overflow, 1u);
                            }
                        }
                    }
                }
            }
            FSTAMP(7);
            // (this workgroup's own appends: written through, and read past this CU's cache by the record
            // builder -- no cache write-back needed, only their completion)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        FSTAMP(5);
        // (d) records, checksum, summary into mapped host memory; the counters back to zero
        // (the records built in place are there already; what is left is what the second look found, if it ran)
        records_block<FROM_MAG, false, true, U8>(p, p.fused_rec, 0u, 1u, nullptr, false, gridDim.x, fs.bits);
        FSTAMP(6);
    }

