// adsb_resamp_body.inc -- one tile of the resampler: outputs [blockIdx.x L R, + L R) of the call `p` describes.  The body
// of k_resamp and of k_resamp_bank (adsb_resamp.hip, where the method is described), included into each: they differ only
// in where the call's own fields (src, n_in, out, n_out, p0, q0, the mixer's phase, the history) come from.  Expects FMT,
// MIX and a ResampParams `p` in scope.
    extern __shared__ uint32_t lds[];
    constexpr bool U8 = FMT == kIn8Bit;
    constexpr int kBps = (int)in_bytes_per_sample(FMT);
    constexpr int kPerLoad = 16 / kBps;    // samples per 16-byte load
    constexpr int kBatch = 4;              // loads in flight per lane
    const int tid = threadIdx.x;
    const uint32_t L = p.up, M = p.down, H = p.k_taps - 1, RL = p.row_len, R = p.rows;
    const uint32_t tile = L * R;
    uint32_t *stage = lds + ((M * RL + 3u) & ~3u);   // the tile's outputs, then (8-bit input) the table
    // input index (0 = the call's first sample) of the first input the tile needs, the origin of its local samples, and
    // how many of those there are: the tile's outputs reach from its first output's newest input - H to that + R M
    const long long i0 = (long long)p.q0 + (long long)blockIdx.x * (long long)(R * M) - (long long)H;
    const long long a0 = (i0 - 8) & ~7ll;
    const uint32_t e = (uint32_t)(i0 - a0);   // 8 .. 15
    const uint32_t ltot = R * M + 1u + H + e;
    const long long base = a0 > 0 ? a0 : 0;   // (< n_in: the tile has an output, whose newest input is i0 + H or behind)
    const unsigned long long left = (p.n_in - (unsigned long long)base) * kBps;
    const uint32_t bytes = (uint32_t)(left < (1ull << 30) ? ((left + 3) & ~3ull) : (1ull << 30));
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.src + base * kBps), 0, bytes, 0x00020000);
    const int rel = (int)(a0 - base);   // <= 0: in front of the call the offsets wrap to huge unsigned ones, out of range

    uint16_t *tab = (uint16_t *)(stage + tile);
    if constexpr (U8) {
        tab[tid] = p.u8_table[tid];
        __syncthreads();
    }
    // the table entry of local sample 0 (the tile's origin a0 = q0 + block R M - (H + e), reduced mod N)
    uint32_t t0 = 0;
    if constexpr (MIX) t0 = mix_tile_phase(p.mix.phase, p.q0, blockIdx.x, R * M, H + e, p.mix.period);
    for (uint32_t lb = 0; lb < ltot; lb += (uint32_t)(kBatch * kPerLoad * kThreadsResamp)) {
        u32x4r pre[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; i++) {
            const uint32_t l = lb + (uint32_t)(kPerLoad * (tid + i * kThreadsResamp));
            // (a load the tile does not need is sent out of range too: it returns zero and moves nothing.  Opaque: folded
            // into the instruction's immediate, a constant would be added without wrapping)
            int off = l < ltot ? (rel + (int)l) * kBps : -16;
            asm volatile("" : "+v"(off));
            pre[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < kBatch; i++) {
            const uint32_t l = lb + (uint32_t)(kPerLoad * (tid + i * kThreadsResamp));
            if (l >= ltot) continue;
            const uint32_t w[4] = {pre[i].x, pre[i].y, pre[i].z, pre[i].w};
            uint32_t v[kPerLoad];
#pragma unroll
            for (int c = 0; c < kPerLoad; c++) {
                const long long ii = a0 + (long long)l + c;   // the sample's index in the call
                if constexpr (U8) {
                    const uint32_t b2 = (w[c >> 1] >> (16 * (c & 1))) & 0xFFFFu;
                    v[c] = (ii >= 0 && ii < (long long)p.n_in) ? widen_u8_pair(tab, b2) : 0u;
                } else if constexpr (FMT == kInReal16) {   // (the load is rounded up to a dword: the int16 behind an odd end)
                    v[c] = (ii >= 0 && ii < (long long)p.n_in) ? fmt_halfword(w, c) : 0u;
                } else if constexpr (FMT == kInCf32) {     // (out of range the load gave +0.0, and q(0) = 0)
                    v[c] = fmt_cf32(w[2 * c], w[2 * c + 1], p.scale);
                } else {
                    v[c] = w[c];
                }
            }
            if constexpr (MIX) {   // (in front of the call and behind its end the samples are zero, and stay zero)
                uint32_t t = mix_mod(t0 + l, p.mix.period, p.mix.recip);
#pragma unroll
                for (int c = 0; c < kPerLoad; c++) {
                    v[c] = mix_sample(v[c], p.mix.table[t]);
                    if (++t == p.mix.period) t = 0;
                }
            }
            if (a0 + (long long)l < 0) {   // in front of the call: the history (the first tiles only)
#pragma unroll
                for (int c = 0; c < kPerLoad; c++) {
                    const long long ii = a0 + (long long)l + c;
                    if (ii < 0 && ii >= -(long long)H) v[c] = p.hist_prev[(long long)H + ii];
                }
            }
            uint32_t col = resamp_div(l, M, p.recip_down), row = l - col * M;
#pragma unroll
            for (int c = 0; c < kPerLoad; c++) {
                if (l + c < ltot) lds[row * RL + col] = v[c];
                if (++row == M) row = 0, col++;
            }
        }
    }
    __syncthreads();

    // unit u of the tile: class u mod L, members 64 (u div L) .. + 63; the waves take the units in turn
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6), lane = (uint32_t)tid & 63u;
    const uint32_t units = L * ((R + 63u) >> 6);
    const int round = p.shift ? 1 << (p.shift - 1) : 0;
    const uint32_t blocks = p.k_pad >> 3;
    // (the constant address space: scalar loads)
    typedef const i32x4r __attribute__((address_space(4))) *const_taps_ptr;
    for (uint32_t u = wave; u < units; u += kWavesResamp) {
        const uint32_t chunk = resamp_div(u, L, p.recip_up), c = u - chunk * L;
        // the class's phase, and its first member's newest input counted from the tile's
        const uint32_t x = p.p0 + c * M, qc = resamp_div(x, L, p.recip_up), phase = x - qc * L;
        const uint32_t r = chunk * 64u + lane, rr = min(r, R - 1u);   // (a lane without a member reads the last one's)
        // tap j of member r: local sample (e + H + qc - j) + r M
        const uint32_t l0 = e + H + qc, col0 = resamp_div(l0, M, p.recip_down);
        int ph = (int)(l0 - col0 * M);
        uint32_t addr = (uint32_t)ph * RL + col0 + rr;
        int acc_re = 0, acc_im = 0;
        const const_taps_ptr taps8 = (const_taps_ptr)(uintptr_t)(p.taps + (size_t)phase * p.k_pad);
        for (uint32_t kb = 0; kb < blocks; kb++) {
            const i32x4r ta = taps8[2 * kb], tb = taps8[2 * kb + 1];
            const int h[8] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z, tb.w};
#pragma unroll
            for (int t = 0; t < 8; t++) {
                const uint32_t s = lds[addr];
                const uint32_t hp = (uint32_t)h[t] & 0xFFFFu;
                acc_re = dot_half_r(s, hp, acc_re);
                acc_im = dot_half_r(s, hp << 16, acc_im);
                // one sample back: the row above, or from row 0 to the last row one column to the left
                if (--ph < 0) {
                    ph = (int)M - 1;
                    addr += (M - 1) * RL - 1;
                } else {
                    addr -= RL;
                }
            }
        }
        if (r < R) {
            const int re = round_clamp_r(acc_re, p.shift, round), im = round_clamp_r(acc_im, p.shift, round);
            stage[c + L * r] = ((uint32_t)re & 0xFFFFu) | ((uint32_t)im << 16);
        }
    }
    __syncthreads();

    const unsigned long long nb = (unsigned long long)blockIdx.x * tile;
    const unsigned long long rest = p.n_out - nb;   // (> 0: the grid has no tile without an output)
    const uint32_t cnt = rest < tile ? (uint32_t)rest : tile;
    uint32_t *out = p.out + nb;
    if (((uintptr_t)p.out & 15u) == 0) {   // (tile is a multiple of four: every tile's outputs start on 16 bytes)
        for (uint32_t i = 4u * (uint32_t)tid; i < cnt; i += 4u * kThreadsResamp) {
            if (i + 4u <= cnt) {
                *(u32x4r *)(out + i) = *(const u32x4r *)(stage + i);
            } else {
                for (uint32_t k = i; k < cnt; k++) out[k] = stage[k];
            }
        }
    } else {
        for (uint32_t i = (uint32_t)tid; i < cnt; i += kThreadsResamp) out[i] = stage[i];
    }
