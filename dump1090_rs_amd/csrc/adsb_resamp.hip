// adsb_resamp.hip -- k_resamp: the exact-integer rational resampler in front of the scan (include/adsb_hip.h,
// "Resampling"), and k_resamp_history, which hands the filter's history on to the next call.
//
//   p = (n M) mod L,  q = floor(n M / L),  y[n] = clamp((sum_j h[p + j L] x[q - j] + r) >> s), re and im separately.
//
// A memory-bound pass: (8, 4 or 2) M / L bytes read and 4 written per output.  The phase p differs from output to output,
// but outputs n and n + L share it and their inputs lie exactly M apart.  A workgroup of 256 lanes takes a tile of L R
// consecutive outputs as L CLASSES of R outputs each (output i of the tile: class i mod L, member i div L), and a wave
// works on 64 members of one class at a time:
//   * within a class the phase, hence the sub-filter h[p + j L], is wave-uniform: the taps lie in device memory in
//     polyphase order, each phase padded with zeros to a multiple of eight, and are read eight at a time by scalar loads;
//   * member r's tap j is input q_c + r M - j: k_decim's access pattern with D = M.  The tile's R M + K inputs go to LDS
//     in POLYPHASE order by M -- local sample l at [l mod M][l div M], rows of `row_len` (odd) dwords -- so every tap is
//     a unit-stride read;
//   * re and im stay packed in their dword: one v_dot2_i32_i16 per half, against {h, 0} and {0, h};
//   * a class's outputs are L apart in memory: the tile's outputs are staged in LDS and leave in 16-byte stores;
//   * the inputs come in with back-to-back 16-byte buffer loads from the 32-byte boundary below (the first input the tile
//     needs) - 8, through a resource that spans [max(that, 0), n_in) of the call's input: the hardware range check returns
//     zero for whatever lies in front of the call or past its end.  Inputs in front of the call come from the history
//     buffer instead (the first K - 1 inputs of the first tiles); 8-bit input is widened as it is stored to LDS, through
//     a copy of the context's table in LDS, and masked by position: a sample in front of the stream is zero, not T8[0];
//   * FMT (include/adsb_hip.h, "Sample formats"; adsb_fmt_dev.h): as in k_decim, the format fixes the samples of a
//     16-byte load (4, 8, 2, 8 for CS16, 8-bit, CF32, REAL16) and the conversion to CS16 in front of the mixer;
//   * MIX (include/adsb_hip.h, "Frequency shift"): as in k_decim, a sample of the call is mixed with its table entry
//     between the widening and the store to LDS; the table comes through cached global loads (adsb_mix_dev.h), no LDS.
// The host hands over the call's first output already reduced (p0, q0): the kernel works in offsets that fit 32 bits
// beside one 64-bit tile base.  R (resamp_rows) depends on the ratio alone: the largest of 1024 .. 64 with L R <= 2048
// whose LDS, counted with K = 512, leaves room for eight workgroups per CU (20 KB) and whose L R / 64 units divide evenly
// among the four waves; failing that (a large M, whose inputs alone are more) the largest of 256, 128, 64 with
// L R <= 2048 that fits 64 KB; else the largest of 64, 32, 16, 8 that does, L R unbounded.  Over the ratios
// adsb_resamp_create accepts that third rule takes 5144 of 7223 (every L above 32) and only ever chooses 64 or 32 rows:
// a tile is then 2112 .. 8192 outputs, up to 32 KB of staged outputs and eight passes of the final store loop, and at 32
// rows (48 ratios, both terms near 128) half of every wave has no member.  Rows of 16 and 8 are listed and never chosen;
// tests/test_resamp_cpu.py enumerates this.  No scratch, no spills.
#include "../../include/adsb_hip.h"
#include "adsb_dev_common.h"
#include "adsb_fmt_dev.h"
#include "adsb_mix_dev.h"

namespace adsb {

namespace {

constexpr int kThreadsResamp = 256;
constexpr int kWavesResamp = kThreadsResamp / 64;

typedef uint32_t u32x4r __attribute__((ext_vector_type(4)));
typedef short s16x2r __attribute__((ext_vector_type(2)));
typedef int i32x4r __attribute__((ext_vector_type(4)));

// x / d for x < 2^15 and d <= 128, with recip = ceil(2^32 / d): x (recip d - 2^32) < 2^15 * 2^7 < 2^32.  (d = 1: its
// reciprocal does not fit 32 bits.)
__device__ __forceinline__ uint32_t resamp_div(uint32_t x, uint32_t d, uint32_t recip) { return d == 1 ? x : __umulhi(x, recip); }

__device__ __forceinline__ int dot_half_r(uint32_t sample, uint32_t tap_pair, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2r, sample), __builtin_bit_cast(s16x2r, tap_pair), acc, false);
}

__device__ __forceinline__ int round_clamp_r(int acc, uint32_t shift, int round)
{
    return min(max((acc + round) >> shift, -32768), 32767);
}

template <uint32_t FMT, bool MIX>
__global__ __launch_bounds__(kThreadsResamp) void k_resamp(ResampParams p)
{
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
}

// the last H = K - 1 inputs of the stream so far, widened: from the call's input, or from the previous history where
// the call was shorter than the history (k_decim_history's rule).  MIX: what comes from the call's input is mixed, what
// comes from the previous history is mixed already.
template <uint32_t FMT, bool MIX>
__global__ __launch_bounds__(512) void k_resamp_history(ResampParams p)
{
    constexpr bool U8 = FMT == kIn8Bit;
    const long long H = (long long)p.k_taps - 1, i = threadIdx.x, n = (long long)p.n_in;
    if (i >= H) return;
    const long long idx = n - H + i;
    uint32_t v;
    if (idx < 0) {
        v = p.hist_prev[i + n];
    } else {
        if constexpr (U8) {
            const uint8_t *s = (const uint8_t *)p.src;
            v = widen_u8_pair(p.u8_table, (uint32_t)s[2 * idx] | (uint32_t)s[2 * idx + 1] << 8);
        } else if constexpr (FMT == kInReal16) {
            v = ((const uint16_t *)p.src)[idx];
        } else if constexpr (FMT == kInCf32) {
            const uint2 f = ((const uint2 *)p.src)[idx];
            v = fmt_cf32(f.x, f.y, p.scale);
        } else {
            v = ((const uint32_t *)p.src)[idx];
        }
        if constexpr (MIX) v = mix_sample(v, p.mix.table[((unsigned long long)idx + p.mix.phase) % p.mix.period]);
    }
    p.hist_next[i] = v;
}

}  // namespace

uint32_t resamp_row_len(uint32_t down, uint32_t rows, uint32_t k_taps)
{
    return ((rows * down + k_taps + 15u + down - 1u) / down) | 1u;
}

uint32_t resamp_lds_words(uint32_t up, uint32_t down, uint32_t rows, uint32_t k_taps)
{
    // the polyphase store (rounded up to 16 bytes), the staged outputs, the 8-bit table
    return ((down * resamp_row_len(down, rows, k_taps) + 3u) & ~3u) + up * rows + 128u;
}

uint32_t resamp_rows(uint32_t up, uint32_t down)
{
    if (up < 1 || up > kResampMaxRatio || down < 1 || down > kResampMaxRatio) return 0;
    const auto words = [&](uint32_t r) { return resamp_lds_words(up, down, r, kResampMaxPhaseTaps); };
    const auto fits = [&](uint32_t r) { return words(r) <= kResampLdsWords; };
    // the largest tile of 2048 outputs at most that leaves room for eight workgroups per CU (20 KB each) and deals its
    // units of 64 outputs evenly to the four waves ...
    for (uint32_t r : {1024u, 512u, 256u, 128u, 64u})
        if (up * r <= 2048u && words(r) <= 5120u && (up * (r / 64u)) % 4u == 0) return r;
    // ... else (a large M: the tile's inputs alone are more) the largest that fits at all
    for (uint32_t r : {256u, 128u, 64u})
        if (up * r <= 2048u && fits(r)) return r;
    for (uint32_t r : {64u, 32u, 16u, 8u})
        if (fits(r)) return r;
    return 0;
}

int launch_resamp(const ResampParams &p, void *stream)
{
    if (p.up < 1 || p.up > kResampMaxRatio || p.down < 1 || p.down > kResampMaxRatio || p.k_taps < 1 ||
        p.k_taps > kResampMaxPhaseTaps || p.k_pad != ((p.k_taps + 7u) & ~7u) || p.shift > kResampMaxShift || p.p0 >= p.up ||
        p.q0 >= p.down || !p.rows || p.rows != resamp_rows(p.up, p.down) || p.row_len != resamp_row_len(p.down, p.rows, p.k_taps) ||
        p.recip_up != (uint32_t)(((1ull << 32) + p.up - 1u) / p.up) || p.recip_down != (uint32_t)(((1ull << 32) + p.down - 1u) / p.down) ||
        !p.src || !p.n_in || !p.hist_prev || !p.hist_next || !p.taps)
        return (int)hipErrorInvalidValue;
    if (!mix_params_ok(p.mix) || !in_format_ok(p.format, p.u8_table, p.scale)) return (int)hipErrorInvalidValue;
    const uint32_t lds_words = resamp_lds_words(p.up, p.down, p.rows, p.k_taps);
    if (lds_words > kResampLdsWords) return (int)hipErrorInvalidValue;
    // the call's first output has its newest input inside the call (then every tile's first output has)
    if (p.n_out && (!p.out || ((uintptr_t)p.out & 3u) || p.q0 >= p.n_in)) return (int)hipErrorInvalidValue;
    const uint64_t tile = (uint64_t)p.up * p.rows;
    const unsigned long long blocks = (p.n_out + tile - 1) / tile;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    // ... and so has its last: floor((p0 + (n_out - 1) M) / L) + q0 < n_in  (n_out < 2^31 tiles of 2^13 at most: 64 bits do)
    if (p.n_out && ((p.n_out - 1) * p.down + p.p0) / p.up + p.q0 >= p.n_in) return (int)hipErrorInvalidValue;
    const bool u8 = p.format == kIn8Bit, mix = p.mix.period != 0;
    if (blocks) {
        const size_t lds_bytes = (size_t)lds_words * 4u;
        const auto kernel = p.format == kInCf32    ? (mix ? k_resamp<kInCf32, true> : k_resamp<kInCf32, false>)
                            : p.format == kInReal16 ? (mix ? k_resamp<kInReal16, true> : k_resamp<kInReal16, false>)
                            : u8                    ? (mix ? k_resamp<kIn8Bit, true> : k_resamp<kIn8Bit, false>)
                                                    : (mix ? k_resamp<kInCs16, true> : k_resamp<kInCs16, false>);
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(kThreadsResamp), lds_bytes, (hipStream_t)stream, p);
        if (hipError_t e = hipGetLastError()) return (int)e;
    }
    if (p.k_taps > 1) {
        const auto kernel = p.format == kInCf32    ? (mix ? k_resamp_history<kInCf32, true> : k_resamp_history<kInCf32, false>)
                            : p.format == kInReal16 ? (mix ? k_resamp_history<kInReal16, true> : k_resamp_history<kInReal16, false>)
                            : u8                    ? (mix ? k_resamp_history<kIn8Bit, true> : k_resamp_history<kIn8Bit, false>)
                                                    : (mix ? k_resamp_history<kInCs16, true> : k_resamp_history<kInCs16, false>);
        hipLaunchKernelGGL(kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, p);
    }
    return (int)hipGetLastError();
}

}  // namespace adsb
