// adsb_decim.hip -- k_decim: the integer polyphase FIR decimator in front of the scan (include/adsb_hip.h,
// "Decimation"), and k_decim_history, which hands the filter's history on to the next call.
//
//   y[n] = clamp((sum_k h[k] x[nD - k] + r) >> s), re and im separately, every step an exact integer.
//
// A memory-bound pass: (8, 4 or 2) D bytes read and 4 written per output.  A workgroup of 256 lanes takes a tile of
// kDecimTile = 256 outputs:
//   * it needs the tile D + T - 1 inputs from `i0` on; they are fetched with back-to-back 16-byte buffer loads
//     from the 32-byte boundary below i0 - 8, through a resource that spans [max(that, 0), n_in) of the call's input:
//     the hardware range check returns zero for whatever lies in front of the call or past its end.  Inputs in front
//     of the call come from the history buffer instead (the first T - 1 inputs of the first tiles);
//   * the inputs go to LDS in POLYPHASE order: local sample l sits at [l mod D][l div D], rows of `row_len` (odd)
//     dwords.  Lane j's tap k is local sample jD + q with q = e + T - 1 - k the same for the whole wave, so the
//     wave reads row q mod D from column q div D on -- unit stride, where sample order would be a stride of D dwords
//     (2-way bank conflicts at D = 2, 16-way at D = 16);
//   * the taps are wave-uniform: int32 in device memory, padded with zeros to a multiple of eight, read eight at a
//     time by scalar loads.  (The local origin sits at least eight samples in front of i0, so that the padded taps
//     multiply samples that exist.)
//   * re and im stay packed in their dword: one v_dot2_i32_i16 per half, against {h, 0} and {0, h};
//   * CU8 input is widened as it is stored to LDS, through a copy of the context's table in LDS, and masked by
//     position: a sample in front of the stream is zero, not T[0];
//   * FMT (include/adsb_hip.h, "Sample formats"; adsb_fmt_dev.h): the format fixes the bytes of a sample -- hence the
//     samples of a 16-byte load: 4 for CS16, 8 for 8-bit, 2 for CF32, 8 for REAL16 -- and the conversion to CS16 between
//     the load and the mixer: CF32 is q(x) = clamp(rint(x g)) per component, no table and nothing to mask (out of range
//     the load gives +0.0, and q(0) = 0); REAL16 is the halfword in the low half of the dword, masked by position as
//     8-bit is -- the load of an odd number of samples is rounded up to a dword;
//   * MIX (include/adsb_hip.h, "Frequency shift"): a sample is mixed with its table entry between the widening and the
//     store to LDS -- the samples of the call, not the history's, which holds mixed ones.  The workgroup reduces its
//     tile's origin mod N once, a load its first sample's phase by a multiplication, and the phase then steps with a wrap
//     per sample; the table comes through cached global loads (adsb_mix_dev.h) and takes no LDS.
// No scratch, no spills; LDS per workgroup: 4 (D row_len) bytes, row_len = ceil((256 D + T + 15) / D) | 1 -- 2.3 KB
// at D = 2 with 17 taps, 18.6 KB at D = 16 with 512 -- plus 512 bytes of table for CU8: eight workgroups (32 waves)
// fit a CU's LDS in every case.
#include "../../include/adsb_hip.h"
#include "adsb_dev_common.h"
#include "adsb_fmt_dev.h"
#include "adsb_mix_dev.h"

namespace adsb {

namespace {

constexpr int kThreadsDecim = 256;
static_assert(kThreadsDecim == (int)kDecimTile, "one output per lane");
// local samples a tile stores at most: tile D + T - 1 + 15 = 4622 < 8192 (decim_div's range)
constexpr uint32_t kDecimMaxLocal = kDecimTile * kDecimMaxFactor + kDecimMaxTaps - 1 + 15;
static_assert(kDecimMaxLocal < 8192, "decim_div");

typedef uint32_t u32x4d __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef int i32x4d __attribute__((ext_vector_type(4)));

// l / D for l < 8192 and D <= 16, with recip = ceil(2^20 / D): l (recip D - 2^20) < 8192 * 16 < 2^20
__device__ __forceinline__ uint32_t decim_div(uint32_t l, uint32_t recip) { return (l * recip) >> 20; }

__device__ __forceinline__ int dot_half(uint32_t sample, uint32_t tap_pair, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, sample), __builtin_bit_cast(s16x2, tap_pair), acc, false);
}

__device__ __forceinline__ int round_clamp(int acc, uint32_t shift, int round)
{
    return min(max((acc + round) >> shift, -32768), 32767);
}

template <uint32_t FMT, bool MIX>
__global__ __launch_bounds__(kThreadsDecim) void k_decim(DecimParams p)
{
    extern __shared__ uint32_t lds[];
    constexpr bool U8 = FMT == kIn8Bit;
    constexpr int kBps = (int)in_bytes_per_sample(FMT);
    constexpr int kPerLoad = 16 / kBps;                                                    // samples per 16-byte load
    // loads per lane: CS16 5, 8-bit and REAL16 3, CF32 10
    constexpr int kLoads = (kDecimMaxLocal + kPerLoad * kThreadsDecim - 1) / (kPerLoad * kThreadsDecim);
    const int tid = threadIdx.x;
    const uint32_t D = p.factor, H = p.n_taps - 1, RL = p.row_len, M = p.recip;
    // input index (0 = the call's first sample) of the first input the tile needs, the origin of its local samples,
    // and how many of those there are
    const long long i0 = (long long)p.first + (long long)blockIdx.x * (long long)(kDecimTile * D) - (long long)H;
    const long long a0 = (i0 - 8) & ~7ll;
    const uint32_t e = (uint32_t)(i0 - a0);   // 8 .. 15
    const uint32_t ltot = kDecimTile * D + H + e;
    const long long base = a0 > 0 ? a0 : 0;   // (< n_in: the tile has an output, whose input is behind i0 + H)
    const unsigned long long left = (p.n_in - (unsigned long long)base) * kBps;
    const uint32_t bytes = (uint32_t)(left < (1ull << 30) ? ((left + 3) & ~3ull) : (1ull << 30));
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.src + base * kBps), 0, bytes, 0x00020000);
    const int rel = (int)(a0 - base);   // <= 0: in front of the call the offsets wrap to huge unsigned ones, out of range

    u32x4d pre[kLoads];
#pragma unroll
    for (int i = 0; i < kLoads; i++) {
        const uint32_t l = (uint32_t)(kPerLoad * (tid + i * kThreadsDecim));
        // (a load the tile does not need is sent out of range too: it returns zero and moves nothing.  Opaque: folded
        // into the instruction's immediate, a constant would be added without wrapping)
        int off = l < ltot ? (rel + (int)l) * kBps : -16;
        asm volatile("" : "+v"(off));
        pre[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
    }
    uint16_t *tab = (uint16_t *)(lds + D * RL);
    if constexpr (U8) {
        tab[tid] = p.u8_table[tid];
        __syncthreads();
    }
    // the table entry of local sample 0 (the tile's origin a0 = first + block tile D - (H + e), reduced mod N)
    uint32_t t0 = 0;
    if constexpr (MIX) t0 = mix_tile_phase(p.mix.phase, p.first, blockIdx.x, kDecimTile * D, H + e, p.mix.period);
#pragma unroll
    for (int i = 0; i < kLoads; i++) {
        const uint32_t l = (uint32_t)(kPerLoad * (tid + i * kThreadsDecim));
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
#pragma unroll
        for (int c = 0; c < kPerLoad; c++) {
            const uint32_t lc = l + c;
            if (lc < ltot) {
                const uint32_t q = decim_div(lc, M);
                lds[(lc - q * D) * RL + q] = v[c];
            }
        }
    }
    __syncthreads();

    // tap k of lane j: local sample j D + (e + H - k)
    const uint32_t q0 = e + H, col0 = decim_div(q0, M);
    int ph = (int)(q0 - col0 * D);
    uint32_t addr = (uint32_t)ph * RL + col0 + (uint32_t)tid;
    int acc_re = 0, acc_im = 0;
    // (the constant address space: scalar loads)
    typedef const i32x4d __attribute__((address_space(4))) *const_taps_ptr;
    const const_taps_ptr taps8 = (const_taps_ptr)(uintptr_t)p.taps;
    const uint32_t blocks = (p.n_taps + 7u) >> 3;
    for (uint32_t kb = 0; kb < blocks; kb++) {
        const i32x4d ta = taps8[2 * kb], tb = taps8[2 * kb + 1];
        const int h[8] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z, tb.w};
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t x = lds[addr];
            const uint32_t hp = (uint32_t)h[u] & 0xFFFFu;
            acc_re = dot_half(x, hp, acc_re);
            acc_im = dot_half(x, hp << 16, acc_im);
            // one sample back: the row above, or from row 0 to the last row one column to the left
            if (--ph < 0) {
                ph = (int)D - 1;
                addr += (D - 1) * RL - 1;
            } else {
                addr -= RL;
            }
        }
    }
    const unsigned long long n = (unsigned long long)blockIdx.x * kDecimTile + (unsigned long long)tid;
    if (n < p.n_out) {
        const int round = p.shift ? 1 << (p.shift - 1) : 0;
        const int re = round_clamp(acc_re, p.shift, round), im = round_clamp(acc_im, p.shift, round);
        p.out[n] = ((uint32_t)re & 0xFFFFu) | ((uint32_t)im << 16);
    }
}

// the last H inputs of the stream so far, widened: from the call's input, or from the previous history where the
// call was shorter than the history (k_update_carry's rule).  MIX: what comes from the call's input is mixed, what
// comes from the previous history is mixed already.
template <uint32_t FMT, bool MIX>
__global__ __launch_bounds__(512) void k_decim_history(DecimParams p)
{
    constexpr bool U8 = FMT == kIn8Bit;
    const long long H = (long long)p.n_taps - 1, i = threadIdx.x, n = (long long)p.n_in;
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

// the mixer's table from the kernel's arguments: entry t = {c, s} -> {c, -s}, {s, c}
__global__ __launch_bounds__(256) void k_mix_store(MixTable t, uint32_t period, uint2 *table)
{
    const uint32_t i = threadIdx.x;
    if (i >= period) return;
    const uint32_t cs = t.cs[i], c = cs & 0xFFFFu, s = cs >> 16;
    table[i] = make_uint2(c | ((0u - s) << 16), s | (c << 16));
}

}  // namespace

uint32_t decim_row_len(uint32_t factor, uint32_t n_taps)
{
    return ((kDecimTile * factor + n_taps + 15u + factor - 1u) / factor) | 1u;
}

int launch_decim(const DecimParams &p, void *stream)
{
    if (p.factor < kDecimMinFactor || p.factor > kDecimMaxFactor || p.n_taps < 1 || p.n_taps > kDecimMaxTaps || p.shift > 16 ||
        p.first >= p.factor || p.row_len != decim_row_len(p.factor, p.n_taps) ||
        p.recip != ((1u << 20) + p.factor - 1u) / p.factor || !p.src || !p.n_in || !p.hist_prev || !p.hist_next || !p.taps)
        return (int)hipErrorInvalidValue;
    if (!in_format_ok(p.format, p.u8_table, p.scale)) return (int)hipErrorInvalidValue;
    if (!mix_params_ok(p.mix)) return (int)hipErrorInvalidValue;
    // every output of the call has its input inside it
    if (p.n_out && (!p.out || (unsigned long long)p.first + (p.n_out - 1) * (unsigned long long)p.factor >= p.n_in))
        return (int)hipErrorInvalidValue;
    const unsigned long long blocks = (p.n_out + kDecimTile - 1) / kDecimTile;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    const bool u8 = p.format == kIn8Bit, mix = p.mix.period != 0;
    if (blocks) {
        const size_t lds_bytes = ((size_t)p.factor * p.row_len + (u8 ? 128u : 0u)) * 4u;
        const auto kernel = p.format == kInCf32    ? (mix ? k_decim<kInCf32, true> : k_decim<kInCf32, false>)
                            : p.format == kInReal16 ? (mix ? k_decim<kInReal16, true> : k_decim<kInReal16, false>)
                            : u8                    ? (mix ? k_decim<kIn8Bit, true> : k_decim<kIn8Bit, false>)
                                                    : (mix ? k_decim<kInCs16, true> : k_decim<kInCs16, false>);
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(kThreadsDecim), lds_bytes, (hipStream_t)stream, p);
        if (hipError_t e = hipGetLastError()) return (int)e;
    }
    if (p.n_taps > 1) {
        const auto kernel = p.format == kInCf32    ? (mix ? k_decim_history<kInCf32, true> : k_decim_history<kInCf32, false>)
                            : p.format == kInReal16 ? (mix ? k_decim_history<kInReal16, true> : k_decim_history<kInReal16, false>)
                            : u8                    ? (mix ? k_decim_history<kIn8Bit, true> : k_decim_history<kIn8Bit, false>)
                                                    : (mix ? k_decim_history<kInCs16, true> : k_decim_history<kInCs16, false>);
        hipLaunchKernelGGL(kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, p);
    }
    return (int)hipGetLastError();
}

bool in_format_ok(uint32_t format, const uint16_t *u8_table, float scale)
{
    if (format >= kInFormats || (format == kIn8Bit) != (u8_table != nullptr)) return false;
    return format != kInCf32 || (scale > 0.0f && scale <= kInMaxScale);   // (a NaN fails both)
}

bool mix_params_ok(const MixParams &m)
{
    if (m.period == 0) return true;
    return m.period <= kMixMaxPeriod && m.table && m.phase < m.period && m.recip == (uint32_t)(((1ull << 32) + m.period - 1u) / m.period);
}

int launch_mix_store(const MixTable &t, uint32_t period, uint2 *d_table, void *stream)
{
    if (period < 1 || period > kMixMaxPeriod || !d_table) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mix_store, dim3(1), dim3(256), 0, (hipStream_t)stream, t, period, d_table);
    return (int)hipGetLastError();
}

}  // namespace adsb
