// adsb_resamp.hip -- k_resamp: the exact-integer rational resampler in front of the scan (include/adsb_hip.h,
// "Resampling"), and k_resamp_history, which hands the filter's history on to the next call; k_resamp_bank and
// k_resamp_bank_history, the same two bodies over the runs of a bank's call ("Resampler banks").  The tile's body is
// adsb_resamp_body.inc.
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
#include <algorithm>

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
#include "adsb_resamp_body.inc"
}

// A bank's launch (include/adsb_hip.h, "Resampler banks"): run blockIdx.y's fields replace the call's own in the launch's
// parameters, which keep what the ratio and the filter fix.  The descriptor's index is wave-uniform and the descriptors
// lie in the constant address space: four 16-byte scalar loads.
static_assert(sizeof(ResampBankRun) == 64, "a descriptor is four 16-byte loads");
__device__ __forceinline__ void bank_run_params(ResampParams &p, const ResampBankRun *runs, uint32_t run)
{
    typedef const u32x4r __attribute__((address_space(4))) *const_run_ptr;
    const const_run_ptr d = (const_run_ptr)(uintptr_t)(runs + run);
    const u32x4r a = d[0], b = d[1], c = d[2], e = d[3];
    const auto wide = [](uint32_t lo, uint32_t hi) { return (unsigned long long)lo | (unsigned long long)hi << 32; };
    p.src = (const void *)wide(a.x, a.y);
    p.n_in = wide(a.z, a.w);
    p.out = (uint32_t *)wide(b.x, b.y);
    p.n_out = wide(b.z, b.w);
    p.hist_prev = (const uint32_t *)wide(c.x, c.y);
    p.hist_next = (uint32_t *)wide(c.z, c.w);
    p.p0 = e.x, p.q0 = e.y;
    p.mix.phase = e.z;
}

template <uint32_t FMT, bool MIX>
__global__ __launch_bounds__(kThreadsResamp) void k_resamp_bank(ResampParams common, const ResampBankRun *runs)
{
    ResampParams p = common;
    bank_run_params(p, runs, blockIdx.y);
    // the grid is as wide as the call's longest run: a tile past this run's last output has nothing to do
    if ((unsigned long long)blockIdx.x * (p.up * p.rows) >= p.n_out) return;
#include "adsb_resamp_body.inc"
}

// the last H = K - 1 inputs of the stream so far, widened: from the call's input, or from the previous history where
// the call was shorter than the history (k_decim_history's rule).  MIX: what comes from the call's input is mixed, what
// comes from the previous history is mixed already.
template <uint32_t FMT, bool MIX>
__device__ __forceinline__ void resamp_history(const ResampParams &p)
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

template <uint32_t FMT, bool MIX>
__global__ __launch_bounds__(512) void k_resamp_history(ResampParams p)
{
    resamp_history<FMT, MIX>(p);
}

// ... and of every run of a bank's call: workgroup r follows the same rule for run r
template <uint32_t FMT, bool MIX>
__global__ __launch_bounds__(512) void k_resamp_bank_history(ResampParams common, const ResampBankRun *runs)
{
    ResampParams p = common;
    bank_run_params(p, runs, blockIdx.x);
    resamp_history<FMT, MIX>(p);
}

// what the ratio and the filter fix, a call's own fields aside
bool resamp_common_ok(const ResampParams &p)
{
    if (p.up < 1 || p.up > kResampMaxRatio || p.down < 1 || p.down > kResampMaxRatio || p.k_taps < 1 ||
        p.k_taps > kResampMaxPhaseTaps || p.k_pad != ((p.k_taps + 7u) & ~7u) || p.shift > kResampMaxShift || !p.rows ||
        p.rows != resamp_rows(p.up, p.down) || p.row_len != resamp_row_len(p.down, p.rows, p.k_taps) ||
        p.recip_up != (uint32_t)(((1ull << 32) + p.up - 1u) / p.up) || p.recip_down != (uint32_t)(((1ull << 32) + p.down - 1u) / p.down) ||
        !p.taps)
        return false;
    if (!mix_params_ok(p.mix) || !in_format_ok(p.format, p.u8_table, p.scale)) return false;
    return resamp_lds_words(p.up, p.down, p.rows, p.k_taps) <= kResampLdsWords;
}

// ... and a call's own (p.up, p.down and p.rows checked): its tile count in *blocks
bool resamp_call_ok(const ResampParams &p, unsigned long long *blocks)
{
    if (p.p0 >= p.up || p.q0 >= p.down || !p.src || !p.n_in || !p.hist_prev || !p.hist_next) return false;
    // the call's first output has its newest input inside the call (then every tile's first output has)
    if (p.n_out && (!p.out || ((uintptr_t)p.out & 3u) || p.q0 >= p.n_in)) return false;
    const uint64_t tile = (uint64_t)p.up * p.rows;
    *blocks = (p.n_out + tile - 1) / tile;
    if (*blocks > 0x7FFFFFFFull) return false;
    // ... and so has its last: floor((p0 + (n_out - 1) M) / L) + q0 < n_in  (n_out < 2^31 tiles of 2^13 at most: 64 bits do)
    return !(p.n_out && ((p.n_out - 1) * p.down + p.p0) / p.up + p.q0 >= p.n_in);
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

// the instantiation of a kernel family for a format and a mixer
#define RESAMP_PICK(K, format, mix)                                                                  \
    ((format) == kInCf32     ? ((mix) ? K<kInCf32, true> : K<kInCf32, false>)                         \
     : (format) == kInReal16 ? ((mix) ? K<kInReal16, true> : K<kInReal16, false>)                     \
     : (format) == kIn8Bit   ? ((mix) ? K<kIn8Bit, true> : K<kIn8Bit, false>)                         \
                             : ((mix) ? K<kInCs16, true> : K<kInCs16, false>))

int launch_resamp(const ResampParams &p, void *stream)
{
    unsigned long long blocks = 0;
    if (!resamp_common_ok(p) || !resamp_call_ok(p, &blocks)) return (int)hipErrorInvalidValue;
    const bool mix = p.mix.period != 0;
    if (blocks) {
        const size_t lds_bytes = (size_t)resamp_lds_words(p.up, p.down, p.rows, p.k_taps) * 4u;
        const auto kernel = RESAMP_PICK(k_resamp, p.format, mix);
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(kThreadsResamp), lds_bytes, (hipStream_t)stream, p);
        if (hipError_t e = hipGetLastError()) return (int)e;
    }
    if (p.k_taps > 1) {
        const auto kernel = RESAMP_PICK(k_resamp_history, p.format, mix);
        hipLaunchKernelGGL(kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, p);
    }
    return (int)hipGetLastError();
}

int launch_resamp_bank(const ResampParams &common, const ResampBankRun *runs, const ResampBankRun *d_runs, uint32_t n_runs,
                       void *stream)
{
    if (!resamp_common_ok(common) || !runs || !d_runs || n_runs < 1 || n_runs > kResampBankMaxRuns) return (int)hipErrorInvalidValue;
    // every run as the launch_resamp of a handle would check it, and the widest of them
    unsigned long long widest = 0;
    for (uint32_t r = 0; r < n_runs; r++) {
        ResampParams p = common;
        const ResampBankRun &d = runs[r];
        p.src = d.src, p.n_in = d.n_in, p.out = d.out, p.n_out = d.n_out, p.hist_prev = d.hist_prev, p.hist_next = d.hist_next;
        p.p0 = d.p0, p.q0 = d.q0, p.mix.phase = d.mix_phase;
        unsigned long long blocks = 0;
        if (!resamp_call_ok(p, &blocks) || (common.mix.period && d.mix_phase >= common.mix.period)) return (int)hipErrorInvalidValue;
        widest = std::max(widest, blocks);
    }
    const bool mix = common.mix.period != 0;
    if (widest) {
        const size_t lds_bytes = (size_t)resamp_lds_words(common.up, common.down, common.rows, common.k_taps) * 4u;
        const auto kernel = RESAMP_PICK(k_resamp_bank, common.format, mix);
        hipLaunchKernelGGL(kernel, dim3((uint32_t)widest, n_runs), dim3(kThreadsResamp), lds_bytes, (hipStream_t)stream, common, d_runs);
        if (hipError_t e = hipGetLastError()) return (int)e;
    }
    if (common.k_taps > 1) {
        const auto kernel = RESAMP_PICK(k_resamp_bank_history, common.format, mix);
        hipLaunchKernelGGL(kernel, dim3(n_runs), dim3(512), 0, (hipStream_t)stream, common, d_runs);
    }
    return (int)hipGetLastError();
}

}  // namespace adsb
