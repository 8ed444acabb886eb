// adsb_instat.hip -- k_instat and k_instat_bank: the input statistics of a decimator, a resampler or a bank
// (include/adsb_hip.h, "Input statistics": adsb_input_stats), counted on the RAW input of a call, in front of the filter
// launch that reads the same bytes.  One body, a kernel per format; the bank form takes run blockIdx.y's src, n_in and
// stream index from the descriptors k_resamp_bank reads.
//
// A streaming pass that reads every byte once.  A tile is kInstatThreads x kInstatUnroll 16-byte loads (16 KB): all of a
// lane's loads are issued back to back through a buffer resource that spans exactly the tile's valid bytes (rounded up to
// a dword), then converted by adsb_fmt_dev.h's functions -- the filter's own -- and counted.  A workgroup takes tiles
// blockIdx.x, blockIdx.x + gridDim.x, ...; a sample at or behind n_in is masked by POSITION (a zero byte is a rail of the
// 8-bit format, and the int16 behind an odd REAL16 end shares its dword with the last sample).
//
// Every accumulator is an integer in registers:
//   * sums: re and im through v_dot2_i32_i16 against {1, 0} and {0, 1} into 32 bits per tile (32 samples of 2^15 at most),
//     re^2 and im^2 through the same instruction over PAIRS of samples (2 x 2^30 fits 32 bits unsigned; four rail samples
//     would not), re im per sample; all widened to 64 bits per lane;
//   * peak: |re| and |im| packed (v_pk_sub_i16, v_pk_max_i16: -32768 stays 0x8000 = 32768 unsigned), v_pk_max_u16;
//   * the histogram: no LDS, no atomic per sample.  Bin b = 1 .. 16 of a component is a 4-bit field of one 64-bit
//     register per lane, bumped by (|v| != 0) << 4 (31 - clz |v|); after eight bumps at most the sixteen nibbles are
//     spread (two masks, a shift) over sixteen byte fields in four registers, and those once per tile over sixteen 32-bit
//     counters.  Bin 0 is what is left: components counted minus the other sixteen;
//   * clipped and NaN counts per lane.
// Then shuffles across the wave, LDS across the four waves, and ONE set of 64-bit atomics per workgroup into the
// stream's accumulator (laid out as the record): thread k adds word k, thread 25 takes the maximum of the peak.
// No scratch, no spills.
#include <algorithm>

#include "../../include/adsb_hip.h"
#include "adsb_dev_common.h"
#include "adsb_fmt_dev.h"

namespace adsb {

namespace {

constexpr int kInstatWaves = kInstatThreads / 64;
constexpr int kInstatWords = 25;   // 64-bit words of the record in front of {peak, reserved}

static_assert(sizeof(adsb_input_stats) == 208 && sizeof(adsb_input_stats) == (kInstatWords + 1) * 8, "record layout");
static_assert(offsetof(adsb_input_stats, n_samples) == 0 && offsetof(adsb_input_stats, sum_re) == 8 &&
              offsetof(adsb_input_stats, sum_im) == 16 && offsetof(adsb_input_stats, sum_re2) == 24 &&
              offsetof(adsb_input_stats, sum_im2) == 32 && offsetof(adsb_input_stats, sum_re_im) == 40 &&
              offsetof(adsb_input_stats, n_clipped) == 48 && offsetof(adsb_input_stats, n_nan) == 56 &&
              offsetof(adsb_input_stats, hist) == 64 && offsetof(adsb_input_stats, peak) == 200, "record layout");
static_assert(ADSB_INPUT_BINS == 17, "sixteen nibbles and what is left");

typedef short s16x2i __attribute__((ext_vector_type(2)));
typedef uint16_t u16x2i __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2i, a), __builtin_bit_cast(s16x2i, b), acc, false);
}

// a CS16 dword with a half at -32768 or 32767: adding 0x8001 to a half sends exactly those two to 1 and 0
__device__ __forceinline__ uint32_t rail_cs16(uint32_t w)
{
    const u16x2i two = {2, 2}, k = {0x8001, 0x8001};
    const u16x2i h = __builtin_elementwise_min((u16x2i)(__builtin_bit_cast(u16x2i, w) + k), two);
    return __builtin_bit_cast(uint32_t, h) != 0x00020002u ? 1u : 0u;
}

// a byte pair with a byte at 0 or 255
__device__ __forceinline__ uint32_t rail_u8(uint32_t b2)
{
    const uint32_t re = b2 & 0xFFu, im = (b2 >> 8) & 0xFFu;
    return (((re + 1u) & 0xFFu) < 2u || ((im + 1u) & 0xFFu) < 2u) ? 1u : 0u;
}

struct InstatAcc {
    long long sum_re = 0, sum_im = 0, sum_re_im = 0;
    unsigned long long sum_re2 = 0, sum_im2 = 0;
    int tile_re = 0, tile_im = 0;      // this tile's, 32 bits
    uint32_t clipped = 0, nan = 0;
    u16x2i peak = {0, 0};              // {max |re|, max |im|}
    unsigned long long nibbles = 0;    // bins 1 .. 16, four bits each
    uint32_t bytes[4] = {0, 0, 0, 0};  // [0]: bins 1 3 5 7, [1]: 2 4 6 8, [2]: 9 11 13 15, [3]: 10 12 14 16
    uint32_t bins[16] = {};            // bin k + 1
};

__device__ __forceinline__ void bump_bin(InstatAcc &a, uint32_t mag)
{
    // 1 <= mag <= 32768: clz 31 .. 16, field 0 .. 15.  mag = 0 adds nothing, wherever the shift points
    const uint32_t shift = (4u * (31u - (uint32_t)__clz((int)mag))) & 63u;
    a.nibbles += (unsigned long long)min(mag, 1u) << shift;
}

// two samples as CS16 dwords: everything but the clipped and NaN counts
__device__ __forceinline__ void count_pair(InstatAcc &a, uint32_t w0, uint32_t w1)
{
    a.tile_re = dot2(w1, 0x00000001u, dot2(w0, 0x00000001u, a.tile_re));
    a.tile_im = dot2(w1, 0x00010000u, dot2(w0, 0x00010000u, a.tile_im));
    a.sum_re2 += (uint32_t)dot2(w1, w1 & 0xFFFFu, dot2(w0, w0 & 0xFFFFu, 0));
    a.sum_im2 += (uint32_t)dot2(w1, w1 & 0xFFFF0000u, dot2(w0, w0 & 0xFFFF0000u, 0));
    a.sum_re_im += (long long)dot2(w0, w0 >> 16, 0) + (long long)dot2(w1, w1 >> 16, 0);
    const u16x2i zero = {0, 0};
#pragma unroll
    for (int i = 0; i < 2; i++) {
        // |re|, |im|: the negation wraps (unsigned), so -32768 stays 0x8000 and reads 32768
        const u16x2i u = __builtin_bit_cast(u16x2i, i ? w1 : w0);
        const s16x2i neg = __builtin_bit_cast(s16x2i, (u16x2i)(zero - u));
        const u16x2i mag = __builtin_bit_cast(u16x2i, __builtin_elementwise_max(__builtin_bit_cast(s16x2i, u), neg));
        a.peak = __builtin_elementwise_max(a.peak, mag);
        bump_bin(a, mag.x);
        bump_bin(a, mag.y);
    }
}

// after eight bumps at most: the nibbles join the byte fields
__device__ __forceinline__ void spread_nibbles(InstatAcc &a)
{
    const uint32_t lo = (uint32_t)a.nibbles, hi = (uint32_t)(a.nibbles >> 32), m = 0x0F0F0F0Fu;
    a.bytes[0] += lo & m;
    a.bytes[1] += (lo >> 4) & m;
    a.bytes[2] += hi & m;
    a.bytes[3] += (hi >> 4) & m;
    a.nibbles = 0;
}

// once per tile (64 bumps of one field at most): the byte fields and the tile's two sums join the wide counters
__device__ __forceinline__ void end_tile(InstatAcc &a)
{
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int k = 0; k < 4; k++) a.bins[(r & 1) + 2 * k + 8 * (r >> 1)] += (a.bytes[r] >> (8 * k)) & 0xFFu;
        a.bytes[r] = 0;
    }
    a.sum_re += a.tile_re, a.sum_im += a.tile_im;
    a.tile_re = a.tile_im = 0;
}

// One 16-byte load `v` whose first sample is sample `first` of a tile with `valid` samples.  FULL: every sample of the
// tile is inside the call.
template <uint32_t FMT, bool FULL>
__device__ __forceinline__ void take_load(InstatAcc &a, const uint32_t v[4], uint32_t first, uint32_t valid, const uint16_t *s_tab,
                                          float g)
{
    constexpr int kPer = 16 / (int)in_bytes_per_sample(FMT);   // 4, 8, 2, 8 samples
    uint32_t w[kPer];
#pragma unroll
    for (int i = 0; i < kPer; i++) {
        uint32_t clipped, nan = 0;
        if constexpr (FMT == kInCs16) {
            w[i] = v[i];
            clipped = rail_cs16(w[i]);
        } else if constexpr (FMT == kIn8Bit) {
            const uint32_t b2 = fmt_halfword(v, i);
            w[i] = widen_u8_pair(s_tab, b2);
            clipped = rail_u8(b2);   // the bytes decide, not the table
        } else if constexpr (FMT == kInReal16) {
            w[i] = fmt_halfword(v, i);
            clipped = rail_cs16(w[i]);   // (the high half is zero: no rail)
        } else {
            const float re = __builtin_bit_cast(float, v[2 * i]), im = __builtin_bit_cast(float, v[2 * i + 1]);
            w[i] = fmt_cf32(v[2 * i], v[2 * i + 1], g);
            nan = (re != re || im != im) ? 1u : 0u;   // (x g is a NaN exactly where x is: g is finite and not zero)
            clipped = rail_cs16(w[i]);                // a NaN component converted to 0: never a rail
        }
        if constexpr (!FULL) {
            const bool in = first + (uint32_t)i < valid;
            w[i] = in ? w[i] : 0u, clipped = in ? clipped : 0u, nan = in ? nan : 0u;
        }
        a.clipped += clipped, a.nan += nan;
    }
#pragma unroll
    for (int i = 0; i < kPer; i += 2) {
        count_pair(a, w[i], w[i + 1]);
        // eight bumps: four samples of two components (REAL16: eight of one)
        if (FMT != kInReal16 && (i & 2)) spread_nibbles(a);
    }
    if (FMT == kInReal16 || FMT == kInCf32) spread_nibbles(a);
}

template <uint32_t FMT, bool FULL>
__device__ __forceinline__ void take_tile(InstatAcc &a, const uint32_t v[kInstatUnroll][4], uint32_t valid, const uint16_t *s_tab,
                                          float g)
{
    constexpr uint32_t kPer = 16u / in_bytes_per_sample(FMT);
#pragma unroll
    for (int i = 0; i < kInstatUnroll; i++)
        take_load<FMT, FULL>(a, v[i], ((uint32_t)i * kInstatThreads + threadIdx.x) * kPer, valid, s_tab, g);
    end_tile(a);
}

// The body: n_in > 0 samples of `src` in FMT into the record at `acc` (device memory).
template <uint32_t FMT>
__device__ __forceinline__ void instat_body(const void *src, unsigned long long n_in, const uint16_t *u8_table, float g,
                                            unsigned long long *acc)
{
    constexpr uint32_t kBps = in_bytes_per_sample(FMT), kTile = instat_tile_samples(FMT);
    __shared__ uint16_t s_tab[FMT == kIn8Bit ? 256 : 1];
    __shared__ unsigned long long s_red[kInstatWaves][kInstatWords + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long n_tiles = (n_in + kTile - 1) / kTile;
    if (blockIdx.x >= n_tiles) return;   // (whole workgroups; a bank's grid is as wide as its longest run)
    if constexpr (FMT == kIn8Bit) {
        for (int i = tid; i < 256; i += kInstatThreads) s_tab[i] = u8_table[i];
        __syncthreads();
    }

    InstatAcc a;
    unsigned long long counted = 0;
    for (unsigned long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const unsigned long long start = tile * kTile;
        const uint32_t valid = (uint32_t)min((unsigned long long)kTile, n_in - start);
        // the tile's valid bytes, rounded up to a dword: a load behind them returns zero, and nothing behind the dword
        // that holds the call's last sample is ever fetched
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            (void *)((const uint8_t *)src + start * kBps), 0, (int)((valid * kBps + 3u) & ~3u), 0x00020000);
        uint32_t v[kInstatUnroll][4];
#pragma unroll
        for (int i = 0; i < kInstatUnroll; i++) {
            const u32x4i q = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (i * kInstatThreads + tid) * 16, 0, 0);
            v[i][0] = q.x, v[i][1] = q.y, v[i][2] = q.z, v[i][3] = q.w;
        }
        if (valid == kTile) take_tile<FMT, true>(a, v, valid, s_tab, g);
        else take_tile<FMT, false>(a, v, valid, s_tab, g);
        counted += valid;
    }

    // the record's words as this lane has them, in the record's order
    unsigned long long f[kInstatWords];
    f[0] = counted;   // (the same in every lane: taken from lane 0 below)
    f[1] = (unsigned long long)a.sum_re, f[2] = (unsigned long long)a.sum_im;
    f[3] = a.sum_re2, f[4] = a.sum_im2, f[5] = (unsigned long long)a.sum_re_im;
    f[6] = a.clipped, f[7] = a.nan;
    f[8] = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) f[9 + k] = a.bins[k];
    uint32_t peak = max((uint32_t)a.peak.x, (uint32_t)a.peak.y);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 1; k < kInstatWords; k++) f[k] += __shfl_xor(f[k], d);
        peak = max(peak, (uint32_t)__shfl_xor((int)peak, d));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kInstatWords; k++) s_red[wave][k] = f[k];
        s_red[wave][kInstatWords] = peak;
    }
    __syncthreads();
    if (tid <= kInstatWords) {
        unsigned long long sum = 0, top = 0;
        for (int w = 0; w < kInstatWaves; w++) sum += s_red[w][tid], top = max(top, s_red[w][tid]);
        if (tid == 0) sum = counted;
        if (tid == 8) {
            // bin 0: the components counted (one per sample of REAL16, whose im is no sample) minus the other bins
            sum = counted * (FMT == kInReal16 ? 1u : 2u);
            for (int w = 0; w < kInstatWaves; w++)
                for (int k = 9; k < kInstatWords; k++) sum -= s_red[w][k];
        }
        if (tid == kInstatWords) {
            if (top) atomicMax((uint32_t *)(acc + kInstatWords), (uint32_t)top);
        } else if (sum) {
            atomicAdd(acc + tid, sum);
        }
    }
}

template <uint32_t FMT>
__global__ __launch_bounds__(kInstatThreads) void k_instat(InstatParams p)
{
    instat_body<FMT>(p.src, p.n_in, p.u8_table, p.scale, p.acc);
}

// A bank's launch: run blockIdx.y's src and n_in, and in `reserved` the stream whose record it counts into, from the
// descriptors k_resamp_bank reads -- two 16-byte scalar loads, the index being wave-uniform.
template <uint32_t FMT>
__global__ __launch_bounds__(kInstatThreads) void k_instat_bank(InstatParams p, const ResampBankRun *runs)
{
    typedef const u32x4i __attribute__((address_space(4))) *const_run_ptr;
    const const_run_ptr d = (const_run_ptr)(uintptr_t)(runs + blockIdx.y);
    const u32x4i a = d[0], e = d[3];
    const auto wide = [](uint32_t lo, uint32_t hi) { return (unsigned long long)lo | (unsigned long long)hi << 32; };
    const uint32_t stream = e.w;
    if (stream >= p.n_streams) return;   // (launch_instat_bank has checked every descriptor)
    instat_body<FMT>((const void *)wide(a.x, a.y), wide(a.z, a.w), p.u8_table, p.scale, p.acc + (size_t)stream * (kInstatWords + 1));
}

bool instat_params_ok(const InstatParams &p)
{
    return p.acc && ((uintptr_t)p.acc & 7u) == 0 && p.n_streams >= 1 && in_format_ok(p.format, p.u8_table, p.scale);
}

uint32_t instat_groups(unsigned long long n_in, uint32_t format)
{
    const unsigned long long tile = instat_tile_samples(format);
    return (uint32_t)std::min<unsigned long long>((n_in + tile - 1) / tile, kInstatMaxGroups);
}

#define INSTAT_PICK(K, format)                 \
    ((format) == kInCf32     ? K<kInCf32>      \
     : (format) == kInReal16 ? K<kInReal16>    \
     : (format) == kIn8Bit   ? K<kIn8Bit>      \
                             : K<kInCs16>)

}  // namespace

int launch_instat(const InstatParams &p, void *stream)
{
    if (!instat_params_ok(p) || p.n_streams != 1 || !p.src || ((uintptr_t)p.src & 15u) != 0 || !p.n_in) return (int)hipErrorInvalidValue;
    const auto kernel = INSTAT_PICK(k_instat, p.format);
    hipLaunchKernelGGL(kernel, dim3(instat_groups(p.n_in, p.format)), dim3(kInstatThreads), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

int launch_instat_bank(const InstatParams &common, const ResampBankRun *runs, const ResampBankRun *d_runs, uint32_t n_runs, void *stream)
{
    if (!instat_params_ok(common) || !runs || !d_runs || n_runs < 1 || n_runs > kResampBankMaxRuns) return (int)hipErrorInvalidValue;
    uint32_t widest = 0;
    for (uint32_t r = 0; r < n_runs; r++) {
        const ResampBankRun &d = runs[r];
        if (!d.src || ((uintptr_t)d.src & 15u) != 0 || !d.n_in || d.reserved >= common.n_streams) return (int)hipErrorInvalidValue;
        widest = std::max(widest, instat_groups(d.n_in, common.format));
    }
    // a workgroup's reduction and its 26 atomics cost about what a tile does: where the runs alone fill the device, each
    // run gets few workgroups and every workgroup several tiles (kInstatBankGroups over the whole grid)
    const uint32_t per_run = std::max(1u, std::min(widest, (kInstatBankGroups + n_runs - 1u) / n_runs));
    const auto kernel = INSTAT_PICK(k_instat_bank, common.format);
    hipLaunchKernelGGL(kernel, dim3(per_run, n_runs), dim3(kInstatThreads), 0, (hipStream_t)stream, common, d_runs);
    return (int)hipGetLastError();
}

}  // namespace adsb
