// adsb_stats.hip -- k_signal_stats: the per-buffer signal statistics of a pass (include/adsb_hip.h,
// "Signal statistics": adsb_signal_stats), counted where the magnitudes are -- on the IQ path they never exist
// in memory, so nobody else can.
//
// A streaming pass over the input of a pass, read once: 16-byte loads of CS16 (8-byte loads of CU8, widened
// through the table in LDS), four samples per lane and load, through the scan's own magnitude function
// (adsb_dev_common.h: mag2 / mag4_of), so the two cannot disagree.  Every accumulator is an integer: the result
// does not depend on the order anything is added in.
//
//   * a buffer is cut into SigParams::wg_per_chunk equal parts, one workgroup each (launch_signal_stats: enough
//     workgroups to fill the device for a one-buffer pass and for a 512-buffer pass alike);
//   * per lane, in registers: sum of m^2, peak, strong and clipped counts -- reduced across the wave with
//     shuffles, one atomic per wave and figure into the buffer's partials in device memory;
//   * per wave, in LDS: kSigCopies copies of the 60-bin histogram (a lane adds to copy lane % 8: noise puts
//     most of a wave into three or four bins, and adds to ONE address serialise), bumped with non-returning
//     LDS adds; merged once per workgroup, one atomic per non-empty bin into the partials;
//   * a ticket per buffer: the workgroup that draws the last one reads the partials, writes the finished
//     272-byte record ONCE into the context's mapped host block -- seventeen 16-byte write-through stores, the
//     ones the record builders use (adsb_tail_dev.h: host_store128) -- and leaves partials and ticket zero for
//     the next pass: the invariant the slot lists keep.  No atomic ever touches host memory.
#include "../../include/adsb_hip.h"
#include "adsb_dev_common.h"
#include "adsb_tail_dev.h"

namespace adsb {

namespace {

constexpr int kSigThreads = 256, kSigWaves = kSigThreads / 64;
constexpr int kSigCopies = 8;                             // histogram copies per wave
constexpr int kSigWaveWords = kSigHistBins * kSigCopies;  // 480 words of LDS per wave
constexpr int kSigStride = 4 * kSigThreads;               // samples a workgroup takes per round of loads
constexpr int kSigUnroll = 4;                             // rounds of loads in flight per lane
// 2 m^2 >= 65535^2 (above -3 dBFS)  <=>  m >= 46341: 2 * 46340^2 = 4294791200 < 65535^2 = 4294836225 <= 2 * 46341^2
constexpr uint32_t kSigStrongMag = 46341u;

static_assert(sizeof(adsb_signal_stats) == kSigRecordWords * 4 && kSigRecordWords % 4 == 0, "record layout");
static_assert(offsetof(adsb_signal_stats, sum_power) == 8 && offsetof(adsb_signal_stats, n_samples) == 16 &&
              offsetof(adsb_signal_stats, peak) == 20 && offsetof(adsb_signal_stats, n_strong) == 24 &&
              offsetof(adsb_signal_stats, n_clipped) == 28 && offsetof(adsb_signal_stats, hist) == 32, "record layout");
static_assert(kChunkSamples % (kSigMaxWgPerChunk * kSigStride) == 0, "a workgroup's part is whole rounds of loads");

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

// adsb_signal_bin (include/adsb_hip.h) in closed form: with s = max(floor(log2 m) - 2, 0) the bin is 4 s + (m >> s)
// -- m itself below 8 (s = 0), and 8 + 4 (e - 3) + ((m >> (e - 2)) & 3) from there on, where m >> (e - 2) is 4..7.
__device__ __forceinline__ uint32_t sig_bin(uint32_t m)
{
    const int s = max(29 - (int)__builtin_clz(m | 1u), 0);
    return 4u * (uint32_t)s + (m >> s);
}

struct SigAcc {
    unsigned long long sum = 0;  // sum of m^2: 2^17 samples of < 2^32 each
    u16x2 peak = {0, 0};         // two running maxima (of the even and of the odd samples)
    uint32_t strong = 0, clipped = 0;
};

// one magnitude: everything but the peak and the clip count
__device__ __forceinline__ void sig_count(SigAcc &a, uint32_t *hist_lane, uint32_t m)
{
    // (m < 2^16: the 24-bit multiply is exact and full rate; through uint32_t, so that a square of 2^31 and more --
    // every strong sample's -- is not widened as a negative int)
    a.sum += (unsigned long long)(uint32_t)__umul24(m, m);
    a.strong += m >= kSigStrongMag ? 1u : 0u;
    (void)__hip_atomic_fetch_add(hist_lane + sig_bin(m) * kSigCopies, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// a CS16 sample {re, im} with a component at a rail, -32768 or 32767: adding 0x8001 to a half sends exactly those
// two values to 1 and 0
__device__ __forceinline__ uint32_t clipped_cs16(uint32_t w)
{
    const u16x2 two = {2, 2}, k = {0x8001, 0x8001};
    const u16x2 h = __builtin_elementwise_min((u16x2)(__builtin_bit_cast(u16x2, w) + k), two);
    return __builtin_bit_cast(uint32_t, h) != 0x00020002u ? 1u : 0u;
}

// a CU8 sample (two bytes) with a byte at a rail, 0 or 255
__device__ __forceinline__ uint32_t clipped_cu8(uint32_t b2)
{
    const uint32_t re = b2 & 0xFFu, im = (b2 >> 8) & 0xFFu;
    return (((re + 1u) & 0xFFu) < 2u || ((im + 1u) & 0xFFu) < 2u) ? 1u : 0u;
}

// four samples as CS16 dwords (`cs16`) and their clip count: the magnitudes through mag4_of, then the counters
__device__ __forceinline__ void sig_count4(SigAcc &a, uint32_t *hist_lane, uint4 cs16, uint32_t n_clipped)
{
    const uint2 pk = mag4_of(cs16);
    a.peak = __builtin_elementwise_max(a.peak, __builtin_bit_cast(u16x2, pk.x));
    a.peak = __builtin_elementwise_max(a.peak, __builtin_bit_cast(u16x2, pk.y));
    a.clipped += n_clipped;
    sig_count(a, hist_lane, pk.x & 0xFFFFu);
    sig_count(a, hist_lane, pk.x >> 16);
    sig_count(a, hist_lane, pk.y & 0xFFFFu);
    sig_count(a, hist_lane, pk.y >> 16);
}

// the four samples at k (a multiple of 4, all four inside the buffer) through a buffer resource over exactly this
// buffer's valid samples, as the scan loads its tiles: one 16-byte load of CS16, one 8-byte load of CU8 (the resource
// covers whole dwords), and a load that strayed outside the buffer would read zero, not memory
template <bool U8>
__device__ __forceinline__ uint4 sig_load4(__amdgpu_buffer_rsrc_t rsrc, int k)
{
    if constexpr (U8) {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, k * 2, 0, 0);
        return make_uint4(v.x, v.y, 0u, 0u);
    } else {
        const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, k * 4, 0, 0);
        return make_uint4(v.x, v.y, v.z, v.w);
    }
}

template <bool U8>
__device__ __forceinline__ void sig_take4(SigAcc &a, uint32_t *hist_lane, const uint16_t *tab, uint4 v)
{
    if constexpr (U8) {
        const uint32_t b0 = v.x & 0xFFFFu, b1 = v.x >> 16, b2 = v.y & 0xFFFFu, b3 = v.y >> 16;
        const uint4 w = make_uint4(widen_u8_pair(tab, b0), widen_u8_pair(tab, b1), widen_u8_pair(tab, b2), widen_u8_pair(tab, b3));
        sig_count4(a, hist_lane, w, clipped_cu8(b0) + clipped_cu8(b1) + clipped_cu8(b2) + clipped_cu8(b3));
    } else {
        sig_count4(a, hist_lane, v, clipped_cs16(v.x) + clipped_cs16(v.y) + clipped_cs16(v.z) + clipped_cs16(v.w));
    }
}

template <bool U8>
__global__ __launch_bounds__(kSigThreads) void k_signal_stats(const SigParams p)
{
    __shared__ uint32_t s_hist[kSigWaves * kSigWaveWords];
    __shared__ uint16_t s_tab[U8 ? 256 : 1];
    __shared__ uint32_t s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t chunk = blockIdx.x / p.wg_per_chunk, part = blockIdx.x % p.wg_per_chunk;
    if (chunk >= p.n_chunks) return;   // (whole workgroups: the grid is n_chunks * wg_per_chunk)

    for (int i = tid; i < kSigWaves * kSigWaveWords; i += kSigThreads) s_hist[i] = 0u;
    if constexpr (U8)
        for (int i = tid; i < 256; i += kSigThreads) s_tab[i] = p.u8_table[i];
    __syncthreads();

    const int len = chunk_len(p.n_samples, chunk);          // 1 .. 131072 valid samples in this buffer
    const int part_len = kChunkSamples / (int)p.wg_per_chunk;  // a multiple of kSigStride
    const int k_begin = (int)part * part_len;
    const int k_end = min(k_begin + part_len, len);
    const int full_end = min(k_end, len & ~3);              // below it every group of four is whole
    const void *base = (const uint8_t *)p.src + (size_t)chunk * kChunkSamples * (U8 ? 2u : 4u);
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, U8 ? ((len * 2 + 3) & ~3) : len * 4, 0x00020000);
    uint32_t *hist_lane = s_hist + wave * kSigWaveWords + (lane & (kSigCopies - 1));

    SigAcc a;
    int k = k_begin + 4 * tid;
    for (; k + (kSigUnroll - 1) * kSigStride < full_end; k += kSigUnroll * kSigStride) {
        uint4 v[kSigUnroll];
#pragma unroll
        for (int i = 0; i < kSigUnroll; i++) v[i] = sig_load4<U8>(rsrc, k + i * kSigStride);
#pragma unroll
        for (int i = 0; i < kSigUnroll; i++) sig_take4<U8>(a, hist_lane, s_tab, v[i]);
    }
    for (; k < full_end; k += kSigStride) sig_take4<U8>(a, hist_lane, s_tab, sig_load4<U8>(rsrc, k));
    // the ragged end of a short last buffer: its one to three samples, by the lane whose group they are
    if (k == full_end && k < k_end) {
        const int n = k_end - k;
        uint32_t w[3] = {0u, 0u, 0u}, clip[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (i >= n) continue;
            if constexpr (U8) {
                const uint8_t *b = (const uint8_t *)base + 2 * (size_t)(k + i);
                const uint32_t b2 = (uint32_t)b[0] | (uint32_t)b[1] << 8;
                w[i] = widen_u8_pair(s_tab, b2);
                clip[i] = clipped_cu8(b2);
            } else {
                w[i] = ((const uint32_t *)base)[k + i];
                clip[i] = clipped_cs16(w[i]);
            }
        }
        const uint2 pk = mag4_of(make_uint4(w[0], w[1], w[2], 0u));
        const uint32_t m[3] = {pk.x & 0xFFFFu, pk.x >> 16, pk.y & 0xFFFFu};
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (i >= n) continue;
            a.clipped += clip[i];
            a.peak = __builtin_elementwise_max(a.peak, (u16x2){(uint16_t)m[i], 0});
            sig_count(a, hist_lane, m[i]);
        }
    }

    // the wave's figures: shuffles, then one atomic each into the buffer's partials (laid out as the record is)
    uint32_t peak = max((uint32_t)a.peak.x, (uint32_t)a.peak.y);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a.sum += __shfl_xor(a.sum, d);
        peak = max(peak, (uint32_t)__shfl_xor((int)peak, d));
        a.strong += (uint32_t)__shfl_xor((int)a.strong, d);
        a.clipped += (uint32_t)__shfl_xor((int)a.clipped, d);
    }
    uint32_t *part_words = p.partial + (size_t)chunk * kSigRecordWords;
    if (lane == 0) {
        if (a.sum) atomicAdd((unsigned long long *)(part_words + 2), a.sum);
        if (peak) atomicMax(part_words + 5, peak);
        if (a.strong) atomicAdd(part_words + 6, a.strong);
        if (a.clipped) atomicAdd(part_words + 7, a.clipped);
    }
    __syncthreads();   // every wave's LDS adds are done
    if (tid < kSigHistBins) {
        uint32_t n = 0;
        for (int w = 0; w < kSigWaves; w++)
#pragma unroll
            for (int c = 0; c < kSigCopies; c++) n += s_hist[w * kSigWaveWords + tid * kSigCopies + c];
        if (n) atomicAdd(part_words + 8 + tid, n);
    }

    // the ticket: whoever draws the buffer's last one finds every workgroup's atomics performed
    __threadfence();
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(p.ticket + chunk, 1u) == p.wg_per_chunk - 1u ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    if (tid < kSigRecordWords / 4) {
        u32x4_t v;
        v.x = __hip_atomic_load(part_words + 4 * tid + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v.y = __hip_atomic_load(part_words + 4 * tid + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v.z = __hip_atomic_load(part_words + 4 * tid + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v.w = __hip_atomic_load(part_words + 4 * tid + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid == 0) v.x = chunk, v.y = 0u;      // adsb_signal_stats::chunk
        if (tid == 1) v.x = (uint32_t)len;        // ... ::n_samples
        host_store128((char *)p.records + (size_t)chunk * sizeof(adsb_signal_stats) + 16 * tid, v);
        // (zeroed the way they were counted up and read: at the memory side, past this XCD's L2)
#pragma unroll
        for (int i = 0; i < 4; i++) __hip_atomic_store(part_words + 4 * tid + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 0) __hip_atomic_store(p.ticket + chunk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

inline int hip_ok(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }

}  // namespace

uint32_t signal_stats_wg_per_chunk(uint32_t n_chunks)
{
    // ~8 workgroups of 256 lanes per CU over the whole pass: 64 per buffer for a one-buffer pass, 4 for 512
    uint32_t w = 1;
    while (w < (uint32_t)kSigMaxWgPerChunk && (uint64_t)n_chunks * w < 2048u) w <<= 1;
    return w;
}

int launch_signal_stats(const SigParams &p, SrcFormat fmt, void *stream)
{
    (void)hipGetLastError();
    if (p.n_chunks == 0 || p.wg_per_chunk == 0 || p.wg_per_chunk > (uint32_t)kSigMaxWgPerChunk ||
        (p.wg_per_chunk & (p.wg_per_chunk - 1u)) != 0 || fmt == SrcFormat::kMag || (fmt == SrcFormat::kCu8 && !p.u8_table))
        return (int)hipErrorInvalidValue;
    const dim3 grid(p.n_chunks * p.wg_per_chunk);
    if (fmt == SrcFormat::kCu8) hipLaunchKernelGGL(k_signal_stats<true>, grid, dim3(kSigThreads), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(k_signal_stats<false>, grid, dim3(kSigThreads), 0, (hipStream_t)stream, p);
    return hip_ok(hipGetLastError());
}

}  // namespace adsb
