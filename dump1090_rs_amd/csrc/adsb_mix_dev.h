// adsb_mix_dev.h -- the mixer of the decimator and the resampler (include/adsb_hip.h, "Frequency shift"): the one device
// function the MIX instantiations of k_decim, k_decim_history, k_resamp and k_resamp_history apply to a sample on its
// way from the load to LDS or to the history, and the phase arithmetic around it.
//
//   t = m mod N,  x'[m] = clamp((x[m] (c[t] + i s[t]) + 8192 (1 + i)) >> 14), re and im separately, exact integers.
//
// The table lies in device memory, one uint2 per entry: .x = {c, -s} and .y = {s, c} as int16 pairs, so that re and im
// stay packed in their dword: one v_dot2_i32_i16 each (|c|, |s| <= 32767: -s fits).  It is read with cached 8-byte
// global loads, a lane's consecutive samples at consecutive entries: 2 KB at most, resident in the vector L1 after the
// first wave, and no LDS -- the workgroups per CU are those of the kernels without a mixer.
#pragma once
#include "adsb_dev_common.h"

namespace adsb {

typedef short s16x2m __attribute__((ext_vector_type(2)));

// x (c + i s) / 2^14 of one packed sample.  The int32 accumulator cannot wrap: 2 * 32768 * 32767 + 8192 < 2^31.
__device__ __forceinline__ uint32_t mix_sample(uint32_t x, uint2 w)
{
    const s16x2m v = __builtin_bit_cast(s16x2m, x);
    const int re = __builtin_amdgcn_sdot2(v, __builtin_bit_cast(s16x2m, w.x), 8192, false) >> 14;
    const int im = __builtin_amdgcn_sdot2(v, __builtin_bit_cast(s16x2m, w.y), 8192, false) >> 14;
    return ((uint32_t)min(max(re, -32768), 32767) & 0xFFFFu) | ((uint32_t)min(max(im, -32768), 32767) << 16);
}

// x mod n for x < 2^24 and n <= 256, with recip = ceil(2^32 / n): x (recip n - 2^32) < 2^24 * 2^8.  (n = 1: its
// reciprocal does not fit 32 bits.)
__device__ __forceinline__ uint32_t mix_mod(uint32_t x, uint32_t n, uint32_t recip)
{
    return n == 1 ? 0u : x - __umulhi(x, recip) * n;
}

// The table phase of a tile's local sample 0, which is sample  P + first + block stride - back  of the stream:
// `phase` = P mod n from the host, everything else reduced before it is multiplied -- 32-bit, wave-uniform, once per
// workgroup.  (first < 2^8, back < 2^10, stride < 2^15.)
__device__ __forceinline__ uint32_t mix_tile_phase(uint32_t phase, uint32_t first, uint32_t block, uint32_t stride, uint32_t back,
                                                   uint32_t n)
{
    const uint32_t fwd = phase + first % n + ((block % n) * (stride % n)) % n;   // < 3 n
    return (fwd + n - back % n) % n;
}

}  // namespace adsb
