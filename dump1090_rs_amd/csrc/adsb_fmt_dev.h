// adsb_fmt_dev.h -- the sample formats of the decimator and the resampler (include/adsb_hip.h, "Sample formats"): the
// conversion k_decim, k_decim_history, k_resamp and k_resamp_history apply to a CF32 or REAL16 sample between the load
// and the mixer.  No table, no LDS: the history and everything behind the conversion see CS16 dwords.
//
//   CF32    q(x) = 0 for NaN, else clamp(rint(x g), -32768, 32767): ONE binary32 multiply (the build never contracts:
//           -ffp-contract=off, and there is nothing beside it to contract with), v_rndne_f32 (ties to even), the clamp in
//           float -- +-inf go to the rails -- and a convert that is then exact.
//   REAL16  the halfword r in the low half of the dword, the high half (im) zero.  The caller masks by position.
#pragma once
#include "adsb_dev_common.h"

namespace adsb {

__device__ __forceinline__ uint32_t fmt_q(uint32_t bits, float g)
{
    const float t = __builtin_bit_cast(float, bits) * g;
    // (fmaxf(NaN, a) = a: the clamp never yields a NaN, the convert is always in range)
    const int q = (int)fminf(fmaxf(__builtin_rintf(t), -32768.0f), 32767.0f);
    return t != t ? 0u : (uint32_t)q & 0xFFFFu;
}

// the CS16 dword of a CF32 sample: two dwords of the load, re then im
__device__ __forceinline__ uint32_t fmt_cf32(uint32_t re_bits, uint32_t im_bits, float g)
{
    return fmt_q(re_bits, g) | fmt_q(im_bits, g) << 16;
}

// halfword c (0 .. 7) of a 16-byte load: one int16, REAL16's sample or the byte pair of an 8-bit one
__device__ __forceinline__ uint32_t fmt_halfword(const uint32_t w[4], int c) { return (w[c >> 1] >> (16 * (c & 1))) & 0xFFFFu; }

}  // namespace adsb
