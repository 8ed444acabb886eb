// adsb_resamp_host.h -- what adsb_resamp.cpp (one stream) and adsb_bank.cpp (many) share on the host: the argument checks
// of a create, the count arithmetic of include/adsb_hip.h, "Resampling" (64-bit host arithmetic: no call synchronises to
// learn a count), the taps' polyphase order and the launch parameters a ratio and a filter fix.  Not part of the ABI.
#pragma once
#include <numeric>

#include "adsb_ctx.h"

namespace adsb {
namespace host {

typedef unsigned __int128 u128;

inline bool ratio_ok(uint64_t up, uint64_t down)
{
    return up >= 1 && up <= kResampMaxRatio && down >= 1 && down <= kResampMaxRatio && std::gcd(up, down) == 1 &&
           up <= 2 * down && down <= 16 * up;
}

// ceil(a L / M)
inline uint64_t ceil_mul_div(uint64_t a, uint32_t L, uint32_t M) { return (uint64_t)(((u128)a * L + (M - 1)) / M); }
// outputs of a call of n_in inputs behind P consumed ones: the n with P <= floor(n M / L) < P + n_in
inline void plan(uint32_t L, uint32_t M, uint64_t P, uint64_t n_in, uint64_t *first_n, uint64_t *n_out)
{
    const uint64_t first = ceil_mul_div(P, L, M);
    *first_n = first;
    *n_out = (uint64_t)(((u128)P + n_in) * L / M + ((((u128)P + n_in) * L) % M != 0)) - first;
}
inline uint64_t out_count(uint32_t L, uint32_t M, uint64_t P, uint64_t n_in)
{
    uint64_t first, n;
    plan(L, M, P, n_in, &first, &n);
    return n;
}
// the fewest inputs behind P that produce at least `need` outputs (need >= 1): up to the newest input of output
// first_n + need - 1
inline uint64_t inputs_for(uint32_t L, uint32_t M, uint64_t P, uint64_t need)
{
    const uint64_t last = ceil_mul_div(P, L, M) + need - 1;
    return (uint64_t)((u128)last * M / L) - P + 1;
}
// the first output behind P consumed inputs, reduced: n0 = ceil(P L / M), n0 M = P L + d with d = (-P L) mod M, so
// floor(n0 M / L) = P + d div L and (n0 M) mod L = d mod L
inline void first_output(uint32_t L, uint32_t M, uint64_t P, uint32_t *p0, uint32_t *q0)
{
    const uint32_t d = (uint32_t)((M - (P % M) * L % M) % M);
    *p0 = d % L, *q0 = d / L;
}

// adsb_resamp_create's checks of (up, down, taps, n_taps, shift) that need no device; K in *k_taps
inline bool filter_ok(uint32_t up, uint32_t down, const int16_t *taps, uint32_t n_taps, uint32_t shift, uint32_t *k_taps)
{
    if (!ratio_ok(up, down) || n_taps < 1 || n_taps > kResampMaxTaps || shift > kResampMaxShift) return false;
    *k_taps = (n_taps + up - 1) / up;
    if (*k_taps > kResampMaxPhaseTaps) return false;
    // (an int32 accumulator never wraps: 65534 * 32768 + 32768 < 2^31)
    std::vector<uint32_t> abs_sum(up, 0);
    for (uint32_t k = 0; k < n_taps; k++) abs_sum[k % up] += (uint32_t)std::abs((int)taps[k]);
    for (uint32_t s : abs_sum)
        if (s > 65534u) return false;
    return resamp_rows(up, down) != 0;
}

// the prototype's taps in polyphase order: [p][j] = h[p + j L]
inline std::vector<int32_t> polyphase(const int16_t *taps, uint32_t n_taps, uint32_t L, uint32_t k_pad)
{
    std::vector<int32_t> out((size_t)L * k_pad, 0);
    for (uint32_t k = 0; k < n_taps; k++) out[(size_t)(k % L) * k_pad + k / L] = taps[k];
    return out;
}

// the fields of a launch that the ratio and the filter fix
inline void filter_params(ResampParams &p, uint32_t L, uint32_t M, uint32_t k_taps, uint32_t k_pad, uint32_t shift, const int32_t *d_taps)
{
    p.taps = d_taps;
    p.up = L, p.down = M, p.k_taps = k_taps, p.k_pad = k_pad, p.shift = shift;
    p.rows = resamp_rows(L, M);
    p.row_len = resamp_row_len(M, p.rows, k_taps);
    p.recip_up = (uint32_t)(((1ull << 32) + L - 1u) / L);
    p.recip_down = (uint32_t)(((1ull << 32) + M - 1u) / M);
}

}  // namespace host
}  // namespace adsb
