// adsb_mix.cpp -- the host side of the mixer a decimator or a resampler may carry (include/adsb_hip.h, "Frequency
// shift"): the table's checks and its way to the device (k_mix_store, adsb_decim.hip), and the two host-only helpers,
// adsb_mix_table and adsb_mix_for_shift.  The handles are adsb_decim.cpp's, adsb_resamp.cpp's and adsb_bank.cpp's: mixer_of
// reaches into them.
#include <cmath>
#include <numeric>

#include "adsb_ctx.h"

using namespace adsb::host;

namespace {

int mixer_set(adsb_ctx *c, Registry &mem, Mixer &m, const int16_t *cs_pairs, uint32_t period)
{
    if (!cs_pairs && !period) {
        m.period = 0;   // (a call still running has its parameters; the calls behind this one take the plain kernels)
        return ADSB_OK;
    }
    if (!cs_pairs || period < 1 || period > kMixMaxPeriod) return ADSB_ERR_INVALID;
    MixTable t{};
    for (uint32_t i = 0; i < period; i++) {
        const int16_t co = cs_pairs[2 * i], si = cs_pairs[2 * i + 1];
        if (co == -32768 || si == -32768) return ADSB_ERR_INVALID;   // (-s has to fit an int16)
        t.cs[i] = (uint32_t)(uint16_t)co | (uint32_t)(uint16_t)si << 16;
    }
    ADSB_ON_DEVICE(c);
    if (!m.d_table) {
        const hipError_t e = mem.add(Registry::kDevice, (void **)&m.d_table, kMixMaxPeriod * sizeof(uint2));
        if (e != hipSuccess) return e == hipErrorOutOfMemory ? ADSB_ERR_NOMEM : fail(c, e, "mixer_set");
    }
    // the table travels in the launch's arguments: behind the calls already on the stream, in front of the next one
    if (int e = launch_mix_store(t, period, m.d_table, c->stream)) return fail(c, (hipError_t)e, "launch_mix_store");
    if (c->stream == c->own_stream) c->own_stream_dirty = true;
    m.period = period;
    return ADSB_OK;
}

}  // namespace

extern "C" {

int adsb_mix_set_decim(adsb_decim *d, const int16_t *cs_pairs, uint32_t period)
try {
    if (!d) return ADSB_ERR_INVALID;
    const MixerOwner o = mixer_of(d);
    return mixer_set(o.ctx, *o.mem, *o.mix, cs_pairs, period);
} ADSB_ABI_CATCH

int adsb_mix_set_resamp(adsb_resamp *r, const int16_t *cs_pairs, uint32_t period)
try {
    if (!r) return ADSB_ERR_INVALID;
    const MixerOwner o = mixer_of(r);
    return mixer_set(o.ctx, *o.mem, *o.mix, cs_pairs, period);
} ADSB_ABI_CATCH

int adsb_bank_set_mixer(adsb_bank *b, const int16_t *cs_pairs, uint32_t period)
try {
    if (!b) return ADSB_ERR_INVALID;
    const MixerOwner o = mixer_of(b);
    return mixer_set(o.ctx, *o.mem, *o.mix, cs_pairs, period);
} ADSB_ABI_CATCH

int adsb_mix_table(uint32_t k, uint32_t period, int16_t *cs_pairs, size_t cap)
try {
    if (period < 1 || period > kMixMaxPeriod || (!cs_pairs && cap)) return ADSB_ERR_INVALID;
    if (cap < period) return ADSB_ERR_CAPACITY;
    const double pi = 3.14159265358979323846;
    const uint32_t N = period;
    k %= N;
    for (uint32_t t = 0; t < N; t++) {
        const uint32_t a = (k * t) % N;   // the angle in N-ths of a turn
        long co, si;
        if ((4 * a) % N == 0) {   // a whole number of quarter turns: exact, whatever libm says
            const int quarter = (int)(4 * a / N);
            co = quarter == 0 ? 16384 : quarter == 2 ? -16384 : 0;
            si = quarter == 1 ? 16384 : quarter == 3 ? -16384 : 0;
        } else {
            co = std::lround(16384.0 * std::cos(2.0 * pi * (double)a / (double)N));
            si = std::lround(16384.0 * std::sin(2.0 * pi * (double)a / (double)N));
        }
        cs_pairs[2 * t] = (int16_t)co, cs_pairs[2 * t + 1] = (int16_t)si;
    }
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_mix_for_shift(uint32_t up, uint32_t down, int32_t shift_hz, uint32_t *k, uint32_t *period)
{
    if (!k || !period || up < 1 || up > kResampMaxRatio || down < 1 || down > kResampMaxRatio) return ADSB_ERR_INVALID;
    // k / N = shift_hz up / (2 400 000 down), reduced: |numerator| < 2^38, the denominator < 2^29
    const int64_t num = (int64_t)shift_hz * (int64_t)up, den = 2400000ll * (int64_t)down;
    const int64_t g = std::gcd(num < 0 ? -num : num, den);   // (gcd(0, den) = den: no shift is 0 / 1)
    const int64_t n = den / g;
    *period = (uint32_t)n;
    *k = (uint32_t)(((num / g) % n + n) % n);
    return n <= (int64_t)kMixMaxPeriod ? ADSB_OK : ADSB_ERR_INVALID;
}

}  // extern "C"
