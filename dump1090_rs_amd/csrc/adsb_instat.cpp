// adsb_instat.cpp -- the host side of the input statistics a decimator, a resampler or a bank may count (include/adsb_hip.h,
// "Input statistics"): the mode and its reservation, the launch a handle's run path makes in front of its filter's, the
// fetch, and the two host-only helpers, adsb_input_bin and adsb_input_summary.  The kernels are adsb_instat.hip's.  The
// handles are adsb_decim.cpp's, adsb_resamp.cpp's and adsb_bank.cpp's: instat_of reaches into them.
#include <cmath>
#include <cstring>
#include <limits>

#include "adsb_ctx.h"

using namespace adsb::host;

namespace {

int instat_count(adsb_ctx *c, InStat &st, int format, float scale, const void *d_in, uint64_t n_in)
{
    InstatParams p{};
    p.src = d_in;
    p.n_in = n_in;
    p.u8_table = format == ADSB_DECIM_8BIT ? c->d_u8_table : nullptr;
    p.acc = st.d_acc;
    p.n_streams = 1;
    p.format = (uint32_t)format;
    p.scale = scale;
    if (int e = launch_instat(p, c->stream)) return fail(c, (hipError_t)e, "launch_instat");
    if (c->stream == c->own_stream) c->own_stream_dirty = true;
    st.launches++;
    return ADSB_OK;
}

int instat_count_bank(adsb_ctx *c, InStat &st, uint32_t n_streams, int format, float scale, const ResampBankRun *runs,
                      const ResampBankRun *d_runs, uint32_t n_runs)
{
    InstatParams p{};
    p.u8_table = format == ADSB_DECIM_8BIT ? c->d_u8_table : nullptr;
    p.acc = st.d_acc;
    p.n_streams = n_streams;
    p.format = (uint32_t)format;
    p.scale = scale;
    if (int e = launch_instat_bank(p, runs, d_runs, n_runs, c->stream)) return fail(c, (hipError_t)e, "launch_instat_bank");
    if (c->stream == c->own_stream) c->own_stream_dirty = true;
    st.launches++;
    return ADSB_OK;
}

int mode_set(const InStatOwner &o, int enabled)
{
    adsb_ctx *c = o.ctx;
    InStat &st = *o.st;
    if (!enabled) {
        st.on = false;   // (what was accumulated is discarded by the next enable's zeroing)
        return ADSB_OK;
    }
    if (st.on) return ADSB_OK;
    ADSB_ON_DEVICE(c);
    const size_t bytes = (size_t)o.n_streams * sizeof(adsb_input_stats);
    if (!st.d_acc) {
        // all or nothing
        Rollback undo{*o.mem, o.mem->mark(), false};
        hipError_t e = o.mem->add(Registry::kDevice, (void **)&st.d_acc, bytes);
        if (e == hipSuccess) e = o.mem->add(Registry::kPinned, (void **)&st.h_acc, bytes);
        if (e != hipSuccess) return e == hipErrorOutOfMemory ? ADSB_ERR_NOMEM : fail(c, e, "adsb_instat_set");
        undo.keep = true;
    }
    // behind the calls already on the stream, in front of the next one
    HIP_TRY(c, hipMemsetAsync(st.d_acc, 0, bytes, c->stream));
    if (c->stream == c->own_stream) c->own_stream_dirty = true;
    st.count = instat_count, st.count_bank = instat_count_bank;
    st.on = true;
    return ADSB_OK;
}

int mode_fetch(const InStatOwner &o, uint32_t first, uint32_t n, adsb_input_stats *out)
{
    adsb_ctx *c = o.ctx;
    InStat &st = *o.st;
    if (!out || !st.on || first > o.n_streams || n > o.n_streams - first) return ADSB_ERR_INVALID;
    if (n == 0) return ADSB_OK;
    ADSB_ON_DEVICE(c);
    const size_t words = sizeof(adsb_input_stats) / sizeof(unsigned long long), bytes = (size_t)n * sizeof(adsb_input_stats);
    unsigned long long *d = st.d_acc + (size_t)first * words;
    // on the handle's stream: behind every launch that counted, the copy and the zeroing in front of the next one
    HIP_TRY(c, hipMemcpyAsync(st.h_acc + first, d, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemsetAsync(d, 0, bytes, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::memcpy(out, st.h_acc + first, bytes);
    return ADSB_OK;
}

double log10_or_minus_inf(double x) { return x > 0.0 ? std::log10(x) : -std::numeric_limits<double>::infinity(); }

}  // namespace

extern "C" {

int adsb_instat_set_decim(adsb_decim *d, int enabled)
try {
    return d ? mode_set(instat_of(d), enabled) : ADSB_ERR_INVALID;
} ADSB_ABI_CATCH

int adsb_instat_set_resamp(adsb_resamp *r, int enabled)
try {
    return r ? mode_set(instat_of(r), enabled) : ADSB_ERR_INVALID;
} ADSB_ABI_CATCH

int adsb_instat_set_bank(adsb_bank *b, int enabled)
try {
    return b ? mode_set(instat_of(b), enabled) : ADSB_ERR_INVALID;
} ADSB_ABI_CATCH

int adsb_instat_get_decim(const adsb_decim *d) { return d ? (int)instat_of(const_cast<adsb_decim *>(d)).st->on : ADSB_ERR_INVALID; }
int adsb_instat_get_resamp(const adsb_resamp *r) { return r ? (int)instat_of(const_cast<adsb_resamp *>(r)).st->on : ADSB_ERR_INVALID; }
int adsb_instat_get_bank(const adsb_bank *b) { return b ? (int)instat_of(const_cast<adsb_bank *>(b)).st->on : ADSB_ERR_INVALID; }

int adsb_instat_fetch_decim(adsb_decim *d, adsb_input_stats *out)
try {
    return d ? mode_fetch(instat_of(d), 0, 1, out) : ADSB_ERR_INVALID;
} ADSB_ABI_CATCH

int adsb_instat_fetch_resamp(adsb_resamp *r, adsb_input_stats *out)
try {
    return r ? mode_fetch(instat_of(r), 0, 1, out) : ADSB_ERR_INVALID;
} ADSB_ABI_CATCH

int adsb_instat_fetch_bank(adsb_bank *b, uint32_t first_stream, uint32_t n_streams, adsb_input_stats *out)
try {
    return b ? mode_fetch(instat_of(b), first_stream, n_streams, out) : ADSB_ERR_INVALID;
} ADSB_ABI_CATCH

int adsb_input_bin(int16_t v)
{
    uint32_t mag = (uint32_t)(v < 0 ? -(int)v : (int)v);
    int bin = 0;
    for (; mag; mag >>= 1) bin++;
    return bin;
}

int adsb_input_summary(const adsb_input_stats *s, size_t n, adsb_input_summary_t *out)
{
    if (!out || (!s && n)) return ADSB_ERR_INVALID;
    *out = adsb_input_summary_t{};
    // (the records' own sums wrap at 64 bits; a display's do not have to: doubles from here on)
    double re = 0, im = 0, re2 = 0, im2 = 0, clipped = 0, nan = 0, samples = 0;
    uint32_t peak = 0, bits = 0;
    for (size_t i = 0; i < n; i++) {
        out->n_samples += s[i].n_samples;
        samples += (double)s[i].n_samples;
        re += (double)s[i].sum_re, im += (double)s[i].sum_im;
        re2 += (double)s[i].sum_re2, im2 += (double)s[i].sum_im2;
        clipped += (double)s[i].n_clipped, nan += (double)s[i].n_nan;
        peak = std::max(peak, s[i].peak);
        for (uint32_t b = 0; b < ADSB_INPUT_BINS; b++)
            if (s[i].hist[b]) bits = std::max(bits, b);
    }
    out->n_records = n;
    const bool any = samples > 0;
    out->mean_power_dbfs = any ? 10.0 * log10_or_minus_inf((re2 + im2) / samples / (32768.0 * 32768.0))
                               : -std::numeric_limits<double>::infinity();
    out->peak_dbfs = 20.0 * log10_or_minus_inf((double)peak / 32768.0);
    out->dc_re = any ? re / samples : 0.0;
    out->dc_im = any ? im / samples : 0.0;
    out->clipped_fraction = any ? clipped / samples : 0.0;
    out->nan_fraction = any ? nan / samples : 0.0;
    // sum re^2 / sum im^2: no im power at all is +inf (REAL16), none of either -inf like every logarithm of zero here
    out->iq_gain_db = im2 > 0 ? 10.0 * log10_or_minus_inf(re2 / im2)
                              : re2 > 0 ? std::numeric_limits<double>::infinity() : -std::numeric_limits<double>::infinity();
    out->bits_used = bits;
    return ADSB_OK;
}

int adsb_instat_selftest_geometry(int format, uint32_t *tile_samples, uint32_t *max_groups_per_run)
{
    if (!format_ok(format) || !tile_samples || !max_groups_per_run) return ADSB_ERR_INVALID;
    *tile_samples = adsb::instat_tile_samples((uint32_t)format);
    *max_groups_per_run = adsb::kInstatMaxGroups;
    return ADSB_OK;
}

uint64_t adsb_instat_selftest_launches_decim(const adsb_decim *d) { return d ? instat_of(const_cast<adsb_decim *>(d)).st->launches : 0; }
uint64_t adsb_instat_selftest_launches_resamp(const adsb_resamp *r) { return r ? instat_of(const_cast<adsb_resamp *>(r)).st->launches : 0; }
uint64_t adsb_instat_selftest_launches_bank(const adsb_bank *b) { return b ? instat_of(const_cast<adsb_bank *>(b)).st->launches : 0; }

}  // extern "C"
